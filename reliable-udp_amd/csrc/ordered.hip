// rudp_gather_ordered: rudp_gather_payloads with a permutation -- frame i with
// rank r < K puts its bytes from `skip` on at position r of the output, K read
// on the device (rudp_accept_window's d_info[1] or [5]).  The message of a
// reordering receiver in delivery order, and (skip 0) its pending frames whole
// for the next call.
//
// Five launches, the copy gather.hip's:
//   1. src[k] = none for k < K, the status word zeroed;
//   2. every frame with a rank below K writes its index to src[rank]; a rank
//      at or above K that is not RUDP_RANK_NONE sets RUDP_ST_RANK;
//   3. sums of the lengths in rank order over tiles of 256 ranks (the offset
//      rule's bit in bit 63), as gather.hip's first launch;
//   4. one workgroup: exclusive tile bases, out_off[K], the status;
//   5. one workgroup per tile: out_off[] and the copy of its run, each output
//      chunk gathering the payloads it covers from HBM (gather_chunks).
// The grids are sized by n, the bound of K; tiles and threads past K leave.
// Ranks that repeat below K leave src[] with one of the frames: every index
// it holds is below n, so every read and write stays in bounds.
#include "gather_device.hpp"
#include "scan_device.hpp"

namespace RUDP_NS {

constexpr uint32_t kOrdTile = kBlock;  // ranks per tile, one per thread

__device__ __forceinline__ uint64_t ordered_count(const OrderedArgs& a) {
  const uint64_t K = *a.count;
  return K < a.n ? K : a.n;
}

// Bytes of the frame with rank k; *fo its first byte (0 when it has none).
__device__ __forceinline__ uint64_t ordered_plen(const OrderedArgs& a, uint64_t k, uint64_t* fo, uint32_t* bad) {
  const uint32_t i = a.src[k];
  *fo = 0;
  if (i >= a.n) return 0;  // (no frame has this rank)
  const uint64_t fo0 = a.frame_off[i], fo1 = a.frame_off[i + 1u];
  const uint64_t len = gather_plen(fo0, fo1, a.frames_bytes, a.skip, true, bad);
  if (len) *fo = fo0;
  return len;
}

__global__ void __launch_bounds__(kBlock) ordered_init_kernel(OrderedArgs a) {
  const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k == 0) *a.status = 0;
  if (k < ordered_count(a)) a.src[k] = RUDP_RANK_NONE;
}

__global__ void __launch_bounds__(kBlock) ordered_scatter_kernel(OrderedArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n) return;
  const uint32_t r = a.rank[i];
  if (r == RUDP_RANK_NONE) return;
  if (r < ordered_count(a)) a.src[r] = (uint32_t)i;
  else atomicOr(a.status, RUDP_ST_RANK);
}

__global__ void __launch_bounds__(kBlock) ordered_sums_kernel(OrderedArgs a, uint64_t* sums) {
  __shared__ uint64_t s_wave[kBlock / 64];
  __shared__ uint32_t s_bad;
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  const uint64_t k = (uint64_t)blockIdx.x * kOrdTile + threadIdx.x;
  uint64_t len = 0, fo;
  uint32_t bad = 0;
  if (k < ordered_count(a)) len = ordered_plen(a, k, &fo, &bad);
  if (bad) atomicOr(&s_bad, 1u);
  len = wave_sum64(len);
  if ((threadIdx.x & 63u) == 0) s_wave[threadIdx.x >> 6] = len;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t t = 0;
    for (uint32_t w = 0; w < kBlock / 64; ++w) t += s_wave[w];
    sums[blockIdx.x] = t | ((uint64_t)s_bad << kGatherBadShift);
  }
}

// One workgroup of 1024 threads, as gather_block_bases_kernel: sums[t] <- the
// sum of the tiles before t; out_off[K] <- the total; the status bits or'ed in.
__global__ void __launch_bounds__(1024) ordered_bases_kernel(OrderedArgs a, uint64_t* sums, uint64_t nt) {
  __shared__ uint64_t s_wave[1024 / 64];
  __shared__ uint32_t s_bad;
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  const uint64_t per = (nt + 1023) / 1024;
  const uint64_t lo = threadIdx.x * per < nt ? threadIdx.x * per : nt, hi = lo + per < nt ? lo + per : nt;
  uint64_t mine = 0;
  uint32_t bad = 0;
  for (uint64_t i = lo; i < hi; ++i) {
    const uint64_t v = sums[i];
    mine += v & kGatherSumMask;
    if (mine > kGatherSat) mine = kGatherSat;
    bad |= (uint32_t)(v >> kGatherBadShift);
  }
  if (bad) atomicOr(&s_bad, 1u);
  uint64_t total = 0;
  uint64_t run = block_exclusive_scan(mine, &total, s_wave);  // (its barriers order s_bad)
  for (uint64_t i = lo; i < hi; ++i) {
    const uint64_t v = sums[i] & kGatherSumMask;
    sums[i] = run;
    run += v;
  }
  if (threadIdx.x == 0) {
    a.out_off[ordered_count(a)] = total;
    uint32_t st = s_bad ? RUDP_ST_OFFSETS : 0u;
    if (total >= kGatherSat || total > a.out_cap) st |= RUDP_ST_PAYLOAD_CAP;
    if (st) atomicOr(a.status, st);
  }
}

__global__ void __launch_bounds__(kBlock) ordered_tile_kernel(OrderedArgs a, const uint64_t* bases) {
  __shared__ uint64_t s_fo[kOrdTile + 1], s_po[kOrdTile + 1];
  __shared__ uint64_t s_wave[kBlock / 64];
  const uint64_t K = ordered_count(a);
  const uint64_t k0 = (uint64_t)blockIdx.x * kOrdTile;
  if (k0 >= K) return;  // (uniform)
  const uint32_t Rv = K - k0 < kOrdTile ? (uint32_t)(K - k0) : kOrdTile;
  const uint32_t tid = threadIdx.x;
  const uint64_t base = bases[blockIdx.x];
  const uint32_t call_status = *a.status;
  uint64_t len = 0, fo = 0;
  uint32_t bad = 0;
  if (tid < Rv) len = ordered_plen(a, k0 + tid, &fo, &bad);
  uint64_t total = 0;
  const uint64_t run = block_exclusive_scan(len, &total, s_wave);
  if (tid < Rv) {
    s_fo[tid] = fo;
    s_po[tid] = run;
    a.out_off[k0 + tid] = base + run;
  }
  if (tid == 0) s_po[Rv] = total;
  __syncthreads();
  if ((call_status & RUDP_ST_PAYLOAD_CAP) || total == 0) return;  // (uniform)
  GatherArgs g{};
  g.frames = a.frames;
  g.fmis = a.fmis;
  g.frames_bytes = a.frames_bytes;
  g.H = a.skip;
  gather_chunks<false>(g, s_fo, s_po, Rv, total, a.out + base, nullptr, 0);
}

int launch_gather_ordered(OrderedArgs a, hipStream_t stream) {
  const uint64_t nt = (a.n + kOrdTile - 1u) / kOrdTile;
  const uint64_t nb = (a.n + kBlock - 1u) / kBlock;
  if (nt > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
  uint64_t* sums = nullptr;
  hipError_t e = stream_scratch(reinterpret_cast<void**>(&sums), nt * sizeof(uint64_t), stream, kScratchSums);
  if (e != hipSuccess) return (int)e;
  if (!a.src) {
    e = stream_scratch(reinterpret_cast<void**>(&a.src), a.n * sizeof(uint32_t), stream, kScratchRecords);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(ordered_init_kernel, dim3((uint32_t)nb), dim3(kBlock), 0, stream, a);
  hipLaunchKernelGGL(ordered_scatter_kernel, dim3((uint32_t)nb), dim3(kBlock), 0, stream, a);
  hipLaunchKernelGGL(ordered_sums_kernel, dim3((uint32_t)nt), dim3(kBlock), 0, stream, a, sums);
  hipLaunchKernelGGL(ordered_bases_kernel, dim3(1), dim3(1024), 0, stream, a, sums, nt);
  hipLaunchKernelGGL(ordered_tile_kernel, dim3((uint32_t)nt), dim3(kBlock), 0, stream, a, sums);
  return (int)hipGetLastError();
}

}  // namespace rudp
