// Packed payload copy-out of packed frames (rudp_gather_payloads): the
// receiver's `buffer + payload` (utils/reliableUDP.py:121, :135-136) for a
// batch -- the payloads of the frames the caller keeps, back to back, with
// their offsets -- and the inverse of the packed varlen encode.
//
// Per frame i: plen[i] = max(frame_len_i - H, 0) when its pair of offsets
// passes the decode's rule (frame_off[i] <= frame_off[i + 1] <= frames_bytes)
// and keep[i] != 0, else 0; payload_off = exclusive scan of plen.
//
// Reduce-then-scan in three launches, as scan.hip:
//   1. sums of plen over tiles of R frames (the offset rule's bit in bit 63);
//   2. one workgroup turns them into exclusive tile bases in place, writes
//      payload_off[n] and the status word (capacity check included);
//   3. one workgroup per tile rescans its frames from its base, writes its
//      payload_off[] coalesced and, unless the status has RUDP_ST_PAYLOAD_CAP,
//      copies its output run [base, base + tile total).
//
// The edge rule.  Output runs of neighbouring tiles meet at arbitrary byte
// positions.  A tile deals its run as the 16-B chunks of the output's own
// alignment; a chunk that lies whole inside the run goes out as one 16-B
// store, the partial chunk at either end of the run bytewise.  No store of a
// tile covers a byte outside its run, so none covers a byte outside
// [0, total) of the output.
//
// Each chunk finds the frame of its first byte by a binary search over the
// tile's payload offsets in LDS and gathers the one or more payloads it
// covers, one byte-shifted 16-B window per payload.  Where the windows come
// from is the one choice, made from the typical frame length:
//   small frames (payload hint under 16 B; a chunk covers up to 16 payloads):
//     tiles of 1024 frames, four per thread, whose frame run is staged in LDS
//     with guarded 16-B loads from the aligned-down start of the first kept
//     frame; a window is five LDS dwords.  A tile whose run exceeds the LDS
//     budget (a long frame among small ones, a long dropped stretch between
//     kept frames, offsets out of order) reads HBM as the larger frames do;
//   larger frames (a chunk covers one payload, two at a boundary): tiles of
//     up to 96 KiB of frames, no staging: a window is two aligned 16-B loads
//     of HBM and a funnel shift.  Neighbouring lanes read neighbouring blocks,
//     so every block is read by two lanes of a wave and the loads are cached
//     ones; without an LDS image eight tiles share a CU.  (Staged through LDS
//     in 16-frame tiles, 1M x 1479-B frames with half of them dropped took
//     0.56 ms against 0.36 this way, lengths uniform in [0, 2944] 0.81 against
//     0.65-0.70; with every equal-length frame kept both forms land in one
//     band, 0.62-0.77 from process to process:
//     profiles/r07/gather_forms.json, gather_payloads.json.)
// Only bytes inside [0, frames_bytes) of the caller's buffer are needed; a
// rejected or dropped frame is never fetched for its own sake (the small-frame
// image spans from the first to the last kept frame of its tile).
//
// The chunk copy (gather_chunks) and gather_plen are in gather_device.hpp,
// which ordered.hip shares (its tiles are runs of ranks, not of frames); this
// file has the kernels and the launcher.
#include "gather_device.hpp"
#include "scan_device.hpp"

namespace RUDP_NS {

constexpr uint32_t kGatherSmallFpt = 4;           // small frames: frames per thread (tiles of 1024)
constexpr uint32_t kGatherTileBytes = 98304;      // larger frames: hinted frame bytes per tile

// ITEMS 1: a block of 256 frames holds 256 / R tiles (R a power of two), cut
// out of the block's scan.  ITEMS 4: the block is one tile of 1024 frames.
template <uint32_t ITEMS>
__global__ void __launch_bounds__(kBlock) gather_block_sums_kernel(GatherArgs a, uint64_t* sums, uint64_t nt) {
  __shared__ uint64_t s_wave[kBlock / 64];
  __shared__ uint64_t s_ex[kBlock + 1];
  __shared__ uint32_t s_bad;
  if (threadIdx.x == 0) s_bad = 0;
  const uint64_t base = (uint64_t)blockIdx.x * (kBlock * ITEMS);
  uint64_t acc = 0;
  uint32_t bad = 0;
#pragma unroll
  for (uint32_t j = 0; j < ITEMS; ++j) {
    const uint64_t i = base + j * kBlock + threadIdx.x;
    if (i < a.n) {
      const bool kept = !a.keep || a.keep[i] != 0;
      acc += gather_plen(a.frame_off[i], a.frame_off[i + 1], a.frames_bytes, a.H, kept, &bad);
    }
  }
  __syncthreads();  // s_bad initialised
  if (bad) atomicOr(&s_bad, 1u);
  if (ITEMS == 1) {
    uint64_t total = 0;
    const uint64_t ex = block_exclusive_scan(acc, &total, s_wave);  // (its barriers order s_bad)
    s_ex[threadIdx.x] = ex;
    if (threadIdx.x == 0) s_ex[kBlock] = total;
    __syncthreads();
    const uint32_t tiles = kBlock / a.R;
    const uint64_t t = (uint64_t)blockIdx.x * tiles + threadIdx.x;
    if (threadIdx.x < tiles && t < nt)
      sums[t] = (s_ex[(threadIdx.x + 1u) * a.R] - s_ex[threadIdx.x * a.R]) | ((uint64_t)s_bad << kGatherBadShift);
  } else {
    acc = wave_sum64(acc);
    if ((threadIdx.x & 63u) == 0) s_wave[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint64_t t = 0;
      for (uint32_t w = 0; w < kBlock / 64; ++w) t += s_wave[w];
      sums[blockIdx.x] = t | ((uint64_t)s_bad << kGatherBadShift);
    }
  }
}

// One workgroup of 1024 threads: sums[t] <- sum_{u<t} sums[u]; payload_off[n]
// <- total; the call's status word.
__global__ void __launch_bounds__(1024) gather_block_bases_kernel(uint64_t* sums, uint64_t nt, GatherArgs a) {
  __shared__ uint64_t s_wave[1024 / 64];
  __shared__ uint32_t s_bad;
  if (threadIdx.x == 0) s_bad = 0;
  const uint64_t per = (nt + 1023) / 1024;
  const uint64_t lo = threadIdx.x * per < nt ? threadIdx.x * per : nt, hi = lo + per < nt ? lo + per : nt;
  // (eight loads in flight per thread.  The kernel still takes 33 us for the
  // 16384 tiles of 1M MTU frames, with one load at a time as with eight: a
  // thread's sums are contiguous, so a wave's load touches 64 lines)
  uint64_t mine = 0;
  uint32_t bad = 0;
  for (uint64_t i = lo; i < hi; i += 8) {
    uint64_t v[8];
#pragma unroll
    for (uint32_t u = 0; u < 8; ++u) v[u] = i + u < hi ? sums[i + u] : 0ull;
#pragma unroll
    for (uint32_t u = 0; u < 8; ++u) {
      mine += v[u] & kGatherSumMask;
      if (mine > kGatherSat) mine = kGatherSat;
      bad |= (uint32_t)(v[u] >> kGatherBadShift);
    }
  }
  __syncthreads();  // s_bad initialised
  if (bad) atomicOr(&s_bad, 1u);
  uint64_t total = 0;
  uint64_t run = block_exclusive_scan(mine, &total, s_wave);
  for (uint64_t i = lo; i < hi; i += 8) {
    uint64_t v[8];
#pragma unroll
    for (uint32_t u = 0; u < 8; ++u) v[u] = i + u < hi ? sums[i + u] & kGatherSumMask : 0ull;
#pragma unroll
    for (uint32_t u = 0; u < 8; ++u) {
      if (i + u < hi) sums[i + u] = run;
      run += v[u];
    }
  }
  if (threadIdx.x == 0) {
    a.payload_off[a.n] = total;
    uint32_t st = s_bad ? RUDP_ST_OFFSETS : 0u;
    if (total >= kGatherSat || total > a.payload_cap) st |= RUDP_ST_PAYLOAD_CAP;
    *a.status = st;
  }
}

// One tile of a.R frames (FPT consecutive frames per thread).  Dynamic LDS:
// frame offsets u64 [R + 1] | payload offsets in the tile u64 [R + 1] | and,
// for the small-frame tiles (FPT > 1), guard, the staged frame run, guard.
template <uint32_t FPT>
__global__ void __launch_bounds__(kBlock) gather_tile_kernel(GatherArgs a, const uint64_t* bases, uint64_t nt) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ uint64_t s_wave[kBlock / 64];
  __shared__ unsigned long long s_lo, s_hi;
  constexpr bool kStage = FPT > 1;
  uint64_t* s_fo = reinterpret_cast<uint64_t*>(lds);
  uint64_t* s_po = s_fo + (a.R + 1u);
  unsigned char* img = reinterpret_cast<unsigned char*>(s_po + (a.R + 1u));  // (16 (R + 1) bytes in: 16-B aligned)
  const uint32_t tid = threadIdx.x;
  const uint64_t tile = a.xcd ? xcd_tile(blockIdx.x, (uint32_t)nt) : blockIdx.x;
  const uint64_t p0 = tile * a.R;
  const uint32_t Rv = a.n - p0 < a.R ? (uint32_t)(a.n - p0) : a.R;
  for (uint32_t k = tid; k <= Rv; k += kBlock) s_fo[k] = a.frame_off[p0 + k];
  // everything else the tile reads before its frames, in the same round trip
  bool kept[FPT];
#pragma unroll
  for (uint32_t j = 0; j < FPT; ++j) {
    const uint32_t k = tid * FPT + j;
    kept[j] = k < Rv && (!a.keep || a.keep[p0 + k] != 0);
  }
  const uint64_t base = bases[tile];
  const uint32_t call_status = *a.status;
  if (tid == 0) {
    s_lo = ~0ull;
    s_hi = 0ull;
  }
  __syncthreads();
  // plen of this thread's frames, and the byte range [f_lo, f_hi) of those with a payload
  uint64_t pl[FPT];
  uint64_t mine = 0, f_lo = ~0ull, f_hi = 0;
  uint32_t bad = 0;
#pragma unroll
  for (uint32_t j = 0; j < FPT; ++j) {
    const uint32_t k = tid * FPT + j;
    pl[j] = 0;
    if (k < Rv) {
      const uint64_t fo0 = s_fo[k], fo1 = s_fo[k + 1u];
      pl[j] = gather_plen(fo0, fo1, a.frames_bytes, a.H, kept[j], &bad);
      if (pl[j]) {
        f_lo = fo0 < f_lo ? fo0 : f_lo;
        f_hi = fo1 > f_hi ? fo1 : f_hi;
      }
    }
    mine += pl[j];
  }
  uint64_t total = 0;
  uint64_t run = block_exclusive_scan(mine, &total, s_wave);
#pragma unroll
  for (uint32_t j = 0; j < FPT; ++j) {
    const uint32_t k = tid * FPT + j;
    if (k < Rv) s_po[k] = run;
    run += pl[j];
  }
  if (tid == 0) s_po[Rv] = total;
  if (kStage) {
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint64_t l2 = __shfl_xor(f_lo, d, 64), h2 = __shfl_xor(f_hi, d, 64);
      f_lo = l2 < f_lo ? l2 : f_lo;
      f_hi = h2 > f_hi ? h2 : f_hi;
    }
    if ((tid & 63u) == 0 && f_hi) {
      atomicMin(&s_lo, (unsigned long long)f_lo);
      atomicMax(&s_hi, (unsigned long long)f_hi);
    }
  }
  __syncthreads();
  for (uint32_t k = tid; k < Rv; k += kBlock) a.payload_off[p0 + k] = base + s_po[k];
  if ((call_status & RUDP_ST_PAYLOAD_CAP) || total == 0) return;  // (uniform)

  unsigned char* o = a.out + base;
  if (kStage) {
    // the frame run of the tile's payloads, in bytes of the aligned buffer from gA
    const uint64_t gA = (s_lo + a.fmis) & ~15ull, gE = s_hi + a.fmis;
    if (gE - gA <= a.cap) {
      const uint32_t nvec = (uint32_t)((gE - gA + 15u) >> 4);
      u32x4* dst = reinterpret_cast<u32x4*>(img + kGatherGuard);
      for (uint32_t v0 = tid; v0 < nvec; v0 += 4u * kBlock) {
        u32x4 r[4];
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u)
          if (v0 + u * kBlock < nvec) r[u] = load16_guarded(a.frames, gA + 16ull * (v0 + u * kBlock), gE);
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u)
          if (v0 + u * kBlock < nvec) dst[v0 + u * kBlock] = r[u];
      }
      __syncthreads();
      gather_chunks<true>(a, s_fo, s_po, Rv, total, o, reinterpret_cast<const uint32_t*>(img), gA);
      return;
    }
  }
  gather_chunks<false>(a, s_fo, s_po, Rv, total, o, nullptr, 0);
}

int launch_gather_payloads(GatherArgs a, uint32_t len_hint, hipStream_t stream) {
  // Small frames (payload hint under 16 B, the reference's one-character
  // datagrams): four frames per thread, tiles of 1024 staged in LDS.  Above:
  // the most frames, a power of two up to 256, whose hinted run stays within
  // 96 KiB, read straight from HBM.
  const bool small = len_hint < 16u + a.H;
  size_t lds;
  if (small) {
    a.R = kBlock * kGatherSmallFpt;
    a.cap = (a.R * (16u + a.H) + 15u) & ~15u;
    lds = 16u * ((size_t)a.R + 1u) + 2u * kGatherGuard + a.cap + 16u;
  } else {
    a.R = kBlock;
    while (a.R > 1u && (uint64_t)a.R * len_hint > kGatherTileBytes) a.R >>= 1;
    a.cap = 0;
    lds = 16u * ((size_t)a.R + 1u);
  }
  a.xcd = tuning().tile_xcd ? 1u : 0u;
  const uint64_t nt = (a.n + a.R - 1u) / a.R;
  if (nt > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
  uint64_t* sums = nullptr;
  hipError_t e = stream_scratch(reinterpret_cast<void**>(&sums), nt * sizeof(uint64_t), stream, kScratchSums);
  if (e != hipSuccess) return (int)e;
  if (small) {
    hipLaunchKernelGGL(gather_block_sums_kernel<kGatherSmallFpt>, dim3((uint32_t)nt), dim3(kBlock), 0, stream, a,
                       sums, nt);
  } else {
    const uint64_t nb = (a.n + kBlock - 1u) / kBlock;
    hipLaunchKernelGGL(gather_block_sums_kernel<1>, dim3((uint32_t)nb), dim3(kBlock), 0, stream, a, sums, nt);
  }
  hipLaunchKernelGGL(gather_block_bases_kernel, dim3(1), dim3(1024), 0, stream, sums, nt, a);
  if (small)
    hipLaunchKernelGGL(gather_tile_kernel<kGatherSmallFpt>, dim3((uint32_t)nt), dim3(kBlock), lds, stream, a, sums,
                       nt);
  else
    hipLaunchKernelGGL(gather_tile_kernel<1>, dim3((uint32_t)nt), dim3(kBlock), lds, stream, a, sums, nt);
  return (int)hipGetLastError();
}

}  // namespace rudp
