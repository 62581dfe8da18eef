// The sender's judgement of a reply batch on the device: rudp_ack_progress
// (wait_ack of utils/reliableUDP.py:64-85 over decoded tables) and
// rudp_acknowledge (reply datagrams to new sender state and the closing
// send_ack packet, :87-93, in one call).
//
// The rule, per reply i in arrival order, in characters from the ISN (d_i =
// ack_i - isn; state: p characters acknowledged, L characters of the
// outstanding frame, last, done; T characters in all, C per datagram):
//   valid_i   usable_i && d_i == p + L as integers (EXACT), or usable_i &&
//             p + L <= d_i <= sent && (d_i % C == 0 || d_i == T) (CUMULATIVE);
//   !valid_i  nothing changes;
//   ACK       p = d_i;
//   FIN       end = i, done = 1, stop (L and last stay);
//   else      last ? L = 0 : (L = min(C, T - p), last = (p + L == T)).
//
// The parallel form.  A state is canonical when p <= T lies on the grid (p % C
// == 0 or p == T), L == min(C, T - p) and last == (p + L == T); a fresh
// transfer, a timeout's recomputation and every valid ACK reply out of a
// canonical state leave a canonical one.  While the state stays canonical p
// never decreases, so p before reply i is guessed as the prefix maximum of d_j
// over the candidates j < i (usable, ACK flag, on the grid, d_j <= T, or <=
// sent in CUMULATIVE mode), seeded with the p of d_state_in.  The guess differs
// from the rule only from the first anomaly on: a candidate ahead of the
// guessed p + L (EXACT: the rule rejects it, the maximum absorbs it), or a valid
// reply without the ACK flag (it may drop L to 0 with p < T, which is not
// canonical).  A seed that is not canonical is an anomaly at 0.  Before the
// first anomaly the guess is the rule's state: both satisfy the same recurrence
// from the same seed.
//
// Reduce-then-scan over tiles of 1024 replies, as accept.hip:
//   1. the maximum of every tile's candidates;  2. one workgroup: exclusive
//   tile bases, seeded from d_state_in;  3. one workgroup per tile rescans it,
//   writes valid and pointer under the guess and takes two minima: the first
//   valid FIN and the first anomaly;  4. one workgroup finishes: without an
//   anomaly before the FIN the state follows from pointer[] at the last judged
//   reply; else one lane walks the rule from the anomaly with the exact state
//   before it, the replies staged through LDS in blocks of 1024, overwriting
//   valid and pointer up to the end it finds.  It writes d_state_out and d_info;
//   5. zeroes past the end and the count of valid replies.
// A batch of one tile runs the five steps in one launch, and the fused form of
// rudp_acknowledge runs them on a tile it decoded into LDS itself, out of the
// frame image of frame_image_device.hpp.
#include "frame_image_device.hpp"
#include "scan_device.hpp"

namespace RUDP_NS {

constexpr uint32_t kAckFpt = 4;                   // consecutive replies per thread
constexpr uint32_t kAckTile = kBlock * kAckFpt;   // 1024
constexpr uint32_t kAckHdr = 8;                   // scratch words before the tile maxima
// scratch: [0] p, [1] L, [2] last, [3] done of d_state_in; [4] first valid FIN
// under the guess, [5] first anomaly (n: none); [kAckHdr + t] tile t's maximum.

// The fused form's limits, rudp_receive's (receive.hip): the frame image, the
// tile and the offsets stay within the 64 KiB of LDS a workgroup gets without
// asking, and a frame is decoded by one lane.
constexpr uint32_t kAckFusedBytes = 32768;
constexpr uint32_t kAckFusedMeanFrame = 261;

struct AckSeed {
  uint64_t p, L, last, done;
};

struct AckLds {
  uint64_t ptr[kAckTile];           // p after each reply
  uint32_t pk[kAckTile];            // the walk: ack | flags << 16 | usable << 24
  uint16_t ack[kAckTile];
  uint8_t fl[kAckTile];
  uint8_t us[kAckTile];
  uint8_t val[kAckTile];
  uint64_t wv[kBlock / 64];
  unsigned long long e_min, a_min;  // first valid FIN, first anomaly (n: none)
  uint64_t end, p_out;              // finish: the call's end and p after it
  uint32_t cnt;                     // walk: replies of the block that were judged; final: valid replies
};

__device__ __forceinline__ uint64_t ack_min64(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t ack_max64(uint64_t a, uint64_t b) { return a > b ? a : b; }

__device__ __forceinline__ bool ack_canonical(const AckArgs& a, AckSeed s) {
  if (s.p > a.T || (s.p % a.C != 0 && s.p != a.T)) return false;
  const uint64_t L = ack_min64(a.C, a.T - s.p);
  return s.L == L && s.last == (uint64_t)(s.p + L == a.T);
}
// L and last of the canonical state at p (p <= T).
__device__ __forceinline__ void ack_canon(const AckArgs& a, uint64_t p, uint64_t* L, uint64_t* last) {
  *L = ack_min64(a.C, a.T - p);
  *last = p + *L == a.T;
}

// A candidate's characters, 0 for a reply that is none (0 never raises a maximum).
__device__ __forceinline__ uint64_t ack_cand(const AckArgs& a, uint32_t us, uint32_t fl, uint32_t ack) {
  if (!us || !(fl & 0x40u) || ack < a.isn) return 0;
  const uint64_t d = ack - a.isn;
  if (d > (a.mode == RUDP_ACK_CUMULATIVE ? a.sent : a.T)) return 0;
  return (d % a.C == 0 || d == a.T) ? d : 0;
}

// valid_i for the state (p, L): sums are never formed, so no state overflows.
__device__ __forceinline__ bool ack_valid(const AckArgs& a, uint32_t us, uint32_t ack, uint64_t p, uint64_t L) {
  if (!us || ack < a.isn) return false;
  const uint64_t d = ack - a.isn;
  if (d < p) return false;
  if (a.mode == RUDP_ACK_EXACT) return d - p == L;
  return d - p >= L && d <= a.sent && (d % a.C == 0 || d == a.T);
}

// Replies [p0, p0 + Rv) into LDS, coalesced.
__device__ __forceinline__ void ack_load(const AckArgs& a, AckLds& L, uint64_t p0, uint32_t Rv) {
  for (uint32_t k = threadIdx.x; k < Rv; k += kBlock) {
    L.ack[k] = a.ack[p0 + k];
    L.fl[k] = a.flags[p0 + k];
    L.us[k] = a.usable ? (uint8_t)(a.usable[p0 + k] != 0) : (uint8_t)1;
  }
}

// The maximum of the tile's candidates (all threads get it).
__device__ inline uint64_t ack_tile_max(const AckArgs& a, AckLds& L, uint32_t Rv) {
  uint64_t agg = 0;
#pragma unroll
  for (uint32_t j = 0; j < kAckFpt; ++j) {
    const uint32_t k = threadIdx.x * kAckFpt + j;
    if (k < Rv) agg = ack_max64(agg, ack_cand(a, L.us[k], L.fl[k], L.ack[k]));
  }
  uint64_t total;
  block_exclusive_max(agg, L.wv, &total);
  return total;
}

// The tile in LDS judged under the guess from `base`, the p before reply p0:
// valid and pointer into LDS, the minima into L.e_min / L.a_min.
__device__ inline void ack_scan(const AckArgs& a, AckLds& L, uint64_t p0, uint32_t Rv, uint64_t base) {
  const uint32_t tid = threadIdx.x;
  uint64_t cand[kAckFpt];
  uint64_t agg = 0;
#pragma unroll
  for (uint32_t j = 0; j < kAckFpt; ++j) {
    const uint32_t k = tid * kAckFpt + j;
    cand[j] = k < Rv ? ack_cand(a, L.us[k], L.fl[k], L.ack[k]) : 0ull;
    agg = ack_max64(agg, cand[j]);
  }
  uint64_t s = ack_max64(base, block_exclusive_max(agg, L.wv));
  unsigned long long e_min = a.n, a_min = a.n;
#pragma unroll
  for (uint32_t j = 0; j < kAckFpt; ++j) {
    const uint32_t k = tid * kAckFpt + j;
    if (k >= Rv) break;
    const uint64_t g = p0 + k;
    const uint32_t fl = L.fl[k], ack = L.ack[k];
    const uint64_t Lc = s <= a.T ? ack_min64(a.C, a.T - s) : 0ull;  // (s > T: a seed that is no canonical state)
    const bool valid = ack_valid(a, L.us[k], ack, s, Lc);
    if (valid && !(fl & 0x40u) && g < a_min) a_min = g;
    if (a.mode == RUDP_ACK_EXACT && cand[j] > s && cand[j] - s > Lc && g < a_min) a_min = g;
    if (valid && (fl & 0x20u) && g < e_min) e_min = g;
    L.val[k] = (uint8_t)valid;
    L.ptr[k] = valid && (fl & 0x40u) ? (uint64_t)(ack - a.isn) : s;
    s = ack_max64(s, cand[j]);
  }
  if (e_min < a.n) atomicMin(&L.e_min, e_min);
  if (a_min < a.n) atomicMin(&L.a_min, a_min);
}

__device__ __forceinline__ void ack_write_info(const AckArgs& a, uint64_t end, uint64_t p0, uint64_t p, uint64_t A,
                                               uint64_t done) {
  a.info[0] = end;
  a.info[2] = p - p0;  // (mod 2^64 when a walk from a state that is not canonical went back)
  a.info[3] = p;
  a.info[4] = A;
  a.info[5] = p / a.C + (p % a.C != 0);
  a.info[6] = done;
  a.info[7] = 0;
}

// Step 4 for one workgroup.  E, A: the first valid FIN under the guess and the
// first anomaly (n: none).  one_tile: the batch is the tile in LDS (its inputs
// and the guess's valid and pointer; the walk's results go there too), else the
// guess's pointer[] is in global memory and the walk writes valid and pointer
// there.  Leaves the end and p after it in L.end / L.p_out.
__device__ inline void ack_finish(const AckArgs& a, AckLds& L, AckSeed seed, uint64_t E, uint64_t A, bool one_tile) {
  const uint32_t tid = threadIdx.x;
  const bool canon = ack_canonical(a, seed);
  if (!canon) A = 0;
  const bool slow = A < E || !canon;
  uint64_t p, Lx, last, done = 0, end = E;
  if (slow) {  // the exact state before reply A
    p = A ? (one_tile ? L.ptr[A - 1u] : a.pointer[A - 1u]) : seed.p;
    if (A) ack_canon(a, p, &Lx, &last);
    else Lx = seed.L, last = seed.last;
  } else if (E < a.n) {  // the FIN leaves L and last as they were before it
    const uint64_t pb = E ? (one_tile ? L.ptr[E - 1u] : a.pointer[E - 1u]) : seed.p;
    ack_canon(a, pb, &Lx, &last);
    p = one_tile ? L.ptr[E] : a.pointer[E];
    done = 1;
  } else {
    p = one_tile ? L.ptr[a.n - 1u] : a.pointer[a.n - 1u];
    ack_canon(a, p, &Lx, &last);
  }
  if (slow) {
    if (tid == 0) L.end = a.n;
    const uint32_t o = one_tile ? (uint32_t)A : 0u;  // where the block sits in the LDS tile
    for (uint64_t b0 = A; b0 < a.n; b0 += kAckTile) {
      const uint32_t Rv = a.n - b0 < kAckTile ? (uint32_t)(a.n - b0) : kAckTile;
      __syncthreads();  // (every read of L.ptr above before the walk writes it)
      // one word per reply, so the walking lane reads four replies with one LDS load
      for (uint32_t k = tid; k < Rv; k += kBlock) {
        if (one_tile) {
          L.pk[k] = (uint32_t)L.ack[o + k] | (uint32_t)L.fl[o + k] << 16 | (uint32_t)L.us[o + k] << 24;
        } else {
          const uint32_t us = a.usable ? (uint32_t)(a.usable[b0 + k] != 0) : 1u;
          L.pk[k] = (uint32_t)a.ack[b0 + k] | (uint32_t)a.flags[b0 + k] << 16 | us << 24;
        }
      }
      __syncthreads();
      if (tid == 0) {
        uint32_t judged = Rv;
        for (uint32_t k = 0; k < Rv && judged == Rv; k += 4) {
          uint32_t w[4];
#pragma unroll
          for (uint32_t u = 0; u < 4; ++u) w[u] = L.pk[k + u];  // (k + u < kAckTile; past Rv unused)
#pragma unroll
          for (uint32_t u = 0; u < 4; ++u) {
            if (k + u >= Rv) break;
            const uint32_t ack = w[u] & 0xFFFFu, fl = (w[u] >> 16) & 0xFFu, us = (w[u] >> 24) & 1u;
            const bool valid = ack_valid(a, us, ack, p, Lx);
            bool fin = false;
            if (valid) {
              if (fl & 0x40u) p = ack - a.isn;
              if (fl & 0x20u) fin = true;
              else if (last) Lx = 0;
              else {
                Lx = p <= a.T ? ack_min64(a.C, a.T - p) : 0ull;  // (p > T: from a state that is not canonical)
                last = p + Lx == a.T;
              }
            }
            L.val[o + k + u] = (uint8_t)valid;
            L.ptr[o + k + u] = p;
            if (fin) {
              L.end = b0 + k + u;
              judged = k + u + 1u;
              break;
            }
          }
        }
        L.cnt = judged;
      }
      __syncthreads();
      if (!one_tile)
        for (uint32_t k = tid; k < L.cnt; k += kBlock) {
          a.valid[b0 + k] = L.val[k];
          a.pointer[b0 + k] = L.ptr[k];
        }
      if (L.end != a.n) break;  // (uniform)
    }
    end = L.end;
  }
  __syncthreads();  // every read of L.end before it is written again
  if (tid == 0) {
    if (slow && end < a.n) done = 1;
    a.state_out[0] = p;
    a.state_out[1] = Lx;
    a.state_out[2] = last;
    a.state_out[3] = done;
    ack_write_info(a, end, seed.p, p, slow ? A : a.n, done);
    L.end = end;
    L.p_out = p;
  }
  __syncthreads();
}

// Nothing to judge (n == 0, or done set on entry): the state copied, d_info for
// it.  (valid and pointer of a batch that is not judged are zeroed by the caller.)
__device__ __forceinline__ void ack_idle(const AckArgs& a, AckSeed seed) {
  __syncthreads();  // d_state_out may be d_state_in: every read first
  if (threadIdx.x == 0) {
    a.state_out[0] = seed.p;
    a.state_out[1] = seed.L;
    a.state_out[2] = seed.last;
    a.state_out[3] = seed.done;
    a.info[1] = 0;
    ack_write_info(a, a.n, seed.p, seed.p, a.n, seed.done);
  }
}

// Steps 2 to 5 for a batch of one tile (0 < n <= kAckTile, done not set) whose
// ack, fl and us are in LDS (ack_load, or the fused kernel's decode) and whose
// L.e_min and L.a_min were initialised before the barrier that published them.
// Leaves L.end and L.p_out set and every output in global memory.
__device__ inline void ack_one_tile(const AckArgs& a, AckLds& L, AckSeed seed) {
  const uint32_t Rv = (uint32_t)a.n, tid = threadIdx.x;
  ack_scan(a, L, 0, Rv, seed.p);
  __syncthreads();
  const uint64_t E = L.e_min, A = L.a_min;
  ack_finish(a, L, seed, E, A, true);
  if (tid == 0) L.cnt = 0;
  __syncthreads();
  const uint64_t end = L.end;
  uint32_t mine = 0;
  for (uint32_t k = tid; k < Rv; k += kBlock) {
    const bool in = k <= end;
    a.valid[k] = in ? L.val[k] : (uint8_t)0;
    a.pointer[k] = in ? L.ptr[k] : 0ull;
    mine += in && L.val[k];
  }
  mine = (uint32_t)wave_sum64(mine);
  if ((tid & 63u) == 0 && mine) atomicAdd(&L.cnt, mine);
  __syncthreads();
  if (tid == 0) a.info[1] = L.cnt;
}

__device__ __forceinline__ AckSeed ack_seed(const uint64_t* st) {
  return AckSeed{st[0], st[1], st[2] ? 1ull : 0ull, st[3] ? 1ull : 0ull};
}

// A batch of at most one tile, n == 0 included: every step in one launch.
__global__ void __launch_bounds__(kBlock) ack_single_kernel(AckArgs a) {
  __shared__ AckLds L;
  const uint32_t tid = threadIdx.x;
  const AckSeed seed = ack_seed(a.state_in);
  if (a.n == 0 || seed.done) {  // (uniform)
    for (uint32_t k = tid; k < a.n; k += kBlock) {
      a.valid[k] = 0;
      a.pointer[k] = 0;
    }
    ack_idle(a, seed);
    return;
  }
  if (tid == 0) {
    L.e_min = a.n;
    L.a_min = a.n;
  }
  ack_load(a, L, 0, (uint32_t)a.n);
  __syncthreads();
  ack_one_tile(a, L, seed);
}

__global__ void __launch_bounds__(kBlock) ack_join_kernel(AckArgs a) {
  __shared__ AckLds L;
  const uint64_t p0 = (uint64_t)blockIdx.x * kAckTile;
  const uint32_t Rv = a.n - p0 < kAckTile ? (uint32_t)(a.n - p0) : kAckTile;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const AckSeed seed = ack_seed(a.state_in);
    a.hdr[0] = seed.p;
    a.hdr[1] = seed.L;
    a.hdr[2] = seed.last;
    a.hdr[3] = seed.done;
    a.hdr[4] = a.n;
    a.hdr[5] = a.n;
    a.info[1] = 0;
  }
  ack_load(a, L, p0, Rv);
  __syncthreads();
  const uint64_t t = ack_tile_max(a, L, Rv);
  if (threadIdx.x == 0) a.hdr[kAckHdr + blockIdx.x] = t;
}

// One workgroup: max[t] <- state_in's p joined with the maxima before t, each
// thread over a run of consecutive tiles (one each up to 256 tiles).
__global__ void __launch_bounds__(kBlock) ack_bases_kernel(uint64_t* hdr, uint64_t nt) {
  __shared__ uint64_t wv[kBlock / 64];
  uint64_t* tiles = hdr + kAckHdr;
  const uint64_t per = (nt + kBlock - 1u) / kBlock;
  const uint64_t lo = threadIdx.x * per < nt ? threadIdx.x * per : nt, hi = lo + per < nt ? lo + per : nt;
  uint64_t mine = 0;
  for (uint64_t i = lo; i < hi; ++i) mine = ack_max64(mine, tiles[i]);
  uint64_t run = ack_max64(hdr[0], block_exclusive_max(mine, wv));
  for (uint64_t i = lo; i < hi; ++i) {
    const uint64_t v = tiles[i];
    tiles[i] = run;
    run = ack_max64(run, v);
  }
}

__global__ void __launch_bounds__(kBlock) ack_tile_kernel(AckArgs a) {
  __shared__ AckLds L;
  const uint64_t p0 = (uint64_t)blockIdx.x * kAckTile;
  const uint32_t Rv = a.n - p0 < kAckTile ? (uint32_t)(a.n - p0) : kAckTile;
  if (a.hdr[3]) {  // done on entry: nothing is judged (uniform)
    for (uint32_t k = threadIdx.x; k < Rv; k += kBlock) {
      a.valid[p0 + k] = 0;
      a.pointer[p0 + k] = 0;
    }
    return;
  }
  if (threadIdx.x == 0) {
    L.e_min = a.n;
    L.a_min = a.n;
  }
  const uint64_t base = a.hdr[kAckHdr + blockIdx.x];
  ack_load(a, L, p0, Rv);
  __syncthreads();
  ack_scan(a, L, p0, Rv, base);
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < Rv; k += kBlock) {
    a.valid[p0 + k] = L.val[k];
    a.pointer[p0 + k] = L.ptr[k];
  }
  if (threadIdx.x == 0) {
    if (L.e_min < a.n) atomicMin(reinterpret_cast<unsigned long long*>(a.hdr + 4), L.e_min);
    if (L.a_min < a.n) atomicMin(reinterpret_cast<unsigned long long*>(a.hdr + 5), L.a_min);
  }
}

__global__ void __launch_bounds__(kBlock) ack_finish_kernel(AckArgs a) {
  __shared__ AckLds L;
  const AckSeed seed{a.hdr[0], a.hdr[1], a.hdr[2], a.hdr[3]};
  if (seed.done) {  // (uniform)
    ack_idle(a, seed);
    return;
  }
  ack_finish(a, L, seed, a.hdr[4], a.hdr[5], false);
}

// Step 5 for the tile at blockIdx.x: zeroes past the end, and the tile's valid
// replies added to d_info[1] by one atomic.
__global__ void __launch_bounds__(kBlock) ack_final_kernel(AckArgs a) {
  __shared__ uint32_t s_count;
  const uint64_t p0 = (uint64_t)blockIdx.x * kAckTile, end = a.info[0];
  if (threadIdx.x == 0) s_count = 0;
  __syncthreads();
  uint32_t mine = 0;
#pragma unroll
  for (uint32_t j = 0; j < kAckFpt; ++j) {
    const uint64_t i = p0 + j * kBlock + threadIdx.x;
    if (i >= a.n) break;
    if (i > end) {
      a.valid[i] = 0;
      a.pointer[i] = 0;
    } else {
      mine += a.valid[i] != 0;
    }
  }
  mine = (uint32_t)wave_sum64(mine);
  if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(&s_count, mine);
  __syncthreads();
  if (threadIdx.x == 0 && s_count)
    atomicAdd(reinterpret_cast<unsigned long long*>(a.info + 1), (unsigned long long)s_count);
}

int launch_ack_progress(AckArgs a, hipStream_t stream) {
  if (a.n <= kAckTile) {
    hipLaunchKernelGGL(ack_single_kernel, dim3(1), dim3(kBlock), 0, stream, a);
    return (int)hipGetLastError();
  }
  const uint64_t nt = (a.n + kAckTile - 1u) / kAckTile;
  if (nt > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
  hipError_t e = stream_scratch(reinterpret_cast<void**>(&a.hdr), (kAckHdr + nt) * sizeof(uint64_t), stream,
                                kScratchSums);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(ack_join_kernel, dim3((uint32_t)nt), dim3(kBlock), 0, stream, a);
  hipLaunchKernelGGL(ack_bases_kernel, dim3(1), dim3(kBlock), 0, stream, a.hdr, nt);
  hipLaunchKernelGGL(ack_tile_kernel, dim3((uint32_t)nt), dim3(kBlock), 0, stream, a);
  hipLaunchKernelGGL(ack_finish_kernel, dim3(1), dim3(kBlock), 0, stream, a);
  hipLaunchKernelGGL(ack_final_kernel, dim3((uint32_t)nt), dim3(kBlock), 0, stream, a);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------ the closing datagram

// send_ack's packet (utils/reliableUDP.py:87-93): seq = (isn + p) mod 2^16, ack
// = (seq_end + 1) mod 2^16, flags 0x40; a lane of the calling wave stores one
// byte each.  (Called by whole waves; lanes past the header do nothing.)
template <int H>
__device__ __forceinline__ void ack_put_final(unsigned char* frame, uint16_t* csum_or_null, uint32_t isn, uint64_t p,
                                              uint32_t seq_end) {
  const uint32_t seq = (uint32_t)((isn + p) & 0xFFFFu), ack = (seq_end + 1u) & 0xFFFFu;
  const uint32_t c = packet_csum(0u, seq, ack, 0x40u);
  const uint64_t h = pack_header<H>(seq, ack, 0x40u, c);
  const uint32_t lane = threadIdx.x & 63u;
  if (lane < (uint32_t)H) frame[lane] = (unsigned char)(h >> (8u * lane));
  if (lane == 0 && csum_or_null) *csum_or_null = (uint16_t)c;
}

// The chained form's builder: one wave, after rudp_ack_progress' launches.
template <int H>
__global__ void __launch_bounds__(64) ack_final_frame_kernel(AcknowledgeArgs a) {
  const uint64_t end = a.r.info[0];
  if (end >= a.r.n) return;
  ack_put_final<H>(a.final_frame, a.final_csum, a.r.isn, a.r.state_out[0], a.seq[end]);
}

int launch_ack_final_frame(const AcknowledgeArgs& a, hipStream_t stream) {
  if (a.H == 7u) hipLaunchKernelGGL(ack_final_frame_kernel<7>, dim3(1), dim3(64), 0, stream, a);
  else hipLaunchKernelGGL(ack_final_frame_kernel<5>, dim3(1), dim3(64), 0, stream, a);
  return (int)hipGetLastError();
}

__global__ void __launch_bounds__(kBlock) ack_usable_kernel(const uint8_t* ok, uint8_t* usable, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t o = ok[i];
  usable[i] = (uint8_t)(o == RUDP_OK_GOOD || o == RUDP_OK_UNVERIFIED);
}

int launch_ack_usable(const uint8_t* ok, uint8_t* usable, uint64_t n, hipStream_t stream) {
  const uint64_t nb = (n + kBlock - 1u) / kBlock;
  if (nb == 0 || nb > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(ack_usable_kernel, dim3((uint32_t)nb), dim3(kBlock), 0, stream, ok, usable, n);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------ fused form

struct AckFusedLds {
  AckLds t;
  uint32_t fo[kAckTile + 1];  // frame offsets in the image (kImgBadOff: past the buffer)
  uint16_t seq[kAckTile];
  uint32_t bad;               // a frame failed the offset rule
  // the aligned buffer from the 16-B boundary below d_frames, and window16_dw's reach past it
  __attribute__((aligned(16))) uint32_t img[(kAckFusedBytes + 16u + 32u) / 4u];
};

template <int H>
__global__ void __launch_bounds__(kBlock) acknowledge_fused_kernel(AcknowledgeArgs a) {
  __shared__ AckFusedLds S;
  AckLds& L = S.t;
  const uint32_t tid = threadIdx.x;
  const AckArgs& r = a.r;
  const AckSeed seed = ack_seed(r.state_in);
  if (r.n == 0) {  // (uniform)
    ack_idle(r, seed);
    if (tid == 0) *a.status = 0;
    return;
  }
  const uint32_t n = (uint32_t)r.n;

  // 1. the buffer into LDS once, and its offsets
  {
    image_load(S.img, a.frames, a.frames_bytes ? (uint32_t)(a.fmis + a.frames_bytes) : 0u, kBlock);
    image_offsets(S.fo, a.frame_off, n, a.frames_bytes, a.fmis, kBlock);
    if (tid == 0) {
      L.e_min = r.n;
      L.a_min = r.n;
      S.bad = 0;
    }
  }
  __syncthreads();

  // 2. every frame by one lane: the decode's outputs and usable
  {
    uint32_t any_bad = 0;
#pragma unroll 1
    for (uint32_t j = 0; j < kAckFpt; ++j) {
      const uint32_t q = j * kBlock + tid;
      if (q >= n) break;
      const FrameDecode d = image_decode_frame<H, false>(S.img, S.fo[q], S.fo[q + 1u], a.csum_in != nullptr,
                                                         [&] { return (uint32_t)a.csum_in[q]; });
      any_bad |= d.ok == RUDP_OK_BAD_OFFSETS;
      const uint32_t us = d.ok == RUDP_OK_GOOD || d.ok == RUDP_OK_UNVERIFIED;
      a.seq[q] = (uint16_t)d.seq;
      a.ack[q] = (uint16_t)d.ack;
      a.flags[q] = (uint8_t)d.fl;
      a.ok[q] = (uint8_t)d.ok;
      if (a.csum_out) a.csum_out[q] = (uint16_t)d.cs;
      a.usable[q] = (uint8_t)us;
      S.seq[q] = (uint16_t)d.seq;
      L.ack[q] = (uint16_t)d.ack;
      L.fl[q] = (uint8_t)d.fl;
      L.us[q] = (uint8_t)us;
    }
    if (any_bad) atomicOr(&S.bad, 1u);
  }
  __syncthreads();

  // 3. the rule on the LDS tile;  4. the closing datagram, status
  if (seed.done) {  // (uniform) nothing is judged
    for (uint32_t k = tid; k < n; k += kBlock) {
      r.valid[k] = 0;
      r.pointer[k] = 0;
    }
    ack_idle(r, seed);
  } else {
    ack_one_tile(r, L, seed);  // (its last barrier is behind thread 0's L.end and L.p_out)
    if (tid < 64u && L.end < r.n) ack_put_final<H>(a.final_frame, a.final_csum, r.isn, L.p_out, S.seq[L.end]);
  }
  if (tid == 0) *a.status = S.bad ? RUDP_ST_OFFSETS : 0u;
}

bool acknowledge_fused_ok(uint64_t n, uint64_t frames_bytes) {
  if (n == 0) return true;
  const int knob = tuning().acknowledge_fused;  // (2, diagnostics build: whatever the mean frame length)
  return knob && n <= kAckTile && frames_bytes <= kAckFusedBytes &&
         (knob == 2 || frames_bytes <= (uint64_t)kAckFusedMeanFrame * n);
}

int launch_acknowledge_fused(const AcknowledgeArgs& a, hipStream_t stream) {
  if (a.H == 7u) hipLaunchKernelGGL(acknowledge_fused_kernel<7>, dim3(1), dim3(kBlock), 0, stream, a);
  else hipLaunchKernelGGL(acknowledge_fused_kernel<5>, dim3(1), dim3(kBlock), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace rudp
