// The device functions of the in-order acceptance (accept.hip states the rule
// and the steps): accept.hip's kernels run them on tiles loaded from the
// tables, receive.hip's fused kernel runs acc_one_tile on a tile it decoded
// into LDS itself, and its reply builder classes frames with acc_class.
#pragma once
#include "codec_device.hpp"
#include "internal.hpp"
#include "scan_device.hpp"

namespace RUDP_NS {

constexpr uint32_t kAccFpt = 4;                   // consecutive frames per thread
constexpr uint32_t kAccTile = kBlock * kAccFpt;   // 1024
constexpr uint32_t kAccHdr = 8;                   // scratch words before the tile pairs
// scratch: [0] expect, [1] isn, [2] live of d_state_in; [3] first accepted FIN
// under the guess, [4] first anomaly (n: none); [kAccHdr + 2 t] tile t's pair.

struct AccP {
  uint64_t m;  // prefix maximum of seq + c since the last reset (a reset: its own seq + c)
  uint64_t r;  // 1 + index of the last reset, 0: none
};
__device__ __forceinline__ AccP acc_join(AccP a, AccP b) {
  if (b.r) return b;
  return AccP{a.m > b.m ? a.m : b.m, a.r};
}

enum : uint32_t { kAccSkip = 0, kAccDupSyn = 1, kAccReset = 2, kAccData = 3 };
__device__ __forceinline__ uint32_t acc_class(uint32_t usable, uint32_t fl, uint32_t seq, uint32_t last_isn) {
  if (!usable) return kAccSkip;
  if (fl & 0x80u) return seq == last_isn ? kAccDupSyn : kAccReset;
  return kAccData;
}
// The guessed state after frame g.  (A frame before any reset of a receiver
// that is not live raises m too; m is not used until a reset replaces it.)
__device__ __forceinline__ AccP acc_step(AccP s, uint32_t cls, uint64_t g, uint32_t seq, uint32_t c) {
  const uint64_t v = (uint64_t)seq + c;
  if (cls == kAccReset) return AccP{v, g + 1u};
  if (cls == kAccData && v > s.m) s.m = v;
  return s;
}

struct AccSeed {
  uint64_t expect, isn, live;
};

struct AccLds {
  uint32_t ch[kAccTile];
  uint16_t seq[kAccTile];
  uint16_t ack[kAccTile];
  uint8_t fl[kAccTile];
  uint8_t us[kAccTile];
  uint8_t acc[kAccTile];
  uint8_t rep[kAccTile];
  uint64_t pk[kAccTile];            // the walk: seq | flags << 16 | usable << 24 | chars << 32
  uint64_t wm[kBlock / 64], wr[kBlock / 64];
  unsigned long long e_min, a_min;  // first accepted FIN, first anomaly (n: none)
  uint64_t st_m, st_r;              // the state acc_scan was asked for
  uint64_t end, ms;                 // finish: the call's end and msg_start
  uint32_t cnt;                     // walk: frames of the block that were judged
};

// Exclusive scan of one pair per thread under acc_join (all threads call it).
__device__ inline AccP block_exclusive_join(AccP x, AccP* total, uint64_t* wm, uint64_t* wr) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  AccP incl = x;
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const AccP y{__shfl_up(incl.m, d, 64), __shfl_up(incl.r, d, 64)};
    if (lane >= d) incl = acc_join(y, incl);
  }
  if (lane == 63) {
    wm[wave] = incl.m;
    wr[wave] = incl.r;
  }
  AccP ex{__shfl_up(incl.m, 1, 64), __shfl_up(incl.r, 1, 64)};
  if (lane == 0) ex = AccP{0, 0};
  __syncthreads();
  AccP before{0, 0}, all{0, 0};
  for (uint32_t w = 0; w < nwaves; ++w) {
    const AccP v{wm[w], wr[w]};
    if (w < wave) before = acc_join(before, v);
    all = acc_join(all, v);
  }
  __syncthreads();  // wm / wr may be reused by the caller
  *total = all;
  return acc_join(before, ex);
}

// Frames [p0, p0 + Rv) into LDS, coalesced.
__device__ __forceinline__ void acc_load(const AcceptArgs& a, AccLds& L, uint64_t p0, uint32_t Rv) {
  for (uint32_t k = threadIdx.x; k < Rv; k += kBlock) {
    L.seq[k] = a.seq[p0 + k];
    L.fl[k] = a.flags[p0 + k];
    L.ch[k] = a.chars[p0 + k];
    L.us[k] = a.usable ? (uint8_t)(a.usable[p0 + k] != 0) : (uint8_t)1;
  }
}

// The join of the tile in LDS (all threads get it).
__device__ inline AccP acc_tile_join(const AcceptArgs& a, AccLds& L, uint64_t p0, uint32_t Rv) {
  AccP agg{0, 0};
#pragma unroll
  for (uint32_t j = 0; j < kAccFpt; ++j) {
    const uint32_t k = threadIdx.x * kAccFpt + j;
    if (k < Rv) agg = acc_step(agg, acc_class(L.us[k], L.fl[k], L.seq[k], a.last_isn), p0 + k, L.seq[k], L.ch[k]);
  }
  AccP total;
  block_exclusive_join(agg, &total, L.wm, L.wr);
  return total;
}

// The tile in LDS judged under the guess from `base`, the state before frame
// p0: accept, reply and reply_ack into LDS, the minima into L.e_min / L.a_min.
__device__ inline void acc_scan(const AcceptArgs& a, AccLds& L, uint64_t p0, uint32_t Rv, AccP base,
                                uint64_t seed_live) {
  const uint32_t tid = threadIdx.x;
  uint32_t cls[kAccFpt];
  AccP agg{0, 0};
#pragma unroll
  for (uint32_t j = 0; j < kAccFpt; ++j) {
    const uint32_t k = tid * kAccFpt + j;
    cls[j] = k < Rv ? acc_class(L.us[k], L.fl[k], L.seq[k], a.last_isn) : (uint32_t)kAccSkip;
    if (k < Rv) agg = acc_step(agg, cls[j], p0 + k, L.seq[k], L.ch[k]);
  }
  AccP total;
  AccP s = acc_join(base, block_exclusive_join(agg, &total, L.wm, L.wr));
  unsigned long long e_min = a.n, a_min = a.n;
#pragma unroll
  for (uint32_t j = 0; j < kAccFpt; ++j) {
    const uint32_t k = tid * kAccFpt + j;
    if (k >= Rv) break;
    const uint64_t g = p0 + k;
    const uint32_t seq = L.seq[k], c = L.ch[k];
    const bool live = seed_live || s.r;
    uint32_t acc = cls[j] == kAccReset;
    if (cls[j] == kAccData && live) {
      if ((uint64_t)seq == s.m) acc = 1;
      else if ((uint64_t)seq + c > s.m && g < a_min) a_min = g;
    }
    s = acc_step(s, cls[j], g, seq, c);
    const bool rep = cls[j] != kAccSkip && (seed_live || s.r);
    L.acc[k] = (uint8_t)acc;
    L.rep[k] = (uint8_t)rep;
    L.ack[k] = rep ? (uint16_t)s.m : (uint16_t)0;
    if (acc && (L.fl[k] & 0x20u) && g < e_min) e_min = g;
  }
  if (e_min < a.n) atomicMin(&L.e_min, e_min);
  if (a_min < a.n) atomicMin(&L.a_min, a_min);
}

// The guessed state before (excl) or after frame `want` of the tile in LDS,
// from `base`, the state before frame p0: into L.st_m / L.st_r.  Nothing else
// is written.
__device__ inline void acc_state_at(const AcceptArgs& a, AccLds& L, uint64_t p0, uint32_t Rv, AccP base,
                                    uint64_t want, bool excl) {
  const uint32_t k0 = threadIdx.x * kAccFpt;
  AccP agg{0, 0};
#pragma unroll
  for (uint32_t j = 0; j < kAccFpt; ++j) {
    const uint32_t k = k0 + j;
    if (k < Rv) agg = acc_step(agg, acc_class(L.us[k], L.fl[k], L.seq[k], a.last_isn), p0 + k, L.seq[k], L.ch[k]);
  }
  AccP total;
  AccP s = acc_join(base, block_exclusive_join(agg, &total, L.wm, L.wr));
  if (want < p0 + k0 || want >= p0 + k0 + kAccFpt) return;  // (after the scan's barriers)
  for (uint32_t k = k0; p0 + k <= want; ++k) {
    if (p0 + k == want && excl) break;
    s = acc_step(s, acc_class(L.us[k], L.fl[k], L.seq[k], a.last_isn), p0 + k, L.seq[k], L.ch[k]);
  }
  L.st_m = s.m;
  L.st_r = s.r;
}

// Step 4 for one workgroup.  E, A: the first accepted FIN under the guess and
// the first anomaly (n: none).  pairs: the exclusive tile bases, or null when
// the batch is one tile.  Leaves the end and msg_start in L.end / L.ms.
__device__ inline void acc_finish(const AcceptArgs& a, AccLds& L, AccSeed seed, uint64_t E, uint64_t A,
                                  const uint64_t* pairs) {
  const uint32_t tid = threadIdx.x;
  const bool slow = A < E;
  const uint64_t g = slow ? A : (E < a.n ? E : a.n - 1u);
  {
    const uint64_t tile = g / kAccTile, p0 = tile * kAccTile;
    const uint32_t Rv = a.n - p0 < kAccTile ? (uint32_t)(a.n - p0) : kAccTile;
    const AccP base = pairs ? AccP{pairs[2u * tile], pairs[2u * tile + 1u]} : AccP{seed.expect, 0};
    if (pairs) acc_load(a, L, p0, Rv);  // (a one-tile batch: the caller left its tile's inputs in LDS)
    __syncthreads();
    acc_state_at(a, L, p0, Rv, base, g, slow);
    __syncthreads();
  }
  // the state before frame A (slow) or after the last judged frame
  const uint64_t r = L.st_r;
  uint64_t live = seed.live || r ? 1u : 0u;
  uint64_t isn = r ? (uint64_t)a.seq[r - 1u] : seed.isn;
  uint64_t expect = live ? L.st_m : seed.expect;
  uint64_t ms = r ? r - 1u : a.n;
  uint64_t end = E;
  if (slow) {
    if (tid == 0) L.end = a.n;
    for (uint64_t b0 = A; b0 < a.n; b0 += kAccTile) {
      const uint32_t Rv = a.n - b0 < kAccTile ? (uint32_t)(a.n - b0) : kAccTile;
      __syncthreads();
      acc_load(a, L, b0, Rv);
      __syncthreads();
      // one word per frame, so the walking lane reads four frames with two LDS loads
      for (uint32_t k = tid; k < Rv; k += kBlock)
        L.pk[k] = (uint64_t)L.seq[k] | (uint64_t)L.fl[k] << 16 | (uint64_t)L.us[k] << 24 | (uint64_t)L.ch[k] << 32;
      __syncthreads();
      if (tid == 0) {
        uint32_t judged = Rv;
        for (uint32_t k = 0; k < Rv && judged == Rv; k += 4) {
          uint64_t w[4];
#pragma unroll
          for (uint32_t u = 0; u < 4; ++u) w[u] = L.pk[k + u];  // (k + u < kAccTile; past Rv unused)
#pragma unroll
          for (uint32_t u = 0; u < 4; ++u) {
            if (k + u >= Rv) break;
            const uint32_t seq = (uint32_t)w[u] & 0xFFFFu, fl = (uint32_t)(w[u] >> 16) & 0xFFu;
            const uint32_t us = (uint32_t)(w[u] >> 24) & 1u, c = (uint32_t)(w[u] >> 32);
            uint32_t acc = 0;
            if (us) {
              if (fl & 0x80u) {
                if (seq != a.last_isn) {
                  isn = seq;
                  expect = (uint64_t)seq + c;
                  live = 1;
                  ms = b0 + k + u;
                  acc = 1;
                }
              } else if (live && (uint64_t)seq == expect) {
                expect += c;
                acc = 1;
              }
            }
            L.ch[k + u] = acc | (us && live ? ((uint32_t)expect & 0xFFFFu) << 8 : 0u);  // accept | reply_ack << 8
            if (acc && (fl & 0x20u)) {
              L.end = b0 + k + u;
              judged = k + u + 1u;
              break;
            }
          }
        }
        L.cnt = judged;
      }
      __syncthreads();
      for (uint32_t k = tid; k < L.cnt; k += kBlock) {
        a.accept[b0 + k] = (uint8_t)(L.ch[k] & 1u);
        a.reply_ack[b0 + k] = (uint16_t)(L.ch[k] >> 8);
      }
      if (L.end != a.n) break;  // (uniform)
    }
    end = L.end;
  }
  __syncthreads();  // every read of L.end before it is written again
  if (tid == 0) {
    a.state_out[0] = expect;
    a.state_out[1] = isn;
    a.state_out[2] = live;
    a.state_out[3] = 0;
    a.info[0] = end;
    a.info[2] = ms;
    a.info[3] = live ? expect - isn : 0ull;
    a.info[4] = slow ? A : a.n;
    a.info[5] = 0;
    L.end = end;
    L.ms = ms;
  }
  __syncthreads();
}

// Step 5 for the tile of kAccTile frames at p0 (every thread of the workgroup
// calls it): keep, zeroes past the end, and the tile's accepted frames added to
// d_info[1] by one atomic.
__device__ __forceinline__ void acc_final(const AcceptArgs& a, uint64_t p0, uint64_t end, uint64_t ms,
                                          uint32_t* s_count) {
  if (threadIdx.x == 0) *s_count = 0;
  __syncthreads();
  uint32_t mine = 0;
#pragma unroll
  for (uint32_t j = 0; j < kAccFpt; ++j) {
    const uint64_t i = p0 + j * kBlock + threadIdx.x;
    if (i >= a.n) break;
    if (i > end) {
      a.accept[i] = 0;
      a.keep[i] = 0;
      a.reply[i] = 0;
      a.reply_ack[i] = 0;
    } else {
      const uint32_t acc = a.accept[i] != 0;
      a.keep[i] = (uint8_t)(acc && (ms == a.n || i >= ms));
      mine += acc;
    }
  }
  mine = (uint32_t)wave_sum64(mine);
  if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(s_count, mine);
  __syncthreads();
  if (threadIdx.x == 0 && *s_count)
    atomicAdd(reinterpret_cast<unsigned long long*>(a.info + 1), (unsigned long long)*s_count);
}

__device__ __forceinline__ void acc_store(const AcceptArgs& a, const AccLds& L, uint64_t p0, uint32_t Rv) {
  for (uint32_t k = threadIdx.x; k < Rv; k += kBlock) {
    a.accept[p0 + k] = L.acc[k];
    a.reply[p0 + k] = L.rep[k];
    a.reply_ack[p0 + k] = L.ack[k];
  }
}

// An empty batch: the state copied, d_info for it.
__device__ __forceinline__ void acc_empty(const AcceptArgs& a, AccSeed seed) {
  __syncthreads();  // d_state_out may be d_state_in: every read first
  if (threadIdx.x == 0) {
    a.state_out[0] = seed.expect;
    a.state_out[1] = seed.isn;
    a.state_out[2] = seed.live;
    a.state_out[3] = 0;
    a.info[0] = a.info[1] = a.info[2] = a.info[4] = a.info[5] = 0;
    a.info[3] = seed.live ? seed.expect - seed.isn : 0ull;
  }
}

// Steps 2 to 5 for a batch of one tile (0 < n <= kAccTile) whose seq, fl, ch
// and us are in LDS (acc_load, or the fused receive kernel's decode: those
// four are also at a.seq, a.flags, a.chars and a.usable, which the walk and
// the finish read) and whose L.e_min, L.a_min and a.info[1] were initialised
// before the barrier that published them.  Leaves L.end and L.ms set and every
// output in global memory, visible to the workgroup after a barrier.
__device__ inline void acc_one_tile(const AcceptArgs& a, AccLds& L, AccSeed seed) {
  const uint32_t Rv = (uint32_t)a.n;
  acc_scan(a, L, 0, Rv, AccP{seed.expect, 0}, seed.live);
  __syncthreads();
  acc_store(a, L, 0, Rv);
  const uint64_t E = L.e_min, A = L.a_min;
  acc_finish(a, L, seed, E, A, nullptr);  // (its barriers order the stores above before step 5's loads)
  acc_final(a, 0, L.end, L.ms, &L.cnt);
}

}  // namespace rudp
