// The device functions of rudp_ack_flows (ack_flows.hip states the steps): one
// workgroup groups a batch of at most 1024 replies by flow in LDS and judges
// every flow's run by rudp_ack_progress' rule, the runs side by side.  The
// skeleton (keys, sort, run heads, one block scan) is flows_device.hpp's; the
// guess, the candidates and the anomalies are acknowledge.hip's, taken per run
// with the run's own constants.
#pragma once
#include "codec_device.hpp"
#include "internal.hpp"
#include "scan_device.hpp"

namespace RUDP_NS {

constexpr uint32_t kAfFpt = 4;                  // consecutive sorted positions (and runs) per thread
constexpr uint32_t kAfMax = kBlock * kAfFpt;    // 1024 == RUDP_FLOWS_MAX_BATCH
constexpr uint32_t kAfNil = 0xFFFFu;            // no position
constexpr uint32_t kAfNoEvent = 0xFFFFFFFFu;
constexpr uint32_t kAfCanon = 1u, kAfDone = 2u; // rflag: the row is a canonical state; done was set on entry

// The guess's scan element: m = prefix maximum of the candidates since the
// run's head (the head: the row's p), h = a run head lies in the span.
struct AfP {
  uint64_t m;
  uint32_t h;
};
__device__ __forceinline__ AfP af_join(AfP a, AfP b) {
  if (b.h) return b;
  return AfP{a.m > b.m ? a.m : b.m, a.h};
}

// A run's constants (words 4 to 7 of its row).
struct AfRow {
  uint64_t isn, T, C, sent;
};

struct AckFlowLds {
  uint64_t key[kAfMax];        // step 2: slot << 10 | arrival index, sorted; from step 4: p after position q
  uint64_t rp[kAfMax];         // run: the row's p; from step 5: closing_seq | closing_ack << 16 of a run that ended
  uint64_t rT[kAfMax];         // run: T
  uint64_t rsent[kAfMax];      // run: sent
  uint32_t rslot[kAfMax];      // run: its slot
  uint32_t ev[kAfMax];         // run: its first event, position << 1 | (0: a valid FIN, 1: an anomaly);
                               // from step 6: the valid replies of the runs before it
  uint16_t ack[kAfMax];        // by arrival index, as fl and us
  uint16_t gi[kAfMax];         // position -> arrival index
  uint16_t run[kAfMax];        // position -> run
  uint16_t rstart[kAfMax + 2]; // run: its first position; [A]: the first position outside every run
  uint16_t risn[kAfMax];       // run: isn
  uint16_t rC[kAfMax];         // run: C
  uint16_t fend[kAfMax];       // run: the position that ended it, kAfNil: none
  uint8_t fl[kAfMax];
  uint8_t us[kAfMax];          // usable and of a judged row
  uint8_t val[kAfMax];         // by position
  uint8_t rflag[kAfMax];       // run: kAfCanon | kAfDone
  uint64_t wm[kBlock / 64];
  uint32_t wh[kBlock / 64], sw[kBlock / 64];
  unsigned long long newly;    // characters newly acknowledged in all
  uint32_t bad, walked;
};

__device__ __forceinline__ uint64_t af_min64(uint64_t a, uint64_t b) { return a < b ? a : b; }

// L of the canonical state at p (0 past T: from a state that is not canonical).
__device__ __forceinline__ uint64_t af_canon_len(const AfRow& c, uint64_t p) {
  return p <= c.T ? af_min64(c.C, c.T - p) : 0ull;
}
__device__ __forceinline__ bool af_canonical(const AfRow& c, uint64_t p, uint64_t Lx, bool last) {
  if (p > c.T || (p % c.C != 0 && p != c.T)) return false;
  const uint64_t Lc = af_min64(c.C, c.T - p);
  return Lx == Lc && last == (p + Lc == c.T);
}

// A candidate's characters, 0 for a reply that is none (0 never raises a maximum).
__device__ __forceinline__ uint64_t af_cand(const AfRow& c, uint32_t mode, uint32_t us, uint32_t fl, uint32_t ack) {
  if (!us || !(fl & 0x40u) || (uint64_t)ack < c.isn) return 0;
  const uint64_t d = ack - c.isn;
  if (d > (mode == RUDP_ACK_CUMULATIVE ? c.sent : c.T)) return 0;
  return (d % c.C == 0 || d == c.T) ? d : 0;
}

// valid_i for the state (p, L): isn + p + L is never formed, only differences are compared.
__device__ __forceinline__ bool af_valid(const AfRow& c, uint32_t mode, uint32_t us, uint32_t ack, uint64_t p,
                                         uint64_t Lx) {
  if (!us || (uint64_t)ack < c.isn) return false;
  const uint64_t d = ack - c.isn;
  if (d < p) return false;
  if (mode == RUDP_ACK_EXACT) return d - p == Lx;
  return d - p >= Lx && d <= c.sent && (d % c.C == 0 || d == c.T);
}

// Exclusive scan of one AfP per thread under af_join (all threads call it).
__device__ inline AfP af_block_exclusive_join(AfP x, AckFlowLds& L) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  AfP incl = x;
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const AfP y{__shfl_up(incl.m, d, 64), __shfl_up(incl.h, d, 64)};
    if (lane >= d) incl = af_join(y, incl);
  }
  if (lane == 63) {
    L.wm[wave] = incl.m;
    L.wh[wave] = incl.h;
  }
  AfP ex{__shfl_up(incl.m, 1, 64), __shfl_up(incl.h, 1, 64)};
  if (lane == 0) ex = AfP{0, 0};
  __syncthreads();
  AfP before{0, 0};
  for (uint32_t w = 0; w < nwaves; ++w)
    if (w < wave) before = af_join(before, AfP{L.wm[w], L.wh[w]});
  __syncthreads();  // wm / wh may be reused
  return af_join(before, ex);
}

// One closing datagram (rudp_acknowledge's: flags 0x40) into slot e of the tables.
template <int H>
__device__ __forceinline__ void af_put_final(const AckFlowsArgs& a, uint32_t e, uint32_t seq, uint32_t ack) {
  const uint32_t c = packet_csum(0u, seq, ack, 0x40u);
  const uint64_t h = pack_header<H>(seq, ack, 0x40u, c);
  unsigned char* o = a.final_frames + (uint64_t)e * (uint64_t)H;
#pragma unroll
  for (int b = 0; b < H; ++b) o[b] = (unsigned char)(h >> (8 * b));
  if (a.final_csum) a.final_csum[e] = (uint16_t)c;
}

// The whole call for one workgroup of kBlock threads (0 <= n <= kAfMax).  H:
// final_layout (0: no closing datagrams are built).
template <int H>
__device__ inline void ack_flows_judge(const AckFlowsArgs& a, AckFlowLds& L) {
  const uint32_t tid = threadIdx.x, n = (uint32_t)a.n, mode = a.mode;
  if (n == 0) {  // (uniform)
    if (tid < 8) a.info[tid] = 0;
    if (tid == 0) *a.status = 0;
    return;
  }
  uint32_t N2 = 2;
  while (N2 < n) N2 <<= 1;
  if (tid == 0) {
    L.bad = 0;
    L.walked = 0;
    L.newly = 0;
  }
  __syncthreads();

  // 1. the tables and the keys; a reply whose row is idle or refused has no flow
  for (uint32_t k = tid; k < N2; k += kBlock) {
    if (k >= n) {
      L.key[k] = ~0ull;
      continue;
    }
    const uint32_t f = a.flow[k];
    bool judged = (uint64_t)f < a.n_flows;  // (n_flows <= 2^32 - 2: RUDP_FLOW_NONE never is)
    if (!judged && f != RUDP_FLOW_NONE) atomicOr(&L.bad, RUDP_ST_FLOW);
    if (judged) {
      const uint64_t* row = a.states + 8ull * f;
      const uint64_t isn = row[4], T = row[5], C = row[6], sent = row[7];
      if (C == 0) {
        judged = false;  // an idle slot
      } else if (isn > 65535u || C > 16383u || (mode == RUDP_ACK_CUMULATIVE && sent > T)) {
        judged = false;
        atomicOr(&L.bad, RUDP_ST_FLOW_ROW);
      }
    }
    L.ack[k] = a.ack[k];
    L.fl[k] = a.flags[k];
    L.us[k] = (uint8_t)(judged && (a.usable ? a.usable[k] != 0 : true));
    L.key[k] = (uint64_t)(judged ? f : RUDP_FLOW_NONE) << 10 | k;
  }
  __syncthreads();

  // 2. sorted by slot, then by arrival; the replies without a judged flow last
  for (uint32_t k = 2; k <= N2; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = tid; t < (N2 >> 1); t += kBlock) {
        const uint32_t lo = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), hi = lo | j;
        const uint64_t x = L.key[lo], y = L.key[hi];
        if ((x > y) == ((lo & k) == 0u)) {
          L.key[lo] = y;
          L.key[hi] = x;
        }
      }
      __syncthreads();
    }
  }

  // 3. run heads: A, the order, every run's slot and first position; its row
  const uint32_t p0 = tid * kAfFpt;
  uint32_t A, M;
  {
    uint32_t head[kAfFpt], val[kAfFpt], cnt = 0;
#pragma unroll
    for (uint32_t j = 0; j < kAfFpt; ++j) {
      const uint32_t p = p0 + j;
      val[j] = p < n && (uint32_t)(L.key[p] >> 10) != RUDP_FLOW_NONE;
      head[j] = val[j] && (p == 0 || (L.key[p - 1u] >> 10) != (L.key[p] >> 10));
      cnt += head[j] | val[j] << 16;
    }
    uint32_t total;
    uint32_t run = block_exclusive_scan32(cnt, &total, L.sw) & 0xFFFFu;
    A = total & 0xFFFFu;
    M = total >> 16;
#pragma unroll
    for (uint32_t j = 0; j < kAfFpt; ++j) {
      const uint32_t p = p0 + j;
      if (p >= n) break;
      const uint32_t i = (uint32_t)L.key[p] & (kAfMax - 1u);
      L.gi[p] = (uint16_t)i;
      a.order[p] = i;
      if (head[j]) {
        L.rstart[run] = (uint16_t)p;
        L.rslot[run] = (uint32_t)(L.key[p] >> 10);
        a.order_off[run] = p;
        ++run;
      }
      L.run[p] = val[j] ? (uint16_t)(run - 1u) : (uint16_t)kAfNil;
    }
    if (tid == 0) {
      L.rstart[A] = (uint16_t)M;
      a.order_off[A] = M;
    }
  }
  __syncthreads();
  for (uint32_t r = tid; r < A; r += kBlock) {
    const uint64_t* row = a.states + 8ull * L.rslot[r];
    const AfRow c{row[4], row[5], row[6], row[7]};
    const uint64_t p = row[0];
    L.rp[r] = p;
    L.rT[r] = c.T;
    L.rsent[r] = c.sent;
    L.risn[r] = (uint16_t)c.isn;
    L.rC[r] = (uint16_t)c.C;
    L.rflag[r] = (uint8_t)((af_canonical(c, p, row[1], row[2] != 0) ? kAfCanon : 0u) | (row[3] ? kAfDone : 0u));
    L.ev[r] = kAfNoEvent;
  }
  __syncthreads();

  // 4. every run judged under the guess (the keys are dead: key[q] <- p after q)
  {
    uint64_t cand[kAfFpt];
    AfP agg{0, 0};
#pragma unroll
    for (uint32_t j = 0; j < kAfFpt; ++j) {
      const uint32_t q = p0 + j;
      cand[j] = 0;
      if (q < M) {
        const uint32_t i = L.gi[q], r = L.run[q];
        const AfRow c{L.risn[r], L.rT[r], L.rC[r], L.rsent[r]};
        cand[j] = af_cand(c, mode, L.us[i], L.fl[i], L.ack[i]);
        if (L.rstart[r] == q) agg = AfP{L.rp[r], 1};
        if (cand[j] > agg.m) agg.m = cand[j];
      }
    }
    AfP s = af_block_exclusive_join(agg, L);
#pragma unroll
    for (uint32_t j = 0; j < kAfFpt; ++j) {
      const uint32_t q = p0 + j;
      if (q >= M) break;
      const uint32_t i = L.gi[q], r = L.run[q];
      const AfRow c{L.risn[r], L.rT[r], L.rC[r], L.rsent[r]};
      const uint32_t fl = L.fl[i], ack = L.ack[i];
      if (L.rstart[r] == q) s = AfP{L.rp[r], 1};
      const uint64_t Lc = af_canon_len(c, s.m);
      const bool valid = af_valid(c, mode, L.us[i], ack, s.m, Lc);
      const bool live = !(L.rflag[r] & kAfDone);
      if (live) {
        if (valid && (fl & 0x20u)) atomicMin(&L.ev[r], q << 1);
        if (valid && !(fl & 0x40u)) atomicMin(&L.ev[r], q << 1 | 1u);
        if (mode == RUDP_ACK_EXACT && cand[j] > s.m && cand[j] - s.m > Lc) atomicMin(&L.ev[r], q << 1 | 1u);
      }
      L.val[q] = (uint8_t)valid;
      L.key[q] = valid && (fl & 0x40u) ? (uint64_t)ack - c.isn : s.m;
      if (cand[j] > s.m) s.m = cand[j];
    }
  }
  __syncthreads();

  // 5. one lane per run: the state after its last judged reply, the row and
  // the flow's info; a run whose first event is an anomaly (a seed that is not
  // canonical: at its head) is walked by the rule from there
  for (uint32_t r = tid; r < A; r += kBlock) {
    const uint32_t start = L.rstart[r], stop = L.rstart[r + 1u], e = L.ev[r], flag = L.rflag[r];
    const AfRow c{L.risn[r], L.rT[r], L.rC[r], L.rsent[r]};
    uint64_t* row = a.states + 8ull * L.rslot[r];
    uint64_t* fi = a.flow_info + 8ull * r;
    const uint64_t pin = L.rp[r];
    uint64_t p = pin, Lx = 0, done = 1;
    bool last = false;
    uint32_t endp = kAfNil;
    if (!(flag & kAfDone)) {
      done = 0;
      if ((flag & kAfCanon) && (e == kAfNoEvent || !(e & 1u))) {
        if (e == kAfNoEvent) {
          p = L.key[stop - 1u];
          Lx = af_canon_len(c, p);
          last = p + Lx == c.T;
        } else {  // the FIN leaves L and last as they were before it
          endp = e >> 1;
          const uint64_t pb = endp == start ? pin : L.key[endp - 1u];
          Lx = af_canon_len(c, pb);
          last = pb + Lx == c.T;
          p = L.key[endp];
          done = 1;
        }
      } else {
        uint32_t pa = start;
        if (flag & kAfCanon) {
          pa = e >> 1;
          if (pa != start) p = L.key[pa - 1u];
          Lx = af_canon_len(c, p);
          last = p + Lx == c.T;
        } else {
          Lx = row[1];
          last = row[2] != 0;
        }
        for (uint32_t q = pa; q < stop; ++q) {
          const uint32_t i = L.gi[q], fl = L.fl[i], ack = L.ack[i];
          const bool valid = af_valid(c, mode, L.us[i], ack, p, Lx);
          bool fin = false;
          if (valid) {
            if (fl & 0x40u) p = (uint64_t)ack - c.isn;
            if (fl & 0x20u) fin = true;
            else if (last) Lx = 0;
            else {
              Lx = af_canon_len(c, p);
              last = p + Lx == c.T;
            }
          }
          L.val[q] = (uint8_t)valid;
          L.key[q] = p;
          if (fin) {
            endp = q;
            done = 1;
            break;
          }
        }
        atomicAdd(&L.walked, 1u);
      }
      row[0] = p;
      row[1] = Lx;
      row[2] = last;
      row[3] = done;
    }
    uint64_t closing = 0;
    if (endp != kAfNil)
      closing = ((c.isn + p) & 0xFFFFull) | (uint64_t)((a.seq[L.gi[endp]] + 1u) & 0xFFFFu) << 16;
    L.fend[r] = (uint16_t)endp;
    L.rp[r] = closing;
    fi[0] = L.rslot[r];
    fi[1] = endp != kAfNil ? (uint64_t)L.gi[endp] : (uint64_t)n;
    fi[3] = p - pin;  // (mod 2^64 when a walk from a state that is not canonical went back)
    fi[4] = p;
    fi[5] = p / c.C + (p % c.C != 0);
    fi[6] = done;
    fi[7] = closing;
    if (p != pin) atomicAdd(&L.newly, (unsigned long long)(p - pin));
  }
  __syncthreads();

  // 6. the per-reply outputs, and an exclusive count of the valid replies in
  // sorted order: every run's base
  uint32_t count;
  {
    uint32_t v[kAfFpt], x = 0;
#pragma unroll
    for (uint32_t j = 0; j < kAfFpt; ++j) {
      const uint32_t q = p0 + j;
      v[j] = 0;
      if (q < M) {
        const uint32_t r = L.run[q];
        const bool judged = !(L.rflag[r] & kAfDone) && q <= L.fend[r];  // (kAfNil is above every position)
        v[j] = judged ? 1u | (uint32_t)L.val[q] << 1 : 0u;
      }
      x += v[j] >> 1;
    }
    uint32_t before = block_exclusive_scan32(x, &count, L.sw);
#pragma unroll
    for (uint32_t j = 0; j < kAfFpt; ++j) {
      const uint32_t q = p0 + j;
      if (q >= n) break;
      const uint32_t i = L.gi[q];
      if (q < M && L.rstart[L.run[q]] == q) L.ev[L.run[q]] = before;
      a.valid[i] = (uint8_t)(v[j] >> 1);
      a.pointer[i] = (v[j] & 1u) ? L.key[q] : 0ull;
      before += v[j] >> 1;
    }
  }
  __syncthreads();

  // 7. every flow's valid replies; the closing datagrams of the flows that
  // ended, in flow order (four consecutive runs per thread)
  uint32_t E;
  {
    uint32_t en = 0, cnt = 0;
#pragma unroll
    for (uint32_t j = 0; j < kAfFpt; ++j) {
      const uint32_t r = p0 + j;
      if (r >= A) break;
      a.flow_info[8ull * r + 2u] = (r + 1u < A ? L.ev[r + 1u] : count) - L.ev[r];
      if (L.fend[r] != kAfNil) {
        en |= 1u << j;
        ++cnt;
      }
    }
    uint32_t slot = block_exclusive_scan32(cnt, &E, L.sw);
    if (H != 0) {
#pragma unroll
      for (uint32_t j = 0; j < kAfFpt; ++j) {
        if (!(en & (1u << j))) continue;
        const uint32_t w = (uint32_t)L.rp[p0 + j];
        af_put_final<(H ? H : 5)>(a, slot, w & 0xFFFFu, w >> 16);
        a.final_flow[slot] = p0 + j;
        ++slot;
      }
    }
  }
  if (tid == 0) {
    a.info[0] = A;
    a.info[1] = count;
    a.info[2] = E;
    a.info[3] = L.newly;
    a.info[4] = n - M;
    a.info[5] = L.walked;
    a.info[6] = 0;
    a.info[7] = 0;
    *a.status = L.bad;
  }
}

}  // namespace rudp
