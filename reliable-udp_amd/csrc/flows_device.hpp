// The device functions of rudp_accept_flows (flows.hip states the steps): one
// workgroup groups a batch of at most 1024 datagrams by flow in LDS and judges
// every flow's run by rudp_accept_inorder's rule, the runs side by side.  The
// classes and the step of the one-scan form are accept_device.hpp's; the join
// here is that file's made segmented.
#pragma once
#include "accept_device.hpp"

namespace RUDP_NS {

constexpr uint32_t kFlowFpt = 4;                    // consecutive sorted positions per thread
constexpr uint32_t kFlowMax = kBlock * kFlowFpt;    // 1024 == RUDP_FLOWS_MAX_BATCH
constexpr uint32_t kFlowNil = 0xFFFFu;              // no position
constexpr uint32_t kFlowNoEvent = 0xFFFFFFFFu;

// AccP with a head flag: h = a run head lies in the span, whose state then does
// not depend on anything before the span.
struct FlowP {
  uint64_t m;  // prefix maximum of seq + c since the last reset or the run's head (the head: the row's expect)
  uint32_t r;  // 1 + sorted position of the run's last reset, 0: none
  uint32_t h;
};
__device__ __forceinline__ FlowP flow_join(FlowP a, FlowP b) {
  if (b.h) return b;
  if (b.r) return FlowP{b.m, b.r, a.h};
  return FlowP{a.m > b.m ? a.m : b.m, a.r, a.h};
}
__device__ __forceinline__ FlowP flow_step(FlowP s, uint32_t cls, uint32_t p, uint32_t seq, uint32_t c) {
  const uint64_t v = (uint64_t)seq + c;
  if (cls == kAccReset) return FlowP{v, p + 1u, s.h};
  if (cls == kAccData && v > s.m) s.m = v;
  return s;
}

struct FlowLds {
  uint64_t key[kFlowMax];        // step 2: slot << 10 | arrival index, sorted; from step 4: m after position p
  uint64_t rex[kFlowMax];        // run: the row's expect; from step 5 the run's expect after its last judged datagram
  uint32_t ch[kFlowMax];         // by arrival index, as seq, fl and us
  uint32_t rslot[kFlowMax];      // run: its slot
  uint32_t rlast[kFlowMax];      // run: last_isn (above 65535: none)
  uint32_t ev[kFlowMax];         // run: its first event, position << 1 | (1: an accepted FIN, 0: an anomaly)
  uint32_t rbase[kFlowMax + 1];  // run: kept | accepted << 16 datagrams of the runs before it; [A]: the totals
  uint16_t seq[kFlowMax];
  uint16_t gi[kFlowMax];         // position -> arrival index
  uint16_t run[kFlowMax];        // position -> run
  uint16_t ack[kFlowMax];        // by position, as pr, acc and rep
  uint16_t pr[kFlowMax];         // r after position p
  uint16_t rstart[kFlowMax + 2]; // run: its first position; [A]: the first flowless position
  uint16_t fr[kFlowMax];         // run: 1 + position of the last reset at or before its end, 0: none
  uint16_t fend[kFlowMax];       // run: the position that ended it, kFlowNil: none
  uint8_t fl[kFlowMax];
  uint8_t us[kFlowMax];          // usable and of a valid flow
  uint8_t acc[kFlowMax];
  uint8_t rep[kFlowMax];
  uint8_t rlive[kFlowMax];       // run: the row's live; from step 5 live after its last judged datagram
  uint64_t wm[kBlock / 64];
  uint32_t wr[kBlock / 64], wh[kBlock / 64], sw[kBlock / 64];
  uint32_t bad, ended, walked;
};

// Exclusive scan of one FlowP per thread under flow_join (all threads call it).
__device__ inline FlowP flow_block_exclusive_join(FlowP x, FlowLds& L) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  FlowP incl = x;
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const FlowP y{__shfl_up(incl.m, d, 64), __shfl_up(incl.r, d, 64), __shfl_up(incl.h, d, 64)};
    if (lane >= d) incl = flow_join(y, incl);
  }
  if (lane == 63) {
    L.wm[wave] = incl.m;
    L.wr[wave] = incl.r;
    L.wh[wave] = incl.h;
  }
  FlowP ex{__shfl_up(incl.m, 1, 64), __shfl_up(incl.r, 1, 64), __shfl_up(incl.h, 1, 64)};
  if (lane == 0) ex = FlowP{0, 0, 0};
  __syncthreads();
  FlowP before{0, 0, 0};
  for (uint32_t w = 0; w < nwaves; ++w)
    if (w < wave) before = flow_join(before, FlowP{L.wm[w], L.wr[w], L.wh[w]});
  __syncthreads();  // wm / wr / wh may be reused
  return flow_join(before, ex);
}

// Step 1 is split off from the rest, so that a caller whose tables are already
// in registers (the fused rudp_receive_flows: receive_flows.hip) fills the LDS
// tables itself: flows_reset (a barrier follows, before the first flows_put;
// it returns the padded batch size of the sort), flows_put / flows_pad per
// datagram, and flows_load, the loop over global memory.
__device__ __forceinline__ uint32_t flows_reset(FlowLds& L, uint32_t n) {
  uint32_t N2 = 2;
  while (N2 < n) N2 <<= 1;
  if (threadIdx.x == 0) {
    L.bad = 0;
    L.ended = 0;
    L.walked = 0;
  }
  return N2;
}

// 1. datagram k's entries of the tables and its key (k < n), or the padding key
__device__ __forceinline__ void flows_put(const FlowsArgs& a, FlowLds& L, uint32_t k, uint32_t seq, uint32_t fl,
                                          uint32_t ch, bool usable) {
  const uint32_t f = a.flow[k];
  const bool valid = (uint64_t)f < a.n_flows;  // (n_flows <= 2^32 - 2: RUDP_FLOW_NONE never is)
  if (!valid && f != RUDP_FLOW_NONE) L.bad = 1;
  L.seq[k] = (uint16_t)seq;
  L.fl[k] = (uint8_t)fl;
  L.ch[k] = ch;
  L.us[k] = (uint8_t)(valid && usable);
  L.key[k] = (uint64_t)(valid ? f : RUDP_FLOW_NONE) << 10 | k;
}
__device__ __forceinline__ void flows_pad(FlowLds& L, uint32_t k) { L.key[k] = ~0ull; }

// 1. the tables and the keys from global memory
__device__ __forceinline__ void flows_load(const FlowsArgs& a, FlowLds& L, uint32_t N2) {
  const uint32_t n = (uint32_t)a.n;
  for (uint32_t k = threadIdx.x; k < N2; k += kBlock) {
    if (k < n) flows_put(a, L, k, a.seq[k], a.flags[k], a.chars[k], a.usable ? a.usable[k] != 0 : true);
    else flows_pad(L, k);
  }
}

// Steps 2 to 7 on the tables and keys of step 1 (behind a barrier; 1 <= n <=
// kFlowMax, N2 from flows_reset).  status, when not null, gets the call's word.
__device__ inline void flows_judge_lds(const FlowsArgs& a, FlowLds& L, uint32_t N2, uint32_t* status) {
  const uint32_t tid = threadIdx.x, n = (uint32_t)a.n;

  // 2. sorted by slot, then by arrival; the flowless datagrams last
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

  // 3. run heads: A, the order, every run's slot and first position
  const uint32_t p0 = tid * kFlowFpt;
  uint32_t A, M;
  {
    uint32_t head[kFlowFpt], val[kFlowFpt], cnt = 0;
#pragma unroll
    for (uint32_t j = 0; j < kFlowFpt; ++j) {
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
    for (uint32_t j = 0; j < kFlowFpt; ++j) {
      const uint32_t p = p0 + j;
      if (p >= n) break;
      const uint32_t i = (uint32_t)L.key[p] & (kFlowMax - 1u);
      L.gi[p] = (uint16_t)i;
      a.order[p] = i;
      if (head[j]) {
        L.rstart[run] = (uint16_t)p;
        L.rslot[run] = (uint32_t)(L.key[p] >> 10);
        a.order_off[run] = p;
        ++run;
      }
      L.run[p] = val[j] ? (uint16_t)(run - 1u) : (uint16_t)kFlowNil;
    }
    if (tid == 0) {
      L.rstart[A] = (uint16_t)M;
      a.order_off[A] = M;
    }
  }
  __syncthreads();
  for (uint32_t r = tid; r < A; r += kBlock) {
    const uint64_t* row = a.states + 4ull * L.rslot[r];
    const uint64_t w3 = row[3];
    L.rex[r] = row[0];
    L.rlive[r] = (uint8_t)(row[2] != 0);
    L.rlast[r] = w3 == 0 || w3 - 1u > 0xFFFFull ? 0xFFFFFFFFu : (uint32_t)(w3 - 1u);
    L.ev[r] = kFlowNoEvent;
  }
  __syncthreads();

  // 4. every run judged under the guess (the keys are dead: key[p] <- m after p)
  {
    uint32_t cls[kFlowFpt];
    FlowP agg{0, 0, 0};
#pragma unroll
    for (uint32_t j = 0; j < kFlowFpt; ++j) {
      const uint32_t p = p0 + j;
      cls[j] = kAccSkip;
      if (p < M) {
        const uint32_t i = L.gi[p], r = L.run[p];
        cls[j] = acc_class(L.us[i], L.fl[i], L.seq[i], L.rlast[r]);
        if (L.rstart[r] == p) agg = FlowP{L.rex[r], 0, 1};
        agg = flow_step(agg, cls[j], p, L.seq[i], L.ch[i]);
      }
    }
    FlowP s = flow_block_exclusive_join(agg, L);
#pragma unroll
    for (uint32_t j = 0; j < kFlowFpt; ++j) {
      const uint32_t p = p0 + j;
      if (p >= M) break;
      const uint32_t i = L.gi[p], r = L.run[p];
      const uint32_t seq = L.seq[i], c = L.ch[i];
      const bool seed_live = L.rlive[r] != 0;
      if (L.rstart[r] == p) s = FlowP{L.rex[r], 0, 1};
      uint32_t acc = cls[j] == kAccReset;
      if (cls[j] == kAccData && (seed_live || s.r)) {
        if ((uint64_t)seq == s.m) acc = 1;
        else if ((uint64_t)seq + c > s.m) atomicMin(&L.ev[r], p << 1);
      }
      s = flow_step(s, cls[j], p, seq, c);
      const bool rep = cls[j] != kAccSkip && (seed_live || s.r);
      L.acc[p] = (uint8_t)acc;
      L.rep[p] = (uint8_t)rep;
      L.ack[p] = rep ? (uint16_t)s.m : (uint16_t)0;
      L.key[p] = s.m;
      L.pr[p] = (uint16_t)s.r;
      if (acc && (L.fl[i] & 0x20u)) atomicMin(&L.ev[r], p << 1 | 1u);
    }
  }
  __syncthreads();

  // 5. one lane per run: the state after its last judged datagram; a run whose
  // first event is an anomaly is walked by the rule from there
  for (uint32_t r = tid; r < A; r += kBlock) {
    const uint32_t start = L.rstart[r], stop = L.rstart[r + 1u], e = L.ev[r];
    const uint64_t expect0 = L.rex[r];
    const bool live0 = L.rlive[r] != 0;
    uint32_t endp = kFlowNil, lr;
    uint64_t expect;
    bool live;
    if (e == kFlowNoEvent || (e & 1u)) {
      const uint32_t g = e == kFlowNoEvent ? stop - 1u : e >> 1;
      lr = L.pr[g];
      live = live0 || lr;
      expect = live ? L.key[g] : expect0;
      if (e != kFlowNoEvent) endp = g;
    } else {
      const uint32_t pa = e >> 1, last = L.rlast[r];
      lr = pa == start ? 0u : L.pr[pa - 1u];
      live = live0 || lr;
      expect = live && pa != start ? L.key[pa - 1u] : expect0;
      for (uint32_t p = pa; p < stop; ++p) {
        const uint32_t i = L.gi[p], seq = L.seq[i], fl = L.fl[i], c = L.ch[i], us = L.us[i];
        uint32_t acc = 0;
        if (us) {
          if (fl & 0x80u) {
            if (seq != last) {
              expect = (uint64_t)seq + c;
              live = true;
              lr = p + 1u;
              acc = 1;
            }
          } else if (live && (uint64_t)seq == expect) {
            expect += c;
            acc = 1;
          }
        }
        L.acc[p] = (uint8_t)acc;
        L.ack[p] = us && live ? (uint16_t)expect : (uint16_t)0;
        if (acc && (fl & 0x20u)) {
          endp = p;
          break;
        }
      }
      atomicAdd(&L.walked, 1u);
    }
    L.fr[r] = (uint16_t)lr;
    L.fend[r] = (uint16_t)endp;
    L.rex[r] = expect;
    L.rlive[r] = (uint8_t)live;
    if (endp != kFlowNil) atomicAdd(&L.ended, 1u);
  }
  __syncthreads();

  // 6. keep, the ranks (an exclusive count of the kept datagrams in sorted
  // order is the flow-major message order), the per-datagram outputs
  uint64_t totals;
  {
    uint32_t acc[kFlowFpt], keep[kFlowFpt], rep[kFlowFpt], ack[kFlowFpt];
    uint64_t x = 0;
#pragma unroll
    for (uint32_t j = 0; j < kFlowFpt; ++j) {
      const uint32_t p = p0 + j;
      acc[j] = keep[j] = rep[j] = ack[j] = 0;
      if (p < M) {
        const uint32_t r = L.run[p], lr = L.fr[r];
        if (p <= L.fend[r]) {  // (kFlowNil is above every position)
          acc[j] = L.acc[p];
          keep[j] = acc[j] && (lr == 0 || p + 1u >= lr);
          rep[j] = L.rep[p];
          ack[j] = L.ack[p];
        }
      }
      x += (uint64_t)keep[j] | (uint64_t)acc[j] << 16 | (uint64_t)rep[j] << 32;
    }
    uint64_t before = block_exclusive_scan(x, &totals, L.wm);
#pragma unroll
    for (uint32_t j = 0; j < kFlowFpt; ++j) {
      const uint32_t p = p0 + j;
      if (p >= n) break;
      const uint32_t i = L.gi[p];
      if (p < M && L.rstart[L.run[p]] == p) L.rbase[L.run[p]] = (uint32_t)before;  // kept | accepted << 16
      a.accept[i] = (uint8_t)acc[j];
      a.keep[i] = (uint8_t)keep[j];
      a.reply[i] = (uint8_t)rep[j];
      a.reply_ack[i] = (uint16_t)ack[j];
      a.rank[i] = keep[j] ? (uint32_t)before & 0xFFFFu : RUDP_RANK_NONE;
      before += (uint64_t)keep[j] | (uint64_t)acc[j] << 16 | (uint64_t)rep[j] << 32;
    }
    if (tid == 0) L.rbase[A] = (uint32_t)totals;
  }
  __syncthreads();

  // 7. the rows and the per-flow info
  for (uint32_t r = tid; r < A; r += kBlock) {
    uint64_t* row = a.states + 4ull * L.rslot[r];
    uint64_t* fi = a.flow_info + 8ull * r;
    const uint32_t lr = L.fr[r], endp = L.fend[r], b0 = L.rbase[r], b1 = L.rbase[r + 1u];
    const uint64_t isn = lr ? (uint64_t)L.seq[L.gi[lr - 1u]] : row[1];
    const uint64_t expect = L.rex[r], live = L.rlive[r];
    fi[0] = L.rslot[r];
    fi[1] = endp != kFlowNil ? (uint64_t)L.gi[endp] : (uint64_t)n;
    fi[2] = (b1 >> 16) - (b0 >> 16);
    fi[3] = lr ? (uint64_t)L.gi[lr - 1u] : (uint64_t)n;
    fi[4] = live ? expect - isn : 0ull;
    fi[5] = isn;
    fi[6] = (b1 & 0xFFFFu) - (b0 & 0xFFFFu);
    fi[7] = b0 & 0xFFFFu;
    if (endp != kFlowNil) {  // the flow turns over: closed until a SYN other than this ISN's
      row[0] = 0;
      row[1] = 0;
      row[2] = 0;
      row[3] = isn + 1u;
    } else {
      row[0] = expect;
      row[1] = isn;
      row[2] = live;
    }
  }
  if (tid == 0) {
    a.info[0] = A;
    a.info[1] = totals & 0xFFFFu;
    a.info[2] = (totals >> 32) & 0xFFFFu;
    a.info[3] = L.ended;
    a.info[4] = n - M;
    a.info[5] = L.walked;
    a.info[6] = 0;
    a.info[7] = 0;
    if (status) *status = L.bad ? RUDP_ST_FLOW : 0u;
  }
}

// The whole call for one workgroup of kBlock threads (0 <= n <= kFlowMax).
__device__ inline void flows_judge(const FlowsArgs& a, FlowLds& L) {
  if (a.n == 0) {  // (uniform)
    if (threadIdx.x < 8) a.info[threadIdx.x] = 0;
    if (threadIdx.x == 0) *a.status = 0;
    return;
  }
  const uint32_t N2 = flows_reset(L, (uint32_t)a.n);
  __syncthreads();
  flows_load(a, L, N2);
  __syncthreads();
  flows_judge_lds(a, L, N2, a.status);
}

}  // namespace rudp
