
// The device functions of the reordering receiver's rule (window.hip states
// the steps): win_judge_chunk judges one chunk.  window.hip's kernel runs it on
// the caller's tables, receive_window.hip's fused kernel on the tables it has
// just written.
#pragma once
#include "codec_device.hpp"
#include "internal.hpp"
#include "scan_device.hpp"

namespace RUDP_NS {

constexpr uint32_t kWinBlock = 1024;
constexpr uint32_t kWinNew = 1024;     // new frames per chunk
constexpr uint32_t kWinItems = 2048;   // kWinNew + at most 1023 pending ones, padded to a power of two
constexpr uint32_t kWinNil = 0xFFFFu;
constexpr uint32_t kWinHdr = 16;       // scratch words before the pending indices
// scratch (u64): [0] expect [1] isn [2] live [3] end (n: none) [4] msg_start
// [5] ranked frames [6] delivered frames [7] first anomaly [8] pending frames;
// then the pending frames' indices, u32 [1024].
enum : uint32_t { kWinSkip = 0, kWinDupSyn = 1, kWinReset = 2, kWinData = 3 };

struct WinLds {
  uint64_t key[kWinItems];     // sorted: segment << 27 | seq << 11 | item
  uint32_t gi[kWinItems];      // the item's frame index
  uint32_t ch[kWinItems];
  uint32_t cD[kWinItems];      // chain element j: segment << 11 | delivery time (an item position)
  uint32_t rk[kWinItems];
  uint16_t seq[kWinItems];
  uint16_t seg[kWinItems];     // resets at or before the item
  uint16_t segpos[kWinItems + 1];  // the reset item of segment g >= 1
  uint16_t succ[kWinItems];    // sorted q: successor; after step 4 its chain index
  uint16_t cq[kWinItems];      // chain element j: its q
  uint16_t pos2q[kWinItems];
  uint16_t ack[kWinItems];
  uint16_t ring[1024];
  uint8_t fl[kWinItems];
  uint8_t cls[kWinItems];
  uint8_t mark[kWinItems];
  uint8_t st[kWinItems];       // 0 rejected, 1 delivered, 2 pending
  uint8_t rep[kWinItems];
  uint8_t pend[kWinItems];     // a first arrival that was ahead inside the window
  uint32_t sw[kWinBlock / 64];
  uint32_t pe, pa;             // the item that ended the transfer, the first anomaly (M: none)
  // what the walk leaves
  uint64_t wE, wisn, wms, wrb, wdc;
  uint32_t wpe;
};

struct WinState {
  uint64_t E, isn, live, ms, rb, dc, first;
};

__device__ __forceinline__ uint32_t win_lower_bound64(const uint64_t* a, uint32_t n, uint64_t v) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t m = (lo + hi) >> 1;
    if (a[m] < v) lo = m + 1u; else hi = m;
  }
  return lo;
}
__device__ __forceinline__ uint32_t win_lower_bound32(const uint32_t* a, uint32_t n, uint32_t v) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t m = (lo + hi) >> 1;
    if (a[m] < v) lo = m + 1u; else hi = m;
  }
  return lo;
}

// The candidate that starts at t in segment g: its q, or kWinNil.
__device__ __forceinline__ uint32_t win_find(const WinLds& L, uint32_t Nc, uint32_t g, uint64_t t) {
  if (t > 65535u) return kWinNil;
  const uint64_t want = (uint64_t)g << 27 | t << 11;
  const uint32_t lb = win_lower_bound64(L.key, Nc, want);
  return lb < Nc && (L.key[lb] >> 11) == (want >> 11) ? lb : kWinNil;
}

__device__ __forceinline__ uint64_t win_E0(const WinLds& L, uint32_t g, uint64_t E) {
  if (g == 0) return E;
  const uint32_t p = L.segpos[g];
  return (uint64_t)L.seq[p] + L.ch[p];
}

// expect before (after = 0) or after item p under the guess; *cnt: the chain
// elements delivered before / by p, those of earlier segments included.
__device__ __forceinline__ uint64_t win_guess(const WinLds& L, uint32_t Nch, uint32_t p, uint32_t after, uint64_t E,
                                              uint32_t* cnt) {
  const uint32_t g = L.seg[p];
  const uint32_t c = win_lower_bound32(L.cD, Nch, (g << 11 | p) + after);
  *cnt = c;
  if (c && (L.cD[c - 1u] >> 11) == g) {
    const uint32_t ip = (uint32_t)L.key[L.cq[c - 1u]] & 2047u;
    return (uint64_t)L.seq[ip] + L.ch[ip];
  }
  return win_E0(L, g, E);
}

__device__ __forceinline__ void win_write_final(const WindowArgs& a, const WinState& s, uint64_t end, uint64_t npend) {
  a.state_out[0] = s.E;
  a.state_out[1] = s.isn;
  a.state_out[2] = s.live;
  a.state_out[3] = 0;
  a.info[0] = end;
  a.info[1] = s.rb;
  a.info[2] = s.ms;
  a.info[3] = s.live ? s.E - s.isn : 0ull;
  a.info[4] = s.first;
  a.info[5] = npend;
  a.info[6] = s.dc;
  a.info[7] = 0;
}

// One chunk judged by the workgroup (all kWinBlock threads call it): steps 1-8
// above on a.seq, a.flags, a.chars and a.usable.  receive_window.hip's fused
// kernel calls it too, on the tables it has just written (behind a barrier).
__device__ __forceinline__ void win_judge_chunk(const WindowArgs& a, WinLds& L) {
  const uint32_t tid = threadIdx.x;
  const bool last_chunk = a.chunk + 1u == a.chunks;
  WinState s;
  uint32_t ncar;
  if (a.chunk == 0) {
    s = WinState{a.state_in[0], a.state_in[1], a.state_in[2] ? 1ull : 0ull, a.n, 0, 0, a.n};
    ncar = (uint32_t)a.n_carried;
  } else {
    s = WinState{a.hdr[0], a.hdr[1], a.hdr[2], a.hdr[4], a.hdr[5], a.hdr[6], a.hdr[7]};
    ncar = (uint32_t)a.hdr[8];
    if (a.hdr[3] != a.n) {  // (uniform) the transfer ended in an earlier chunk
      if (last_chunk && tid == 0) win_write_final(a, s, a.hdr[3], 0);
      return;
    }
  }
  const uint32_t* car = reinterpret_cast<const uint32_t*>(a.hdr + kWinHdr);
  uint32_t* car_out = reinterpret_cast<uint32_t*>(a.hdr + kWinHdr);
  const uint64_t new0 = a.n_carried + (uint64_t)a.chunk * kWinNew;
  const uint32_t nnew = a.n - new0 < kWinNew ? (uint32_t)(a.n - new0) : kWinNew;
  const uint32_t M = ncar + nnew;  // (<= 2047)
  const uint32_t Wc = a.Wc;
  uint32_t N2 = 2;
  while (N2 < M) N2 <<= 1;

  // 1. items, classes, segments
  for (uint32_t p = tid; p < kWinItems; p += kWinBlock) {
    uint32_t cls = kWinSkip;
    if (p < M) {
      const uint32_t i = p < ncar ? (a.chunk == 0 ? p : car[p]) : (uint32_t)new0 + (p - ncar);
      const uint32_t seq = a.seq[i], fl = a.flags[i];
      const uint32_t us = a.usable ? (uint32_t)(a.usable[i] != 0) : 1u;
      L.gi[p] = i;
      L.seq[p] = (uint16_t)seq;
      L.fl[p] = (uint8_t)fl;
      L.ch[p] = a.chars[i];
      if (us) cls = (fl & 0x80u) ? (seq == a.last_isn ? kWinDupSyn : kWinReset) : kWinData;
    }
    L.cls[p] = (uint8_t)cls;
    L.pos2q[p] = (uint16_t)kWinNil;
    L.st[p] = 0;
    L.pend[p] = 0;
    L.rep[p] = 0;
    L.ack[p] = 0;
    L.rk[p] = RUDP_RANK_NONE;
  }
  if (tid == 0) {
    L.pe = M;
    L.pa = M;
  }
  __syncthreads();
  uint32_t nseg;
  {
    const uint32_t r0 = L.cls[2u * tid] == kWinReset, r1 = L.cls[2u * tid + 1u] == kWinReset;
    const uint32_t ex = block_exclusive_scan32(r0 + r1, &nseg, L.sw);
    L.seg[2u * tid] = (uint16_t)(ex + r0);
    L.seg[2u * tid + 1u] = (uint16_t)(ex + r0 + r1);
    if (r0) L.segpos[ex + r0] = (uint16_t)(2u * tid);
    if (r1) L.segpos[ex + r0 + r1] = (uint16_t)(2u * tid + 1u);
  }
  __syncthreads();

  // 2. the candidates, sorted
  for (uint32_t p = tid; p < N2; p += kWinBlock) {
    uint64_t key = ~0ull;
    if (p < M && L.cls[p] == kWinData && L.ch[p] > 0) {
      const uint32_t g = L.seg[p];
      if ((g || s.live) && (uint64_t)L.seq[p] >= win_E0(L, g, s.E)) key = (uint64_t)g << 27 | (uint64_t)L.seq[p] << 11 | p;
    }
    L.key[p] = key;
  }
  __syncthreads();
  for (uint32_t k = 2; k <= N2; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      if (tid < (N2 >> 1)) {
        const uint32_t lo = ((tid & ~(j - 1u)) << 1) | (tid & (j - 1u)), hi = lo | j;
        const uint64_t x = L.key[lo], y = L.key[hi];
        if ((x > y) == ((lo & k) == 0u)) {
          L.key[lo] = y;
          L.key[hi] = x;
        }
      }
      __syncthreads();
    }
  }
  const uint32_t Nc = win_lower_bound64(L.key, N2, ~0ull);

  // 3. nodes, successors, chains
  for (uint32_t q = tid; q < Nc; q += kWinBlock) {
    const uint64_t key = L.key[q];
    const uint32_t p = (uint32_t)key & 2047u;
    L.pos2q[p] = (uint16_t)q;
    const bool node = q == 0 || (L.key[q - 1u] >> 11) != (key >> 11);
    uint32_t nx = kWinNil;
    if (node && !(L.fl[p] & 0x20u)) nx = win_find(L, Nc, (uint32_t)(key >> 27), (uint64_t)L.seq[p] + L.ch[p]);
    L.succ[q] = (uint16_t)nx;
    L.mark[q] = 0;
    // (whether q is a node is read again from the keys)
  }
  __syncthreads();
  for (uint32_t g = tid; g <= nseg; g += kWinBlock) {
    if (g || s.live) {
      const uint32_t r = win_find(L, Nc, g, win_E0(L, g, s.E));
      if (r != kWinNil) L.mark[r] = 1;
    }
  }
  __syncthreads();
  for (uint32_t reach = 1; reach < Nc; reach <<= 1) {  // (uniform)
    uint32_t nx[2];
#pragma unroll
    for (uint32_t u = 0; u < 2; ++u) {
      const uint32_t q = tid + u * kWinBlock;
      nx[u] = kWinNil;
      if (q < Nc) {
        const uint32_t sq = L.succ[q];
        if (sq != kWinNil) {
          if (L.mark[q]) L.mark[sq] = 1;  // (a mark seen early only marks further along the same chain)
          nx[u] = L.succ[sq];
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t u = 0; u < 2; ++u)
      if (tid + u * kWinBlock < Nc) L.succ[tid + u * kWinBlock] = (uint16_t)nx[u];
    __syncthreads();
  }

  // 4. the chain elements in order and their delivery times
  uint32_t Nch;
  {
    const uint32_t q0 = 2u * tid, q1 = q0 + 1u;
    const uint32_t m0 = q0 < Nc && L.mark[q0], m1 = q1 < Nc && L.mark[q1];
    const uint32_t v0 = m0 ? (uint32_t)(L.key[q0] >> 27) << 11 | ((uint32_t)L.key[q0] & 2047u) : 0u;
    const uint32_t v1 = m1 ? (uint32_t)(L.key[q1] >> 27) << 11 | ((uint32_t)L.key[q1] & 2047u) : 0u;
    uint32_t j = block_exclusive_scan32(m0 + m1, &Nch, L.sw);
    uint32_t run = block_exclusive_max(v0 > v1 ? v0 : v1, L.sw);
    if (m0) {
      run = v0 > run ? v0 : run;
      L.cq[j] = (uint16_t)q0;
      L.cD[j] = run;
      L.succ[q0] = (uint16_t)j;
      ++j;
    }
    if (m1) {
      run = v1 > run ? v1 : run;
      L.cq[j] = (uint16_t)q1;
      L.cD[j] = run;
      L.succ[q1] = (uint16_t)j;
    }
  }
  __syncthreads();

  // 5. every item under the guess
  for (uint32_t p = tid; p < M; p += kWinBlock) {
    const uint32_t cls = L.cls[p], g = L.seg[p];
    const bool lv = g || s.live;
    uint32_t cb, ca;
    const uint64_t Gb = win_guess(L, Nch, p, 0, s.E, &cb);
    const uint64_t Ga = win_guess(L, Nch, p, 1, s.E, &ca);
    if (cls == kWinReset) {
      L.st[p] = 1;
      L.rk[p] = 0;
      if (L.fl[p] & 0x20u) atomicMin(&L.pe, p);
    } else if (cls == kWinData && lv) {
      const uint64_t sq = L.seq[p];
      const uint32_t c = L.ch[p];
      if ((sq == Gb && c == 0) || (c > 0 && sq >= Gb + Wc)) atomicMin(&L.pa, p);
      const uint32_t q = L.pos2q[p];
      if (q != kWinNil) {
        const bool node = q == 0 || (L.key[q - 1u] >> 11) != (L.key[q] >> 11);
        const bool pend = node && Gb < sq && sq < Gb + Wc;
        L.pend[p] = (uint8_t)pend;
        if (L.mark[q]) {
          const uint32_t j = L.succ[q];
          L.st[p] = 1;
          L.rk[p] = (uint32_t)(g ? 1ull : s.rb) + j - win_lower_bound32(L.cD, Nch, g << 11);
          if (L.fl[p] & 0x20u) atomicMin(&L.pe, L.cD[j] & 2047u);
        } else if (pend) {
          L.st[p] = 2;
        }
      }
    }
    if (cls != kWinSkip && lv && p >= ncar) {
      L.rep[p] = 1;
      L.ack[p] = (uint16_t)Ga;
    }
  }
  __syncthreads();
  uint32_t pe = L.pe;
  const uint32_t pa = L.pa;
  const bool slow = pa < pe;  // (uniform)
  if (slow) {
    // 7. the exact state before pa, the pending set into the ring, the walk
    const uint32_t g = L.seg[pa];
    uint32_t cnt;
    const uint64_t Eb = win_guess(L, Nch, pa, 0, s.E, &cnt);
    for (uint32_t w = tid; w < Wc; w += kWinBlock) L.ring[w] = (uint16_t)kWinNil;
    __syncthreads();
    for (uint32_t p = tid; p < pa; p += kWinBlock) {
      if (L.cls[p] == kWinReset) continue;
      const uint32_t q = L.pos2q[p];
      if (q != kWinNil && L.mark[q] && (L.cD[L.succ[q]] & 2047u) < pa) continue;
      uint32_t st = 0;
      if (L.pend[p] && L.seg[p] == g && (uint64_t)L.seq[p] > Eb) {
        st = 2;
        L.ring[L.seq[p] % Wc] = (uint16_t)p;
      }
      L.st[p] = (uint8_t)st;
      L.rk[p] = RUDP_RANK_NONE;
    }
    __syncthreads();
    if (tid == 0) {
      uint64_t E = Eb, isn = s.isn, ms = s.ms, live = 1;
      uint64_t r = (g ? 1ull : s.rb) + cnt - win_lower_bound32(L.cD, Nch, g << 11);
      uint64_t dc = s.dc + g + cnt;
      if (g) {
        isn = L.seq[L.segpos[g]];
        ms = L.gi[L.segpos[g]];
      }
      uint32_t wpe = M;
      // every pending frame with a start in (from, to) leaves the set
      auto advance = [&](uint64_t from, uint64_t to) {
        const uint64_t stop = to < from + Wc ? to : from + Wc;
        for (uint64_t v = from + 1u; v < stop; ++v) {
          const uint32_t w = (uint32_t)(v % Wc);
          if (L.ring[w] != kWinNil) {
            L.st[L.ring[w]] = 0;
            L.ring[w] = (uint16_t)kWinNil;
          }
        }
      };
      auto clear = [&]() {
        for (uint32_t w = 0; w < Wc; ++w)
          if (L.ring[w] != kWinNil) {
            L.st[L.ring[w]] = 0;
            L.ring[w] = (uint16_t)kWinNil;
          }
      };
      for (uint32_t p = pa; p < M; ++p) {
        const uint32_t cls = L.cls[p];
        L.st[p] = 0;
        L.rk[p] = RUDP_RANK_NONE;
        L.rep[p] = 0;
        L.ack[p] = 0;
        if (cls == kWinSkip) continue;
        const uint64_t sq = L.seq[p];
        const uint32_t fl = L.fl[p], c = L.ch[p];
        bool fin = false;
        if (cls == kWinReset) {
          isn = sq;
          E = sq + c;
          live = 1;
          ms = L.gi[p];
          clear();
          L.st[p] = 1;
          L.rk[p] = 0;
          r = 1;
          ++dc;
          fin = (fl & 0x20u) != 0;
        } else if (cls == kWinData && live) {
          if (sq == E) {
            L.st[p] = 1;
            L.rk[p] = (uint32_t)r++;
            ++dc;
            fin = (fl & 0x20u) != 0;
            if (c) {
              advance(E, E + c);
              E += c;
              while (!fin && L.ring[E % Wc] != kWinNil) {
                const uint32_t j = L.ring[E % Wc];
                L.ring[E % Wc] = (uint16_t)kWinNil;
                L.st[j] = 1;
                L.rk[j] = (uint32_t)r++;
                ++dc;
                fin = (L.fl[j] & 0x20u) != 0;
                advance(E, E + L.ch[j]);
                E += L.ch[j];
              }
            }
          } else if (E < sq && sq < E + Wc && c > 0 && L.ring[sq % Wc] == kWinNil) {
            L.ring[sq % Wc] = (uint16_t)p;
            L.st[p] = 2;
          }
        }
        if (live && p >= ncar) {
          L.rep[p] = 1;
          L.ack[p] = (uint16_t)E;
        }
        if (fin) {
          wpe = p;
          clear();
          break;
        }
      }
      L.wE = E;
      L.wisn = isn;
      L.wms = ms;
      L.wrb = r;
      L.wdc = dc;
      L.wpe = wpe;
    }
    __syncthreads();
    s.E = L.wE;
    s.isn = L.wisn;
    s.live = 1;
    s.ms = L.wms;
    s.rb = L.wrb;
    s.dc = L.wdc;
    pe = L.wpe;
    if ((uint64_t)L.gi[pa] < s.first) s.first = L.gi[pa];
  } else if (M) {
    // 6. the guess was exact: the state after the last judged item
    const uint32_t pl = pe < M ? pe : M - 1u;
    const uint32_t g = L.seg[pl];
    uint32_t cnt;
    const uint64_t En = win_guess(L, Nch, pl, 1, s.E, &cnt);
    if (g || s.live) s.E = En;
    s.rb = (g ? 1ull : s.rb) + cnt - win_lower_bound32(L.cD, Nch, g << 11);
    s.dc += g + cnt;
    if (g) {
      s.isn = L.seq[L.segpos[g]];
      s.ms = L.gi[L.segpos[g]];
      s.live = 1;
    }
    // what is still pending: ahead of the final expect in the last segment, with no end
    for (uint32_t p = tid; p < M; p += kWinBlock)
      if (L.st[p] == 2 && !(pe == M && L.seg[p] == g && (uint64_t)L.seq[p] > s.E)) L.st[p] = 0;
    __syncthreads();
  }

  // 8. outputs (two consecutive items per thread: the pending ones keep their order)
  uint32_t npend;
  {
    const uint32_t p0 = 2u * tid;
    uint32_t pd[2];
#pragma unroll
    for (uint32_t u = 0; u < 2; ++u) pd[u] = p0 + u < M && p0 + u <= pe && L.st[p0 + u] == 2;
    uint32_t k = block_exclusive_scan32(pd[0] + pd[1], &npend, L.sw);
#pragma unroll
    for (uint32_t u = 0; u < 2; ++u) {
      const uint32_t p = p0 + u;
      if (p >= M) break;
      const uint32_t i = L.gi[p];
      const bool judged = p <= pe;
      const uint32_t st = judged ? L.st[p] : 0u;
      a.accept[i] = (uint8_t)st;
      a.rank[i] = st == 1 && !(s.ms < a.n && i < s.ms) ? L.rk[p] : RUDP_RANK_NONE;
      a.carry_rank[i] = pd[u] && last_chunk ? k : RUDP_RANK_NONE;
      if (p >= ncar || a.chunk == 0) {
        a.reply[i] = judged ? L.rep[p] : (uint8_t)0;
        a.reply_ack[i] = judged ? L.ack[p] : (uint16_t)0;
      }
      if (pd[u]) {
        if (k < kWinNew - 1u) car_out[k] = i;  // (distinct starts inside the window: never more)
        ++k;
      }
    }
  }
  if (tid == 0) {
    const uint64_t end = pe < M ? (uint64_t)L.gi[pe] : a.n;
    a.hdr[0] = s.E;
    a.hdr[1] = s.isn;
    a.hdr[2] = s.live;
    a.hdr[3] = end;
    a.hdr[4] = s.ms;
    a.hdr[5] = s.rb;
    a.hdr[6] = s.dc;
    a.hdr[7] = s.first;
    a.hdr[8] = npend < kWinNew - 1u ? npend : kWinNew - 1u;
    if (last_chunk) win_write_final(a, s, end, npend);
  }
}

}  // namespace rudp
