// rudp_receive_window: the reordering receiver in one call -- rudp_receive for
// a windowed sender.  The frames the call before left pending (source 0) and
// the new datagrams (source 1) stay two buffers, each with its own offsets and
// its own limit for the offset rule; item i < n_carried is carried frame i,
// else new frame i - n_carried.  Decode + strict UTF-8, usable, characters,
// the window's rule (window.hip), the message in delivery order, the pending
// frames whole for the next call, and the reply datagrams.
//
// Two forms behind the one entry point (capi.hip chooses):
//
//   fused    at most kWinNew new frames (one chunk of window.hip: at most 2047
//            items) in at most kRwFusedBytes of both buffers and
//            kRwFusedMeanFrame bytes per item: one workgroup of 1024 threads,
//            one launch.
//              1. both buffers into LDS once, as two sub-images: each read
//                 with aligned 16-B guarded loads from the boundary at or below
//                 its pointer, the second starting on the next 16-B boundary
//                 of the image; per item its start and end in the image
//                 (kImgBadOff: rejected by its source's offset rule);
//              2. one lane per item (at most two per thread): header, RFC 1071
//                 sum, UTF-8 verdict, lead bytes (image_decode_frame of
//                 frame_image_device.hpp, as receive.hip's fused kernel);
//                 the decode tables, usable and chars;
//              3. the chunk judged by win_judge_chunk (window_device.hpp) on the tables just
//                 written (behind a barrier), anomaly walk included;
//              4. the frame of every rank and of every carry rank (two LDS
//                 source tables), and two scans of their lengths in rank order
//                 (the message without the header, the pending frames whole);
//              5. both gathers out of the image as 16-B chunks of the output's
//                 own alignment (image_copy_ranked with a rank -> item
//                 indirection: no store covers a byte outside [0, total));
//              6. the replies, two consecutive items per thread, the last
//                 reset counted from n_carried on;
//              7. carry_csum, info[8..11] and status.
//   chained  everything else: a join of the two sources into one packed view
//            in a temporary (every good item's bytes back to back, a rejected
//            item empty; lengths summed over blocks of 1024 items, the block
//            bases, the offsets, then the copy by 16-B chunks of the view),
//            the existing launches on that view (decode + UTF-8, usable,
//            payload_chars, the window's rule, gather_ordered twice, the reply
//            builder with its resets counted from n_carried on), and one pass
//            that gives the rejected items their tables, gathers carry_csum
//            and completes info and status.
#include "frame_image_device.hpp"
#include "window_device.hpp"

namespace RUDP_NS {

// The fused form's byte limit (both buffers together): the image, the item
// tables and the rank tables fit beside WinLds in the 160 KiB a workgroup can
// declare.
constexpr uint32_t kRwFusedBytes = 32768;
// and its mean frame length: an item is decoded by one lane, so long frames
// serialise the workgroup.  1005 B is the largest measured mean, and the fused
// form still beat the chained one there in every round (32 x 1005 B: 47 against
// 83 us; 125 x 261 B: 37 against 85; profiles/r13/receive_window.json).  Longer
// means are not measured and chain.
constexpr uint32_t kRwFusedMeanFrame = 1005;
constexpr uint32_t kRwCarryMax = kWinNew - 1u;  // pending frames a call can leave (distinct starts inside the window)

// Item i's source, its index there, and whether its offsets pass that
// source's rule; *o0, *o1 its offsets.
__device__ __forceinline__ bool rw_item(const RecvWindowArgs& a, uint64_t i, uint32_t* s, uint64_t* o0, uint64_t* o1) {
  *s = i < a.w.n_carried ? 0u : 1u;
  const uint64_t k = *s ? i - a.w.n_carried : i;
  *o0 = a.off[*s][k];
  *o1 = a.off[*s][k + 1u];
  return *o0 <= *o1 && *o1 <= a.bytes[*s];
}

// ------------------------------------------------------------------ fused form

struct RwLds {
  WinLds win;
  uint32_t is[kWinItems], ie[kWinItems];  // every item's start and end in the image (kImgBadOff: rejected)
  uint32_t mo[kWinItems + 1];             // message offsets in rank order
  uint32_t co[kWinNew + 1];               // the pending frames' offsets in carry-rank order
  uint16_t msrc[kWinItems];               // the item of every rank (kWinNil: none)
  uint16_t csrc[kWinNew];                 // the item of every carry rank
  uint32_t sw32[kWinBlock / 64];
  uint32_t bad;                           // an item failed the offset rule
  // the two aligned sub-images, and window16_dw's reach past them
  __attribute__((aligned(16))) uint32_t img[(kRwFusedBytes + 4u * 16u + 32u) / 4u];
};
static_assert(sizeof(RwLds) <= 160 * 1024, "the fused receive_window's LDS exceeds a gfx950 workgroup's 160 KiB");

// Ranks 2 tid and 2 tid + 1 of K: their lengths (past `skip`) scanned into
// po[0..K], the offsets and, when not null, the sources written out.
__device__ inline uint32_t rw_rank_offsets(const RwLds& S, const uint16_t* src, uint32_t K, uint32_t skip,
                                           uint32_t* po, uint32_t* sw32, uint64_t* out_off, uint32_t* out_src) {
  const uint32_t tid = threadIdx.x;
  uint32_t len[2];
#pragma unroll
  for (uint32_t u = 0; u < 2; ++u) {
    const uint32_t k = 2u * tid + u;
    len[u] = 0;
    if (k < K) {
      const uint32_t p = src[k];
      if (p != kWinNil && S.is[p] != kImgBadOff) {
        const uint32_t F = S.ie[p] - S.is[p];
        len[u] = F > skip ? F - skip : 0u;
      }
      if (out_src) out_src[k] = p != kWinNil ? p : RUDP_RANK_NONE;
    }
  }
  uint32_t total = 0;
  uint32_t run = block_exclusive_scan32(len[0] + len[1], &total, sw32);
#pragma unroll
  for (uint32_t u = 0; u < 2; ++u) {
    const uint32_t k = 2u * tid + u;
    if (k < K) {
      po[k] = run;
      out_off[k] = run;
      run += len[u];
    }
  }
  if (tid == 0) {
    po[K] = total;
    out_off[K] = total;
  }
  return total;
}

template <int H>
__global__ void __launch_bounds__(kWinBlock) receive_window_fused_kernel(RecvWindowArgs a) {
  __shared__ RwLds S;
  const uint32_t tid = threadIdx.x;
  const uint32_t n = (uint32_t)a.w.n, nc = (uint32_t)a.w.n_carried;  // (n <= 2047)

  // 1. both buffers into LDS once, and every item's place in the image
  if (n) {  // (uniform)
    uint32_t ib[2], nv[2];
#pragma unroll
    for (uint32_t s = 0; s < 2; ++s) {
      ib[s] = a.bytes[s] ? (uint32_t)(a.mis[s] + a.bytes[s]) : 0u;
      nv[s] = (ib[s] + 15u) >> 4;
    }
    u32x4* dst = reinterpret_cast<u32x4*>(S.img);
    for (uint32_t v = tid; v < nv[0] + nv[1]; v += kWinBlock) {
      const uint32_t s = v < nv[0] ? 0u : 1u, w = s ? v - nv[0] : v;
      dst[v] = load16_guarded(a.src[s], 16ull * w, ib[s]);
    }
    uint32_t any_bad = 0;
    for (uint32_t p = tid; p < n; p += kWinBlock) {
      uint32_t s;
      uint64_t o0, o1;
      if (rw_item(a, p, &s, &o0, &o1)) {
        const uint32_t base = (s ? 16u * nv[0] : 0u) + (uint32_t)a.mis[s];
        S.is[p] = base + (uint32_t)o0;
        S.ie[p] = base + (uint32_t)o1;
      } else {
        S.is[p] = S.ie[p] = kImgBadOff;
        any_bad = 1;
      }
    }
    if (tid == 0) S.bad = 0;
    __syncthreads();
    if (any_bad) atomicOr(&S.bad, 1u);

    // 2. every item by one lane: the decode's outputs, usable and chars
#pragma unroll 1
    for (uint32_t q = tid; q < n; q += kWinBlock) {
      const FrameDecode d = image_decode_frame<H, true>(S.img, S.is[q], S.ie[q], a.csum[1] != nullptr, [&] {
        return (uint32_t)(q < nc ? a.csum[0][q] : a.csum[1][q - nc]);
      });
      const uint32_t us = (d.ok == RUDP_OK_GOOD || d.ok == RUDP_OK_UNVERIFIED) && d.valid == 1u;
      a.seq[q] = (uint16_t)d.seq;
      a.ack[q] = (uint16_t)d.ack;
      a.flags[q] = (uint8_t)d.fl;
      a.ok[q] = (uint8_t)d.ok;
      if (a.csum_out) a.csum_out[q] = (uint16_t)d.cs;
      a.valid[q] = (uint8_t)d.valid;
      a.usable[q] = (uint8_t)us;
      a.chars[q] = d.chars;
    }
    __syncthreads();  // the tables are final in global memory
  }

  // 3. the chunk judged (n == 0: the state copied, info[0..7])
  win_judge_chunk(a.w, S.win);
  __syncthreads();  // accept, rank, carry_rank, reply, reply_ack and info[0..7] are final in global memory
  if (n == 0) {  // (uniform)
    if (tid == 0) {
      a.info[8] = a.info[9] = a.info[10] = a.info[11] = 0;
      *a.status = 0;
      if (a.carry_off) a.carry_off[0] = 0;
    }
    return;
  }
  const uint32_t K = a.info[1] < n ? (uint32_t)a.info[1] : n;
  const uint32_t P = a.info[5] < kRwCarryMax ? (uint32_t)a.info[5] : kRwCarryMax;

  // 4. the item of every rank, and the offsets in rank order
  for (uint32_t k = tid; k < kWinItems; k += kWinBlock) {
    S.msrc[k] = (uint16_t)kWinNil;
    if (k < kWinNew) S.csrc[k] = (uint16_t)kWinNil;
  }
  __syncthreads();
  for (uint32_t p = tid; p < n; p += kWinBlock) {
    const uint32_t r = a.w.rank[p], c = a.w.carry_rank[p];
    if (r < K) S.msrc[r] = (uint16_t)p;
    if (c < P) S.csrc[c] = (uint16_t)p;
  }
  __syncthreads();
  const uint32_t mtotal = rw_rank_offsets(S, S.msrc, K, (uint32_t)H, S.mo, S.sw32, a.payload_off, a.payload_src);
  const uint32_t ctotal = rw_rank_offsets(S, S.csrc, P, 0u, S.co, S.sw32, a.carry_off, nullptr);

  // 6. the replies: two consecutive items per thread
  {
    const ReplyOut out{a.reply_frames, a.reply_csum, a.reply_index, a.reply_peer, a.w.n};
    uint32_t rp = 0, rs = 0, cnt = 0, ra[2] = {0, 0};
#pragma unroll
    for (uint32_t u = 0; u < 2; ++u) {
      const uint32_t p = 2u * tid + u;
      if (p < n) {
        if (a.w.reply[p]) {
          rp |= 1u << u;
          ra[u] = a.w.reply_ack[p];
          ++cnt;
        }
        if (p >= nc && S.win.cls[p] == kWinReset) rs |= 1u << u;
      }
    }
    uint32_t R = 0;
    uint32_t slot = block_exclusive_scan32(cnt, &R, S.sw32);
    uint32_t r = block_exclusive_max(rs ? 2u * tid + (rs >> 1 ? 1u : 0u) + 1u : 0u, S.sw32);
#pragma unroll
    for (uint32_t u = 0; u < 2; ++u) {
      const uint32_t p = 2u * tid + u;
      if (rs & (1u << u)) r = p + 1u;
      if (rp & (1u << u)) put_reply<H>(out, slot++, p, ra[u], r);
    }
    if (tid == 0) a.info[8] = R;
  }
  __syncthreads();  // mo[], co[] complete

  // 5. both gathers out of the image;  7. carry_csum, info and status
  const bool mfits = mtotal <= a.payload_cap, cfits = ctotal <= a.carry_cap;
  if (mfits && mtotal)
    image_copy_ranked(S.img, S.mo, K, mtotal, a.payload, kWinBlock,
                      [&](uint32_t q) { return S.is[S.msrc[q]] + (uint32_t)H; });
  if (cfits && ctotal)
    image_copy_ranked(S.img, S.co, P, ctotal, a.carry_frames, kWinBlock, [&](uint32_t q) { return S.is[S.csrc[q]]; });
  if (a.carry_csum && a.csum[1]) {
    for (uint32_t k = tid; k < P; k += kWinBlock) {
      const uint32_t p = S.csrc[k];
      if (p != kWinNil) a.carry_csum[k] = p < nc ? a.csum[0][p] : a.csum[1][p - nc];
    }
  }
  if (tid == 0) {
    a.info[9] = mtotal;
    a.info[10] = ctotal;
    a.info[11] = 0;
    *a.status = (S.bad ? RUDP_ST_OFFSETS : 0u) | (mfits ? 0u : RUDP_ST_PAYLOAD_CAP) | (cfits ? 0u : RUDP_ST_CARRY_CAP);
  }
}

bool receive_window_fused_ok(uint64_t n_carried, uint64_t n_new, uint64_t total_bytes) {
  const uint64_t n = n_carried + n_new;
  if (n == 0) return true;
  const int knob = tuning().receive_window_fused;  // (2, diagnostics build: whatever the mean frame length)
  return knob && n_new <= kWinNew && n_carried <= kRwCarryMax && total_bytes <= kRwFusedBytes &&
         (knob == 2 || total_bytes <= (uint64_t)kRwFusedMeanFrame * n);
}

int launch_receive_window_fused(RecvWindowArgs a, hipStream_t stream) {
  a.w.chunk = 0;
  a.w.chunks = 1;
  hipError_t e = stream_scratch(reinterpret_cast<void**>(&a.w.hdr),
                                kWinHdr * sizeof(uint64_t) + 1024u * sizeof(uint32_t), stream, kScratchSums);
  if (e != hipSuccess) return (int)e;
  if (a.H == 7u) hipLaunchKernelGGL(receive_window_fused_kernel<7>, dim3(1), dim3(kWinBlock), 0, stream, a);
  else hipLaunchKernelGGL(receive_window_fused_kernel<5>, dim3(1), dim3(kWinBlock), 0, stream, a);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------- chained form

constexpr uint32_t kRwJoinFpt = 4;                        // consecutive items per thread
constexpr uint32_t kRwJoinTile = kBlock * kRwJoinFpt;     // 1024 items per block of the join's scan

__device__ __forceinline__ uint64_t rw_item_len(const RecvWindowArgs& a, uint64_t i, bool* bad) {
  uint32_t s;
  uint64_t o0, o1;
  *bad = !rw_item(a, i, &s, &o0, &o1);
  return *bad ? 0ull : o1 - o0;
}

// sums[b] = the bytes of the good items of block b; words[0] |= a rejected item.
__global__ void __launch_bounds__(kBlock) rw_join_sums_kernel(RecvWindowArgs a) {
  __shared__ uint64_t s_wave[kBlock / 64];
  uint64_t mine = 0;
  bool any_bad = false;
#pragma unroll
  for (uint32_t j = 0; j < kRwJoinFpt; ++j) {
    const uint64_t i = (uint64_t)blockIdx.x * kRwJoinTile + threadIdx.x * kRwJoinFpt + j;
    if (i >= a.w.n) break;
    bool bad;
    mine += rw_item_len(a, i, &bad);
    any_bad |= bad;
  }
  uint64_t total = 0;
  (void)block_exclusive_scan(mine, &total, s_wave);
  if (threadIdx.x == 0) a.sums[blockIdx.x] = total;
  if (any_bad) atomicOr(a.words, 1u);
}

// One workgroup: exclusive block bases in place, each thread over a run of
// consecutive blocks; joined_off[n] = the view's bytes.
__global__ void __launch_bounds__(kBlock) rw_join_bases_kernel(RecvWindowArgs a, uint64_t nb) {
  __shared__ uint64_t s_wave[kBlock / 64];
  const uint64_t per = (nb + kBlock - 1u) / kBlock;
  const uint64_t lo = threadIdx.x * per < nb ? threadIdx.x * per : nb, hi = lo + per < nb ? lo + per : nb;
  uint64_t mine = 0;
  for (uint64_t b = lo; b < hi; ++b) mine += a.sums[b];
  uint64_t total = 0;
  uint64_t run = block_exclusive_scan(mine, &total, s_wave);
  for (uint64_t b = lo; b < hi; ++b) {
    const uint64_t v = a.sums[b];
    a.sums[b] = run;
    run += v;
  }
  if (threadIdx.x == 0) a.joined_off[a.w.n] = total;
}

// joined_off[i] of every item, and its sideband checksum.
__global__ void __launch_bounds__(kBlock) rw_join_offsets_kernel(RecvWindowArgs a) {
  __shared__ uint64_t s_wave[kBlock / 64];
  uint64_t len[kRwJoinFpt], mine = 0;
#pragma unroll
  for (uint32_t j = 0; j < kRwJoinFpt; ++j) {
    const uint64_t i = (uint64_t)blockIdx.x * kRwJoinTile + threadIdx.x * kRwJoinFpt + j;
    bool bad;
    len[j] = i < a.w.n ? rw_item_len(a, i, &bad) : 0ull;
    mine += len[j];
  }
  uint64_t total = 0;
  uint64_t run = a.sums[blockIdx.x] + block_exclusive_scan(mine, &total, s_wave);
#pragma unroll
  for (uint32_t j = 0; j < kRwJoinFpt; ++j) {
    const uint64_t i = (uint64_t)blockIdx.x * kRwJoinTile + threadIdx.x * kRwJoinFpt + j;
    if (i >= a.w.n) break;
    a.joined_off[i] = run;
    run += len[j];
    if (a.joined_csum) a.joined_csum[i] = i < a.w.n_carried ? a.csum[0][i] : a.csum[1][i - a.w.n_carried];
  }
}

// The view's bytes, one 16-B chunk of it per thread (the view is 16-B
// aligned): the chunk's first item by a search of joined_off, then bytewise
// from the sources.  The grid covers both buffers' bytes, the bound of the view.
__global__ void __launch_bounds__(kBlock) rw_join_copy_kernel(RecvWindowArgs a) {
  const uint64_t total = a.joined_off[a.w.n];
  const uint64_t y0 = 16ull * ((uint64_t)blockIdx.x * kBlock + threadIdx.x);
  if (y0 >= total) return;
  // the item of byte y0: the last q with joined_off[q] <= y0 (joined_off[0] = 0 <= y0 < total)
  uint64_t q = 0, qh = a.w.n;
  while (qh - q > 1u) {
    const uint64_t m = (q + qh) >> 1;
    if (a.joined_off[m] <= y0) q = m; else qh = m;
  }
  uint64_t lo = 0, hi = 0, y = y0, qo = a.joined_off[q], qe = a.joined_off[q + 1u];
  const uint32_t nb = total - y0 < 16u ? (uint32_t)(total - y0) : 16u;
  for (uint32_t b = 0; b < nb; ++b, ++y) {
    while (qe <= y) {  // (y < total: stops at an item with bytes)
      ++q;
      qo = qe;
      qe = a.joined_off[q + 1u];
    }
    const uint32_t s = q < a.w.n_carried ? 0u : 1u;
    const uint64_t o0 = a.off[s][s ? q - a.w.n_carried : q];
    const uint64_t v = a.src[s][a.mis[s] + o0 + (y - qo)];
    if (b < 8) lo |= v << (8 * b); else hi |= v << (8 * (b - 8));
  }
  if (nb == 16u) {
    *reinterpret_cast<u32x4*>(a.joined + y0) = make_u32x4(lo, hi);
  } else {
    for (uint32_t b = 0; b < nb; ++b) a.joined[y0 + b] = (unsigned char)(b < 8 ? lo >> (8 * b) : hi >> (8 * (b - 8)));
  }
}

int launch_recv_window_join(const RecvWindowArgs& a, hipStream_t stream) {
  const uint64_t nb = (a.w.n + kRwJoinTile - 1u) / kRwJoinTile;
  const uint64_t nc = (a.bytes[0] + a.bytes[1] + 16ull * kBlock - 1u) / (16ull * kBlock);
  if (nb == 0 || nb > 0x7FFFFFFFull || nc > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(rw_join_sums_kernel, dim3((uint32_t)nb), dim3(kBlock), 0, stream, a);
  hipLaunchKernelGGL(rw_join_bases_kernel, dim3(1), dim3(kBlock), 0, stream, a, nb);
  hipLaunchKernelGGL(rw_join_offsets_kernel, dim3((uint32_t)nb), dim3(kBlock), 0, stream, a);
  if (nc) hipLaunchKernelGGL(rw_join_copy_kernel, dim3((uint32_t)nc), dim3(kBlock), 0, stream, a);
  return (int)hipGetLastError();
}

// Behind the existing launches: a rejected item (the join gave the decode an
// empty frame for it) gets the decode's tables of a rejected frame; the first
// workgroup gathers carry_csum and completes info and status.
__global__ void __launch_bounds__(kBlock) rw_finish_kernel(RecvWindowArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < a.w.n) {
    bool bad;
    (void)rw_item_len(a, i, &bad);
    if (bad) {
      a.seq[i] = 0;
      a.ack[i] = 0;
      a.flags[i] = 0;
      a.ok[i] = RUDP_OK_BAD_OFFSETS;
      if (a.csum_out) a.csum_out[i] = 0;
      a.valid[i] = 0;
      a.usable[i] = 0;
      a.chars[i] = 0;
    }
  }
  if (blockIdx.x) return;
  const uint64_t K = a.info[1] < a.w.n ? a.info[1] : a.w.n;
  const uint64_t P = a.info[5] < kRwCarryMax ? a.info[5] : kRwCarryMax;
  if (a.carry_csum && a.joined_csum) {
    for (uint64_t k = threadIdx.x; k < P; k += kBlock) {
      const uint32_t p = a.carry_src[k];
      if (p < a.w.n) a.carry_csum[k] = a.joined_csum[p];
    }
  }
  if (threadIdx.x == 0) {
    a.info[8] = a.rinfo[5];
    a.info[9] = a.payload_off[K];
    a.info[10] = a.carry_off[P];
    a.info[11] = 0;
    *a.status = (a.words[0] ? RUDP_ST_OFFSETS : 0u) | (a.words[2] & RUDP_ST_PAYLOAD_CAP) |
                ((a.words[3] & RUDP_ST_PAYLOAD_CAP) ? RUDP_ST_CARRY_CAP : 0u);
  }
}

int launch_recv_window_finish(const RecvWindowArgs& a, hipStream_t stream) {
  const uint64_t nb = (a.w.n + kBlock - 1u) / kBlock;
  if (nb == 0 || nb > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(rw_finish_kernel, dim3((uint32_t)nb), dim3(kBlock), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace rudp
