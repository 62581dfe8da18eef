// rudp_receive: a datagram batch to message and replies in one call -- what the
// reference's recv() loop (utils/reliableUDP.py:97-137) makes of the datagrams
// one recvmmsg returned, and the send_ack packets it answers them with
// (:139-146): decode + strict UTF-8, usable, characters, in-order acceptance,
// payload gather and the reply datagrams.
//
// Two forms behind the one entry point (capi.hip chooses):
//
//   fused    a batch of at most one accept tile (kAccTile frames) whose buffer
//            is at most kRecvFusedBytes and kRecvFusedMeanFrame bytes per
//            frame: one workgroup, one launch.  The frames
//            go into LDS once, with aligned 16-B loads from the boundary at or
//            below d_frames; every later step reads that image.  A thread
//            decodes four frames (offset rule, header, checksum, UTF-8 verdict,
//            lead bytes), the acceptance runs on the LDS tile (acc_one_tile of
//            accept.hip, anomaly walk included), two block scans place the kept
//            payloads and the replies, and the payloads leave LDS as 16-B
//            chunks of the output's own alignment (gather.hip's edge rule: no
//            store covers a byte outside [0, total)).
//   chained  everything else: the existing decode, payload_chars, accept and
//            gather launches on the stream, with the two steps only this call
//            has: usable[] (one elementwise kernel) and the reply builder
//            (reduce-then-scan of reply[] over tiles of kAccTile frames; the
//            last reset before each frame is rescanned from seq, flags and
//            usable, which class a frame without the state: acc_class).
//
// A reply datagram is the header-only frame of Packet().to_byte() with seq 0,
// ack = reply_ack[i] and flags 0x40 (ACK); for rudp7 its RFC 1071 checksum is
// in-band, and d_reply_csum carries it for both layouts.
#define RUDP_ACCEPT_DEVICE_ONLY 1
#include "accept.hip"
#include "utf8_device.hpp"

namespace RUDP_NS {

// The fused form's byte limit: the frame image, the accept tile and the offset
// arrays stay within the 64 KiB of LDS a workgroup gets without asking.
constexpr uint32_t kRecvFusedBytes = 32768;
// and its mean frame length: a frame is decoded by one lane, so long frames
// serialise the workgroup.  261 B is the largest measured mean at which the
// fused form still beat the chained one in every round (125 x 261 B: 38 against
// 42-43 us; 32 x 1005 B: 50 against 44; profiles/r10/receive.json).
constexpr uint32_t kRecvFusedMeanFrame = 261;
constexpr uint32_t kRecvBadOff = 0xFFFFFFFFu;  // an offset past frames_bytes, in the LDS copy

// Exclusive prefix maximum of one u64 per thread over the block (all threads call it).
__device__ inline uint64_t block_exclusive_max(uint64_t x, uint64_t* s_wave) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint64_t incl = x;
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint64_t y = __shfl_up(incl, d, 64);
    if (lane >= d && y > incl) incl = y;
  }
  if (lane == 63) s_wave[wave] = incl;
  uint64_t ex = __shfl_up(incl, 1, 64);
  if (lane == 0) ex = 0;
  __syncthreads();
  uint64_t before = 0;
  for (uint32_t w = 0; w < wave; ++w) before = s_wave[w] > before ? s_wave[w] : before;
  __syncthreads();  // s_wave may be reused by the caller
  return before > ex ? before : ex;
}

// Reply `slot`: the send_ack packet for datagram i, and its tables.  r: 1 +
// the index of the last reset at or before i (0: none in this batch).
template <int H>
__device__ __forceinline__ void recv_put_reply(const ReceiveArgs& a, uint64_t slot, uint64_t i, uint32_t ack,
                                               uint64_t r) {
  const uint32_t c = packet_csum(0u, 0u, ack, 0x40u);
  const uint64_t h = pack_header<H>(0u, ack, 0x40u, c);
  unsigned char* o = a.reply_frames + slot * (uint64_t)H;
#pragma unroll
  for (int b = 0; b < H; ++b) o[b] = (unsigned char)(h >> (8 * b));
  if (a.reply_csum) a.reply_csum[slot] = (uint16_t)c;
  a.reply_index[slot] = (uint32_t)i;
  a.reply_peer[slot] = r ? r - 1u : a.n;
}

// ------------------------------------------------------------------ fused form

struct RecvLds {
  AccLds acc;
  uint32_t fo[kAccTile + 1];  // frame offsets in the image (kRecvBadOff: past the buffer)
  uint32_t po[kAccTile + 1];  // payload offsets
  uint64_t sw[kBlock / 64];
  uint32_t sw32[kBlock / 64];
  uint32_t bad;               // a frame failed the offset rule
  // the aligned buffer from the 16-B boundary below d_frames, and window16_dw's reach past it
  __attribute__((aligned(16))) uint32_t img[(kRecvFusedBytes + 16u + 32u) / 4u];
};

// The kept payloads [0, total) out of the image to `o`, dealt as the 16-B
// chunks of o's own alignment: a whole chunk is one 16-B store, the partial
// chunk at either end goes bytewise.
__device__ inline void recv_copy_payloads(const RecvLds& S, uint32_t n, uint32_t total, uint32_t H, unsigned char* o) {
  const unsigned char* img = reinterpret_cast<const unsigned char*>(S.img);
  const uint32_t lead = (uint32_t)(-(uintptr_t)o) & 15u;  // bytes before the first aligned chunk
  const uint32_t nch = total > lead ? (total - lead + 15u) / 16u + 1u : 1u;  // chunk 0 is the head [0, lead)
  for (uint32_t c = threadIdx.x; c < nch; c += kBlock) {
    const int x = c == 0 ? (int)lead - 16 : (int)(lead + 16u * (c - 1u));
    const int b_lo = x < 0 ? -x : 0;
    const int b_hi = (uint32_t)(x + 16) <= total ? 16 : (int)total - x;
    if (b_hi <= b_lo) continue;
    uint32_t y = (uint32_t)(x + b_lo);
    // the frame of output byte y: the last q with po[q] <= y (po[0] = 0 <= y < total = po[n])
    uint32_t q = 0, qh = n;
    while (qh - q > 1u) {
      const uint32_t m = (q + qh) >> 1;
      if (S.po[m] <= y) q = m; else qh = m;
    }
    uint64_t lo = 0, hi = 0;
    for (int b = b_lo; b < b_hi; ++b, ++y) {
      while (S.po[q + 1u] <= y) ++q;  // (y < po[n]: stops at a frame with a payload)
      const uint64_t v = img[S.fo[q] + H + (y - S.po[q])];
      if (b < 8) lo |= v << (8 * b); else hi |= v << (8 * (b - 8));
    }
    if (b_lo == 0 && b_hi == 16) {
      *reinterpret_cast<u32x4*>(o + x) = make_u32x4(lo, hi);
    } else {
      for (int b = b_lo; b < b_hi; ++b) o[x + b] = (unsigned char)(b < 8 ? lo >> (8 * b) : hi >> (8 * (b - 8)));
    }
  }
}

template <int H>
__global__ void __launch_bounds__(kBlock) receive_fused_kernel(ReceiveArgs a) {
  __shared__ RecvLds S;
  AccLds& L = S.acc;
  const uint32_t tid = threadIdx.x;
  const AccSeed seed{a.state_in[0], a.state_in[1], a.state_in[2] ? 1ull : 0ull};
  AcceptArgs acc{};
  acc.seq = a.seq;
  acc.flags = a.flags;
  acc.chars = a.chars;
  acc.usable = a.usable;
  acc.n = a.n;
  acc.last_isn = a.last_isn;
  acc.state_in = a.state_in;
  acc.state_out = a.state_out;
  acc.accept = a.accept;
  acc.keep = a.keep;
  acc.reply = a.reply;
  acc.reply_ack = a.reply_ack;
  acc.info = a.info;
  if (a.n == 0) {  // (uniform)
    acc_empty(acc, seed);
    if (tid == 0) {
      a.info[6] = a.info[7] = 0;
      *a.status = 0;
    }
    return;
  }
  const uint32_t n = (uint32_t)a.n;

  // 1. the buffer into LDS once, and its offsets
  {
    const uint32_t img_bytes = a.frames_bytes ? (uint32_t)(a.fmis + a.frames_bytes) : 0u;
    const uint32_t nvec = (img_bytes + 15u) >> 4;
    u32x4* dst = reinterpret_cast<u32x4*>(S.img);
    for (uint32_t v0 = tid; v0 < nvec; v0 += 4u * kBlock) {
      u32x4 r[4];
#pragma unroll
      for (uint32_t u = 0; u < 4; ++u)
        if (v0 + u * kBlock < nvec) r[u] = load16_guarded(a.frames, 16ull * (v0 + u * kBlock), img_bytes);
#pragma unroll
      for (uint32_t u = 0; u < 4; ++u)
        if (v0 + u * kBlock < nvec) dst[v0 + u * kBlock] = r[u];
    }
    for (uint32_t k = tid; k <= n; k += kBlock) {
      const uint64_t o = a.frame_off[k];
      S.fo[k] = o <= a.frames_bytes ? (uint32_t)(o + a.fmis) : kRecvBadOff;
    }
    if (tid == 0) {
      L.e_min = a.n;
      L.a_min = a.n;
      a.info[1] = 0;
      S.bad = 0;
    }
  }
  __syncthreads();

  // 2, 3. every frame by one lane: the decode's outputs, usable and chars
  {
    const uint32_t* dw = S.img;
    const unsigned char* ib = reinterpret_cast<const unsigned char*>(S.img);
    uint32_t any_bad = 0;
#pragma unroll 1
    for (uint32_t j = 0; j < kAccFpt; ++j) {
      const uint32_t q = j * kBlock + tid;
      if (q >= n) break;
      const uint32_t fs = S.fo[q], fe = S.fo[q + 1u];
      uint32_t seq = 0, ack = 0, fl = 0, ok = RUDP_OK_BAD_OFFSETS, cs = 0, valid = 0, ch = 0;
      if (fs == kRecvBadOff || fe == kRecvBadOff || fs > fe) {
        any_bad = 1;  // rejected: nothing of it is read
      } else {
        const uint32_t F = fe - fs, ps = fs + (uint32_t)H;
        uint32_t ev = 0, od = 0, hib = 0;  // byte sums at even / odd image offsets; high bits of the payload
        if (fe > ps) {  // the payload's dwords, the edge ones masked to it
          const uint32_t w0 = ps >> 2, w1 = (fe - 1u) >> 2;
          for (uint32_t w = w0; w <= w1; ++w) {
            uint32_t v = dw[w], lanes = 0xFu;
            if (w == w0 || w == w1) {
              const int lo = (int)ps - (int)(4u * w), hi = (int)fe - (int)(4u * w);
              const int l0 = lo < 0 ? 0 : lo, h0 = hi < 4 ? hi : 4;
              v &= (uint32_t)byte_mask(l0, h0);
              lanes = ((1u << h0) - 1u) & ~((1u << l0) - 1u);
            }
            hib |= v;
            ev = even_bytes_acc(v, ev);
            od = odd_bytes_acc(v, od);
            ch += __popc(lead4(v) & lanes);
          }
        }
        valid = (hib & 0x80808080u) && utf8_check_bytes(ps, fe, [&](uint32_t i) { return (uint32_t)ib[i]; }) ? 0u : 1u;
        const uint32_t sum = (fs & 1u) ? (ev + (od << 8)) : ((ev << 8) + od);
        const u32x4 h = window16_dw(dw, fs);
        const uint32_t b0 = h.x & 0xFFu, b1 = (h.x >> 8) & 0xFFu, b2 = (h.x >> 16) & 0xFFu, b3 = h.x >> 24,
                       b4 = h.y & 0xFFu, b5 = (h.y >> 8) & 0xFFu, b6 = (h.y >> 16) & 0xFFu;
        if (F < (uint32_t)H) {  // short frame: fields truncated as utils/packet.py:31 slices them
          const uint32_t c0 = F > 0 ? b0 : 0u, c1 = F > 1 ? b1 : 0u, c2 = F > 2 ? b2 : 0u, c3 = F > 3 ? b3 : 0u,
                         c4 = F > 4 ? b4 : 0u;
          seq = F >= 2 ? (c0 << 8) | c1 : c0;
          ack = F >= 4 ? (c2 << 8) | c3 : c2;
          fl = c4;
          ok = RUDP_OK_SHORT;
        } else {
          seq = (b0 << 8) | b1;
          ack = (b2 << 8) | b3;
          fl = b4;
          cs = packet_csum(sum, seq, ack, fl);
          if (H == 7) ok = cs == ((b5 << 8) | b6) ? RUDP_OK_GOOD : RUDP_OK_BAD_CSUM;
          else ok = a.csum_in ? (cs == a.csum_in[q] ? RUDP_OK_GOOD : RUDP_OK_BAD_CSUM) : RUDP_OK_UNVERIFIED;
        }
      }
      const uint32_t us = (ok == RUDP_OK_GOOD || ok == RUDP_OK_UNVERIFIED) && valid == 1u;
      a.seq[q] = (uint16_t)seq;
      a.ack[q] = (uint16_t)ack;
      a.flags[q] = (uint8_t)fl;
      a.ok[q] = (uint8_t)ok;
      if (a.csum_out) a.csum_out[q] = (uint16_t)cs;
      a.valid[q] = (uint8_t)valid;
      a.usable[q] = (uint8_t)us;
      a.chars[q] = ch;
      L.seq[q] = (uint16_t)seq;
      L.fl[q] = (uint8_t)fl;
      L.ch[q] = ch;
      L.us[q] = (uint8_t)us;
    }
    if (any_bad) atomicOr(&S.bad, 1u);
  }
  __syncthreads();

  // 4. the acceptance on the LDS tile
  acc_one_tile(acc, L, seed);
  __syncthreads();  // keep, reply and reply_ack are final in global memory

  // 5. payload offsets and reply slots: four consecutive frames per thread
  uint32_t pl[kAccFpt], ra[kAccFpt];
  uint32_t rp = 0, rs = 0;  // bit j: frame j is answered / is a reset
  uint32_t mine = 0, cnt = 0;
#pragma unroll
  for (uint32_t j = 0; j < kAccFpt; ++j) {
    const uint32_t k = tid * kAccFpt + j;
    pl[j] = 0;
    ra[j] = 0;
    if (k < n) {
      const uint32_t fs = S.fo[k], fe = S.fo[k + 1u];
      const bool good = fs != kRecvBadOff && fe != kRecvBadOff && fs <= fe;
      if (a.keep[k] && good && fe - fs > (uint32_t)H) pl[j] = fe - fs - (uint32_t)H;
      if (a.reply[k]) {
        rp |= 1u << j;
        ra[j] = a.reply_ack[k];
        ++cnt;
      }
      if (acc_class(a.usable[k], a.flags[k], a.seq[k], a.last_isn) == kAccReset) rs |= 1u << j;
    }
    mine += pl[j];
  }
  uint32_t total = 0, R = 0;
  uint32_t run = block_exclusive_scan32(mine, &total, S.sw32);
  uint32_t slot = block_exclusive_scan32(cnt, &R, S.sw32);
  uint64_t r = block_exclusive_max(rs ? (uint64_t)(tid * kAccFpt + (31u - __clz(rs))) + 1u : 0ull, S.sw);
#pragma unroll
  for (uint32_t j = 0; j < kAccFpt; ++j) {
    const uint32_t k = tid * kAccFpt + j;
    if (k >= n) break;
    S.po[k] = run;
    a.payload_off[k] = run;
    run += pl[j];
    if (rs & (1u << j)) r = (uint64_t)k + 1u;
    if (rp & (1u << j)) recv_put_reply<H>(a, slot++, k, ra[j], r);
  }
  if (tid == 0) {
    S.po[n] = total;
    a.payload_off[n] = total;
  }
  __syncthreads();

  // 6. the kept payloads out of LDS;  7. info and status
  const bool fits = total <= a.payload_cap;
  if (fits && total) recv_copy_payloads(S, n, total, (uint32_t)H, a.payload);
  if (tid == 0) {
    a.info[5] = R;
    a.info[6] = total;
    a.info[7] = 0;
    *a.status = (S.bad ? RUDP_ST_OFFSETS : 0u) | (fits ? 0u : RUDP_ST_PAYLOAD_CAP);
  }
}

bool receive_fused_ok(uint64_t n, uint64_t frames_bytes) {
  if (n == 0) return true;
  const int knob = tuning().receive_fused;  // (2, diagnostics build: whatever the mean frame length)
  return knob && n <= kAccTile && frames_bytes <= kRecvFusedBytes &&
         (knob == 2 || frames_bytes <= (uint64_t)kRecvFusedMeanFrame * n);
}

int launch_receive_fused(const ReceiveArgs& a, hipStream_t stream) {
  if (a.H == 7u) hipLaunchKernelGGL(receive_fused_kernel<7>, dim3(1), dim3(kBlock), 0, stream, a);
  else hipLaunchKernelGGL(receive_fused_kernel<5>, dim3(1), dim3(kBlock), 0, stream, a);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------- chained form

__global__ void __launch_bounds__(kBlock) receive_usable_kernel(const uint8_t* ok, const uint8_t* valid,
                                                                uint8_t* usable, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t o = ok[i];
  usable[i] = (uint8_t)((o == RUDP_OK_GOOD || o == RUDP_OK_UNVERIFIED) && valid[i] == 1);
}

int launch_receive_usable(const uint8_t* ok, const uint8_t* valid, uint8_t* usable, uint64_t n, hipStream_t stream) {
  const uint64_t nb = (n + kBlock - 1u) / kBlock;
  if (nb > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(receive_usable_kernel, dim3((uint32_t)nb), dim3(kBlock), 0, stream, ok, valid, usable, n);
  return (int)hipGetLastError();
}

// The reply builder, reduce-then-scan over tiles of kAccTile frames, four
// consecutive frames per thread.  tiles[2 t] = replies of tile t, tiles[2 t +
// 1] = 1 + the index of its last reset (0: none); the bases pass turns both
// into what precedes the tile.
struct ReplyMine {
  uint32_t rp, rs, cnt;
  uint64_t last;  // 1 + index of the thread's last reset, 0: none
};
__device__ __forceinline__ ReplyMine reply_mine(const ReceiveArgs& a, uint64_t p0) {
  ReplyMine m{0, 0, 0, 0};
#pragma unroll
  for (uint32_t j = 0; j < kAccFpt; ++j) {
    const uint64_t i = p0 + threadIdx.x * kAccFpt + j;
    if (i >= a.n) break;
    if (a.reply[i]) {
      m.rp |= 1u << j;
      ++m.cnt;
    }
    if (i >= a.first && acc_class(a.usable[i], a.flags[i], a.seq[i], a.last_isn) == kAccReset) {
      m.rs |= 1u << j;
      m.last = i + 1u;
    }
  }
  return m;
}

__global__ void __launch_bounds__(kBlock) reply_count_kernel(ReceiveArgs a) {
  __shared__ uint64_t s_cnt[kBlock / 64], s_last[kBlock / 64];
  const ReplyMine m = reply_mine(a, (uint64_t)blockIdx.x * kAccTile);
  const uint64_t cnt = wave_sum64(m.cnt);
  uint64_t last = m.last;
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint64_t y = __shfl_xor(last, d, 64);
    last = y > last ? y : last;
  }
  if ((threadIdx.x & 63u) == 0) {
    s_cnt[threadIdx.x >> 6] = cnt;
    s_last[threadIdx.x >> 6] = last;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t c = 0, l = 0;
    for (uint32_t w = 0; w < kBlock / 64; ++w) {
      c += s_cnt[w];
      l = s_last[w] > l ? s_last[w] : l;
    }
    a.tiles[2u * blockIdx.x] = c;
    a.tiles[2u * blockIdx.x + 1u] = l;
  }
}

// One workgroup: exclusive tile bases in place, each thread over a run of
// consecutive tiles; R, the message bytes and the reserved word of d_info.
__global__ void __launch_bounds__(kBlock) reply_bases_kernel(ReceiveArgs a, uint64_t nt) {
  __shared__ uint64_t s_wave[kBlock / 64];
  const uint64_t per = (nt + kBlock - 1u) / kBlock;
  const uint64_t lo = threadIdx.x * per < nt ? threadIdx.x * per : nt, hi = lo + per < nt ? lo + per : nt;
  uint64_t mine = 0, last = 0;
  for (uint64_t t = lo; t < hi; ++t) {
    mine += a.tiles[2u * t];
    last = a.tiles[2u * t + 1u] ? a.tiles[2u * t + 1u] : last;
  }
  uint64_t total = 0;
  uint64_t run = block_exclusive_scan(mine, &total, s_wave);
  uint64_t r = block_exclusive_max(last, s_wave);
  for (uint64_t t = lo; t < hi; ++t) {
    const uint64_t c = a.tiles[2u * t], l = a.tiles[2u * t + 1u];
    a.tiles[2u * t] = run;
    a.tiles[2u * t + 1u] = r;
    run += c;
    r = l ? l : r;
  }
  if (threadIdx.x == 0) {
    a.info[5] = total;
    a.info[6] = a.payload_off[a.n];
    a.info[7] = 0;
  }
}

template <int H>
__global__ void __launch_bounds__(kBlock) reply_write_kernel(ReceiveArgs a) {
  __shared__ uint64_t s_wave[kBlock / 64];
  __shared__ uint32_t s_wave32[kBlock / 64];
  const uint64_t p0 = (uint64_t)blockIdx.x * kAccTile;
  const ReplyMine m = reply_mine(a, p0);
  uint32_t ra[kAccFpt];
#pragma unroll
  for (uint32_t j = 0; j < kAccFpt; ++j)
    ra[j] = (m.rp & (1u << j)) ? (uint32_t)a.reply_ack[p0 + threadIdx.x * kAccFpt + j] : 0u;
  const uint64_t base = a.tiles[2u * blockIdx.x], base_r = a.tiles[2u * blockIdx.x + 1u];
  uint32_t total = 0;
  uint64_t slot = base + block_exclusive_scan32(m.cnt, &total, s_wave32);
  uint64_t r = block_exclusive_max(m.last, s_wave);
  if (!r) r = base_r;
#pragma unroll
  for (uint32_t j = 0; j < kAccFpt; ++j) {
    const uint64_t i = p0 + threadIdx.x * kAccFpt + j;
    if (m.rs & (1u << j)) r = i + 1u;
    if (m.rp & (1u << j)) recv_put_reply<H>(a, slot++, i, ra[j], r);
  }
}

int launch_receive_replies(ReceiveArgs a, hipStream_t stream) {
  const uint64_t nt = (a.n + kAccTile - 1u) / kAccTile;
  if (nt == 0 || nt > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
  hipError_t e = stream_scratch(reinterpret_cast<void**>(&a.tiles), 2u * nt * sizeof(uint64_t), stream,
                                kScratchRecords);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(reply_count_kernel, dim3((uint32_t)nt), dim3(kBlock), 0, stream, a);
  hipLaunchKernelGGL(reply_bases_kernel, dim3(1), dim3(kBlock), 0, stream, a, nt);
  if (a.H == 7u) hipLaunchKernelGGL(reply_write_kernel<7>, dim3((uint32_t)nt), dim3(kBlock), 0, stream, a);
  else hipLaunchKernelGGL(reply_write_kernel<5>, dim3((uint32_t)nt), dim3(kBlock), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace rudp
