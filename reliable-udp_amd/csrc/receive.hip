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
//            accept_device.hpp, anomaly walk included), two block scans place
//            the kept payloads and the replies, and the payloads leave LDS as
//            16-B chunks of the output's own alignment (gather.hip's edge rule:
//            no store covers a byte outside [0, total)).  The image, the
//            per-lane decode, the copy-out and the reply writer are
//            frame_image_device.hpp's, shared with rudp_receive_window and
//            rudp_acknowledge.
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
#include "accept_device.hpp"
#include "frame_image_device.hpp"

namespace RUDP_NS {

// The fused form's byte limit: the frame image, the accept tile and the offset
// arrays stay within the 64 KiB of LDS a workgroup gets without asking.
constexpr uint32_t kRecvFusedBytes = 32768;
// and its mean frame length: a frame is decoded by one lane, so long frames
// serialise the workgroup.  261 B is the largest measured mean at which the
// fused form still beat the chained one in every round (125 x 261 B: 38 against
// 42-43 us; 32 x 1005 B: 50 against 44; profiles/r10/receive.json).
constexpr uint32_t kRecvFusedMeanFrame = 261;

__device__ __forceinline__ ReplyOut recv_reply_out(const ReceiveArgs& a) {
  return ReplyOut{a.reply_frames, a.reply_csum, a.reply_index, a.reply_peer, a.n};
}

// ------------------------------------------------------------------ fused form

struct RecvLds {
  AccLds acc;
  uint32_t fo[kAccTile + 1];  // frame offsets in the image (kImgBadOff: past the buffer)
  uint32_t po[kAccTile + 1];  // payload offsets
  uint64_t sw[kBlock / 64];
  uint32_t sw32[kBlock / 64];
  uint32_t bad;               // a frame failed the offset rule
  // the aligned buffer from the 16-B boundary below d_frames, and window16_dw's reach past it
  __attribute__((aligned(16))) uint32_t img[(kRecvFusedBytes + 16u + 32u) / 4u];
};

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
    image_load(S.img, a.frames, a.frames_bytes ? (uint32_t)(a.fmis + a.frames_bytes) : 0u, kBlock);
    image_offsets(S.fo, a.frame_off, n, a.frames_bytes, a.fmis, kBlock);
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
    uint32_t any_bad = 0;
#pragma unroll 1
    for (uint32_t j = 0; j < kAccFpt; ++j) {
      const uint32_t q = j * kBlock + tid;
      if (q >= n) break;
      const FrameDecode d = image_decode_frame<H, true>(S.img, S.fo[q], S.fo[q + 1u], a.csum_in != nullptr,
                                                        [&] { return (uint32_t)a.csum_in[q]; });
      any_bad |= d.ok == RUDP_OK_BAD_OFFSETS;
      const uint32_t us = (d.ok == RUDP_OK_GOOD || d.ok == RUDP_OK_UNVERIFIED) && d.valid == 1u;
      a.seq[q] = (uint16_t)d.seq;
      a.ack[q] = (uint16_t)d.ack;
      a.flags[q] = (uint8_t)d.fl;
      a.ok[q] = (uint8_t)d.ok;
      if (a.csum_out) a.csum_out[q] = (uint16_t)d.cs;
      a.valid[q] = (uint8_t)d.valid;
      a.usable[q] = (uint8_t)us;
      a.chars[q] = d.chars;
      L.seq[q] = (uint16_t)d.seq;
      L.fl[q] = (uint8_t)d.fl;
      L.ch[q] = d.chars;
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
      const bool good = fs != kImgBadOff && fe != kImgBadOff && fs <= fe;
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
  uint64_t r = block_exclusive_max<uint64_t>(rs ? tid * kAccFpt + (31u - __clz(rs)) + 1u : 0u, S.sw);
#pragma unroll
  for (uint32_t j = 0; j < kAccFpt; ++j) {
    const uint32_t k = tid * kAccFpt + j;
    if (k >= n) break;
    S.po[k] = run;
    a.payload_off[k] = run;
    run += pl[j];
    if (rs & (1u << j)) r = (uint64_t)k + 1u;
    if (rp & (1u << j)) put_reply<H>(recv_reply_out(a), slot++, k, ra[j], r);
  }
  if (tid == 0) {
    S.po[n] = total;
    a.payload_off[n] = total;
  }
  __syncthreads();

  // 6. the kept payloads out of LDS;  7. info and status
  const bool fits = total <= a.payload_cap;
  if (fits && total)
    image_copy_ranked(S.img, S.po, n, total, a.payload, kBlock, [&](uint32_t q) { return S.fo[q] + (uint32_t)H; });
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
    if (m.rp & (1u << j)) put_reply<H>(recv_reply_out(a), slot++, i, ra[j], r);
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
