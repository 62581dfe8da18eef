// rudp_receive_flows: the many-peer receiver in one call -- rudp_receive for a
// server whose recvmmsg batch carries datagrams of many transfers.  Decode +
// strict UTF-8, usable, characters, the per-flow in-order rule with every
// peer's row in a device table (flows.hip), every active flow's message piece
// back to back in flow order, the reply datagrams, and for every flow whose
// transfer ended the closing datagram (FIN|ACK) its peer is owed.
//
// Two forms behind the one entry point (capi.hip chooses):
//
//   fused    a batch (at most kFlowMax datagrams) in at most kRfFusedBytes and
//            kRfFusedMeanFrame bytes per datagram: one workgroup of 256
//            threads, one launch, no scratch.
//              1. the buffer into LDS once, with aligned 16-B guarded loads
//                 from the boundary at or below d_frames, and every frame's
//                 place in the image (kImgBadOff: rejected by the offset rule);
//              2. one lane per frame: header, RFC 1071 sum, UTF-8 verdict, lead
//                 bytes (image_decode_frame, as receive.hip's fused kernel);
//                 the decode tables, usable and chars to global memory, and the
//                 same values with the flow's key straight into FlowLds
//                 (flows_put: step 1 of flows.hip without its loads);
//              3. steps 2-7 of flows.hip on those tables (flows_judge_lds);
//              4. the datagram of every rank (an LDS table) and a scan of the
//                 ranked payload lengths: payload_off, payload_src;
//              5. the replies and the closing datagrams (rf_tail, below);
//              6. the message out of the image as 16-B chunks of the output's
//                 own alignment (image_copy_ranked: no store covers a byte
//                 outside [0, total));
//              7. info[8..11] and status.
//   chained  everything else: the existing launches (decode + UTF-8, usable,
//            payload_chars, the flows' rule, gather_ordered), each with a
//            status word of its own in the call's scratch, and one workgroup
//            behind them: rf_tail, info[8..11] and the merged status.
//
// A reply datagram is rudp_receive's (seq 0, ack = reply_ack[i], flags 0x40); a
// closing datagram is the header-only frame with seq 0, ack = isn + characters
// mod 2^16 and flags 0x60.  For rudp7 the RFC 1071 checksum is in-band, and the
// csum tables carry it for both layouts.
#include "flows_device.hpp"
#include "frame_image_device.hpp"

namespace RUDP_NS {

// The fused form's byte limit: the image and the offset tables fit beside
// FlowLds in the 160 KiB a workgroup can declare.
constexpr uint32_t kRfFusedBytes = 32768;
// and its mean frame length: a frame is decoded by one lane, so long frames
// serialise the workgroup, while the chained form gets cheaper with fewer
// frames.  133 B is the largest measured mean at which the fused form beat the
// chained one in every round.  One flow, buffers filled to 32 KiB, fused
// against chained in us (profiles/r15/receive_flows.json): 1024 x 6 B 36.8 / 58.5,
// 1024 x 21 B 48.6 / 52.0, 246 x 133 B 43.1 / 44.5 (every round); 474 x 69 B
// 46.8 / 44.9, 166 x 197 B 47.3 / 45.7, 125 x 261 B 45.8 / 42.5, 32 x 1005 B
// 55.3 / 42.4 (lost).  From 69 B on the two forms are within 2 us of each other
// up to the limit; longer means chain.
constexpr uint32_t kRfFusedMeanFrame = 133;

// Header-only frame `slot` of a table of frames at stride H, and its checksum.
template <int H>
__device__ __forceinline__ void rf_put_frame(unsigned char* frames, uint16_t* csum, uint32_t slot, uint32_t ack,
                                             uint32_t flags) {
  const uint32_t c = packet_csum(0u, 0u, ack, flags);
  const uint64_t h = pack_header<H>(0u, ack, flags, c);
  unsigned char* o = frames + (uint64_t)slot * (uint64_t)H;
#pragma unroll
  for (int b = 0; b < H; ++b) o[b] = (unsigned char)(h >> (8 * b));
  if (csum) csum[slot] = (uint16_t)c;
}

// The replies and the closing datagrams from what the rule left in global
// memory (final behind a barrier or a launch boundary): reply[] scanned in
// arrival order, four consecutive datagrams per thread; the ended runs
// (flow_info[a][1] < n) scanned in flow order, four consecutive runs per
// thread.  All kBlock threads call it; A <= n <= kFlowMax.
template <int H>
__device__ inline void rf_tail(const RecvFlowsArgs& a, uint32_t n, uint32_t A, uint32_t* sw32) {
  const uint32_t tid = threadIdx.x;
  {
    uint32_t rp = 0, cnt = 0, ra[kFlowFpt];
#pragma unroll
    for (uint32_t j = 0; j < kFlowFpt; ++j) {
      const uint32_t i = tid * kFlowFpt + j;
      ra[j] = 0;
      if (i < n && a.f.reply[i]) {
        rp |= 1u << j;
        ra[j] = a.f.reply_ack[i];
        ++cnt;
      }
    }
    uint32_t R = 0;
    uint32_t slot = block_exclusive_scan32(cnt, &R, sw32);
#pragma unroll
    for (uint32_t j = 0; j < kFlowFpt; ++j) {
      if (!(rp & (1u << j))) continue;
      rf_put_frame<H>(a.reply_frames, a.reply_csum, slot, ra[j], 0x40u);
      a.reply_index[slot] = tid * kFlowFpt + j;
      ++slot;
    }
  }
  {
    uint32_t en = 0, cnt = 0, fa[kFlowFpt];
#pragma unroll
    for (uint32_t j = 0; j < kFlowFpt; ++j) {
      const uint32_t r = tid * kFlowFpt + j;
      fa[j] = 0;
      if (r < A) {
        const uint64_t* fi = a.f.flow_info + 8ull * r;
        if (fi[1] < (uint64_t)n) {
          en |= 1u << j;
          fa[j] = (uint32_t)(fi[5] + fi[4]) & 0xFFFFu;
          ++cnt;
        }
      }
    }
    uint32_t E = 0;
    uint32_t slot = block_exclusive_scan32(cnt, &E, sw32);
#pragma unroll
    for (uint32_t j = 0; j < kFlowFpt; ++j) {
      if (!(en & (1u << j))) continue;
      rf_put_frame<H>(a.fin_frames, a.fin_csum, slot, fa[j], 0x60u);
      a.fin_flow[slot] = tid * kFlowFpt + j;
      ++slot;
    }
  }
}

// ------------------------------------------------------------------ fused form

struct RfLds {
  FlowLds flow;
  uint32_t fo[kFlowMax + 1];   // frame offsets in the image (kImgBadOff: past the buffer)
  uint32_t po[kFlowMax + 1];   // message offsets in rank order
  uint16_t src[kFlowMax];      // the datagram of every rank
  uint32_t sw32[kBlock / 64];
  uint32_t bad;                // a frame failed the offset rule
  // the aligned buffer from the 16-B boundary below d_frames, and window16_dw's reach past it
  __attribute__((aligned(16))) uint32_t img[(kRfFusedBytes + 16u + 32u) / 4u];
};
static_assert(sizeof(RfLds) <= 160 * 1024, "the fused receive_flows' LDS exceeds a gfx950 workgroup's 160 KiB");

template <int H>
__global__ void __launch_bounds__(kBlock) receive_flows_fused_kernel(RecvFlowsArgs a) {
  __shared__ RfLds S;
  FlowLds& L = S.flow;
  const uint32_t tid = threadIdx.x, n = (uint32_t)a.f.n;  // (n <= kFlowMax)
  if (n == 0) {  // (uniform)
    if (tid < 12) a.info[tid] = 0;
    if (tid == 0) *a.status = 0;
    return;
  }

  // 1. the buffer into LDS once, and its offsets
  image_load(S.img, a.frames, a.frames_bytes ? (uint32_t)(a.fmis + a.frames_bytes) : 0u, kBlock);
  image_offsets(S.fo, a.frame_off, n, a.frames_bytes, a.fmis, kBlock);
  const uint32_t N2 = flows_reset(L, n);
  if (tid == 0) S.bad = 0;
  __syncthreads();

  // 2. every frame by one lane: the decode's outputs, usable and chars, and step 1 of the rule
  {
    uint32_t any_bad = 0;
#pragma unroll 1
    for (uint32_t q = tid; q < N2; q += kBlock) {
      if (q >= n) {
        flows_pad(L, q);
        continue;
      }
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
      flows_put(a.f, L, q, d.seq, d.fl, d.chars, us != 0u);
    }
    if (any_bad) atomicOr(&S.bad, 1u);
  }
  __syncthreads();

  // 3. the flows judged on the LDS tables
  flows_judge_lds(a.f, L, N2, nullptr);
  __syncthreads();  // rank, reply, reply_ack, flow_info and info[0..7] are final in global memory
  const uint32_t A = a.info[0] < n ? (uint32_t)a.info[0] : n;
  const uint32_t K = a.info[1] < n ? (uint32_t)a.info[1] : n;

  // 4. the datagram of every rank (every rank below K is some datagram's), and the offsets in rank order
  for (uint32_t i = tid; i < n; i += kBlock) {
    const uint32_t r = a.f.rank[i];
    if (r < K) S.src[r] = (uint16_t)i;
  }
  __syncthreads();
  uint32_t total = 0;
  {
    uint32_t len[kFlowFpt], mine = 0;
#pragma unroll
    for (uint32_t j = 0; j < kFlowFpt; ++j) {
      const uint32_t k = tid * kFlowFpt + j;
      len[j] = 0;
      if (k < K) {
        const uint32_t i = S.src[k], fs = S.fo[i], fe = S.fo[i + 1u];
        if (fs != kImgBadOff && fe != kImgBadOff && fs <= fe && fe - fs > (uint32_t)H) len[j] = fe - fs - (uint32_t)H;
        if (a.payload_src) a.payload_src[k] = i;
      }
      mine += len[j];
    }
    uint32_t run = block_exclusive_scan32(mine, &total, S.sw32);
#pragma unroll
    for (uint32_t j = 0; j < kFlowFpt; ++j) {
      const uint32_t k = tid * kFlowFpt + j;
      if (k >= K) break;
      S.po[k] = run;
      a.payload_off[k] = run;
      run += len[j];
    }
    if (tid == 0) {
      S.po[K] = total;
      a.payload_off[K] = total;
    }
  }

  // 5. the replies and the closing datagrams
  rf_tail<H>(a, n, A, S.sw32);
  __syncthreads();  // po[] complete

  // 6. the message out of the image;  7. info and status
  const bool fits = total <= a.payload_cap;
  if (fits && total)
    image_copy_ranked(S.img, S.po, K, total, a.payload, kBlock,
                      [&](uint32_t q) { return S.fo[S.src[q]] + (uint32_t)H; });
  if (tid == 0) {
    a.info[8] = total;
    a.info[9] = a.info[10] = a.info[11] = 0;
    *a.status = (S.bad ? RUDP_ST_OFFSETS : 0u) | (L.bad ? RUDP_ST_FLOW : 0u) | (fits ? 0u : RUDP_ST_PAYLOAD_CAP);
  }
}

bool receive_flows_fused_ok(uint64_t n, uint64_t frames_bytes) {
  if (n == 0) return true;
  const int knob = tuning().receive_flows_fused;  // (2, diagnostics build: whatever the mean frame length)
  return knob && n <= kFlowMax && frames_bytes <= kRfFusedBytes &&
         (knob == 2 || frames_bytes <= (uint64_t)kRfFusedMeanFrame * n);
}

int launch_receive_flows_fused(const RecvFlowsArgs& a, hipStream_t stream) {
  if (a.H == 7u) hipLaunchKernelGGL(receive_flows_fused_kernel<7>, dim3(1), dim3(kBlock), 0, stream, a);
  else hipLaunchKernelGGL(receive_flows_fused_kernel<5>, dim3(1), dim3(kBlock), 0, stream, a);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------- chained form

// Behind the existing launches: the replies, the closing datagrams,
// info[8..11] and the three status words merged into the caller's.
template <int H>
__global__ void __launch_bounds__(kBlock) receive_flows_finish_kernel(RecvFlowsArgs a) {
  __shared__ uint32_t s_wave32[kBlock / 64];
  const uint32_t n = (uint32_t)a.f.n;  // (1 <= n <= kFlowMax)
  const uint32_t A = a.info[0] < n ? (uint32_t)a.info[0] : n;
  const uint32_t K = a.info[1] < n ? (uint32_t)a.info[1] : n;
  rf_tail<H>(a, n, A, s_wave32);
  if (threadIdx.x == 0) {
    a.info[8] = a.payload_off[K];
    a.info[9] = a.info[10] = a.info[11] = 0;
    *a.status = (a.words[0] & RUDP_ST_OFFSETS) | (a.words[1] & RUDP_ST_FLOW) | (a.words[2] & RUDP_ST_PAYLOAD_CAP);
  }
}

int launch_receive_flows_finish(const RecvFlowsArgs& a, hipStream_t stream) {
  if (a.H == 7u) hipLaunchKernelGGL(receive_flows_finish_kernel<7>, dim3(1), dim3(kBlock), 0, stream, a);
  else hipLaunchKernelGGL(receive_flows_finish_kernel<5>, dim3(1), dim3(kBlock), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace rudp
