// A datagram batch as an LDS image, shared by the fused kernels of
// rudp_receive, rudp_receive_window and rudp_acknowledge: the buffer goes into
// LDS once, with aligned 16-B loads from the boundary at or below its pointer,
// and every later step reads that image -- one lane decodes one frame, and the
// kept bytes leave as 16-B chunks of the output's own alignment.  The reply
// datagram writer of the two receivers is here too.
#pragma once
#include "codec_device.hpp"
#include "internal.hpp"
#include "utf8_device.hpp"

namespace RUDP_NS {

constexpr uint32_t kImgBadOff = 0xFFFFFFFFu;  // a frame offset the offset rule rejects, in the LDS tables

// `bytes` of the aligned buffer `src` into the image by the workgroup's B
// threads, four loads in flight each; the last vector's bytes past `bytes` are
// zero.
__device__ __forceinline__ void image_load(uint32_t* img, const unsigned char* src, uint32_t bytes, uint32_t B) {
  const uint32_t nvec = (bytes + 15u) >> 4;
  u32x4* dst = reinterpret_cast<u32x4*>(img);
  for (uint32_t v0 = threadIdx.x; v0 < nvec; v0 += 4u * B) {
    u32x4 r[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u)
      if (v0 + u * B < nvec) r[u] = load16_guarded(src, 16ull * (v0 + u * B), bytes);
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u)
      if (v0 + u * B < nvec) dst[v0 + u * B] = r[u];
  }
}

// fo[0..n]: the frame offsets as image positions (the caller's frames[0] is
// image byte fmis), kImgBadOff for one past frames_bytes.
__device__ __forceinline__ void image_offsets(uint32_t* fo, const uint64_t* frame_off, uint32_t n,
                                              uint64_t frames_bytes, uint64_t fmis, uint32_t B) {
  for (uint32_t k = threadIdx.x; k <= n; k += B) {
    const uint64_t o = frame_off[k];
    fo[k] = o <= frames_bytes ? (uint32_t)(o + fmis) : kImgBadOff;
  }
}

struct FrameDecode {
  uint32_t seq, ack, fl, ok, cs;
  uint32_t valid, chars;  // TEXT: the strict UTF-8 verdict and the lead bytes of the payload; else 0
};

// Frame [fs, fe) of the image `dw` by one lane: header, RFC 1071 sum and the
// checksum verdict (H 5: against the sideband when there is one; want() gives
// the caller's, and is asked only where the verdict needs it: loaded ahead of
// the decode it made every lane wait for the stores of the frame before).  A
// frame whose offsets are rejected is RUDP_OK_BAD_OFFSETS and nothing of it is
// read.
template <int H, bool TEXT, typename Want>
__device__ __forceinline__ FrameDecode image_decode_frame(const uint32_t* dw, uint32_t fs, uint32_t fe, bool has_want,
                                                          Want want) {
  FrameDecode d{0, 0, 0, RUDP_OK_BAD_OFFSETS, 0, 0, 0};
  if (fs == kImgBadOff || fe == kImgBadOff || fs > fe) return d;
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
      ev = even_bytes_acc(v, ev);
      od = odd_bytes_acc(v, od);
      if (TEXT) {
        hib |= v;
        d.chars += __popc(lead4(v) & lanes);
      }
    }
  }
  if (TEXT) {
    const unsigned char* ib = reinterpret_cast<const unsigned char*>(dw);
    d.valid = (hib & 0x80808080u) && utf8_check_bytes(ps, fe, [&](uint32_t i) { return (uint32_t)ib[i]; }) ? 0u : 1u;
  }
  const uint32_t sum = (fs & 1u) ? (ev + (od << 8)) : ((ev << 8) + od);
  const u32x4 h = window16_dw(dw, fs);
  const uint32_t b0 = h.x & 0xFFu, b1 = (h.x >> 8) & 0xFFu, b2 = (h.x >> 16) & 0xFFu, b3 = h.x >> 24,
                 b4 = h.y & 0xFFu, b5 = (h.y >> 8) & 0xFFu, b6 = (h.y >> 16) & 0xFFu;
  if (F < (uint32_t)H) {  // short frame: fields truncated as utils/packet.py:31 slices them
    const uint32_t c0 = F > 0 ? b0 : 0u, c1 = F > 1 ? b1 : 0u, c2 = F > 2 ? b2 : 0u, c3 = F > 3 ? b3 : 0u,
                   c4 = F > 4 ? b4 : 0u;
    d.seq = F >= 2 ? (c0 << 8) | c1 : c0;
    d.ack = F >= 4 ? (c2 << 8) | c3 : c2;
    d.fl = c4;
    d.ok = RUDP_OK_SHORT;
  } else {
    d.seq = (b0 << 8) | b1;
    d.ack = (b2 << 8) | b3;
    d.fl = b4;
    d.cs = packet_csum(sum, d.seq, d.ack, d.fl);
    if (H == 7) d.ok = d.cs == ((b5 << 8) | b6) ? RUDP_OK_GOOD : RUDP_OK_BAD_CSUM;
    else d.ok = has_want ? (d.cs == want() ? RUDP_OK_GOOD : RUDP_OK_BAD_CSUM) : RUDP_OK_UNVERIFIED;
  }
  return d;
}

// The K ranked byte runs [0, total) out of the image to `o`, dealt over the
// `stride` threads of the workgroup as the 16-B chunks of o's own alignment: a
// whole chunk is one 16-B store, the partial chunk at either end goes
// bytewise, so no store covers a byte outside [0, total).  po[0..K]: the runs'
// offsets in the output (po[K] = total); pos(q): the image position of rank
// q's first byte, asked only for a rank with bytes.
template <typename Pos>
__device__ __forceinline__ void image_copy_ranked(const uint32_t* img_dw, const uint32_t* po, uint32_t K,
                                                  uint32_t total, unsigned char* o, uint32_t stride, Pos pos) {
  const unsigned char* img = reinterpret_cast<const unsigned char*>(img_dw);
  const uint32_t lead = (uint32_t)(-(uintptr_t)o) & 15u;  // bytes before the first aligned chunk
  const uint32_t nch = total > lead ? (total - lead + 15u) / 16u + 1u : 1u;  // chunk 0 is the head [0, lead)
  for (uint32_t c = threadIdx.x; c < nch; c += stride) {
    const int x = c == 0 ? (int)lead - 16 : (int)(lead + 16u * (c - 1u));
    const int b_lo = x < 0 ? -x : 0;
    const int b_hi = (uint32_t)(x + 16) <= total ? 16 : (int)total - x;
    if (b_hi <= b_lo) continue;
    uint32_t y = (uint32_t)(x + b_lo);
    // the rank of output byte y: the last q with po[q] <= y (po[0] = 0 <= y < total = po[K])
    uint32_t q = 0, qh = K;
    while (qh - q > 1u) {
      const uint32_t m = (q + qh) >> 1;
      if (po[m] <= y) q = m; else qh = m;
    }
    uint64_t lo = 0, hi = 0;
    for (int b = b_lo; b < b_hi; ++b, ++y) {
      while (po[q + 1u] <= y) ++q;  // (y < po[K]: stops at a rank with bytes)
      const uint64_t v = img[pos(q) + (y - po[q])];
      if (b < 8) lo |= v << (8 * b); else hi |= v << (8 * (b - 8));
    }
    if (b_lo == 0 && b_hi == 16) {
      *reinterpret_cast<u32x4*>(o + x) = make_u32x4(lo, hi);
    } else {
      for (int b = b_lo; b < b_hi; ++b) o[x + b] = (unsigned char)(b < 8 ? lo >> (8 * b) : hi >> (8 * (b - 8)));
    }
  }
}

// Where the reply datagrams of a call go (ReceiveArgs and RecvWindowArgs both fill it).
struct ReplyOut {
  unsigned char* frames;  // [slots * H]
  uint16_t* csum;         // may be null
  uint32_t* index;
  uint64_t* peer;
  uint64_t n;             // the batch's frames: the peer of a reply with no reset before it
};

// Reply `slot`: the send_ack packet for datagram i, and its tables.  r: 1 +
// the index of the last reset at or before i (0: none in this batch).
template <int H>
__device__ __forceinline__ void put_reply(const ReplyOut& out, uint64_t slot, uint64_t i, uint32_t ack, uint64_t r) {
  const uint32_t c = packet_csum(0u, 0u, ack, 0x40u);
  const uint64_t h = pack_header<H>(0u, ack, 0x40u, c);
  unsigned char* o = out.frames + slot * (uint64_t)H;
#pragma unroll
  for (int b = 0; b < H; ++b) o[b] = (unsigned char)(h >> (8 * b));
  if (out.csum) out.csum[slot] = (uint16_t)c;
  out.index[slot] = (uint32_t)i;
  out.peer[slot] = r ? r - 1u : out.n;
}

}  // namespace rudp
