// The device functions of the packed payload copy-out (gather.hip states the
// edge rule and where the windows come from): a frame's payload length under
// the offset rule and the chunk copy of one tile's output run.  gather.hip's
// tiles are runs of frames, ordered.hip's runs of ranks.
#pragma once
#include "codec_device.hpp"
#include "internal.hpp"

namespace RUDP_NS {

constexpr uint32_t kGatherGuard = 32;            // LDS bytes before and after a staged run (window16_dw's reach)
constexpr int kGatherBadShift = 63;               // a tile sum's bit 63: a frame of the block failed the offset rule
constexpr uint64_t kGatherSumMask = (1ull << kGatherBadShift) - 1ull;
// Totals saturate here (no payload buffer is this large): sums of frames that
// overlap (valid pairs of unordered offsets) cannot wrap past payload_cap.
constexpr uint64_t kGatherSat = 1ull << 53;

// Payload bytes frame [fo0, fo1) contributes; *bad set when its offsets are rejected.
__device__ __forceinline__ uint64_t gather_plen(uint64_t fo0, uint64_t fo1, uint64_t lim, uint32_t H, bool kept,
                                                uint32_t* bad) {
  if (fo0 > fo1 || fo1 > lim) {
    *bad = 1u;
    return 0;
  }
  const uint64_t f = fo1 - fo0;
  return kept && f > H ? f - H : 0ull;
}

// load16_guarded with a plain (cached) load: the HBM path reads every aligned
// block from two neighbouring lanes, and the second read is to hit in cache.
__device__ __forceinline__ u32x4 gather_load16(const unsigned char* frames, uint64_t off, uint64_t total) {
  if (off + 16 <= total) return *reinterpret_cast<const u32x4*>(frames + off);
  return load16_guarded(frames, off, total);
}

// The tile's output run [0, total) at `o`, dealt as the 16-B chunks of o's own
// alignment over the workgroup.  LDS: windows from the staged run (`img_dw`,
// whose byte kGatherGuard is byte gA of the aligned frames buffer); else from HBM.
template <bool LDS>
__device__ __forceinline__ void gather_chunks(const GatherArgs& a, const uint64_t* s_fo, const uint64_t* s_po,
                                              uint32_t Rv, uint64_t total, unsigned char* o, const uint32_t* img_dw,
                                              uint64_t gA) {
  const uint32_t lead = (uint32_t)(-(uintptr_t)o) & 15u;  // bytes before the run's first aligned chunk
  const uint64_t nch = total > lead ? (total - lead + 15u) / 16u + 1u : 1u;  // chunk 0 is the head [0, lead)
  const uint64_t src0 = a.fmis + a.H;
  const uint64_t lim = a.fmis + a.frames_bytes;
  for (uint64_t c = threadIdx.x; c < nch; c += kBlock) {
    // chunk c covers run bytes [x, x + 16) of which [b_lo, b_hi) are the tile's
    const int64_t x = c == 0 ? (int64_t)lead - 16 : (int64_t)(lead + 16u * (c - 1u));
    const int b_lo = x < 0 ? (int)-x : 0;
    const int b_hi = (uint64_t)(x + 16) <= total ? 16 : (int)((int64_t)total - x);
    if (b_hi <= b_lo) continue;
    const uint64_t y = (uint64_t)(x + b_lo);
    // the frame of run byte y: the last q with s_po[q] <= y (s_po[0] = 0 <= y < total = s_po[Rv])
    uint32_t q = 0, qh = Rv;
    while (qh - q > 1u) {
      const uint32_t m = (q + qh) >> 1;
      if (s_po[m] <= y) q = m; else qh = m;
    }
    uint64_t j = y - s_po[q];
    uint64_t lo = 0, hi = 0;
    for (int b = b_lo; b < b_hi; ++q, j = 0) {
      const uint64_t left = s_po[q + 1] - s_po[q] - j;  // (0: a dropped, rejected or empty frame)
      if (left == 0) continue;
      const int take = left < (uint64_t)(b_hi - b) ? (int)left : b_hi - b;
      // chunk byte b is payload q's byte j, byte s_fo[q] + src0 + j of the aligned buffer
      u32x4 w;
      if (LDS) {
        w = window16_dw(img_dw, kGatherGuard + (uint32_t)(s_fo[q] + src0 - gA) + (uint32_t)j - (uint32_t)b);
      } else {
        const int64_t pos = (int64_t)(s_fo[q] + src0 + j) - b;  // (>= -15)
        const int64_t blk = pos & ~(int64_t)15;
        const uint32_t sh = (uint32_t)(pos & 15);
        const u32x4 zero = {0u, 0u, 0u, 0u};
        const u32x4 w0 = blk >= 0 ? gather_load16(a.frames, (uint64_t)blk, lim) : zero;
        const u32x4 w1 = sh ? gather_load16(a.frames, (uint64_t)(blk + 16), lim) : zero;
        w = funnel32(w0, w1, sh);
      }
      lo |= lo64(w) & byte_mask(b, b + take);
      hi |= hi64(w) & byte_mask(b - 8, b + take - 8);
      b += take;
    }
    if (b_lo == 0 && b_hi == 16) {
      __builtin_nontemporal_store(make_u32x4(lo, hi), reinterpret_cast<u32x4*>(o + x));
    } else {
      for (int b = b_lo; b < b_hi; ++b) o[x + b] = (unsigned char)(b < 8 ? lo >> (8 * b) : hi >> (8 * (b - 8)));
    }
  }
}

}  // namespace rudp
