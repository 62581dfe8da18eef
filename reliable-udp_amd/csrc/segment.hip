// A UTF-8 message cut into datagrams on the device (rudp_segment_utf8): the
// sender's loop of utils/reliableUDP.py:44-60 -- slices of chunk_chars
// *characters*, seq = ISN + character pointer, ack 0, SYN on the first frame
// and FIN on the last -- as the packed rudp_batch the varlen encode takes.
//
// A character starts at every lead byte ((b & 0xC0) != 0x80); packet k >= 1
// starts at the lead byte of character k * chunk_chars, packet 0 at byte 0.
//
// Reduce-then-scan over tiles of the message, as gather.hip:
//   1. lead bytes per tile (16-B loads, a 16-bit lead mask per vector, popcount);
//   2. one workgroup turns the counts into exclusive character bases in place
//      and writes d_count and the status word (the capacity check);
//   3. one workgroup per tile rescans it in rounds of 256 vectors and finds
//      the byte position of every lead byte whose character index is a
//      multiple of chunk_chars: start[k].  A round's starts are consecutive
//      packets, staged in LDS.  Then one of two forms of len[]:
//      differences (any chunk_chars): the starts go out as one run, to
//        d_payload_off when the caller wants the offsets, else to the stream's
//        scratch, and
//   4.   one thread per packet writes len = start[k + 1] - start[k] (the last
//        packet ends at msg_bytes), seq, ack, flags and the RUDP_ST_LEN check;
//      apron (chunk_chars <= 16, the shipped choice there: 22% less time at 1M
//        one-character datagrams): the tile pass writes whole rows.  A round's
//        packets end at the next start of the round; its last one ends at a
//        lead byte behind the round, which for valid UTF-8 lies in the next 64
//        bytes (16 characters of 4 bytes): one byte per lane of the first wave
//        and a ballot.  A packet that ends past the apron (invalid UTF-8 only)
//        is closed by a workgroup-wide search of at most 17 rounds, after
//        which it is longer than 65535 bytes and the call's status says so.
//        No fourth launch, no start[] traffic without d_payload_off.
// With RUDP_ST_PACKETS_CAP launches 3 and 4 write nothing.
//
// The message is read as whole aligned 16-B blocks from the boundary at or
// below its first byte; the bytes of a block outside the message are masked
// out of its lead mask.
#include "codec_device.hpp"
#include "internal.hpp"
#include "scan_device.hpp"

namespace RUDP_NS {

constexpr uint32_t kSegRoundBytes = 4096;   // one round: a 16-B vector per thread
constexpr uint32_t kSegTileBytes = 4096;    // a tile: one round (more for long messages, launch_segment_utf8)
constexpr uint64_t kSegMaxTiles = 16384;    // tiles double up to kSegMaxRounds rounds while there are more
constexpr uint32_t kSegMaxRounds = 16;

// Lead mask of the aligned block at byte A of the aligned buffer (A < E =
// mis + msg_bytes): bit i is byte A + i, bytes outside [mis, E) cleared.
__device__ __forceinline__ uint32_t seg_lead_mask(const SegmentArgs& a, uint64_t A, uint64_t E) {
  const u32x4 v = *reinterpret_cast<const u32x4*>(a.msg + A);
  uint32_t m = lead_mask16(v);
  const uint32_t lo = A < a.mis ? (uint32_t)(a.mis - A) : 0u;  // (only block 0)
  const uint32_t hi = E - A < 16u ? (uint32_t)(E - A) : 16u;
  m &= (0xFFFFu >> (16u - hi)) & (0xFFFFu << lo);
  return m;
}

// U: rounds whose loads are in flight together (rounds % U == 0).
template <uint32_t U>
__global__ void __launch_bounds__(kBlock) segment_counts_kernel(SegmentArgs a, uint64_t* counts) {
  __shared__ uint64_t s_wave[kBlock / 64];
  const uint64_t E = a.mis + a.bytes;
  const uint64_t t0 = (uint64_t)blockIdx.x * a.rounds * kSegRoundBytes + threadIdx.x * 16u;
  uint32_t cnt = 0;
  for (uint32_t r = 0; r < a.rounds; r += U) {
    uint32_t m[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      const uint64_t A = t0 + (uint64_t)(r + u) * kSegRoundBytes;
      m[u] = A < E ? seg_lead_mask(a, A, E) : 0u;
    }
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) cnt += __popc(m[u]);
  }
  const uint64_t w = wave_sum64(cnt);
  if ((threadIdx.x & 63u) == 0) s_wave[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t t = 0;
    for (uint32_t i = 0; i < kBlock / 64; ++i) t += s_wave[i];
    counts[blockIdx.x] = t;
  }
}

// One workgroup of 1024 threads: counts[t] <- sum_{u<t} counts[u]; d_count and
// the status word.
__global__ void __launch_bounds__(1024) segment_bases_kernel(uint64_t* counts, uint64_t nt, SegmentArgs a) {
  __shared__ uint64_t s_wave[1024 / 64];
  const uint64_t per = (nt + 1023) / 1024;
  const uint64_t lo = threadIdx.x * per < nt ? threadIdx.x * per : nt, hi = lo + per < nt ? lo + per : nt;
  uint64_t mine = 0;
  for (uint64_t i = lo; i < hi; ++i) mine += counts[i];
  uint64_t total = 0;
  uint64_t run = block_exclusive_scan(mine, &total, s_wave);
  for (uint64_t i = lo; i < hi; ++i) {
    const uint64_t v = counts[i];
    counts[i] = run;
    run += v;
  }
  if (threadIdx.x == 0) {
    const uint64_t packets = total ? (total + a.chunk - 1u) / a.chunk : 1ull;
    a.count[0] = packets;
    a.count[1] = total;
    *a.status = packets > a.max_packets ? RUDP_ST_PACKETS_CAP : 0u;
  }
}

constexpr uint64_t kSegNone = ~0ull;
constexpr uint32_t kSegApron = 64;  // bytes behind a round the apron form looks at first: 16 characters of 4 bytes

// One table row (the last pass of the differences form, the tile pass of the apron form).
__device__ __forceinline__ void seg_write_row(const SegmentArgs& a, uint64_t k, uint64_t packets, uint64_t s,
                                              uint64_t e) {
  const uint64_t len = e - s;
  a.len[k] = (uint32_t)(len > 0xFFFFFFFFull ? 0xFFFFFFFFull : len);
  a.seq[k] = (uint16_t)((uint64_t)a.isn + k * a.chunk);
  a.ack[k] = 0;
  a.flags[k] = (uint8_t)((k == 0 ? 0x80u : 0u) | (k + 1u == packets ? 0x20u : 0u));
  if (len > kMaxPayload) atomicOr(a.status, RUDP_ST_LEN);
}

// The aligned-buffer position of the lead byte of rank `need` at or after `pos`
// (a multiple of 16), for the whole workgroup: E when the message ends first,
// kSegNone when it is not within 17 rounds (a packet that started before `pos`
// then exceeds 65535 bytes).  Only invalid UTF-8 gets here: the apron finds
// every other end.
__device__ inline uint64_t seg_find_lead(const SegmentArgs& a, uint64_t pos, uint64_t E, uint32_t need,
                                         uint32_t* s_wave, unsigned long long* s_end) {
  for (uint32_t it = 0; it < 17u; ++it, pos += kSegRoundBytes) {
    if (pos >= E) return E;  // (uniform)
    const uint64_t A = pos + threadIdx.x * 16u;
    const uint32_t m = A < E ? seg_lead_mask(a, A, E) : 0u;
    const uint32_t pc = __popc(m);
    uint32_t tot = 0;
    const uint32_t ex = block_exclusive_scan32(pc, &tot, s_wave);
    if (need < tot) {  // (uniform)
      if (ex <= need && need < ex + pc) {
        uint32_t mm = m;
        for (uint32_t j = ex; j < need; ++j) mm &= mm - 1u;
        *s_end = A + (uint32_t)__builtin_ctz(mm);
      }
      __syncthreads();
      return *s_end;
    }
    need -= tot;
  }
  return kSegNone;
}

// ROWS false: the differences form, start[k] for the last pass.  ROWS true: the
// apron form, whole rows from here: a round's packets end at the next start in
// the round, its last one at the lead byte found in the 64 bytes behind the
// round (one byte per lane of the first wave), else by seg_find_lead.
template <uint32_t U, bool ROWS>
__global__ void __launch_bounds__(kBlock) segment_tile_kernel(SegmentArgs a, const uint64_t* bases) {
  __shared__ uint32_t s_wave[kBlock / 64];
  __shared__ uint16_t s_st[kSegRoundBytes];  // a round's starts: byte in the round, in packet order
  __shared__ unsigned long long s_end;       // ROWS: where the round's last packet ends (aligned-buffer position)
  if (*a.status & RUDP_ST_PACKETS_CAP) return;  // (uniform)
  const uint32_t tid = threadIdx.x, chunk = a.chunk;
  const uint64_t E = a.mis + a.bytes;
  const uint64_t packets = ROWS ? a.count[0] : 0;
  if (ROWS && a.count[1] == 0) {  // (uniform) no lead byte: one packet of all bytes, and no tile has a start
    if (blockIdx.x == 0 && tid == 0) {
      seg_write_row(a, 0, 1, 0, a.bytes);
      if (a.payload_off) a.payload_off[0] = 0, a.payload_off[1] = a.bytes;
    }
    return;
  }
  const uint64_t T0 = (uint64_t)blockIdx.x * a.rounds * kSegRoundBytes;
  // character c of the message starts packet c / chunk when c % chunk == 0; inside
  // the tile characters are counted from kr = (characters before it) % chunk
  const uint64_t cb = bases[blockIdx.x];
  const uint64_t kq = cb / chunk;
  uint32_t run = (uint32_t)(cb % chunk);  // (< 16383 + 65536 characters of a tile)
  for (uint32_t r = 0; r < a.rounds; r += U) {
    if (T0 + (uint64_t)r * kSegRoundBytes >= E) break;  // (uniform)
    uint32_t m[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      const uint64_t A = T0 + (uint64_t)(r + u) * kSegRoundBytes + tid * 16u;
      m[u] = A < E ? seg_lead_mask(a, A, E) : 0u;
    }
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      const uint32_t pc = __popc(m[u]);
      uint32_t tot = 0;
      // (the scan's barriers also order the previous round's reads of s_st before this round's writes)
      const uint32_t c0 = run + block_exclusive_scan32(pc, &tot, s_wave);  // this vector's first character
      const uint32_t k_round = (run + chunk - 1u) / chunk;  // ceil: the round's first start is packet kq + k_round
      const uint32_t k_vec = (c0 + chunk - 1u) / chunk;
      uint32_t next = k_vec * chunk - c0;  // rank in the vector of its first start
      if (next < pc) {
        uint32_t slot = k_vec - k_round, rank = 0;
        for (uint32_t mm = m[u]; mm; mm &= mm - 1u, ++rank) {
          if (rank == next) {
            s_st[slot++] = (uint16_t)(tid * 16u + (uint32_t)__builtin_ctz(mm));
            next += chunk;
          }
        }
      }
      __syncthreads();
      const uint32_t np = (run + tot + chunk - 1u) / chunk - k_round;
      const uint64_t R0 = T0 + (uint64_t)(r + u) * kSegRoundBytes - a.mis;  // (mod 2^64: a start is >= mis)
      if (!ROWS) {
        for (uint32_t i = tid; i < np; i += kBlock) {
          const uint64_t k = kq + k_round + i;
          // packet 0 starts at byte 0, wherever the first lead byte is
          if (k != 0 && k < a.max_packets) a.starts[k] = R0 + s_st[i];
        }
      } else if (np) {  // (uniform)
        // the round's last packet ends at the lead byte of rank `need` behind the round
        const uint64_t Rend = T0 + (uint64_t)(r + u + 1u) * kSegRoundBytes;
        const uint32_t need = (k_round + np) * chunk - (run + tot);  // (< chunk)
        if (tid < 64u) {
          const uint64_t g = Rend + tid;
          const bool lead = g < E && (a.msg[g] & 0xC0u) != 0x80u;
          const uint64_t bal = __ballot(lead);
          if (lead && (uint32_t)__popcll(bal & ((1ull << tid) - 1ull)) == need) s_end = g;
          if (tid == 0 && (uint32_t)__popcll(bal) <= need) s_end = Rend + kSegApron >= E ? E : kSegNone;
        }
        __syncthreads();
        uint64_t end = s_end;
        if (end == kSegNone) {  // (uniform)
          __syncthreads();  // (every read of s_end before seg_find_lead writes it)
          end = seg_find_lead(a, Rend, E, need, s_wave, &s_end);
          if (end == kSegNone) {
            if (tid == 0) atomicOr(a.status, RUDP_ST_LEN);
            end = E;
          }
        }
        for (uint32_t i = tid; i < np; i += kBlock) {
          const uint64_t k = kq + k_round + i;
          if (k >= a.max_packets) continue;
          // packet 0 starts at byte 0, wherever the first lead byte is
          const uint64_t s0 = k ? R0 + s_st[i] : 0ull;
          const uint64_t e0 = i + 1u < np ? R0 + s_st[i + 1u] : end - a.mis;
          seg_write_row(a, k, packets, s0, e0);
          if (a.payload_off) {
            a.payload_off[k] = s0;
            if (k + 1u == packets) a.payload_off[packets] = a.bytes;
          }
        }
      }
      run += tot;
    }
  }
}

__global__ void __launch_bounds__(kBlock) segment_rows_kernel(SegmentArgs a) {
  if (*a.status & RUDP_ST_PACKETS_CAP) return;
  const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t packets = a.count[0];
  if (k >= packets || k >= a.max_packets) return;
  // (entries 0 and `packets` of the starts are never read: they are written here when the caller wants them)
  const uint64_t s = k ? a.starts[k] : 0ull;
  const uint64_t e = k + 1u < packets ? a.starts[k + 1u] : a.bytes;
  seg_write_row(a, k, packets, s, e);
  if (a.payload_off) {
    if (k == 0) a.payload_off[0] = 0;
    if (k + 1u == packets) a.payload_off[packets] = a.bytes;
  }
}

int launch_segment_utf8(SegmentArgs a, hipStream_t stream) {
  // Tiles of one round: 1M one-character datagrams took 16.5 us (ASCII) and
  // 14.8 us (1-4-byte characters) against 33.3 and 24.4 with four rounds a tile
  // and 104 and 65.9 with sixteen (a 1 MB message is 64 tiles of 16 KiB on 256
  // CUs).  A message of more than 16384 tiles takes tiles of 2, 4, 8 or 16
  // rounds, which keeps the one-workgroup bases pass short: 1.5 GB measured the
  // same from every starting size (profiles/r08/segment.json).
  const uint64_t span = a.bytes ? a.mis + a.bytes : 0;
  const int knob = tuning().segment_rounds;
  a.rounds = knob == 1 || knob == 2 || knob == 4 || knob == 8 || knob == 16 ? (uint32_t)knob
                                                                            : kSegTileBytes / kSegRoundBytes;
  uint64_t nt = (span + (uint64_t)a.rounds * kSegRoundBytes - 1u) / ((uint64_t)a.rounds * kSegRoundBytes);
  while (nt > kSegMaxTiles && a.rounds < kSegMaxRounds) {
    a.rounds *= 2u;
    nt = (nt + 1u) / 2u;
  }
  // the most packets a message of this many bytes can have, at most max_packets:
  // the rows the last pass covers and the starts the scratch holds
  const uint64_t bound = a.bytes ? (a.bytes + a.chunk - 1u) / a.chunk : 1u;
  const uint64_t rows = a.max_packets < bound ? a.max_packets : bound;
  const uint64_t nb = (rows + kBlock - 1u) / kBlock;
  if (nt > 0x7FFFFFFFull || nb > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
  // The apron form (whole rows from the tile pass) for chunks whose every valid
  // packet ends within the 64-byte apron: interleaved at 1M one-character
  // datagrams 21.3 -> 16.7 us (ASCII) and 19.4 -> 14.9 (1-4-byte characters;
  // profiles/r08/segment.json).  An empty message has no tile.
  const bool apron = tuning().segment_apron && a.chunk * 4u <= kSegApron && nt;
  uint64_t* counts = nullptr;
  hipError_t e = stream_scratch(reinterpret_cast<void**>(&counts), (nt ? nt : 1u) * sizeof(uint64_t), stream,
                                kScratchSums);
  if (e != hipSuccess) return (int)e;
  a.starts = a.payload_off;
  if (rows && !a.starts && !apron) {
    e = stream_scratch(reinterpret_cast<void**>(&a.starts), (rows + 1u) * sizeof(uint64_t), stream, kScratchRecords);
    if (e != hipSuccess) return (int)e;
  }
  const bool u4 = a.rounds % 4u == 0;  // four rounds' loads in flight where a tile has them
  const dim3 grid((uint32_t)nt), block(kBlock);
  if (nt) {
    if (u4) hipLaunchKernelGGL(segment_counts_kernel<4>, grid, block, 0, stream, a, counts);
    else hipLaunchKernelGGL(segment_counts_kernel<1>, grid, block, 0, stream, a, counts);
  }
  hipLaunchKernelGGL(segment_bases_kernel, dim3(1), dim3(1024), 0, stream, counts, nt, a);
  if (rows && apron) {
    if (u4) hipLaunchKernelGGL((segment_tile_kernel<4, true>), grid, block, 0, stream, a, counts);
    else hipLaunchKernelGGL((segment_tile_kernel<1, true>), grid, block, 0, stream, a, counts);
  } else if (rows) {
    if (nt) {
      if (u4) hipLaunchKernelGGL((segment_tile_kernel<4, false>), grid, block, 0, stream, a, counts);
      else hipLaunchKernelGGL((segment_tile_kernel<1, false>), grid, block, 0, stream, a, counts);
    }
    hipLaunchKernelGGL(segment_rows_kernel, dim3((uint32_t)nb), block, 0, stream, a);
  }
  return (int)hipGetLastError();
}

}  // namespace rudp
