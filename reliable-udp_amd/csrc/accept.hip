// The receiver's in-order acceptance of a datagram batch on the device:
// rudp_payload_chars (characters per payload) and rudp_accept_inorder (which
// datagrams receive_data of utils/reliableUDP.py:116-137 accepts, and the
// ack_num of the reply send_ack builds for each, :139-146).
//
// The rule, per frame i in arrival order, in absolute sequence space (state:
// expect = ISN + characters received, never reduced mod 2^16; isn; live):
//   ignored   !usable: nothing changes, no reply; a SYN whose seq equals
//             last_isn (a repeated SYN): nothing changes, a reply is sent;
//   reset     any other SYN: isn = seq, expect = seq + c, live = 1, accepted;
//   in-order  a non-SYN with live && seq == expect: accepted, expect += c;
//   else      not accepted.
// A reply goes out for every usable frame while live is set after it, with
// ack_num = expect after the frame mod 2^16.  The first accepted FIN ends the
// call's transfer; later frames are not judged.
//
// The parallel form.  expect never decreases between resets, so the state
// before every frame is guessed as a segmented prefix maximum of seq + c over
// the usable non-SYN frames, a reset restarting the segment with its own
// seq + c (AccP: m = the maximum, r = 1 + index of the last reset, 0 none;
// isn = seq[r - 1]).  Reduce-then-scan over tiles of 1024 frames as gather.hip:
//   1. the join of every tile;  2. one workgroup: exclusive tile bases, seeded
//   from d_state_in;  3. one workgroup per tile rescans it, writes accept,
//   reply and reply_ack under the guess and takes two minima: the first
//   accepted FIN, and the first anomaly, a live non-SYN frame with
//   seq != guess && seq + c > guess.  Before the first anomaly the guess is
//   the true state (the recurrence has one solution).
//   4. one workgroup finishes: without an anomaly before the FIN it rescans the
//   tile of the last judged frame for the state after it; else it takes the
//   exact state before the anomaly the same way and one lane walks the rule
//   from there, the frames staged through LDS in blocks of 1024, overwriting
//   accept and reply_ack up to the end it finds (reply does not depend on the
//   guess: resets are known without it).  It writes d_state_out and d_info.
//   5. keep, the count of accepted frames, and zeroes past the end.
// A batch of one tile (a recvmmsg batch is at most 1024 datagrams) runs the
// five steps in one launch.
//
// The device functions of the five steps are in accept_device.hpp, which
// receive.hip's fused kernel shares (it judges a tile it decoded into LDS
// itself); this file has payload_chars and the accept kernels and launchers.
#include "accept_device.hpp"

namespace RUDP_NS {

// ------------------------------------------------------------ payload_chars

// G = 1 << glog lanes per frame walk the aligned 16-B blocks of its payload
// [S, E) (positions in the aligned buffer), four loads in flight per lane; the
// bytes of a block outside the payload are masked out of its lead mask.
__global__ void __launch_bounds__(kBlock) payload_chars_kernel(CharsArgs a) {
  const uint32_t G = 1u << a.glog, lane = threadIdx.x & (G - 1u);
  const uint64_t i = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> a.glog;
  uint32_t cnt = 0;
  if (i < a.n) {
    const uint64_t fo0 = a.frame_off[i], fo1 = a.frame_off[i + 1];
    if (fo0 <= fo1 && fo1 <= a.frames_bytes && fo1 - fo0 > a.H) {
      const uint64_t S = a.fmis + fo0 + a.H, E = a.fmis + fo1;
      const uint64_t step = 16ull * G;
      for (uint64_t A = (S & ~15ull) + 16ull * lane; A < E; A += 4u * step) {
        u32x4 v[4];
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u)
          if (A + u * step < E) v[u] = *reinterpret_cast<const u32x4*>(a.frames + A + u * step);
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) {
          const uint64_t B = A + u * step;
          if (B < E) {
            const uint32_t lo = S > B ? (uint32_t)(S - B) : 0u;
            const uint32_t hi = E - B < 16u ? (uint32_t)(E - B) : 16u;
            cnt += __popc(lead_mask16(v[u]) & (0xFFFFu >> (16u - hi)) & (0xFFFFu << lo));
          }
        }
      }
    }
  }
  cnt = group_sum(cnt, G);  // (every lane of the wave is here)
  if (lane == 0 && i < a.n) a.chars[i] = cnt;
}

uint32_t payload_chars_glog(uint32_t len_hint, uint32_t H) {
  const int knob = tuning().chars_glog;
  if (knob >= 0 && knob <= 6) return (uint32_t)knob;
  // the fewest lanes, a power of two up to 64, that leave a lane at most four blocks
  const uint32_t blocks = (len_hint > H ? len_hint - H : 0u) / 16u + 1u;
  uint32_t glog = 0;
  while (glog < 6u && blocks > (4u << glog)) ++glog;
  return glog;
}

int launch_payload_chars(CharsArgs a, uint32_t len_hint, hipStream_t stream) {
  a.glog = payload_chars_glog(len_hint, a.H);
  const uint64_t per = kBlock >> a.glog;
  const uint64_t nb = (a.n + per - 1u) / per;
  if (nb > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(payload_chars_kernel, dim3((uint32_t)nb), dim3(kBlock), 0, stream, a);
  return (int)hipGetLastError();
}

// ----------------------------------------------------------- accept_inorder

// A batch of at most one tile, n == 0 included: every step in one launch.
__global__ void __launch_bounds__(kBlock) accept_single_kernel(AcceptArgs a) {
  __shared__ AccLds L;
  const uint32_t tid = threadIdx.x;
  const AccSeed seed{a.state_in[0], a.state_in[1], a.state_in[2] ? 1ull : 0ull};
  if (a.n == 0) {  // (uniform)
    acc_empty(a, seed);
    return;
  }
  if (tid == 0) {
    L.e_min = a.n;
    L.a_min = a.n;
    a.info[1] = 0;
  }
  acc_load(a, L, 0, (uint32_t)a.n);
  __syncthreads();
  acc_one_tile(a, L, seed);
}

__global__ void __launch_bounds__(kBlock) accept_join_kernel(AcceptArgs a) {
  __shared__ AccLds L;
  const uint64_t p0 = (uint64_t)blockIdx.x * kAccTile;
  const uint32_t Rv = a.n - p0 < kAccTile ? (uint32_t)(a.n - p0) : kAccTile;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.hdr[0] = a.state_in[0];
    a.hdr[1] = a.state_in[1];
    a.hdr[2] = a.state_in[2] ? 1ull : 0ull;
    a.hdr[3] = a.n;
    a.hdr[4] = a.n;
    a.info[1] = 0;
  }
  acc_load(a, L, p0, Rv);
  __syncthreads();
  const AccP t = acc_tile_join(a, L, p0, Rv);
  if (threadIdx.x == 0) {
    a.hdr[kAccHdr + 2u * blockIdx.x] = t.m;
    a.hdr[kAccHdr + 2u * blockIdx.x + 1u] = t.r;
  }
}

// One workgroup: pair[t] <- state_in's expect joined with the pairs before t,
// each thread over a run of consecutive tiles (one each up to 256 tiles).
__global__ void __launch_bounds__(kBlock) accept_bases_kernel(uint64_t* hdr, uint64_t nt) {
  __shared__ uint64_t wm[kBlock / 64], wr[kBlock / 64];
  uint64_t* pairs = hdr + kAccHdr;
  const uint64_t per = (nt + kBlock - 1u) / kBlock;
  const uint64_t lo = threadIdx.x * per < nt ? threadIdx.x * per : nt, hi = lo + per < nt ? lo + per : nt;
  AccP mine{0, 0};
  for (uint64_t i = lo; i < hi; ++i) mine = acc_join(mine, AccP{pairs[2u * i], pairs[2u * i + 1u]});
  AccP total;
  AccP run = acc_join(AccP{hdr[0], 0}, block_exclusive_join(mine, &total, wm, wr));
  for (uint64_t i = lo; i < hi; ++i) {
    const AccP v{pairs[2u * i], pairs[2u * i + 1u]};
    pairs[2u * i] = run.m;
    pairs[2u * i + 1u] = run.r;
    run = acc_join(run, v);
  }
}

__global__ void __launch_bounds__(kBlock) accept_tile_kernel(AcceptArgs a) {
  __shared__ AccLds L;
  const uint64_t p0 = (uint64_t)blockIdx.x * kAccTile;
  const uint32_t Rv = a.n - p0 < kAccTile ? (uint32_t)(a.n - p0) : kAccTile;
  if (threadIdx.x == 0) {
    L.e_min = a.n;
    L.a_min = a.n;
  }
  const AccP base{a.hdr[kAccHdr + 2u * blockIdx.x], a.hdr[kAccHdr + 2u * blockIdx.x + 1u]};
  const uint64_t seed_live = a.hdr[2];
  acc_load(a, L, p0, Rv);
  __syncthreads();
  acc_scan(a, L, p0, Rv, base, seed_live);
  __syncthreads();
  acc_store(a, L, p0, Rv);
  if (threadIdx.x == 0) {
    if (L.e_min < a.n) atomicMin(reinterpret_cast<unsigned long long*>(a.hdr + 3), L.e_min);
    if (L.a_min < a.n) atomicMin(reinterpret_cast<unsigned long long*>(a.hdr + 4), L.a_min);
  }
}

__global__ void __launch_bounds__(kBlock) accept_finish_kernel(AcceptArgs a) {
  __shared__ AccLds L;
  const AccSeed seed{a.hdr[0], a.hdr[1], a.hdr[2]};
  acc_finish(a, L, seed, a.hdr[3], a.hdr[4], a.hdr + kAccHdr);
}

__global__ void __launch_bounds__(kBlock) accept_final_kernel(AcceptArgs a) {
  __shared__ uint32_t s_count;
  acc_final(a, (uint64_t)blockIdx.x * kAccTile, a.info[0], a.info[2], &s_count);
}

int launch_accept_inorder(AcceptArgs a, hipStream_t stream) {
  if (a.n <= kAccTile && tuning().accept_single) {
    hipLaunchKernelGGL(accept_single_kernel, dim3(1), dim3(kBlock), 0, stream, a);
    return (int)hipGetLastError();
  }
  if (a.n == 0) {  // (the diagnostics build with the knob off)
    hipLaunchKernelGGL(accept_single_kernel, dim3(1), dim3(kBlock), 0, stream, a);
    return (int)hipGetLastError();
  }
  const uint64_t nt = (a.n + kAccTile - 1u) / kAccTile;
  if (nt > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
  hipError_t e = stream_scratch(reinterpret_cast<void**>(&a.hdr), (kAccHdr + 2u * nt) * sizeof(uint64_t), stream,
                                kScratchSums);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(accept_join_kernel, dim3((uint32_t)nt), dim3(kBlock), 0, stream, a);
  hipLaunchKernelGGL(accept_bases_kernel, dim3(1), dim3(kBlock), 0, stream, a.hdr, nt);
  hipLaunchKernelGGL(accept_tile_kernel, dim3((uint32_t)nt), dim3(kBlock), 0, stream, a);
  hipLaunchKernelGGL(accept_finish_kernel, dim3(1), dim3(kBlock), 0, stream, a);
  hipLaunchKernelGGL(accept_final_kernel, dim3((uint32_t)nt), dim3(kBlock), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace rudp
