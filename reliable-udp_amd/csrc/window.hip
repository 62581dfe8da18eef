// rudp_accept_window: the reordering receiver of a windowed sender -- the rule
// of rudp_accept_inorder with a pending set: a frame ahead of `expect` inside
// the window waits, and is delivered when the gap before it fills
// (include/rudp.h states the rule; tests/window_ref.py restates it as a loop
// and this file's steps as chunk_model).
//
// One workgroup of 1024 threads judges a chunk: the frames pending before it
// (at most window_chars - 1, their starts are distinct inside the window;
// for the first chunk the caller's carried frames) and up to 1024 new frames,
// at most 2047 items in arrival order.  Larger batches are one launch per
// chunk in stream order; the state, the ranks' base and the pending indices
// pass from launch to launch in the stream's scratch.
//
// A chunk, every reset segment at once (a reset's own seq + c is the expect its
// segment starts from, so no segment waits for the one before it):
//   1. classes as accept.hip, the segment of every item (a scan of resets);
//   2. the candidates -- usable non-SYN frames of a live segment with c > 0
//      and seq >= the segment's first expect -- sorted by (segment, seq,
//      arrival), a bitonic sort of 38-bit keys in LDS;
//   3. the first arrival of every start is its node; a node's successor is
//      the node that starts at seq + c (binary search), none behind a FIN; the
//      chain of every segment is what pointer doubling reaches from the node
//      that starts at the segment's first expect;
//   4. the chain elements in sorted order are in delivery order; the delivery
//      time of element k is the prefix maximum of the arrivals along the chain;
//   5. expect before and after item p = the end of the last chain element of
//      its segment delivered before / by p (a search per item): in-order,
//      ahead, reply_ack, ranks.  An item the guess cannot judge is an anomaly:
//      a frame at or beyond guess + window with c > 0, and an in-order frame
//      with c == 0.  Before the first anomaly the guess is the rule's state;
//   6. without an anomaly before the end: the state after the last judged item;
//   7. else one lane walks the rule from the exact state before the anomaly to
//      the chunk's end, the pending set an LDS ring of window_chars item
//      positions addressed by start mod window_chars;
//   8. outputs, the pending items' indices for the next chunk, and in the
//      last chunk d_state_out and d_info.
// A batch of more than one chunk ends with one pass that clears what lies
// behind `end` and the ranks before the last reset.
//
// The chunk's device function, win_judge_chunk, is in window_device.hpp, which
// receive_window.hip's fused kernel shares; this file has the two kernels and
// the launcher.
#include "window_device.hpp"

namespace RUDP_NS {

__global__ void __launch_bounds__(kWinBlock) accept_window_kernel(WindowArgs a) {
  __shared__ WinLds L;
  win_judge_chunk(a, L);
}

// More than one chunk: what lies behind `end` cleared, and the ranks of the
// frames delivered before the last reset.
__global__ void __launch_bounds__(256) accept_window_final_kernel(WindowArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= a.n) return;
  const uint64_t end = a.info[0], ms = a.info[2];
  if (i > end) {
    a.accept[i] = 0;
    a.rank[i] = RUDP_RANK_NONE;
    a.carry_rank[i] = RUDP_RANK_NONE;
    a.reply[i] = 0;
    a.reply_ack[i] = 0;
  } else if (ms < a.n && i < ms) {
    a.rank[i] = RUDP_RANK_NONE;
  }
}

int launch_accept_window(WindowArgs a, hipStream_t stream) {
  const uint64_t nnew = a.n - a.n_carried;
  a.chunks = nnew ? (nnew + kWinNew - 1u) / kWinNew : 1u;
  if (a.chunks > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
  hipError_t e = stream_scratch(reinterpret_cast<void**>(&a.hdr), kWinHdr * sizeof(uint64_t) + 1024u * sizeof(uint32_t),
                                stream, kScratchSums);
  if (e != hipSuccess) return (int)e;
  for (uint64_t c = 0; c < a.chunks; ++c) {
    a.chunk = c;
    hipLaunchKernelGGL(accept_window_kernel, dim3(1), dim3(kWinBlock), 0, stream, a);
  }
  if (a.chunks > 1u)
    hipLaunchKernelGGL(accept_window_final_kernel, dim3((uint32_t)((a.n + 255u) / 256u)), dim3(256), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace rudp
