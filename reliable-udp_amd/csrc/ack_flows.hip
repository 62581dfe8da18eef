// rudp_ack_flows: one reply batch judged for many transfers.  Every reply
// carries the slot of its peer's row {p, L, last, done, isn, T, C, sent} in a
// device table; per slot the rule is rudp_ack_progress' (acknowledge.hip states
// it, and its parallel form), applied to the slot's replies in arrival order
// with words 0 to 3 as the state and words 4 to 7 as the call's scalars, the
// slots independently.  A flow's first valid FIN ends it: done becomes 1 and
// its later replies are not judged.
//
// One launch of one workgroup of 256 threads, the whole batch (at most 1024
// replies) in LDS, no work proportional to the table:
//   1. the tables and d_flow into LDS; every reply reads words 4 to 7 of its
//      row: an idle row (C == 0) or a refused one leaves the reply without a
//      flow; the keys slot << 10 | arrival index, padded with all-ones to a
//      power of two;
//   2. a bitonic sort of the keys: every flow's replies become one run, in
//      arrival order, the runs by ascending slot, the rest last;
//   3. run heads and a block scan of the head flags: A, d_order, d_order_off,
//      every run's slot; one lane per run loads its row and tests the seed;
//   4. acknowledge.hip's one-scan form, segmented: the prefix maximum of the
//      candidates restarts at a run head from that row's p, so one block scan
//      guesses the p before every reply of every run; validity, candidacy and
//      the anomalies with the run's own isn, T, C and sent; per run its first
//      event by an LDS atomicMin: a valid FIN under the guess, or an anomaly;
//   5. one lane per run takes the run's final state from the scan (no loop);
//      a run whose first event is an anomaly, or whose seed is no canonical
//      state, is walked by the rule from there by its lane, such runs
//      concurrently (d_info[5] counts them); the lane writes the row;
//   6. the per-reply outputs and a block count of the valid replies;
//   7. a block count of the ended runs: the closing datagrams in flow order.
// The device functions are in ack_flows_device.hpp.
#include "ack_flows_device.hpp"

namespace RUDP_NS {

static_assert(kAfMax == RUDP_FLOWS_MAX_BATCH, "the kernel holds exactly one batch");
static_assert(sizeof(AckFlowLds) <= 65536, "static LDS: what a workgroup gets without asking");

template <int H>
__global__ void __launch_bounds__(kBlock) ack_flows_kernel(AckFlowsArgs a) {
  __shared__ AckFlowLds L;
  ack_flows_judge<H>(a, L);
}

int launch_ack_flows(const AckFlowsArgs& a, hipStream_t stream) {
  if (a.H == 7u) hipLaunchKernelGGL(ack_flows_kernel<7>, dim3(1), dim3(kBlock), 0, stream, a);
  else if (a.H == 5u) hipLaunchKernelGGL(ack_flows_kernel<5>, dim3(1), dim3(kBlock), 0, stream, a);
  else hipLaunchKernelGGL(ack_flows_kernel<0>, dim3(1), dim3(kBlock), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace rudp
