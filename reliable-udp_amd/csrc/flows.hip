// rudp_accept_flows: one datagram batch judged for many peers.  Every datagram
// carries the slot of its peer's row {expect, isn, live, last_isn + 1} in a
// device table; per slot the rule is rudp_accept_inorder's (accept.hip states
// it), applied to the slot's datagrams in arrival order, the slots
// independently.  A flow's first accepted FIN ends its transfer: the later
// datagrams of that flow are not judged and its row turns over to
// {0, 0, 0, isn + 1}, a closed flow that only a SYN with another ISN opens.
//
// One launch of one workgroup of 256 threads, the whole batch (at most 1024
// datagrams) in LDS, no work proportional to the table:
//   1. the tables and d_flow into LDS; the keys slot << 10 | arrival index, a
//      datagram without a valid slot under RUDP_FLOW_NONE, padded with all-ones
//      to a power of two;
//   2. a bitonic sort of the keys: every flow's datagrams become one run, in
//      arrival order, the runs by ascending slot, the flowless datagrams last;
//   3. run heads (the slot differs from the predecessor's) and a block scan of
//      the head flags: A, d_order, d_order_off, every run's slot; one lane per
//      run loads its row;
//   4. accept.hip's one-scan form, segmented: the join (FlowP) restarts at a
//      run head from that flow's row, so one block scan guesses the state
//      before every datagram of every run; accept, reply and reply_ack under
//      the guess, and per run its first event: an accepted FIN or an anomaly;
//   5. one lane per run takes the run's final state from the scan (no loop);
//      a run whose first event is an anomaly is walked by the rule from there
//      by its lane, such runs concurrently (d_info[5] counts them);
//   6. keep, and an exclusive count of the kept datagrams in sorted order: the
//      ranks of the flow-major message order, K, R, every run's rank base;
//   7. the rows and d_flow_info.
// The device functions are in flows_device.hpp: flows_judge is step 1
// (flows_reset, flows_load) and flows_judge_lds, steps 2 to 7 on the LDS
// tables, which the fused rudp_receive_flows (receive_flows.hip) enters with
// tables it filled itself.
#include "flows_device.hpp"

namespace RUDP_NS {

static_assert(kFlowMax == RUDP_FLOWS_MAX_BATCH, "the kernel holds exactly one batch");
static_assert(sizeof(FlowLds) <= 65536, "static LDS");

__global__ void __launch_bounds__(kBlock) accept_flows_kernel(FlowsArgs a) {
  __shared__ FlowLds L;
  flows_judge(a, L);
}

int launch_accept_flows(const FlowsArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(accept_flows_kernel, dim3(1), dim3(kBlock), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace rudp
