# round 14: the receivers' shared device code moved into headers (no kernel changes intended).
# Parent build (a build of the parent commit copied to .ab_prev/) against this build on one
# MI355X, six rounds, alternating parent / this, one process per probe:
#   RUDP_LIB=.ab_prev/librudp.so RUDP_TOOLS_LIB=.ab_prev/librudp_tools.so \
#   python tools/receive_probe.py --shapes batch1024,sweep
#   python tools/ack_probe.py --shapes batch1024,sweep
#   python tools/window_probe.py --windowed-only --windowed-out <file>
# and the same without the two variables for this build.
# ab_summary.json: a line per shape and form with every process's us_per_call median
# (parent_us, new_us: the probes' raw figures; the rest of their output is not kept), the
# parent's median, the parent-vs-parent spread (max - min over its processes) and this
# build's median.
# kernel_resources.md: hipcc -Rpass-analysis=kernel-resource-usage, same flags, parent -> this.
# bench.json: python bench.py --gpus 1 --steps 20 --warmup 5, the headline leg of both builds.
#
# rudp_accept_flows (many peers in one batch), one MI355X, the product library with a build
# of the parent commit (git worktree, python reliable-udp_amd/rudp/_build.py) beside it:
#   python tools/flows_probe.py --parent <parent build>/librudp.so --out profiles/r14/flows_probe.json
# flows_probe.json: medians over 11 rounds of 200 back-to-back calls, the forms in rotation.
