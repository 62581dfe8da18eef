# round 10: rudp_receive (one MI355X; each result bit-exact against the chain first)
python tools/receive_probe.py --reps 7 > profiles/r10/receive.json   # receive_run1.json: an earlier run on another box,
#   before the reply builder's own forms were added to the probe
# the one kernel of the parent this round refactored (accept_single_kernel), against a
# git worktree build of the parent commit copied to .ab_prev/
python tools/lib_ab.py --op accept --L 1024,1048576 --reps 9 \
  --libs parent=.ab_prev/librudp_parent.so,this=reliable-udp_amd/rudp/librudp.so > profiles/r10/accept_single_ab_parent.json
# the chained form's launches at 1M one-character frames (synthetic tables: the launches, not a transfer)
rocprofv3 --kernel-trace --stats -f csv -d trace_receive_1M -o run -- python3 tools/run_kernel.py \
  --op receive --L 1 --n 1048576 --layout rudp5 --steps 20   # run_kernel_stats.csv -> receive_1Mx1char_kernel_stats.csv
