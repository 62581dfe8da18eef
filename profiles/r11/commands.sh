# round 11: rudp_ack_progress / rudp_acknowledge and the windowed sender (one MI355X; each result
# bit-exact against the chain of separate calls and tests/ack_ref.py first)
python tools/ack_probe.py --reps 7 > profiles/r11/ack.json
