"""The closed-loop conversation (tests/conversation.py) on the CPU references:
every scenario runs to its stated end inside its round cap, the text that comes
out is the text that went in, the clean stop-and-wait conversation reproduces
the reference's wire trace byte for byte, a flow among many fares as it does
alone, and the per-round comparison catches a backend that is subtly wrong."""
import pytest

import ack_ref
import conversation as cv
import window_ref
from accept_ref import SYN

REF = cv.RefBackend()
ref_run, check_end = cv.ref_run, cv.check_end


@pytest.mark.parametrize("name", sorted(cv.SCENARIOS))
def test_scenario(name):
    sc = cv.SCENARIOS[name]
    res = ref_run(name)
    assert res.rounds < cv.cap(sc), (name, res.rounds)            # it ended; the cap did not cut it off
    check_end(sc, res)
    if sc.p:
        assert sc.outcome == "delivered"
        assert res.channel.faults > 0 or sc.T <= 1   # (a handful of datagrams may meet none)
    elif sc.rules:
        assert res.channel.faults > 0, "the script met no datagram"


def test_stalls_are_the_stated_stalls():
    for layout in (5, 7):
        # beyond the domain: the transfer stops at the line (expect passes 65535 after 5 characters)
        r = ref_run(f"inorder_beyond_domain_rudp{layout}")
        assert r.sender.p == 65535 - 65530 and r.receiver.restarts == 1
        # the late SYN copy: receive_data started over, the sender never hears a matching ack again
        r = ref_run(f"inorder_late_syn_copy_rudp{layout}")
        assert r.receiver.restarts == 2 and 0 < r.sender.p < 12
        r = ref_run(f"inorder_exact_W8_reply_lost_rudp{layout}")
        assert r.sender.p == 1 and r.receiver.restarts == 1
        # the reordering receiver stops at the line too: two frames of 3 characters from 65530 take expect
        # to 65536, which no seq_num equals; the frame behind them (seq 0 on the wire) is never taken
        r = ref_run(f"window_beyond_domain_rudp{layout}")
        calls = [rec for rnd in r.transcript.rounds for call, rec in rnd if call == "receive_window"]
        # (the ack of the second is 65536 mod 2^16 = 0 on the wire, below what the sender expects: it stays at 3)
        assert r.sender.p == 3 and r.receiver.restarts == 1
        assert [int(v) for v in calls[-1]["state"]] == [65536, 65530, 1]
        assert all(int(rec["state"][0]) <= 65536 for rec in calls)
        late = [rec for rec in calls if int(rec["state"][0]) == 65536]
        assert len(late) >= 2 and not any(rec["accept"].any() for rec in late[1:])   # nothing matches any more


def test_window_meets_frames_beyond_the_window():
    met = {}
    for name in sorted(n for n in cv.SCENARIOS if n.startswith("window_beyond_rudp")):
        sc = cv.SCENARIOS[name]
        Wc = sc.window_chars
        count = 0
        for rnd in ref_run(name).transcript.rounds:
            for call, rec in rnd:
                if call != "receive_window":
                    continue
                for i in range(len(rec["seq"])):
                    # (a frame that is not taken leaves expect as it was: its reply's ack is the expect it met)
                    ahead = (int(rec["seq"][i]) - int(rec["reply_ack"][i])) & 0xFFFF
                    if rec["usable"][i] and rec["reply"][i] and not rec["flags"][i] & SYN and Wc <= ahead < 0x8000:
                        assert not rec["accept"][i] and rec["carry_rank"][i] == 0xFFFFFFFF, (name, i)
                        count += 1
        met[name] = count
        assert count >= 1, (name, met)
    assert {cv.SCENARIOS[n].window_chars for n in met} == {1, 8, 64}


def test_scenarios_cover_the_table():
    names = set(cv.SCENARIOS)
    for what in ("clean", "random", "syn_lost", "fin_lost", "replies_lost", "finack_lost", "closing_ack_lost",
                 "stale_reply"):
        for layout in (5, 7):
            for mode in ("exact_W1", "cumulative_W8"):
                assert any(n.startswith(f"inorder_{what}") and f"rudp{layout}_{mode}" in n for n in names), (what, mode)
    for what in ("reversed", "gap", "beyond", "carried_dups", "random"):
        for Wc in (1, 8, 64):
            assert any(n.startswith(f"window_{what}") and f"_Wc{Wc}_" in n for n in names)
    ts = {(s.T, s.C) for s in cv.SCENARIOS.values() if s.kind != "flows"}
    assert {T for T, _ in ts} >= {0, 1, 300} and {C for _, C in ts} == {1, 3, 16}
    assert any(T == C and C > 1 for T, C in ts) and any(T == 2 * C + 1 for T, C in ts)
    assert any(s.isn + s.T == 65535 for s in cv.SCENARIOS.values())
    for ch in cv.ALPHABET:
        assert any(ch in cv.message_of(s) for s in cv.SCENARIOS.values() if s.kind != "flows")
    assert sorted(len(c.encode()) for c in cv.ALPHABET) == [1, 2, 3, 4]


def test_window_gap_is_carried_over_two_calls():
    for name in sorted(cv.SCENARIOS):
        if not name.startswith("window_gap") or "_Wc1_" in name:
            continue
        calls = [rec for rnd in ref_run(name).transcript.rounds for call, rec in rnd if call == "receive_window"]
        pending = [int(rec["info"][4]) for rec in calls]
        assert any(a > 0 and b > 0 for a, b in zip(pending, pending[1:])), (name, pending)


def test_window_meets_copies_of_carried_frames():
    for name in sorted(cv.SCENARIOS):
        if not name.startswith("window_carried_dups") or "_Wc1_" in name:
            continue
        calls = [rec for rnd in ref_run(name).transcript.rounds for call, rec in rnd if call == "receive_window"]
        met = 0
        for before, rec in zip(calls, calls[1:]):
            m = len(before["carry_off"]) - 1            # the frames this call found carried
            held = set(rec["seq"][:m].tolist())
            met += sum(1 for i in range(m, len(rec["seq"])) if int(rec["seq"][i]) in held and not rec["accept"][i]
                       and rec["usable"][i])
        assert met >= 2, (name, met)


def test_flows128_first_batch_is_the_limit():
    for layout in (5, 7):
        tr = ref_run(f"flows128_rudp{layout}").transcript
        first = [rec for call, rec in tr.rounds[1] if call == "receive_flows"]
        assert len(first) == 1 and len(first[0]["seq"]) == cv.MAX_BATCH
        assert max(len(rec["seq"]) for rnd in tr.rounds for call, rec in rnd if "flows" in call) == cv.MAX_BATCH


def test_slot_reuse():
    for layout in (5, 7):
        sc = cv.SCENARIOS[f"flows_slot_reuse_rudp{layout}"]
        res = ref_run(sc.name)
        # peer 7 held the table's last row twice, peer 5 the first all along
        assert res.receiver.slot_history.count((7, sc.n_flows - 1)) == 2 and (5, 0) in res.receiver.slot_history
        assert res.sender.slot_history.count((7, sc.n_flows - 1)) == 2
        # the closed transfer's SYN came again while its row waited for the closing ACK, and was ignored
        late = [rec for rnd in res.transcript.rounds[2:5] for call, rec in rnd if call == "receive_flows"
                for i in range(len(rec["seq"])) if rec["flags"][i] & SYN and rec["seq"][i] == 4999]
        assert late and all(not rec["accept"][i] for rec in late for i in range(len(rec["seq"]))
                            if rec["flags"][i] & SYN and rec["seq"][i] == 4999)
        assert [t for p, t, _ in res.receiver.done if p == 7] == [cv.text_of(f"{sc.name}/7/0", 4),
                                                                  cv.text_of(f"{sc.name}/7/1", 9)]


def test_second_recv_tells_the_repeated_syn_by_last_isn():
    for name in sorted(n for n in cv.SCENARIOS if "_again_" in n):
        res = ref_run(name)
        met = 0
        for rnd in res.transcript.rounds[4:]:          # (the second send() starts in round 2 or 4)
            for call, rec in rnd:
                if call.startswith("receive"):
                    for i in range(len(rec["seq"])):
                        if rec["flags"][i] & SYN and rec["seq"][i] == 4999:
                            assert not rec["accept"][i] and rec["reply"][i], name   # ignored, and answered
                            met += 1
        assert met == 1, (name, met)


def test_flows_end_in_different_rounds():
    res = ref_run("flows37_rudp5_cumulative_W8")
    assert len({rnd for _, rnd in res.sender.done.values()}) >= 4


def test_wire_trace():
    cv.check_wire_trace(REF)


@pytest.mark.parametrize("name", ["flows37_rudp5_exact_W1", "flows37_rudp7_cumulative_W8"])
def test_flow_alone_fares_the_same(name):
    sc = cv.SCENARIOS[name]
    many = ref_run(name)
    texts = {peer: text for peer, text, _ in many.receiver.done}
    for k, (peer, T, _, _, _, _) in enumerate(sc.flows):
        alone = cv.solo(sc, k, REF)
        assert alone.outcome == "delivered", (name, k)
        state, rnd = many.sender.done[peer]
        assert (state, rnd) == ("done", alone.sender.finished_round), (name, k)
        assert texts[peer] == alone.receiver.text == cv.text_of(f"{sc.name}/{peer}/0", T), (name, k)
        assert many.sender.pointers[peer] == alone.sender.pointers[:rnd + 1], (name, k)


@pytest.mark.parametrize("name", ["inorder_random0_rudp7_cumulative_W8_T40_C1", "window_random1_rudp7_Wc8_T300_C16",
                                  "flows37_rudp7_cumulative_W8"])
def test_same_seed_same_transcript(name):
    again = cv.converse(cv.SCENARIOS[name], cv.RefBackend())
    cv.compare(ref_run(name).transcript, again.transcript)
    cv.compare(again.transcript, ref_run(name).transcript)


# ------------------------------------------------------------ wrong backends
def ack_before_drain(seq, flags, chars, usable=None, state=(0, 0, 0), last_isn=None, *, window_chars, n_carried=0):
    """window_ref, but a frame that fills the gap is answered with the expect
    it had before the pending frames behind it were delivered."""
    r = window_ref.window_ref(seq, flags, chars, usable, state, last_isn, window_chars=window_chars,
                              n_carried=n_carried)
    ack = r.reply_ack.copy()
    for i in range(len(seq)):
        # delivered on arrival (a frame delivered from the pending set was answered with an ack below its seq)
        behind = (int(seq[i]) + int(chars[i])) & 0xFFFF
        if r.reply[i] and r.accept[i] == 1 and (int(ack[i]) - behind) & 0xFFFF < 0x8000:
            ack[i] = behind
    return r._replace(reply_ack=ack)


class AckBeforeDrain(cv.RefBackend):
    window_rule = staticmethod(ack_before_drain)


def ack_at_least(*args, **kw):
    """ack_ref, but exact mode takes ack >= expected."""
    real = ack_ref.is_valid

    def loose(ack, usable, isn, T, C, p, L, mode=ack_ref.EXACT, sent=None):
        if mode == ack_ref.EXACT:
            return bool(usable) and ack >= isn + p + L
        return real(ack, usable, isn, T, C, p, L, mode, sent)
    ack_ref.is_valid = loose
    try:
        return ack_ref.ack_ref(*args, **kw)
    finally:
        ack_ref.is_valid = real


class AckAtLeast(cv.RefBackend):
    ack = staticmethod(ack_at_least)


class LeakyFlows(cv.RefBackend):
    """The first active flow's new state also lands in the next slot."""

    def flows(self, frames, off, flow, table, H):
        r = super().flows(frames, off, flow, table, H)
        rows = r.flows.flow_info
        if len(rows) and int(rows[0][0]) + 1 < len(r.flows.states):
            slot = int(rows[0][0])
            r.flows.states[slot + 1] = r.flows.states[slot]
        return r


@pytest.mark.parametrize("wrong, name", [
    (AckBeforeDrain, "window_gap_rudp5_Wc8_"), (AckBeforeDrain, "window_gap_rudp7_Wc64_"),
    (AckBeforeDrain, "window_reversed_rudp5_Wc64_"),
    (AckAtLeast, "inorder_exact_W8_reply_lost_rudp5"),
    (LeakyFlows, "flows37_rudp5_exact_W1"), (LeakyFlows, "flows_slot_reuse_rudp7")])
def test_wrong_backend_is_caught(wrong, name):
    name, = [n for n in cv.SCENARIOS if n.startswith(name)]
    sc = cv.SCENARIOS[name]
    want = ref_run(name)
    got = cv.converse(sc, wrong(), rounds=want.rounds)
    with pytest.raises(AssertionError, match=r"round \d+, call \d+ \(\w+\), array \w+"):
        cv.compare(want.transcript, got.transcript)
    # and the right one passes the same comparison over the same rounds
    cv.compare(want.transcript, cv.converse(sc, cv.RefBackend(), rounds=want.rounds).transcript)


def test_compare_names_the_round_the_call_and_the_array():
    a, b = cv.Transcript(), cv.Transcript()
    for t, v in ((a, 1), (b, 2)):
        t.begin()
        t.add("receive", dict(seq=[7], ack=[0]))
        t.begin()
        t.add("receive", dict(seq=[8], ack=[0]))
        t.add("acknowledge", dict(valid=[1], pointer=[v]))
    with pytest.raises(AssertionError, match=r"round 1, call 1 \(acknowledge\), array pointer"):
        cv.compare(a, b)


def test_channel_is_keyed_by_the_flow():
    """The same flow meets the same fate whatever else the channel carries."""
    d = [ack_ref.header(k, 0, 0, 7, b"x") for k in range(1, 40)]
    alone = cv.Channel("s", 7, p=0.5, budget=10)
    among = cv.Channel("s", 7, p=0.5, budget=10)
    got_a, got_b = [], []
    for rnd in range(4):
        got_a.append(alone.carry(3, cv.C2S, rnd, d[10 * rnd:10 * rnd + 10]))
        among.carry(2, cv.C2S, rnd, d[:5])
        got_b.append(among.carry(3, cv.C2S, rnd, d[10 * rnd:10 * rnd + 10]))
        among.carry(4, cv.S2C, rnd, d[5:9])
    assert got_a == got_b and alone.faults == 10
    # the budget spent, the channel is perfect
    assert alone.carry(3, cv.C2S, 9, d) == d
    # rudp5 conversations meet no damage
    five = cv.Channel("s", 5, p=1.0, budget=200)
    out = [x for rnd in range(5) for x in five.carry(0, cv.C2S, rnd, d)] + five.carry(0, cv.C2S, 5, []) \
        + five.carry(0, cv.C2S, 6, [])
    assert set(out) <= set(d)
    # a SYN is never duplicated or delayed at random
    syn = ack_ref.header(1, 0, SYN, 5, b"x")
    for seed in range(50):
        ch = cv.Channel(seed, 5, p=1.0, budget=5)
        got = ch.carry(0, cv.C2S, 0, [syn])
        assert got in ([], [syn]) and not ch.pending()


def test_no_module_level_torch():
    import subprocess
    import sys
    code = "import sys; sys.path[:0] = %r; import conversation; assert 'torch' not in sys.modules" % sys.path
    assert subprocess.run([sys.executable, "-c", code]).returncode == 0
