"""The closed-loop conversation (tests/conversation.py) on the device: for every
scenario the CPU transcript is computed first, then the library's calls drive
their own conversation through the same channel -- the frames they make judged
by their receivers, the replies those build judged by their senders, the state
kept on the device from round to round -- and every round is compared with the
transcript bit for bit.  The loop runs exactly as many rounds as the
transcript has.  Both forms ("chained": receive_batch, receive_window,
receive_flows, unpack_batch_varlen -> ack_progress; "fused": receive,
receive_windowed, receive_flows_fused, acknowledge; acknowledge_flows in
both), both layouts."""
import pytest

import conversation as cv
from conversation import check_end, check_wire_trace, ref_run

pytestmark = pytest.mark.gpu


def run(cuda, name, form, stream=None):
    sc = cv.SCENARIOS[name]
    want = ref_run(name)
    be = cv.DeviceBackend(form, cuda, stream)
    got = cv.converse(sc, be, rounds=want.rounds)
    cv.compare(want.transcript, got.transcript, need=be.NEED)  # the first differing round, call and array
    assert got.rounds == want.rounds
    calls = sum(1 for rnd in got.transcript.rounds for call, _ in rnd if call.startswith(("receive", "acknowledge")))
    assert be.guarded == calls > 0   # every call's own output allocations lay between sentinels
    check_end(sc, got)
    if sc.kind != "flows":   # the conversation is over where the transcript's was
        assert got.sender.finished == want.sender.finished and not got.sender.outbox and not got.channel.pending()
        assert got.sender.pointers == want.sender.pointers
        assert got.receiver.finished_round == want.receiver.finished_round
    else:
        assert got.sender.done == want.sender.done and got.sender.pointers == want.sender.pointers
        assert got.sender.ended == want.sender.ended
        assert got.receiver.done == want.receiver.done
        assert got.receiver.slot_history == want.receiver.slot_history
        assert got.sender.slot_history == want.sender.slot_history


@pytest.mark.parametrize("form", ["chained", "fused"])
@pytest.mark.parametrize("name", sorted(cv.SCENARIOS))
def test_conversation(cuda, name, form):
    run(cuda, name, form)


@pytest.mark.parametrize("form", ["chained", "fused"])
def test_wire_trace(cuda, form):
    """The device's clean stop-and-wait conversation puts the reference's own
    datagrams on the wire (tests/golden/wire_trace.json), both ways."""
    check_wire_trace(cv.DeviceBackend(form, cuda))


class CumulativeAlways(cv.DeviceBackend):
    """A device sender that judges in cumulative mode whatever it is asked."""

    def tx_ack(self, dgrams, state, *, isn, T, C, mode, sent, H):
        return super().tx_ack(dgrams, state, isn=isn, T=T, C=C, mode=cv.CUMULATIVE, sent=sent, H=H)


@pytest.mark.parametrize("form", ["chained", "fused"])
def test_a_wrong_device_sender_is_caught(cuda, form):
    """The comparison has teeth on the device as well: in the exact-mode
    conversation that stalls behind a lost reply, a sender that takes the later
    acks differs from the transcript in the round they arrive."""
    name = "inorder_exact_W8_reply_lost_rudp5"
    want = ref_run(name)
    be = CumulativeAlways(form, cuda)
    got = cv.converse(cv.SCENARIOS[name], be, rounds=want.rounds)
    with pytest.raises(AssertionError, match=r"round 1, call 1 \(acknowledge\), array valid"):
        cv.compare(want.transcript, got.transcript, need=be.NEED)


@pytest.mark.parametrize("form", ["chained", "fused"])
def test_many_peers_on_a_side_stream(cuda, form):
    """The many-peer conversation with every call of every round on a stream
    of its own (the wrappers' host reads follow on the same stream)."""
    import torch
    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        run(cuda, "flows37_rudp7_cumulative_W8", form, stream=side)
    torch.cuda.current_stream(cuda).wait_stream(side)
