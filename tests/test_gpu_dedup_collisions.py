"""Dedup's byte confirm under true hash collisions (csrc/dedup.hip: "exact,
never a probabilistic answer").

Every other dedup test draws its frames from random byte strings, where an
equal hash means equal bytes, so the rejecting half of each confirm never
runs there.  tests/golden/dedup_collisions.json holds constructed pairs of
unequal frames with equal hash, for the 32-bit hash of the one-launch
small-frame form and for the 64-bit hash of the two-pass table and scan
forms; tests/dedup_scenarios.py puts them where a wrong confirm shows (a
collider in front of, behind and between true repeats, at the window's edge,
across workgroups and tiles, in a tile that works from HBM, next to a
rejected frame, across the pushes of a stream).  The expected flags are the
proxy's list scan (tests/dedup_ref.py), compared bit for bit.

test_device_hashes_are_the_restated_ones comes first: it reads the hashes the
kernels compute (rudpx_dedup_hashes of the diagnostics build) and fails, with
the way to regenerate the fixture, once a hash changes and the pairs stop
colliding on the device.
"""
import contextlib
import ctypes

import numpy as np
import pytest

import dedup_ref as ref
import dedup_scenarios as scn
from rudp import _native, batch

pytestmark = pytest.mark.gpu

REGENERATE = ("a dedup hash changed: restate it in tests/dedup_ref.py and regenerate the collisions with "
              "python tests/golden/make_dedup_collisions.py")

# form -> (diagnostics build?, rudpx_tune knobs): 62 = 0 two passes (table), 32 = 0 window scan,
# 70 the one-launch form's frames per thread (1024- or 512-frame tiles)
FORMS = {"default": (False, {}), "table": (True, {62: 0}), "scan": (True, {32: 0}),
         "small-1024": (True, {70: 4}), "small-512": (True, {70: 2})}


@contextlib.contextmanager
def form(name):
    tools, knobs = FORMS[name]
    if not tools:
        yield _native.lib()
        return
    lib = _native.tools_lib()
    old = {}
    try:
        for key, value in knobs.items():
            old[key] = lib.rudpx_tune(key, value)
        yield lib
    finally:
        for key, value in old.items():
            lib.rudpx_tune(key, value)


def dev(a, cuda):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to(cuda)


def packed(flat, cuda, misalign=0):
    """The frames on the device, `misalign` bytes past a 16-byte boundary."""
    import torch
    raw = torch.zeros(len(flat) + 32, dtype=torch.uint8, device=cuda)
    view = raw[misalign:misalign + len(flat)]
    view.copy_(dev(flat, cuda))
    assert view.data_ptr() % 16 == misalign
    return view


def device_hashes(frames, which, cuda):
    """rudpx_dedup_hashes of a list of frames: which = -1 the 32-bit small_hash,
    0..3 the 64-bit hash with 2^which lanes per frame."""
    import torch
    lib = _native.tools_lib(activate=False)
    flat, off = scn._pack(frames)
    d_flat, d_off = packed(flat, cuda), dev(off, cuda)
    out = torch.zeros(len(frames), dtype=torch.int64, device=cuda)
    _native.check(lib.rudpx_dedup_hashes(d_flat.data_ptr(), len(flat), d_off.data_ptr(), len(frames), which,
                                         out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return out.cpu().numpy().view(np.uint64).tolist()


def test_device_hashes_are_the_restated_ones(cuda):
    rng = np.random.default_rng(20)
    pairs = scn.all_pairs()
    frames = [f for _, x, y in pairs for f in (x, y)]
    frames += [b"", bytes(5), bytes(4), b"\x00"]
    frames += [rng.integers(0, 256, int(L), dtype=np.uint8).tobytes() for L in rng.integers(0, 1501, 2000)]
    small = [ref.small_hash(f) for f in frames]
    wide = [ref.wide_hash(f) for f in frames]
    got = {which: device_hashes(frames, which, cuda) for which in (-1, 0, 1, 2, 3)}
    assert got[-1] == small, REGENERATE
    for glog in (0, 1, 2, 3):
        assert got[glog] == wide, (glog, REGENERATE)
    for k, (kind, x, y) in enumerate(pairs):  # on the device too: equal hash, unequal bytes
        assert x != y
        for which in ((-1,) if kind == "small" else (0, 1, 2, 3)):
            assert got[which][2 * k] == got[which][2 * k + 1], (kind, x.hex(), y.hex(), REGENERATE)


def _cases():
    for name in sorted(scn.SCENARIOS):
        for f in FORMS:
            if scn.takes_small_form(name) or not f.startswith("small"):
                yield name, f


@pytest.mark.parametrize("name,form_name", list(_cases()))
def test_flags_equal_the_list_scan(cuda, name, form_name):
    sc = scn.scenario(name)
    want = np.array(sc.want, np.uint8)
    d_off = dev(sc.off, cuda)
    one_launch = form_name.startswith("small")
    assert sc.small_form() or not one_launch, "the one-launch form would not take this scenario"
    with form(form_name):
        got = batch.detect_retransmissions(packed(sc.flat, cuda), frame_off=d_off, window=sc.window, check=False)
        assert np.array_equal(got.cpu().numpy(), want), ("packed", np.nonzero(got.cpu().numpy() != want)[0][:8])
        if sc.check:  # (the checked call reads the same flags and raises on a 2)
            got = batch.detect_retransmissions(packed(sc.flat, cuda), frame_off=d_off, window=sc.window)
            assert np.array_equal(got.cpu().numpy(), want), "packed, check=True"
        if one_launch:
            return
        # a buffer one byte past a 16-byte boundary: no vector staging, the two-pass forms
        got = batch.detect_retransmissions(packed(sc.flat, cuda, 1), frame_off=d_off, window=sc.window, check=False)
        assert np.array_equal(got.cpu().numpy(), want), ("misaligned", np.nonzero(got.cpu().numpy() != want)[0][:8])
        if sc.fixed_len:  # the fixed-length [N, F] entry
            fr = dev(sc.flat.reshape(sc.n, sc.fixed_len), cuda)
            got = batch.detect_retransmissions(fr, window=sc.window)
            assert np.array_equal(got.cpu().numpy(), want), ("[N, F]", np.nonzero(got.cpu().numpy() != want)[0][:8])


def test_a_rejected_frame_raises_when_checked(cuda):
    sc = scn.scenario("s9-rejected-decreasing")
    with pytest.raises(ValueError, match="non-decreasing"):
        batch.detect_retransmissions(packed(sc.flat, cuda), frame_off=dev(sc.off, cuda), window=sc.window)


STREAMS = [(g, w, f) for g in ("s9", "w40", "w200") for w in (1, 500) for f in FORMS
           if g == "s9" or not f.startswith("small")]


@pytest.mark.parametrize("group,window,form_name", STREAMS)
def test_stream_flags_and_counts_equal_the_list_scan(cuda, group, window, form_name):
    """X in one push, Y in the next, X in a third: the collider sits in the
    kept history when the repeat arrives, on either side of the seam."""
    import torch
    seq, sides, pushes, want_flags, want_counts = scn.stream(group, window)
    s = torch.cuda.Stream(device=cuda)
    with form(form_name) as lib:
        h = ctypes.c_void_p()
        _native.check(lib.rudp_dedup_stream_create(window, 512, max(len(f) for f in seq), 0, s.cuda_stream,
                                                   ctypes.byref(h)))
        try:
            got = torch.empty(len(seq), dtype=torch.uint8, device=cuda)
            pos = 0
            for k in pushes:
                part = seq[pos:pos + k]
                fr = np.frombuffer(b"".join(part) + b"\x00", np.uint8)
                off = np.concatenate([[0], np.cumsum([len(p) for p in part])]).astype(np.uint64)
                side = np.array(sides[pos:pos + k], np.uint8)
                _native.check(lib.rudp_dedup_stream_push(h, fr.ctypes.data, off.ctypes.data, k, side.ctypes.data,
                                                         got.data_ptr() + pos))
                pos += k
            counts = (ctypes.c_uint64 * 2)()
            _native.check(lib.rudp_dedup_stream_counts(h, counts))
            assert got.cpu().numpy().tolist() == want_flags
            assert [int(counts[0]), int(counts[1])] == want_counts
        finally:
            lib.rudp_dedup_stream_destroy(h)
