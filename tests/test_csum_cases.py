"""The checksum corpus (tests/csum_cases.py) held to its claims, on the CPU.

Three things: every batch holds every class and twin at every row parity,
alignment and position the GPU tests rely on (so none of them can pass on an
empty class); the oracles (numpy and C) agree with the definition on it; and
three deliberately wrong checksums each fail on it, on exactly their class.
"""
import functools

import numpy as np
import pytest

import csum_cases as cc
from oracle import codec_np

LAYOUTS = (5, 7)
ROTS = len(cc.FIXED_CYCLE)


@functools.lru_cache(maxsize=None)
def _classes(fr, layout):
    return cc.classify(fr.seq, fr.ack, fr.flags, fr.payload, layout)


def _is(fr, name, layout):
    """Whether the frame is of the class (or twin) ``name``, judged by ref_csum, not by its label."""
    if fr.label == "SHORT" or cc.CLASS_OF[name] not in _classes(fr, layout):
        return False
    return fr.twin == name.endswith("_T")


# ------------------------------------------------------------ the reference
def test_reference_known_answers():
    # RFC 1071 section 3: sum 0xddf2, checksum 0x220d
    assert cc.ref_csum(bytes.fromhex("0001f203f4f5f6f7"), 5) == (0x220D, 0x2DDF0)
    assert cc.ref_csum(b"", 5) == (0xFFFF, 0)
    assert cc.ref_csum(b"\x01", 5) == (0xFEFF, 0x0100)
    # layout 7 takes bytes 5-6 as zero
    assert cc.ref_csum(b"\0\0\0\0\0\xab\xcd", 7) == (0xFFFF, 0)
    assert cc.ref_csum(b"\0\0\0\0\0\xab\xcd", 5)[1] == 0x00AB + 0xCD00
    # the top of the accumulator: all ones under a 65535-byte all-0xFF payload
    top = cc.make_frame(0xFFFF, 0xFFFF, 0xFF, b"\xff" * 65535, 7, 0)
    assert cc.ref_csum(top, 7)[1] == 32770 * 0xFFFF == 0x80017FFE
    # the smallest S whose second fold works
    s, a, f = cc.solve_fold2(0, b"", 5, 0)
    assert cc.ref_csum(cc.make_frame(s, a, f, b"", 5), 5)[1] == 0x1FFFF


@pytest.mark.parametrize("layout", LAYOUTS)
def test_solved_classes_have_their_checksums(layout):
    rng = np.random.default_rng(5)
    for L in (0, 1, 2, 3, 15, 16, 17, 31, 64, 1471, 1472, 4096, 65535):
        for kind in ("rand", "ff", "zero"):
            for name, want in (("ZK", {0x0000}), ("NEAR1", {0xFFFE}), ("NEARM", {0x0001})):
                seq, ack, flags, pay = cc.class_fields(name, L, layout, rng, kind)
                c, S = cc.ref_csum(cc.make_frame(seq, ack, flags, pay, layout), layout)
                assert c in want and S > 0, (name, L, kind)
                for field in ("ack", "seq"):
                    v = cc.solve(seq, ack, flags, pay, layout, 0, field)
                    fr = cc.make_frame(*((seq, v) if field == "ack" else (v, ack)), flags, pay, layout)
                    assert cc.ref_csum(fr, layout)[0] == 0 and cc.ref_csum(fr, layout)[1] > 0
            seq, ack, flags, pay = cc.class_fields("FOLD2", L, layout, rng, kind)
            assert "FOLD2" in cc.classify(seq, ack, flags, pay, layout), (L, kind)
        assert cc.ref_csum(cc.make_frame(0, 0, 0, b"\0" * L, layout), layout) == (0xFFFF, 0)


# ------------------------------------------------- the corpus is what it claims
def _fixed_cases():
    for L in cc.FIXED_LENGTHS + cc.MAX_LENGTHS:
        for layout in LAYOUTS:
            yield L, layout


def _fixed_names(L):
    return ("TOP", "ZK", "ZK_T", "FOLD2") if L in cc.MAX_LENGTHS else cc.CLASSES


@pytest.mark.parametrize("L,layout", list(_fixed_cases()))
def test_fixed_batches_hold_every_class_everywhere(L, layout):
    names = _fixed_names(L)
    rots = len(cc.MAX_CYCLE) if L in cc.MAX_LENGTHS else ROTS
    first, last = set(), set()
    for rot in range(rots):
        b = cc.fixed_batch(L, layout, rot)
        assert b.payload.shape == (b.n, L) and b.n <= (16 if L in cc.MAX_LENGTHS else 600)
        rows = {name: [r for r, fr in enumerate(b.frames) if _is(fr, name, layout)] for name in names}
        for name in names:
            assert rows[name], (name, L, layout, rot)
            assert {r % 2 for r in rows[name]} == {0, 1}, f"{name}: a row parity is missing (L={L} rot={rot})"
            if L not in cc.MAX_LENGTHS:
                assert {r % 16 for r in rows[name]} == set(range(16)), \
                    f"{name}: not at every row of the 16-row tile (L={L} rot={rot})"
            if 0 in rows[name]:
                first.add(name)
            if b.n - 1 in rows[name]:
                last.add(name)
        # a twin is the copy of the frame before it wherever there is one
        for r, fr in enumerate(b.frames):
            if fr.twin and r:
                assert fr[1:] == b.frames[r - 1][1:] and not b.frames[r - 1].twin
            # every ZK / Z0 frame has its twin after it
            if fr.label in ("ZK", "Z0") and r + 1 < b.n:
                assert b.frames[r + 1].twin
    assert first >= set(names) and last >= set(names), (L, layout, set(names) - first, set(names) - last)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_packed_batches_hold_every_class_everywhere(layout):
    first, last = set(), set()
    for rot in range(len(cc.CLASSES)):
        # the whole batch, then shorter ones that put the other classes first and last
        cover = cc.PACKED_COVER if rot == 0 else cc.PACKED_ROT_COVER
        b = cc.packed_batch(layout, rot) if rot == 0 else cc.packed_batch(layout, rot, cover=cover)
        _, off, _ = b.wire()
        enc = b.encodable()
        _, eoff, _ = b.encoded()
        lens = np.diff(off)
        if rot == 0:
            assert 1900 <= len(b.frames) <= 2100
            assert sorted(set(lens[lens > 40 + layout] - layout)) == [1472, 2944, 4000, 65535]
            assert (lens == 65535 + layout).sum() == 1
            top = [fr for fr in b.frames if len(fr.payload) == 65535]
            assert "TOP" in _classes(top[0], layout)
        # the covering section has the same offsets in the encode's stream and the decode's
        assert np.array_equal(off[:cover + 1], eoff[:cover + 1])
        assert enc[:cover] == list(range(cover))
        for name in cc.CLASSES:
            at = [i for i in range(cover) if _is(b.frames[i], name, layout)]
            assert {int(off[i]) % 16 for i in at} == set(range(16)), f"{name}: an alignment is missing (rot={rot})"
            near_short = [i for i, fr in enumerate(b.frames) if _is(fr, name, layout)
                          and ((i and b.frames[i - 1].label == "SHORT")
                               or (i + 1 < len(b.frames) and b.frames[i + 1].label == "SHORT"))]
            assert near_short, f"{name}: never next to a short frame"
            if _is(b.frames[0], name, layout):
                first.add(name)
            if _is(b.frames[-1], name, layout):
                last.add(name)
        shorts = sorted({len(fr.raw) for fr in b.frames if fr.label == "SHORT"})
        assert shorts == list(range(layout))
    assert first >= set(cc.CLASSES) and last >= set(cc.CLASSES)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_small_frame_batch_holds_every_class(layout):
    b = cc.small_batch(layout)
    frames, off, _ = b.wire()
    assert max(len(fr.payload) for fr in b.frames) <= 8 and len(frames) // len(b.frames) < 16
    for name in cc.CLASSES:
        at = [i for i, fr in enumerate(b.frames) if _is(fr, name, layout)]
        assert {int(off[i]) % 16 for i in at} == set(range(16)), name
    assert any(fr.label == "SHORT" for fr in b.frames)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_twins_are_bad_checksums_with_the_true_value_out(layout):
    for b in (cc.fixed_batch(17, layout), cc.fixed_batch(65535, layout), cc.packed_batch(layout)):
        seq, ack, flags, ok, cs = b.expected()
        n_twin = 0
        for i, fr in enumerate(b.frames):
            if fr.label == "SHORT":
                assert ok[i] == cc.OK_SHORT and cs[i] == 0
                continue
            true = cc.ref_csum(cc.wire_bytes(fr, layout, False), layout)[0]
            assert cs[i] == true
            if fr.twin:
                n_twin += 1
                assert true in (0, 0xFFFF) and cc.carried_csum(fr, layout) == true ^ 0xFFFF
                assert ok[i] == cc.OK_BAD_CSUM
            else:
                assert ok[i] == cc.OK_GOOD
        assert n_twin
        if layout == 5:
            assert (b.expected(sideband=False)[3][[f.label != "SHORT" for f in b.frames]] == cc.OK_UNVERIFIED).all()


# --------------------------------- the oracles agree with the definition here
def _eq(got, want, what, b, where):
    got, want = np.asarray(got), np.asarray(want)
    if not np.array_equal(got, want):
        i = int(np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))[0])
        frames = getattr(b, "frames", b)
        raise AssertionError(f"{what} differs: {where}, frame {i} ({frames[i].label}): "
                             f"got {got[i]!r}, want {want[i]!r}")


@pytest.mark.parametrize("L,layout", list(_fixed_cases()))
def test_oracles_match_the_definition_fixed(L, layout):
    from oracle import codec_c
    b = cc.fixed_batch(L, layout, 3)
    where = f"L={L} layout={layout}"
    for name, codec in (("codec_np", codec_np), ("codec_c", codec_c)):
        fr, cs = codec.encode(b.seq, b.ack, b.flags, b.payload, layout)
        _eq(fr, b.wire(twins=False), f"{name}.encode frames", b, where)
        _eq(cs, b.true_csum(), f"{name}.encode csum", b, where)
        for side in ((True, False) if layout == 5 else (True,)):
            got = codec.decode(b.wire(), layout, b.carried() if (side and layout == 5) else None)
            for g, w, what in zip(got, b.expected(side), ("seq", "ack", "flags", "ok", "csum")):
                _eq(g, w, f"{name}.decode {what} (sideband={side})", b, where)
    for i in range(0, b.n, 7):
        raw = cc.wire_bytes(b.frames[i], layout, False)
        raw = raw[:5] + raw[7:] if layout == 7 else raw
        for name, fn in (("codec_np", codec_np.inet_checksum), ("codec_c", codec_c.inet_checksum)):
            assert fn(raw) == b.true_csum()[i], (name, where, i, b.frames[i].label)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_oracles_match_the_definition_packed(layout):
    b = cc.packed_batch(layout, 1)
    seq, ack, flags, pay, lens = b.tables()
    off = np.concatenate([[0], np.cumsum(lens)])
    pays = [pay[off[i]:off[i + 1]].tobytes() for i in range(len(lens))]
    fr, foff, cs = codec_np.encode_varlen(seq, ack, flags, pays, layout)
    wf, woff, wcs = b.encoded()
    assert np.array_equal(foff, woff) and np.array_equal(fr, wf)
    _eq(cs, wcs, "codec_np.encode_varlen csum", [b.frames[i] for i in b.encodable()], f"layout={layout}")
    frames, off, side = b.wire()
    for s in ((True, False) if layout == 5 else (True,)):
        got = codec_np.decode_varlen(frames, off, layout, side if (s and layout == 5) else None)
        for g, w, what in zip(got, b.expected(s), ("seq", "ack", "flags", "ok", "csum")):
            _eq(g, w, f"codec_np.decode_varlen {what} (sideband={s})", b, f"layout={layout}")


# ------------------------------------------------------ the corpus discriminates
def _fold(s):
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def _wrong_mod(S, carried):
    """1: reduces mod 0xFFFF, so the non-zero multiples look like zero."""
    c = ~(S % 0xFFFF) & 0xFFFF
    return c, int(c == carried)


def _wrong_single_fold(S, carried):
    """2: folds once and truncates."""
    c = ~((S & 0xFFFF) + (S >> 16)) & 0xFFFF
    return c, int(c == carried)


def _wrong_sum_and_verify(S, carried):
    """3: the right value, but verified by summing the carried field in and expecting all ones."""
    return ~_fold(S) & 0xFFFF, int(_fold(S + carried) == 0xFFFF)


def _all_batches():
    for L, layout in _fixed_cases():
        yield f"fixed L={L} layout={layout}", cc.fixed_batch(L, layout)
    for layout in LAYOUTS:
        yield f"packed layout={layout}", cc.packed_batch(layout)


@pytest.mark.parametrize("wrong,cls,twins", [(_wrong_mod, "ZK", None), (_wrong_single_fold, "FOLD2", None),
                                              (_wrong_sum_and_verify, "ZK", True)])
def test_wrong_checksums_fail_on_their_class_only(wrong, cls, twins):
    for where, b in _all_batches():
        layout = b.layout
        hit = 0
        for i, fr in enumerate(b.frames):
            if fr.label == "SHORT":
                continue
            wire = cc.wire_bytes(fr, layout)
            carried = cc.carried_csum(fr, layout)
            _, _, _, ok, cs = cc.ref_decode(wire, layout, carried)
            got = wrong(cc.ref_csum(wire, layout)[1], carried)
            inside = cls in _classes(fr, layout) and (twins is None or fr.twin)
            if got != (cs, ok):
                assert inside, f"{wrong.__name__} differs outside its class: {where}, frame {i} ({fr.label})"
                hit += 1
            else:
                assert not inside, f"{wrong.__name__} agrees inside its class: {where}, frame {i} ({fr.label})"
        assert hit, f"{wrong.__name__} passes {where}"
