"""Datagram streams around the constructed hash collisions of
tests/golden/dedup_collisions.json, for the tests of dedup's byte confirm
(test_dedup_collisions.py on the CPU, test_gpu_dedup_collisions.py on the GPU).

X and Y are a colliding pair: unequal frames with equal hash under the 32-bit
small_hash (``small`` pairs, for the one-launch form) or under the 64-bit
position-sum hash (``wide`` pairs, for the two-pass table and scan forms).
Fillers are distinct random frames of the pairs' length class.

Every scenario is built by ``_finish``, which takes the expected flags from
the list scan of dedup_ref (never from a kernel) and asserts, from the
reference side alone, that the scenario holds what its name says: at every
``probe`` index a frame of equal hash and unequal bytes lies inside the
frame's window, and the flags the scenario is about are what its name states.
A scenario whose fixture stopped colliding fails there, on the CPU.
"""
from __future__ import annotations

import functools
import json
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

import dedup_ref as ref

FIXTURE = Path(__file__).resolve().parent / "golden" / "dedup_collisions.json"
HASH = {"small": ref.small_hash, "wide": ref.wide_hash}
ORDERS = {"xy": [0, 0], "xyx": [0, 0, 1], "yxxy": [0, 0, 1, 1], "xyyx": [0, 0, 1, 1]}
SMALL_WIN, SMALL_LEN, WIDE_WIN = 1024, 16, 4096  # kDedupSmallWin, kDedupSmallLen, kMaxWindow


@functools.lru_cache(maxsize=None)
def fixture():
    doc = json.loads(FIXTURE.read_text())
    un = bytes.fromhex
    small = {k: [(un(p["x"]), un(p["y"])) for p in v] for k, v in doc["small"].items()}
    wide = {k: [dict(p, x=un(p["x"]), y=un(p["y"])) for p in v] for k, v in doc["wide"].items()}
    return {"small": small, "wide": wide}


def all_pairs():
    """(kind, x, y) of every committed pair."""
    fx = fixture()
    out = [("small", x, y) for v in fx["small"].values() for x, y in v]
    out += [("wide", p["x"], p["y"]) for v in fx["wide"].values() for p in v]
    return out


@functools.lru_cache(maxsize=None)
def groups():
    """name -> (kind, pairs, filler lengths): pairs of one length class, so a
    stream of them has one mean length (one hash-pass lane count)."""
    s, w = fixture()["small"], fixture()["wide"]

    def wide(L):
        return [(p["x"], p["y"]) for p in w["equal_length"] + w["mixed_length"] if p["L"] == L]
    return {
        "s9": ("small", s["equal_length"] + s["prefix"] + s["mixed_length"], (6, 7, 8, 9)),
        "s16": ("small", s["extended16"] + s["mixed_length16"], (16,)),
        "w16": ("wide", wide(16), (16,)),      # one lane per frame
        "w17": ("wide", wide(17), (17,)),      # two
        "w40": ("wide", wide(40), (40,)),      # two; the block at 0, across two 16-byte steps, in the tail
        "w200": ("wide", wide(200), (200,)),   # four
        "w1472": ("wide", wide(1472), (1472,)),  # eight
    }


class _Fill:
    """Distinct random frames, none equal to a fixture frame."""

    def __init__(self, seed, lengths):
        self.rng = np.random.default_rng(seed)
        self.lengths = lengths
        self.seen = {f for _, x, y in all_pairs() for f in (x, y)}

    def __call__(self, length=None):
        while True:
            L = length if length is not None else int(self.rng.choice(self.lengths))
            f = self.rng.integers(0, 256, L, dtype=np.uint8).tobytes()
            if f not in self.seen:
                self.seen.add(f)
                return f


@dataclass
class Scenario:
    name: str
    kind: str            # the hash its pairs collide under: "small" or "wide"
    window: int
    flat: np.ndarray     # u8: the frames back to back
    off: np.ndarray      # i64 [n + 1]
    want: list           # the list scan's flags (2: a rejected frame)
    check: bool = True   # False: some offsets are bad on purpose
    fixed_len: int = 0   # > 0: every frame has this length (the [N, F] entry applies)
    extra: dict = field(default_factory=dict)

    @property
    def n(self):
        return len(self.off) - 1

    @property
    def mean_len(self):
        return len(self.flat) // self.n

    def small_form(self):
        """The one-launch form takes it (packed, 16-B aligned buffer)."""
        return self.mean_len <= SMALL_LEN and self.window <= SMALL_WIN


def _pack(seq):
    off = np.concatenate([[0], np.cumsum([len(f) for f in seq])]).astype(np.int64)
    flat = np.frombuffer(b"".join(seq), np.uint8) if off[-1] else np.zeros(0, np.uint8)
    return flat, off


def _finish(name, kind, seq, window, probes, expect, *, flat=None, off=None, rejected=(), **extra):
    """Expected flags from the list scan; the presence checks of the scenario."""
    want, _ = ref.proxy_scan(seq, window, rejected=rejected)
    cache = {}

    def h(i):
        f = ref.canonical(seq[i])
        if f not in cache:
            cache[f] = HASH[kind](f)
        return cache[f]
    for i in probes:
        lo = max(0, i - window)
        assert any(j not in rejected and h(j) == h(i) and ref.canonical(seq[j]) != ref.canonical(seq[i])
                   for j in range(lo, i)), (name, "no same-hash unequal frame inside the window of", i)
    for i, v in expect.items():
        assert want[i] == v, (name, i, want[i], v)
    if flat is None:
        flat, off = _pack(seq)
    lens = {len(f) for f in seq}
    fixed = lens.pop() if len(lens) == 1 and not rejected else 0
    return Scenario(name, kind, window, flat, off, want, check=not rejected, fixed_len=fixed, extra=extra)


# ---- the scenarios ---------------------------------------------------------------
def orders(group, window=7):
    """Every pair of the group in the four orders X Y, X Y X, Y X X Y, X Y Y X,
    more than `window` fillers between them."""
    kind, pairs, lens = groups()[group]
    fill = _Fill(1, lens)
    seq, probes, expect = [fill() for _ in range(3)], [], {}
    for x, y in pairs:
        for order, flags in ORDERS.items():
            at = len(seq)
            seq += [x if c == "x" else y for c in order]
            expect.update({at + k: v for k, v in enumerate(flags)})
            probes += [at + 1, at + len(order) - 1]
            seq += [fill() for _ in range(window + 1)]
    return _finish(f"{group}-orders", kind, seq, window, probes, expect)


def tiny(group, order):
    """One pattern alone: a batch of 2 to 4 frames."""
    kind, pairs, _ = groups()[group]
    x, y = pairs[-1]  # (the last pair of a group is its mixed-length one where it has any)
    seq = [x if c == "x" else y for c in order]
    return _finish(f"{group}-tiny-{order}", kind, seq, 500, [len(seq) - 1], dict(enumerate(ORDERS[order])))


def window_edges(group, window):
    """Pair A: X, and X again exactly `window` later with Y in between: 1.  Pair
    B: X, and X again `window + 1` later with Y just before it: 0, though Y is
    inside the window.  (Window 1 has no room between: Y X X and X Y X.)"""
    kind, pairs, lens = groups()[group]
    (ax, ay), (bx, by) = pairs[0], pairs[1]
    fill = _Fill(2 + window, lens)
    n, ia, ib = window + 600, 250, 255
    put = {ia: ax, ia + window: ax, (ia + window - 1 if window > 1 else ia - 1): ay,
           ib: bx, ib + window: by, ib + window + 1: bx}
    assert len(put) == 6
    seq = [put[i] if i in put else fill() for i in range(n)]
    probes = [ib + window + 1, ia + window if window > 1 else ia]
    return _finish(f"{group}-edges-w{window}", kind, seq, window, probes,
                   {ia: 0, ib: 0, ia + window: 1, ib + window + 1: 0, ib + window: 0})


def workgroup_edges(group, window):
    """X Y | Y X across frame indices 256 (a workgroup of the two-pass forms),
    512 and 1024 (the small form's tiles) and 2048: the repeat's chain holds
    the collider of its own tile and the one in the halo."""
    kind, pairs, lens = groups()[group]
    fill = _Fill(3 + window, lens)
    put, probes, expect = {}, [], {}
    for k, b in enumerate((256, 512, 1024, 2048)):
        x, y = pairs[k % len(pairs)]
        put.update({b - 2: x, b - 1: y, b: y, b + 1: x})
        probes += [b, b + 1]
        expect.update({b - 2: 0, b - 1: 0, b: 1, b + 1: 1})
    seq = [put[i] if i in put else fill() for i in range(2304)]
    return _finish(f"{group}-workgroups-w{window}", kind, seq, window, probes, expect)


def zero_header(group):
    """b"" and the 5-byte zero header equal each other and nothing else, with
    a colliding pair in the same window."""
    kind, pairs, lens = groups()[group]
    fill = _Fill(4, lens)
    x, y = pairs[0]
    seq = [fill(), b"", x, bytes(5), y, b"", x, bytes(5), y, fill(), bytes(4), bytes(6)]
    expect = dict(enumerate([0, 0, 0, 1, 0, 1, 1, 1, 1, 0, 0, 0]))
    return _finish(f"{group}-zero-header", kind, seq, 500, [4, 6, 8], expect)


def small_cap(mean, window):
    """dedup_small_cap: the one-launch form's LDS run budget in bytes."""
    return ((4 * 256 + window) * max(mean, 1) * 5 // 4 + 256 + 15) & ~15


def burst_tile():
    """The first 1024 frames are 16 bytes long among 1-byte frames behind
    them: their tile's run is over the budget of 1.25 times the batch mean, so
    that tile works from HBM while the last one is staged in LDS."""
    kind, pairs, _ = groups()["s16"]
    fill = _Fill(5, (16,))
    window, n = 7, 3072
    put, probes, expect = {}, [], {}
    for at, (x, y), order in ((100, pairs[0], "xyyx"), (1022, pairs[1], "xyyx"), (2000, pairs[2], "yxxy"),
                              (509, pairs[3], "yxxy"), (2558, pairs[4], "xyyx")):
        put.update({at + k: (x if c == "x" else y) for k, c in enumerate(order)})
        expect.update({at + k: v for k, v in enumerate(ORDERS[order])})
        probes += [at + 2, at + 3]
    ones = fill.rng.integers(0, 256, n, dtype=np.uint8)  # (1-byte frames repeat: 256 values)
    seq = [put[i] if i in put else fill(16) if i < 1024 else bytes([ones[i]]) for i in range(n)]
    sc = _finish("s16-burst-tile", kind, seq, window, probes, expect)
    cap = small_cap(sc.mean_len, window)
    assert sc.small_form() and cap <= 16 * 11 * 256
    for T in (1024, 512):  # both tile sizes: the first tile bursts, the last is staged
        runs = [((int(sc.off[min(p + T, n)]) + 15) & ~15) - (int(sc.off[max(p - window, 0)]) & ~15)
                for p in range(0, n, T)]
        assert runs[0] > cap and runs[-1] <= cap, (T, runs, cap)
    return sc


def rejected(group, how):
    """A frame whose offsets the library refuses (decreasing, or past the
    buffer) next to the colliders: flag 2, equal to nothing, and the
    colliders' flags as without it."""
    kind, pairs, lens = groups()[group]
    fill = _Fill(6, lens)
    x, y = pairs[0]
    clean = [fill(), fill(), fill(), x, y, x, y, fill(), x, fill()]
    flat, off = _pack(clean)
    off = off.copy()
    if how == "decreasing":  # frame 2; frame 1 now runs through it into one byte of frame 3
        off[2] = off[3] + 1
        bad = 2
    else:                    # the last frame ends past the buffer
        off[-1] = len(flat) + 7
        bad = len(clean) - 1
    seq = [b"" if i == bad else flat[off[i]:off[i + 1]].tobytes() for i in range(len(clean))]
    unchanged = {i: v for i, v in enumerate(ref.proxy_scan(clean, 500)[0]) if 3 <= i <= 8}
    assert [unchanged[i] for i in range(3, 9)] == [0, 0, 1, 1, 0, 1]
    return _finish(f"{group}-rejected-{how}", kind, seq, 500, [4, 5, 6, 8], {**unchanged, bad: 2},
                   flat=flat, off=off, rejected={bad})


SCENARIOS = {}
for _g in ("s9", "s16", "w16", "w17", "w40", "w200", "w1472"):
    SCENARIOS[f"{_g}-orders"] = functools.partial(orders, _g)
    for _o in ORDERS:
        SCENARIOS[f"{_g}-tiny-{_o}"] = functools.partial(tiny, _g, _o)
    _wins = (1, 7, 500, SMALL_WIN) if _g[0] == "s" else (1, 7, 500, WIDE_WIN) if _g in ("w16", "w40") else (7, 500)
    for _w in _wins:
        SCENARIOS[f"{_g}-edges-w{_w}"] = functools.partial(window_edges, _g, _w)
    for _w in (7, 500):
        SCENARIOS[f"{_g}-workgroups-w{_w}"] = functools.partial(workgroup_edges, _g, _w)
    SCENARIOS[f"{_g}-zero-header"] = functools.partial(zero_header, _g)
    for _how in ("decreasing", "past"):
        SCENARIOS[f"{_g}-rejected-{_how}"] = functools.partial(rejected, _g, _how)
SCENARIOS["s16-burst-tile"] = burst_tile


def takes_small_form(name):
    """Scenario.small_form() from the name alone (no scenario is built while
    the tests are collected; test_dedup_collisions.py holds the two equal):
    frames of 16 bytes at the mean, window within 1024."""
    short = name.split("-")[0] in ("s9", "s16", "w16") or name == "w17-zero-header"  # (17 B among 0 and 5)
    return short and not name.endswith(f"-w{WIDE_WIN}")


@functools.lru_cache(maxsize=None)
def scenario(name) -> Scenario:
    sc = SCENARIOS[name]()
    assert sc.name == name
    return sc


# ---- streams of pushes -----------------------------------------------------------
def stream(group, window):
    """(seq, sides, push sizes, flags, counts): X at the end of one push, Y in
    the next, X in a third, so the pair straddles the seam between the kept
    history and the new batch; both sides; then repeats at and past the window."""
    kind, pairs, lens = groups()[group]
    fill = _Fill(7 + window, lens)
    x, y = pairs[0]
    if window == 1:
        seq, pushes, probes = [fill(), x, y, x, x, y, y], [2, 1, 1, 2, 1], [3, 5]
        expect = dict(enumerate([0, 0, 0, 0, 1, 0, 1]))
    else:
        seq = [fill(), fill(), fill(), x, y, fill(), fill(), x, y, fill()]
        pushes, probes = [4, 3, 3], [7, 8]
        expect = {3: 0, 4: 0, 7: 1, 8: 1}
        # X again exactly `window` after index 7 (1), Y `window + 1` after index 8 (0, X inside its window)
        gap = [fill() for _ in range(window - 3)]
        seq += gap + [x, fill(), y]
        pushes += [len(gap) - 200, 200 + 1, 2]
        expect.update({7 + window: 1, 9 + window: 0})
        probes.append(9 + window)
    assert sum(pushes) == len(seq)
    sides = [(i * 7 // 3) % 2 for i in range(len(seq))]
    flags, counts = ref.proxy_scan(seq, window, sides)
    sc = _finish(f"{group}-stream-w{window}", kind, seq, window, probes, expect)
    assert sc.want == flags and counts[0] and counts[1]
    return seq, sides, pushes, flags, counts
