"""Generate tests/golden/dedup_collisions.json: unequal frames with equal hash.

Both hashes of csrc/dedup.hip only pick candidates; a byte compare confirms
each hit.  Random test data never makes two unequal frames hash equal, so the
rejecting half of the confirm needs constructed collisions.  This script
builds them on the CPU with numpy, from a fixed seed, and checks every pair
with tests/dedup_ref.py (frames unequal, hashes equal) before it writes.  The
suite reads the JSON and never runs this.

32-bit hash (small_hash: FNV-1a, length, murmur finalizer): a birthday search.
2^20 random frames give about 2^40 / 2 / 2^32 = 128 unequal pairs of equal
hash.  A search over frames that share a prefix puts the difference in the
last 6 bytes; a search over mixed lengths yields pairs of different lengths.
Equal-length pairs end in equal FNV states, so any common suffix keeps the
collision: ``extended16`` appends one up to 16 bytes.  (A pair of different
lengths ends in different states and cannot be extended; ``mixed_length16``
is a fresh search over lengths 15..17 behind a common prefix.)

64-bit hash (sum over positions of dmix(k << 8 | byte) plus a length term): a
generalized-birthday search (Wagner's k-tree).  The frames X and Y differ in a
block of 16 positions from `base`; list i of 8 holds 2^18 values
    dmix(p << 8 | x_p) - dmix(p << 8 | y_p) + dmix(q << 8 | x_q) - dmix(q << 8 | y_q)
for its two positions p, q (x_p != y_p, so X != Y).  One value from each list
summing to 0 mod 2^64 is a collision: merge the lists in pairs on the low 18
bits, then on the next 18, then on all 64.  The hash is additive by position,
so the block collides inside any common bytes, at any frame length.  For a
pair of different lengths the length terms' difference and the longer
frame's extra bytes are a constant, added to one list.

The JSON: ``small`` and ``wide`` sections, each a dict of lists of pairs
``{"x": hex, "y": hex}`` (wide pairs also carry ``L``, ``base``).

usage: python tests/golden/make_dedup_collisions.py [--check]
  --check: regenerate in memory and compare with the committed file
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import dedup_ref as ref  # noqa: E402

SEED = 0xDED0C011
OUT = HERE / "dedup_collisions.json"
KEEP = 2  # pairs kept per entry


# ---- 32-bit ---------------------------------------------------------------------
def _equal_hash_pairs(hashes: np.ndarray):
    """Index pairs (i, j), i < j, of equal entries (adjacent in sorted order)."""
    order = np.argsort(hashes, kind="stable")
    s = hashes[order]
    at = np.nonzero(s[1:] == s[:-1])[0]
    return [(int(order[a]), int(order[a + 1])) for a in at]


def small_search(rng, prefix: bytes, tails, count: int):
    """Pairs of frames prefix + random tail (tail lengths from `tails`, 2^20
    frames in all) with equal small_hash, unequal bytes: the first `count`, or
    all of them for count = 0."""
    state = ref.fnv_state(prefix)
    per = (1 << 20) // len(tails)
    frames, hashes = [], []
    for t in tails:
        body = rng.integers(0, 256, (per, t), dtype=np.uint8)
        hashes.append(ref.small_hash_many(body, state, len(prefix) + t))
        frames += [(t, body)]
    hashes = np.concatenate(hashes)

    def frame(i):
        t, body = frames[i // per]
        return prefix + body[i % per].tobytes()
    pairs = [(frame(i), frame(j)) for i, j in _equal_hash_pairs(hashes)]
    pairs = [(x, y) for x, y in pairs if x != y]
    return pairs[:count] if count else pairs


def build_small(rng):
    out = {"equal_length": [], "prefix": [], "mixed_length": [], "extended16": [], "mixed_length16": []}
    for L in (6, 7, 8, 9):
        out["equal_length"] += small_search(rng, b"", (L,), KEEP)
    for plen in (1, 3):  # lengths 7 and 9, the difference in the last 6 bytes
        prefix = rng.integers(0, 256, plen, dtype=np.uint8).tobytes()
        out["prefix"] += small_search(rng, prefix, (6,), KEEP)
    mixed = [p for p in small_search(rng, b"", (6, 7, 8, 9), 0) if len(p[0]) != len(p[1])]
    out["mixed_length"] = mixed[:2 * KEEP]
    for x, y in out["equal_length"] + out["prefix"]:
        tail = rng.integers(0, 256, 16 - len(x), dtype=np.uint8).tobytes()
        out["extended16"].append((x + tail, y + tail))
    prefix = rng.integers(0, 256, 10, dtype=np.uint8).tobytes()
    mixed16 = [p for p in small_search(rng, prefix, (5, 6, 7), 0) if len(p[0]) != len(p[1])]
    out["mixed_length16"] = mixed16[:KEEP]
    for name, pairs in out.items():
        assert len(pairs) >= 2, name
        for x, y in pairs:
            assert x != y and ref.small_hash(x) == ref.small_hash(y), name
            same = len(x) == len(y)
            assert same == (name not in ("mixed_length", "mixed_length16")), name
    assert len(out["equal_length"]) + len(out["prefix"]) >= 8
    for x, y in out["prefix"]:
        assert x[:-6] == y[:-6] and len(x) in (7, 9)
    assert all(len(x) == 16 == len(y) for x, y in out["extended16"])
    return {k: [{"x": x.hex(), "y": y.hex()} for x, y in v] for k, v in out.items()}


# ---- 64-bit ---------------------------------------------------------------------
NLIST, PER_LIST, BITS = 8, 1 << 18, 18


def _merge(va, ia, vb, ib, shift, width):
    """All (a, b) with bits [shift, shift + width) of va[a] + vb[b] zero (the
    bits below are zero in both already): values and index rows of the sums."""
    mask = np.uint64((1 << width) - 1) if width < 64 else np.uint64(ref.M64)
    ka = (va >> np.uint64(shift)) & mask
    kb = ((np.uint64(0) - vb) >> np.uint64(shift)) & mask  # key of the value that cancels b
    order = np.argsort(kb, kind="stable")
    kb_s = kb[order]
    lo = np.searchsorted(kb_s, ka, "left")
    hi = np.searchsorted(kb_s, ka, "right")
    cnt = hi - lo
    a_idx = np.repeat(np.arange(len(va)), cnt)
    first = np.cumsum(cnt) - cnt  # where each a's matches start in the output
    b_idx = order[np.repeat(lo, cnt) + (np.arange(int(cnt.sum())) - np.repeat(first, cnt))]
    return va[a_idx] + vb[b_idx], np.concatenate([ia[a_idx], ib[b_idx]], axis=1)


def wide_search(rng, base: int, target: int = 0):
    """Blocks (x, y) of 16 bytes at positions base .. base + 15 with
    sum dmix(p << 8 | x_p) - sum dmix(p << 8 | y_p) == target mod 2^64."""
    vals, idx, choice = [], [], []
    for li in range(NLIST):
        p, q = base + 2 * li, base + 2 * li + 1
        c = rng.integers(0, 256, (PER_LIST, 4), dtype=np.uint8).astype(np.uint64)  # x_p, y_p, x_q, y_q
        c[:, 1] = np.where(c[:, 1] == c[:, 0], c[:, 0] ^ np.uint64(1), c[:, 1])  # x_p != y_p
        v = (ref.dmix_many(np.uint64(p << 8) | c[:, 0]) - ref.dmix_many(np.uint64(p << 8) | c[:, 1])
             + ref.dmix_many(np.uint64(q << 8) | c[:, 2]) - ref.dmix_many(np.uint64(q << 8) | c[:, 3]))
        if li == 0:
            v = v - np.uint64(target & ref.M64)
        vals.append(v)
        idx.append(np.arange(PER_LIST, dtype=np.int64)[:, None])
        choice.append(c)
    for shift, width in ((0, BITS), (BITS, BITS), (0, 64)):  # 8 lists -> 4 -> 2 -> 1
        merged = [_merge(vals[k], idx[k], vals[k + 1], idx[k + 1], shift, width) for k in range(0, len(vals), 2)]
        vals, idx = [m[0] for m in merged], [m[1] for m in merged]
    assert len(vals) == 1 and not vals[0].any()
    blocks = []
    for row in idx[0]:
        x = bytes(int(b) for li in range(NLIST) for b in (choice[li][row[li], 0], choice[li][row[li], 2]))
        y = bytes(int(b) for li in range(NLIST) for b in (choice[li][row[li], 1], choice[li][row[li], 3]))
        blocks.append((x, y))
    return blocks


EQUAL = ((16, 0), (17, 1), (40, 0), (40, 8), (40, 24), (200, 184), (1472, 0), (1472, 1456))
MIXED = ((40, 41, 24), (200, 216, 184))  # (shorter, longer, block base)


def build_wide(rng):
    found = {}  # base -> unused blocks: a block collides at its positions whatever the frame length

    def blocks(base, k):
        if base not in found:
            found[base] = wide_search(rng, base)
        assert len(found[base]) >= k, (base, len(found[base]))
        take, found[base] = found[base][:k], found[base][k:]
        return take
    equal, mixed = [], []
    for L, base in EQUAL:
        for bx, by in blocks(base, KEEP):
            common = rng.integers(0, 256, L, dtype=np.uint8).tobytes()
            x = common[:base] + bx + common[base + 16:]
            y = common[:base] + by + common[base + 16:]
            assert len(x) == L == len(y)
            equal.append({"L": L, "base": base, "x": x, "y": y})
    for L1, L2, base in MIXED:
        common = rng.integers(0, 256, L2, dtype=np.uint8).tobytes()
        extra = sum(ref.dmix(k << 8 | common[k]) for k in range(L1, L2))
        # hash(X) = S + bx + len(L1), hash(Y) = S + by + extra + len(L2):  bx - by = target
        target = (extra + ref.dmix(ref.LEN_MARK | L2) - ref.dmix(ref.LEN_MARK | L1)) & ref.M64
        got = wide_search(rng, base, target)
        assert len(got) >= KEEP, (L1, L2, len(got))
        for bx, by in got[:KEEP]:
            x = common[:base] + bx + common[base + 16:L1]
            y = common[:base] + by + common[base + 16:]
            assert len(x) == L1 and len(y) == L2
            mixed.append({"L": L1, "L2": L2, "base": base, "x": x, "y": y})
    for p in equal + mixed:
        assert p["x"] != p["y"] and ref.wide_hash(p["x"]) == ref.wide_hash(p["y"]), (p["L"], p["base"])
        p["x"], p["y"] = p["x"].hex(), p["y"].hex()
    return {"equal_length": equal, "mixed_length": mixed}


def build():
    rng = np.random.default_rng(SEED)
    doc = {"seed": SEED, "small": build_small(rng), "wide": build_wide(rng)}
    return json.dumps(doc, indent=1) + "\n"


if __name__ == "__main__":
    text = build()
    if "--check" in sys.argv:
        assert OUT.read_text() == text, "dedup_collisions.json differs from what the seed gives"
        print("dedup_collisions.json reproduces from its seed")
    else:
        OUT.write_text(text)
        print(f"wrote {OUT} ({len(text)} bytes)")
