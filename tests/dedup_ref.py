"""Plain restatements of what csrc/dedup.hip computes, for the collision tests.

Three things, numpy and Python only:

* ``small_hash``: the 32-bit hash of the one-launch small-frame form
  (dedup_small_kernel / dedup_tile): FNV-1a over the canonical bytes, the
  length folded in, the murmur3 finalizer, 0 mapped to 1.
* ``wide_hash``: the 64-bit hash of the two-pass forms (dedup_hash_kernel): the
  sum mod 2^64 of ``dmix(k << 8 | byte_k)`` over the canonical bytes plus
  ``dmix(0xFFFFFFFF00000000 | clen)``.  A sum, so it does not depend on how
  many lanes split the frame.
* ``proxy_scan``: the proxy's rule itself (proxy.py:90-94 with Packet.__eq__),
  a list scan ``key in hist[-window:]`` with per-side counters.

The canonical bytes of a frame are the frame, or five zero bytes when it is
empty (Packet(b"") is the 40-bit zero header).

The ``*_many`` forms hash an [N, L] array of equal-length frames at once; the
generator tests/golden/make_dedup_collisions.py searches with them.
"""
from __future__ import annotations

import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
FNV_BASIS, FNV_PRIME = 0x811C9DC5, 0x01000193
LEN_MARK = 0xFFFFFFFF00000000


def canonical(frame: bytes) -> bytes:
    return bytes(frame) if len(frame) else bytes(5)


# ---- 32-bit: small_hash -------------------------------------------------------
def fnv_state(data: bytes, h: int = FNV_BASIS) -> int:
    """FNV-1a state after `data`, from state `h`."""
    for b in data:
        h = ((h ^ b) * FNV_PRIME) & M32
    return h


def small_finish(h: int, clen: int) -> int:
    h ^= (clen * 0x9E3779B1) & M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h if h else 1


def small_hash(frame: bytes) -> int:
    c = canonical(frame)
    return small_finish(fnv_state(c), len(c))


def small_hash_many(frames: np.ndarray, state: int = FNV_BASIS, clen: int | None = None) -> np.ndarray:
    """small_hash of every row of u8 [N, L] (L >= 1), the FNV state starting at
    `state` (a common prefix's) and the length taken as `clen` (default L)."""
    frames = np.asarray(frames, np.uint8)
    n, L = frames.shape
    assert L >= 1
    h = np.full(n, state, np.uint64)
    for k in range(L):
        h = ((h ^ frames[:, k]) * np.uint64(FNV_PRIME)) & np.uint64(M32)
    h ^= np.uint64(((L if clen is None else clen) * 0x9E3779B1) & M32)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    h[h == 0] = 1
    return h.astype(np.uint32)


# ---- 64-bit: dedup_hash_kernel --------------------------------------------------
def dmix(z: int) -> int:
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def dmix_many(z: np.ndarray) -> np.ndarray:
    z = np.asarray(z, np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)  # (u64 arrays wrap)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def wide_hash(frame: bytes) -> int:
    c = np.frombuffer(canonical(frame), np.uint8)
    terms = dmix_many((np.arange(len(c), dtype=np.uint64) << np.uint64(8)) | c)
    return (int(terms.sum(dtype=np.uint64)) + dmix(LEN_MARK | len(c))) & M64


def wide_hash_many(frames: np.ndarray) -> np.ndarray:
    frames = np.asarray(frames, np.uint8)
    n, L = frames.shape
    assert L >= 1
    pos = (np.arange(L, dtype=np.uint64) << np.uint64(8))[None, :]
    h = dmix_many(pos | frames).sum(axis=1, dtype=np.uint64)
    return h + np.uint64(dmix(LEN_MARK | L))


# ---- the proxy's rule -----------------------------------------------------------
def proxy_scan(seq, window: int, sides=None, rejected=()):
    """(flags, counts): flags[i] = 1 iff frame i equals one of the `window`
    frames before it; counts[side] = the flagged frames of that side (all side
    0 without `sides`).  A frame in `rejected` (the library refused its
    offsets: RUDP_DUP_BAD_OFFSETS) gets 2 and equals nothing, but keeps its
    place in the history."""
    hist, flags, counts = [], [], [0, 0]
    for i, data in enumerate(seq):
        if i in rejected:
            flags.append(2)
            hist.append(None)
            continue
        key = canonical(data)
        dup = key in hist[-window:] if window else False
        flags.append(int(dup))
        counts[sides[i] if sides is not None else 0] += int(dup)
        hist.append(key)
    return flags, counts
