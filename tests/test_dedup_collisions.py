"""The constructed hash collisions of tests/golden/dedup_collisions.json and
the scenarios built around them (tests/dedup_scenarios.py), checked on the
CPU: every committed pair is unequal and collides under the restated hashes
(tests/dedup_ref.py), every scenario holds the situation it names, and the
list scan the GPU tests expect is the oracle's proxy rule."""
import numpy as np
import pytest

import dedup_ref as ref
import dedup_scenarios as scn
from rudp import _native


def test_fixture_holds_what_the_tests_need():
    fx = scn.fixture()
    s, w = fx["small"], fx["wide"]
    assert len(s["equal_length"]) + len(s["prefix"]) >= 8
    assert {len(x) for x, _ in s["equal_length"] + s["prefix"]} == {6, 7, 8, 9}
    assert len(s["prefix"]) >= 2 and all(x[:-6] == y[:-6] and len(x) == len(y) > 6 for x, y in s["prefix"])
    assert len(s["mixed_length"]) >= 2 and all(len(x) != len(y) for x, y in s["mixed_length"])
    assert len(s["extended16"]) == len(s["equal_length"]) + len(s["prefix"])
    assert all(len(x) == 16 == len(y) for x, y in s["extended16"])
    have = {}
    for p in w["equal_length"]:
        assert len(p["x"]) == len(p["y"]) == p["L"]
        b = p["base"]  # the frames differ inside the 16-position block only
        assert p["x"][:b] == p["y"][:b] and p["x"][b + 16:] == p["y"][b + 16:]
        have[p["L"], b] = have.get((p["L"], b), 0) + 1
    assert set(have) == {(16, 0), (17, 1), (40, 0), (40, 8), (40, 24), (200, 184), (1472, 0), (1472, 1456)}
    assert min(have.values()) >= 2
    mixed = sorted({(len(p["x"]), len(p["y"])) for p in w["mixed_length"]})
    assert mixed == [(40, 41), (200, 216)] and len(w["mixed_length"]) >= 4


def test_every_pair_is_unequal_and_collides():
    pairs = scn.all_pairs()
    assert len(pairs) >= 40
    for kind, x, y in pairs:
        assert x != y
        assert scn.HASH[kind](x) == scn.HASH[kind](y), (kind, x.hex(), y.hex())


def test_hash_restatements_agree_with_their_vector_forms():
    """The generator searches with the *_many forms; the tests check with the
    scalar ones."""
    rng = np.random.default_rng(5)
    for L in (1, 5, 6, 16, 17, 200):
        fr = rng.integers(0, 256, (50, L), dtype=np.uint8)
        assert ref.small_hash_many(fr).tolist() == [ref.small_hash(r.tobytes()) for r in fr]
        assert ref.wide_hash_many(fr).tolist() == [ref.wide_hash(r.tobytes()) for r in fr]
    assert ref.small_hash(b"") == ref.small_hash(bytes(5)) != ref.small_hash(bytes(4))
    assert ref.wide_hash(b"") == ref.wide_hash(bytes(5)) != ref.wide_hash(bytes(6))
    # FNV-1a's published vectors: the state after "a" and after "foobar"
    assert ref.fnv_state(b"a") == 0xE40C292C and ref.fnv_state(b"foobar") == 0xBF9CF968


@pytest.mark.parametrize("name", sorted(scn.SCENARIOS))
def test_scenario_holds_the_situation_it_names(name):
    sc = scn.scenario(name)  # (its presence checks are asserted while it is built)
    assert len(sc.want) == sc.n and set(sc.want) <= {0, 1, 2}
    assert (2 in sc.want) == (not sc.check)
    assert sc.small_form() == scn.takes_small_form(name)
    if sc.kind == "small":
        assert sc.small_form(), "a small-hash scenario the one-launch form would not take"


@pytest.mark.parametrize("group,window", [("s9", 1), ("s9", 500), ("w40", 1), ("w40", 500), ("w200", 500)])
def test_stream_scenario_holds_the_situation_it_names(group, window):
    seq, sides, pushes, flags, counts = scn.stream(group, window)
    assert sum(pushes) == len(seq) == len(flags) and sum(flags) == sum(counts)


def test_list_scan_is_the_oracles_proxy_rule(golden_dedup):
    from oracle.bitstring_packet import proxy_retransmitted
    g = golden_dedup
    off = np.concatenate([[0], np.cumsum(g["lengths"])]).astype(np.int64)
    seq = [g["frames"][off[i]:off[i + 1]].tobytes() for i in range(len(g["lengths"]))]
    assert ref.proxy_scan(seq, 500)[0] == g["dup"].tolist() == proxy_retransmitted(seq, 500)
    for name in ("s9-orders", "w40-orders", "s9-zero-header"):
        sc = scn.scenario(name)
        seq = [sc.flat[sc.off[i]:sc.off[i + 1]].tobytes() for i in range(sc.n)]
        assert sc.want == proxy_retransmitted(seq, sc.window), name


def test_hash_hook_is_in_the_diagnostics_build_only():
    """rudpx_dedup_hashes, which keeps the GPU tests from going vacuous after a
    hash change, is bound in librudp_tools.so; librudp.so does not have it."""
    assert _native.tools_lib(activate=False).rudpx_dedup_hashes.argtypes is not None
    assert not hasattr(_native.lib(), "rudpx_dedup_hashes")
