"""A plain bench.py run on the GPU: the headline alone, and --dump-outputs' files
against the oracle."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import codec_np, synth

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent


def test_plain_run_times_the_headline_only_and_dumps_its_frames(cuda, tmp_path):
    import bench
    n, L, steps, warmup = 4099, 1472, 3, 2
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--packets", str(n), "--payload", str(L), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == warmup and line["full"] is False
    assert line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "GiB/s"
    assert abs(line["value"] - n * L / (line["ms_per_step"] / 1e3) / bench.GIB) <= 1e-6 * line["value"]
    # nothing measured or checked beside the headline
    assert "legs" not in line and line["cpu_baseline"] is None and line["config"]["matches_reference"] is None
    assert list(line["baseline_legs"]) == ["headline_C4_encode_1Mx1472"]

    seq, ack, flags, payload = synth.synth(bench.SEEDS[L], 0, n, L)
    want, _ = codec_np.encode(seq, ack, flags, payload, 7)
    rows = np.load(tmp_path / "frames_rows.npy")
    assert np.array_equal(rows, np.arange(n, dtype=np.float64))  # 4099 x 1479 floats fit the sample
    got = np.load(tmp_path / "frames.npy")
    assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "frame_sums.npy"), want.sum(axis=1, dtype=np.int64).astype(np.float64))
