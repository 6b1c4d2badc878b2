"""bench.py --dump-outputs DIR: what the timed path's last step computed, as DIR/<name>.npy (float32), at most 64 MB in all — a fixed, seeded
sample of the rows when the outputs are larger — so that two builds run with the same arguments can be compared output for output."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _outputs(rng, E, N, G, dims):
    return {k: None if d == 0 else rng.random((1, T, d), dtype=np.float32) for k, T, d in zip(("ef", "nf", "gf"), (E, N, G), dims)}


def test_small_outputs_are_written_whole(tmp_path):
    arrays = _outputs(np.random.default_rng(0), 5000, 700, 3, (3, 4, 0))
    written = bench.dump_outputs(str(tmp_path), arrays)
    assert sorted(os.listdir(tmp_path)) == ["ef.npy", "nf.npy"] and set(written) == {"ef", "nf"}  # (a width-0 output is no array)
    for k in ("ef", "nf"):
        got = np.load(tmp_path / f"{k}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, arrays[k])


def test_large_outputs_are_a_seeded_sample_below_the_cap(tmp_path):
    rng = np.random.default_rng(1)
    arrays = _outputs(rng, 40_000, 9_000, 1, (96, 64, 5))
    cap = 4 << 20
    assert sum(a.nbytes for a in arrays.values()) > 3 * cap
    written = bench.dump_outputs(str(tmp_path / "a"), arrays, max_bytes=cap)
    again = bench.dump_outputs(str(tmp_path / "b"), {k: v.copy() for k, v in arrays.items()}, max_bytes=cap)
    assert written == again
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= cap
    assert np.array_equal(np.load(tmp_path / "a" / "gf.npy"), arrays["gf"])  # one row of every output survives
    for k in ("ef", "nf"):
        a, b = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert np.array_equal(a, b) and a.dtype == np.float32
        assert 1 < a.shape[1] < arrays[k].shape[1] and a.shape[::2] == arrays[k].shape[::2] and written[k][1] == arrays[k].shape[1]
        # the rows written are rows of the output, in their original order (sorted indices)
        first = {row.tobytes(): i for i, row in enumerate(arrays[k][0])}
        idx = [first[row.tobytes()] for row in a[0]]
        assert idx == sorted(idx) and len(set(idx)) == len(idx)


@pytest.mark.parametrize("argv", [["--gpus", "2"], ["--force-dist"], ["--dist-backend", "gnx"]])
def test_dump_outputs_is_refused_off_the_single_gpu_paths(argv, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dump-outputs", str(tmp_path / "d")] + argv,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--dump-outputs" in r.stderr and not os.path.exists(tmp_path / "d")


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(tmp_path):
    """The headline workload (C2, README dims) at K = 3 and K = 11: with 8 rotating buffer sets the last timed step of both runs is set 2, so the two
    dumps hold the same numbers; every output whole (14 MB), float32, the plan's [1][T][D] layout."""
    def run(K, d):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", "2", "--no-secondary", "--no-c-abi",
               "--no-cpu-baseline", "--no-live-traffic", "--full-line", "--dump-outputs", str(d)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return {k: np.load(d / f"{k}.npy") for k in ("ef", "nf", "gf")}
    a, b = run(3, tmp_path / "k3"), run(11, tmp_path / "k11")
    assert [a[k].shape for k in ("ef", "nf", "gf")] == [(1, 1_000_000, 3), (1, 100_000, 4), (1, 1, 5)]
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all() and np.abs(a[k]).max() > 0
        np.testing.assert_allclose(a[k], b[k], rtol=1e-6, atol=1e-6)
