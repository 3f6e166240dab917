"""bench.py's host logic without a GPU: the PMC record is used only for the library it profiled
(its source-hash stamp), and a multi-rank RCCL run with fewer GPUs than ranks fails loudly."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

import bench

ROOT = Path(__file__).resolve().parents[1]


def _record(tmp_path, monkeypatch, **fields):
    prof = tmp_path / "profiles"
    prof.mkdir(exist_ok=True)
    rec = {"kernel": "void mh::mh_kernel<64, 1, 1>(mh::LaunchArgs)", "chains_per_launch": 65536,
           "hbm_bytes_per_launch": 1.0, "srchash": "abc123"}
    rec.update(fields)
    (prof / "pmc_step_kernel_n64.json").write_text(json.dumps(rec))
    monkeypatch.setattr(bench, "ROOT", tmp_path)


def test_pmc_record_current_only_for_its_library(tmp_path, monkeypatch):
    _record(tmp_path, monkeypatch)
    d, status = bench.pmc_record(64, 65536, "full", "abc123")
    assert d["hbm_bytes_per_launch"] == 1.0 and status.startswith("current")
    d, status = bench.pmc_record(64, 65536, "full", "def456")
    assert d == {} and status.startswith("stale")
    d, status = bench.pmc_record(64, 65536, "full", None)
    assert d == {} and status.startswith("stale")


def test_pmc_record_without_stamp_is_stale(tmp_path, monkeypatch):
    _record(tmp_path, monkeypatch, srchash=None)
    d, status = bench.pmc_record(64, 65536, "full", "abc123")
    assert d == {} and "stale" in status


def test_pmc_record_of_another_workload(tmp_path, monkeypatch):
    _record(tmp_path, monkeypatch)
    assert bench.pmc_record(64, 1024, "full", "abc123")[0] == {}
    assert bench.pmc_record(64, 65536, "incremental", "abc123")[0] == {}
    assert bench.pmc_record(256, 65536, "full", "abc123")[1] == "no PMC record for this room"


class _FakeSession:
    def __init__(self, chains, n):
        rng = np.random.default_rng(1)
        self.pts = rng.standard_normal((chains, n, 6)).astype(np.float32)
        self.costs = rng.standard_normal((chains, 8)).astype(np.float32)

    def download(self):
        return self.pts, self.costs


def test_dump_outputs_whole_when_small(tmp_path):
    sess = _FakeSession(50, 4)
    bench.dump_outputs(sess, tmp_path / "out", 0, 1)
    pts, costs, rows = (np.load(tmp_path / "out" / f"{k}.npy")
                        for k in ("points", "costs", "sample_chains"))
    assert pts.dtype == np.float32 and costs.dtype == np.float32 and rows.dtype == np.float64
    assert np.array_equal(rows, np.arange(50))
    assert np.array_equal(pts, sess.pts) and np.array_equal(costs, sess.costs)


def test_dump_outputs_fixed_sample_when_large(tmp_path, monkeypatch):
    """Past the size cap the same seeded rows of points and costs are written on every run."""
    sess = _FakeSession(1000, 4)
    monkeypatch.setattr(bench, "DUMP_POINTS_BYTES", 100 * 4 * 6 * 4)
    for d, rank, world in (("a", 0, 1), ("b", 0, 1), ("c", 1, 2)):
        bench.dump_outputs(sess, tmp_path / d, rank, world)
    rows = np.load(tmp_path / "a" / "sample_chains.npy").astype(np.int64)
    assert len(rows) == 100 and len(set(rows)) == 100 and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "points.npy"), sess.pts[rows])
    assert np.array_equal(np.load(tmp_path / "a" / "costs.npy"), sess.costs[rows])
    for k in ("points", "costs", "sample_chains"):
        a = np.load(tmp_path / "a" / f"{k}.npy")
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{k}.npy"))
        assert np.array_equal(a, np.load(tmp_path / "c" / f"{k}_rank1.npy"))  # (rank-tagged)
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) < 64 << 20


def test_nccl_with_too_few_gpus_fails_loudly():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT="29555", MH_BENCH_BACKEND="nccl")
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "need 2 GPUs" in r.stderr


def test_committed_pmc_records_are_stamped():
    """Every committed PMC record carries the source hash of the library it profiled."""
    for p in (ROOT / "profiles").glob("pmc_step_kernel_n*.json"):
        d = json.loads(p.read_text())
        assert d.get("srchash"), p.name
