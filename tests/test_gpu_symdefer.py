"""Symmetry rows carried as marked estimates across the steps the rejection bound decides
(eval_costs FAST in mh_chain.hip; DESIGN.md "Marked symmetry rows"): the plain full-evaluation
step with one chain per wavefront, in both of its instances -- the few-chains one these chain
counts get by default and the register-capped one config 3 runs ($MH_STEP_FEW=0). Every case is
compared bit for bit with the oracle; the check build's counters bound how often the exact pair
value is still evaluated.
"""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from parity_util import check_chains

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

INSTANCES = ["few", "capped"]
KEEP = [0, 1, 2, 3, 4, 5, 7]  # all but OffLimits, which the step path does not evaluate
SYM = 4  # resultCosts.SymmetryCosts
# Chosen on the oracle alone (64 chains x 600 steps, seed 5316): a 50 m room, 44.8 % of the steps
# accepted, the final Symmetry cost zero on 15 chains and non-zero on 49. (Scale 3: no chain at
# zero; scale 10: 42 of 64.)
FLOOR_SCALE = 5.0


def _use_full_step(monkeypatch, instance: str):
    monkeypatch.setenv("MH_DELTA", "0")
    monkeypatch.setenv("MH_SPEC", "0")
    if instance == "capped":
        monkeypatch.setenv("MH_STEP_FEW", "0")
    else:
        monkeypatch.delenv("MH_STEP_FEW", raising=False)


def _is_full(session) -> bool:
    return session.step_kernel()[2].split("-")[0] == "full"


def zero_floor_room(mh, scale: float = FLOOR_SCALE):
    """synthetic_room(16) with the object positions and the room rectangle (and the centroid and
    focal point that go with it) scaled, so that many pair distances straddle 25 m, where the
    pair value 5 - sqrt(d) - 0.4 |dtheta| changes sign and a row's maximum meets its 0 floor."""
    room = mh.synthetic_room(16)
    for i in range(room.n):
        room.cfg[i].x *= scale
        room.cfg[i].y *= scale
    for k in range(4):
        room.surface_rectangle[k].x *= scale
        room.surface_rectangle[k].y *= scale
    for f in ("centroidX", "centroidY", "focalX", "focalY"):
        setattr(room.srf, f, getattr(room.srf, f) * scale)
    return room


@pytest.mark.parametrize("instance", INSTANCES)
@pytest.mark.parametrize("n", [9, 64])
def test_launch_ends(mh, orc, hiplib, monkeypatch, instance, n):
    """40 launches of one step, then 37 and 3: marked rows never cross a launch. The costs a
    chain carries after each of the first launches equal those of a finalized copy, and the 80
    steps are the oracle's."""
    _use_full_step(monkeypatch, instance)
    room = mh.synthetic_room(n)
    chains, seed = 64, 5100 + n
    with mh.Session(room, chains, seed=seed) as s, mh.Session(room, chains, seed=seed) as copy:
        assert _is_full(s) and _is_full(copy)
        for k in range(40):
            s.run(1)
            if k < 4:
                copy.run(1)
                copy.finalize()
                _, fresh = copy.download()
                cur = s.current_costs()
                assert np.array_equal(cur[:, KEEP].view(np.uint32), fresh[:, KEEP].view(np.uint32)), k
        s.run(37)
        s.run(3)
        s.finalize()
        pts, costs = s.download()
    ref_pts, ref_costs, _ = orc.run_chains(room, chains, 80, seed, threads=8)
    check_chains(f"launch ends {instance} N={n}", pts, costs, ref_pts, ref_costs)


@pytest.mark.parametrize("instance", INSTANCES)
@pytest.mark.parametrize("slack", ["1", "1e6"])
@pytest.mark.parametrize("n", [8, 16])
def test_tied_estimates(mh, orc, hiplib, monkeypatch, instance, slack, n):
    """Objects 1..N/2-1 stacked on object 0, every second one frozen: the rows' estimates tie
    exactly for the whole run, so no row may be taken on its estimates."""
    _use_full_step(monkeypatch, instance)
    monkeypatch.setenv("MH_BOUND_SLACK", slack)
    room = mh.synthetic_room(n)
    p0 = room.cfg[0]
    for i in range(1, n // 2):
        room.cfg[i].x, room.cfg[i].y, room.cfg[i].rotY = p0.x, p0.y, p0.rotY
        room.cfg[i].frozen = i % 2 == 1
    chains, steps, seed = 64, 500, 5200 + n
    with mh.Session(room, chains, seed=seed) as s:
        assert _is_full(s)
        s.run(steps)
        s.finalize()
        pts, costs = s.download()
    ref_pts, ref_costs, _ = orc.run_chains(room, chains, steps, seed, threads=8)
    check_chains(f"ties {instance} slack {slack} N={n}", pts, costs, ref_pts, ref_costs)


@pytest.fixture(scope="module")
def floor_reference(mh, orc):
    room = zero_floor_room(mh)
    chains, steps, seed = 64, 600, 5316
    ref = orc.run_chains(room, chains, steps, seed, threads=8)
    return room, chains, steps, seed, ref


@pytest.mark.parametrize("instance", INSTANCES)
def test_zero_floor(mh, orc, hiplib, monkeypatch, instance, floor_reference):
    """Pair values around zero: estimates whose sign is not certain, rows that fall to the
    floor and rise from it."""
    _use_full_step(monkeypatch, instance)
    room, chains, steps, seed, (ref_pts, ref_costs, ref_acc) = floor_reference
    assert ref_acc.sum() >= chains * steps // 20
    zero = ref_costs[:, SYM] == 0
    assert zero.any() and (~zero).any(), int(zero.sum())
    with mh.Session(room, chains, seed=seed) as s:
        assert _is_full(s)
        s.run(steps)
        s.finalize()
        pts, costs = s.download()
    check_chains(f"zero floor {instance}", pts, costs, ref_pts, ref_costs)


def test_running_costs_equal_fresh_capped(mh, hiplib, monkeypatch):
    """After many proposals accepted on the bound (their rows committed as estimates), the
    costs a chain carries equal a fresh evaluation of its state, bit for bit."""
    _use_full_step(monkeypatch, "capped")
    room = mh.synthetic_room(64)
    chains, steps = 256, 300
    with mh.Session(room, chains, seed=5464) as s:
        assert _is_full(s)
        s.run(steps)
        s.finalize()
        _, fresh = s.download()
        running = s.current_costs()
        acc = s.summary().accepted
    assert acc > chains * steps // 20
    same = np.all(running[:, KEEP].view(np.uint32) == fresh[:, KEEP].view(np.uint32), axis=1)
    assert same.all(), f"{(~same).sum()} of {chains} chains drifted"


def test_check_build_counters(mh):
    """The check build on config 3's room: every marked row verified each step against a fresh
    exact scan (0 violations), and the exact pair value evaluated no more often than the steps
    that need exact rows: open steps, exact passes of the current configuration, resolutions of
    overlapping estimates and launch ends. Resolutions stay below 1 % of the steps."""
    lib = mh.LIB_PATH.with_name("libmhgpu_check.so")
    assert lib.exists(), "run __graft_entry__.build() (it builds libmhgpu_check.so)"
    chains, steps = 1024, 500
    out = subprocess.run([sys.executable, str(ROOT / "tools" / "bound_check.py"), "--one", "syn",
                          "64", str(chains), str(steps), "full"],
                         capture_output=True, text=True, timeout=120, cwd=ROOT)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("[bound]")][-1]
    assert "violations 0" in line, line
    m = re.search(r"symmetry rows: (\d+) exact passes, (\d+) overlap resolutions, (\d+) marked rows "
                  r"in (\d+) exactifying passes, (\d+) open steps, (\d+) exact current passes, "
                  r"(\d+) launches", line)
    assert m, line
    passes, overlaps, marked, exactify, open_, exact_cur, launches = map(int, m.groups())
    total = chains * steps
    print(f"per chain-step: exact passes {passes / total:.5f}, overlap resolutions "
          f"{overlaps / total:.5f}, open {open_ / total:.5f}, exact current {exact_cur / total:.5f}; "
          f"marked rows per exactifying pass {marked / max(exactify, 1):.2f}")
    assert passes <= open_ + exact_cur + overlaps + chains * launches
    assert overlaps < total // 100
