"""Times mh_session_suggest against what a caller pays without it, mh_session_download of every
chain (DESIGN.md "Suggestions"; the record is profiles/suggest_n64.txt).

    python tools/suggest_timing.py [--n 64] [--chains 65536] [--steps 1000] [--k 16]
                                   [--min-dist 2.0] [--runs 10] [--trace]

Both are warmed up, then timed `runs` times each on the wall clock around the C call (outputs
preallocated; no Python copies inside the timed region); medians are reported. --trace runs two
suggest calls and nothing else after the set-up, for a kernel trace that gives every round
kernel's device time (rocprofv3 --kernel-trace --stats -- python tools/suggest_timing.py --trace;
the rounds run on the session's own stream inside one synchronous call, so events recorded from
outside cannot bracket a single round)."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import __graft_entry__ as graft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--min-dist", type=float, default=2.0)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    mh = graft.load_package()
    lib = mh.load_library()
    room = mh.synthetic_room(a.n)
    s = mh.Session(room, a.chains, 20251015)
    s.run(a.steps)
    s.finalize()
    s.summary()  # (synchronises)
    pts = (mh.abi.point * (a.chains * a.n))()
    cs = (mh.abi.resultCosts * a.chains)()
    so = mh.suggest_options(a.k, a.min_dist)
    ids = (C.c_int64 * a.k)()
    spts = (mh.abi.point * (a.k * a.n))()
    scs = (mh.abi.resultCosts * a.k)()

    def download():
        t = time.perf_counter()
        rc = lib.mh_session_download(s.h, pts, cs)
        dt = time.perf_counter() - t
        assert rc == 0, mh.last_error(lib)
        return dt

    def suggest():
        t = time.perf_counter()
        m = lib.mh_session_suggest(s.h, C.byref(so), ids, spts, scs)
        dt = time.perf_counter() - t
        assert m >= 0, mh.last_error(lib)
        return dt, m

    out = {"n": a.n, "chains": a.chains, "steps": a.steps, "k": a.k, "min_dist": a.min_dist,
           "runs": a.runs}
    if a.trace:
        suggest()
        suggest()
        print(json.dumps({"trace": True, **out}))
        return
    for _ in range(2):
        download()
    times = [download() for _ in range(a.runs)]
    out["download_ms"] = {"median": 1e3 * statistics.median(times), "min": 1e3 * min(times),
                          "max": 1e3 * max(times)}
    for _ in range(2):
        suggest()
    res = [suggest() for _ in range(a.runs)]
    times = [r[0] for r in res]
    out["suggest_ms"] = {"median": 1e3 * statistics.median(times), "min": 1e3 * min(times),
                         "max": 1e3 * max(times)}
    out["m"] = res[-1][1]
    # the picks are the rule's (numpy restatement on the download)
    p = np.frombuffer(bytes(pts), dtype=np.float32).reshape(a.chains, a.n, 6)
    c = mh.abi.costs_to_array(cs)
    want = mh.suggest_reference(p, c, a.k, a.min_dist)[0].tolist()
    out["matches_reference"] = list(ids[:out["m"]]) == want
    out["plain_top_k_distinct_from_picks"] = want != mh.suggest_reference(p, c, a.k, 0.0)[0].tolist()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
