"""Suggestions without a GPU: the mh_suggest_options layout, the header compiling as C99 and
C++17 with the new entry points, the numpy restatement of the selection rule on an example
worked out by hand, and KernelWrapperSuggest's validation (which returns before any HIP call).
The device selection itself is checked against the restatement in tests/test_gpu_suggest.py."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_suggest_options_layout(mh):
    so = mh.mh_suggest_options
    assert C.sizeof(so) == 32
    assert (so.k.offset, so.min_dist.offset, so.reserved.offset) == (0, 4, 8)
    assert so.k.size == 4 and so.min_dist.size == 4 and so.reserved.size == 24
    assert mh.STRUCT_LAYOUT[so] == (32, {"k": 0, "min_dist": 4, "reserved": 8})
    o = mh.suggest_options(16, 2.0)
    assert (o.k, o.min_dist, list(o.reserved)) == (16, 2.0, [0] * 6)
    assert {"mh_session_suggest", "KernelWrapperSuggest", "mh_debug_suggest"} <= set(mh.EXPORTS)


@pytest.mark.parametrize("lang,compiler,std", [("c", "gcc", "-std=c99"), ("c++", "g++", "-std=c++17")])
def test_header_with_suggest_compiles_and_links(mh, tmp_path, lang, compiler, std):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text("""
#include "mh_kernel.h"
#include <stdio.h>
int main(void) {
    mh_suggest_options o = {16, 2.0f, {0, 0, 0, 0, 0, 0}};
    result* (*kws)(relationshipStruct*, relationshipAngleStruct*, positionAndRotation*,
                   rectangle*, rectangle*, vertex*, vertex*, Surface*, gpuConfig*,
                   const mh_options*, const mh_suggest_options*, int32_t*, int64_t*) =
        KernelWrapperSuggest;
    int (*ss)(mh_session*, const mh_suggest_options*, int64_t*, point*, resultCosts*) =
        mh_session_suggest;
    int (*ds)(const point*, const resultCosts*, int64_t, int, int, const mh_suggest_options*,
              int64_t*) = mh_debug_suggest;
    printf("%d %d %p %p %p\\n", (int)sizeof o, o.k, (void*)kws, (void*)ss, (void*)ds);
    return sizeof(mh_suggest_options) == 32 ? 0 : 1;
}
""")
    exe = tmp_path / "t"
    subprocess.run([compiler, std, "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src),
                    "-o", str(exe), str(mh.LIB_PATH), f"-Wl,-rpath,{mh.LIB_PATH.parent}"],
                   check=True)


def _example():
    """Six layouts of two objects, min_dist = 0.5 (md2 = 0.25 exactly). Object 1 sits at (1, 1)
    everywhere, so d2 is decided by object 0:

      row  total  object 0          note
      0    5.0    (0, 0)
      1    5.0    (0.5, 0)          ties with row 0 (lower id first); d2 to row 0 == 0.25 == md2
      2    NaN    (10, 10)          far from everything, but never a candidate
      3    4.0    (0.5 - 2^-25, 0)  d2 to row 0 = fl((0.5 - 2^-25)^2) = 0.25 - 2^-25 < md2
      4    -0.0   (3, 3)            ties with row 5 (-0 == +0): lower id first
      5    +0.0   (6, 6)
    """
    below = np.nextafter(np.float32(0.5), np.float32(0))
    assert float(below) == 0.5 - 2.0 ** -25
    pts = np.zeros((6, 2, 6), dtype=np.float32)
    pts[:, 1, :2] = 1.0
    for row, xy in enumerate([(0, 0), (0.5, 0), (10, 10), (below, 0), (3, 3), (6, 6)]):
        pts[row, 0, :2] = xy
    pts[:, :, 2:] = np.arange(6 * 2 * 4, dtype=np.float32).reshape(6, 2, 4)  # (ignored: z, rotations)
    costs = np.arange(6 * 8, dtype=np.float32).reshape(6, 8)
    costs[:, 0] = [5.0, 5.0, np.nan, 4.0, -0.0, 0.0]
    return pts, costs


def test_suggest_reference_hand_example(mh):
    pts, costs = _example()
    # Order: 0, 1 (tie at 5.0, by id), 3 (4.0), 4, 5 (tie at zero, by id); 2 is NaN.
    # Picks: 0. 1: d2 to 0 is exactly md2, not below: kept. 3: d2 to 0 is 0.25 - 2^-25 < md2:
    # dropped. 4 and 5: metres away from every pick: kept, in id order.
    ids, p, c = mh.suggest_reference(pts, costs, 6, 0.5)
    assert ids.dtype == np.int64 and ids.tolist() == [0, 1, 4, 5]
    assert np.array_equal(p.view(np.uint32), pts[[0, 1, 4, 5]].view(np.uint32))
    assert np.array_equal(c.view(np.uint32), costs[[0, 1, 4, 5]].view(np.uint32))
    # k cuts the walk short
    assert mh.suggest_reference(pts, costs, 2, 0.5)[0].tolist() == [0, 1]
    assert mh.suggest_reference(pts, costs, 3, 0.5)[0].tolist() == [0, 1, 4]
    # min_dist = 0: plain top-k (a pick is still removed; NaN still never picked)
    assert mh.suggest_reference(pts, costs, 6, 0.0)[0].tolist() == [0, 1, 3, 4, 5]
    # one ulp more and row 1 is the same suggestion as row 0 (the comparison is strict at 0.5)
    wider = float(np.nextafter(np.float32(0.5), np.float32(1)))
    assert mh.suggest_reference(pts, costs, 6, wider)[0].tolist() == [0, 4, 5]
    # group = 2: rows 0, 2, 4 are the candidates; 2 is NaN
    assert mh.suggest_reference(pts, costs, 6, 0.5, group=2)[0].tolist() == [0, 4]
    # global ids break the ties: with ids reversed row 1 (id 14) goes before row 0 (id 15) and
    # row 5 (id 10) before row 4 (id 11); row 3 is then dropped by row 1 (dx = 2^-25)
    ids, p, _ = mh.suggest_reference(pts, costs, 6, 0.5, ids=[15, 14, 13, 12, 11, 10])
    assert ids.tolist() == [14, 15, 10, 11]
    assert np.array_equal(p.view(np.uint32), pts[[1, 0, 5, 4]].view(np.uint32))


def test_suggest_reference_infinities_and_empty(mh):
    pts = np.zeros((4, 1, 6), dtype=np.float32)
    pts[:, 0, 0] = [0, 10, 20, 30]
    costs = np.zeros((4, 8), dtype=np.float32)
    costs[:, 0] = [-np.inf, np.inf, np.nan, 1.0]
    assert mh.suggest_reference(pts, costs, 4, 1.0)[0].tolist() == [1, 3, 0]
    costs[:, 0] = np.nan
    ids, p, c = mh.suggest_reference(pts, costs, 4, 1.0)
    assert ids.shape == (0,) and p.shape == (0, 1, 6) and c.shape == (0, 8)


def _suggest(hiplib, mh, room, sopts, n_out=True, reserved=None):
    g = mh.abi.gpuConfig(4, 0, 64, 0, 0, 10)
    opts = mh.abi.options(1)
    m = C.c_int32(-7)
    if sopts is not None and reserved is not None:
        sopts.reserved[reserved] = 1
    return hiplib.KernelWrapperSuggest(*room.args(), C.byref(g), C.byref(opts),
                                       C.byref(sopts) if sopts is not None else None,
                                       C.byref(m) if n_out else None, None)


@pytest.mark.parametrize("k,min_dist,reserved,needle", [
    (0, 1.0, None, "mh_suggest_options.k"),
    (257, 1.0, None, "mh_suggest_options.k"),
    (-1, 1.0, None, "mh_suggest_options.k"),
    (16, -1.0, None, "min_dist"),
    (16, float("nan"), None, "min_dist"),
    (16, float("inf"), None, "min_dist"),
    (16, 1.0, 0, "reserved"),
    (16, 1.0, 5, "reserved"),
])
def test_wrapper_suggest_rejects_bad_options(mh, hiplib, k, min_dist, reserved, needle):
    """Validation precedes the first HIP call, so this runs without a GPU."""
    room = mh.main_fixture()
    assert not _suggest(hiplib, mh, room, mh.suggest_options(k, min_dist), reserved=reserved)
    assert needle in mh.last_error(hiplib)


def test_wrapper_suggest_rejects_null_arguments(mh, hiplib):
    room = mh.main_fixture()
    assert not _suggest(hiplib, mh, room, None)
    assert "sopts" in mh.last_error(hiplib)
    assert not _suggest(hiplib, mh, room, mh.suggest_options(16, 1.0), n_out=False)
    assert "n_out" in mh.last_error(hiplib)
    # the other entry points validate the same way before touching a device
    ids = (C.c_int64 * 16)()
    pts = (mh.abi.point * 2)()
    cs = (mh.abi.resultCosts * 2)()
    bad = mh.suggest_options(0, 1.0)
    assert hiplib.mh_debug_suggest(pts, cs, 2, 1, 1, C.byref(bad), ids) == -1
    assert "mh_suggest_options.k" in mh.last_error(hiplib)
    assert hiplib.mh_debug_suggest(pts, cs, 2, 1, 1, None, ids) == -1
    assert hiplib.mh_session_suggest(None, C.byref(mh.suggest_options(1, 0.0)), ids, None, None) == -1
