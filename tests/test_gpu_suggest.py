"""Suggestions on the MI355X: mh_session_suggest, KernelWrapperSuggest and mh_debug_suggest
against the numpy restatement of the selection rule (mh.suggest_reference) applied to the
session's own download(): chain ids, point bits and cost bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 16


def _same(got, want):
    ids, pts, costs = got
    rids, rpts, rcosts = want
    assert ids.tolist() == rids.tolist()
    assert np.array_equal(pts.view(np.uint32), rpts.view(np.uint32))
    assert np.array_equal(costs.view(np.uint32), rcosts.view(np.uint32))


@pytest.fixture(scope="module")
def finished(mh, hiplib):
    """Finalised sessions with their downloads, one per (n, chains, steps, seed), shared by the
    cases below and left unchanged by them."""
    made = {}

    def get(n, chains, steps, seed):
        key = (n, chains, steps, seed)
        if key not in made:
            s = mh.Session(mh.synthetic_room(n), chains, seed)
            s.run(steps)
            s.finalize()
            made[key] = (s,) + s.download()
        return made[key]

    yield get
    for s, _, _ in made.values():
        s.close()


# (n, chains, steps, seed, min_dist, picks of the rule, whether they differ from the plain top)
CHAIN_CASES = [
    (8, 1024, 200, 4242, 1.0, 16, False),
    (8, 1024, 200, 4242, 3.0, 16, True),
    (8, 1024, 200, 4242, 6.0, 2, True),
    (8, 1024, 200, 4242, 8.0, 1, False),
    (5, 300, 300, 4244, 3.0, 13, True),
    (5, 300, 300, 4244, 4.0, 7, True),
    (64, 512, 100, 4243, 18.0, 16, True),
    (64, 512, 100, 4243, 100.0, 1, False),
    (256, 128, 20, 4245, 30.0, 16, True),
    (256, 128, 20, 4245, 40.0, 7, True),
    (1, 64, 50, 4246, 0.5, 6, True),
    (1, 64, 50, 4246, 0.3, 12, True),
]


@pytest.mark.parametrize("n,chains,steps,seed,min_dist,m,differs", CHAIN_CASES)
def test_session_suggest_matches_rule(mh, finished, n, chains, steps, seed, min_dist, m, differs):
    s, pts, costs = finished(n, chains, steps, seed)
    want = mh.suggest_reference(pts, costs, K, min_dist)
    plain = mh.suggest_reference(pts, costs, K, 0.0)[0]
    # the case is what it was chosen for (a failure here is a failure, not a skip)
    assert len(want[0]) == m
    assert (want[0].tolist() != plain[:m].tolist()) == differs
    _same(s.suggest(K, min_dist), want)
    _same(s.suggest(K, 0.0), mh.suggest_reference(pts, costs, K, 0.0))  # plain top-k falls out
    if n == 8:
        assert s.step_kernel()[2] == "speculative"


def test_zero_steps_ties_by_global_id(mh, hiplib):
    """Every chain equals the initial layout: all totals tie and all distances are zero."""
    with mh.Session(mh.synthetic_room(8), 5, 7, chain_offset=1000) as s:
        s.finalize()
        pts, costs = s.download()
        assert len(np.unique(costs.view(np.uint32)[:, 0])) == 1
        ids, p, c = s.suggest(K, 0.0)  # a winner is always removed: m = 5 < k, by id
        assert ids.tolist() == [1000, 1001, 1002, 1003, 1004]
        _same((ids, p, c), mh.suggest_reference(pts, costs, K, 0.0, ids=np.arange(1000, 1005)))
        ids, p, c = s.suggest(K, 0.5)
        assert ids.tolist() == [1000]
        _same((ids, p, c), mh.suggest_reference(pts, costs, K, 0.5, ids=np.arange(1000, 1005)))


def test_repeat_and_resume(mh, hiplib):
    with mh.Session(mh.synthetic_room(8), 1024, 4242) as s:
        s.run(100)
        s.finalize()
        before = s.download()
        first = s.suggest(K, 3.0)
        _same(s.suggest(K, 3.0), first)
        after = s.download()  # the rounds leave the outputs untouched
        assert np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32))
        assert np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
        _same(first, mh.suggest_reference(*before, K, 3.0))
        s.run(100)
        s.finalize()
        pts, costs = s.download()
        assert not np.array_equal(pts.view(np.uint32), before[0].view(np.uint32))
        _same(s.suggest(K, 3.0), mh.suggest_reference(pts, costs, K, 3.0))
        _same(s.suggest(3, 6.0), mh.suggest_reference(pts, costs, 3, 6.0))


def test_best_tracking_and_tempering(mh, hiplib):
    room = mh.synthetic_room(64)
    with mh.Session(room, 996, 4243, track=2) as s:
        s.run(100)
        s.finalize()
        pts, costs = s.download()  # the best configurations
        _same(s.suggest(K, 18.0), mh.suggest_reference(pts, costs, K, 18.0))
    with mh.Session(room, 996, 4243, chain_offset=2000, track=2, temps=4, swap_interval=50,
                    beta_min=0.5) as s:
        s.run(100)
        s.finalize()
        pts, costs = s.download()
        gids = np.arange(2000, 2996)
        for md in (18.0, 0.0):
            got = s.suggest(K, md)
            _same(got, mh.suggest_reference(pts, costs, K, md, ids=gids, group=4))
            assert len(got[0]) >= 1 and (got[0] % 4 == 0).all()  # rung-0 outputs only
        # every candidate: 249 rung-0 outputs, each picked once
        got = s.suggest(256, 0.0)
        assert sorted(got[0].tolist()) == list(range(2000, 2996, 4))


def test_wrapper_suggest_and_sharding(mh, hiplib, monkeypatch):
    room = mh.synthetic_room(64)
    chains, steps, seed, md = 512, 100, 4243, 18.0
    monkeypatch.delenv("MH_DEVICES", raising=False)
    pts, costs = mh.kernel_wrapper(room, chains, steps, seed=seed)
    want = mh.suggest_reference(pts, costs, K, md)
    assert len(want[0]) == K
    one = mh.kernel_wrapper_suggest(room, chains, steps, seed, K, md)
    _same(one, want)
    monkeypatch.setenv("MH_DEVICES", "0,0")
    with pytest.raises(mh.MHError, match="listed twice"):
        mh.kernel_wrapper_suggest(room, 8, 1, seed, K, md)
    monkeypatch.setenv("MH_DEVICES_ALLOW_DUPLICATES", "1")
    _same(mh.kernel_wrapper_suggest(room, chains, steps, seed, K, md), one)
    monkeypatch.setenv("MH_DEVICES", "0,0,0")  # uneven shards
    _same(mh.kernel_wrapper_suggest(room, chains, steps, seed, K, md), one)
    _same(mh.kernel_wrapper_suggest(room, chains, steps, seed, 3, 100.0),
          mh.suggest_reference(pts, costs, 3, 100.0))
    # tracking and tempering groups over three shards against one
    kw = dict(track=2, temps=4, swap_interval=50, beta_min=0.5)
    sharded = mh.kernel_wrapper_suggest(room, 996, steps, seed, K, md, **kw)
    monkeypatch.delenv("MH_DEVICES")
    _same(sharded, mh.kernel_wrapper_suggest(room, 996, steps, seed, K, md, **kw))
    p4, c4 = mh.kernel_wrapper(room, 996, steps, seed=seed, **kw)
    _same(sharded, mh.suggest_reference(p4, c4, K, md, group=4))
    assert (sharded[0] % 4 == 0).all()


TOTALS = np.array([-2.5, -1.0, -0.5, 0.25, 1.0, 1.5, 3.0, 7.0], dtype=np.float32)
SPECIAL = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, np.nan, 0.0, -0.0], dtype=np.float32)


def _generated(rng, chains, n):
    """Layouts = one of five centres (coordinates on a 0.5 grid) with up to two objects moved by
    -0.25, 0 or +0.25 per axis, so layouts of one centre are 0, 0.25 or 0.5 apart per axis: with
    min_dist = 0.5, d2 lands on 0.25 == md2 exactly, below it and above it. Rows 0 and 1 are such a
    pair on purpose. Totals come from eight values with a few NaN, +-inf and +-0 mixed in."""
    centres = rng.integers(0, 32, (5, n, 2)).astype(np.float32) * np.float32(0.5)
    pts = rng.standard_normal((chains, n, 6)).astype(np.float32)
    which = rng.integers(0, 5, chains)
    pts[:, :, :2] = centres[which]
    for c in range(chains):
        for obj in rng.integers(0, n, 2):
            pts[c, obj, :2] += rng.integers(-1, 2, 2).astype(np.float32) * np.float32(0.25)
    if chains >= 2:
        pts[0, :, :2] = centres[0]
        pts[1, :, :2] = centres[0]
        pts[1, 0, 0] += np.float32(0.5)
    costs = rng.standard_normal((chains, 8)).astype(np.float32)
    costs[:, 0] = TOTALS[rng.integers(0, 8, chains)]
    odd = rng.random(chains) < 0.1
    costs[odd, 0] = SPECIAL[rng.integers(0, 8, int(odd.sum()))]
    if chains >= 2:
        costs[0, 0] = costs[1, 0] = np.float32(np.inf)  # the pair leads the order, by id
    return pts, costs


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 200, 256])
def test_debug_suggest_generated(mh, hiplib, n):
    rng = np.random.default_rng(0)
    for chains in (1, 63, 64, 65, 1000):
        pts, costs = _generated(rng, chains, n)
        if chains >= 2:  # the pair on the threshold: both kept at 0.5, one dropped one ulp above
            d = pts[1, :, :2] - pts[0, :, :2]
            assert float((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).max()) == 0.25
            assert mh.suggest_reference(pts, costs, K, 0.5)[0][:2].tolist() == [0, 1]
            wider = float(np.nextafter(np.float32(0.5), np.float32(1)))
            want = mh.suggest_reference(pts, costs, K, wider)[0].tolist()
            assert want[0] == 0 and 1 not in want
            assert mh.debug_suggest(pts, costs, K, wider).tolist() == want
        for k, md, group in ((K, 0.5, 1), (K, 0.0, 1), (5, 0.26, 1), (K, 0.5, 3), (256, 0.75, 1)):
            want = mh.suggest_reference(pts, costs, k, md, group=group)[0]
            got = mh.debug_suggest(pts, costs, k, md, group=group)
            assert got.tolist() == want.tolist(), (chains, k, md, group)
        if chains == 1000:  # elimination bites: the rule's picks are not the plain top
            assert mh.suggest_reference(pts, costs, K, 0.5)[0].tolist() != \
                mh.suggest_reference(pts, costs, K, 0.0)[0].tolist()


def test_debug_suggest_all_nan_is_empty(mh, hiplib):
    pts = np.zeros((70, 3, 6), dtype=np.float32)
    costs = np.full((70, 8), np.nan, dtype=np.float32)
    assert mh.debug_suggest(pts, costs, K, 1.0).tolist() == []
    costs[69, 0] = -np.inf
    assert mh.debug_suggest(pts, costs, K, 1.0).tolist() == [69]


@pytest.mark.parametrize("n,chains", [(64, 8300), (3, 66000)])
def test_debug_suggest_more_passes_than_workgroups(mh, hiplib, n, chains):
    """More candidates than one pass of the round's grid covers (2,048 workgroups of 256 / L
    candidates): every workgroup strides over several passes."""
    pts, costs = _generated(np.random.default_rng(1), chains, n)
    for k, md in ((K, 0.5), (K, 0.0), (40, 0.75)):
        want = mh.suggest_reference(pts, costs, k, md)[0]
        assert mh.debug_suggest(pts, costs, k, md).tolist() == want.tolist(), (k, md)
