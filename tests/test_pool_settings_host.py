"""The argument errors of the pool entry points, one bad setting per case:
every public entry point that accepts the keyword raises the same exception
type with the same fixed text, before any engine is made (no GPU here).

The texts are the ones the entry points have always raised, written out: a
change of wording, or of which check wins, fails here.
"""
import numpy as np
import pytest

from hyperopt_amd import Domain, hp, tpe
from tests import joint_util as U

BATCH_LIAR = ("batch='liar' is supported with joint=True on a Pool or a SampledPool "
              "(suggest_from_pool, suggest_sampled, pick_batch)")
GRID_JOINT = ("the joint criterion is not separable over the axes of a GridPool; build the grid "
              "with GridPool(..., joint=True), which scores it from per-axis factor tables, or "
              "score its rows as a Pool (GridPool.to_pool())")
GRID_DISTINCT = ("GridPool rows are distinct by construction; exclude evaluated rows with "
                 "GridPool.exclude")
IDS = [100, 101]


def _problem():
    domain = Domain(lambda x: 0, {"a": hp.choice("a", [0, 1]), "q": hp.quniform("q", 0, 4, 1)})
    trials = U.make_trials(domain, [], [])
    pool = tpe.Pool(domain, [{"a": 0, "q": 1.0}, {"a": 1, "q": 2.0}, {"a": 1, "q": 3.0}])
    return domain, trials, pool


def _grid(domain, **kw):
    return tpe.GridPool(domain, {"a": [0, 1], "q": [0, 1, 2]}, **kw)


def _from_pool(pool=None, **kw):
    domain, trials, own = _problem()
    pool = own if pool is None else pool
    return lambda: tpe.suggest_from_pool(IDS, domain, trials, 0, pool=pool, **kw)


def _sampled(**kw):
    domain, trials, _pool = _problem()
    return lambda: tpe.suggest_sampled(IDS, domain, trials, 0, **kw)


def _pick(pool=None, **kw):
    domain, trials, own = _problem()
    pool = own if pool is None else pool
    return lambda: tpe.pick_batch(domain, trials, pool, 2, **kw)


def _score(pool=None, **kw):
    domain, trials, own = _problem()
    pool = own if pool is None else pool
    return lambda: tpe.score_configs(domain, trials, pool, **kw)


def _sample(**kw):
    domain, trials, _pool = _problem()
    return lambda: tpe.Pool.sample(domain, trials, 0, 8, **kw)


def _joint_everywhere(**kw):
    """Every entry point that takes ``bandwidth`` / ``cat_smoothing``."""
    return [_from_pool(joint=True, **kw), _sampled(joint=True, **kw), _pick(**kw),
            _score(joint=True, **kw), _sample(joint=True, **kw),
            _from_pool(joint="tree", **kw), _score(joint="tree", **kw)]


def _cases():
    domain, _trials, _pool = _problem()
    plain, planned = _grid(domain), _grid(domain, joint=True)
    other = tpe.Pool(Domain(lambda x: 0, {"z": hp.uniform("z", 0, 1)}), [{"z": 0.5}])
    liar = dict(batch="liar", joint=True)
    yield "batch other than liar", ": None or 'liar'", [
        _from_pool(batch="kriging", joint=True), _sampled(batch="kriging", joint=True),
        _from_pool(batch="kriging"), _sampled(batch="kriging")]
    for w in (0.0, float("inf"), float("nan")):
        yield "lie_weight %r" % w, "must be a finite number > 0", [
            _from_pool(lie_weight=w, **liar), _sampled(lie_weight=w, **liar), _pick(lie_weight=w)]
    yield "liar without joint", BATCH_LIAR + "; the factorised criterion (joint=False)", [
        _from_pool(batch="liar"), _sampled(batch="liar")]
    yield "liar with tree", BATCH_LIAR + "; joint='tree' keeps no log L_above per group", [
        _from_pool(batch="liar", joint="tree"), _sampled(batch="liar", joint="tree")]
    yield "liar on a grid", BATCH_LIAR + "; a GridPool has no row values to lie with", [
        _from_pool(pool=planned, **liar), _pick(pool=planned), _pick(pool=plain)]
    for bw in (0.0, -0.2):
        yield "bandwidth %r" % bw, "must be > 0, cat_smoothing=", _joint_everywhere(bandwidth=bw)
    yield "cat_smoothing < 0", "must be > 0, cat_smoothing=-0.5 >= 0", \
        _joint_everywhere(cat_smoothing=-0.5)
    yield "draw joint without joint", "draw='joint' draws from the joint criterion's below " \
        "mixture: it needs joint=True", [_sampled(draw="joint")]
    yield "unknown draw", "draw='both': 'factorised' or 'joint'", [
        _sampled(draw="both"), _sampled(draw="both", joint=True)]
    yield "distinct on a grid", GRID_DISTINCT, [
        _from_pool(pool=plain, distinct=True), _from_pool(pool=planned, distinct=True, joint=True),
        lambda: tpe.distinct_rows(plain)]
    yield "joint on a grid without its plan", GRID_JOINT, [
        _from_pool(pool=plain, joint=True), _from_pool(pool=plain, joint="tree"),
        _score(pool=plain, joint=True), _score(pool=plain, joint="tree")]
    yield "a pool of another space", "the pool was built for another space (labels differ)", [
        _from_pool(pool=other), _from_pool(pool=other, joint=True), _pick(pool=other),
        _score(pool=other), _score(pool=other, joint=True),
        lambda: tpe.distinct_rows(other, domain=domain)]


CASES = list(_cases())


@pytest.fixture(autouse=True)
def _no_engine(monkeypatch):
    def engine():
        raise AssertionError("the check came after the engine was made")
    monkeypatch.setattr(tpe, "engine", engine)


@pytest.mark.parametrize("text,calls", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_bad_setting_raises_the_same_error_everywhere(text, calls):
    for call in calls:
        with pytest.raises(ValueError) as e:
            call()
        assert text in str(e.value)


def test_error_precedence_of_suggest_from_pool():
    """Where several checks could fire, the order is: no pool, ``distinct`` on
    a grid, the joint keywords, the batch, a grid without the plan, another
    space."""
    domain, trials, _pool = _problem()
    other = Domain(lambda x: 0, {"z": hp.uniform("z", 0, 1)})
    plain = _grid(domain)
    bad = dict(distinct=True, joint=True, bandwidth=0.0, batch="kriging")
    with pytest.raises(TypeError, match="needs pool="):
        tpe.suggest_from_pool(IDS, other, trials, 0, **bad)
    for drop, text in ((), GRID_DISTINCT), (("distinct",), "must be > 0, cat_smoothing="), \
            (("distinct", "bandwidth"), ": None or 'liar'"), \
            (("distinct", "bandwidth", "batch"), GRID_JOINT):
        kw = {k: v for k, v in bad.items() if k not in drop}
        with pytest.raises(ValueError) as e:
            tpe.suggest_from_pool(IDS, other, trials, 0, pool=plain, **kw)
        assert text in str(e.value)
    with pytest.raises(ValueError, match="labels differ"):
        tpe.suggest_from_pool(IDS, other, trials, 0, pool=_grid(domain, joint=True), joint=True)
    assert np.count_nonzero(plain.taken) == 0
