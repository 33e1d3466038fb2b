"""tests/lazy_ref.py (the numpy restatement of the verdict stage, towr_gpu_alsolve_verdict_batch_device, and the GN
iterations that carry it): every branch of the verdict on a small quadratic, and the identity that defines the feature —
on the monoped's six starts the lazy loop's state is bit-equal to the eager loop's after every iteration, with and
without probes, while the direction runs only in the iterations whose candidate the line search takes. No GPU."""
import copy

import numpy as np
import pytest

from tests import alsolve_ref as R
from tests import lazy_ref as LZ
from tests import probe_ref as PR
from tests.test_chol_ref import SOLVE_SEEDS
from tests.test_pgn_ref import SOLVE_PAR
from tests.test_probe_ref import _monoped_memo

NAN = np.float64(np.nan)
N = 4
INT32_MIN = -2 ** 31


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- the verdict on a quadratic -------------------------------------------------------------------------------------------
# merit = 0.5 |x - 1|^2 from X = 0 (m0 = 2) with GR = -1 and the candidate at u in every column: gs = -4 u, and the
# Armijo test passes iff 0.5 * 4 (u - 1)^2 <= 2 - 4 c1 u, i.e. u <= 2 (1 - c1). The merit is split into FC and RSUM[3].
def _st(u=1.0, phase=R.SEARCH, m0=2.0, split=0.25):
    mc = 0.5 * N * (u - 1.0) ** 2
    return dict(X=np.zeros(N), GR=-np.ones(N), XC=np.full(N, u), FC=np.float64(mc - split), RSUM=np.array([0.5, 0.0, 0.0, split, 0.0]),
                SCAL=np.array([m0, 0.5, 0.1, 0.1, 0.4, 0.75, 0.0, 0.0]), ISTATE=np.array([phase, 3, 3, 2], dtype=np.int32))


PAR = R.params(c1=1e-4)


def _verdict(st, **kw):
    before = copy.deepcopy(st)
    w = LZ.verdict(st, PAR, **kw)
    for k in before:   # the stage writes nothing of the state
        assert np.array_equal(_bits(before[k]) if before[k].dtype.kind == "f" else before[k],
                              _bits(st[k]) if np.asarray(st[k]).dtype.kind == "f" else st[k]), k
    return w


def test_restart_always_runs():
    assert _verdict(_st(u=1.0, phase=R.RESTART)) == 0
    # whatever the operands hold: the line search takes a RESTART candidate without a test
    st = _st(u=100.0, phase=R.RESTART, m0=NAN)
    st["FC"] = NAN
    st["GR"][:] = NAN
    assert _verdict(st) == 0


def test_search_passing():
    assert _verdict(_st(u=1.0)) == 0
    assert _verdict(_st(u=1.9)) == 0
    # gs = 0 passes when the merit does (XC = X, the merit at m0)
    st = _st(u=0.0)
    assert st["FC"] + st["RSUM"][3] == 2.0 and _verdict(st) == 0


def test_search_failing_on_ascent():
    # gs = +4 u > 0 fails whatever the merit
    st = _st(u=1.0)
    st["GR"] = np.ones(N)
    st["FC"] = np.float64(-100.0)
    assert _verdict(st) == 2


def test_search_failing_on_armijo():
    assert _verdict(_st(u=2.0)) == 2        # mc = 2 > 2 - 8 c1
    assert _verdict(_st(u=8.0)) == 2
    # the tie: mc == m0 + c1 gs passes, the next double above fails
    st = _st(u=1.0)
    rhs = np.float64(2.0) + np.float64(1e-4) * np.float64(-4.0)
    st["FC"], st["RSUM"][3] = rhs, 0.0
    assert _verdict(st) == 0
    st["FC"] = np.nextafter(rhs, np.inf)
    assert _verdict(st) == 2


@pytest.mark.parametrize("where", ["FC", "RSUM3", "M0", "GR", "XC"])
def test_a_nan_fails(where):
    st = _st(u=1.0)
    assert _verdict(st) == 0
    if where == "FC":
        st["FC"] = NAN
    elif where == "RSUM3":
        st["RSUM"][3] = NAN
    elif where == "M0":
        st["SCAL"][0] = NAN
    else:
        st[where][2] = NAN
    assert _verdict(st) == 2


@pytest.mark.parametrize("phase", [2, 3, 4, 5, 6, 7, -1, INT32_MIN])
def test_frozen_and_garbage_words_skip(phase):
    assert _verdict(_st(u=1.0, phase=phase)) == 2


def test_the_sum_is_a_parameter_and_the_batch_form_counts():
    # both sums give the verdicts above; the device's tree is the default
    for u, w in ((1.0, 0), (2.0, 2)):
        assert _verdict(_st(u=u), gsum=np.sum) == w and _verdict(_st(u=u), gsum=PR.device_tree) == w
    sts = [_st(u=1.0), _st(u=2.0), _st(u=1.0, phase=R.RESTART), _st(u=1.0, phase=3)]
    h = dict(X=np.stack([s["X"] for s in sts]), GR=np.stack([s["GR"] for s in sts]), XC=np.stack([s["XC"] for s in sts]),
             FC=np.array([s["FC"] for s in sts]), SCAL=np.stack([s["SCAL"] for s in sts]), RSUM=np.stack([s["RSUM"] for s in sts]),
             ISTATE=np.concatenate([s["ISTATE"] for s in sts]), VERDICT=np.full(4, -7, dtype=np.int32),
             NDIR=np.array([5, 5, 5, 5], dtype=np.int32))
    LZ.verdict_batch(h, PAR, N)
    assert list(h["VERDICT"]) == [0, 2, 0, 2] and list(h["NDIR"]) == [6, 5, 6, 5]
    h["NDIR"] = None
    LZ.verdict_batch(h, PAR, N)
    assert list(h["VERDICT"]) == [0, 2, 0, 2]


# ---- the identity: the lazy loop's state is the eager loop's ---------------------------------------------------------------
STATE_KEYS = ("X", "GR", "XC", "GRC", "D", "LAM", "LAMP", "HS", "HY", "HMETA", "ALPHA", "RHO", "FC", "SCAL", "ISTATE", "RSUM",
              "SSUM", "USUM", "LSUM")
CAP = 400
# the directions of the lazy loop per start (seeds 900 .. 905): SOLVE_PAR without probes, and shrink = 0.5 with T = 2. The
# first row is the sequential loop's iterations minus its refused trials (67 / 9 / 39 / 32 / 10 / 12
# iterations, 28 / 0 / 14 / 11 / 0 / 0 refused)
NDIR_REF = {None: (39, 9, 25, 21, 10, 12)}


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(a, b) if a.dtype.kind == "i" else np.array_equal(_bits(a), _bits(b))


def _pair_run(seed, shrink, T):
    """The eager and the lazy loop side by side from x0 + 0.05 randn(seed) until frozen: the states are compared after
    every iteration. Returns (iterations, rejected trials, NDIR, the verdicts)."""
    o, x0, lo, up, ev, direct_for = _monoped_memo()
    par = R.params(**{**SOLVE_PAR, "shrink": shrink})
    new = lambda: R.new_state(o.n, o.m, par["mem"], x0 + 0.05 * np.random.default_rng(seed).standard_normal(o.n),
                              n_rsum=4 + o.desc.n_constraints, n_ssum=5 + o.desc.n_varsets)
    eager, lazy = new(), new()
    R.init(eager, par, lo, up)
    R.init(lazy, par, lo, up)
    trace, ltrace, verdicts = [], [], []
    while len(trace) < CAP and eager["ISTATE"][0] < R.CONVERGED:
        PR.iterate(eager, par, None, T, ev, lo, up, direct_for(eager), 8, 1, None, trace)
        LZ.iterate(lazy, par, None, T, ev, lo, up, direct_for(lazy), 8, 1, None, ltrace, None, verdicts)
        tag = f"seed {seed} T {T} iteration {len(trace)}"
        for k in STATE_KEYS:
            assert _same(eager[k], lazy[k]), f"{tag}: {k}"
        assert trace[-1] == ltrace[-1], tag
        code = trace[-1][0]
        assert verdicts[-1] == (0 if code in (1, 2) else 2), f"{tag}: verdict {verdicts[-1]}, the line search's code {code}"
        if code in (1, 2):   # the direction the select step has just read is the eager loop's
            assert _same(eager["DC"], lazy["DC"]) and _same(eager["GSUM"], lazy["GSUM"]), f"{tag}: DC / GSUM"
    assert eager["ISTATE"][0] >= R.CONVERGED, f"seed {seed}: not frozen after {CAP} iterations"
    rejected = sum(1 for t in trace if t[0] not in (1, 2))
    return len(trace), rejected, int(lazy["NDIR"]), verdicts


@pytest.mark.parametrize("shrink,T", [(SOLVE_PAR["shrink"], None), (0.5, 2)])
def test_lazy_loop_is_the_eager_loop(shrink, T):
    """Seeds 900 .. 905, SOLVE_PAR, mu = 1e-6, the tiled reference, without probes and with T = 2 at shrink = 0.5: every
    state array is bit-equal after every iteration, the verdict is 0 exactly where the line search's code is 1 or 2, and
    NDIR = iterations - rejected trials."""
    counts, skipped = [], 0
    for seed in SOLVE_SEEDS:
        iters, rejected, ndir, verdicts = _pair_run(seed, shrink, T)
        assert ndir == iters - rejected == verdicts.count(0), (seed, iters, rejected, ndir)
        counts.append(ndir)
        skipped += rejected
        print(f"seed {seed} shrink {shrink} T {T}: {iters} iterations, {rejected} rejected trials, {ndir} directions")
    print(f"shrink {shrink} T {T}: directions {' / '.join(map(str, counts))}")
    assert skipped > 0, "no run rejected a trial: the identity was not exercised"
    if T in NDIR_REF:
        assert tuple(counts) == NDIR_REF[T], counts
