"""tests/probe_ref.py (the numpy restatement of the probe stage, towr_gpu_alsolve_probe_batch_device, and the iterations
that carry it): every branch of the stage on hand-made states; the identity that defines the feature — on the monoped's
six starts the probed loop visits, bit for bit, the accepted bases of the loop without probes, in fewer iterations; and
the case that motivates it — the feasible ANYmal trot from start 901 ends CONVERGED or ACCEPTABLE with shrink = 0.5 and
four probes, while the loop as it stands (SOLVE_PAR, no probes) is still searching at that iteration. No GPU.

The ANYmal test takes on the order of a minute on one core (about 0.3 s per iteration of the oracle and the tiled
reference, two loops); evaluations and directions are shared through tests/test_stop_ref.py's memo."""
import copy
import functools

import numpy as np
import pytest

from tests import alsolve_ref as R
from tests import feasible_cases as FC
from tests import probe_ref as PR
from tests import stop_ref as S
from tests import tile_chol_ref as TC
from tests.test_chol_ref import SOLVE_MU, SOLVE_SEEDS, _layout_handle
from tests.test_pgn_ref import SOLVE_PAR, _monoped
from tests.test_stop_ref import _anymal

NAN = np.float64(np.nan)
EX = S.params(**S.EXAMPLE)
# the probed iterations of the repository's tiled reference on the feasible ANYmal from starts 900, 901 and 902 (shrink = 0.5,
# T = 4, the example stop parameters): all three end ACCEPTABLE, after 266, 310 and 261 rejected lengths skipped (a dense
# float64 Cholesky in the tiled reference's place gave 115, 175 and 129). The tests are capped at twice these
ANYMAL_PROBED_REF = {900: 134, 901: 185, 902: 143}
N = 4


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- the stage on a quadratic ---------------------------------------------------------------------------------------------
# merit = 0.5 |x - 1|^2 from X = 0 with D = k GR, GR = -1: the trial at length a stands at u = a k in every column,
# gs = -4 u, and the Armijo test passes iff u <= 2 (1 - c1)
def _quad(x, lam, rho):
    return np.float64(0.5 * np.sum((x - 1.0) ** 2))


def _st(k=1.0, alpha=1.0, phase=R.SEARCH, inner=3, m0=2.0):
    gr = -np.ones(N)
    return dict(X=np.zeros(N), GR=gr, D=k * gr, XC=np.full(N, 7.0), LAM=np.zeros(2), RHO=np.float64(10.0), ALPHA=np.float64(alpha),
                SCAL=np.array([m0, 0.5, 0.1, 0.1, 0.4, 0.75, 0.0, 0.0]), ISTATE=np.array([phase, 3, inner, 2], dtype=np.int32))


def _par(**kw):
    return R.params(**{**dict(shrink=0.5, c1=1e-4, alpha_min=1e-10), **kw})


LO, UP = np.full(N, -1e20), np.full(N, 1e20)


def _run(st, T, par=None, merit=_quad, lo=LO, up=UP):
    out = copy.deepcopy(st)
    return PR.probe(out, par or _par(), T, merit, lo, up), out


def test_first_length_passes():
    ps, out = _run(_st(k=1.0), 4)
    assert list(ps[:4]) == [1, 0, 1, 1.0] and ps[4] == 0.0 and ps[5] == -4.0 and list(ps[6:]) == [0, 0]
    assert out["ALPHA"] == 1.0 and np.array_equal(out["XC"], np.ones(N)) and list(out["ISTATE"]) == [R.SEARCH, 3, 3, 2]


def test_a_later_length_passes():
    # u = 8, 4, 2 fail (2 > 2 (1 - c1)), u = 1 passes
    ps, out = _run(_st(k=8.0), 4)
    assert list(ps[:4]) == [1, 3, 4, 0.125] and ps[4] == 0.0 and ps[5] == -4.0
    assert out["ALPHA"] == 0.125 and np.array_equal(out["XC"], np.ones(N)) and out["ISTATE"][2] == 6
    # the ladder is the line search's: one rounded product per rejection
    ps, out = _run(_st(k=8.0 / 0.3, alpha=0.3), 8, _par(shrink=0.7))
    t = int(ps[1])
    b = np.float64(0.3)
    for _ in range(t):
        b = b * np.float64(0.7)
    assert ps[0] == 1 and _bits(out["ALPHA"]) == _bits(b) and out["ISTATE"][2] == 3 + t and ps[2] == t + 1


def test_none_passes_and_the_next_length_is_untested():
    for T in (1, 2, 3):
        ps, out = _run(_st(k=8.0), T)
        assert list(ps[:4]) == [2, T, T, 0.5 ** T] and np.isnan(ps[4]) and ps[5] == -4.0 * 8.0 * 0.5 ** T
        assert out["ALPHA"] == 0.5 ** T and np.array_equal(out["XC"], np.full(N, 8.0 * 0.5 ** T)) and out["ISTATE"][2] == 3 + T
    # exactly at alpha_min the length is valid
    ps, out = _run(_st(k=8.0), 2, _par(alpha_min=0.25))
    assert list(ps[:4]) == [2, 2, 2, 0.25]


def test_none_passes_and_the_last_valid_length_stays():
    # a = 1, 0.5 are valid, 0.25 is not: v = 2, both fail, t* = 1
    ps, out = _run(_st(k=8.0), 4, _par(alpha_min=0.3))
    assert list(ps[:4]) == [3, 1, 2, 0.5] and ps[4] == _quad(np.full(N, 4.0), None, None) and ps[5] == -16.0
    assert out["ALPHA"] == 0.5 and np.array_equal(out["XC"], np.full(N, 4.0)) and out["ISTATE"][2] == 4
    # the line search behind it then leaves SEARCH or resets the history at this base: a = 0.25 < alpha_min
    # v = 1 (only t = 0 counts, although ALPHA itself is below alpha_min): t* = 0, nothing moves but XC
    ps, out = _run(_st(k=80.0, alpha=0.2), 4, _par(alpha_min=0.3))
    assert list(ps[:4]) == [3, 0, 1, 0.2] and out["ALPHA"] == 0.2 and out["ISTATE"][2] == 3
    # T = 1 with an invalid a_1
    ps, out = _run(_st(k=8.0), 1, _par(alpha_min=0.75))
    assert list(ps[:4]) == [3, 0, 1, 1.0]


def test_an_ascent_direction_fails_whatever_the_merit():
    low = lambda x, lam, rho: np.float64(-100.0)
    ps, out = _run(_st(k=-1.0), 2, merit=low)
    assert ps[0] == 2 and ps[5] == 1.0 and out["ALPHA"] == 0.25      # gs = +4, +2 failed; gs of the untested 0.25 is +1
    ps, out = _run(_st(k=1.0), 2, merit=low)
    assert list(ps[:2]) == [1, 0] and ps[4] == -100.0
    # gs = 0 passes when the merit does (D = 0)
    st = _st()
    st["D"] = np.zeros(N)
    ps, out = _run(st, 2)
    assert list(ps[:2]) == [1, 0] and ps[5] == 0.0 and np.array_equal(out["XC"], st["X"])


def test_nan_operands_fail_every_test():
    ps, out = _run(_st(k=1.0), 3, merit=lambda x, lam, rho: NAN)
    assert list(ps[:4]) == [2, 3, 3, 0.125] and np.isnan(ps[4])
    ps, out = _run(_st(k=1.0, m0=NAN), 3)
    assert list(ps[:4]) == [2, 3, 3, 0.125]
    # a NaN ALPHA: t = 0 counts and fails, a_1 = NaN ends the run: the NaN stays for the line search's own branch
    ps, out = _run(_st(k=1.0, alpha=NAN), 3)
    assert list(ps[:3]) == [3, 0, 1] and np.isnan(ps[3]) and np.isnan(ps[4]) and np.isnan(ps[5])
    assert np.isnan(out["ALPHA"]) and np.isnan(out["XC"]).all() and out["ISTATE"][2] == 3
    # a NaN column of D poisons gs, not the other columns of XC
    st = _st(k=1.0)
    st["D"][2] = NAN
    ps, out = _run(st, 2)
    assert ps[0] == 2 and np.isnan(ps[5]) and np.isnan(out["XC"][2]) and not np.isnan(out["XC"][[0, 1, 3]]).any()


@pytest.mark.parametrize("phase", [R.RESTART, 2, 3, 4, 5, 6, 7, -1, -2 ** 31])
def test_other_phases_are_untouched(phase):
    st = _st(phase=phase)
    ps, out = _run(st, 4)
    assert ps is None
    for k in st:
        assert np.array_equal(np.asarray(st[k]), np.asarray(out[k])), k


def test_one_and_eight_probes_and_the_bounds():
    # T = 8: u = 300 a fails down to a = 2^-8 (u = 1.17 passes): t* = 8 would be untested, t = 7 gives u = 2.34
    ps, out = _run(_st(k=300.0), 8)
    assert list(ps[:4]) == [2, 8, 8, 2.0 ** -8] and out["ISTATE"][2] == 11
    ps, out = _run(_st(k=200.0), 8)
    assert list(ps[:4]) == [1, 7, 8, 2.0 ** -7]                       # u = 1.5625
    ps, out = _run(_st(k=1.0), 1)
    assert list(ps[:4]) == [1, 0, 1, 1.0]
    with pytest.raises(AssertionError):
        _run(_st(), 9)
    # the candidate is projected: column 1 stops at its bound and gs counts the projected step
    up = UP.copy()
    up[1] = 0.25
    ps, out = _run(_st(k=1.0), 2, up=up)
    assert ps[0] == 1 and np.array_equal(out["XC"], [1.0, 0.25, 1.0, 1.0]) and ps[5] == -3.25
    # a side beyond 1e19 does not count
    up[1] = 2e19
    assert np.array_equal(_run(_st(k=1.0), 2, up=up)[1]["XC"], np.ones(N))


def test_device_tree_is_a_sum():
    rng = np.random.default_rng(5)
    for n in (0, 1, 63, 64, 255, 256, 257, 1090):
        t = rng.standard_normal(n)
        assert abs(PR.device_tree(t) - np.sum(t)) <= 1e-12 * max(1.0, np.sum(np.abs(t)))
    assert PR.device_tree(np.arange(1, 601, dtype=np.float64)) == 600 * 601 / 2   # integers: exact in any order
    assert np.isnan(PR.device_tree([1.0, NAN]))


# ---- the identity: the probed loop visits the sequential loop's bases --------------------------------------------------------
BASE_KEYS = ("X", "GR", "LAM", "RHO", "HS", "HY", "HMETA", "D")


@functools.lru_cache(maxsize=None)
def _monoped_memo():
    """tests/test_pgn_ref.py's monoped with a memo on the operands' bytes for the evaluation and the tiled direction: the
    probed loops evaluate only points the sequential loop has seen."""
    o, P, x0, lo, up, evaluate = _monoped()
    info = _layout_handle("monoped_procedural").gn_factor_info()
    memo_e, memo_d = {}, {}

    def ev(x, lam, rho):
        key = (x.tobytes(), lam.tobytes(), rho)
        if key not in memo_e:
            memo_e[key] = evaluate(x, lam, rho)
        return memo_e[key]

    def direct_for(st):
        def direct(vals, held):
            key = (vals.tobytes(), st["LAMP"].tobytes(), float(st["RHO"]), st["GRC"].tobytes(), held.tobytes())
            if key not in memo_d:
                d = TC.direction(P, vals, st["LAMP"], st["RHO"], st["GRC"], SOLVE_MU, info["pos"], info["first"], held, np.float64)
                memo_d[key] = (d["D"].astype(np.float64), TC.summary(d))
            return memo_d[key]
        return direct
    return o, x0, lo, up, ev, direct_for


def _snapshot(st):
    s = {k: np.array(st[k], copy=True) for k in BASE_KEYS}
    s["SCAL"] = st["SCAL"][:6].copy()
    s["ISTATE"] = st["ISTATE"][[0, 2, 3]].copy()
    return s


def _monoped_run(seed, shrink, T, cap):
    """The loop from x0 + 0.05 randn(seed) until it is frozen or `cap` iterations: (iterations, the state after every
    iteration in which a base was accepted, the sum of PSUM[1], frozen)."""
    o, x0, lo, up, ev, direct_for = _monoped_memo()
    par = R.params(**{**SOLVE_PAR, "shrink": shrink})
    st = R.new_state(o.n, o.m, par["mem"], x0 + 0.05 * np.random.default_rng(seed).standard_normal(o.n),
                     n_rsum=4 + o.desc.n_constraints, n_ssum=5 + o.desc.n_varsets)
    R.init(st, par, lo, up)
    bases, trace, psums = [], [], []
    while len(trace) < cap and st["ISTATE"][0] < R.CONVERGED:
        PR.iterate(st, par, None, T, ev, lo, up, direct_for(st), 8, 1, None, trace, psums)
        if trace[-1][0] in (1, 2):
            bases.append(_snapshot(st))
    skipped = sum(int(ps[1]) for ps in psums if ps is not None)
    return len(trace), bases, skipped, bool(st["ISTATE"][0] >= R.CONVERGED)


SEQ_CAP = 400


@pytest.mark.parametrize("shrink", [0.1, 0.5])
def test_probed_loop_visits_the_sequential_bases(shrink):
    """Seeds 900 .. 905, tiled reference, no stop rule, T in {1, 2, 4}: the state after every accepted base of the probed
    loop (X, GR, LAM, RHO, SCAL[0..5], the history, HMETA, D, {phase, inner, outer}) is bit-equal to the state after the
    same accepted base of alsolve_ref's sequential loop, and sequential iterations = probed iterations + sum of PSUM[1]."""
    fewer = 0
    for seed in SOLVE_SEEDS:
        seq_iters, seq_bases, zero, seq_done = _monoped_run(seed, shrink, None, SEQ_CAP)
        assert zero == 0 and seq_done, f"seed {seed}: the sequential loop is not frozen after {SEQ_CAP} iterations"
        for T in (1, 2, 4):
            iters, bases, skipped, done = _monoped_run(seed, shrink, T, SEQ_CAP)
            tag = f"seed {seed} shrink {shrink} T {T}"
            assert done and len(bases) == len(seq_bases), f"{tag}: {len(bases)} bases, the sequential loop has {len(seq_bases)}"
            for i, (a, b) in enumerate(zip(bases, seq_bases)):
                for k in a:
                    same = np.array_equal(a[k], b[k]) if a[k].dtype.kind == "i" else np.array_equal(_bits(a[k]), _bits(b[k]))
                    assert same, f"{tag}: base {i}: {k}"
            assert seq_iters == iters + skipped, f"{tag}: {seq_iters} sequential, {iters} probed + {skipped} skipped"
            assert iters <= seq_iters
            fewer += seq_iters - iters
            print(f"{tag}: {seq_iters} sequential iterations, {iters} probed, {len(bases)} bases")
    assert fewer > 0, "no run rejected a trial: the identity was not exercised"


# ---- the case that motivates it ---------------------------------------------------------------------------------------------
def test_anymal_901_is_solved_with_probes_and_a_finer_ladder():
    """The feasible ANYmal from start 901: shrink = 0.5 and T = 4 probes with the example stop parameters end CONVERGED or
    ACCEPTABLE within twice ANYMAL_PROBED_REF[901] probed iterations; the loop as it stands (SOLVE_PAR, shrink = 0.1, no probes,
    the same stop parameters) is still in SEARCH or RESTART after as many iterations."""
    desc, h, x0, evaluate, direct_for, forget = _anymal()
    lo, up = FC.bounds()["feasible"]
    gl, gu = h.constraint_bounds()
    from oracle.oracle import Oracle
    merit = PR.al_merit(Oracle(desc), gl, gu)
    par = R.params(**{**SOLVE_PAR, "shrink": 0.5})
    plain_par = R.params(**SOLVE_PAR)
    new = lambda p: R.new_state(h.n, h.m, p["mem"], FC.start(x0, 901), n_rsum=4 + desc.n_constraints, n_ssum=5 + desc.n_varsets)
    st, plain = new(par), new(plain_par)
    R.init(st, par, lo, up)
    R.init(plain, plain_par, lo, up)
    trace, psums = [], []
    for k in range(2 * ANYMAL_PROBED_REF[901]):
        PR.iterate(st, par, EX, 4, evaluate, lo, up, direct_for(st), 8, 1, merit, trace, psums)
        S.iterate(plain, plain_par, EX, evaluate, lo, up, direct_for(plain), 8, 1, np.float64, False)
        forget()
        assert not np.isnan(st["SCAL"]).any() and not np.isnan(st["LSUM"]).any(), f"iteration {k}: NaN"
        if st["ISTATE"][0] >= R.CONVERGED:
            break
    iters, phase = len(trace), int(st["ISTATE"][0])
    skipped = sum(int(ps[1]) for ps in psums if ps is not None)
    print(f"probed: phase {phase} after {iters} iterations ({skipped} rejected lengths skipped), viol {st['SCAL'][4]:.3e}, "
          f"pg {st['SCAL'][1]:.3e}, rho {float(st['RHO']):g}; as it stands: phase {int(plain['ISTATE'][0])}, viol {plain['SCAL'][4]:.3e}")
    assert phase in (R.CONVERGED, S.ACCEPTABLE), (phase, iters)
    assert st["SCAL"][4] <= EX["acc_eta"]
    assert int(plain["ISTATE"][0]) in (R.RESTART, R.SEARCH), "the loop as it stands stopped too"
