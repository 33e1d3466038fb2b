"""tests/stop_ref.py (the numpy restatement of the stop rule, towr_gpu_alsolve_stop_batch_device, and the iterations that
carry it): every branch of the rule on hand-made states; the monoped's six starts, which the rule must leave alone; and
the two ANYmal cases of tests/feasible_cases.py driven by the CPU oracle through tests/tile_chol_ref.py under the
handle's ordering — the solvable trot ends ACCEPTABLE, the default one ends INFEASIBLE, and without the rule both are
still searching at that iteration. No GPU.

The ANYmal runs take tens of seconds each on one core (about 0.3 s per iteration of the oracle and the tiled reference);
a dense numpy solve of the 1090-column system is slower than the tiled reference, so the repository's own reference is
used. The run without the rule shares the evaluations and directions of the run with it through a memo on the operands'
bytes: until the rule fires both loops see the same operands."""
import copy
import functools

import numpy as np
import pytest

from oracle.oracle import Oracle
from tests import alsolve_ref as R
from tests import feasible_cases as FC
from tests import gn_ref as G
from tests import stop_ref as S
from tests import tile_chol_ref as TC
from tests.test_chol_ref import SOLVE_K, SOLVE_MU, SOLVE_SEEDS, _layout_handle
from tests.test_pgn_ref import SOLVE_PAR, _monoped

EX = S.params(**S.EXAMPLE)
PAR = R.params(max_inner=7)
NAN = np.float64(np.nan)
# the iterations of the repository's tiled reference from start 900: the feasible ANYmal ends ACCEPTABLE
# after 138, the default one INFEASIBLE after ANYMAL_REF["default"]; the tests are capped at twice these
ANYMAL_REF = dict(feasible=138, default=207)
ANYMAL_PAR = dict(feasible=SOLVE_PAR, default={**SOLVE_PAR, "max_inner": 50})
MONOPED_ITERS = (67, 9, 39, 32, 10, 12)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _st(phase=R.SEARCH, flags=1 | 2, inner=3, outer=2, pg=0.5, eta=0.1, omega=0.1, viol=0.4, run=0.0, last=0.0, rho=1e4, alpha=0.25):
    return dict(ISTATE=np.array([phase, flags, inner, outer], dtype=np.int32),
                SCAL=np.array([1.5, pg, eta, omega, viol, 0.75, run, last]), ALPHA=np.float64(alpha), RHO=np.float64(rho))


def _same(a, b):
    return (np.array_equal(a["ISTATE"], b["ISTATE"]) and np.array_equal(_bits(a["SCAL"]), _bits(b["SCAL"]))
            and _bits(a["ALPHA"]) == _bits(b["ALPHA"]) and _bits(a["RHO"]) == _bits(b["RHO"]))


def _run(st, sp=EX, par=PAR):
    out = copy.deepcopy(st)
    return S.stop(out, par, sp), out


# ---- the rule ------------------------------------------------------------------------------------------------------------
def test_run_length_counts_resets_and_fires_at_acc_iters():
    ok = dict(viol=1e-7, pg=1e-5, flags=0)
    did, out = _run(_st(run=3.0, **ok))
    assert did is None and out["SCAL"][6] == 4.0 and out["ISTATE"][0] == R.SEARCH and out["ALPHA"] == 0.25
    # exactly at the thresholds counts; just above either resets
    did, out = _run(_st(run=3.0, viol=1e-6, pg=1e-4, flags=0))
    assert did is None and out["SCAL"][6] == 4.0
    for kw in (dict(viol=np.nextafter(1e-6, 1), pg=1e-5), dict(viol=1e-7, pg=np.nextafter(1e-4, 1))):
        did, out = _run(_st(run=9.0, flags=0, **kw))
        assert did is None and out["SCAL"][6] == 0.0 and out["ISTATE"][0] == R.SEARCH
    # 13 -> 14 does not fire, 14 -> 15 does: phase, flags and ALPHA, nothing else
    did, out = _run(_st(run=13.0, **ok))
    assert did is None and out["SCAL"][6] == 14.0 and out["ISTATE"][0] == R.SEARCH
    before = _st(run=14.0, viol=1e-7, pg=1e-5, flags=1 | 2)
    did, out = _run(before)
    assert did == "acceptable" and list(out["ISTATE"]) == [S.ACCEPTABLE, 0, 3, 2] and out["ALPHA"] == 0.0
    want = before["SCAL"].copy()
    want[6] = 15.0
    assert np.array_equal(_bits(out["SCAL"]), _bits(want)) and out["RHO"] == before["RHO"]
    # acc_iters = 1 fires at the first acceptable base; acc_iters = 0 switches the rule off and SCAL[6] is not written
    did, out = _run(_st(**ok), sp=S.params(**{**S.EXAMPLE, "acc_iters": 1}))
    assert did == "acceptable"
    st = _st(run=99.0, **ok)
    did, out = _run(st, sp=S.params(**{**S.EXAMPLE, "acc_iters": 0}))
    assert did is None and _same(out, st)
    # the acceptable rule comes first: a state that would also be INFEASIBLE
    did, out = _run(_st(run=14.0, viol=1e-7, pg=1e-5, eta=1e-8, omega=1.0, last=1e-7, flags=1))
    assert did == "acceptable"


INFEASIBLE_STATE = dict(flags=1 | 2, pg=0.05, omega=0.1, viol=0.4, eta=0.1, last=0.4, rho=1e4)


def test_infeasible_rule_and_each_conjunct():
    did, out = _run(_st(**INFEASIBLE_STATE))
    assert did == "infeasible" and list(out["ISTATE"]) == [S.INFEASIBLE, 0, 3, 2] and out["ALPHA"] == 0.0
    assert np.array_equal(_bits(out["SCAL"]), _bits(_st(**INFEASIBLE_STATE)["SCAL"])) and out["RHO"] == 1e4
    # the outer update finds no SEARCH problem and writes nothing
    full = dict(out, LAM=np.zeros(2), LAMP=np.ones(2), HMETA=np.array([3, 1], dtype=np.int32))
    keep = copy.deepcopy(full)
    assert R.outer(full, PAR) is None and _same(full, keep) and np.array_equal(full["LAM"], keep["LAM"])
    # pg > omega but inner >= max_inner: the outer update is forced, so the rule looks too
    did, out = _run(_st(**{**INFEASIBLE_STATE, "pg": 0.5}, inner=7))
    assert did == "infeasible"
    # the predicate's three conjuncts false in turn: the rule does nothing at all
    for kw in (dict(flags=2), dict(pg=0.5), dict(viol=0.05, last=0.05)):
        st = _st(**{**INFEASIBLE_STATE, **kw})
        did, out = _run(st)
        assert did is None and _same(out, st), kw
    # the outer update is about to grow RHO, one of the other conditions fails: SCAL[7] = viol, nothing else
    for kw in (dict(last=0.0), dict(last=0.41), dict(rho=np.nextafter(1e4, 0))):
        st = _st(**{**INFEASIBLE_STATE, **kw})
        did, out = _run(st)
        want = copy.deepcopy(st)
        want["SCAL"][7] = 0.4
        assert did == "recorded" and _same(out, want), kw
    # viol >= keep * last with the one rounded product: at the product it stops, one ulp below it records
    last = 0.4037
    edge = np.float64(0.99) * np.float64(last)
    assert _run(_st(**{**INFEASIBLE_STATE, "viol": edge, "last": last}))[0] == "infeasible"
    assert _run(_st(**{**INFEASIBLE_STATE, "viol": np.nextafter(edge, 0), "last": last}))[0] == "recorded"
    # infeas_rho = inf switches the rule off: the violation is still recorded
    assert _run(_st(**INFEASIBLE_STATE), sp=S.params(**{**S.EXAMPLE, "infeas_rho": np.inf}))[0] == "recorded"
    assert _run(_st(**{**INFEASIBLE_STATE, "rho": np.inf}), sp=S.params(**{**S.EXAMPLE, "infeas_rho": np.inf}))[0] == "infeasible"


def test_the_predicate_is_the_outer_updates():
    """Over a grid of flags, pg, inner and viol (NaNs included): the rule records or stops exactly when the outer update,
    run on a copy without the rule, takes its RHO branch."""
    vals = (0.0, 0.05, 0.1, 0.5, NAN)
    for flags in (0, 1, 2, 3, 7):
        for inner in (3, 7, 8):
            for pg in vals:
                for viol in vals:
                    st = _st(flags=flags, inner=inner, pg=pg, viol=viol, last=0.0)
                    full = dict(copy.deepcopy(st), LAM=np.zeros(2), LAMP=np.ones(2), HMETA=np.zeros(2, dtype=np.int32))
                    did = S.stop(st, PAR, S.params(**{**S.EXAMPLE, "acc_iters": 0}))
                    assert (did == "recorded") == (R.outer(full, PAR) == "rho"), (flags, inner, pg, viol)


def test_nan_operands_never_stop():
    # the acceptable rule: a NaN viol or pg resets the run
    for kw in (dict(viol=NAN, pg=1e-5), dict(viol=1e-7, pg=NAN)):
        did, out = _run(_st(run=14.0, flags=0, **kw))
        assert did is None and out["SCAL"][6] == 0.0 and out["ISTATE"][0] == R.SEARCH, kw
    # the infeasible rule: a NaN viol is "not feasible" as in the outer update, fails viol >= keep and is recorded
    st = _st(**{**INFEASIBLE_STATE, "viol": NAN})
    did, out = _run(st)
    assert did == "recorded" and np.isnan(out["SCAL"][7]) and out["ISTATE"][0] == R.SEARCH
    # ... and as SCAL[7] it fails last > 0 the next time; a NaN RHO fails RHO >= infeas_rho; a NaN pg with inner below
    # max_inner fails the predicate (nothing written), at max_inner the rule looks and every other operand decides
    for kw, want in ((dict(last=NAN), "recorded"), (dict(rho=NAN), "recorded"), (dict(pg=NAN), None)):
        st = _st(**{**INFEASIBLE_STATE, **kw})
        did, out = _run(st)
        assert did == want and out["ISTATE"][0] == R.SEARCH, kw
        if want is None:
            assert _same(out, st)
    assert _run(_st(**{**INFEASIBLE_STATE, "pg": NAN}, inner=7))[0] == "infeasible"


@pytest.mark.parametrize("phase", [R.RESTART, 2, 3, 4, 5, 6, 7, -1, -2 ** 31])
def test_other_phases_are_untouched(phase):
    for kw in (dict(run=14.0, viol=1e-7, pg=1e-5), INFEASIBLE_STATE):
        st = _st(phase=phase, **kw)
        did, out = _run(st)
        assert did is None and _same(out, st)


def test_stop_batch_is_the_rule_per_problem():
    B = 5
    rows = [_st(run=14.0, viol=1e-7, pg=1e-5), _st(**INFEASIBLE_STATE), _st(phase=R.RESTART), _st(**{**INFEASIBLE_STATE, "last": 0.0}),
            _st(phase=9)]
    h = dict(ISTATE=np.concatenate([r["ISTATE"] for r in rows]), SCAL=np.stack([np.append(r["SCAL"], 7.0) for r in rows]),
             ALPHA=np.array([r["ALPHA"] for r in rows]), RHO=np.array([r["RHO"] for r in rows]))
    S.stop_batch(h, PAR, EX, B)
    assert list(h["ISTATE"][::4]) == [S.ACCEPTABLE, S.INFEASIBLE, R.RESTART, R.SEARCH, 9]
    assert list(h["ALPHA"]) == [0.0, 0.0, 0.25, 0.25, 0.25] and h["SCAL"][3, 7] == 0.4 and (h["SCAL"][:, 8] == 7.0).all()


# ---- the loops -----------------------------------------------------------------------------------------------------------
def _solve_monoped(seed, sp):
    o, P, x0, lo, up, evaluate = _monoped()
    info = _layout_handle("monoped_procedural").gn_factor_info()
    gn = dict(mu=SOLVE_MU, pos=info["pos"], first=info["first"])
    par = R.params(**SOLVE_PAR)
    x0 = x0 + 0.05 * np.random.default_rng(seed).standard_normal(o.n)
    st = R.new_state(o.n, o.m, par["mem"], x0, n_rsum=4 + o.desc.n_constraints, n_ssum=5 + o.desc.n_varsets)
    R.init(st, par, lo, up)
    trace = []
    for k in range(SOLVE_K):
        S.tile_iterate(st, par, sp, gn, P, evaluate, lo, up, 1, np.float64, trace)
        if st["ISTATE"][0] >= R.CONVERGED:
            break
    return st, trace


def test_monoped_still_converges_with_the_example_parameters():
    """Seeds 900 .. 905 through tile_chol_ref with the rule: all six end CONVERGED in 67 / 9 / 39 / 32 / 10 / 12
    iterations, the counts of the loop without it."""
    out = [_solve_monoped(seed, EX) for seed in SOLVE_SEEDS]
    got = [(int(st["ISTATE"][0]), len(trace)) for st, trace in out]
    print(got, [st["SCAL"][6:8].tolist() for st, _ in out])
    assert got == [(R.CONVERGED, k) for k in MONOPED_ITERS], got
    assert all(t[3] in (None, "recorded") for _, trace in out for t in trace)


def test_without_stop_the_wrappers_are_the_reference_iterations():
    """stop = None: tile_iterate leaves tile_chol_ref.iterate's bits in every array, iteration by iteration (monoped,
    seed 900, 30 iterations: a RESTART, accepted and rejected trials); with the rule switched off by its parameters
    likewise, except that SCAL[7] records the violation at a penalty growth."""
    o, P, x0, lo, up, evaluate = _monoped()
    info = _layout_handle("monoped_procedural").gn_factor_info()
    gn = dict(mu=SOLVE_MU, pos=info["pos"], first=info["first"])
    par = R.params(**SOLVE_PAR)
    x0 = x0 + 0.05 * np.random.default_rng(900).standard_normal(o.n)
    new = lambda: R.new_state(o.n, o.m, par["mem"], x0, n_rsum=4 + o.desc.n_constraints, n_ssum=5 + o.desc.n_varsets)
    a, b, c = new(), new(), new()
    for st in (a, b, c):
        R.init(st, par, lo, up)
    ta, tb = [], []
    for k in range(30):
        TC.iterate(a, par, gn, P, evaluate, lo, up, 1, np.float64, ta)
        S.tile_iterate(b, par, None, gn, P, evaluate, lo, up, 1, np.float64, tb)
        S.tile_iterate(c, par, S.params(), gn, P, evaluate, lo, up, 1, np.float64)
        assert ta[-1] == tb[-1][:3] and tb[-1][3] is None
        for key in a:
            if a[key].dtype.kind == "f":
                assert np.array_equal(_bits(a[key]), _bits(b[key])), (k, key)
                if key != "SCAL":
                    assert np.array_equal(_bits(a[key]), _bits(c[key])), (k, key)
            else:
                assert np.array_equal(a[key], b[key]) and np.array_equal(a[key], c[key]), (k, key)
        assert np.array_equal(_bits(a["SCAL"][:7]), _bits(c["SCAL"][:7]))
    assert {t[0] for t in ta} >= {1, 2, 3}


@functools.lru_cache(maxsize=None)
def _anymal():
    """The oracle of the feasible ANYmal trot, a layout-only handle for the bounds and the pattern, and the evaluation and
    the tiled direction with a memo on their operands' bytes (shared by the runs with and without the rule)."""
    desc = FC.formulation(True).to_desc()
    o = Oracle(desc)
    h = FC.problem(-1)
    gl, gu = h.constraint_bounds()
    rp, col = h.jac_csr()
    P = G.Pattern(rp, col, h.n)
    info = h.gn_factor_info()
    x0 = h.initial_x()
    has_l, has_u = gl > -R.SIDE_INF, gu < R.SIDE_INF
    memo_e, memo_d = {}, {}

    def evaluate(x, lam, rho):
        key = (x.tobytes(), lam.tobytes(), rho)
        if key not in memo_e:
            g = o.eval_g(x)
            r_, c_, v = o.eval_jac(x)
            assert np.array_equal(r_, P.row) and np.array_equal(c_, P.col)
            t = g + lam / rho
            r = t - R.clamp(t, gl, gu)
            lamp = rho * r
            phi = np.sum(0.5 * rho * r * r - 0.5 * lam * lam / rho)
            viol = max(0.0, np.max(np.where(has_l, gl - g, 0.0)), np.max(np.where(has_u, g - gu, 0.0)))
            memo_e[key] = (o.eval_f(x), o.eval_grad_f(x) + G.jtvec(P, v, lamp), lamp, viol, phi, v)
        return memo_e[key]

    def direct_for(st):
        def direct(vals, held):
            key = (vals.tobytes(), st["LAMP"].tobytes(), float(st["RHO"]), st["GRC"].tobytes(), held.tobytes())
            if key not in memo_d:
                d = TC.direction(P, vals, st["LAMP"], st["RHO"], st["GRC"], SOLVE_MU, info["pos"], info["first"], held, np.float64)
                memo_d[key] = (d["D"].astype(np.float64), TC.summary(d))
            return memo_d[key]
        return direct

    def forget():
        memo_e.clear()
        memo_d.clear()
    return desc, h, x0, evaluate, direct_for, forget


@pytest.mark.parametrize("kind", ["feasible", "default"])
def test_anymal_ends_acceptable_or_infeasible(kind):
    """Start 900 (x0 + 0.05 randn(900)) under the feasible bounds (SOLVE_PAR) and the default ones (max_inner = 50), with
    the example parameters, capped at twice the reference's own count (ANYMAL_REF). The loop without the rule,
    on the same operands, is still in RESTART or SEARCH when the rule fires."""
    desc, h, x0, evaluate, direct_for, forget = _anymal()
    lo, up = FC.bounds()[kind]
    par = R.params(**ANYMAL_PAR[kind])
    cap = 2 * ANYMAL_REF[kind]
    new = lambda: R.new_state(h.n, h.m, par["mem"], FC.start(x0, 900), n_rsum=4 + desc.n_constraints, n_ssum=5 + desc.n_varsets)
    st, plain = new(), new()
    R.init(st, par, lo, up)
    R.init(plain, par, lo, up)
    trace, grown = [], []
    for k in range(cap):
        recorded = st["SCAL"][7]
        S.iterate(st, par, EX, evaluate, lo, up, direct_for(st), 8, 1, np.float64, False, trace)
        S.iterate(plain, par, None, evaluate, lo, up, direct_for(plain), 8, 1, np.float64, False)
        forget()
        assert not np.isnan(st["SCAL"]).any() and not np.isnan(st["LSUM"]).any(), f"iteration {k}: NaN"
        if trace[-1][1] == "rho":
            grown.append(k + 1)
        if st["ISTATE"][0] >= R.CONVERGED:
            break
    iters, phase, viol = len(trace), int(st["ISTATE"][0]), float(st["SCAL"][4])
    print(f"{kind}: phase {phase} after {iters} iterations, viol {viol:.3e}, pg {st['SCAL'][1]:.3e}, rho {float(st['RHO']):g}, "
          f"rho updates at {grown}, recorded {recorded:.6e}; without the rule: phase {int(plain['ISTATE'][0])}")
    if kind == "feasible":
        assert phase == S.ACCEPTABLE and trace[-1][3] == "acceptable", (phase, iters)
        assert viol <= EX["acc_eta"] and st["SCAL"][6] == EX["acc_iters"]
    else:
        assert phase == S.INFEASIBLE and trace[-1][3] == "infeasible", (phase, iters)
        assert recorded > 0 and viol >= 0.99 * recorded and float(st["RHO"]) >= EX["infeas_rho"]
        assert viol == pytest.approx(0.4, abs=1e-3)           # the base cannot stand at z = 0
    assert int(plain["ISTATE"][0]) in (R.RESTART, R.SEARCH), "the loop without the rule stopped too"
    assert np.array_equal(_bits(plain["X"]), _bits(st["X"])), "until the rule fires both loops are at the same base"
