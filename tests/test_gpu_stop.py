"""The stop rule on the device (towr_gpu_alsolve_stop_batch_device) against tests/stop_ref.py, bit for bit: the rule is
IEEE comparisons and one product. And the solve with the rule in every iteration
(towr_gpu_alsolve_solve_ex_batch_device): against the public pieces in sequence, against the plain solve entry when no rule
is given, on the monoped's six starts (the rule never fires) and on a mixed ANYmal batch of two solvable problems and an
unsolvable one (tests/feasible_cases.py). Padded leading dimensions with NaN padding everywhere."""
import numpy as np
import pytest

from tests import alsolve_ref as R
from tests import compact_ref as CR
from tests import feasible_cases as FC
from tests import stop_ref as S
from tests.gpu_helpers import _dev, _nan, _same_bits, _vec
from tests.test_gpu_alsolve import ALL, FUSED_PAR, SOLVE_PAR, _assert_same, _start, _state
from tests.test_gpu_lbfgs import _problem
from tests.test_gpu_solve import _assert_rows, _row, _snapshot, _tiled
from tests.test_stop_ref import ANYMAL_REF
from towr2025_amd import _capi as capi, alsolve_params, alsolve_stop_params, gn_params

pytestmark = pytest.mark.gpu

MU = 1e-6
INT32_MIN = -2 ** 31
PERSISTENT = CR.PERSISTENT
NAN = float("nan")
MAX_INNER = 7
EX = S.params(**S.EXAMPLE)
# the branches of the rule; problem b of a batch takes KINDS[(b + offset) % len(KINDS)]
KINDS = ("count", "fire", "reset_viol", "reset_pg", "infeasible", "infeasible_forced", "no_flag", "pg_large", "feasible", "first",
         "progress", "rho_small", "nan_viol", "nan_pg", "nan_rho", "nan_last", "nan_run", "restart", "converged", "stalled", "maxed",
         "acceptable", "infeasible_word", "seven", "minus_one", "int32_min", "edge_keep", "edge_below")
WORDS = dict(restart=0, converged=2, stalled=3, maxed=4, acceptable=5, infeasible_word=6, seven=7, minus_one=-1, int32_min=INT32_MIN)


def _synthetic(B, seed, offset):
    """Host arrays ISTATE (B, 4), SCAL (B, 8), ALPHA, RHO (B) and the kinds: every branch of the rule, with the scalars
    that do not decide a branch drawn at random."""
    rng = np.random.default_rng(seed)
    IS = np.zeros((B, 4), dtype=np.int32)
    SC = np.zeros((B, 8))
    AL, RHO = rng.uniform(0.1, 1.0, B), np.full(B, 1e4)
    kinds = [KINDS[(b + offset) % len(KINDS)] for b in range(B)]
    for b, kind in enumerate(kinds):
        # a state on which the infeasible rule fires (and the acceptable rule resets), varied by the kind
        phase, flags, inner, outer = R.SEARCH, int(rng.choice([1, 3, 7])), int(rng.integers(1, MAX_INNER)), int(rng.integers(0, 5))
        viol = rng.uniform(0.3, 0.5)
        pg, eta, omega, run, last = rng.uniform(0.01, 0.09), 0.1, 0.1, float(rng.integers(0, 12)), viol * rng.uniform(0.8, 1.0)
        if kind in ("count", "fire"):
            viol, pg, run = rng.uniform(0, 1e-6), rng.uniform(0, 1e-4), (14.0 if kind == "fire" else run)
        elif kind == "reset_viol":
            viol, pg, flags = 2e-6, 1e-5, 0
        elif kind == "reset_pg":
            viol, pg, flags = 1e-7, 2e-4, 0
        elif kind == "infeasible_forced":
            pg, inner = 0.7, MAX_INNER + int(rng.integers(0, 2))
        elif kind == "no_flag":
            flags = int(rng.choice([0, 2, 6]))
        elif kind == "pg_large":
            pg = 0.7
        elif kind == "feasible":
            viol = last = 0.05
        elif kind == "first":
            last = 0.0
        elif kind == "progress":
            last = viol * 1.5
        elif kind == "rho_small":
            RHO[b] = np.nextafter(1e4, 0)
        elif kind == "nan_viol":
            viol = NAN
        elif kind == "nan_pg":
            pg = NAN
        elif kind == "nan_rho":
            RHO[b] = NAN
        elif kind == "nan_last":
            last = NAN
        elif kind == "nan_run":
            viol, pg, run = 1e-7, 1e-5, NAN
        elif kind in WORDS:
            phase = WORDS[kind]
            if b % 2:
                viol, pg, run = 1e-7, 1e-5, 14.0
        elif kind == "edge_keep":
            viol = np.float64(0.99) * np.float64(last)
        elif kind == "edge_below":
            viol = np.nextafter(np.float64(0.99) * np.float64(last), 0)
        IS[b] = (phase, flags, inner, outer)
        SC[b] = (rng.standard_normal(), pg, eta, omega, viol, rng.standard_normal(), run, last)
    return dict(ISTATE=IS, SCAL=SC, ALPHA=AL, RHO=RHO), kinds


EXPECT = dict(count=R.SEARCH, fire=S.ACCEPTABLE, reset_viol=R.SEARCH, reset_pg=R.SEARCH, infeasible=S.INFEASIBLE,
              infeasible_forced=S.INFEASIBLE, no_flag=R.SEARCH, pg_large=R.SEARCH, feasible=R.SEARCH, first=R.SEARCH,
              progress=R.SEARCH, rho_small=R.SEARCH, nan_viol=R.SEARCH, nan_pg=R.SEARCH, nan_rho=R.SEARCH, nan_last=R.SEARCH,
              nan_run=R.SEARCH, edge_keep=S.INFEASIBLE, edge_below=R.SEARCH, **WORDS)


@pytest.mark.parametrize("B", [1, 2, 64, 65, 257])
def test_kernel_equals_the_reference(B):
    """Seeded synthetic states (every branch of tests/test_stop_ref.py, NaN operands and the phase words 2..7, -1 and
    INT32_MIN among them; B = 257 is one thread into a second block): ISTATE, SCAL (NaN padding included) and ALPHA are
    tests/stop_ref.py's in every byte; RHO, X and every other array are unchanged; a problem the rule does not act on has
    no byte written. The same bits in reversed batch order on another stream."""
    import torch
    p, lo, up, _ = _problem("monoped_procedural")
    n, mem = p.n, 2
    par = alsolve_params(mem=mem, max_inner=MAX_INNER)
    sp = alsolve_stop_params(**S.EXAMPLE)
    seen = set()
    for rnd, offset in enumerate(range(0, len(KINDS), B) if B <= 2 else [B]):   # (the small batches walk every kind)
        h, kinds = _synthetic(B, 8100 + B + rnd, offset)
        rng = np.random.default_rng(8200 + B + rnd)
        host = dict(h, X=rng.standard_normal((B, n)), LAM=rng.standard_normal((B, p.m)), HMETA=rng.integers(0, 2, (B, 2)))
        st = _state(p, B, mem, host)
        before = _snapshot(st)
        want = S.stop_batch(dict(ISTATE=h["ISTATE"].reshape(-1).copy(), SCAL=h["SCAL"].copy(), ALPHA=h["ALPHA"].copy(),
                                 RHO=h["RHO"].copy()), {"max_inner": MAX_INNER}, EX, B)
        p.alsolve_stop(par, sp, st)
        torch.cuda.synchronize()
        after = _snapshot(st)
        for k in ALL:
            if k not in ("ISTATE", "SCAL", "ALPHA"):
                assert after[k] == before[k], f"B={B}: {k} changed"
        got_is = st.ISTATE.cpu().numpy()
        assert np.array_equal(got_is, want["ISTATE"]), f"B={B}: ISTATE"
        sc = st.SCAL.cpu().numpy()
        assert sc[:, :8].tobytes() == want["SCAL"].tobytes() and np.isnan(sc[:, 8:]).all(), f"B={B}: SCAL"
        assert st.ALPHA.cpu().numpy().tobytes() == want["ALPHA"].tobytes(), f"B={B}: ALPHA"
        for b, kind in enumerate(kinds):
            assert got_is[4 * b] == EXPECT[kind], (B, b, kind, got_is[4 * b:4 * b + 4])
            if kind in WORDS:                       # not acted on: not one byte written
                for k in ("ISTATE", "SCAL", "ALPHA"):
                    per = len(before[k]) // B
                    assert after[k][b * per:(b + 1) * per] == before[k][b * per:(b + 1) * per], (B, b, kind, k)
        seen |= set(kinds)
        # another batch position, another stream
        order = list(range(B))[::-1]
        st2 = _state(p, B, mem, {k: np.asarray(v)[order] for k, v in host.items()})
        s2 = torch.cuda.Stream(device=_dev())
        s2.wait_stream(torch.cuda.current_stream())
        p.alsolve_stop(par, sp, st2, stream=s2)
        torch.cuda.synchronize()
        idx = torch.tensor(order, device=_dev())
        assert torch.equal(st2.ISTATE.view(B, 4)[idx], st.ISTATE.view(B, 4)) and _same_bits(st2.SCAL[idx], st.SCAL) \
            and _same_bits(st2.ALPHA[idx], st.ALPHA), f"B={B}: reversed order on another stream"
    assert seen == set(KINDS), set(KINDS) - seen
    # the rule switched off by its parameters: only SCAL[7] of the problems about to grow RHO changes
    st = _state(p, B, mem, host)
    p.alsolve_stop(par, alsolve_stop_params(), st)
    off = S.stop_batch(dict(ISTATE=h["ISTATE"].reshape(-1).copy(), SCAL=h["SCAL"].copy(), ALPHA=h["ALPHA"].copy(),
                            RHO=h["RHO"].copy()), {"max_inner": MAX_INNER}, S.params(), B)
    assert np.array_equal(st.ISTATE.cpu().numpy(), h["ISTATE"].reshape(-1)) and st.SCAL.cpu().numpy()[:, :8].tobytes() == off["SCAL"].tobytes()
    assert st.ALPHA.cpu().numpy().tobytes() == h["ALPHA"].tobytes()


# ---- the iterations with the rule --------------------------------------------------------------------------------------
def _pieces_with_stop(p, par, sp, gn, st, DC, GSUM, W, Gs, Vs):
    """tests/test_gpu_gn_tiled._pieces_iteration with the stop call between the line search and the outer update."""
    import torch
    B, n = st.B, p.n
    p.eval_cost_batch_device(st.XC, st.FC, GRAD=st.GRC)
    p.eval_batch_device(st.XC, Gs, Vs)
    rho = st.RHO.cpu().numpy()
    for b in range(B):
        p.residual_batch_device(Gs[b:b + 1], st.RSUM[b:b + 1], LAM=st.LAM[b:b + 1], rho=float(rho[b]), LAMP=st.LAMP[b:b + 1])
    p.jac_tvec_batch_device(Vs, st.LAMP, st.GRC, accumulate=True)
    p.gn_tiled_direction_batch_device(gn, Vs, st.LAMP, st.GRC, DC, GSUM, W, rho=st.RHO, X=st.XC, RUN=st.ISTATE, run_stride=4)
    p.linesearch_batch_device(par, st)
    p.alsolve_stop(par, sp, st)
    p.auglag_outer_batch_device(par, st)
    flags = st.ISTATE.view(B, 4)[:, 1]
    acc = (flags & 1) != 0
    retry = ~acc & ((flags & 4) != 0)
    st.D[acc, :n] = DC[acc, :n]
    st.D[retry, :n] = st.GR[retry, :n]
    p.step_batch_device(st.X, st.D, st.SSUM, XP=st.XC, alpha=st.ALPHA)
    torch.cuda.synchronize()


# (params, stop parameters, SCAL[6] per problem behind alsolve_init): the acceptable rule fires in iteration 1 (problem
# 2), 3 (problem 1) and not at all (problem 0); the infeasible rule, with the outer update forced in every iteration
# and RHO = 10, 12.5, 15 growing tenfold, records twice and fires in iteration 3 (problem 0) or records once and fires
# in iteration 2 (problems 1 and 2)
FUSED_RULES = [
    (dict(FUSED_PAR), dict(acc_eta=np.inf, acc_omega=np.inf, acc_iters=4), (0.0, 1.0, 5.0), [R.SEARCH, S.ACCEPTABLE, S.ACCEPTABLE]),
    (dict(FUSED_PAR, max_inner=1, rho_grow=10.0), dict(infeas_keep=0.99, infeas_rho=120.0), (0.0, 0.0, 0.0), [S.INFEASIBLE] * 3),
]


@pytest.mark.parametrize("case", range(len(FUSED_RULES)))
def test_iterations_with_the_rule_equal_the_pieces(case):
    """monoped_procedural, B = 3, the tiled method: solve_ex with compact = 0, check_every = max_iters = 3 — three
    iterations of the tiled iterate entry with the rule — is bit-equal in every state array, DC and GSUM to the public calls
    in sequence with towr_gpu_alsolve_stop_batch_device between the line search and the outer update."""
    import torch
    pr, spd, run0, phases = FUSED_RULES[case]
    name, B = "monoped_procedural", 3
    p, lo, up, _ = _problem(name)
    n, mem = p.n, pr["mem"]
    par, sp, gn = alsolve_params(**pr), alsolve_stop_params(**spd), gn_params(mu=1e-2)
    h0 = _start(p, lo, up, B, mem, 7400)

    def fresh():
        st = _state(p, B, mem, h0)
        p.alsolve_init(par, st)
        st.RHO.copy_(_vec(10.0 * (1.0 + 0.25 * np.arange(B))))
        st.SCAL[:, 6] = _vec(np.array(run0))
        return (st,) + _tiled(p, B, 2)

    Gs, Vs = _nan(B, p.m + 1), _nan(B, p.nnz + 5)
    ref, DCr, GSr, Wr = fresh()
    seen = []
    for k in range(3):
        _pieces_with_stop(p, par, sp, gn, ref, DCr, GSr, Wr, Gs, Vs)
        seen.append(ref.ISTATE.view(B, 4)[:, 0].tolist())
    print(f"case {case}: phases per iteration {seen}, SCAL[6..7] {ref.SCAL[:, 6:8].tolist()}, RHO {ref.RHO.tolist()}")
    assert seen[-1][1:] == phases[1:] and (seen[-1][0] == phases[0] or seen[-1][0] + phases[0] == 1), seen     # (0: RESTART or SEARCH)
    phases = seen[-1]
    st, DC, GS, W = fresh()
    rep = p.alsolve_solve(par, st, method=capi.SOLVE_GN_TILED, gn=gn, DC=DC, GSUM=GS, W=W, max_iters=3, check_every=3,
                          compact=False, stop=sp)
    torch.cuda.synchronize()
    assert (rep["rounds"], rep["iters_run"], rep["problem_iters"]) == (1, 3, 9)
    assert rep["n_acceptable"] == phases.count(S.ACCEPTABLE) and rep["n_infeasible"] == phases.count(S.INFEASIBLE)
    assert rep["n_phase"][5] == rep["n_acceptable"] + rep["n_infeasible"] and sum(rep["n_phase"]) == B
    _assert_same(st, ref, f"case {case}")
    assert _same_bits(DC, DCr) and _same_bits(GS, GSr), f"case {case}: DC / GSUM"
    # without the rule the same three iterations leave every problem searching
    st, DC, GS, W = fresh()
    p.alsolve_gn_tiled_iterate(par, st, gn, DC, GS, W, iters=3)
    assert all(ph in (R.RESTART, R.SEARCH) for ph in st.ISTATE.view(B, 4)[:, 0].tolist())


@pytest.mark.parametrize("compact", [False, True])
def test_solve_ex_without_stop_is_the_plain_solve(compact):
    """Sweep seed 196 (n = 78), B = 7, the tiled method, rows 0 and 3 pre-frozen, max_iters = 6 in rounds of 2:
    towr_gpu_alsolve_solve_ex_batch_device with stop == NULL leaves every byte of the state, DC, GSUM and the report as
    towr_gpu_alsolve_solve_batch_device does."""
    import torch
    p, lo, up, _ = _problem("sweep_seed_196")
    B, n, mem = 7, p.n, SOLVE_PAR["mem"]
    assert n == 78
    par, gn = alsolve_params(**SOLVE_PAR), gn_params(mu=MU)
    h0 = _start(p, lo, up, B, mem, 19600)

    def solve(ex):
        st = _state(p, B, mem, h0)
        p.alsolve_init(par, st)
        st.RHO.copy_(_vec(10.0 * (1.0 + 0.25 * np.arange(B))))
        st.ISTATE.view(B, 4)[0, 0] = R.CONVERGED
        st.ISTATE.view(B, 4)[3, 0] = 7
        DC, GS, W = _tiled(p, B, 2)
        rep = p.alsolve_solve(par, st, method=capi.SOLVE_GN_TILED, gn=gn, DC=DC, GSUM=GS, W=W, max_iters=6, check_every=2,
                              compact=compact, ex=ex)
        torch.cuda.synchronize()
        return _snapshot(st, DC=DC, GSUM=GS), rep

    a, ra = solve(False)
    b, rb = solve(True)
    assert ra == rb and ra["iters_run"] == 6 and "n_acceptable" not in ra
    for k in a:
        assert a[k] == b[k], f"compact {compact}: {k}"


def test_monoped_short_solve_is_untouched_by_the_rule():
    """tests/test_gpu_solve.py's short solve (B = 6, seeds 900..905, wrows = 4, check_every = 4, max_iters = 100) with the
    example parameters: all six end CONVERGED, no problem ends ACCEPTABLE or INFEASIBLE, and the persistent arrays are
    bit-equal to the run without the rule — SCAL in its columns 0..5: columns 6 and 7 are the rule's own memory."""
    import torch
    name, B = "monoped_procedural", 6
    p, lo, up, _ = _problem(name)
    n, mem = p.n, SOLVE_PAR["mem"]
    par, gn, sp = alsolve_params(**SOLVE_PAR), gn_params(mu=MU), alsolve_stop_params(**S.EXAMPLE)
    x0 = p.initial_x()
    h0 = dict(X=np.stack([x0 + 0.05 * np.random.default_rng(900 + b).standard_normal(n) for b in range(B)]), LAM=np.zeros((B, p.m)))

    def solve(stop):
        st = _state(p, B, mem, h0)
        DC, GS, W = _tiled(p, B, 4)
        p.alsolve_init(par, st)
        rep = p.alsolve_solve(par, st, method=capi.SOLVE_GN_TILED, gn=gn, DC=DC, GSUM=GS, W=W, max_iters=100, check_every=4,
                              compact=True, stop=stop)
        torch.cuda.synchronize()
        return st, rep

    s1, r1 = solve(sp)
    s0, r0 = solve(None)
    print(f"with the rule {r1}; without {r0}; SCAL[6..7] {s1.SCAL[:, 6:8].tolist()}")
    assert r1["n_phase"] == [0, 0, B, 0, 0, 0] and (r1["n_acceptable"], r1["n_infeasible"]) == (0, 0)
    assert {k: r1[k] for k in r0} == r0
    _assert_rows(s1, s0, range(B), [k for k in PERSISTENT if k != "SCAL"], "with the rule against without")
    assert _same_bits(s1.SCAL[:, :6], s0.SCAL[:, :6]) and torch.isnan(s1.SCAL[:, 8:]).all()
    assert (s0.SCAL[:, 6:8] == 0).all(), "the plain solve wrote the rule's slots"


def test_anymal_mixed_batch():
    """The feasible ANYmal trot's handle, B = 3, the tiled method, compact = 1, max_inner = 50, check_every = 8, the example
    parameters: rows 0 and 2 carry the feasible variable bounds, row 1 the default formulation's, all three start from
    x0 + 0.05 randn(900). max_iters = 2 x the CPU reference's larger count (tests/test_stop_ref.ANYMAL_REF).
    Rows 0 and 2 end ACCEPTABLE or CONVERGED with viol <= 1e-6 and identical bits (the same operands at two batch
    positions: compaction did not disturb them); row 1 ends INFEASIBLE with RHO >= 1e4; the report counts them; the frozen
    rows were compacted out (problem_iters < B x iters_run); no NaN in the scalars, and where a row's last line search
    accepted a base it did not raise M0 (LSUM[2] <= LSUM[3]; the solve is one call, so only the last is seen).
    Iterates are not compared with the CPU reference: a rounding difference may steer a decision. On MI355X:
    iters_run 344 of the 414 allowed, problem_iters 896, rows 0 and 2 ACCEPTABLE with viol 9.0e-12 at RHO = 1000, row 1
    INFEASIBLE with viol 0.4 at RHO = 1e4 (1.6 s)."""
    import torch
    p = FC.problem(0)
    B, n, m, mem = 3, p.n, p.m, SOLVE_PAR["mem"]
    par = alsolve_params(**{**SOLVE_PAR, "max_inner": 50})
    gn, sp = gn_params(mu=MU), alsolve_stop_params(**S.EXAMPLE)
    xl, xu = FC.bounds_rows(("feasible", "default", "feasible"))
    x = FC.start(p.initial_x(), 900)
    st = _state(p, B, mem, dict(X=np.stack([x] * B), LAM=np.zeros((B, m))))
    XL, XU = _nan(B, n + 1), _nan(B, n + 1)
    XL[:, :n], XU[:, :n] = _vec(xl), _vec(xu)
    DC, GS, W = _tiled(p, B, 2)
    p.alsolve_init(par, st, XL=XL, XU=XU)
    cap = 2 * max(ANYMAL_REF.values())
    rep = p.alsolve_solve(par, st, method=capi.SOLVE_GN_TILED, gn=gn, DC=DC, GSUM=GS, W=W, max_iters=cap, check_every=8,
                          compact=True, XL=XL, XU=XU, stop=sp)
    torch.cuda.synchronize()
    ph = st.ISTATE.view(B, 4)[:, 0].tolist()
    sc, ls = st.SCAL.cpu().numpy()[:, :8], st.LSUM.cpu().numpy()[:, :8]
    rho = st.RHO.cpu().numpy()
    print(f"report {rep}; phases {ph}; inner / outer {st.ISTATE.view(B, 4)[:, 2:].tolist()}; viol {sc[:, 4].tolist()}; "
          f"pg {sc[:, 1].tolist()}; RHO {rho.tolist()}; SCAL[6..7] {sc[:, 6:].tolist()}")
    assert not np.isnan(sc).any() and np.isfinite(st.X.cpu().numpy()[:, :n]).all() and not np.isnan(ls[:, 1:]).any()
    assert ph[0] in (S.ACCEPTABLE, R.CONVERGED) and ph[2] == ph[0] and sc[0, 4] <= 1e-6 and sc[2, 4] <= 1e-6
    assert ph[1] == S.INFEASIBLE and rho[1] >= 1e4 and sc[1, 7] > 0 and sc[1, 4] >= 0.99 * sc[1, 7]
    for k in PERSISTENT:
        assert _row(st, k, 0) == _row(st, k, 2), f"rows 0 and 2: {k}"
    assert rep["n_infeasible"] == 1 and rep["n_acceptable"] == ph.count(S.ACCEPTABLE) and rep["n_phase"][2] == ph.count(R.CONVERGED)
    assert rep["n_phase"][5] == rep["n_acceptable"] + 1 and sum(rep["n_phase"]) == B
    assert rep["iters_run"] < cap and rep["problem_iters"] < B * rep["iters_run"], rep
    acc = ls[:, 0] == 2
    assert (ls[acc, 2] <= ls[acc, 3]).all(), "an accepted base raised M0"
    assert torch.isnan(XL[:, n:]).all() and _same_bits(XL[0], XL[2]) and not _same_bits(XL[0], XL[1])
