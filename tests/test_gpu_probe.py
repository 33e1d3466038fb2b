"""The probe stage on the device (towr_gpu_alsolve_probe_batch_device) against tests/probe_ref.py, and the solve with the
stage in front of every iteration (towr_gpu_alsolve_solve_probe_batch_device): against the public pieces in sequence,
against the _ex entry when no probe is given, on the monoped's six starts (the bases of the loop without probes, in fewer
iterations) and on the feasible ANYmal from starts 900, 901 and 902. Padded leading dimensions with NaN padding.

The stage's reference is exact: the merit of every candidate is the device's own (the f-only objective call, the g-only
evaluation and the residual call, added on the host in one float64 addition), gs is summed on the line search's tree
(probe_ref.device_tree), and everything else is one rounded operation or a comparison. A NaN is compared as a NaN: which
payload an operation hands on is not part of the contract."""
import numpy as np
import pytest

from tests import alsolve_ref as R
from tests import compact_ref as CR
from tests import feasible_cases as FC
from tests import probe_ref as PR
from tests import stop_ref as S
from tests.gpu_helpers import _dev, _nan, _np_bits, _padded, _same_bits, _vec
from tests.test_gpu_alsolve import ALL, FUSED_PAR, SOLVE_PAR, _assert_same, _start, _state
from tests.test_gpu_lbfgs import _problem
from tests.test_gpu_solve import _snapshot, _tiled
from tests.test_probe_ref import ANYMAL_PROBED_REF
from towr2025_amd import _capi as capi, alsolve_params, alsolve_stop_params, gn_params

pytestmark = pytest.mark.gpu

MU = 1e-6
NAN = float("nan")
INT32_MIN = -2 ** 31
AMIN = 0.2
STAGE_PAR = dict(mem=2, c1=0.25, shrink=0.5, alpha0=1.0, alpha_min=AMIN)
WORDS = dict(restart=0, converged=2, stalled=3, maxed=4, acceptable=5, infeasible_word=6, seven=7, minus_one=-1, int32_min=INT32_MIN)
# the branches of the stage; problem b of a batch takes KINDS[(b + offset) % len(KINDS)]
KINDS = ("first", "later_1", "later_2", "later_last", "none_next", "none_last", "none_last_0", "ascent", "nan_lam", "nan_alpha",
         "nan_m0") + tuple(WORDS)


def _eq(a, b):
    """Bit-equal, a NaN equal to a NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(((_np_bits(a) == _np_bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def _device_merits(p, X, LAM, RHO):
    """f + phi of the rows of X (host, (R, n)) with the rows of LAM and RHO, as the stage evaluates them: the f-only
    objective call, the g-only evaluation, the residual call per distinct rho; one float64 addition on the host."""
    import torch
    rows, n, m = X.shape[0], p.n, p.m
    Xd, Fd, Gd = _padded(X, n + 1), _nan(1, rows)[0], _nan(rows, m + 1)
    p.eval_cost_batch_device(Xd, Fd)
    p.eval_batch_device(Xd, Gd, None, want_g=True, want_jac=False)
    phi = np.full(rows, NAN)
    for rho in np.unique(RHO):
        idx = np.flatnonzero(RHO == rho)
        Gs, Ls = Gd[torch.from_numpy(idx).to(_dev())].contiguous(), _padded(LAM[idx], m + 1)
        SUM, LP = _nan(len(idx), 4 + p.desc.n_constraints), _nan(len(idx), m + 1)
        p.residual_batch_device(Gs, SUM, LAM=Ls, rho=float(rho), LAMP=LP)
        phi[idx] = SUM.cpu().numpy()[:, 3]
    torch.cuda.synchronize()
    with np.errstate(invalid="ignore", over="ignore"):
        return Fd.cpu().numpy() + phi


def _stage_operands(p, lo, up, B, T, seed, offset, tighten):
    """Host arrays of a batch whose problem b takes branch KINDS[(b + offset) % len(KINDS)], its per-problem bounds
    (lo, up when `tighten` is off) and the device merits of every candidate of the ladder, by (b, the candidate's bytes)."""
    n, m = p.n, p.m
    rng = np.random.default_rng(seed)
    kinds = [KINDS[(b + offset) % len(KINDS)] for b in range(B)]
    X = np.clip(p.initial_x() + 0.05 * rng.standard_normal((B, n)), lo, up)
    GR = rng.standard_normal((B, n))
    D = 0.05 * GR * rng.uniform(0.5, 2.0, (B, n))
    LO, UP = np.tile(lo, (B, 1)), np.tile(up, (B, 1))
    if tighten:                                  # a third of the columns stop 0.02 above X: the projection is at work
        cut = rng.random((B, n)) < 0.33
        UP = np.where(cut, np.minimum(UP, X + 0.02), UP)
    h = dict(X=X, GR=GR, D=D, XC=rng.standard_normal((B, n)), LAM=0.1 * rng.standard_normal((B, m)),
             RHO=np.where(np.arange(B) % 2 == 1, 12.5, 10.0), ALPHA=np.full(B, AMIN * 2.0 ** T * 1.5),
             SCAL=np.tile([0.0, 0.3, 0.1, 0.1, 0.2, 0.9, 0.0, 0.0], (B, 1)),
             ISTATE=np.array([(R.SEARCH, 5, 3 + b % 5, b % 4) for b in range(B)], dtype=np.int32))
    for b, kind in enumerate(kinds):
        if kind in WORDS:
            h["ISTATE"][b, 0] = WORDS[kind]
        elif kind == "ascent":
            D[b] = -D[b]
        elif kind == "nan_lam":
            h["LAM"][b, b % m] = NAN
        elif kind == "nan_alpha":
            h["ALPHA"][b] = NAN
        elif kind == "none_last":
            h["ALPHA"][b] = AMIN * 3.0           # a = 0.6, 0.3 are valid, 0.15 is not
        elif kind == "none_last_0":
            h["ALPHA"][b] = AMIN * 1.5           # a_1 = 0.15 is not valid
    # the ladder's candidates and their device merits
    cand, owner = [], []
    with np.errstate(invalid="ignore"):
        for b in range(B):
            a = np.float64(h["ALPHA"][b])
            for t in range(T):
                cand.append(R.clamp(X[b] - a * D[b], LO[b], UP[b]))
                owner.append((b, t))
                a = a * np.float64(STAGE_PAR["shrink"])
    cand = np.array(cand)
    ob = np.array([b for b, _ in owner])
    mc = _device_merits(p, cand, h["LAM"][ob], h["RHO"][ob])
    merits = {(b, cand[i].tobytes()): mc[i] for i, (b, t) in enumerate(owner)}
    # M0: what decides the branch. hk = MC - c1 gs of trial k (the test passes where hk <= M0, up to rounding)
    c1 = STAGE_PAR["c1"]
    for b, kind in enumerate(kinds):
        hk = [mc[b * T + t] - c1 * np.sum(GR[b] * (cand[b * T + t] - X[b])) for t in range(T)]
        if kind in ("first", "ascent", "nan_lam", "nan_alpha") or kind in WORDS:
            m0 = 1e30
        elif kind.startswith("none"):
            m0 = -1e30
        elif kind == "nan_m0":
            m0 = NAN
        else:                                    # later_k: between trial k and the smallest before it, when that is above
            k = min(T - 1, {"later_1": 1, "later_2": 2, "later_last": T - 1}[kind])
            before = min(hk[:k]) if k else np.inf
            m0 = 0.5 * (hk[k] + before) if hk[k] < before and np.isfinite(before) else hk[k] + 1.0
        h["SCAL"][b, 0] = m0
    return h, kinds, LO, UP, merits


@pytest.mark.parametrize("B,T", [(1, 4), (2, 4), (64, 4), (65, 4), (257, 4), (5, 1), (5, 8)])
def test_stage_equals_the_reference(B, T):
    """Seeded states of every branch (a first or a later length passes; none passes with and without a valid a_T; an
    ascent direction; a NaN merit, ALPHA and M0; the phase words 0, 2..7, -1 and INT32_MIN) on the monoped's handle, with
    the handle's bounds or per-problem rows that cut into the step (B = 2, 65): ALPHA, XC, ISTATE and PSUM are
    tests/probe_ref.py's in every byte, NaN padding kept; every other array is unchanged; a problem that is not in SEARCH
    has no byte written but PSUM[0] = 0. The same bits in reversed row order on another stream."""
    import torch
    p, lo, up, _ = _problem("monoped_procedural")
    n, m, mem = p.n, p.m, STAGE_PAR["mem"]
    par = alsolve_params(**STAGE_PAR)
    pd = {k: getattr(par, k) for k in R.DEFAULTS}
    per_rows = B in (2, 65)
    seen = set()
    rounds = range(0, len(KINDS), B) if B <= 5 else [B]
    for rnd, offset in enumerate(rounds):
        h, kinds, LO, UP, merits = _stage_operands(p, lo, up, B, T, 9100 + 10 * B + rnd, offset, per_rows)
        XL = _padded(LO, n + 2) if per_rows else None
        XU = _padded(UP, n + 2) if per_rows else None
        st = _state(p, B, mem, h)
        PSUM = _nan(B, 8 + 3)
        before = _snapshot(st)
        p.alsolve_probe(par, st, T, PSUM, XL=XL, XU=XU)
        torch.cuda.synchronize()
        after = _snapshot(st)
        for k in ALL:
            if k not in ("ALPHA", "XC", "ISTATE"):
                assert after[k] == before[k], f"B={B}: {k} changed"
        if per_rows:
            assert _eq(XL.cpu().numpy()[:, :n], LO) and _eq(XU.cpu().numpy()[:, :n], UP)
        want = dict(X=h["X"], D=h["D"], GR=h["GR"], LAM=h["LAM"], XC=h["XC"].copy(), ALPHA=h["ALPHA"].copy(), RHO=h["RHO"],
                    SCAL=h["SCAL"], ISTATE=h["ISTATE"].reshape(-1).copy(), PSUM=np.full((B, 8), NAN))
        PR.probe_batch(want, pd, T, lambda b, x, lam, rho: merits[(b, x.tobytes())], LO, UP, n, m)
        got_ps, got_xc = PSUM.cpu().numpy(), st.XC.cpu().numpy()
        assert np.array_equal(st.ISTATE.cpu().numpy(), want["ISTATE"]), f"B={B}: ISTATE"
        assert _eq(st.ALPHA.cpu().numpy(), want["ALPHA"]), f"B={B}: ALPHA"
        assert np.isnan(got_ps[:, 8:]).all() and np.isnan(got_xc[:, n:]).all(), f"B={B}: padding written"
        for b, kind in enumerate(kinds):
            tag = f"B={B} T={T} problem {b} ({kind}): got {got_ps[b, :8]} want {want['PSUM'][b]}"
            assert _eq(got_ps[b, :8], want["PSUM"][b]), tag
            assert _eq(got_xc[b, :n], want["XC"][b]), tag
            if kind in WORDS:
                assert got_ps[b, 0] == 0.0 and np.isnan(got_ps[b, 1:]).all(), tag
                for k in ("ALPHA", "XC", "ISTATE"):
                    per = len(before[k]) // B
                    assert after[k][b * per:(b + 1) * per] == before[k][b * per:(b + 1) * per], tag
            else:
                code, ts = int(got_ps[b, 0]), int(got_ps[b, 1])
                seen.add((code, min(ts, 1)))
                # (T = 1: a_1 = 0.3 of "none_last" is the valid untested length, code 2)
                assert code == {"first": 1, "none_next": 2, "none_last": 3 if T > 1 else 2, "none_last_0": 3, "ascent": 2, "nan_lam": 2,
                                "nan_alpha": 3, "nan_m0": 2}.get(kind, code), tag
                if kind in ("first", "none_last_0", "nan_alpha"):
                    assert ts == 0, tag
                if kind == "none_last" and T > 1:
                    assert (ts, got_ps[b, 2]) == (1, 2.0), tag
        # another batch position, another stream
        order = list(range(B))[::-1]
        st2 = _state(p, B, mem, {k: np.asarray(v)[order] for k, v in h.items()})
        PS2 = _nan(B, 8 + 3)
        s2 = torch.cuda.Stream(device=_dev())
        s2.wait_stream(torch.cuda.current_stream())
        p.alsolve_probe(par, st2, T, PS2, XL=None if XL is None else XL.flip(0).contiguous(),
                        XU=None if XU is None else XU.flip(0).contiguous(), stream=s2)
        torch.cuda.synchronize()
        idx = torch.tensor(order, device=_dev())
        assert torch.equal(st2.ISTATE.view(B, 4)[idx], st.ISTATE.view(B, 4)) and _same_bits(st2.ALPHA[idx], st.ALPHA) \
            and _same_bits(st2.XC[idx], st.XC) and _same_bits(PS2[idx], PSUM), f"B={B}: reversed order on another stream"
    if T == 4:
        assert len(rounds) * B < len(KINDS) or seen >= {(1, 0), (1, 1), (2, 1), (3, 0), (3, 1)}, seen
    print(f"B={B} T={T}: (code, t* > 0) seen {sorted(seen)}")


def test_iterations_with_probes_equal_the_pieces():
    """monoped_procedural, B = 3, the tiled method, T = 2: the new solve entry with compact = 0 and check_every =
    max_iters = 3 — three probed iterations — is bit-equal in every state array, DC, GSUM and PSUM to the public pieces in
    sequence: towr_gpu_alsolve_probe_batch_device, then the tiled iterate entry with iters = 1."""
    import torch
    name, B, T = "monoped_procedural", 3, 2
    p, lo, up, _ = _problem(name)
    mem = FUSED_PAR["mem"]
    par, gn = alsolve_params(**{**FUSED_PAR, "shrink": 0.5}), gn_params(mu=1e-2)
    h0 = _start(p, lo, up, B, mem, 7400)

    def fresh():
        st = _state(p, B, mem, h0)
        p.alsolve_init(par, st)
        st.RHO.copy_(_vec(10.0 * (1.0 + 0.25 * np.arange(B))))
        return (st,) + _tiled(p, B, 2) + (_nan(B, 8 + 1),)

    ref, DCr, GSr, Wr, PSr = fresh()
    codes = []
    for k in range(3):
        p.alsolve_probe(par, ref, T, PSr)
        p.alsolve_gn_tiled_iterate(par, ref, gn, DCr, GSr, Wr, iters=1)
        torch.cuda.synchronize()
        codes.append((PSr[:, 0].tolist(), ref.LSUM[:, 0].tolist()))
    print(f"(PSUM[0], LSUM[0]) per iteration: {codes}")
    assert codes[0][0] == [0.0] * B and any(c != 0.0 for k in (1, 2) for c in codes[k][0]), "iteration 1 is the RESTART; no later one probed"
    st, DC, GS, W, PS = fresh()
    rep = p.alsolve_solve(par, st, method=capi.SOLVE_GN_TILED, gn=gn, DC=DC, GSUM=GS, W=W, max_iters=3, check_every=3,
                          compact=False, probes=T, PSUM=PS)
    torch.cuda.synchronize()
    assert (rep["rounds"], rep["iters_run"], rep["problem_iters"]) == (1, 3, 9)
    _assert_same(st, ref, "probed iterations")
    assert _same_bits(DC, DCr) and _same_bits(GS, GSr) and _same_bits(PS, PSr), "DC / GSUM / PSUM"


@pytest.mark.parametrize("compact", [False, True])
def test_solve_without_probe_is_solve_ex(compact):
    """Sweep seed 196 (n = 78), B = 7, the tiled method, rows 0 and 3 pre-frozen, max_iters = 6 in rounds of 2: the new
    entry with probe == NULL leaves every byte of the state, DC, GSUM and the report as
    towr_gpu_alsolve_solve_ex_batch_device does."""
    import torch
    p, lo, up, _ = _problem("sweep_seed_196")
    B, mem = 7, SOLVE_PAR["mem"]
    par, gn = alsolve_params(**SOLVE_PAR), gn_params(mu=MU)
    h0 = _start(p, lo, up, B, mem, 19600)

    def solve(**kw):
        st = _state(p, B, mem, h0)
        p.alsolve_init(par, st)
        st.RHO.copy_(_vec(10.0 * (1.0 + 0.25 * np.arange(B))))
        st.ISTATE.view(B, 4)[0, 0] = R.CONVERGED
        st.ISTATE.view(B, 4)[3, 0] = 7
        DC, GS, W = _tiled(p, B, 2)
        rep = p.alsolve_solve(par, st, method=capi.SOLVE_GN_TILED, gn=gn, DC=DC, GSUM=GS, W=W, max_iters=6, check_every=2,
                              compact=compact, **kw)
        torch.cuda.synchronize()
        return _snapshot(st, DC=DC, GSUM=GS), rep

    a, ra = solve(ex=True)
    b, rb = solve(probes=0)
    assert ra == rb and ra["iters_run"] == 6
    for k in a:
        assert a[k] == b[k], f"compact {compact}: {k}"


def test_compacted_probed_solve_with_terrains_and_per_problem_rows():
    """Sweep seed 196 (n = 78), B = 7, the tiled method, T = 2, shrink = 0.5, batch terrains set, per-problem GL / GU / XL /
    XU rows with NaN padding, distinct RHO, rows 0 and 3 pre-frozen, max_iters = 6 in rounds of 2 with compact = 1: the
    stage sees the permuted terrains and bounds rows of the compacted batch. Every row's persistent arrays are bit-equal to
    six rounds of the public pieces (the stage, then the tiled iterate entry with iters = 1) on the whole batch in the
    caller's order, the rows still active at the end in every state array, DC and GSUM; the bounds are back in place."""
    import torch
    from tests.gpu_helpers import _terrains
    from tests.shape_sweep import make
    from tests.test_gpu_solve import _assert_rows, _bytes
    from towr2025_amd import TowrGpuProblem
    f = make(196)[0]
    f.params_.enable_stance_tracking = False
    p = TowrGpuProblem(f.to_desc(), device=0, data=f.var_bounds_data())
    B, T, n, m, mem = 7, 2, p.n, p.m, SOLVE_PAR["mem"]
    lo, up = p.variable_bounds()
    gl, gu = p.constraint_bounds()
    p.set_batch_terrain(_terrains("sweep_seed_196", B, np.random.default_rng(196)))
    par, gn = alsolve_params(**{**SOLVE_PAR, "shrink": 0.5}), gn_params(mu=MU)
    h0 = _start(p, lo, up, B, mem, 19600)
    shift = 1e-3 * np.arange(B)[:, None]

    def fresh():
        st = _state(p, B, mem, h0)
        bounds = dict(GL=_padded(gl[None, :] + shift, m + 1), GU=_padded(gu[None, :] + shift, m + 1),
                      XL=_padded(lo[None, :] - shift, n + 1), XU=_padded(up[None, :] + shift, n + 1))
        p.alsolve_init(par, st, XL=bounds["XL"], XU=bounds["XU"])
        st.RHO.copy_(_vec(10.0 * (1.0 + 0.25 * np.arange(B))))
        st.ISTATE.view(B, 4)[0, 0] = R.CONVERGED
        st.ISTATE.view(B, 4)[3, 0] = 7
        return (st,) + _tiled(p, B, 2) + (_nan(B, 8), bounds)

    ref, DCr, GSr, Wr, PSr, br = fresh()
    probed = 0
    for k in range(6):
        p.alsolve_probe(par, ref, T, PSr, **br)
        probed += int((PSr[:, 0] != 0).sum())
        p.alsolve_gn_tiled_iterate(par, ref, gn, DCr, GSr, Wr, iters=1, **br)
    st, DC, GS, W, PS, bd = fresh()
    bounds0 = {k: _bytes(t) for k, t in bd.items()}
    rep = p.alsolve_solve(par, st, method=capi.SOLVE_GN_TILED, gn=gn, DC=DC, GSUM=GS, W=W, max_iters=6, check_every=2,
                          compact=True, probes=T, PSUM=PS, **bd)
    torch.cuda.synchronize()
    print(f"{rep}; problems probed over the six iterations {probed}")
    assert probed > 0 and rep["iters_run"] == 6 and rep["problem_iters"] < 6 * B
    ph = st.ISTATE.view(B, 4)[:, 0].tolist()
    _assert_rows(st, ref, range(B), CR.PERSISTENT, "persistent arrays")
    _assert_rows(st, ref, [b for b in range(B) if ph[b] in (R.RESTART, R.SEARCH)], ALL, "active rows",
                 extra=(("DC", DC, DCr), ("GSUM", GS, GSr)))
    for k, t in bd.items():
        assert _bytes(t) == bounds0[k], f"{k} is not back in the caller's order (or its padding was written)"


# what the identity covers (tests/test_probe_ref.py): the base, the multipliers, the history and the counters
IDENTITY = ("X", "GR", "LAM", "RHO", "HS", "HY", "HMETA", "D")


@pytest.mark.parametrize("method", [capi.SOLVE_GN_TILED, capi.SOLVE_LBFGS])
def test_monoped_probed_solve_ends_at_the_same_bases(method):
    """monoped_procedural, B = 6 (seeds 900 .. 905), shrink = 0.5, no stop rule, compact = 1, until every problem is frozen,
    with T = 4 probes and without: X, GR, LAM, RHO, SCAL[0..5], the history, HMETA, D and ISTATE {phase, inner, outer} are
    bit-equal, and the probed solve ran strictly fewer iterations. The cap holds every run: once inner has reached max_inner
    the next accepted base ends the outer iteration, and before it come at most the 54 halvings from alpha0 down to
    alpha_min, a reset of the history and 54 more (then the problem is STALLED); there are max_outer outer iterations."""
    import torch
    name, B, T = "monoped_procedural", 6, 4
    p, lo, up, _ = _problem(name)
    n, mem = p.n, SOLVE_PAR["mem"]
    pr = {**SOLVE_PAR, "shrink": 0.5}
    par, gn = alsolve_params(**pr), gn_params(mu=MU)
    cap = par.max_outer * (par.max_inner + 2 * 54)
    x0 = p.initial_x()
    h0 = dict(X=np.stack([x0 + 0.05 * np.random.default_rng(900 + b).standard_normal(n) for b in range(B)]), LAM=np.zeros((B, p.m)))

    def solve(probes):
        st = _state(p, B, mem, h0)
        DC, GS, W = _tiled(p, B, 4)
        p.alsolve_init(par, st)
        kw = dict(probes=probes, PSUM=_nan(B, 8)) if probes else {}
        rep = p.alsolve_solve(par, st, method=method, gn=gn, DC=DC, GSUM=GS, W=W, max_iters=cap, check_every=4, compact=True, **kw)
        torch.cuda.synchronize()
        return st, rep

    s1, r1 = solve(T)
    s0, r0 = solve(None)
    print(f"method {method}: with probes {r1}; without {r0}")
    assert r0["n_phase"][0] + r0["n_phase"][1] == 0 and r1["n_phase"] == r0["n_phase"], "a problem is not frozen"
    for k in IDENTITY:
        assert _same_bits(getattr(s1, k), getattr(s0, k)), k
    assert _same_bits(s1.SCAL[:, :6], s0.SCAL[:, :6]), "SCAL[0..5]"
    assert torch.equal(s1.ISTATE.view(B, 4)[:, [0, 2, 3]], s0.ISTATE.view(B, 4)[:, [0, 2, 3]]), "phase, inner, outer"
    assert r1["iters_run"] < r0["iters_run"], (r1["iters_run"], r0["iters_run"])


def test_anymal_three_starts_are_solved():
    """The feasible ANYmal trot, B = 3 (starts 900, 901, 902), the tiled method, compact = 1, shrink = 0.5, T = 4, the example
    stop parameters, check_every = 8, max_iters = 2 x the CPU reference's largest count (tests/test_probe_ref.py
    ANYMAL_PROBED_REF): all three end CONVERGED or ACCEPTABLE with viol <= 1e-6. Iterates are not compared with the CPU
    reference: a rounding difference may steer a decision."""
    import torch
    p = FC.problem(0)
    B, n, m, mem = 3, p.n, p.m, SOLVE_PAR["mem"]
    par = alsolve_params(**{**SOLVE_PAR, "shrink": 0.5})
    gn, sp = gn_params(mu=MU), alsolve_stop_params(**S.EXAMPLE)
    x0 = p.initial_x()
    st = _state(p, B, mem, dict(X=np.stack([FC.start(x0, s) for s in (900, 901, 902)]), LAM=np.zeros((B, m))))
    DC, GS, W = _tiled(p, B, 2)
    PS = _nan(B, 8 + 1)
    p.alsolve_init(par, st)
    cap = 2 * max(ANYMAL_PROBED_REF.values())
    rep = p.alsolve_solve(par, st, method=capi.SOLVE_GN_TILED, gn=gn, DC=DC, GSUM=GS, W=W, max_iters=cap, check_every=8,
                          compact=True, stop=sp, probes=4, PSUM=PS)
    torch.cuda.synchronize()
    ph = st.ISTATE.view(B, 4)[:, 0].tolist()
    sc = st.SCAL.cpu().numpy()[:, :8]
    print(f"report {rep}; phases {ph}; inner / outer {st.ISTATE.view(B, 4)[:, 2:].tolist()}; viol {sc[:, 4].tolist()}; "
          f"pg {sc[:, 1].tolist()}; RHO {st.RHO.tolist()}")
    assert not np.isnan(sc).any() and np.isfinite(st.X.cpu().numpy()[:, :n]).all()
    assert all(x in (R.CONVERGED, S.ACCEPTABLE) for x in ph), ph
    assert (sc[:, 4] <= 1e-6).all(), sc[:, 4]
    assert rep["iters_run"] <= cap and rep["n_phase"][2] + rep["n_acceptable"] == B
