"""Batches whose problems carry terrains that tilt the friction basis (tests/terrain_cases.py: mixed ids, every parameter
and friction_coeff drawn per problem), on the device. Every other per-problem terrain of the g / J tests is Flat or
Stairs with mu = 0.5, on which every problem has the same normalised basis and mu: the constraint sets that read only
those (ForceConstraintDiscretized, Force, TorqueConstraintDiscretized, Torque) could read any problem's terrain there.
tests/test_terrain_cases.py holds the conditions on the inputs (teeth for every problem, the pieces reached, the host
emulation); here the launches: device batches of 5 and 67 (past kSplitBatch: the gait path's side stream, composer
groups of 4 with a remainder), g only / Jacobian only, the host-pointer batch, the chunked products entry, the solve
drivers that permute or move terrain rows, tie points of every terrain predicate, and the Gap class.

The reference of row b is always the oracle built with desc.terrain = terrains[b]. Outputs are NaN-filled, ldv is rounded
up to 16 and the padding is asserted untouched. No tolerance of its own: tests/parity.py's gate, bit equality, NaN
padding. DESIGN.md 7e has the cases and the figures."""
import functools

import numpy as np
import pytest

from tests import terrain_cases as TC
from tests.gpu_helpers import _nan, _np_bits, _padded, _same_bits, _vec
from towr2025_amd import TowrGpuProblem, _capi as capi, alsolve_params, gn_params

pytestmark = pytest.mark.gpu

MU = 1e-6
TIE_CASES = (154, 16, 191, 74, TC.GAP)
IDS = [f"{c}-B{B}" for c, B in TC.CASE_BATCHES]


def _ldv(nnz):
    return (nnz + 15) // 16 * 16


@functools.lru_cache(maxsize=None)
def _handle(case):
    return TowrGpuProblem(TC.get(case).desc, device=0)


def _c_terrains(terrains):
    return [t.to_c() for t in terrains]


def _evaluate(p, terrains, X, want_g=True, want_jac=True):
    """set_batch_terrain + one eval_batch_device into NaN-filled G (B, m) and V (B, ldv): the host copies, the padding
    checked, an output that was not wanted checked untouched."""
    import torch
    B = len(terrains)
    p.set_batch_terrain(_c_terrains(terrains))
    Gd, Vd = _nan(B, p.m), _nan(B, _ldv(p.nnz))
    p.eval_batch_device(_vec(np.array(X)), Gd, Vd, want_g=want_g, want_jac=want_jac)
    torch.cuda.synchronize()
    G, V = Gd.cpu().numpy(), Vd.cpu().numpy()
    assert np.isnan(V[:, p.nnz:]).all(), "write past nnz"
    assert want_g or np.isnan(G).all(), "G written though it was not wanted"
    assert want_jac or np.isnan(V).all(), "V written though it was not wanted"
    return G, np.ascontiguousarray(V[:, :p.nnz])


@functools.lru_cache(maxsize=None)
def _device_batch(case, B):
    """(G, V) of the case's batch of B on the device, computed once and left unchanged."""
    terrains, X = TC.batch(case, B)
    G, V = _evaluate(_handle(case), terrains, X)
    G.setflags(write=False)
    V.setflags(write=False)
    return G, V


def _assert_bits(a, b, what):
    diff = np.argwhere(_np_bits(a) != _np_bits(b))
    assert diff.size == 0, f"{what}: {len(diff)} entries differ, first at {tuple(diff[0])}: {a[tuple(diff[0])]!r} != {b[tuple(diff[0])]!r}"


@pytest.mark.parametrize("case,B", TC.CASE_BATCHES, ids=IDS)
def test_device_batch_matches_each_problems_oracle(case, B):
    """eval_batch_device at B = 5 and B = 67: row b against the oracle of terrains[b] under the gate. The Gap case
    (B = 5, gap_terrains: the parameters and mu vary): the values on the frozen pattern, and pattern_outside counts equal
    to the oracle's count of reference entries outside it, as tests/test_gpu_parity.py test_gap_batch."""
    import torch
    cs, p = TC.get(case), _handle(case)
    assert (p.n, p.m, p.nnz) == (cs.n, cs.m, cs.nnz)
    r, c = p.jac_structure()
    assert np.array_equal(r, cs.r) and np.array_equal(c, cs.c)
    terrains, X = TC.batch(case, B)
    G, V = _device_batch(case, B)
    assert np.isfinite(G).all() and np.isfinite(V).all()
    worst, refs = 0.0, []
    for b, t in enumerate(terrains):
        refs.append(TC.reference(case, t, X[b]))
        st = TC.gate(case, refs[b], G[b], V[b], f"{case} B = {B} problem {b} ({TC.NAMES[t.id]}, mu = {t.friction_coeff:.3f})")
        worst = max(worst, st["worst"])
    print(f"{case} B = {B}: n={p.n} m={p.m} nnz={p.nnz} worst |err| / tolerance {worst:.3g}")
    if cs.gap:
        p.set_batch_terrain(_c_terrains(terrains))
        counts = np.full(B, -1, dtype=np.int32)
        p.pattern_outside_batch(_vec(np.array(X)), counts)
        torch.cuda.synchronize()
        assert counts.tolist() == [ref[2] for ref in refs], f"{case}: pattern_outside {counts.tolist()}"


@pytest.mark.parametrize("B", TC.BATCHES)
@pytest.mark.parametrize("case", TC.GAIT_SEEDS)
def test_g_only_and_jacobian_only(case, B):
    """The gait-optimising cases with want_jac = 0 and with want_g = 0 (the record kernels skip what is not wanted; the
    terrain staging is shared): rows bit-equal to the full batch, the unwanted output untouched."""
    terrains, X = TC.batch(case, B)
    G, V = _device_batch(case, B)
    Gg, _ = _evaluate(_handle(case), terrains, X, want_jac=False)
    _assert_bits(Gg, G, f"{case} B = {B} g only")
    _, Vj = _evaluate(_handle(case), terrains, X, want_g=False)
    _assert_bits(Vj, V, f"{case} B = {B} Jacobian only")


@pytest.mark.parametrize("case", [154, 191])
def test_host_batch_equals_device_batch(case):
    """towr_gpu_eval_batch (host pointers, chunked through the pinned staging, the terrains offset per chunk) on a
    tile-path case (154) and a record-path case (191) at B = 67: bit-equal to the device batch."""
    B = TC.BATCHES[1]
    terrains, X = TC.batch(case, B)
    G, V = _device_batch(case, B)
    p = _handle(case)
    p.set_batch_terrain(_c_terrains(terrains))
    Gh, Vh = np.full((B, p.m), np.nan), np.full((B, p.nnz), np.nan)
    p.eval_batch(np.array(X), Gh, Vh)
    _assert_bits(Gh, G, f"{case} host batch G")
    _assert_bits(Vh, V, f"{case} host batch V")


@pytest.mark.parametrize("case", TC.SEEDS)
def test_products_chunks_offset_the_terrains(case):
    """towr_gpu_eval_products_batch_device at B = 5 with the products chunk set to 2 (chunks of 2, 2 and 1 problems, each
    with its terrain offset): G bit-equal to the device batch's, and J p / J^T lam of the values it keeps in handle
    scratch bit-equal to the separate product calls on the device batch's V, for the first chunk and the last, shorter
    one alike."""
    import torch
    B = TC.BATCHES[0]
    terrains, X = TC.batch(case, B)
    G, V = _device_batch(case, B)
    p = _handle(case)
    rng = np.random.default_rng(5100 + case)
    Pd, LAMd = _padded(rng.standard_normal((B, p.n)), p.n + 7), _padded(rng.standard_normal((B, p.m)), p.m + 9)
    Vd, Xd = _padded(np.array(V), _ldv(p.nnz)), _padded(np.array(X), p.n + 1)
    Y0, Z0 = _nan(B, p.m + 5), _nan(B, p.n + 3)
    p.jac_vec_batch_device(Vd, Pd, Y0)
    p.jac_tvec_batch_device(Vd, LAMd, Z0)
    p.set_batch_terrain(_c_terrains(terrains))
    try:
        p.set_products_chunk(2)
        Gk, Yk, Zk = _nan(B, p.m + 2), _nan(B, p.m + 5), _nan(B, p.n + 3)
        p.eval_products_batch_device(Xd, G=Gk, LAM=LAMd, Z=Zk, P=Pd, Y=Yk)
        torch.cuda.synchronize()
    finally:
        p.set_products_chunk(0)
    Gh = Gk.cpu().numpy()
    assert np.isnan(Gh[:, p.m:]).all()
    _assert_bits(Gh[:, :p.m], G, f"{case} products G")
    assert torch.isfinite(Y0[:, :p.m]).all() and torch.isfinite(Z0[:, :p.n]).all()
    for b in range(B):
        assert _same_bits(Yk[b], Y0[b]), f"{case} products: J p of problem {b} (chunk {b // 2})"
        assert _same_bits(Zk[b], Z0[b]), f"{case} products: J^T lam of problem {b} (chunk {b // 2})"


# ---- the drivers that move terrain rows ------------------------------------------------------------------------------
def _solver_case(N):
    """The smallest case's handle with variable bounds, N tilted terrains (all seven ids at N = 7) set on it, and the
    starts: x0 of each problem's terrain + 0.05 N(0, 1), LAM = 0.1 N(0, 1)."""
    from tests.shape_sweep import make
    f = make(TC.SMALLEST)[0]
    f.params_.enable_stance_tracking = False
    p = TowrGpuProblem(f.to_desc(), device=0, data=f.var_bounds_data())
    rng = np.random.default_rng(15400 + N)
    terrains = TC.tilted_terrains(N, rng)
    X = np.stack([p.initial_x_for(p.desc.init, t.to_c()) + 0.05 * rng.standard_normal(p.n) for t in terrains])
    p.set_batch_terrain(_c_terrains(terrains))
    return p, terrains, dict(X=X, LAM=0.1 * rng.standard_normal((N, p.m)))


def _eval_now(p, X):
    import torch
    G, V = _nan(X.shape[0], p.m), _nan(X.shape[0], _ldv(p.nnz))
    p.eval_batch_device(_vec(X), G, V)
    torch.cuda.synchronize()
    return G, V


SOLVE_M, SOLVE_K = 24, 4     # iterations and iterations per round of the two driver tests


def test_compacting_solve_permutes_the_terrains():
    """alsolve_solve with compact = 1 on the smallest case, B = 7 (one problem of every id, drawn mu), rows 0, 2 and 3
    pre-frozen so that the permutation is not the identity, 24 iterations in rounds of 4 (the first round on 7 rows,
    the others on the 4 active ones at the front of a permuted private terrain copy): the persistent arrays of every
    problem are bit-equal to the uncompacted run; an evaluation after the call equals one before it (the handle's
    terrains are untouched) and equals each problem's oracle. Teeth on the device: the uncompacted solve run as its
    first round and the rest is bit-equal to the one call, and with the terrains rolled by one problem for the rest
    alone every active problem ends elsewhere, so a terrain row misplaced by the permutation could not pass."""
    import torch
    from tests.test_gpu_alsolve import SOLVE_PAR, _state
    from tests.test_gpu_solve import PERSISTENT, _assert_rows, _tiled
    B, M, K = 7, SOLVE_M, SOLVE_K
    p, terrains, h0 = _solver_case(B)
    par, gn, mem = alsolve_params(**SOLVE_PAR), gn_params(mu=MU), SOLVE_PAR["mem"]
    frozen, active = (0, 2, 3), (1, 4, 5, 6)
    own, rolled = _c_terrains(terrains), _c_terrains(terrains[1:] + terrains[:1])

    def solve(compact, schedule):
        """alsolve_init, rows `frozen` pre-frozen, then one alsolve_solve per (iterations, terrains) of `schedule`"""
        st = _state(p, B, mem, h0)
        p.set_batch_terrain(own)
        p.alsolve_init(par, st)
        for b, ph in zip(frozen, (2, 3, 4)):
            st.ISTATE.view(B, 4)[b, 0] = ph
        DC, GS, W = _tiled(p, B, 2)
        for iters, ter in schedule:
            p.set_batch_terrain(ter)
            rep = p.alsolve_solve(par, st, method=capi.SOLVE_GN_TILED, gn=gn, DC=DC, GSUM=GS, W=W, max_iters=iters, check_every=K,
                                  compact=compact)
        torch.cuda.synchronize()
        p.set_batch_terrain(own)
        return st, rep

    G0, V0 = _eval_now(p, h0["X"])
    plain, rp = solve(False, [(M, own)])
    comp, rc = solve(True, [(M, own)])
    print(f"compact {rc}; plain {rp}")
    assert rc["iters_run"] == rp["iters_run"] and rc["n_phase"] == rp["n_phase"]
    assert rc["problem_iters"] < rp["problem_iters"], "nothing was compacted"
    _assert_rows(comp, plain, range(B), PERSISTENT, "compact = 1 against compact = 0 with tilted terrains")
    G1, V1 = _eval_now(p, h0["X"])
    assert _same_bits(G0, G1) and _same_bits(V0, V1), "the handle's batch terrains changed"
    for b, t in enumerate(terrains):
        TC.gate(TC.SMALLEST, TC.reference(TC.SMALLEST, t, h0["X"][b]), G1[b].cpu().numpy(), V1[b, :p.nnz].cpu().numpy(),
                f"evaluation after the compacting solve, problem {b}")
    if rp["iters_run"] == M:      # (no problem froze early: the rounds after the first are there to be misplaced)
        split, _ = solve(False, [(K, own), (M - K, own)])
        _assert_rows(split, plain, range(B), PERSISTENT, "the first round and the rest against one call")
        late, _ = solve(False, [(K, own), (M - K, rolled)])
        Xa, Xb = plain.X.cpu().numpy()[:, :p.n], late.X.cpu().numpy()[:, :p.n]
        for b in active:
            assert (_np_bits(Xa[b]) != _np_bits(Xb[b])).any(), f"problem {b}: the rounds after the first do not depend on its terrain"
    assert rp["iters_run"] == M, rp
    p.close()


def test_queued_solve_moves_the_terrains():
    """alsolve_solve_queue on the smallest case: N = 7 problems (one of every id, drawn mu) through B = 3 slots, 24
    iterations in rounds of 4, so that every slot changes its tenant and its terrain row. The outputs are bit-equal to
    the one-batch solve on 7 rows, and an evaluation after the call equals one before it. Teeth on the device: the
    one-batch solve with the terrains rolled by one problem ends elsewhere in every problem."""
    import torch
    from tests.test_gpu_alsolve import SOLVE_PAR, _state
    from tests.test_gpu_queue import _assert_outputs, _assert_report, _outputs
    from tests.test_gpu_solve import _tiled
    N, B, M, K = 7, 3, SOLVE_M, SOLVE_K
    p, terrains, h0 = _solver_case(N)
    n, m = p.n, p.m
    par, gn, mem = alsolve_params(**SOLVE_PAR), gn_params(mu=MU), SOLVE_PAR["mem"]
    G0, V0 = _eval_now(p, h0["X"])

    def batch():
        st = _state(p, N, mem, h0)
        DCr, GSr, Wr = _tiled(p, N, 2)
        p.alsolve_init(par, st)
        rep = p.alsolve_solve(par, st, method=capi.SOLVE_GN_TILED, gn=gn, DC=DCr, GSUM=GSr, W=Wr, max_iters=M, check_every=K, compact=False)
        torch.cuda.synchronize()
        return st, rep

    ref, rref = batch()
    X0, LAM0 = _padded(h0["X"], n + 2), _padded(h0["LAM"], m + 3)
    st = _state(p, B, mem)
    DC, GS, W = _tiled(p, B, 2)
    res = p.alsolve_solve_queue(par, st, X0, LAM0=LAM0, method=capi.SOLVE_GN_TILED, gn=gn, DC=DC, GSUM=GS, W=W, max_iters=M,
                                check_every=K, out=_outputs(N, n, m))
    torch.cuda.synchronize()
    iters, ph = _assert_report(res, N, B, K)
    print(f"queue {res['rounds']} rounds, ITERS_OUT {iters.tolist()}, phases {ph.tolist()}; batch {rref}")
    assert res["rounds"] > M // K, "no slot changed its tenant"
    _assert_outputs(res, ref, N, n, m, "queued solve with tilted terrains")
    assert res["n_phase"] == rref["n_phase"]
    G1, V1 = _eval_now(p, h0["X"])
    assert _same_bits(G0, G1) and _same_bits(V0, V1), "the handle's batch terrains changed"
    p.set_batch_terrain(_c_terrains(terrains[1:] + terrains[:1]))
    other, _ = batch()
    Xa, Xb = ref.X.cpu().numpy()[:, :n], other.X.cpu().numpy()[:, :n]
    for b in range(N):
        assert (_np_bits(Xa[b]) != _np_bits(Xb[b])).any(), f"problem {b}: the solve does not depend on its terrain"
    p.close()


# ---- tie points ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TIE_CASES)
def test_tie_points_of_every_predicate(case):
    """Stance-node x variables set below, on and above every boundary of the terrain's closed comparisons
    (terrain_cases.tie_rows; the Steps boundaries decide whether the device's double division is the host's): one batch
    whose row b carries that row's terrain, and per terrain a handle created with desc.terrain = t evaluated row by row
    with eval_g_jac. Both against the oracle of that terrain on the rows where the foot position is a variable
    (Case.tie_rows_mask: every row but the instants after t = 0 of the discretised sets); outside the Gap class, whose
    single handles freeze their own pattern, the single call is bit-equal to the batch row in every row."""
    from tests.gap_frozen import frozen_reference
    from tests.parity import assert_close
    cs, p = TC.get(case), _handle(case)
    terrains, X = TC.tie_rows(case)
    G, V = _evaluate(p, terrains, X)
    assert np.isfinite(G).all() and np.isfinite(V).all()
    rows = cs.tie_rows_mask()

    def compared(g, v, g_ref, v_ref, r):
        """(g, v) with the rows that are not compared at a tie taken from the reference"""
        return np.where(rows, g, g_ref), np.where(rows[r], v, v_ref)
    worst = 0.0
    for b, t in enumerate(terrains):
        ref = TC.reference(case, t, X[b])
        st = TC.gate(case, ref, *compared(G[b], V[b], ref[0], ref[1], cs.r), f"{case} tie row {b} ({TC.NAMES[t.id]}) in the batch")
        worst = max(worst, st["worst"])
    single = {}
    for b, t in enumerate(terrains):
        if id(t) not in single:
            single[id(t)] = TowrGpuProblem(TC.with_terrain(cs.desc, t), device=0)
        q = single[id(t)]
        g, v = q.eval_g_jac(np.array(X[b]))
        what = f"{case} tie row {b} ({TC.NAMES[t.id]}) alone"
        if cs.gap:
            o, (r, c) = TC.oracle_for(case, t), q.jac_structure()
            g_ref, v_ref = o.eval_g(X[b]), frozen_reference(o, r, c, X[b])[0]
            gc, vc = compared(g, v, g_ref, v_ref, r)
            st = assert_close(g_ref, gc, r, v_ref, vc, q.m, what, cols_ref=c, floor_cols=TC.floor_cols(case))
        else:
            ref = TC.reference(case, t, X[b])
            st = TC.gate(case, ref, *compared(g, v, ref[0], ref[1], cs.r), what)
            _assert_bits(g[None], G[b:b + 1], what + ": g against the batch row")
            _assert_bits(v[None], V[b:b + 1], what + ": J against the batch row")
        worst = max(worst, st["worst"])
    for q in single.values():
        q.close()
    print(f"{case}: {len(terrains)} tie rows on {len(single)} terrains, worst |err| / tolerance {worst:.3g}")
