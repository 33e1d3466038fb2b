"""The queued solve on the device (include/towr_gpu.h): the retire key (towr_gpu_alsolve_retire_key_batch_device) and the
row move by index (towr_gpu_alsolve_move_rows_batch_device) against numpy, and the driver
(towr_gpu_alsolve_solve_queue_batch_device) against the solve entries on all N problems as one batch. The driver is compared
bit for bit: problem b's outputs are a function of its own operands alone, so neither the slot a problem occupies, nor its
neighbours, nor what an earlier tenant left in the slot may change a bit. Padded leading dimensions with NaN padding."""
import functools

import numpy as np
import pytest

from tests import alsolve_ref as R
from tests import compact_ref as CR
from tests import queue_ref as QR
from tests import stop_ref as S
from tests.gpu_helpers import _dev, _nan, _same_bits, _terrains, _vec
from tests.test_gpu_alsolve import ALL, SOLVE_PAR, _start, _state
from tests.test_gpu_lbfgs import _ints, _problem
from tests.test_gpu_solve import _bytes, _row, _tiled, method_iterate, method_operands
from towr2025_amd import _capi as capi, alsolve_params, alsolve_stop_params, gn_params

pytestmark = pytest.mark.gpu

MU = 1e-6
INT32_MIN = -2 ** 31
OUTS = ("X_OUT", "LAM_OUT", "RHO_OUT", "SCAL_OUT", "ISTATE_OUT")


# ---- the retire key ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 64, 65, 257])
def test_retire_key_equals_numpy(B):
    """Seeded phase words (0..7, -1, INT32_MIN; the other three words of a row are noise) and ages on both sides of max_age
    (and on it): KEY[4 b] equals numpy's, the other KEY words keep their fill, ISTATE and (add = 0) AGE are byte-unchanged;
    the partition on KEY equals tests/compact_ref.py's of the keyed words; add > 0 is added to AGE first."""
    import torch
    p = _problem("monoped_procedural")[0]
    rng = np.random.default_rng(6100 + B)
    words = np.array([0, 1, 2, 3, 4, 5, 6, 7, -1, INT32_MIN])
    max_age = 12
    ist = rng.integers(-5, 9, size=(B, 4))
    ist[:, 0] = rng.choice(words, size=B, p=[.25, .25] + [.0625] * 8)
    if B >= 10:
        ist[:10, 0] = words
    age = rng.choice([0, 4, 8, 11, 12, 13, 16, 400], size=B)
    ISTATE, AGE, KEY = _ints(ist.reshape(-1)), _ints(age), _ints(np.full(4 * B + 3, -77))
    p.alsolve_retire_key(ISTATE, AGE, KEY, max_age, B=B)
    torch.cuda.synchronize()
    want = QR.retire_key(ist[:, 0], age, max_age)
    assert ((want == 7) & (ist[:, 0] != 7)).any() or B == 1
    key = KEY.cpu().numpy()
    assert np.array_equal(key[:4 * B].reshape(B, 4)[:, 0], want), f"B={B}: KEY"
    assert (key[:4 * B].reshape(B, 4)[:, 1:] == -77).all() and (key[4 * B:] == -77).all(), f"B={B}: KEY written beyond its word"
    assert np.array_equal(ISTATE.cpu().numpy(), ist.reshape(-1).astype(np.int32)), f"B={B}: ISTATE written"
    assert np.array_equal(AGE.cpu().numpy(), age.astype(np.int32)), f"B={B}: AGE written with add = 0"
    HEAD, PAIRS = _ints(np.full(8, -77)), _ints(np.full(2 * (B // 2) + 2, -77))
    p.alsolve_partition(KEY, HEAD, PAIRS, B=B)
    head_ref, pairs_ref = CR.partition(want)
    npairs = int(head_ref[1])
    assert np.array_equal(HEAD.cpu().numpy(), head_ref), f"B={B}: HEAD"
    assert np.array_equal(PAIRS.cpu().numpy()[:2 * npairs].reshape(-1, 2), pairs_ref) and (PAIRS.cpu().numpy()[2 * npairs:] == -77).all()
    p.alsolve_retire_key(ISTATE, AGE, KEY, max_age, add=4, B=B)
    assert np.array_equal(AGE.cpu().numpy(), (age + 4).astype(np.int32)), f"B={B}: AGE += add"
    assert np.array_equal(KEY.cpu().numpy()[:4 * B].reshape(B, 4)[:, 0], QR.retire_key(ist[:, 0], age + 4, max_age))
    assert np.array_equal(ISTATE.cpu().numpy(), ist.reshape(-1).astype(np.int32))


# ---- the move ------------------------------------------------------------------------------------------------------------
def test_move_rows_scatters_and_gathers_the_used_bytes_only():
    """Five array pairs in one call: doubles at ld = n + 3 (NaN padding) into ld = n + 1, int32 rows of 4, rows of 1 double,
    int32 rows of 3 at ld = 5 (the 4-byte path; -99 padding) and 80-byte rows. Rows 5..41 of the 50 slot rows are scattered
    into 300 by a seeded ID with two negative entries; the result equals numpy byte for byte, every padding byte and every
    untouched row kept; gathered back (reverse) into NaN-filled slots it restores the moved rows and nothing else;
    count = 0 changes nothing."""
    import torch
    p = _problem("monoped_procedural")[0]
    slots, rows, n, r0, count = 50, 300, 77, 5, 37
    rng = np.random.default_rng(6200)
    ids = np.full(slots, 10 ** 6)            # (rows outside [r0, r0 + count) are never read)
    ids[r0:r0 + count] = rng.permutation(rows)[:count]
    skipped = [r0 + 3, r0 + 30]
    ids[skipped] = [-1, INT32_MIN]
    ID = _ints(ids)
    cols = [n, 4, None, 3, 10]

    def make(nrows, lds, seed):
        g = np.random.default_rng(seed)
        A = _nan(nrows, lds[0])
        A[:, :n] = _vec(g.standard_normal((nrows, n)))
        I4 = _ints(g.integers(-9, 9, (nrows, 4)))
        V1 = _vec(g.standard_normal(nrows))
        I3 = _ints(np.full((nrows, lds[1]), -99))
        I3[:, :3] = _ints(g.integers(-9, 9, (nrows, 3)))
        W10 = _nan(nrows, lds[2])
        W10[:, :10] = _vec(g.standard_normal((nrows, 10)))
        return [A, I4, V1, I3, W10]

    def arrays(ts):
        return [t if c is None else (t, c) for t, c in zip(ts, cols)]

    def host(ts):
        return [t.cpu().numpy().copy() for t in ts]

    def same(x, y):
        return all(a.tobytes() == b.tobytes() for a, b in zip(x, y))

    S_, O_ = make(slots, (n + 3, 5, 10), 1), make(rows, (n + 1, 5, 12), 2)
    s0, o0 = host(S_), host(O_)
    want = [a.copy() for a in o0]
    for a, s, c in zip(want, s0, cols):
        for i in range(r0, r0 + count):
            if ids[i] >= 0:
                if c is None:
                    a[ids[i]] = s[i]
                else:
                    a[ids[i], :c] = s[i, :c]
    p.alsolve_move_rows(ID, arrays(S_), arrays(O_), count, r0=r0)
    torch.cuda.synchronize()
    assert same(host(O_), want), "the scatter differs from numpy's (or touched padding or another row)"
    assert same(host(S_), s0), "the scatter wrote its source"
    assert not same(want, o0)
    p.alsolve_move_rows(ID, arrays(S_), arrays(O_), 0, r0=r0)
    p.alsolve_move_rows(ID, arrays(S_), arrays(O_), 0, r0=r0, reverse=True)
    p.alsolve_move_rows(ID, [], [], count, r0=r0)
    assert same(host(O_), want) and same(host(S_), s0), "count = 0 or no arrays moved something"
    # back into fresh slots: only the moved rows' used bytes arrive
    T_ = make(slots, (n + 3, 5, 10), 3)
    t0 = host(T_)
    back = [a.copy() for a in t0]
    for a, s, c in zip(back, s0, cols):
        for i in range(r0, r0 + count):
            if ids[i] >= 0:
                if c is None:
                    a[i] = s[i]
                else:
                    a[i, :c] = s[i, :c]
    p.alsolve_move_rows(ID, arrays(T_), arrays(O_), count, r0=r0, reverse=True)
    torch.cuda.synchronize()
    assert same(host(T_), back), "the gather differs from numpy's (or touched padding or another row)"
    assert same(host(O_), want), "the gather wrote its source"


# ---- the driver --------------------------------------------------------------------------------------------------------
def _outputs(N, n, m):
    """NaN / -77 filled outputs at padded leading dimensions."""
    import torch
    return dict(X_OUT=_nan(N, n + 2), LAM_OUT=_nan(N, m + 1), RHO_OUT=torch.full((N,), float("nan"), dtype=torch.float64, device=_dev()),
                SCAL_OUT=_nan(N, 8), ISTATE_OUT=_ints(np.full(4 * N, -77)), ITERS_OUT=_ints(np.full(N, -77)))


def _assert_outputs(res, ref, N, n, m, what, scal=8):
    """The queue's five outputs are the batch state's rows in every bit; the outputs' padding is untouched."""
    import torch
    assert _same_bits(res["X_OUT"][:, :n], ref.X[:N, :n]), f"{what}: X_OUT"
    assert _same_bits(res["LAM_OUT"][:, :m], ref.LAM[:N, :m]), f"{what}: LAM_OUT"
    assert _same_bits(res["RHO_OUT"], ref.RHO[:N]), f"{what}: RHO_OUT"
    assert _same_bits(res["SCAL_OUT"][:, :scal], ref.SCAL[:N, :scal]), f"{what}: SCAL_OUT"
    assert torch.equal(res["ISTATE_OUT"], ref.ISTATE[:4 * N]), f"{what}: ISTATE_OUT"
    assert torch.isnan(res["X_OUT"][:, n:]).all() and torch.isnan(res["LAM_OUT"][:, m:]).all(), f"{what}: output padding written"


def _assert_report(rep, N, B, K):
    iters = rep["ITERS_OUT"].cpu().numpy()
    assert rep["problem_iters"] == int(iters.sum()), rep
    assert rep["rounds"] >= -(-rep["problem_iters"] // (B * K)) and rep["iters_run"] == K * rep["rounds"], rep
    ph = rep["ISTATE_OUT"].cpu().numpy().reshape(N, 4)[:, 0]
    counts = [int((ph == k).sum()) for k in range(5)]
    assert rep["n_phase"] == counts + [N - sum(counts)], rep
    return iters, ph


def _monoped_starts(p, N):
    x0 = p.initial_x()
    return dict(X=np.stack([x0 + 0.05 * np.random.default_rng(900 + b).standard_normal(p.n) for b in range(N)]),
                LAM=np.zeros((N, p.m)))


@functools.lru_cache(maxsize=None)
def _monoped_batch(N, M, K, stop=False):
    """The reference, computed once and left unchanged: alsolve_init and the solve entry on the N starts as one batch."""
    import torch
    p = _problem("monoped_procedural")[0]
    par, gn = alsolve_params(**SOLVE_PAR), gn_params(mu=MU)
    st = _state(p, N, SOLVE_PAR["mem"], _monoped_starts(p, N))
    DC, GS, W = _tiled(p, N, 4)
    p.alsolve_init(par, st)
    rep = p.alsolve_solve(par, st, method=capi.SOLVE_GN_TILED, gn=gn, DC=DC, GSUM=GS, W=W, max_iters=M, check_every=K,
                          compact=False, stop=alsolve_stop_params(**S.EXAMPLE) if stop else None)
    torch.cuda.synchronize()
    return st, rep


@pytest.mark.parametrize("N,M", [(13, 40), (6, 100)])
def test_queue_equals_batch(N, M):
    """monoped_procedural, seeds 900.., B = 4 slots, TOWR_SOLVE_GN_TILED, wrows = 4, K = 4, SOLVE_PAR, mu = 1e-6: the five
    outputs of all N problems are bit-equal to alsolve_solve on N rows with compact = 0 and the same M, K. Start 900 freezes
    at iteration 67: at M = 40 it comes out expired (its phase word still active, ITERS_OUT = 40), at M = 100 CONVERGED with
    ITERS_OUT = 68. The slots are NaN-filled in the first run and hold the first run's leftovers in the second: the results
    are the same."""
    import torch
    B, K = 4, 4
    p = _problem("monoped_procedural")[0]
    n, m, mem = p.n, p.m, SOLVE_PAR["mem"]
    par, gn = alsolve_params(**SOLVE_PAR), gn_params(mu=MU)
    ref, rref = _monoped_batch(N, M, K)
    h0 = _monoped_starts(p, N)
    X0 = _nan(N, n + 1)
    X0[:, :n] = _vec(h0["X"])
    st = _state(p, B, mem)                  # NaN everywhere: nothing of a slot may reach a result
    DC, GS, W = _tiled(p, B, 4)
    for fill in ("NaN", "the previous solve's state"):
        res = p.alsolve_solve_queue(par, st, X0, method=capi.SOLVE_GN_TILED, gn=gn, DC=DC, GSUM=GS, W=W, max_iters=M,
                                    check_every=K, out=_outputs(N, n, m))
        torch.cuda.synchronize()
        iters, ph = _assert_report(res, N, B, K)
        print(f"N={N} M={M} slots filled with {fill}: rounds {res['rounds']}, problem_iters {res['problem_iters']}, "
              f"ITERS_OUT {iters.tolist()}, phases {ph.tolist()}; batch {rref}")
        _assert_outputs(res, ref, N, n, m, f"N={N} M={M} ({fill})")
        assert res["n_phase"] == rref["n_phase"]
        assert ((iters % K == 0) & (iters > 0) & (iters <= M)).all()
        assert (iters[np.isin(ph, (0, 1))] == M).all(), "only an expired problem comes out with an active word"
        if M == 40:
            assert ph[0] in (R.RESTART, R.SEARCH) and iters[0] == 40
        else:
            assert ph[0] == R.CONVERGED and iters[0] == 68
        assert _same_bits(X0[:, :n], _vec(h0["X"])) and torch.isnan(X0[:, n:]).all(), "X0 was written"


def test_shapes_of_the_queue():
    """monoped_procedural, the tiled method, M = 8, K = 4: B = 1 with N = 3 (serial), N = 3 through B = 8 (the slot rows
    beyond N keep every byte), N = B = 5 and N = 0 (nothing runs, the report is zero); each bit-equal to the batch solve.
    A second run on another stream gives the same bits."""
    import torch
    p = _problem("monoped_procedural")[0]
    n, m, mem, M, K = p.n, p.m, SOLVE_PAR["mem"], 8, 4
    par, gn = alsolve_params(**SOLVE_PAR), gn_params(mu=MU)
    s2 = torch.cuda.Stream(device=_dev())
    for N, B in ((3, 1), (3, 8), (5, 5), (0, 2)):
        h0 = _monoped_starts(p, max(N, 1))
        X0 = _vec(h0["X"][:N])
        st = _state(p, B, mem)
        DC, GS, W = _tiled(p, B, 2)
        before = {k: [_row(st, k, b) for b in range(B)] for k in ALL}
        before.update(DC=_bytes(DC[N:]), GSUM=_bytes(GS[N:]))
        res = p.alsolve_solve_queue(par, st, X0, method=capi.SOLVE_GN_TILED, gn=gn, DC=DC, GSUM=GS, W=W, max_iters=M, check_every=K,
                                    out=_outputs(N, n, m))
        torch.cuda.synchronize()
        if N == 0:
            assert {k: res[k] for k in ("rounds", "iters_run", "problem_iters", "n_phase")} == \
                dict(rounds=0, iters_run=0, problem_iters=0, n_phase=[0] * 6)
            assert all(_row(st, k, b) == before[k][b] for k in ALL for b in range(B)), "N = 0 wrote the slots"
            continue
        ref, _ = _monoped_batch(N, M, K)
        iters, ph = _assert_report(res, N, B, K)
        _assert_outputs(res, ref, N, n, m, f"N={N} B={B}")
        if (iters == M).all():          # (no start froze within the 8 iterations)
            assert res["rounds"] == {(3, 1): 6, (3, 8): 2, (5, 5): 2}[N, B], (N, B, res["rounds"])
        for b in range(N, B):
            for k in ALL:
                assert _row(st, k, b) == before[k][b], f"N={N} B={B}: slot row {b}: {k} written"
        assert _bytes(DC[N:]) == before["DC"] and _bytes(GS[N:]) == before["GSUM"]
        s2.wait_stream(torch.cuda.current_stream())
        res2 = p.alsolve_solve_queue(par, st, X0, method=capi.SOLVE_GN_TILED, gn=gn, DC=DC, GSUM=GS, W=W, max_iters=M,
                                     check_every=K, out=_outputs(N, n, m), stream=s2)
        torch.cuda.synchronize()
        for k in OUTS + ("ITERS_OUT",):
            assert _bytes(res2[k]) == _bytes(res[k]), f"N={N} B={B}: {k} on another stream"


def test_per_problem_everything():
    """Sweep seed 196 (n = 78), N = 7 through B = 3, the tiled method, N batch terrains, per-problem GL / GU / XL / XU rows
    at ld = m + 1 / n + 1 with NaN padding (work rows at other leading dimensions), LAM0 given, M = 6, K = 2: the outputs
    are bit-equal to the ex entry on 7 rows; the caller's bound rows, X0 and LAM0 are byte-unchanged, and an evaluation
    after the call equals one before it (the handle's terrains are untouched)."""
    import torch
    from tests.shape_sweep import make
    from towr2025_amd import TowrGpuProblem
    f = make(196)[0]
    f.params_.enable_stance_tracking = False
    p = TowrGpuProblem(f.to_desc(), device=0, data=f.var_bounds_data())
    N, B, n, m, M, K = 7, 3, p.n, p.m, 6, 2
    assert n == 78
    lo, up = p.variable_bounds()
    gl, gu = p.constraint_bounds()
    p.set_batch_terrain(_terrains("sweep_seed_196", N, np.random.default_rng(196)))
    par, gn, mem = alsolve_params(**SOLVE_PAR), gn_params(mu=MU), SOLVE_PAR["mem"]
    h0 = _start(p, lo, up, N, mem, 19600)
    shift = 1e-3 * np.arange(N)[:, None]

    def padded(a, ld):
        t = _nan(a.shape[0], ld)
        t[:, :a.shape[1]] = _vec(a)
        return t

    bounds = dict(GL=padded(gl[None, :] + shift, m + 1), GU=padded(gu[None, :] + shift, m + 1),
                  XL=padded(lo[None, :] - shift, n + 1), XU=padded(up[None, :] + shift, n + 1))
    Xe = _vec(h0["X"])
    G0, V0 = _nan(N, m), _nan(N, p.nnz)
    p.eval_batch_device(Xe, G0, V0)
    ref = _state(p, N, mem, h0)
    DCr, GSr, Wr = _tiled(p, N, 2)
    p.alsolve_init(par, ref, XL=bounds["XL"], XU=bounds["XU"])
    rref = p.alsolve_solve(par, ref, method=capi.SOLVE_GN_TILED, gn=gn, DC=DCr, GSUM=GSr, W=Wr, max_iters=M, check_every=K,
                           compact=True, ex=True, **bounds)
    torch.cuda.synchronize()
    X0, LAM0 = padded(h0["X"], n + 2), padded(h0["LAM"], m + 3)
    inputs = dict(bounds, X0=X0, LAM0=LAM0)
    inputs0 = {k: _bytes(t) for k, t in inputs.items()}
    work = dict(GLW=_nan(B, m + 2), GUW=_nan(B, m + 2), XLW=_nan(B, n + 4), XUW=_nan(B, n + 4))
    st = _state(p, B, mem)
    DC, GS, W = _tiled(p, B, 2)
    res = p.alsolve_solve_queue(par, st, X0, LAM0=LAM0, method=capi.SOLVE_GN_TILED, gn=gn, DC=DC, GSUM=GS, W=W, max_iters=M,
                                check_every=K, work=work, out=_outputs(N, n, m), **bounds)
    torch.cuda.synchronize()
    iters, ph = _assert_report(res, N, B, K)
    print(f"queue {res['rounds']} rounds, ITERS_OUT {iters.tolist()}, phases {ph.tolist()}; batch {rref}")
    _assert_outputs(res, ref, N, n, m, "per-problem everything")
    assert res["n_phase"] == rref["n_phase"] and (res["rounds"] == 9 or not (iters == M).all())
    for k, t in inputs.items():
        assert _bytes(t) == inputs0[k], f"{k} was written"
    assert all(torch.isnan(work[k][:, c:]).all() for k, c in (("GLW", m), ("GUW", m), ("XLW", n), ("XUW", n))), "work rows' padding"
    G1, V1 = _nan(N, m), _nan(N, p.nnz)
    p.eval_batch_device(Xe, G1, V1)
    assert _same_bits(G0, G1) and _same_bits(V0, V1), "the handle's batch terrains changed"


@pytest.mark.parametrize("method", [capi.SOLVE_LBFGS, capi.SOLVE_GN_PC, capi.SOLVE_GN, capi.SOLVE_GN_DIRECT])
def test_methods_equal_their_iterate_entry(method):
    """monoped_procedural, N = 5 through B = 2, M = 8, K = 4: the outputs are the method's iterate entry's after 8 iterations
    on the 5 rows. With L-BFGS a slot's history rows are an earlier tenant's when a problem enters: the slots start with NaN
    history rows and a HMETA that points into them, so a history that leaked would show. The operands beside the state are
    tests/test_gpu_solve.py's method_operands: the direct method's W has one row for the two slots."""
    import torch
    p, lo, up, _ = _problem("monoped_procedural")
    N, B, n, m, mem, M, K = 5, 2, p.n, p.m, SOLVE_PAR["mem"], 8, 4
    par = alsolve_params(**SOLVE_PAR)
    h0 = _start(p, lo, up, N, mem, 7700)
    ref = _state(p, N, mem, h0)
    p.alsolve_init(par, ref)
    method_iterate(p, method, par, ref, method_operands(p, method, N, 2), M)
    torch.cuda.synchronize()
    st = _state(p, B, mem)
    st.HMETA.fill_(3)                       # (a count and a head that point into the NaN history rows)
    kw = method_operands(p, method, B, 1)
    res = p.alsolve_solve_queue(par, st, _vec(h0["X"]), LAM0=_vec(h0["LAM"]), method=method, max_iters=M, check_every=K,
                                out=_outputs(N, n, m), **kw)
    torch.cuda.synchronize()
    iters, ph = _assert_report(res, N, B, K)
    _assert_outputs(res, ref, N, n, m, f"method {method}")
    assert res["rounds"] == 6 or not (iters == M).all(), (iters, res["rounds"])
    if "GSUM" in kw:
        assert torch.isnan(kw["GSUM"][:, 6 if method == capi.SOLVE_GN else 8:]).all() and torch.isnan(kw["DC"][:, n:]).all(), "padding written"
    if "W" in kw:
        assert torch.isnan(kw["W"][:, p.gn_factor_info()["ldw_min"]:]).all(), "the workspace's padding was written"


def test_with_a_stop_rule():
    """monoped_procedural, the example parameters of the stop rule, N = 6 through B = 2, the tiled method, M = 40, K = 4:
    bit-equal to solve_ex with the rule on the six as one batch, SCAL[6..7] (the rule's memory) included."""
    import torch
    N, B, M, K = 6, 2, 40, 4
    p = _problem("monoped_procedural")[0]
    n, m, mem = p.n, p.m, SOLVE_PAR["mem"]
    par, gn, sp = alsolve_params(**SOLVE_PAR), gn_params(mu=MU), alsolve_stop_params(**S.EXAMPLE)
    ref, rref = _monoped_batch(N, M, K, True)
    st = _state(p, B, mem)
    DC, GS, W = _tiled(p, B, 4)
    res = p.alsolve_solve_queue(par, st, _vec(_monoped_starts(p, N)["X"]), method=capi.SOLVE_GN_TILED, gn=gn, DC=DC, GSUM=GS, W=W,
                                max_iters=M, check_every=K, out=_outputs(N, n, m), stop=sp)
    torch.cuda.synchronize()
    iters, ph = _assert_report(res, N, B, K)
    print(f"ITERS_OUT {iters.tolist()}, phases {ph.tolist()}, SCAL[6..7] {res['SCAL_OUT'][:, 6:].tolist()}; batch {rref}")
    _assert_outputs(res, ref, N, n, m, "with the rule")
    assert (res["n_acceptable"], res["n_infeasible"]) == (rref["n_acceptable"], rref["n_infeasible"])
    assert res["n_phase"] == rref["n_phase"] and (res["SCAL_OUT"][:, 6:] != 0).any(), "the rule never wrote its memory"
