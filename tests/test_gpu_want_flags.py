"""Device batches with want_g = 0 or want_jac = 0 on the shapes of the seeded sweep and four named configurations
(tests/want_flags_cases.py has the (case, B) list and why no fixed-gait layout meets B >= 64 here;
tests/test_want_flags_cases.py the launch shapes the list reaches), and the consumer entry that forwards the flags.

Operands: X, G and V are each an interior view of a larger NaN-filled device tensor, GUARD rows before row 0 and after
row B - 1, leading dimensions ldx > n (odd, so that every second row is not 16-byte aligned), ldg = m + 3,
ldv = nnz + 5. X's padding and guard rows are NaN, so a read outside a row's first n entries reaches the outputs as
NaN. After every call the whole backing tensors come back to the host: every element outside the addressed [B, m] /
[B, nnz] windows must still hold the fill's bits, and X must be untouched.

Order within a test: the full call (oracle gate on rows 0..2, every row bit-equal to eval_g_jac of the same handle),
g only and the Jacobian only with the unwanted output non-null and NaN-filled (bit-equal to the full call, the whole
unwanted backing tensor still NaN), and only then the same two calls with the unwanted pointer None, back to back
without a synchronisation. A kernel that wrongly stores to an unwanted output thus fails an assertion first and never
meets a null pointer. No tolerance of its own: bit equality, and tests/parity.py's gate for the full call."""
import functools

import numpy as np
import pytest

from oracle.oracle import Oracle
from tests.parity import assert_close, residue_cols
from tests.test_gpu_sweep_consumers import CONSUMER_SEEDS
from tests.test_shape_sweep import _assert_pattern, _case, _points, _reference
from tests.want_flags_cases import CASE_B, NAMED, TERRAIN_CASES, desc_of
from towr2025_amd import TowrGpuProblem

pytestmark = pytest.mark.gpu

GUARD = 2
NAN_BITS = np.array([np.nan]).view(np.uint64)[0]   # the fill: torch.full's NaN


def _ldx(n):
    """The smallest leading dimension past n that is odd, so that rows alternate between 16-byte aligned and not
    (tests/gpu_helpers.py _ldx, with padding for an odd n too): n + 1 for an even n, n + 2 for an odd one."""
    return n + 1 if n % 2 == 0 else n + 2


class Guarded:
    """A (B, cols) window of a NaN-filled (B + 2 GUARD, ld) device tensor: `view` is what the engine gets, `host()` the
    whole backing tensor copied back and `check(what)` that everything outside the window still holds the fill."""

    def __init__(self, B, cols, ld, rows=None):
        import torch
        self.B, self.cols, self.ld = B, cols, ld
        self.back = torch.full((B + 2 * GUARD, ld), float("nan"), dtype=torch.float64, device="cuda:0")
        self.view = self.back[GUARD:GUARD + B]
        assert self.view.data_ptr() == self.back.data_ptr() + 8 * GUARD * ld and self.view.stride(0) == ld
        if rows is not None:
            self.view[:, :cols] = torch.from_numpy(np.ascontiguousarray(rows)).to("cuda:0")

    def host(self):
        return self.back.cpu().numpy()

    def window(self, H=None):
        H = self.host() if H is None else H
        return np.ascontiguousarray(H[GUARD:GUARD + self.B, :self.cols])

    def check(self, what, untouched=False):
        """The padding and guard rows (untouched: the whole tensor) still NaN, bit for bit; returns the window."""
        H = self.host()
        outside = np.ones(H.shape, dtype=bool)
        if not untouched:
            outside[GUARD:GUARD + self.B, :self.cols] = False
        bad = np.argwhere(outside & (H.view(np.uint64) != NAN_BITS))
        where = "of an output that was not wanted" if untouched else "outside the addressed window"
        assert bad.size == 0, (f"{what}: {len(bad)} elements {where} were written, first at backing row "
                               f"{bad[0][0]} (window rows {GUARD}..{GUARD + self.B - 1}) column {bad[0][1]} of {self.cols}")
        return self.window(H)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b, what):
    diff = np.argwhere(_bits(a) != _bits(b))
    assert diff.size == 0, f"{what}: {len(diff)} entries differ, first at row {diff[0][0]} column {diff[0][1]}: {a[tuple(diff[0])]!r} != {b[tuple(diff[0])]!r}"


@functools.lru_cache(maxsize=None)
def _wf_case(case):
    """test_shape_sweep._case for a seed or STAGE_OVERFLOW, the same tuple for a named configuration (shared by the
    case's batch sizes and left unchanged)."""
    if case not in NAMED:
        return _case(case)
    desc = desc_of(case)
    o = Oracle(desc)
    x0 = o.initial_x()
    r, c, _ = o.eval_jac(x0)
    return desc, {"seed": case}, o, x0, r, c


def _wf_points(case, x0, count):
    if case not in NAMED:
        return _points(case, x0, count)
    rng = np.random.default_rng(2000003 + NAMED.index(case))
    return [x0] + [x0 + 0.05 * rng.standard_normal(x0.size) for _ in range(count - 1)]


def _run(p, Xg, X, B, want_g, want_jac, what):
    """One eval_batch_device into fresh guarded outputs; returns (G window or None, V window or None) after the
    padding, guard and untouched-output checks."""
    import torch
    Gg, Vg = Guarded(B, p.m, p.m + 3), Guarded(B, p.nnz, p.nnz + 5)
    p.eval_batch_device(Xg.view, Gg.view, Vg.view, want_g=want_g, want_jac=want_jac)
    torch.cuda.synchronize()
    _same(Xg.check(f"{what}: X"), X, f"{what}: X was written")
    G = Gg.check(f"{what}: G", untouched=not want_g)
    V = Vg.check(f"{what}: V", untouched=not want_jac)
    return (G if want_g else None), (V if want_jac else None)


def _flag_steps(p, Xg, X, B, G, V, what, null_variants=True):
    """Steps 2-4 of the module docstring against the full call's (G, V)."""
    import torch
    Gg, _ = _run(p, Xg, X, B, True, False, f"{what} g only")
    _same(Gg, G, f"{what} g only: G against the full call")
    _, Vj = _run(p, Xg, X, B, False, True, f"{what} Jacobian only")
    _same(Vj, V, f"{what} Jacobian only: V against the full call")
    if not null_variants:
        return
    Gn, Vn = Guarded(B, p.m, p.m + 3), Guarded(B, p.nnz, p.nnz + 5)
    p.eval_batch_device(Xg.view, Gn.view, None, want_g=True, want_jac=False)
    p.eval_batch_device(Xg.view, None, Vn.view, want_g=False, want_jac=True)
    torch.cuda.synchronize()
    _same(Gn.check(f"{what} g only, V = None: G"), G, f"{what} g only, V = None: G against the full call")
    _same(Vn.check(f"{what} Jacobian only, G = None: V"), V, f"{what} Jacobian only, G = None: V against the full call")
    _same(Xg.check(f"{what} None variants: X"), X, f"{what} None variants: X was written")


@pytest.mark.parametrize("case,B", CASE_B, ids=[f"{c}-B{B}" for c, B in CASE_B])
def test_g_only_and_jacobian_only_batches(case, B):
    desc, info, o, x0, r, c = _wf_case(case)
    p = TowrGpuProblem(desc, device=0)
    _assert_pattern(p, o, x0, r, c, f"{case}")
    X = np.stack(_wf_points(case, x0, B))
    Xg = Guarded(B, p.n, _ldx(p.n), X)
    what = f"{case} B = {B}"
    G, V = _run(p, Xg, X, B, True, True, f"{what} full call")
    fc = residue_cols(desc, o.n)
    worst = 0.0
    for k in range(3):
        g_ref, v_ref = _reference(o, r, c, X[k], f"{what} point {k}")
        st = assert_close(g_ref, G[k], r, v_ref, V[k], o.m, f"{what} full call row {k}", cols_ref=c, floor_cols=fc)
        worst = max(worst, st["worst"])
    print(f"{what}: n={p.n} m={p.m} nnz={p.nnz} worst |err|/tol {worst:.3f}")
    for k, x in enumerate(X):
        g, v = p.eval_g_jac(x)
        _same(G[k:k + 1], g[None], f"{what}: g of batch row {k} against eval_g_jac")
        _same(V[k:k + 1], v[None], f"{what}: J of batch row {k} against eval_g_jac")
    _flag_steps(p, Xg, X, B, G, V, what)
    p.close()


@pytest.mark.parametrize("case,B", TERRAIN_CASES, ids=[f"{c}-B{B}" for c, B in TERRAIN_CASES])
def test_flags_with_per_problem_terrains(case, B):
    """set_batch_terrain (bench.make_batch's randomised start, goal and Flat / Stairs terrain per problem): the full
    call, g only and the Jacobian only; rows 0 and B - 1 against an oracle built with that row's terrain."""
    import bench
    desc, info, o0, x0, r, c = _wf_case(case)
    gait = bool(desc.optimize_timings)
    p = TowrGpuProblem(desc, device=0)
    Xh, terrains = bench.make_batch(p, B, first_id=4400, optimize_timings=gait)
    X = np.ascontiguousarray(Xh[0])
    p.set_batch_terrain(terrains)
    Xg = Guarded(B, p.n, _ldx(p.n), X)
    what = f"{case} B = {B} per-problem terrains"
    G, V = _run(p, Xg, X, B, True, True, f"{what} full call")
    for b in (0, B - 1):
        d = type(desc).from_buffer_copy(desc)   # the shared description stays untouched
        d.terrain = terrains[b]
        o = Oracle(d)
        g_ref, v_ref = _reference(o, r, c, X[b], f"{what} row {b}")
        st = assert_close(g_ref, G[b], r, v_ref, V[b], o.m, f"{what} full call row {b}", cols_ref=c, floor_cols=residue_cols(d, o.n))
        print(f"{what} row {b}: worst |err|/tol {st['worst']:.3f}")
    _flag_steps(p, Xg, X, B, G, V, what, null_variants=False)
    p.close()


CONSUMER_B = 5


@pytest.mark.parametrize("seed", CONSUMER_SEEDS)
def test_products_entry_forwards_the_flags(seed):
    """towr_gpu_eval_products_batch_device at B = 5 on CONSUMER_SEEDS: with G alone it evaluates with want_jac = 0 and
    no V (its `!want_v` branch), with LAM / Z and no G with want_g = 0 and no G. G is bit-equal to the evaluator's, Z
    has the same bits with and without G, and nothing outside the windows of G, Z, LAM or X is written."""
    import torch
    desc, info, o, x0, r, c = _wf_case(seed)
    p = TowrGpuProblem(desc, device=0)
    B = CONSUMER_B
    X = np.stack(_wf_points(seed, x0, B))
    LAM = np.random.default_rng(31000 + seed).standard_normal((B, p.m))
    Xg, Lg = Guarded(B, p.n, _ldx(p.n), X), Guarded(B, p.m, p.m + 9, LAM)
    what = f"seed {seed} products entry"
    G, _ = _run(p, Xg, X, B, True, True, f"{what}: the evaluator's full call")
    Gg = Guarded(B, p.m, p.m + 3)
    p.eval_products_batch_device(Xg.view, G=Gg.view)
    torch.cuda.synchronize()
    _same(Gg.check(f"{what} G alone: G"), G, f"{what} G alone: G against the evaluator's")
    G2, Z1, Z2 = Guarded(B, p.m, p.m + 3), Guarded(B, p.n, p.n + 3), Guarded(B, p.n, p.n + 3)
    p.eval_products_batch_device(Xg.view, G=G2.view, LAM=Lg.view, Z=Z1.view)
    p.eval_products_batch_device(Xg.view, LAM=Lg.view, Z=Z2.view)
    torch.cuda.synchronize()
    _same(G2.check(f"{what} G, LAM, Z: G"), G, f"{what} G, LAM, Z: G against the evaluator's")
    z1, z2 = Z1.check(f"{what} G, LAM, Z: Z"), Z2.check(f"{what} LAM, Z: Z")
    assert np.isfinite(z1).all(), f"{what}: Z is not finite"
    _same(z2, z1, f"{what}: Z without G against Z with G")
    _same(Xg.check(f"{what}: X"), X, f"{what}: X was written")
    _same(Lg.check(f"{what}: LAM"), LAM, f"{what}: LAM was written")
    p.close()
