"""towr_gn_direct_kernel (the envelope Cholesky) and towr_gn_tiled_kernel (the 16 x 16 block Cholesky) on shapes of the
seeded sweep (tests/shape_sweep.py) instead of the five Jacobian patterns of tests/test_gpu_gn_direct.py /
tests/test_gpu_gn_tiled.py: the thirteen CONSUMER_SEEDS and three seeds with one, fifteen and no live row in the last
tile's padding (144, 81, 180; the last has fewer block rows than the kernel has waves). Which branch of either kernel
each case reaches is computed and asserted on the CPU (tests/test_chol_branches.py). B = 3, wrows = 2 (two
launches, the second partial), padded leading dimensions with NaN padding, NaN-filled D, SUM and W.

Operands: tests/test_gpu_sweep_gn.py's (the device's own CSR values, lam+ of the residual kernel, rho_b = 10 (1 + b),
the handle's bounds or, where they hold no column, drawn ones passed as XL / XU), mu = 1e-6.

Gates, none of them measured on a kernel. The held columns of D, the held count, the code and SUM[7] are exact. The
backward error max |g_f - (H D)_f|, H assembled in long double from the device's V, is held to 8 x the larger backward
error of the two float64 evaluations of tests/chol_ref.py (the rule of the two files above). SUM[1] and SUM[3] are held
to long double sums within 8 n 2^-53. SUM[2] and SUM[6], the smallest and largest counted pivot, are held to the long
double tiled reference within tests/test_chol_branches.pivot_gate: 8 x the largest distance of the three float64
references from it, at least n 2^-53 of the value; where the long double smallest pivot is mu itself (a free column
without an active entry: rho * 0 + mu, no rounding) SUM[2] must be mu exactly. The two entries are compared with each
other where include/towr_gpu.h promises the same bits: the held columns of D, SUM[0], [4], [5], [7], and SUM[1] (the tiled
entry keeps "bb and its sum" of the direct entry word for word). The ratios per case on MI355X: DESIGN 4m / 4n."""
import functools

import numpy as np
import pytest

from tests import chol_ref as CH
from tests import lbfgs_ref
from tests import test_gpu_alsolve as AL
from tests import test_gpu_gn_direct as DI
from tests import test_gpu_gn_tiled as TI
from tests import test_gpu_sweep_gn as SG
from tests.gpu_helpers import _nan, _np_bits, _padded, _same_bits, _vec
from tests.test_chol_branches import CASES, EDGE_SEEDS, hold_small_pivots, pivot_gate, pivot_refs
from tests.test_gpu_lbfgs import _problem
from towr2025_amd import alsolve_params, gn_params

pytestmark = pytest.mark.gpu

B, WROWS = 3, 2
MU = 1e-6
MU_OF = {}          # a case whose float64 references do not all solve at MU on the device's V: its raised mu (none needs one)
KERNELS = {"direct": DI, "tiled": TI}
# the isolation and breakdown checks: the three edge shapes, then the largest n and the widest envelope
ISOLATION = [f"sweep_seed_{s}" for s in EDGE_SEEDS + (93, 10)]
# (name, iterations): the fused entries; every problem of both seeds accepts a base in its second iteration, under either
# entry (measured on MI355X: LSUM[0] = 1, 2, 2)
FUSED = [("sweep_seed_144", 3), ("sweep_seed_175", 3)]


@functools.lru_cache(maxsize=None)
def _operands(name):
    c = dict(SG._operands(name)[0])
    c["info"] = c["p"].gn_factor_info()
    c["tile"] = c["p"].gn_tile_info()
    return c


@pytest.mark.parametrize("name", CASES)
def test_directions_against_numpy(name):
    c = _operands(name)
    n, mu = c["n"], MU_OF.get(name, MU)
    assert c["B"] == B and c["held"].any() and (c["LAMP"] == 0).any()
    out = {}
    for kind, mod in KERNELS.items():
        D, SUM = mod._run(c, mu=mu, wrows=WROWS)
        out[kind] = (D.cpu().numpy(), SUM.cpu().numpy())
        assert np.isnan(out[kind][0][:, n:]).all() and np.isnan(out[kind][1][:, 8:]).all(), f"{name} {kind}: padding written"
    worst = {kind: [0.0, 0.0] for kind in KERNELS}
    for b in range(B):
        g, held = c["GR"][b], c["held"][b]
        ld, f64 = pivot_refs(c["P"], c["V"][b], c["LAMP"][b], c["rho"][b], g, mu, c["info"]["pos"], c["info"]["first"], held)
        codes = [f["code"] for f in f64]
        assert codes == [1, 1, 1] and ld["code"] == 1, f"{name} problem {b}: the references do not solve at mu = {mu:g}: {codes}, {ld['code']}"
        a = (c["P"], c["V"][b], c["LAMP"][b], c["rho"][b], g, mu, held)
        H = CH.system(*a[:4], mu)
        gate = 8 * max(CH.backward_error(*a, f["D"], H=H) for f in f64[:2])
        bb = float(np.sum(g[~held].astype(np.longdouble) ** 2))
        exact = {2: float(ld["pmin"]), 6: float(ld["pmax"])}
        pgate = {2: pivot_gate(n, exact[2], [f["pmin"] for f in f64]), 6: pivot_gate(n, exact[6], [f["pmax"] for f in f64])}
        assert 0 < exact[2] <= exact[6]
        for kind in KERNELS:
            tag = f"{name} {kind} problem {b}"
            Dh, S = out[kind][0][b, :n], out[kind][1][b]
            assert (S[0], S[4], S[5], S[7]) == (1.0, held.sum(), 1.0, -1.0), f"{tag}: solved / held / code / column {S[:8]}"
            assert np.array_equal(_np_bits(Dh[held]), _np_bits(g[held])), f"{tag}: held columns"
            assert S[3] > 0, f"{tag}: the slope sum g D = {S[3]}"
            err = CH.backward_error(*a, Dh, H=H)
            slope = float(np.sum(g.astype(np.longdouble) * Dh.astype(np.longdouble)))
            ratios = {k: abs(S[k] - exact[k]) / pgate[k] for k in (2, 6)}
            print(f"{tag}: backward error {err:.3e} gate {gate:.3e} ratio {err / gate:.3e}; pivots {S[2]:.17g} .. {S[6]:.17g}, long double "
                  f"{exact[2]:.17g} .. {exact[6]:.17g}, gates {pgate[2]:.3e} {pgate[6]:.3e}, ratios {ratios[2]:.3e} {ratios[6]:.3e}")
            assert err <= gate, f"{tag}: backward error {err:.3e} gate {gate:.3e}"
            assert abs(S[1] - bb) <= 8 * n * 2.0 ** -53 * bb, f"{tag}: bb {S[1]} against {bb}"
            assert abs(S[3] - slope) <= 8 * n * 2.0 ** -53 * float(np.sum(np.abs(g * Dh))), f"{tag}: the slope sum {S[3]} against {slope}"
            for k, what in ((2, "smallest"), (6, "largest")):
                assert ratios[k] <= 1, f"{tag}: the {what} pivot {S[k]:.17g} against {exact[k]:.17g}, gate {pgate[k]:.3e}"
            if exact[2] == mu:
                assert S[2] == mu, f"{tag}: the smallest pivot {S[2]:.17g} is not mu itself"
            worst[kind] = [max(worst[kind][0], err / gate), max(worst[kind][1], ratios[2], ratios[6])]
        (Dd, Sd), (Dt, St) = out["direct"], out["tiled"]
        assert np.array_equal(_np_bits(Dd[b, :n][held]), _np_bits(Dt[b, :n][held])), f"{name} problem {b}: the entries' held columns differ"
        assert np.array_equal(_np_bits(Sd[b, [0, 1, 4, 5, 7]]), _np_bits(St[b, [0, 1, 4, 5, 7]])), \
            f"{name} problem {b}: SUM[0, 1, 4, 5, 7] {Sd[b, :8]} (envelope) against {St[b, :8]} (tiled)"
    print(f"{name}: n {n}, explicit bounds {'XLd' in c}, held {c['held'].sum(axis=1).tolist()}; largest backward error / gate and pivot ratio: "
          + "; ".join(f"{kind} {w[0]:.3e} {w[1]:.3e}" for kind, w in worst.items()))


@pytest.mark.parametrize("seed", EDGE_SEEDS)
def test_pivots_leave_out_held_and_padding_columns(seed):
    """On the operands as they are the counted pivots run from mu = 1e-6 to about 1e8, so the 1.0 of a held or a padding
    column, counted by mistake, would change neither SUM[2] nor SUM[6]. Here it would. Problem 0 runs with rho = 1e-12:
    every counted pivot is below 1 and SUM[6] shows a counted 1.0. Problems 1 and 2 get XL = XU = X (a fixed column is
    held) on the columns of tests/test_chol_branches.hold_small_pivots, so every counted pivot is above 1 and SUM[2]
    shows it. The gates are test_directions_against_numpy's; that 1.0 lies outside them is asserted. Seeds 144 and 81
    have 15 and 1 padding columns, seed 180 none."""
    name = f"sweep_seed_{seed}"
    base = _operands(name)
    n, pos, first, P = base["n"], base["info"]["pos"], base["info"]["first"], base["P"]
    rho = base["rho"].copy()
    rho[0] = 1e-12
    lo, up, held = np.array(base["lo"]), np.array(base["up"]), base["held"].copy()
    for b in (1, 2):
        held[b] = hold_small_pivots(P, base["V"][b], base["LAMP"][b], rho[b], MU, held[b], pos)
        more = held[b] & ~base["held"][b]
        assert more.any() and not held[b].all(), f"{name} problem {b}: held {held[b].sum()} of {n}"
        lo[b, more] = up[b, more] = base["X"][b, more]
        assert np.array_equal(lbfgs_ref.held_mask(base["X"][b], base["GR"][b], lo[b], up[b]), held[b])
    c = dict(base, rho=rho, RHOd=_vec(rho), lo=lo, up=up, held=held, XLd=_padded(lo, n + 4), XUd=_padded(up, n + 4))
    refs = [pivot_refs(P, c["V"][b], c["LAMP"][b], rho[b], c["GR"][b], MU, pos, first, held[b]) for b in range(B)]
    for kind, mod in KERNELS.items():
        S = mod._run(c, wrows=WROWS)[1].cpu().numpy()
        for b, (ld, f64) in enumerate(refs):
            tag = f"{name} {kind} problem {b}"
            assert ld["code"] == 1 and all(f["code"] == 1 for f in f64), f"{tag}: the references do not solve"
            assert (S[b, 0], S[b, 4], S[b, 5], S[b, 7]) == (1.0, held[b].sum(), 1.0, -1.0), f"{tag}: {S[b, :8]}"
            k, key = (6, "pmax") if b == 0 else (2, "pmin")
            exact = float(ld[key])
            gate = pivot_gate(n, exact, [f[key] for f in f64])
            print(f"{tag}: held {held[b].sum()} of {n}; SUM[{k}] {S[b, k]:.17g}, long double {exact:.17g}, gate {gate:.3e}, "
                  f"ratio {abs(S[b, k] - exact) / gate:.3e}")
            assert (exact < 1.0 if b == 0 else exact > 1.0) and abs(1.0 - exact) > gate, f"{tag}: a counted 1.0 would not show"
            assert abs(S[b, k] - exact) <= gate, f"{tag}: SUM[{k}] {S[b, k]:.17g} against {exact:.17g}, gate {gate:.3e}"
            assert 0 < S[b, 2] <= S[b, 6]


@pytest.mark.parametrize("name", ISOLATION)
@pytest.mark.parametrize("kind", list(KERNELS))
def test_bits_and_isolation(kind, name):
    """tests/test_gpu_gn_direct.py / tests/test_gpu_gn_tiled.py's checks on the sweep's operands: the same bits for wrows in
    (1, 2, B), the reversed batch and a problem alone on another stream; a NaN in one problem's V; RUN."""
    KERNELS[kind].check_bits_and_isolation(_operands(name), WROWS)


@pytest.mark.parametrize("name", ISOLATION)
@pytest.mark.parametrize("kind", list(KERNELS))
def test_breakdown_and_nothing_to_solve(kind, name):
    """Those files' mu = 0 breakdown (code 2 at the first free permuted column, pivots 0) and code 3 (GR = +-0 on the free
    columns) on the sweep's operands."""
    c = _operands(name)
    if kind == "direct":
        DI.check_breakdown_and_nothing_to_solve(c, name, WROWS)
    else:
        TI.check_breakdown_and_nothing_to_solve(c, WROWS)


# ---- the fused entries ---------------------------------------------------------------------------------------------------
def check_fused(kind, name, p, lo, up, iters):
    """`iters` calls of the kind's fused iterate entry (iters=1) against the public calls in sequence
    (_pieces_iteration of the kind's file): every state array, DC and GSUM bit-identical after every iteration, at the
    automatic products chunk (wrows = 3) and at chunk 2 (a ragged last chunk, wrows = 2), a RHO row of distinct values,
    mu = 1e-2; iters=3 against three calls. An accepted base (LSUM[0] == 2) must occur, so that the select D <- DC runs."""
    import torch
    mod = KERNELS[kind]
    entry = p.alsolve_gn_direct_iterate if kind == "direct" else p.alsolve_gn_tiled_iterate
    ldw = (p.gn_factor_info() if kind == "direct" else p.gn_tile_info())["ldw_min"]
    n, mem = p.n, AL.FUSED_PAR["mem"]
    par = alsolve_params(**AL.FUSED_PAR)
    gn = gn_params(mu=1e-2)
    h0 = AL._start(p, lo, up, B, mem, 7300)

    def fresh():
        st = AL._state(p, B, mem, h0)
        p.alsolve_init(par, st)
        st.RHO.copy_(_vec(10.0 * (1.0 + 0.25 * np.arange(B))))
        return st, _nan(B, n + 3), _nan(B, 8 + 2)

    Gs, Vs = _nan(B, p.m + 1), _nan(B, p.nnz + 5)
    (ref, DCr, GSr), want, codes = fresh(), [], []
    Wr = _nan(B, ldw + 1)
    for k in range(iters):
        mod._pieces_iteration(p, par, gn, ref, DCr, GSr, Wr, Gs, Vs)
        want.append((ref.clone(), DCr.clone(), GSr.clone()))
        codes.append(ref.LSUM[:, 0].cpu().numpy().astype(int).tolist())
    print(f"{name} {kind}: LSUM[0] per iteration {codes}; direction codes at the end {GSr[:, 5].tolist()}")
    assert 2 in {c for row in codes for c in row}, "no accepted base: the select would show nothing"
    assert (GSr[:, 5] == 1).all() and np.isnan(GSr.cpu().numpy()[:, 8:]).all() and np.isnan(DCr.cpu().numpy()[:, n:]).all()
    try:
        for chunk, wrows in ((0, 3), (2, 2)):
            p.set_products_chunk(chunk)
            W = _nan(wrows, ldw + 2)
            st, DC, GS = fresh()
            for k in range(iters):
                entry(par, st, gn, DC, GS, W)
                torch.cuda.synchronize()
                what = f"{name} {kind} chunk {chunk} wrows {wrows} iteration {k}"
                AL._assert_same(st, want[k][0], what)
                assert _same_bits(DC, want[k][1]) and _same_bits(GS, want[k][2]), f"{what}: DC / GSUM"
            st, DC, GS = fresh()
            entry(par, st, gn, DC, GS, W, iters=3)
            torch.cuda.synchronize()
            AL._assert_same(st, want[2][0], f"{name} {kind} chunk {chunk} iters=3")
            assert _same_bits(DC, want[2][1]) and _same_bits(GS, want[2][2]), f"{name} {kind} chunk {chunk} iters=3: DC / GSUM"
            assert np.isnan(W.cpu().numpy()[:, ldw:]).all(), "the workspace's padding was written"
    finally:
        p.set_products_chunk(0)


@pytest.mark.parametrize("name,iters", FUSED)
@pytest.mark.parametrize("kind", list(KERNELS))
def test_fused_entries(kind, name, iters):
    """sweep_seed_144: one live row in the last tile; sweep_seed_175: empty constraint sets."""
    p, lo, up, _ = _problem(name)
    assert iters >= 3
    if name == "sweep_seed_175":
        assert AL.empty_sets(p), "seed 175 has no empty constraint set"
    check_fused(kind, name, p, lo, up, iters)
