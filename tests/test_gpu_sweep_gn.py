"""towr_gn_direction_kernel and the resident AL loop (line search, outer update, select, the two fused iterate entries) on
shapes of the seeded sweep (tests/shape_sweep.py) and on tests/configs.py many_short_rows / many_short_columns, instead of the three Jacobian
patterns of tests/test_gpu_gn.py / tests/test_gpu_alsolve.py. Which branch of the kernel's two passes each case reaches
is computed and asserted on the CPU (tests/test_gn_emu.py test_branch_coverage). B = 3, padded leading
dimensions with NaN padding, NaN-filled outputs.

Two comparisons. (1) Bit for bit with the host walk of the kernel (tests/host_emu/emu.hip emu_gn_direction_ex) fed the
device's own V, LAMP, GR, X and the bounds used: DESIGN 4k promises that every J p / J^T t element is the product
kernels' tree and every dot product one fixed tree, and the walk is those trees. A stale prefetched segment, a wrong carry
parity or another wave order moves D by a few ulps of a small column, far inside any gate scaled by max |D|. (2) The gate
of tests/gn_gate.py against the long double reference of tests/gn_ref.py, which holds the walk and the kernel to the
formulas (the walk alone is held to it on the CPU, tests/test_gn_emu.py). No tolerance of its own anywhere."""
import functools

import numpy as np
import pytest

from tests import gn_gate as GATE
from tests import jp_emu
from tests import test_gn_emu as E
from tests import test_gpu_alsolve as AL
from tests import test_gpu_gn as GN
from tests.configs import config_descs
from tests.gpu_helpers import _nan, _np_bits, _padded, _vec
from tests.test_gpu_lbfgs import _problem
from tests.test_gpu_sweep_consumers import CONSUMER_SEEDS
from towr2025_amd import TowrGpuProblem, gn_params

pytestmark = pytest.mark.gpu

B = 3
CASES = [f"sweep_seed_{s}" for s in CONSUMER_SEEDS] + ["many_short_rows", "many_short_columns"]
FUSED_SEEDS = [154, 13, 175]   # one chunk of entries; the record path with tile-path fallbacks; empty constraint sets
GN_ITERS = 4        # every seed accepts a base in its second iteration (measured: codes 1, 2, 2, 2)
LBFGS_ITERS = 10    # the L-BFGS loop's first direction is steepest descent: 5 or 6 shrinks, a base accepted from the 7th or 8th on


def _redraw(seed):
    def draw(X):
        rng = np.random.default_rng(53 + seed)
        lo, up = zip(*(E.drawn_bounds(x, rng) for x in X))
        return np.stack(lo), np.stack(up)
    return draw


@functools.lru_cache(maxsize=None)
def _operands(name):
    """tests/test_gpu_gn.py's operands on the case's handle; (the description, its side data) for the host walk."""
    if name not in E.BUILT:
        p, lo, up, _ = _problem(name)
        c = GN.build_operands(p, lo, up, B, redraw=_redraw(int(name[len("sweep_seed_"):])))
        return c, (p.desc, None)
    # the handle is created with its matrix; it has no bounds data: LAMP and GR are synthetic (tests/test_gn_emu.py),
    # on the device's own V, and XL / XU are drawn
    import torch
    desc, data = E.desc_of(name)
    p = TowrGpuProblem(desc, device=0, data=data)
    n, m, nnz = p.n, p.m, p.nnz
    rng = np.random.default_rng(8100 + B)
    X = p.initial_x() + 0.05 * rng.standard_normal((B, n))
    Xd, Gd, Vd = _padded(X, n + 1), _nan(B, m + 2), _nan(B, nnz + 3)
    p.eval_batch_device(Xd, Gd, Vd)
    torch.cuda.synchronize()
    V = Vd.cpu().numpy()[:, :nnz]
    rp, col = p.jac_csr()
    P = GN.G.Pattern(rp, col, n)
    LAMP, GR = (np.stack(a) for a in zip(*(E.synthetic_multipliers(P, V[b], rng)[:2] for b in range(B))))
    lo, up = _redraw(0)(X)
    rho = 10.0 * (1.0 + np.arange(B))
    c = GN.finish_operands(p, lo, up, B, X, V, LAMP, GR, rho, Xd, Vd, _padded(LAMP, m + 4), _padded(GR, n + 7))
    c.update(XLd=_padded(lo, n + 4), XUd=_padded(up, n + 4))
    return c, (desc, data)


def _walk(c, src, b, gn, GR=None, LAMP=None):
    """The host walk of problem b on the device's operands."""
    desc, data = src
    return jp_emu.gn_direction(desc, c["V"][b], c["LAMP"][b] if LAMP is None else LAMP, c["GR"][b] if GR is None else GR, c["rho"][b],
                               gn.mu, gn.tol, gn.ncg, X=c["X"][b], XL=c["lo"][b], XU=c["up"][b], data=data)


def _assert_bits(tag, c, src, gn, Dh, S, rows=None):
    n = c["n"]
    assert np.isnan(Dh[:, n:]).all() and np.isnan(S[:, 6:]).all(), f"{tag}: padding written"
    for b in range(c["B"]) if rows is None else rows:
        Dw, Sw = _walk(c, src, b, gn)
        bad = np.flatnonzero(_np_bits(Dh[b, :n]) != _np_bits(Dw))
        assert bad.size == 0, (f"{tag} problem {b}: D is not the walk's tree in {bad.size} columns, first {bad[:5]}: "
                               f"{Dh[b, bad[:5]]} vs {Dw[bad[:5]]}")
        assert np.array_equal(_np_bits(S[b, :6]), _np_bits(Sw)), f"{tag} problem {b}: SUM {S[b, :6]} vs the walk's {Sw}"


@pytest.mark.parametrize("name", CASES)
def test_direction_bits_and_gate(name):
    """Every (mu, ncg): D and SUM bit for bit the host walk's, then within the gate of the long double reference."""
    c, src = _operands(name)
    n = c["n"]
    assert c["held"].any() and (c["LAMP"] == 0).any() and c["mu_base"] > 0
    worst = 0.0
    for mk, ncg in GN.COMBOS:
        mu = mk * c["mu_base"]
        gn = gn_params(ncg=ncg, mu=mu, tol=0.0)
        refs = [GN._refs(c, b, ncg, mu, 0.0) for b in range(B)]
        for b, (ld, _) in enumerate(refs):
            assert ld["steps"] == ncg and ld["code"] == 0, f"{name} mu={mk:g} ncg={ncg} problem {b}: the reference stopped early"
        D, SUM = GN._run(c, gn)
        Dh, S = D.cpu().numpy(), SUM.cpu().numpy()
        tag = f"{name} mu={mk:g} ncg={ncg}"
        _assert_bits(tag, c, src, gn, Dh, S)
        for b, (ld, f64) in enumerate(refs):
            worst = max(worst, GN._check_problem(f"{tag} problem {b}", c, b, Dh[b], S[b], ld, f64))
    print(f"{name}: explicit bounds {'XLd' in c}; held {c['held'].sum(axis=1).tolist()}; largest err / gate {worst:.3e}")


@pytest.mark.parametrize("name,nb", [c for c in GN.CASES if c[1] > 1])
def test_existing_cases_bits(name, nb):
    """The three patterns of tests/test_gpu_gn.py at ncg = 8: bit for bit the host walk's on every problem
    (anymal_stairs_gaitopt has more than kGnBlock short column segments in a chunk)."""
    c = GN._operands(name, nb)
    gn = gn_params(ncg=8, mu=GN.MUS[1] * c["mu_base"], tol=0.0)
    D, SUM = GN._run(c, gn)
    _assert_bits(f"{name} B={nb}", c, (config_descs()[name], None), gn, D.cpu().numpy(), SUM.cpu().numpy())


@pytest.mark.parametrize("name", ["sweep_seed_196", "anymal_trot_2p4s"])
def test_stop_codes_on_the_device(name):
    """Stop code 3 (bb == 0: GR zero, some -0.0, on every free column) and stop code 2 without a NaN (no active row and
    mu = 0: pHp == 0.0) in problem 1 of a B = 3 batch: exact SUM, D == GR with its sign bits; the other problems' bits
    are those of the batch without it."""
    import torch
    if name.startswith("sweep_seed_"):
        c, src = _operands(name)
    else:
        c, src = GN._operands(name, B), (config_descs()[name], None)
    n, m, bad = c["n"], c["m"], 1
    others = [b for b in range(B) if b != bad]
    blk = jp_emu.tables(*src)["gn_block"]
    held = c["held"][bad]
    GR3 = E.zero_free_gradient(c["GR"][bad], held, np.random.default_rng(5))
    assert np.array_equal(GN.lbfgs_ref.held_mask(c["X"][bad], GR3, c["lo"][bad], c["up"][bad]), held)
    GRd3 = c["GRd"].clone()
    GRd3[bad, :n] = _vec(GR3)
    LPd2 = c["LPd"].clone()
    LPd2[bad, :m] = 0.0
    cases = (("code 3", gn_params(ncg=8, mu=GN.MUS[0] * c["mu_base"], tol=0.0), dict(GR=GRd3), dict(GR=GR3), 3.0, GR3),
             ("code 2", gn_params(ncg=8, mu=0.0, tol=0.0), dict(LAMP=LPd2), dict(LAMP=np.zeros(m)), 2.0, c["GR"][bad]))
    for what, gn, dev_kw, walk_kw, code, g in cases:
        D0, S0 = GN._run(c, gn)
        assert (S0[:, 0] == 8).all() and (S0[:, 5] == 0).all(), f"{name} {what}: the plain batch does not run normally {S0[:, :6].tolist()}"
        D1, S1 = GN._run(c, gn, **dev_kw)
        Dh, S = D1.cpu().numpy(), S1.cpu().numpy()
        assert np.isnan(Dh[:, n:]).all() and np.isnan(S[:, 6:]).all()
        Dw, Sw = _walk(c, src, bad, gn, **walk_kw)
        assert (Sw[0], Sw[5]) == (0.0, code)
        assert np.array_equal(_np_bits(S[bad, :6]), _np_bits(Sw)), f"{name} {what}: SUM {S[bad, :6]} vs {Sw}"
        assert np.array_equal(_np_bits(Dh[bad, :n]), _np_bits(g)), f"{name} {what}: D must be GR with its sign bits"
        if code == 3.0:
            want = np.array([0.0, 0.0, 0.0, E.block_tree(GR3 * GR3, blk), float(held.sum()), 3.0])
            assert np.array_equal(_np_bits(S[bad, :6]), _np_bits(want)) and want[3] > 0, f"{name} {what}: SUM {S[bad, :6]} vs {want}"
        else:
            assert _np_bits(S[bad, 1]) == _np_bits(S[bad, 2]) and S[bad, 1] > 0 and S[bad, 4] == held.sum()
        idx = torch.tensor(others, device=D0.device)
        assert GN._same_bits(D1[idx], D0[idx]) and GN._same_bits(S1[idx], S0[idx]), f"{name} {what} reached another problem"
        _assert_bits(f"{name} {what}", c, src, gn, Dh, S, rows=others)


# ---- the loop's kernels on sweep shapes -------------------------------------------------------------------------------
LOOP_SEEDS = [196, 93, 175, 126]   # n = 78; n = 1173 (odd); empty constraint sets (4 and 3 of them)


@pytest.mark.parametrize("seed", LOOP_SEEDS)
def test_linesearch_and_outer(seed):
    """tests/test_gpu_alsolve.py's line-search and outer-update checks at B = 9: every branch kind of the line search in
    one round, RSUM's length that of the seed's constraint sets."""
    name = f"sweep_seed_{seed}"
    if seed in (175, 126):
        assert AL.empty_sets(_problem(name)[0]), f"seed {seed} has no empty constraint set"
    AL.check_linesearch(name, 9)
    AL.check_outer(name, 9)


@pytest.mark.parametrize("seed", FUSED_SEEDS)
def test_fused_gn_iterate(seed):
    """alsolve_gn_iterate against the public calls in sequence (tests/test_gpu_gn.py check_fused): every state array, DC
    and GSUM bit-identical after every iteration, chunks 0 and 2, distinct RHO; an accepted base occurs, so the select
    D <- DC runs; an empty set's maximum stays +0.0 through the loop's residual call."""
    p, lo, up, _ = _problem(f"sweep_seed_{seed}")
    if seed == 175:
        assert AL.empty_sets(p)
    GN.check_fused(f"sweep_seed_{seed}", p, lo, up, B, GN_ITERS, {1, 2})


@pytest.mark.parametrize("seed", FUSED_SEEDS)
def test_fused_lbfgs_iterate(seed):
    """alsolve_iterate against the public calls in sequence (tests/test_gpu_alsolve.py check_fused) on the same seeds,
    LBFGS_ITERS iterations so that a restart, shrinks and accepted bases occur and a pair is used."""
    p, lo, up, _ = _problem(f"sweep_seed_{seed}")
    AL.check_fused(f"sweep_seed_{seed}", p, lo, up, B, LBFGS_ITERS, {1, 2, 3})
