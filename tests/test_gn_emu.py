"""The host walk of towr_gn_direction_kernel (tests/host_emu/emu.hip emu_gn_direction_ex, through tests/jp_emu.py) on the
CPU: against tests/gn_ref.py under the gate of tests/gn_gate.py, every stop code, and which branches of the kernel's two
passes the cases of this file and of tests/test_gpu_sweep_gn.py reach (computed from the product tables alone). The
device's bits are compared with this walk in tests/test_gpu_sweep_gn.py; here the walk itself is held to the reference,
so that the two cannot be wrong together unseen.

Operands, without a GPU: V of emu_eval_ex at x0 + 0.05 sigma, LAMP = standard normal with about a third of its entries
exactly zero (inactive rows), GR = J^T LAMP in numpy, rho = 10, mu = {1e-2, 1e-6} max diag(rho J^T W J), ncg in {1, 3, 8},
tol = 0; X = x0 with XL / XU drawn as in tests/test_gpu_sweep_consumers.py test_projected_step (a quarter of the columns
fixed, a quarter unbounded on either or both sides, the others in a box around a point near x).

Cases: the 13 CONSUMER_SEEDS of the sweep, monoped_procedural and two built shapes of tests/configs.py: many_short_rows
(1315 short row segments in one chunk: three trips per lane through the J p pass's reload path, which no formulation
reaches) and many_short_columns (1090 short column segments in one chunk: three trips in the J^T t pass)."""
import functools

import numpy as np
import pytest

from tests import gn_gate as GATE
from tests import gn_ref as G
from tests import jp_emu
from tests import lbfgs_ref
from tests.configs import config_descs, many_short_columns, many_short_rows
from tests.gpu_helpers import _np_bits
from tests.shape_sweep import make
from tests.test_gpu_sweep_consumers import CONSUMER_SEEDS
from towr2025_amd import TowrGpuProblem

LD = np.longdouble
CASES = [f"sweep_seed_{s}" for s in CONSUMER_SEEDS] + ["monoped_procedural", "many_short_rows", "many_short_columns"]
BUILT = {"many_short_rows": many_short_rows, "many_short_columns": many_short_columns}
GPU_ONLY_CASES = ["anymal_trot_2p4s", "anymal_stairs_gaitopt"]   # the other cases of tests/test_gpu_sweep_gn.py
STOP_CASES = ["sweep_seed_196", "sweep_seed_154", "monoped_procedural", "many_short_rows"]
MUS = (1e-2, 1e-6)
NCGS = (1, 3, 8)
RHO = 10.0


def desc_of(name):
    """(ProblemDesc, side data or None) of a case name."""
    if name.startswith("sweep_seed_"):
        return make(int(name[len("sweep_seed_"):]))[0].to_desc(), None
    if name in BUILT:
        return BUILT[name]()
    return config_descs()[name], None


def drawn_bounds(x, rng):
    """XL / XU around x as test_projected_step draws them."""
    n = x.size
    kind = rng.integers(0, 8, n)                # 0, 1: fixed; 2: no lower; 3: no upper; 4: neither; 5..7: a box
    half = 0.2 * rng.random(n) + 0.01
    mid = x + 0.1 * rng.standard_normal(n)
    lo = np.where(kind <= 1, mid, np.where((kind == 2) | (kind == 4), -1e20, mid - half))
    up = np.where(kind <= 1, mid, np.where((kind == 3) | (kind == 4), 1e20, mid + half))
    return lo, up


def synthetic_multipliers(P, V, rng):
    """LAMP with about a third of its entries exactly zero, GR = J^T LAMP, max diag(RHO J^T W J)."""
    lamp = rng.standard_normal(P.m) * (rng.random(P.m) >= 1 / 3)
    gr = np.bincount(P.col, weights=V * lamp[P.row], minlength=P.n)
    mu_base = float(np.max(RHO * np.bincount(P.col, weights=G.weights(lamp)[P.row] * V * V, minlength=P.n)))
    return lamp, gr, mu_base


@functools.lru_cache(maxsize=None)
def _case(name):
    desc, data = desc_of(name)
    p = TowrGpuProblem(desc, device=-1, data=data)
    n, m, nnz = p.sizes()
    rp, col = p.jac_csr()
    P = G.Pattern(rp, col, n)
    seed = sum(name.encode())
    rng = np.random.default_rng(8200 + seed)
    x = p.initial_x() + 0.05 * rng.standard_normal(n)
    _, V = jp_emu.evaluate(desc, x, m, nnz, data)
    assert np.isfinite(V).all()
    lamp, gr, mu_base = synthetic_multipliers(P, V, rng)
    lo, up = drawn_bounds(x, rng)
    held = lbfgs_ref.held_mask(x, gr, lo, up)
    assert mu_base > 0 and (lamp == 0).any() and (lamp != 0).any() and held.any() and not held.all(), f"{name}: the case shows nothing"
    return dict(desc=desc, data=data, n=n, m=m, nnz=nnz, P=P, x=x, V=V, LAMP=lamp, GR=gr, lo=lo, up=up, held=held, mu_base=mu_base)


def _walk(c, ncg, mu, tol, GR=None, LAMP=None, bounds=True):
    kw = dict(X=c["x"], XL=c["lo"], XU=c["up"]) if bounds else {}
    return jp_emu.gn_direction(c["desc"], c["V"], c["LAMP"] if LAMP is None else LAMP, c["GR"] if GR is None else GR, RHO, mu, tol,
                               ncg, data=c["data"], **kw)


def block_tree(terms, block):
    """The kernel's dot-product tree over per-column terms, in float64: lane l's partial over columns l, l + block, ...
    in order from 0.0, each wave's 64-lane __shfl_down tree (offsets 32..1, lane 0's value), the waves in order."""
    lane = np.zeros(block)
    for l in range(min(block, terms.size)):
        acc = np.float64(0.0)
        for v in terms[l::block]:
            acc = acc + v
        lane[l] = acc
    part = []
    for w in range(block // 64):
        v = lane[64 * w:64 * w + 64].copy()
        o = 32
        while o:
            v[:o] = v[:o] + v[o:2 * o]
            o >>= 1
        part.append(v[0])
    t = part[0]
    for w in range(1, len(part)):
        t = t + part[w]
    return np.float64(t)


@pytest.mark.parametrize("name", CASES)
def test_walk_against_reference(name):
    """Every (mu, ncg): steps, held count and stop code equal the reference's, the held columns of D carry g bit for
    bit, the free columns and bb, rr, slope lie within the gate; once with every column free (X null)."""
    c = _case(name)
    n, worst = c["n"], 0.0
    for mk in MUS:
        for ncg in NCGS:
            mu = mk * c["mu_base"]
            D, S = _walk(c, ncg, mu, 0.0)
            ld, f64 = GATE.refs(c["P"], c["V"], c["LAMP"], RHO, c["GR"], ncg, mu, 0.0, c["held"])
            tag = f"{name} mu={mk:g} ncg={ncg}"
            assert ld["steps"] == ncg and ld["code"] == 0, f"{tag}: the reference stopped early {ld['steps'], ld['code']}"
            worst = max(worst, GATE.check_values(tag, n, c["GR"], c["held"], D, S, ld, f64))
    mu = MUS[1] * c["mu_base"]
    D, S = _walk(c, 8, mu, 0.0, bounds=False)
    none = np.zeros(n, dtype=bool)
    ld, f64 = GATE.refs(c["P"], c["V"], c["LAMP"], RHO, c["GR"], 8, mu, 0.0, none)
    assert S[4] == 0 and ld["steps"] == 8
    worst = max(worst, GATE.check_values(f"{name} every column free", n, c["GR"], none, D, S, ld, f64))
    print(f"{name}: largest err / gate of the walk {worst:.3e}")


@pytest.mark.parametrize("name", STOP_CASES)
def test_stop_codes(name):
    c = _case(name)
    n, m, P, held = c["n"], c["m"], c["P"], c["held"]
    mu = MUS[0] * c["mu_base"]
    # code 1: tol between two consecutive rr / bb of the long double run; no decision is a tie
    hist = [float(v) for v in GATE.refs(P, c["V"], c["LAMP"], RHO, c["GR"], 8, mu, 0.0, held)[0]["hist"]]
    k = next(i for i in range(2, 8) if hist[i] < min(hist[:i]))
    tol = float(np.sqrt(np.sqrt(hist[k] * min(hist[:k]))))
    ld, f64 = GATE.refs(P, c["V"], c["LAMP"], RHO, c["GR"], 8, mu, tol, held)
    for r in [ld] + f64:
        assert min(abs(float(h) / (tol * tol) - 1.0) for h in r["hist"]) > 1e-6, f"{name}: a stop decision is a tie"
    assert (ld["steps"], ld["code"]) == (k, 1)
    D, S = _walk(c, 8, mu, tol)
    GATE.check_values(f"{name} tol={tol:.3e}", n, c["GR"], held, D, S, ld, f64)
    # code 2 from a NaN in GR on a free column: no step, D == GR bit for bit
    GRn = c["GR"].copy()
    GRn[int(np.flatnonzero(~held)[3])] = np.nan
    D, S = _walk(c, 8, mu, 0.0, GR=GRn)
    assert (S[0], S[5]) == (0.0, 2.0) and np.array_equal(_np_bits(D), _np_bits(GRn)), f"{name}: NaN in GR {S}"
    # code 2 without a NaN: no row active and mu = 0, pHp is exactly 0.0
    zero = np.zeros(m)
    D, S = _walk(c, 8, 0.0, 0.0, LAMP=zero)
    ld, f64 = GATE.refs(P, c["V"], zero, RHO, c["GR"], 8, 0.0, 0.0, held)
    assert (ld["steps"], ld["code"]) == (0, 2) and (S[0], S[5]) == (0.0, 2.0), f"{name}: pHp == 0 {S}"
    assert np.array_equal(_np_bits(D), _np_bits(c["GR"])) and _np_bits(S[1]) == _np_bits(S[2])
    GATE.check_values(f"{name} pHp == 0", n, c["GR"], held, D, S, ld, f64)
    # code 3: GR zero (some -0.0) on every free column, as it was on the held ones
    GR3 = zero_free_gradient(c["GR"], held, np.random.default_rng(5))
    assert np.array_equal(lbfgs_ref.held_mask(c["x"], GR3, c["lo"], c["up"]), held)
    D, S = _walk(c, 8, mu, 0.0, GR=GR3)
    assert np.array_equal(_np_bits(D), _np_bits(GR3)), f"{name}: bb == 0, D must be GR with its sign bits"
    block = jp_emu.tables(c["desc"], c["data"])["gn_block"]
    want = np.array([0.0, 0.0, 0.0, block_tree(GR3 * GR3, block), float(held.sum()), 3.0])
    assert np.array_equal(_np_bits(S), _np_bits(want)), f"{name}: bb == 0 {S} vs {want}"
    assert want[3] > 0


def zero_free_gradient(GR, held, rng):
    """GR with +0.0 or -0.0 (about half each) on the free columns."""
    z = np.where(rng.random(GR.size) < 0.5, -0.0, 0.0)
    out = np.where(held, GR, z)
    assert np.signbit(out[~held]).any() and not np.signbit(out[~held]).all() and (out[held] != 0).any()
    return out


# ---- which branches of the kernel's passes the cases reach ----------------------------------------------------------------
BRANCHES = ("nch=1", "nch=2", "nch>=3", "short>blk", "short>2blk", "long>waves", "carried row", "empty rows", "n<128", "n odd", "n>2blk")


def branches(t):
    """Per branch of towr_gn_direction_kernel, where a pattern's tables reach it: 'r' in the J p pass (row segments), 'c'
    in the J^T t pass (column segments), 'x' for a property of the pattern as a whole; '' when not reached."""
    blk, ch = t["gn_block"], t["chunks"]
    nch, n = ch.shape[0], t["n"]
    rc = lambda r, c: ("r" if r else "") + ("c" if c else "")
    x = lambda b: "x" if b else ""
    return {"nch=1": x(nch == 1), "nch=2": x(nch == 2), "nch>=3": x(nch >= 3),
            "short>blk": rc((ch[:, 1] > blk).any(), (ch[:, 4] > blk).any()),
            "short>2blk": rc((ch[:, 1] > 2 * blk).any(), (ch[:, 4] > 2 * blk).any()),
            "long>waves": rc((ch[:, 2] > blk // 64).any(), (ch[:, 5] > blk // 64).any()),
            "carried row": rc((t["rseg"][:, 3] & 1).any(), False), "empty rows": x(t["empty_rows"].size > 0),
            "n<128": x(n < 128), "n odd": x(n % 2 == 1), "n>2blk": x(n > 2 * blk)}


def test_branch_coverage():
    """Every branch is reached by some case, in both passes where it has two sides; the table is DESIGN 4k's."""
    table = {}
    for name in CASES + GPU_ONLY_CASES:
        desc, data = desc_of(name)
        t = jp_emu.tables(desc, data)
        table[name] = (t, branches(t))
    print(f"{'case':24s} {'n':>5s} {'m':>5s} {'nnz':>7s} {'nch':>4s} {'rns':>5s} {'rnl':>4s} {'cns':>4s} {'cnl':>4s} " + " ".join(f"{b:>11s}" for b in BRANCHES))
    for name, (t, br) in table.items():
        ch = t["chunks"]
        print(f"{name:24s} {t['n']:5d} {t['m']:5d} {t['nnz']:7d} {ch.shape[0]:4d} {ch[:, 1].max():5d} {ch[:, 2].max():4d} {ch[:, 4].max():4d} "
              f"{ch[:, 5].max():4d} " + " ".join(f"{br[b] or '-':>11s}" for b in BRANCHES))
    for b in BRANCHES:
        assert any(br[b] for _, br in table.values()), f"no case reaches {b}"
    for b in ("short>blk", "short>2blk", "long>waves"):
        for side in "rc":
            assert any(side in br[b] for _, br in table.values()), f"no case reaches {b} in pass {side}"
    t, br = table["many_short_rows"]
    assert t["chunks"][:, 1].max() > 2 * t["gn_block"] and "r" in br["short>2blk"]
    assert table["sweep_seed_154"][0]["chunks"].shape[0] == 1
    assert any(t["chunks"][:, 4].max() > t["gn_block"] for t, _ in table.values())
    t, br = table["many_short_columns"]
    assert t["chunks"][:, 4].max() > 2 * t["gn_block"] and "c" in br["short>2blk"]
    # by this table only the two built shapes walk a second row trip: "always cur.s" in gn_jp_pass can show on no other
    assert [name for name, (_, br) in table.items() if "r" in br["short>blk"]] == ["many_short_rows", "many_short_columns"]
