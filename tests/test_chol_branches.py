"""Which branches of towr_gn_tiled_kernel and towr_gn_direct_kernel (towr2025_amd/csrc/jprod.hip) the cases of
tests/test_gpu_sweep_chol.py reach, computed from towr_gpu_gn_factor_info / towr_gpu_gn_tile_info on layout-only handles
and asserted here (the table is DESIGN 4n's); and, on synthetic operands on the three shapes with 1, 15 and 0 live rows
in the last tile, the power of the two gates the device tests use: the backward-error gate refuses two wrong systems, the
pivot gate refuses a smallest pivot that counts the held columns. No GPU.

What decides a branch of the tiled kernel is the tile table, not the problem's size: cnt[J] is the number of block rows
I > J whose first stored tile bfirst[I] is <= J (the kernel's tcol_ptr differences, gn_tile_tables in auglag.hip), and
a pair (I, J), I > J, is "mixed" when bfirst[J] < bfirst[I] < J: its tile product starts at K = bfirst[I], not bfirst[J].

Synthetic operands: V standard normal, LAMP / GR of tests/test_gn_emu.synthetic_multipliers, rho = 10, mu = 1e-6, a
tenth of the columns held (drawn)."""
import functools

import numpy as np
import pytest

from tests import chol_ref as CH
from tests import gn_ref as G
from tests import jp_emu
from tests import tile_chol_ref as TC
from tests.test_chol_ref import _gate, _layout_handle
from tests.test_gn_emu import desc_of, synthetic_multipliers
from tests.test_gpu_sweep_consumers import CONSUMER_SEEDS
from towr2025_amd import _capi as capi

EDGE_SEEDS = (144, 81, 180)   # n % 16 = 1, 15, 0 (the last with fewer block rows than the kernel has waves)
CASES = [f"sweep_seed_{s}" for s in EDGE_SEEDS + tuple(CONSUMER_SEEDS)]
RHO, MU = 10.0, 1e-6
TILED = ("n%16=1", "n%16=15", "n%16=0", "nt<waves", "cnt<=7", "cnt 8..14", "cnt>14", "16cnt>blk", "inner cnt=0", "mixed>0", "mixed=0",
         "lone row")
ENVELOPE = ("n<blk", "n>2blk", "width>blk", "env%blk!=0")
PROPERTIES = TILED + ENVELOPE


def pivot_gate(n, exact, f64):
    """The gate of a pivot extreme (SUM[2], SUM[6]): 8 x the largest distance of the float64 references' values `f64` from
    the long double value `exact`, and at least n 2^-53 |exact| (where every reference agrees exactly, the device's
    sum of MFMA products is not held to bit equality)."""
    exact = float(exact)
    return max(8 * max(abs(float(v) - exact) for v in f64), n * 2.0 ** -53 * abs(exact))


def pivot_refs(P, V, lamp, rho, g, mu, pos, first, held):
    """(the long double tiled reference, [chol_ref forward, chol_ref reversed, tile_chol_ref] in float64)."""
    a = (P, V, lamp, rho, g, mu, pos, first)
    ld = TC.direction(*a, held=held, dtype=np.longdouble)
    return ld, [CH.direction(*a, held=held, reverse=False), CH.direction(*a, held=held, reverse=True), TC.direction(*a, held=held)]


def hold_small_pivots(P, V, lamp, rho, mu, held, pos, bar=4.0):
    """`held` enlarged until every free column's pivot is >= bar: the columns whose pivot in a dense right-looking
    factorisation of the permuted H (float64) is below `bar` are held as well, and again on the new H. Holding a column
    takes its elimination out of every later pivot, which only raises them, so the loop ends. A held column's pivot, like a
    padding column's, is 1.0: with every counted pivot above 1 an entry that counted one of them shows in SUM[2]."""
    inv = np.argsort(np.asarray(pos, dtype=np.int64))
    held = np.array(held, dtype=bool)
    for _ in range(P.n + 1):
        A = assemble_permuted(P, V, lamp, rho, mu, held, inv)
        piv = np.zeros(P.n)
        for k in range(P.n):
            piv[k] = A[k, k]
            if not piv[k] > 0:      # (taken as small: the column is held in the next round)
                piv[k] = 0.0
                A[k + 1:, k] = 0.0
            A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k + 1:, k]) / max(piv[k], np.finfo(float).tiny)
        small = np.zeros(P.n, dtype=bool)
        small[inv] = piv < bar
        small &= ~held
        if not small.any():
            return held
        held |= small
    raise AssertionError("unreachable: every round holds at least one more column")


def assemble_permuted(P, V, lamp, rho, mu, held, inv):
    """chol_ref.assemble's H (float64) by permuted position, symmetric."""
    return CH.assemble(P, V, lamp, rho, mu, held)[np.ix_(inv, inv)].copy()


@functools.lru_cache(maxsize=None)
def _blocks():
    """(kGnBlock, kGnWaves, kGnTile) from where the Python side exposes them."""
    blk = jp_emu.tables(*desc_of("sweep_seed_196"))["gn_block"]
    return blk, blk // 64, capi.GN_TILE


@functools.lru_cache(maxsize=None)
def tile_stats(name):
    """The tables' figures of a case: n, nt, tiles, cnt (nt), mixed, lone (block rows I > 0 of one tile), env, width."""
    h = _layout_handle(name)
    f, t = h.gn_factor_info(), h.gn_tile_info()
    nt, bf = t["nt"], t["bfirst"].astype(np.int64)
    assert t["tile"] == _blocks()[2] and nt == -(-h.n // t["tile"])
    I = np.arange(nt)
    reach = (I[:, None] > I[None, :]) & (bf[:, None] <= I[None, :])          # (I, J): block row I reaches block column J
    mixed = reach & (bf[None, :] < bf[:, None]) & (bf[:, None] < I[None, :])
    return dict(n=h.n, nt=nt, tiles=t["tiles"], cnt=reach.sum(axis=0), mixed=int(mixed.sum()), lone=int((bf[1:] == I[1:]).sum()),
                env=f["envelope"], width=f["bandwidth"])


def branches(s):
    blk, waves, tile = _blocks()
    cmax = int(s["cnt"].max())
    return {"n%16=1": s["n"] % tile == 1, "n%16=15": s["n"] % tile == tile - 1, "n%16=0": s["n"] % tile == 0,
            "nt<waves": s["nt"] < waves, "cnt<=7": cmax <= waves - 1, "cnt 8..14": waves - 1 < cmax <= 2 * (waves - 1),
            "cnt>14": cmax > 2 * (waves - 1), "16cnt>blk": tile * cmax > blk, "inner cnt=0": bool((s["cnt"][:-1] == 0).any()),
            "mixed>0": s["mixed"] > 0, "mixed=0": s["mixed"] == 0, "lone row": s["lone"] > 0,
            "n<blk": s["n"] < blk, "n>2blk": s["n"] > 2 * blk, "width>blk": s["width"] > blk, "env%blk!=0": s["env"] % blk != 0}


def test_branch_coverage():
    """Every property is reached by some case of tests/test_gpu_sweep_chol.py; the printed table is DESIGN 4n's."""
    blk, waves, tile = _blocks()
    assert (blk, waves, tile) == (512, 8, 16), "the kernels' block changed: reread the properties against jprod.hip"
    table = {name: (tile_stats(name), branches(tile_stats(name))) for name in CASES}
    print(f"{'case':15s} {'n':>5s} {'n%16':>4s} {'nt':>3s} {'tiles':>5s} {'cnt':>3s} {'cnt=0':>5s} {'mixed':>5s} {'lone':>4s} {'env':>7s} "
          f"{'width':>5s}  " + " ".join(PROPERTIES))
    for name, (s, br) in table.items():
        print(f"{name:15s} {s['n']:5d} {s['n'] % tile:4d} {s['nt']:3d} {s['tiles']:5d} {s['cnt'].max():3d} {(s['cnt'] == 0).sum():5d} "
              f"{s['mixed']:5d} {s['lone']:4d} {s['env']:7d} {s['width']:5d}  " + " ".join(f"{'x' if br[p] else '-':>{len(p)}s}" for p in PROPERTIES))
    for prop in PROPERTIES:
        assert any(br[prop] for _, br in table.values()), f"no case reaches {prop}"
    # the three shapes the list was extended by, as the issue's table has them: one, fifteen and no live row in the last
    # tile's padding, the last with fewer block rows than waves
    want = {"sweep_seed_144": (145, 10, 44, 7, 2, 5), "sweep_seed_81": (95, 6, 16, 4, 2, 0), "sweep_seed_180": (96, 6, 21, 5, 1, 0)}
    for name, w in want.items():
        s = table[name][0]
        assert (s["n"], s["nt"], s["tiles"], int(s["cnt"].max()), int((s["cnt"] == 0).sum()), s["mixed"]) == w, (name, s)
    assert table["sweep_seed_180"][1]["n%16=0"] and table["sweep_seed_180"][1]["nt<waves"]
    assert [n for n, (_, br) in table.items() if br["n%16=1"]] == ["sweep_seed_144"]
    assert [n for n, (_, br) in table.items() if br["n%16=15"]] == ["sweep_seed_81"]


# ---- the gates' power on the three edge shapes ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _synthetic(seed):
    h = _layout_handle(f"sweep_seed_{seed}")
    n = h.n
    rp, col = h.jac_csr()
    P = G.Pattern(rp, col, n)
    rng = np.random.default_rng(9300 + seed)
    V = rng.standard_normal(h.nnz)
    lamp, g, _ = synthetic_multipliers(P, V, rng)
    held = rng.random(n) < 0.1
    info = h.gn_factor_info()
    assert held.any() and not held.all() and (lamp == 0).any()
    return dict(P=P, V=V, lamp=lamp, g=g, held=held, pos=info["pos"], first=info["first"], n=n)


@pytest.mark.parametrize("seed", EDGE_SEEDS)
def test_backward_error_gate_refuses_a_wrong_system(seed):
    """tests/test_tile_chol_ref.py test_direction_solves_the_dense_system's assertion with 1, 15 and 0 live rows in the
    last tile: the three float64 references solve (code 1), the tiled one lies inside the gate, and the directions of the
    two wrong systems (every row active; no column held) lie more than 1000 gates outside it."""
    c = _synthetic(seed)
    a = (c["P"], c["V"], c["lamp"], RHO, c["g"], MU)
    gate = _gate(*a, c["held"], c["pos"], c["first"])          # (asserts code 1 of both orders of chol_ref)
    H = CH.system(*a[:4], MU)
    d = TC.direction(*a, c["pos"], c["first"], held=c["held"])
    assert d["code"] == 1 and d["nheld"] == c["held"].sum()
    err = CH.backward_error(*a, c["held"], d["D"], H=H)
    assert err <= gate, (err, gate)
    for kw in (dict(ignore_w=True), dict(ignore_held=True)):
        other = TC.direction(*a, c["pos"], c["first"], held=c["held"], **kw)
        assert other["code"] == 1
        far = CH.backward_error(*a, c["held"], other["D"], H=H)
        print(f"seed {seed} {kw}: backward error {far:.3e}, gate {gate:.3e}, ratio {far / gate:.3e}")
        assert far > 1000 * gate, (kw, far, gate)


def test_pivot_gate_refuses_the_held_columns():
    """Seed 144. A held column's pivot is 1.0 (its row and column are the identity's). On the operands as drawn the
    smallest counted pivot is mu itself (a free column without an active entry), far below 1.0, so counting the held
    columns would show nothing in SUM[2]. The held set is therefore chosen: every column whose pivot, with nothing held,
    is below 4 is held as well. Then every counted pivot of the references lies above 1, the smallest pivot over all
    columns is the held columns' 1.0, and it differs from the counted one by more than the gate."""
    c = _synthetic(144)
    n, pos, first = c["n"], c["pos"], c["first"]
    a = (c["P"], c["V"], c["lamp"], RHO, c["g"], MU, pos, first)
    ld0, _ = pivot_refs(*a, c["held"])
    assert ld0["pmin"] == MU, "the drawn operands: a free column without an active entry has the pivot mu exactly"
    inv = np.argsort(pos)
    _, bfirst, _ = TC.tile_tables(first, n)

    held = hold_small_pivots(c["P"], c["V"], c["lamp"], RHO, MU, c["held"], pos)
    assert not held.all() and held.sum() > c["held"].sum()
    ld, f64 = pivot_refs(*a, held)
    assert ld["code"] == 1 and all(f["code"] == 1 for f in f64)
    gate = pivot_gate(n, ld["pmin"], [f["pmin"] for f in f64])
    # the tiled reference with no column excluded from the count (the padding's pivots stay uncounted)
    every = TC.factor_solve(assemble_permuted(c["P"], c["V"], c["lamp"], RHO, MU, held, inv), c["g"][inv], bfirst,
                            np.zeros(n, dtype=bool))["pmin"]
    print(f"seed 144: held {held.sum()} of {n}; counted pmin {float(ld['pmin']):.6e}, over all columns {every:.6e}, gate {gate:.3e}")
    assert every == 1.0 and float(ld["pmin"]) > 1.0
    assert abs(every - float(ld["pmin"])) > gate
    assert all(abs(f["pmin"] - float(ld["pmin"])) <= gate for f in f64)
