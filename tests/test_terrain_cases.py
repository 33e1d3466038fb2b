"""What tests/test_gpu_terrain_batch.py runs is worth its GPU time only while these hold (CPU, layout-only handles, the
oracle and the test-only host emulation): the cases of tests/terrain_cases.py hold every terrain-reading launch; mixed
terrain ids in one batch are legitimate (the pattern does not depend on a non-curved terrain); reading any other
terrain of the batch, or only another friction coefficient, would be refused by the gate on the rows of every
basis-only constraint set, for every problem; every piece of ter_h / ter_dh is reached; and the host emulation of the
kernels' item loop equals the oracle at every point the GPU file evaluates, tie points included.
No tolerance of its own: tests/parity.py's gate, bit equality and NaN pre-fill. DESIGN.md 7e has the table."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import bounds_ref as R
from tests import terrain_cases as TC
from tests.shape_sweep import make
from towr2025_amd import TowrGpuProblem, _capi as capi
from towr2025_amd import formulation as F

HERE = os.path.dirname(os.path.abspath(__file__))
D = C.POINTER(C.c_double)
H = F.HeightMap
DYN, ROM, FDISC, TQDISC = 0, 1, 2, 3   # launch classes of TowrGpuProblem.kernel_path


@pytest.fixture(scope="module")
def emu():
    lib = os.path.join(HERE, "host_emu", "build", "libemu.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "host_emu")])
    L = C.CDLL(lib)
    L.emu_eval.argtypes = [C.POINTER(capi.ProblemDesc), D, D, D, C.c_char_p, C.c_int]
    return L


def test_cases_hold_every_terrain_reading_launch():
    """Each case is here for a reason, asserted from make(seed)'s info, constraint_info and kernel_path; every case has
    the TerrainConstraint rows the foot positions are read through, and every height reader and basis-only set is in
    some case on the tile path and on the record + compose path."""
    def shape(seed):
        cs, info = TC.get(seed), make(seed)[1]
        return cs, info, [cs.p.kernel_path(k) for k in (DYN, ROM, FDISC, TQDISC)]
    cs, info, pt = shape(154)
    assert info["n_ee"] == 1 and not info["optimize"] and capi.C_FORCE_DISCRETIZED in cs.kinds and pt[FDISC] == 0
    cs, info, pt = shape(16)
    assert info["n_ee"] == 2 and not info["optimize"] and {capi.C_FORCE, capi.C_TORQUE_DISCRETIZED, capi.C_TERRAIN_HARD} <= cs.kinds
    assert pt[TQDISC] == 0 and pt[FDISC] == -1
    cs, info, pt = shape(191)
    assert info["n_ee"] == 1 and info["optimize"] and info["rotvec"] and pt[FDISC] == 1 and pt[TQDISC] == 1
    assert {capi.C_FORCE_DISCRETIZED, capi.C_TORQUE_DISCRETIZED, capi.C_TERRAIN_HARD} <= cs.kinds
    cs, info, pt = shape(74)
    assert info["n_ee"] == 1 and info["optimize"] and {capi.C_FORCE, capi.C_TORQUE} <= cs.kinds and pt[FDISC] == -1 and pt[TQDISC] == -1
    cs, info, pt = shape(0)
    assert info["n_ee"] == 4 and info["optimize"] and pt[FDISC] == 1 and pt[TQDISC] == 1
    assert {capi.C_FORCE_DISCRETIZED, capi.C_TORQUE_DISCRETIZED} <= cs.kinds
    gap = TC.get(TC.GAP)
    assert gap.gap and not gap.desc.optimize_timings and {capi.C_FORCE_DISCRETIZED, capi.C_TORQUE_DISCRETIZED} <= gap.kinds
    assert gap.p.kernel_path(FDISC) == 0 and gap.p.kernel_path(TQDISC) == 0
    assert TC.SMALLEST == min(TC.SEEDS, key=lambda s: TC.get(s).nnz)
    assert set(TC.GAIT_SEEDS) == {s for s in TC.SEEDS if TC.get(s).desc.optimize_timings}
    for case in TC.CASES:
        cs = TC.get(case)
        assert capi.C_TERRAIN in cs.kinds and capi.C_BASE_HEIGHT in cs.kinds and cs.kinds & set(TC.BASIS_ONLY), case
        assert sorted(cs.foot_cols) == list(range(cs.desc.robot.n_ee)) and all(len(v) for v in cs.stance_cols.values()), case
    kinds = set().union(*(TC.get(s).kinds for s in TC.SEEDS))
    assert set(TC.BASIS_ONLY) | set(TC.HEIGHT_READERS) <= kinds


def test_pieces_restate_the_height_map():
    """pieces() with piece_height / piece_deriv is formulation.HeightMap.GetHeight and bounds_ref.height_deriv bit for
    bit, on drawn terrains of every id at drawn points and at every tie point; every name is in PIECES."""
    rng = np.random.default_rng(20261021)
    for rep in range(20):
        for t in TC.one_of_each(rng) + TC.gap_terrains(1, rng):
            xs = list(rng.uniform(-0.5, 2.5, 40)) + [v for _, v in TC.tie_points(t)]
            for x in xs:
                y = float(rng.uniform(-0.5, 0.5))
                ph, pd = TC.pieces(t, x, y)
                assert ph in TC.PIECES[t.id]["h"] and pd in TC.PIECES[t.id]["dh"], (TC.NAMES[t.id], ph, pd)
                h = np.array([TC.piece_height(t, ph, x, y), t.GetHeight(x, y)])
                assert h.view(np.uint64)[0] == h.view(np.uint64)[1], (TC.NAMES[t.id], ph, x, y, h)
                for dim in (0, 1):
                    d = np.array([TC.piece_deriv(t, pd, dim, x, y), R.height_deriv(t.to_c(), dim, x, y)])
                    assert d.view(np.uint64)[0] == d.view(np.uint64)[1], (TC.NAMES[t.id], pd, dim, x, y, d)
    for t in TC.one_of_each(rng):   # the drawn terrains differ from the member defaults in every parameter that is read
        used = {H.FlatID: 1, H.BlockID: 4, H.StairsID: 5, H.SlopeID: 4, H.ChimneyID: 4, H.ChimneyLRID: 4, H.StepsID: 3}[t.id]
        assert all(a != b for a, b in zip(t.params[:used], H.MakeTerrain(t.id).params[:used])) and TC.MU_RANGE[0] <= t.friction_coeff <= TC.MU_RANGE[1]
    t = TC._draw(H.StepsID, rng)
    assert len(TC.tie_points(t)) == 3 * (int(t.params[3]) + 2)


@pytest.mark.parametrize("case", TC.SEEDS)
def test_pattern_does_not_depend_on_the_terrain(case):
    """For every non-Gap id with drawn parameters the layout-only handle of desc.terrain = t has the description's n, m,
    nnz and (row, col) list, bit for bit: what makes mixed ids in one batch legitimate."""
    cs = TC.get(case)
    for t in TC.one_of_each(np.random.default_rng(31 + case)):
        q = TowrGpuProblem(TC.with_terrain(cs.desc, t), device=-1)
        assert q.sizes() == (cs.n, cs.m, cs.nnz), (case, TC.NAMES[t.id])
        r, c = q.jac_structure()
        assert np.array_equal(r, cs.r) and np.array_equal(c, cs.c), (case, TC.NAMES[t.id])
        assert q.constraint_info() == cs.info


def _refused(case, ref, other, rows):
    """Does the gate refuse the reference with the rows `rows` (g and Jacobian entries) taken from `other`?"""
    cs = TC.get(case)
    g, v = ref[0].copy(), ref[1].copy()
    g[rows] = other[0][rows]
    sel = rows[cs.r]
    v[sel] = other[1][sel]
    try:
        TC.gate(case, ref, g, v, "teeth")
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("case,B", TC.CASE_BATCHES, ids=[f"{c}-B{B}" for c, B in TC.CASE_BATCHES])
def test_another_problems_terrain_would_be_refused(case, B):
    """Teeth, a condition on the drawn inputs: for every problem b and every terrain a defective launch could read
    instead of terrains[b] (problem b - 1's, b + 1's, problem 0's, the description's), the oracle with that terrain at
    X[b], restricted to the rows of a basis-only constraint set, is refused by the gate against the oracle with
    terrains[b]; likewise terrains[b] with only the neighbour's friction coefficient. The sets whose rows carry mu
    (ForceConstraintDiscretized, Force, TorqueConstraintDiscretized) refuse every alternative. The node-based Torque's g
    and Jacobian carry the basis alone (its mu is in the bounds, test_host_functions_follow_the_terrain): it refuses every
    alternative where either terrain is of a sloped id, and a sloped terrain with its slope taken away."""
    cs = TC.get(case)
    terrains, X = TC.batch(case, B)
    present = [k for k in TC.BASIS_ONLY if k in cs.kinds]
    assert present
    for b, t in enumerate(terrains):
        ref = TC.reference(case, t, X[b])
        wrong = dict(TC.wrong_terrains(case, terrains, b))
        nb = terrains[(b + 1) % B]
        assert nb.friction_coeff != t.friction_coeff
        wrong["terrains[b] with the neighbour's mu"] = H(t.id, t.params, nb.friction_coeff)
        if t.id in TC.SLOPED or cs.gap:
            wrong["terrains[b] flattened"] = H(H.FlatID, (0.0,), t.friction_coeff)
        for name, w in wrong.items():
            if name in ("terrains[b - 1]", "terrains[b + 1]", "terrains[0]") and w is t:
                continue   # (problem 0 is its own terrains[0])
            other = TC.reference(case, w, X[b])
            for k in present:
                sloped = t.id in TC.SLOPED or w.id in TC.SLOPED or cs.gap
                if name == "terrains[b] flattened":
                    must = True   # the feet stand on the sloped pieces: the basis is tilted where the set reads it
                elif k in TC.CARRIES_MU:
                    must = True
                else:
                    must = sloped and name != "terrains[b] with the neighbour's mu"
                if must:
                    assert _refused(case, ref, other, cs.rows_of((k,))), \
                        f"{case} B = {B} problem {b} ({TC.NAMES[t.id]}): constraint kind {k} would pass with {name} ({TC.NAMES[w.id]})"


def _reached(case, terrains, X, who, table):
    cs = TC.get(case)
    for b, t in enumerate(terrains):
        for ee, i, x, y in cs.foot_points(X[b]):
            ph, pd = TC.pieces(t, x, y)
            table.setdefault((t.id, "h", ph), []).append(who(b))
            table.setdefault((t.id, "dh", pd), []).append(who(b))


def test_every_piece_is_reached():
    """The table of (id, piece) of ter_h and ter_dh against the first (case, B, problem) whose foot nodes (read from x
    through the TerrainConstraint rows' columns) reach it, over everything tests/test_gpu_terrain_batch.py evaluates:
    the batches of 5 and 67 and the tie-point rows. No entry of PIECES may be unreached."""
    points, ties = {}, {}
    for case, B in TC.CASE_BATCHES:
        terrains, X = TC.batch(case, B)
        _reached(case, terrains, X, lambda b: f"{case} B={B} b={b}", points)
    for case in TC.CASES:
        terrains, X = TC.tie_rows(case)
        _reached(case, terrains, X, lambda b: f"{case} tie row {b}", ties)
    missing = []
    print()
    for tid in TC.CYCLE + (H.GapID,):
        for which in ("h", "dh"):
            for piece in TC.PIECES[tid][which]:
                if tid == H.StepsID and piece.startswith("step ") and int(piece.split()[1]) >= TC.MAX_STEPS:
                    continue
                a, t = points.get((tid, which, piece), []), ties.get((tid, which, piece), [])
                print(f"{TC.NAMES[tid]:10s} {which:2s} {piece:12s} batch points: {len(a):5d} (first: {a[0] if a else '-'}); tie rows: {len(t):4d}")
                if not a and not t:
                    missing.append((TC.NAMES[tid], which, piece))
    assert not missing, f"unreached pieces: {missing}"
    assert not set(points) - {(tid, w, pc) for tid in TC.PIECES for w in ("h", "dh") for pc in TC.PIECES[tid][w]}


def _emulate(emu, desc, x, m, nnz):
    g, v = np.full(m, np.nan), np.full(nnz, np.nan)
    err = C.create_string_buffer(256)
    x = np.ascontiguousarray(x)
    assert emu.emu_eval(C.byref(desc), x.ctypes.data_as(D), g.ctypes.data_as(D), v.ctypes.data_as(D), err, 256) == 0, err.value
    return g, v


@pytest.mark.parametrize("case", TC.CASES)
def test_emulated_values_match_oracle(emu, case):
    """The host emulation of the kernels' item loop with a layout of desc.terrain = terrains[b] (it reads the layout's
    terrain) against the oracle with the same terrain, into NaN-filled outputs under the unchanged gate: at every point
    of the batches of 5 and 67 and at every tie-point row. The sizes and the pattern are those of a layout-only handle
    of the same description: the case's own outside the Gap class, on Gap the pattern frozen at that terrain's x0."""
    from tests.gap_frozen import frozen_reference
    from tests.parity import assert_close
    cs = TC.get(case)
    worst, layouts = 0.0, {}
    sets = [TC.batch(c, B) for c, B in TC.CASE_BATCHES if c == case] + [TC.tie_rows(case)]
    for k, (terrains, X) in enumerate(sets):
        for b, t in enumerate(terrains):
            what = f"{case} set {k} row {b} ({TC.NAMES[t.id]})"
            desc = TC.with_terrain(cs.desc, t)
            if id(t) not in layouts:
                q = TowrGpuProblem(desc, device=-1)
                layouts[id(t)] = (q.sizes(), q.jac_structure())
            (n, m, nnz), (r, c) = layouts[id(t)]
            assert (n, m) == (cs.n, cs.m) and (cs.gap or (nnz == cs.nnz and np.array_equal(r, cs.r) and np.array_equal(c, cs.c))), what
            g, v = _emulate(emu, desc, X[b], m, nnz)
            if cs.gap:
                o = TC.oracle_for(case, t)
                st = assert_close(o.eval_g(X[b]), g, r, frozen_reference(o, r, c, X[b])[0], v, m, what, cols_ref=c, floor_cols=TC.floor_cols(case))
            else:
                st = TC.gate(case, TC.reference(case, t, X[b]), g, v, what)
            worst = max(worst, st["worst"])
    print(f"{case}: worst |err| / tolerance {worst:.3g}")


@pytest.mark.parametrize("case", [74, 16])
def test_host_functions_follow_the_terrain(case):
    """towr_gpu_initial_x_for and towr_gpu_constraint_bounds_for for one drawn terrain of every id with a drawn mu: x0
    bit-equal to the oracle's of desc.terrain = t; the bounds equal to tests/bounds_ref.py's at that x0 and terrain
    (bit-exact but the node Torque's (-L, L) rows, within 4 ulp as in tests/test_bounds.py). With the node-based Torque
    (seed 74) the third row of a node carries mu and the normal: another mu alone moves every such row whose limit is not zero."""
    cs = TC.get(case)
    rng = np.random.default_rng(7400 + case)
    tq = R.torque_rows(cs.desc)
    assert (tq.size > 0) == (capi.C_TORQUE in cs.kinds)
    for t in TC.one_of_each(rng):
        x0 = cs.p.initial_x_for(cs.desc.init, t.to_c())
        ref = TC.oracle_for(case, t).initial_x()
        assert np.array_equal(x0.view(np.uint64), ref.view(np.uint64)), (case, TC.NAMES[t.id])
        got = cs.p.constraint_bounds_for(cs.desc.init, t.to_c())
        lo, up, _ = R.bounds_ref(cs.desc, x0, terrain=t.to_c())
        exact = np.ones(cs.m, dtype=bool)
        exact[tq] = False
        for a, b, side in ((got[0], lo, "lower"), (got[1], up, "upper")):
            assert np.array_equal(a[exact].view(np.uint64), b[exact].view(np.uint64)), (case, TC.NAMES[t.id], side)
            assert (np.abs(a[tq] - b[tq]) <= 4 * np.spacing(np.abs(b[tq]))).all(), (case, TC.NAMES[t.id], side)
        if tq.size:
            other = H(t.id, t.params, float(rng.uniform(*TC.MU_RANGE)))
            moved = cs.p.constraint_bounds_for(cs.desc.init, other.to_c())
            live = got[1][tq] != 0.0     # (a phase whose first force node is zero at x0 has L = 0 whatever mu is)
            assert live.any() and (moved[1][tq] != got[1][tq])[live].all() and np.array_equal(moved[1][exact], got[1][exact])
