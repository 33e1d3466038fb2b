"""Seeded sweep of formulation shapes (tests/shape_sweep.py) against the oracle. tests/configs.py keeps the reference's
default shape parameters; here the polynomial counts, time steps, phase counts and durations, feet that start in flight
or never touch down, and the optional constraint sets vary, since they select the spline tables, instant counts, tile
emitters and, under phase-duration optimisation, the record + compose path or its fallbacks to the tile path.

CPU, seeds 0..199: the layout-only handle (sizes, x0, pattern, bounds) and the values of the test-only host emulation.
GPU, the 32 seeds of GPU_SEEDS, the 16 fixed-gait shapes of real size of FIXED_GAIT_SEEDS and STAGE_OVERFLOW: single calls, the fused
call and a device batch of 3, against the oracle and each other; and a device batch of 65 (one above the batch size
at which the launch paths change), every row against the single call and rows 0..2 against the oracle.
The gate is tests/parity.py's, unchanged. DESIGN.md "Shape sweep" has the generator's table and the results."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.oracle import Oracle
from tests import bounds_ref as R
from tests.parity import assert_close, residue_cols
from tests.shape_sweep import FORCE_POLYS, ROBOTS, SWING_POLYS, TERRAINS, make, refused_descs
from towr2025_amd import TowrGpuProblem, _capi as capi
from towr2025_amd import formulation as F
from towr2025_amd.problem import TowrGpuError

HERE = os.path.dirname(os.path.abspath(__file__))
D = C.POINTER(C.c_double)
CPU_SEEDS = range(200)
# chosen with layout-only handles, small problems first, so that test_gpu_seeds_cover_the_shapes holds; 13, 86 and 131
# are the shape that used to divide by zero in build_fstream (phase-duration optimisation with a foot that never
# touches down; 86 also has TorqueConstraintDiscretized on that foot), 85 has such a foot with a fixed gait
GPU_SEEDS = [0, 10, 13, 16, 18, 35, 45, 59, 74, 79, 82, 83, 85, 86, 94, 99, 109, 110, 116, 117, 123, 126, 131, 154, 160, 167,
             176, 182, 191, 194, 195, 196]
# fixed-gait shapes of real size (GPU_SEEDS' seven fixed-gait seeds have n <= 363 and nnz <= 3283): the tile path, the
# fused RangeOfMotion + FDISC launch and the per-class launches at the sizes they are built for. 93: the largest n, odd
# and above the 1152 columns the fused launch's 192 threads keep in flight (3 16-byte units each: beyond them
# XStage::commit's overflow branch); 39: the largest m; 8, 2, 36, 11: FDISC + TQDISC tiles on 4 / 4 (one foot never touches down) / 2 / 1 feet,
# 11 with n < 192; 134, 50: node-based Force, TQDISC tile; 179: few columns, the longest column; 9: neither grid;
# 124, 96, 175, 66, 70, 155: RotVec (the pre-pass and per-class launches), 175 with 4 empty sets, 66 with 880 empty rows
FIXED_GAIT_SEEDS = [2, 8, 9, 11, 36, 39, 50, 66, 70, 93, 96, 124, 134, 155, 175, 179]
# One shape that is no seed. In every shape of the sweep (93 included) the columns past 1152 belong to the torque
# variables, which come last and which only the 256-thread Dynamic tiles read: the overflow branch of the fused launch's
# 192-thread FDISC staging runs there, but nothing reads what it stages. The default ANYmal trot with a base polynomial
# of 0.04 s (n = 1522) pushes the force variables of feet 2 and 3 past column 1152, where the FDISC tiles read them.
STAGE_OVERFLOW = "anymal_trot_base_poly_0p04"
GPU_CASES = GPU_SEEDS + FIXED_GAIT_SEEDS + [STAGE_OVERFLOW]
DYN, ROM, FDISC, TQDISC = 0, 1, 2, 3   # launch classes of TowrGpuProblem.kernel_path
BIG = 65   # one above the batch size at which the launch paths change (kSplitBatch = 64), odd, 16 * 4 + 1: the last
           # composer group is ragged whether a block takes 16, 4 or 1 problems


@pytest.fixture(scope="module")
def emu():
    lib = os.path.join(HERE, "host_emu", "build", "libemu.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "host_emu")])
    L = C.CDLL(lib)
    L.emu_eval.argtypes = [C.POINTER(capi.ProblemDesc), D, D, D, C.c_char_p, C.c_int]
    return L


def _stage_overflow_formulation():
    f = F.anymal_trot()
    f.params_.duration_base_polynomial_ = 0.04
    return f


def _case(seed):
    """(description, info, oracle, x0, reference rows, reference cols) of a seed (or of STAGE_OVERFLOW). The oracle
    accepts every seed of the generator: a refusal here is a generator bug, never a skip."""
    f, info = (_stage_overflow_formulation(), {"seed": seed}) if seed == STAGE_OVERFLOW else make(seed)
    desc = f.to_desc()
    o = Oracle(desc)
    x0 = o.initial_x()
    r, c, _ = o.eval_jac(x0)
    return desc, info, o, x0, r, c


def _points(seed, x0, count):
    """x0 and count - 1 perturbations x0 + 0.05 N(0, 1)."""
    rng = np.random.default_rng(1000003 + (424242 if seed == STAGE_OVERFLOW else seed))
    return [x0] + [x0 + 0.05 * rng.standard_normal(x0.size) for _ in range(count - 1)]


def _reference(o, r, c, x, what):
    rr, cc, v = o.eval_jac(x)
    assert np.array_equal(rr, r) and np.array_equal(cc, c), f"{what}: the reference pattern moved (no Gap terrain here)"
    return o.eval_g(x), v


def _assert_pattern(p, o, x0, r, c, what):
    assert (p.n, p.m, p.nnz) == (o.n, o.m, len(r)), what
    np.testing.assert_array_equal(p.initial_x().view(np.uint64), x0.view(np.uint64), err_msg=what)
    pr, pc = p.jac_structure()
    np.testing.assert_array_equal(pr, r, err_msg=what)
    np.testing.assert_array_equal(pc, c, err_msg=what)


@pytest.mark.parametrize("seed", CPU_SEEDS)
def test_layout_matches_oracle(seed):
    """Layout-only handle: n, m, nnz, x0 and the (row, col) list bit-exact against the oracle; the constraint sets'
    rows against the oracle's and their bounds against tests/bounds_ref.py (bit-exact but the node-Torque (-L, L)
    rows, within 4 ulp as in tests/test_bounds.py)."""
    desc, info, o, x0, r, c = _case(seed)
    p = TowrGpuProblem(desc, device=-1)
    _assert_pattern(p, o, x0, r, c, f"seed {seed}")
    assert [(r0, n) for _, _, r0, n in p.constraint_info()] == o.constraint_rows()
    assert [(c0, n) for _, _, c0, n in p.varset_info()] == o.varset_cols()
    lo, up, sets = R.bounds_ref(desc, x0)
    assert [s[3] for s in sets] == [n for _, _, _, n in p.constraint_info()]
    got = p.constraint_bounds()
    exact = np.ones(p.m, dtype=bool)
    tq = R.torque_rows(desc)
    exact[tq] = False
    for g, ref, side in ((got[0], lo, "lower"), (got[1], up, "upper")):
        np.testing.assert_array_equal(g[exact].view(np.uint64), ref[exact].view(np.uint64), err_msg=f"seed {seed}: {side}")
        assert (np.abs(g[tq] - ref[tq]) <= 4 * np.spacing(np.abs(ref[tq]))).all(), f"seed {seed}: {side} (-L, L) rows"


@pytest.mark.parametrize("seed", CPU_SEEDS)
def test_emulated_values_match_oracle(emu, seed):
    """The host emulation of the kernels' item loop at x0 and one perturbation, outputs pre-filled with NaN."""
    desc, info, o, x0, r, c = _case(seed)
    fc = residue_cols(desc, o.n)
    for k, x in enumerate(_points(seed, x0, 2)):
        g_ref, v_ref = _reference(o, r, c, x, f"seed {seed} point {k}")
        g, v = np.full(o.m, np.nan), np.full(len(r), np.nan)
        err = C.create_string_buffer(256)
        assert emu.emu_eval(C.byref(desc), x.ctypes.data_as(D), g.ctypes.data_as(D), v.ctypes.data_as(D), err, 256) == 0, err.value
        assert_close(g_ref, g, r, v_ref, v, o.m, f"seed {seed} point {k}", cols_ref=c, floor_cols=fc)


def test_gpu_seeds_cover_the_shapes():
    """GPU_SEEDS must not collapse back to the default shape: conditions on the drawn values and on the launch paths
    of the layout-only handles of exactly that list."""
    assert len(GPU_SEEDS) == 32 and len(set(GPU_SEEDS)) == 32
    infos, paths = [], []
    for seed in GPU_SEEDS:
        f, info = make(seed)
        p = TowrGpuProblem(f.to_desc(), device=-1)
        infos.append(info)
        paths.append([p.kernel_path(k) for k in (DYN, ROM, FDISC, TQDISC)])
    assert sum(i["optimize"] for i in infos) >= 12
    assert sum(i["rotvec"] for i in infos) >= 8
    assert {i["force_polys"] for i in infos} == set(FORCE_POLYS)
    assert {i["swing_polys"] for i in infos} == set(SWING_POLYS)
    assert sum(bool(i["starts_in_flight"]) for i in infos) >= 4
    never = [i for i in infos if i["never_touches_down"]]
    assert len(never) >= 2 and any(i["optimize"] for i in never)
    assert sum(bool(i["single_stance"]) for i in infos) >= 2
    assert {i["terrain"] for i in infos} == set(TERRAINS)
    assert {i["robot"] for i in infos} == set(ROBOTS)
    assert any(i["dt_force"] == 0.0 for i in infos), "node-based Force"
    assert any(i["torque"] and i["dt_torque"] == 0.0 for i in infos), "node-based Torque"
    gait = [pt for i, pt in zip(infos, paths) if i["optimize"]]
    for k, name in ((DYN, "Dynamic"), (ROM, "RangeOfMotion"), (FDISC, "FDISC"), (TQDISC, "TQDISC")):
        assert sum(pt[k] == 1 for pt in gait) >= 3, f"{name} on the record + compose path"
    # fallbacks to the tile path on gait-optimising seeds (no Gap terrain here): a foot that never touches down has
    # empty FDISC / TQDISC rows (build_fstream's and build_gstream_class's exits for a constraint without entries)
    assert any(pt[FDISC] == 0 for pt in gait), "FDISC fallback to the tile path"
    assert any(pt[TQDISC] == 0 for pt in gait), "TQDISC fallback to the tile path"
    for i, pt in zip(infos, paths):   # and nothing else falls back in the table's range
        if i["optimize"] and not i["never_touches_down"]:
            assert all(k in (1, -1) for k in pt), i["seed"]
    for i, pt in zip(infos, paths):   # the fixed-gait seeds never stream
        if not i["optimize"]:
            assert all(k in (0, -1) for k in pt), i["seed"]


def _launch_shape(seed):
    """(info, p, paths by class, kernels by index, step_launches) of a seed's layout-only handle."""
    f, info = make(seed)
    p = TowrGpuProblem(f.to_desc(), device=-1)
    return info, p, [p.kernel_path(k) for k in (DYN, ROM, FDISC, TQDISC)], {k: nt for k, _, nt, _ in p.kernels()}, p.step_launches()


def test_fixed_gait_seeds_cover_the_shapes():
    """FIXED_GAIT_SEEDS is worth its GPU time only while these hold, on the layout-only handles of exactly that list."""
    assert len(FIXED_GAIT_SEEDS) == 16 and len(set(FIXED_GAIT_SEEDS)) == 16 and not set(FIXED_GAIT_SEEDS) & set(GPU_SEEDS)
    assert set(FIXED_GAIT_SEEDS) <= set(CPU_SEEDS)
    rows = [_launch_shape(seed) for seed in FIXED_GAIT_SEEDS]
    for info, p, pt, kern, launches in rows:   # fixed gait, nothing on the record + compose path
        assert not info["optimize"] and all(k in (0, -1) for k in pt), info["seed"]
        assert pt[DYN] == 0 and pt[ROM] == 0, info["seed"]
    assert sum(i["rotvec"] for i, *_ in rows) >= 6
    assert {i["robot"] for i, *_ in rows} == set(ROBOTS)
    assert sum(pt[FDISC] == 0 and pt[TQDISC] == 0 for _, _, pt, _, _ in rows) >= 6, "FDISC and TQDISC tiles together"
    assert any(pt[FDISC] == -1 and pt[TQDISC] == -1 for _, _, pt, _, _ in rows), "neither grid"
    assert any(p.n % 2 == 1 and p.n > 1152 for _, p, *_ in rows), "n odd and beyond the fused launch's 3 * 192 staged units"
    assert any(p.n < 192 for _, p, *_ in rows), "fewer columns than the fused launch has threads"
    assert any(sum(n == 0 for _, _, _, n in p.constraint_info()) >= 3 for _, p, *_ in rows), "3 or more empty constraint sets"
    assert sum(bool(i["never_touches_down"]) for i, *_ in rows) >= 2
    # the fused RangeOfMotion + FDISC launch (a kernel index past the launch classes) on Euler shapes only, the RotVec
    # shapes launch class by class
    assert sum(any(k >= 5 for k in launches) for _, _, _, _, launches in rows) >= 6
    for info, _, pt, _, launches in rows:
        assert any(k >= 5 for k in launches) == (not info["rotvec"] and pt[FDISC] == 0), info["seed"]


def test_stage_overflow_shape_reads_what_the_overflow_stages():
    """STAGE_OVERFLOW: fixed-gait Euler with the fused RangeOfMotion + FDISC launch of 192 threads, more than 3 * 192
    16-byte units of x, and FDISC rows with entries in columns past 1152 (the units XStage::commit's overflow branch
    stages) - while no seed of the sweep has such rows, which is why the shape is here."""
    p = TowrGpuProblem(_stage_overflow_formulation().to_desc(), device=-1)
    names = {k: name for k, name, _, _ in p.kernels()}
    assert [names[k] for k in p.step_launches() if k >= 5] == ["range_of_motion+force_discretized"]
    assert p.kernel_path(FDISC) == 0 and p.n // 2 > 3 * 192 and p.n // 2 <= 3 * 256

    def fdisc_entries_past(p, first):
        rp, col = p.jac_csr()
        return sum(int((col[rp[r0]:rp[r0 + rows]] >= first).sum()) for kind, _, r0, rows in p.constraint_info() if kind == capi.C_FORCE_DISCRETIZED)
    assert fdisc_entries_past(p, 1152) > 1000
    for seed in CPU_SEEDS:
        f, info = make(seed)
        if not info["optimize"] and info["dt_force"] != 0.0:
            q = TowrGpuProblem(f.to_desc(), device=-1)
            assert q.n <= 1152 or fdisc_entries_past(q, 1152) == 0, seed


def _large_batch_shapes(optimize, rotvec, pt, kern, launches, what):
    """The launch shapes of one layout at B >= kSplitBatch, by name, from its paths by class, kernels by index and
    step_launches() (shared with tests/test_want_flags_cases.py)."""
    for k in (DYN, ROM, FDISC, TQDISC):   # a class is launched exactly when it has tiles
        assert (pt[k] != -1) == (k in kern), (what, k)
    fused = [k for k in launches if k >= 5]
    assert all(k in kern for k in launches) and not (fused and optimize), what
    streamed = [k for k in (DYN, ROM, FDISC, TQDISC) if pt[k] == 1]
    tiled = [k for k in (FDISC, TQDISC) if pt[k] == 0]
    shapes = []
    if not optimize:
        shapes.append("fixed-gait RotVec" if rotvec else "fixed-gait Euler with a fusion group" if fused else "fixed-gait Euler")
    else:
        assert DYN in streamed and ROM in streamed, what
        if FDISC in streamed and TQDISC in streamed:
            shapes.append("FDISC + TQDISC streamed")
        elif FDISC in streamed:
            shapes.append("FDISC streamed beside RangeOfMotion / Dynamic")
        elif TQDISC in streamed and pt[FDISC] == -1:
            shapes.append("TQDISC streamed without an FDISC grid")
        elif pt[FDISC] == -1 and pt[TQDISC] == -1:
            shapes.append("RangeOfMotion / Dynamic streamed alone")
        if tiled:
            shapes.append("tile-path FDISC or TQDISC beside streamed classes")
    return shapes


def test_seed_lists_reach_the_large_batch_launch_shapes():
    """What test_gpu_batch_above_the_split runs at B = 65 (>= kSplitBatch, towr_gpu.hip): the launch shapes the two
    lists reach between them, from kernel_path, kernels() and step_launches() of the layout-only handles."""
    reached = {}
    for seed in GPU_SEEDS + FIXED_GAIT_SEEDS:
        info, p, pt, kern, launches = _launch_shape(seed)
        for sh in _large_batch_shapes(info["optimize"], info["rotvec"], pt, kern, launches, seed):
            reached.setdefault(sh, []).append(seed)
    print({k: v for k, v in sorted(reached.items())})
    assert len(reached.get("fixed-gait Euler with a fusion group", [])) >= 6
    assert len(reached.get("fixed-gait RotVec", [])) >= 6
    assert len(reached.get("FDISC streamed beside RangeOfMotion / Dynamic", [])) >= 3
    assert {0, 191} <= set(reached.get("FDISC + TQDISC streamed", []))
    assert {10, 94, 126} <= set(reached.get("TQDISC streamed without an FDISC grid", []))
    assert {45, 83} <= set(reached.get("RangeOfMotion / Dynamic streamed alone", []))
    assert {13, 86, 131} <= set(reached.get("tile-path FDISC or TQDISC beside streamed classes", []))


@pytest.mark.parametrize("name", sorted(refused_descs()))
def test_swing_at_trajectory_boundary_is_refused(name):
    """A foot in swing at a trajectory boundary with the Swing constraint: the oracle refuses it (the reference reads
    out of range), and engine creation returns TOWR_ERR_INVALID with a message, neither crashing nor accepting."""
    desc, foot = refused_descs()[name]
    with pytest.raises(ValueError, match="swing node at trajectory boundary"):
        Oracle(desc)
    lib = capi.load_library()
    h = C.c_void_p()
    rc = lib.towr_gpu_create_ex(C.byref(desc), 0, None, -1, C.byref(h))
    assert rc == capi.TOWR_ERR_INVALID and not h.value
    msg = lib.towr_gpu_last_error(None).decode()
    assert "swing node at trajectory boundary" in msg and f"endeffector {foot}" in msg, msg
    with pytest.raises(TowrGpuError, match=r"\(-1\).*swing node at trajectory boundary"):
        TowrGpuProblem(desc, device=-1)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", GPU_CASES)
def test_gpu_values_match_oracle(seed):
    """Device 0: pattern against the oracle; eval_g + eval_jac_values, eval_g_jac bit-equal to them; a device batch
    of 3 (x0 and two perturbations) into NaN-filled outputs with ldv rounded up to 16, each row bit-equal to the
    single calls and the padding untouched; everything against the oracle under the gate."""
    import torch
    desc, info, o, x0, r, c = _case(seed)
    p = TowrGpuProblem(desc, device=0)
    _assert_pattern(p, o, x0, r, c, f"seed {seed}")
    fc = residue_cols(desc, o.n)
    X = np.stack(_points(seed, x0, 3))
    single = []
    for k, x in enumerate(X):
        g_ref, v_ref = _reference(o, r, c, x, f"seed {seed} point {k}")
        g, v = p.eval_g(x), p.eval_jac_values(x)
        st = assert_close(g_ref, g, r, v_ref, v, o.m, f"seed {seed} point {k}", cols_ref=c, floor_cols=fc)
        g2, v2 = p.eval_g_jac(x)
        np.testing.assert_array_equal(g2.view(np.uint64), g.view(np.uint64), err_msg=f"seed {seed} point {k}: g of eval_g_jac")
        np.testing.assert_array_equal(v2.view(np.uint64), v.view(np.uint64), err_msg=f"seed {seed} point {k}: J of eval_g_jac")
        single.append((g, v))
        print(f"seed {seed} point {k}: n={p.n} m={p.m} nnz={p.nnz} max relative error {st['max_rel']:.3e}, worst |err|/tol {st['worst']:.3f}")
    dev = torch.device("cuda:0")
    ldv = (p.nnz + 15) // 16 * 16
    Gd = torch.full((3, p.m), np.nan, dtype=torch.float64, device=dev)
    Vd = torch.full((3, ldv), np.nan, dtype=torch.float64, device=dev)
    p.eval_batch_device(torch.from_numpy(X).to(dev), Gd, Vd)
    torch.cuda.synchronize()
    G, V = Gd.cpu().numpy(), Vd.cpu().numpy()
    assert np.isnan(V[:, p.nnz:]).all(), f"seed {seed}: write past nnz"
    for k, (g, v) in enumerate(single):
        np.testing.assert_array_equal(G[k].view(np.uint64), g.view(np.uint64), err_msg=f"seed {seed}: g of batch row {k}")
        np.testing.assert_array_equal(V[k, :p.nnz].view(np.uint64), v.view(np.uint64), err_msg=f"seed {seed}: J of batch row {k}")
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", GPU_CASES)
def test_gpu_batch_above_the_split(seed):
    """Device 0, one eval_batch_device call of B = 65 (x0 and 64 perturbations) with want_g = want_jac = 1 into
    NaN-filled outputs with odd leading dimensions (ldg = m + 3, ldv = nnz + 5): the side-stream fork beside the fused
    launch, the RotVec side chain, the two- and three-chain streaming path and the per-class composer launches with a
    ragged last group (test_seed_lists_reach_the_large_batch_launch_shapes). Every row bit-equal to eval_g_jac of the
    same handle at that row's x, every padding element still NaN, rows 0..2 against the oracle under the gate."""
    import torch
    desc, info, o, x0, r, c = _case(seed)
    p = TowrGpuProblem(desc, device=0)
    _assert_pattern(p, o, x0, r, c, f"seed {seed}")
    X = np.stack(_points(seed, x0, BIG))
    dev = torch.device("cuda:0")
    ldg, ldv = p.m + 3, p.nnz + 5
    Gd = torch.full((BIG, ldg), np.nan, dtype=torch.float64, device=dev)
    Vd = torch.full((BIG, ldv), np.nan, dtype=torch.float64, device=dev)
    p.eval_batch_device(torch.from_numpy(X).to(dev), Gd, Vd, want_g=True, want_jac=True)
    torch.cuda.synchronize()
    G, V = Gd.cpu().numpy(), Vd.cpu().numpy()
    assert np.isnan(G[:, p.m:]).all(), f"seed {seed}: write past m"
    assert np.isnan(V[:, p.nnz:]).all(), f"seed {seed}: write past nnz"
    for k, x in enumerate(X):
        g, v = p.eval_g_jac(x)
        np.testing.assert_array_equal(G[k, :p.m].view(np.uint64), g.view(np.uint64), err_msg=f"seed {seed}: g of batch row {k}")
        np.testing.assert_array_equal(V[k, :p.nnz].view(np.uint64), v.view(np.uint64), err_msg=f"seed {seed}: J of batch row {k}")
    fc = residue_cols(desc, o.n)
    for k in range(3):
        g_ref, v_ref = _reference(o, r, c, X[k], f"seed {seed} point {k}")
        assert_close(g_ref, np.ascontiguousarray(G[k, :p.m]), r, v_ref, np.ascontiguousarray(V[k, :p.nnz]), o.m, f"seed {seed} batch row {k}",
                     cols_ref=c, floor_cols=fc)
    p.close()
