"""The objective and the trajectory export on swept formulation shapes, CPU side (DESIGN.md "Cost sweep"). The two
kernels of cost_traj.hip had only run on default-shape descriptions (configs.cost_descs, TRAJ_CASES, ext_cases); here
shape_sweep.make_with_costs draws, on top of make(seed)'s shape, which cost kinds are present, their weights, the energy
torque weight and the cost sample periods, and configs.anymal_trot_slot_limit builds the two horizons either side of
kCostSlotMax with their RotVec twins.

Seeds 0..199 and the four built shapes: engine_math.h's cost items and traj_row through the host emulation against the
oracle (tests/parity.py's gate, unchanged), the rules of the two deterministic accumulations, the contact columns of
feet that start in flight or never touch down, the number of gradient entries per column on the limb path. On
COST_GPU_SEEDS only: the oracle's gradient against central differences, and what the list reaches.
tests/test_gpu_cost_sweep.py runs COST_GPU_SEEDS and the built shapes on the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.oracle import Oracle
from tests.configs import anymal_long_gait, anymal_slot_horizons, anymal_trot_slot_limit, emu_cost_slots
from tests.parity import assert_cost_close
from tests.shape_sweep import COST_KINDS, DT_BASE_HEIGHT, DT_COST, DT_COST_EE_BASE_POS, ROBOTS, TORQUE_WEIGHTS, make_with_costs
from tests.test_costs import _fd_grad, _sched_cols
from towr2025_amd import TowrGpuProblem, _capi as capi
from towr2025_amd import formulation as F

HERE = os.path.dirname(os.path.abspath(__file__))
D = C.POINTER(C.c_double)
CPU_SEEDS = range(200)
SLOT_LIMIT = anymal_trot_slot_limit()     # searched here, at import (configs.anymal_trot_slot_limit)
K_COST_SLOT_MAX = 8192                    # layout.h kCostSlotMax (TOWR_COST_SLOT_MAX)
# Chosen on the CPU from info and layout-only handles so that test_gpu_seeds_cover_the_cost_shapes holds, small problems
# first. 93: the sweep's largest n, slots; 13: phase-duration optimisation, every foot starts in flight, foot 0 never
# touches down, EEBasePos and BaseHeight; 2: the same with fixed durations (foot 2), torque weight 2; 11, 196: n < 192;
# 167, 18: the large phase-duration shapes, 18 with RotVec and Node items only; 19, 129, 164: bipeds under phase-duration
# optimisation with feet in flight at the start, EEBasePos and BaseHeight (129 the per-sample Energy items with torque
# weight 2, 164 RotVec); 150: fixed durations, RotVec, both feet start in flight, 244 entries in one column.
COST_GPU_SEEDS = [2, 11, 13, 18, 19, 42, 62, 93, 126, 129, 150, 163, 164, 167, 180, 196]
CASES = list(CPU_SEEDS) + sorted(SLOT_LIMIT)
LIMB_EXACT = 2 ** 11                      # engine_math.h limb_value: the column sums stay exact below 2^11 entries


@pytest.fixture(scope="module")
def emu():
    lib = os.path.join(HERE, "host_emu", "build", "libemu.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "host_emu")])
    L = C.CDLL(lib)
    L.emu_cost.argtypes = [C.POINTER(capi.ProblemDesc), D, D, D, C.c_char_p, C.c_int]
    L.emu_cost_acc.argtypes = [C.POINTER(capi.ProblemDesc), D, C.c_int, D, D]
    L.emu_cost_col_max.argtypes = [C.POINTER(capi.ProblemDesc), D]
    L.emu_traj.argtypes = [C.POINTER(capi.ProblemDesc), D, C.c_double, D, C.c_int]
    return L


def cost_case(case):
    """(description, info) of a seed of make_with_costs or of a built shape's name; info of a built shape holds what
    the tests here read (optimize, rotvec, ee_base_pos)."""
    if case in SLOT_LIMIT:
        desc = SLOT_LIMIT[case]
        return desc, {"seed": case, "optimize": False, "rotvec": bool(desc.angular_rep), "ee_base_pos": True}
    f, info, costs = make_with_costs(case)
    return f.to_desc(costs=costs), info


def cost_points(case, x0, count, scale=0.05):
    """x0 and count - 1 perturbations x0 + scale N(0, 1)."""
    stream = case if isinstance(case, int) else 1000 + (sorted(SLOT_LIMIT) + ["anymal_long_gait"]).index(case)
    rng = np.random.default_rng([2000003, stream])
    return [x0] + [x0 + scale * rng.standard_normal(x0.size) for _ in range(count - 1)]


def feet_off_the_ground_at_start(desc):
    """Feet whose first phase is a flight phase (a foot that never touches down is one with a single such phase)."""
    return [ee for ee in range(desc.robot.n_ee) if not desc.contact_at_start[ee]]


def contact_col(ee):
    return 19 + 25 * ee + 24     # trajectory.csv_header: is_contact_phase_<ee>


def instantiation(desc):
    """towr_cost_kernel<accumulation, phase-duration optimisation, RotVec> of a description's gradient launch
    (towr_gpu.hip cost_acc, cost_traj.hip cost_kernel_for)."""
    return ("slots" if emu_cost_slots(desc) > 0 else "limbs", "yes" if desc.optimize_timings else "no",
            "yes" if desc.angular_rep else "no")


def _emu_cost(emu, desc, x):
    f, g = C.c_double(), np.full(len(x), np.nan)
    err = C.create_string_buffer(256)
    assert emu.emu_cost(C.byref(desc), x.ctypes.data_as(D), C.byref(f), g.ctypes.data_as(D), err, 256) == 0, err.value
    return f.value, g


def _emu_acc(emu, desc, x, acc):
    f, g = C.c_double(np.nan), np.full(len(x), np.nan)
    rc = emu.emu_cost_acc(C.byref(desc), x.ctypes.data_as(D), acc, C.byref(f), g.ctypes.data_as(D))
    return rc, f.value, g


def test_slot_limit_pair_is_where_the_issue_found_it():
    """The searched horizons are 3.5 s and 3.6 s; the first keeps more than 0.9 kCostSlotMax slots (the slot path at its
    largest LDS footprint), the second has none, and RotVec changes neither."""
    assert anymal_slot_horizons() == (35, 36)
    for name, desc in SLOT_LIMIT.items():
        nslot = emu_cost_slots(desc)
        assert not desc.optimize_timings and bool(desc.angular_rep) == name.endswith("_rotvec")
        if "slots_max" in name:
            assert 0.9 * K_COST_SLOT_MAX < nslot <= K_COST_SLOT_MAX, (name, nslot)
        else:
            assert nslot == 0, (name, nslot)
        print(f"{name}: n {TowrGpuProblem(desc, device=-1).n} nslot {nslot} <{', '.join(instantiation(desc))}>")
    assert {instantiation(d) for d in SLOT_LIMIT.values()} == {("slots", "no", "no"), ("slots", "no", "yes"),
                                                               ("limbs", "no", "no"), ("limbs", "no", "yes")}


def test_make_with_costs_leaves_make_alone():
    """make_with_costs(seed) is make(seed) plus costs: the same description but for the cost list, and two calls agree."""
    from tests.shape_sweep import make
    for seed in (0, 13, 93, 196):
        f0, info0 = make(seed)
        f1, info1, costs = make_with_costs(seed)
        assert all(info1[k] == v for k, v in info0.items())
        d0, d1, d2 = f0.to_desc(), f1.to_desc(costs=[]), make_with_costs(seed)[0].to_desc(costs=make_with_costs(seed)[2])
        assert bytes(d0) == bytes(d1)
        assert bytes(d2) == bytes(f1.to_desc(costs=costs)) and d2.n_costs == len(costs) > 0


@pytest.mark.parametrize("case", CASES)
def test_emulated_costs_match_oracle(emu, case):
    """engine_math.h's cost items (host instantiation; the segment rows by pointer) at x0 and two 0.05 perturbations."""
    desc, info = cost_case(case)
    o = Oracle(desc)
    for k, x in enumerate(cost_points(case, o.initial_x(), 3)):
        f, g = _emu_cost(emu, desc, x)
        assert_cost_close(o.eval_f(x), f, o.eval_grad_f(x), g, f"{case} point {k}")


@pytest.mark.parametrize("case", CASES)
def test_accumulation_rules(emu, case):
    """The kernel's two deterministic accumulations with its own emitters (emu_cost_acc). The limbs (acc 2) always run
    and pass the gate. The slots (acc 1) exist exactly when the phase durations are fixed and the layout has slots
    (emu_cost_slots > 0: cost items, and at most kCostSlotMax entries); the emitter then fills exactly the host pass's
    slots (rc 2 otherwise) at x0, at a 0.05 and at a 0.5 perturbation, which pins that an entry's presence does not
    depend on x. Where both run they agree to rounding."""
    desc, info = cost_case(case)
    o = Oracle(desc)
    x0 = o.initial_x()
    nslot = emu_cost_slots(desc)
    slots = not desc.optimize_timings and nslot > 0
    assert nslot == 0 or not desc.optimize_timings
    for k, x in enumerate(cost_points(case, x0, 2)):
        f_ref, g_ref = o.eval_f(x), o.eval_grad_f(x)
        rc2, f2, g2 = _emu_acc(emu, desc, x, 2)
        assert rc2 == 0
        assert_cost_close(f_ref, f2, g_ref, g2, f"{case} point {k} limbs")
        rc1, f1, g1 = _emu_acc(emu, desc, x, 1)
        assert rc1 == (0 if slots else 1), f"{case} point {k}: slots rc {rc1}, nslot {nslot}"
        if slots:
            assert_cost_close(f_ref, f1, g_ref, g1, f"{case} point {k} slots")
            np.testing.assert_allclose(g1, g2, rtol=1e-12, atol=1e-15 * max(1.0, np.abs(g_ref).max()))
    far = cost_points(case, x0, 2, scale=0.5)[1]
    assert _emu_acc(emu, desc, far, 1)[0] == (0 if slots else 1), f"{case}: the slot count moved with x"


@pytest.mark.parametrize("case", CASES)
def test_emulated_trajectory_matches_oracle(emu, case):
    """traj_row through the host emulation against the oracle at two sample periods (test_trajectory.py's gate); the
    is_contact_phase columns of feet whose first phase is a flight phase (TrajPhases::c0 = 0), a foot that never
    touches down among them, compared for equality."""
    desc, info = cost_case(case)
    o = Oracle(desc)
    x = cost_points(case, o.initial_x(), 2, scale=0.03)[1]
    for dt in (0.01, 0.037):
        ref = o.sample_trajectory(x, dt)
        out = np.full_like(ref, np.nan)
        assert emu.emu_traj(C.byref(desc), x.ctypes.data_as(D), dt, out.ctypes.data_as(D), out.shape[0]) == ref.shape[0]
        np.testing.assert_allclose(out, ref, rtol=1e-12, atol=1e-12)
        for ee in feet_off_the_ground_at_start(desc):
            np.testing.assert_array_equal(out[:, contact_col(ee)], ref[:, contact_col(ee)], err_msg=f"{case} dt {dt} foot {ee}")
            assert ref[0, contact_col(ee)] == 0.0
            if desc.n_phases[ee] == 1:
                assert not ref[:, contact_col(ee)].any(), f"{case}: foot {ee} never touches down"


def _limb_shapes():
    out = [c for c in CASES if (c in SLOT_LIMIT and "past_slots" in c) or (c not in SLOT_LIMIT and make_with_costs(c)[1]["optimize"])]
    return out + ["anymal_long_gait"]


@pytest.mark.parametrize("case", _limb_shapes())
def test_limb_columns_stay_below_the_exact_range(emu, case):
    """Every shape the device sends through the limbs (phase-duration optimisation, and fixed durations past
    kCostSlotMax), ANYmal's 17-phase gait with every cost kind included: the largest number of gradient entries one
    column receives (emu_cost_col_max, at x0 and at a perturbation: PhaseSpline windows move with x) is below 2^11,
    the documented exactness bound of limb_value. A shape at or above it would be compared here against the
    big-integer restatement of tests/test_costs.py instead of raising the bound; none is (the largest: DESIGN.md)."""
    desc = anymal_long_gait(costs=True) if case == "anymal_long_gait" else cost_case(case)[0]
    x0 = TowrGpuProblem(desc, device=-1).initial_x()
    for x in cost_points(case, x0, 2):
        mx = emu.emu_cost_col_max(C.byref(desc), x.ctypes.data_as(D))
        assert 0 <= mx < LIMB_EXACT, f"{case}: {mx} entries in one column"


@pytest.mark.parametrize("case", COST_GPU_SEEDS)
def test_oracle_gradient_matches_fd(case):
    """The oracle checks itself on the shapes the device is compared with: its gradient against central differences of
    its objective, test_costs.py's formula and bound, every 8th column. With EEBasePos on, the schedule columns are
    left out (the reference quirk: EEBasePosCost reports no schedule block, test_costs.py pins it). BaseHeightCost has
    a second quirk of that kind, which this test found: base_height_cost.cc FillJacobianBlock fills the base-linear
    block only, and there only the row of z, while its value also reads the feet in contact (their z, and through
    IsContactPhase the schedule) or, with no foot in contact, the terrain under the base's x and y. The oracle and the
    engine report what the reference reports, so with BaseHeightCost on the comparison keeps, of the node columns, the
    base-angular and force / torque sets and the z columns of the base-linear set (column c0 + 6 node + 3 deriv + dim)."""
    desc, info = cost_case(case)
    o = Oracle(desc)
    x = o.initial_x() + 0.02 * np.random.default_rng(5).standard_normal(o.n)
    g = o.eval_grad_f(x)
    skip = set(_sched_cols(o, desc)) if desc.optimize_timings and (info["ee_base_pos"] or info["base_height"]) else set()
    if info["base_height"]:
        for i, (c0, nc) in enumerate(o.varset_cols()):
            if desc.varsets[i].kind == capi.VAR_EE_MOTION:
                skip |= set(range(c0, c0 + nc))
            elif desc.varsets[i].kind == capi.VAR_BASE_LIN:
                skip |= {c0 + k for k in range(nc) if k % 3 != 2}
    cols = [j for j in range(0, o.n, 8) if j not in skip]
    fd = _fd_grad(o, x, cols)
    noise = 8 * np.finfo(float).eps * abs(o.eval_f(x)) / 1e-4
    err = np.abs(fd - g[cols]) / (np.maximum(1.0, np.abs(g[cols])) + noise)
    assert err.max() < 2e-5, f"col {cols[err.argmax()]}: FD {fd[err.argmax()]} grad {g[cols][err.argmax()]}"


def test_gpu_seeds_cover_the_cost_shapes():
    """What COST_GPU_SEEDS reaches, from info and layout-only handles of exactly that list."""
    assert len(COST_GPU_SEEDS) <= 24 and len(set(COST_GPU_SEEDS)) == len(COST_GPU_SEEDS)
    assert {93, 13, 2, 11, 196, 167, 18} <= set(COST_GPU_SEEDS) <= set(CPU_SEEDS)
    rows = []
    for seed in COST_GPU_SEEDS:
        f, info, costs = make_with_costs(seed)
        desc = f.to_desc(costs=costs)
        rows.append((info, TowrGpuProblem(desc, device=-1).n, {c["kind"] for c in costs}, instantiation(desc)))
        print(f"seed {seed}: n {rows[-1][1]} <{', '.join(rows[-1][3])}>")
    infos = [r[0] for r in rows]
    assert {i["robot"] for i in infos} == set(ROBOTS)
    assert sum(i["optimize"] for i in infos) >= 6
    assert sum(i["rotvec"] for i in infos) >= 6
    assert sum(i["optimize"] and i["rotvec"] for i in infos) >= 2
    never = [i for i in infos if i["never_touches_down"]]
    assert any(not i["optimize"] for i in never) and any(i["optimize"] for i in never)
    assert sum(bool(i["starts_in_flight"]) and i["ee_base_pos"] for i in infos) >= 3
    assert any(i["starts_in_flight"] and i["ee_base_pos"] and i["optimize"] for i in infos), "the device's swing test"
    assert sum(i["base_height"] for i in infos) >= 2
    assert any(i["base_height"] and i["starts_in_flight"] for i in infos), "BaseHeightCost contact masks with such feet"
    assert all(capi.COST_BASE_HEIGHT in kinds for i, _, kinds, _ in rows if i["base_height"])
    for name in COST_KINDS:
        assert sum(name not in i["cost_kinds"] for i in infos) >= 2, name
    energy = [i for i in infos if F.Parameters.EnergyCostID in i["cost_kinds"]]
    ang_mom = [i for i in infos if F.Parameters.AngMomCostID in i["cost_kinds"]]
    assert {i["torque_weight"] for i in energy} == set(TORQUE_WEIGHTS)
    assert {i["dt_cost_energy"] for i in energy} == set(DT_COST)
    assert {i["dt_cost_ang_mom"] for i in ang_mom} == set(DT_COST)
    assert {i["dt_cost_ee_base_pos"] for i in infos if i["ee_base_pos"]} == set(DT_COST_EE_BASE_POS)
    assert {i["dt_base_height"] for i in infos if i["base_height"]} == set(DT_BASE_HEIGHT)
    ns = [n for _, n, _, _ in rows]
    assert min(ns) < 192, "the wave schedule with few items of one kind"
    assert max(ns) == max(TowrGpuProblem(make_with_costs(s)[0].to_desc(), device=-1).n for s in CPU_SEEDS), "the sweep's largest n"
    assert {r[3] for r in rows} == {("slots", "no", "no"), ("slots", "no", "yes"), ("limbs", "yes", "no"), ("limbs", "yes", "yes")}
