"""Variable bounds, host side (no GPU): towr_gpu_variable_bounds / _with on layout-only handles against
tests/varbounds_ref.py (NodesVariables::AddBound's double loop restated in Python) on every configuration, the
formulation mirrors' var_bounds_data(), hand-checkable pins, malformed side data, the C++ mirror, and the argument
checks of the device entry points built on the bounds (step_batch_device, auglag_step_batch_device)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import varbounds_ref as R
from tests.configs import config_descs, ext_cases
from towr2025_amd import TowrGpuProblem, _capi as capi
from towr2025_amd import formulation as F
from towr2025_amd.problem import TowrGpuError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "towr2025_amd", "host")


def _cases():
    out = {name: (d, []) for name, d in config_descs().items()}
    out.update(ext_cases())
    return out


CASES = _cases()


def _plain(f):
    f.params_.enable_stance_tracking = False
    return f


def rich(f):
    """The variant `towr_host_check --varbounds rich` sets: every knob that only the variable bounds use."""
    P = f.params_
    P.constrain_base_pitch_ = True
    P.base_pitch_target_ = 0.05
    P.bounds_final_lin_pos_ = [0, 1]
    P.base_lin_waypoints_.append(F.BaseWaypoint(0.52, 0, [2], (0.0, 0.0, 0.5)))
    P.base_ang_waypoints_.append(F.BaseWaypoint(0.25, 1, [0, 2], (0.1, 0.0, -0.1), (0.05, 0.0, 0.025)))
    for ee in range(P.GetEECount()):
        P.ee_stance_position_.append([(0.125 * k + 0.0625 * ee, -0.25 * ee, 0.0) for k in range(P.GetPhaseCount(ee))])
    P.ee_stance_rpy_.append([(0.0, 0.03125 * k, 0.5) for k in range(P.GetPhaseCount(0))])
    return f


def _forms():
    """name -> (ProblemDesc, var_bounds_data) of the configurations that come from a formulation."""
    stairs = F.HeightMap.MakeTerrain(F.HeightMap.StairsID)
    forms = {
        "monoped_hopper_flat": _plain(F.monoped_hopper()),
        "biped_walk_2s": _plain(F.biped_walk()),
        "anymal_trot_2p4s": _plain(F.anymal_trot()),
        "anymal_trot_stairs": _plain(F.anymal_trot(terrain=stairs)),
        "anymal_slope_yaw": _plain(F.anymal_trot(terrain=F.HeightMap.MakeTerrain(F.HeightMap.SlopeID), goal=(1.8, 0.3, 0.0), goal_yaw=0.3)),
        "anymal_stairs_gaitopt": _plain(F.anymal_trot(terrain=stairs, optimize_timings=True)),
        "anymal_trot_rich": rich(F.anymal_trot()),
        "biped_gaitopt_rich": rich(F.biped_walk()),
        "hopper_rich": rich(F.monoped_hopper()),
    }
    forms["biped_gaitopt_rich"].params_.OptimizePhaseDurations()
    out = {name: (f.to_desc(), f.var_bounds_data()) for name, f in forms.items()}
    f, vs, cs, goal, T = F.procedural_monoped()
    out["monoped_procedural"] = (F.procedural_desc(),
                                 f.var_bounds_data(varsets=vs, init_mode=capi.INIT_PROCEDURAL, ee_goal=goal, total_time=T))
    f, vs, cs, goal, T, costs = F.backflip_monoped()
    out["monoped_backflip_rotvec"] = (F.backflip_desc(),
                                      f.var_bounds_data(varsets=vs, init_mode=capi.INIT_PROCEDURAL, ee_goal=goal, total_time=T))
    return out


FORMS = _forms()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _data(records):
    return [(capi.DATA_VAR_BOUNDS, i, np.asarray(v, dtype=np.float64)) for i, v in records.items()]


def _assert_equals_ref(p, desc, records, what):
    lo, up = R.varbounds_ref(desc, records)
    got = p.variable_bounds()
    assert lo.size == p.n
    np.testing.assert_array_equal(_bits(got[0]), _bits(lo), err_msg=f"{what}: lower")
    np.testing.assert_array_equal(_bits(got[1]), _bits(up), err_msg=f"{what}: upper")
    assert (got[0] <= got[1]).all() and np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    return got


@pytest.mark.parametrize("name", sorted(CASES))
def test_random_records_match_reference_restatement(name):
    desc, data = CASES[name]
    records = R.random_records(desc, seed=17)
    assert len(records) == sum(desc.varsets[i].kind != capi.VAR_EE_SCHEDULE for i in range(desc.n_varsets))
    p = TowrGpuProblem(desc, device=-1, data=list(data) + _data(records))
    lo, up = _assert_equals_ref(p, desc, records, name)
    assert (lo == up).any() and ((lo > -1e19) & (lo < up)).any() and (lo == -1e20).any()
    # the sets tile [0, n) as the restatement lays them out
    assert [(c0, n) for _, _, c0, n in p.varset_info()] == [(c0, rows) for _, _, c0, rows, _, _ in R.set_layout(desc)]


@pytest.mark.parametrize("name", sorted(FORMS))
def test_formulation_records_match_reference_restatement(name):
    desc, vb = FORMS[name]
    assert vb and all(k == capi.DATA_VAR_BOUNDS and len(v) % 5 == 0 for k, _, v in vb)
    if name in CASES:   # the same problem as the configuration of that name
        assert bytes(desc) == bytes(CASES[name][0])
    p = TowrGpuProblem(desc, device=-1, data=vb)
    _assert_equals_ref(p, desc, {i: v for _, i, v in vb}, name)


def test_stance_tracking_without_positions_raises():
    f = F.anymal_trot()
    assert f.params_.enable_stance_tracking and f.params_.enable_stance_rpy_tracking   # the reference's defaults
    with pytest.raises(ValueError, match="ee_stance_position_"):
        f.var_bounds_data()
    f.params_.ee_stance_position_ = [[(0.0, 0.0, 0.0)]] * 4                            # too few stance phases
    with pytest.raises(ValueError, match="ee_stance_position_"):
        f.var_bounds_data()


def test_rich_records_hit_what_they_claim():
    """Stance nodes share their variables, the stance loops visit every stance phase once, the waypoints land on
    round(t / poly_dt) (half away from zero) and split into exact and toleranced."""
    desc, vb = FORMS["anymal_trot_rich"]
    rec = {i: np.asarray(v).reshape(-1, 5) for _, i, v in vb}
    lo, up = TowrGpuProblem(desc, device=-1, data=vb).variable_bounds()
    f = rich(F.anymal_trot())
    P = f.params_
    for ee in range(4):
        n_stance = sum(1 for ph in range(P.GetPhaseCount(ee)) if (ph % 2 == 0) == bool(P.ee_in_contact_at_start_[ee]))
        r = rec[2 + ee]
        assert len(r) == 2 * n_stance and (r[:, 1] == 0).all()
        for k in range(n_stance):
            node = int(r[2 * k, 0])
            for dim, want in ((0, 0.125 * k + 0.0625 * ee), (1, -0.25 * ee)):
                a, b = R.column_of(desc, 2 + ee, node, 0, dim), R.column_of(desc, 2 + ee, node + 1, 0, dim)
                assert a is not None and a == b and lo[a] == up[a] == want
            z = R.column_of(desc, 2 + ee, node, 0, 2)
            assert (lo[z], up[z]) == (-1e20, 1e20)
    j = R.column_of(desc, 0, 5, 0, 2)                       # t = 0.52 -> node 5, exact
    assert lo[j] == up[j] == 0.5
    jx, jz = R.column_of(desc, 1, 3, 1, 0), R.column_of(desc, 1, 3, 1, 2)   # t = 0.25 -> 2.5 -> node 3, toleranced
    assert 0.25 / 0.1 == 2.5
    assert (lo[jx], up[jx]) == (0.1 - 0.05, 0.1 + 0.05) and (lo[jz], up[jz]) == (-0.1 - 0.025, -0.1 + 0.025)
    pitch = [R.column_of(desc, 1, node, 0, 1) for node in range(25)]
    assert (lo[pitch] == 0.05).all() and (up[pitch] == 0.05).all()
    # foot 0 tracks its stance angles, the other feet keep the start / goal bounds
    assert len(rec[6]) == 3 * len(rec[2]) // 2 and len(rec[7]) == 6


def test_pins_anymal_trot():
    desc, vb = FORMS["anymal_trot_2p4s"]
    f = _plain(F.anymal_trot())
    p = TowrGpuProblem(desc, device=-1, data=vb)
    lo, up = p.variable_bounds()
    info = p.varset_info()
    assert [k for k, *_ in info[:2]] == [capi.VAR_BASE_LIN, capi.VAR_BASE_ANG]
    c0 = info[0][2]
    init = list(f.initial_base_.lin_p) + list(f.initial_base_.lin_v)
    np.testing.assert_array_equal(lo[c0:c0 + 6], init)      # node 0 of base-lin: pos then vel
    np.testing.assert_array_equal(up[c0:c0 + 6], init)
    n_last = info[0][3] // 6 - 1
    fin = c0 + 6 * n_last
    np.testing.assert_array_equal(lo[fin:fin + 6], list(f.final_base_.lin_p) + [0.0, 0.0, 0.0])
    np.testing.assert_array_equal(up[fin:fin + 6], list(f.final_base_.lin_p) + [0.0, 0.0, 0.0])
    assert (lo[c0 + 6:fin] == -1e20).all() and (up[c0 + 6:fin] == 1e20).all()   # the nodes in between are free
    dm = f.model_.dynamic_model
    fz = dm.mass * dm.g / 4
    for i, (kind, ee, col0, n) in enumerate(info):
        if kind != capi.VAR_EE_FORCE:
            continue
        n_nodes = R.set_layout(desc)[i][5]
        for node in (0, n_nodes - 1):                       # the trot starts and ends with every foot on the ground
            cols = [R.column_of(desc, i, node, deriv, dim) for deriv in range(2) for dim in range(3)]
            np.testing.assert_array_equal(lo[cols], [0.0, 0.0, fz, 0.0, 0.0, 0.0])
            np.testing.assert_array_equal(up[cols], [0.0, 0.0, fz, 0.0, 0.0, 0.0])
    # a deriv = 2 record changes nothing
    extra = [(k, i, np.concatenate([np.asarray(v), [3.0, 2.0, 1.0, -7.0, 7.0]]) if i == 0 else v) for k, i, v in vb]
    q = TowrGpuProblem(desc, device=-1, data=extra)
    for a, b in zip(q.variable_bounds(), (lo, up)):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    # bounds_final_lin_pos_ = {X, Y}: the final z is free
    g = _plain(F.anymal_trot())
    g.params_.bounds_final_lin_pos_ = [0, 1]
    lo2, up2 = TowrGpuProblem(g.to_desc(), device=-1, data=g.var_bounds_data()).variable_bounds()
    assert (lo2[fin + 2], up2[fin + 2]) == (-1e20, 1e20)
    moved = (_bits(lo2) != _bits(lo)) | (_bits(up2) != _bits(up))
    assert moved.sum() == 1 and moved[fin + 2]


def test_pins_schedule_box():
    desc, vb = FORMS["anymal_stairs_gaitopt"]
    p = TowrGpuProblem(desc, device=-1, data=vb)
    lo, up = p.variable_bounds()
    sched = [(ee, c0, n) for k, ee, c0, n in p.varset_info() if k == capi.VAR_EE_SCHEDULE]
    assert len(sched) == 4
    for ee, c0, n in sched:
        assert n == desc.n_phases[ee] - 1
        assert (lo[c0:c0 + n] == 0.2).all() and (up[c0:c0 + n] == 1.0).all()
    assert sum(n for _, _, n in sched) == ((lo == 0.2) & (up == 1.0)).sum()
    q = TowrGpuProblem(desc, device=-1)                      # the box needs no side data
    lo0, up0 = q.variable_bounds()
    for ee, c0, n in sched:
        assert (lo0[c0:c0 + n] == 0.2).all() and (up0[c0:c0 + n] == 1.0).all()


@pytest.mark.parametrize("name", ["anymal_trot_2p4s", "anymal_stairs_gaitopt", "procedural_lineq"])
def test_handle_without_entries_is_unbounded(name):
    desc, data = CASES[name]
    p = TowrGpuProblem(desc, device=-1, data=data)
    lo, up = p.variable_bounds()
    for kind, _, c0, n in p.varset_info():
        if kind != capi.VAR_EE_SCHEDULE:
            assert (lo[c0:c0 + n] == -1e20).all() and (up[c0:c0 + n] == 1e20).all()
    _assert_equals_ref(p, desc, {}, name)


def test_with_moves_only_the_named_columns():
    f = _plain(F.anymal_trot())
    desc, vb = f.to_desc(), f.var_bounds_data()
    p = TowrGpuProblem(desc, device=-1, data=vb)
    base = p.variable_bounds()
    other = F.anymal_trot(goal=(1.6, 0.2, 0.0), start_xy=(0.3, -0.1), goal_yaw=0.2, terrain=F.HeightMap.MakeTerrain(F.HeightMap.SlopeID))
    vb2 = f.var_bounds_data(init=other.init_desc(), terrain=other.terrain_.to_c())
    assert [(k, i, list(v)) for k, i, v in vb2] == [(k, i, list(v)) for k, i, v in _plain(other).var_bounds_data()]
    got = p.variable_bounds_with(vb2)
    _lo, _up = R.varbounds_ref(desc, {i: v for _, i, v in vb2})
    np.testing.assert_array_equal(_bits(got[0]), _bits(_lo))
    np.testing.assert_array_equal(_bits(got[1]), _bits(_up))
    named = np.zeros(p.n, dtype=bool)
    for (_, i, a), (_, i2, b) in zip(vb, vb2):
        assert i == i2
        for ra, rb in zip(np.asarray(a).reshape(-1, 5), np.asarray(b).reshape(-1, 5)):
            assert (ra[:3] == rb[:3]).all()
            col = R.column_of(desc, i, int(ra[0]), int(ra[1]), int(ra[2]))
            if col is not None and (ra[3:] != rb[3:]).any():
                named[col] = True
    moved = (_bits(got[0]) != _bits(base[0])) | (_bits(got[1]) != _bits(base[1]))
    assert moved.any() and (moved <= named).all()
    for a, b in zip(p.variable_bounds(), base):              # the handle's own answer is unchanged
        np.testing.assert_array_equal(_bits(a), _bits(b))
    LO, UP = p.variable_bounds_batch([vb, vb2, []])
    assert LO.shape == UP.shape == (3, p.n)
    np.testing.assert_array_equal(_bits(LO[0]), _bits(base[0]))
    np.testing.assert_array_equal(_bits(UP[1]), _bits(got[1]))
    assert (LO[2] == -1e20).all() and (UP[2] == 1e20).all()


def test_malformed_side_data_is_refused_with_the_set_named():
    desc = CASES["anymal_stairs_gaitopt"][0]
    info = TowrGpuProblem(desc, device=-1).varset_info()
    force = [i for i, (k, *_) in enumerate(info) if k == capi.VAR_EE_FORCE][1]
    sched = [i for i, (k, *_) in enumerate(info) if k == capi.VAR_EE_SCHEDULE][0]
    n_nodes = R.set_layout(desc)[force][5]
    nan = float("nan")
    bad = [(0, [0, 0, 0, 1.0]), (0, [0, 0, 0, 1.0, 2.0, 0.0]),             # a count not divisible by 5
           (1, [0.5, 0, 0, 0.0, 1.0]), (1, [-1, 0, 0, 0.0, 1.0]),           # node: non-integral, out of range
           (force, [n_nodes, 0, 0, 0.0, 1.0]), (force, [0, 3, 0, 0.0, 1.0]), (force, [0, 0.5, 0, 0.0, 1.0]),
           (force, [0, -1, 0, 0.0, 1.0]), (0, [0, 0, 3, 0.0, 1.0]), (0, [0, 0, 1.5, 0.0, 1.0]), (0, [0, 0, -1, 0.0, 1.0]),
           (0, [nan, 0, 0, 0.0, 1.0]), (0, [0, nan, 0, 0.0, 1.0]), (0, [0, 0, nan, 0.0, 1.0]),
           (0, [0, 0, 0, nan, 1.0]), (0, [0, 0, 0, 0.0, nan]),
           (0, [0, 0, 0, 1.0, 0.5]),                                        # lower > upper
           (0, [0, 0, 0, 0.0, 1.0, 0, 2, 0, 2.0, 1.0]),                    # ... even on a record that names nothing
           (sched, [0, 0, 0, 0.0, 1.0]), (len(info), [0, 0, 0, 0.0, 1.0]), (-1, [0, 0, 0, 0.0, 1.0])]   # not a node set
    p = TowrGpuProblem(desc, device=-1)
    for index, rec in bad:
        entry = [(capi.DATA_VAR_BOUNDS, index, np.array(rec, dtype=np.float64))]
        with pytest.raises(TowrGpuError, match=rf"variable set {index}: .*TOWR_DATA_VAR_BOUNDS"):
            TowrGpuProblem(desc, device=-1, data=entry)
        with pytest.raises(TowrGpuError, match=rf"variable set {index}: "):
            p.variable_bounds_with(entry)
    ok = [(capi.DATA_VAR_BOUNDS, force, np.array([n_nodes - 1, 1, 2, -1.0, -1.0]))]     # the last node is in range
    TowrGpuProblem(desc, device=-1, data=ok).variable_bounds()


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "build", "towr_host_check")


@pytest.mark.parametrize("cfg,variant,form", [("anymal", "plain", lambda: _plain(F.anymal_trot())), ("anymal", "rich", lambda: rich(F.anymal_trot())),
                                               ("hopper", "rich", lambda: rich(F.monoped_hopper())),
                                               ("anymal_gait", "rich", lambda: rich(F.anymal_trot(terrain=F.HeightMap.MakeTerrain(F.HeightMap.StairsID),
                                                                                                  optimize_timings=True)))])
def test_cpp_mirror_records_and_bounds_match_python(exe, cfg, variant, form):
    """towr_host_check --varbounds: the C++ mirror's TOWR_DATA_VAR_BOUNDS entries and the bounds of an engine created
    with them, bit for bit."""
    f = form()
    vb = f.var_bounds_data()
    lo, up = TowrGpuProblem(f.to_desc(), device=-1, data=vb).variable_bounds()
    lines = subprocess.check_output([exe, cfg, "--varbounds", variant], text=True).splitlines()
    words = [ln.split() for ln in lines]
    got = [(int(w[1]), np.array([float(v) for v in w[3:]])) for w in words if w[0] == "data"]
    assert all(int(w[2]) == len(w) - 3 for w in words if w[0] == "data")
    assert [i for i, _ in got] == [i for _, i, _ in vb]
    for (i, a), (_, _, b) in zip(got, vb):
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f"records of variable set {i}")
    cols = np.array([[float(w[2]), float(w[3])] for w in words if w[0] == "col"])
    np.testing.assert_array_equal(_bits(cols[:, 0]), _bits(lo))
    np.testing.assert_array_equal(_bits(cols[:, 1]), _bits(up))


# ---- the device entry points' argument checks (nothing runs: fake pointers) ---------------------------------------
def _step_ok(p):
    q, n = C.c_void_p(4096), p.n
    return [q, n, q, n, None, 1.0, None, None, 0, q, n, q, 5 + p.desc.n_varsets]


def _fused_ok(p):
    q, n, m = C.c_void_p(4096), p.n, p.m
    return [q, n, None, None, 0, q, m, 1.0, None, 1.0, None, None, 0, q, q, m, q, m, q, 4 + p.desc.n_constraints,
            q, n, q, 5 + p.desc.n_varsets]


def test_device_calls_refuse_layout_only_handle():
    p = TowrGpuProblem(CASES["monoped_procedural"][0], device=-1)
    q, lib, h = C.c_void_p(4096), p._lib, p._h
    assert lib.towr_gpu_step_batch_device(h, 1, *_step_ok(p), None) == capi.TOWR_ERR_NO_DEVICE
    a = _step_ok(p)
    a[4], a[6], a[7], a[9] = q, q, q, None                   # ALPHA, XL / XU shared, XP = NULL
    assert lib.towr_gpu_step_batch_device(h, 1, *a, None) == capi.TOWR_ERR_NO_DEVICE
    assert lib.towr_gpu_auglag_step_batch_device(h, 1, *_fused_ok(p), None) == capi.TOWR_ERR_NO_DEVICE
    with pytest.raises(TowrGpuError, match=r"towr_gpu error -4"):
        p._check(lib.towr_gpu_step_batch_device(h, 1, *_step_ok(p), None))


def test_argument_errors_are_invalid_before_anything_runs():
    """Every bad operand is TOWR_ERR_INVALID on a layout-only handle, where a good call is TOWR_ERR_NO_DEVICE: the
    checks come first, in the order tests/test_bounds.py pins for the residual call."""
    p = TowrGpuProblem(CASES["monoped_procedural"][0], device=-1)
    q, nul, lib, h = C.c_void_p(4096), None, p._lib, p._h
    n, m, _ = p.sizes()
    lds = 5 + p.desc.n_varsets
    INV = capi.TOWR_ERR_INVALID
    step, fused = lib.towr_gpu_step_batch_device, lib.towr_gpu_auglag_step_batch_device

    def but(ok, *changes):
        a = list(ok)
        for i, v in changes:
            a[i] = v
        return a
    ok = _step_ok(p)
    assert step(h, 1, *ok, None) == capi.TOWR_ERR_NO_DEVICE
    for what, ch in (("null X", [(0, nul)]), ("null D", [(2, nul)]), ("null SUM", [(11, nul)]), ("lds", [(12, lds - 1)]),
                     ("ldx", [(1, n - 1)]), ("ldd", [(3, n - 1)]), ("ldxp", [(10, n - 1)]),
                     ("0 < ldb < n", [(6, q), (7, q), (8, n - 1)]), ("only XL", [(6, q)]), ("only XU", [(7, q)]),
                     ("NaN alpha", [(5, float("nan"))])):
        assert step(h, 1, *but(ok, *ch), None) == INV, what
    assert b"alpha" in lib.towr_gpu_last_error(h)
    assert step(h, -1, *ok, None) == INV
    assert step(h, 1, *but(ok, (4, q), (5, float("nan"))), None) == capi.TOWR_ERR_NO_DEVICE   # ALPHA given: the scalar is unused
    assert step(h, 1, *but(ok, (9, nul), (10, 0)), None) == capi.TOWR_ERR_NO_DEVICE           # XP = NULL needs no ldxp
    assert step(h, 1, *but(ok, (6, q), (7, q), (8, n)), None) == capi.TOWR_ERR_NO_DEVICE
    okf = _fused_ok(p)
    assert fused(h, 1, *okf, None) == capi.TOWR_ERR_NO_DEVICE
    ldr = 4 + p.desc.n_constraints
    for what, ch in (("null X", [(0, nul)]), ("ldx", [(1, n - 1)]), ("null XP", [(20, nul)]), ("ldxp", [(21, n - 1)]),
                     ("null SSUM", [(22, nul)]), ("ldss", [(23, lds - 1)]), ("null RSUM", [(18, nul)]), ("ldrs", [(19, ldr - 1)]),
                     ("ldg", [(15, m - 1)]), ("ldlp", [(17, m - 1)]), ("ldl", [(6, m - 1)]), ("rho", [(7, 0.0)]),
                     ("only GL", [(2, q)]), ("only GU", [(3, q)]), ("0 < ldgb < m", [(2, q), (3, q), (4, m - 1)]),
                     ("only XL", [(10, q)]), ("only XU", [(11, q)]), ("0 < ldxb < n", [(10, q), (11, q), (12, n - 1)]),
                     ("NaN alpha", [(9, float("nan"))])):
        assert fused(h, 1, *but(okf, *ch), None) == INV, what
    assert fused(h, -1, *okf, None) == INV
    assert fused(h, 1, *but(okf, (13, nul), (14, nul), (16, nul)), None) == capi.TOWR_ERR_NO_DEVICE   # F, G, LAMP optional


def test_methods_refuse_bad_operands():
    torch = pytest.importorskip("torch")
    p = TowrGpuProblem(CASES["monoped_procedural"][0], device=-1)
    n, m, _ = p.sizes()
    lds, ldr = 5 + p.desc.n_varsets, 4 + p.desc.n_constraints
    host = lambda cols, dt=torch.float64: torch.zeros((2, cols), dtype=dt)
    with pytest.raises(TowrGpuError, match="expected a HIP device tensor"):
        p.step_batch_device(host(n), host(n), host(lds))
    with pytest.raises(TowrGpuError, match="expected a HIP device tensor"):
        p.auglag_step_batch_device(host(n), host(n), host(lds), host(ldr))

    class OnDevice:
        def __init__(self, t):
            self.dtype, self.shape, self._t = t.dtype, t.shape, t
            self.device = type("D", (), {"type": "cuda", "index": -1})()
        def dim(self): return self._t.dim()
        def stride(self, i): return self._t.stride(i)
        def data_ptr(self): raise AssertionError("operand reached the C-ABI")
    dev = lambda cols: OnDevice(host(cols))
    vec = lambda k: OnDevice(torch.zeros(k, dtype=torch.float64))
    with pytest.raises(TowrGpuError, match="SUM: "):
        p.step_batch_device(dev(n), dev(n), dev(lds - 1))
    with pytest.raises(TowrGpuError, match="D: "):
        p.step_batch_device(dev(n), dev(n - 1), dev(lds))
    with pytest.raises(TowrGpuError, match="XP: "):
        p.step_batch_device(dev(n), dev(n), dev(lds), XP=dev(n - 1))
    with pytest.raises(TowrGpuError, match="D: dtype"):
        p.step_batch_device(dev(n), OnDevice(host(n, torch.float32)), dev(lds))
    with pytest.raises(TowrGpuError, match="both or neither"):
        p.step_batch_device(dev(n), dev(n), dev(lds), XL=vec(n))
    with pytest.raises(TowrGpuError, match="XL: "):
        p.step_batch_device(dev(n), dev(n), dev(lds), XL=vec(n - 1), XU=vec(n))
    with pytest.raises(TowrGpuError, match="XU: "):
        p.step_batch_device(dev(n), dev(n), dev(lds), XL=dev(n), XU=dev(n - 1))
    with pytest.raises(TowrGpuError, match="ALPHA: "):
        p.step_batch_device(dev(n), dev(n), dev(lds), alpha=vec(1))
    with pytest.raises(TowrGpuError, match="SSUM: "):
        p.auglag_step_batch_device(dev(n), dev(n), dev(lds - 1), dev(ldr))
    with pytest.raises(TowrGpuError, match="RSUM: "):
        p.auglag_step_batch_device(dev(n), dev(n), dev(lds), dev(ldr - 1))
