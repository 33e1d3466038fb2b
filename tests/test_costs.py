"""Cost terms (IpoptAdapter::eval_f / eval_grad_f) on the CPU:
  * the oracle's gradient against central differences of its objective (self-consistency pin);
  * the reference quirk EEBasePosCost adds no schedule block (ee_base_pos_cost.cc:150-154);
  * engine_math.h's cost items through the test-only host emulation against the oracle;
  * description validation of cost terms at handle creation (layout-only handle, no GPU).
Parity of the objective is "pinned by FD and the oracle only": the reference's own tests hold no
cost fixtures."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from oracle.oracle import Oracle
from tests.configs import cost_descs, _with_costs
from tests.parity import assert_cost_close
from towr2025_amd import _capi as capi
from towr2025_amd import formulation as F

HERE = os.path.dirname(os.path.abspath(__file__))
COSTS = cost_descs()
D = C.POINTER(C.c_double)


def _fd_grad(o, x, cols, h_rel=1e-4):
    out = np.zeros(len(cols))
    for k, j in enumerate(cols):
        h = h_rel * max(1.0, abs(x[j]))
        xp, xm = x.copy(), x.copy()
        xp[j] += h
        xm[j] -= h
        out[k] = (o.eval_f(xp) - o.eval_f(xm)) / (2 * h)
    return out


def _sched_cols(o, desc):
    cols = []
    for i, (c0, n) in enumerate(o.varset_cols()):
        if desc.varsets[i].kind == capi.VAR_EE_SCHEDULE:
            cols += list(range(c0, c0 + n))
    return cols


@pytest.mark.parametrize("name", sorted(COSTS))
def test_oracle_gradient_matches_fd(name):
    desc = COSTS[name]
    o = Oracle(desc)
    x = o.initial_x() + 0.02 * np.random.default_rng(5).standard_normal(o.n)
    g = o.eval_grad_f(x)
    skip = set(_sched_cols(o, desc)) if desc.optimize_timings else set()   # EEBasePos quirk: below
    cols = [j for j in range(0, o.n, 2) if j not in skip]
    fd = _fd_grad(o, x, cols)
    # central differences with h = 1e-4: truncation O(h^2), cancellation ~ eps |f| / h
    noise = 8 * np.finfo(float).eps * abs(o.eval_f(x)) / 1e-4
    err = np.abs(fd - g[cols]) / (np.maximum(1.0, np.abs(g[cols])) + noise)
    assert err.max() < 2e-5, f"col {cols[err.argmax()]}: FD {fd[err.argmax()]} grad {g[cols][err.argmax()]}"


def test_gait_schedule_gradient_and_eebase_quirk():
    """With phase-duration optimisation: the schedule gradient of Energy/AngularMomentum/Node costs is
    FD-consistent; EEBasePosCost's is missing exactly as in the reference (no schedule block)."""
    f = _with_costs(F.anymal_trot(terrain=F.HeightMap.MakeTerrain(F.HeightMap.StairsID), optimize_timings=True),
                    ee_base_pos=False)
    desc = f.to_desc()
    o = Oracle(desc)
    x = o.initial_x() + 0.01 * np.random.default_rng(3).standard_normal(o.n)
    sc = _sched_cols(o, desc)
    assert sc
    g = o.eval_grad_f(x)
    fd = _fd_grad(o, x, sc, h_rel=1e-6)   # durations enter nonlinearly; f is O(100) here
    assert np.max(np.abs(fd - g[sc]) / np.maximum(1.0, np.abs(g[sc]))) < 5e-5
    # EEBasePos only: its true schedule derivative is not zero, its reported one is
    f2 = _with_costs(F.anymal_trot(terrain=F.HeightMap.MakeTerrain(F.HeightMap.StairsID), optimize_timings=True),
                     costs=[], ee_base_pos=True)
    f2.params_.swing_ee_base_pos_tracking_weight_ = 10.0
    d2 = f2.to_desc()
    o2 = Oracle(d2)
    g2 = o2.eval_grad_f(x)
    assert np.all(g2[sc] == 0.0)
    assert np.max(np.abs(_fd_grad(o2, x, sc, h_rel=1e-6))) > 1e-6


def test_no_costs_is_zero():
    desc = F.anymal_trot().to_desc()
    o = Oracle(desc)
    x = o.initial_x()
    assert o.eval_f(x) == 0.0
    assert not np.any(o.eval_grad_f(x))


@pytest.fixture(scope="module")
def emu():
    lib = os.path.join(HERE, "host_emu", "build", "libemu.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "host_emu")])
    L = C.CDLL(lib)
    L.emu_cost.argtypes = [C.POINTER(capi.ProblemDesc), D, D, D, C.c_char_p, C.c_int]
    L.emu_cost_acc.argtypes = [C.POINTER(capi.ProblemDesc), D, C.c_int, D, D]
    L.emu_limb_sum.argtypes = [D, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_int), D]
    L.emu_limb_sum.restype = None
    return L


@pytest.mark.parametrize("name", sorted(COSTS))
def test_emulated_costs_match_oracle(emu, name):
    desc = COSTS[name]
    o = Oracle(desc)
    for seed in (0, 1, 2):
        x = o.initial_x()
        if seed:
            x = x + 0.05 * np.random.default_rng(seed).standard_normal(o.n)
        f, g = C.c_double(), np.zeros(o.n)
        err = C.create_string_buffer(256)
        assert emu.emu_cost(C.byref(desc), x.ctypes.data_as(D), C.byref(f), g.ctypes.data_as(D), err, 256) == 0, err.value
        assert_cost_close(o.eval_f(x), f.value, o.eval_grad_f(x), g, f"{name} seed {seed}")


@pytest.mark.parametrize("name", sorted(COSTS))
def test_deterministic_gradient_paths_match_oracle(emu, name):
    """The objective kernel's two deterministic gradient accumulations (cost_traj.hip), run on the host with
    the kernel's own emitters: per-entry slots summed per column in the host's fixed order (fixed phase
    durations) and exact fixed-point limbs (phase-duration optimisation; any layout). Both match the oracle;
    the slot path must exist for every fixed-duration config here (ANYmal: 5,976 slots < kCostSlotMax)."""
    desc = COSTS[name]
    o = Oracle(desc)
    for seed in (0, 1):
        x = o.initial_x()
        if seed:
            x = x + 0.05 * np.random.default_rng(seed).standard_normal(o.n)
        f_ref, g_ref = o.eval_f(x), o.eval_grad_f(x)
        got = {}
        for acc in (1, 2):
            f, g = C.c_double(), np.zeros(o.n)
            rc = emu.emu_cost_acc(C.byref(desc), x.ctypes.data_as(D), acc, C.byref(f), g.ctypes.data_as(D))
            if acc == 1 and desc.optimize_timings:
                assert rc == 1   # phase-duration optimisation has no slots: the limbs run
                continue
            assert rc == 0, f"acc {acc}: rc {rc}"
            assert_cost_close(f_ref, f.value, g_ref, g, f"{name} seed {seed} acc {acc}")
            got[acc] = g
        if len(got) == 2:   # the two accumulations agree to rounding
            np.testing.assert_allclose(got[1], got[2], rtol=1e-12, atol=1e-15 * max(1.0, np.abs(g_ref).max()))


def _limb_sum(emu, vals):
    """engine_math.h's own CostLimbEmit and limb_value on one column (emu_limb_sum): (limbs, bad, value)."""
    v = np.ascontiguousarray(vals, dtype=np.float64)
    limbs = (C.c_longlong * 3)()
    bad, value = C.c_int(-1), C.c_double()
    emu.emu_limb_sum(v.ctypes.data_as(D), len(v), limbs, C.byref(bad), C.byref(value))
    return [int(q) for q in limbs], bad.value, value.value


def _limb_ref(vals):
    """The encoding restated with Python integers: per entry the magnitude of v * 2^60 truncated toward zero (exact:
    Fraction of a double is exact), split at bits 42 and 84, the sign applied to each limb; entries that are not
    finite or reach 2^65 set bad and add nothing. (limbs, bad)."""
    acc, bad = [0, 0, 0], 0
    for x in vals:
        x = float(x)
        if not np.isfinite(x) or abs(x) >= 2.0 ** 65:
            bad = 1
            continue
        q = int(abs(Fraction(x)) * 2 ** 60)   # floor of a non-negative rational: truncation toward zero
        parts = [q & (2 ** 42 - 1), (q >> 42) & (2 ** 42 - 1), q >> 84]
        assert parts[2] < 2 ** 42
        sign = -1 if x < 0 else 1
        acc = [a + sign * p for a, p in zip(acc, parts)]
    return acc, bad


def _limb_exact(limbs):
    return Fraction(limbs[0] + limbs[1] * 2 ** 42 + limbs[2] * 2 ** 84, 2 ** 60)


def _check_limb_sum(emu, vals, what):
    """The real code's limbs equal the reference's as integers, in forward, reversed and shuffled order; the value is
    the exact limb sum to 2^-52 relative, and 0 when that sum is 0. The bound is derived, not measured: limb_value is
    (l2 2^24 + l1 2^-18) + l0 2^-60, every product exact while |l_k| < 2^53 (a conversion and a power of two), so there
    are two roundings of at most 2^-53 relative each. The first sum t is a multiple of 2^-18, so it is inexact only
    when |t| >= 2^35, and |l0 2^-60| < 2^-7 cannot cancel against such a t: no rounding error is amplified. (In exact
    arithmetic over 200,000 random triples with |l_k| < 2^53 the worst relative error was 2.12e-16 < 2^-52.)"""
    ref, bad_ref = _limb_ref(vals)
    orders = [np.asarray(vals, dtype=np.float64), np.asarray(vals, dtype=np.float64)[::-1],
              np.random.default_rng(len(vals)).permutation(np.asarray(vals, dtype=np.float64))]
    got = [_limb_sum(emu, o) for o in orders]
    for limbs, bad, value in got:
        assert limbs == ref, f"{what}: limbs {limbs} != {ref}"
        assert bad == bad_ref, f"{what}: bad {bad} != {bad_ref}"
        assert all(abs(q) < 2 ** 53 for q in limbs), f"{what}: a limb sum left the exact range of a double"
        exact = _limb_exact(limbs)
        if exact == 0:
            assert value == 0.0, f"{what}: {value!r} for an exact zero"
        else:
            assert abs(Fraction(value) - exact) <= abs(exact) / 2 ** 52, f"{what}: {value!r} vs {float(exact)!r}"
    assert len({np.float64(g[2]).view(np.uint64) for g in got}) == 1, f"{what}: the value depends on the order"
    return got[0]


def test_limb_accumulation_is_order_independent(emu):
    """The limb arithmetic of cost_traj.hip's phase-duration path, the real code (CostLimbEmit::operator(), limb_of and
    limb_value of engine_math.h through the host emulation's emu_limb_sum) against a Python big-integer restatement:
    random entries over a wide magnitude range added in different orders give the same limbs, hence the same bits, and
    the value is the exact sum to within the 2^-60 resolution per entry; then the boundaries of the encoding."""
    rng = np.random.default_rng(11)
    v = rng.standard_normal(500) * 10.0 ** rng.integers(-14, 12, 500)
    v[::7] *= -1
    a, bad, value = _check_limb_sum(emu, v, "wide range")
    assert bad == 0
    exact = sum(int(round(x * 2.0 ** 60)) for x in v)   # python ints: the exact fixed-point sum (to rounding per entry)
    got = a[0] + (a[1] << 42) + (a[2] << 84)
    assert abs(got - exact) <= len(v)

    one, top = 2.0 ** -60, float(np.nextafter(2.0 ** 65, 0.0))
    # one unit of the resolution, either sign
    assert _check_limb_sum(emu, [one], "+unit")[0] == [1, 0, 0]
    assert _check_limb_sum(emu, [-one], "-unit")[0] == [-1, 0, 0]
    # below the resolution: dropped, and not bad (a subnormal and the zeros too)
    for x in (float(np.nextafter(one, 0.0)), 2.0 ** -61, -2.0 ** -61, 5e-324, -2.2e-308, 0.0, -0.0):
        assert _check_limb_sum(emu, [x], f"dropped {x!r}") == ([0, 0, 0], 0, 0.0)
    # the largest accepted magnitude, (2^53 - 1) 2^12: times 2^60 it is (2^53 - 1) 2^72, whose bits from 84 up are the
    # mantissa's top 41 and whose bits 72..83 (its low 12) are the top of limb 1; the value is exact
    limbs, bad, value = _check_limb_sum(emu, [top], "largest accepted")
    assert bad == 0 and value == top and limbs[2] == 2 ** 41 - 1 and limbs[1] == (2 ** 12 - 1) << 30
    assert _check_limb_sum(emu, [-top], "largest accepted, negative")[2] == -top
    # refused: each sets bad and adds nothing, whatever stands beside it
    for x in (2.0 ** 65, -2.0 ** 65, 1e30, np.inf, -np.inf, np.nan):
        assert _limb_sum(emu, [x])[:2] == ([0, 0, 0], 1), f"{x!r} was not refused"
        limbs, bad, _ = _check_limb_sum(emu, [1.5, x, -0.25], f"refused {x!r} among others")
        assert bad == 1 and limbs == _limb_ref([1.5, -0.25])[0]
    # limb boundaries: the lowest bit of limbs 1 and 2, and the bits just under them
    assert _check_limb_sum(emu, [2.0 ** -18], "limb 1 unit")[0] == [0, 1, 0]
    assert _check_limb_sum(emu, [2.0 ** 24], "limb 2 unit")[0] == [0, 0, 1]
    assert _check_limb_sum(emu, [2.0 ** -18 - one], "limb 0 full")[0] == [2 ** 42 - 1, 0, 0]
    assert _check_limb_sum(emu, [-(2.0 ** 24 - 2.0 ** -18)], "limb 1 full, negative")[0] == [0, -(2 ** 42 - 1), 0]
    # cancellations: the sign is applied per limb, so sums of mixed signs leave limbs of mixed signs
    for x in (1.0, 3.7e-9, 12345.678, top, 2.0 ** -18 + one):
        assert _check_limb_sum(emu, [x, -x], f"{x!r} - itself") == ([0, 0, 0], 0, 0.0)
        limbs, bad, value = _check_limb_sum(emu, [x, -x, 3 * one], f"{x!r} - itself + tiny")
        assert limbs == [3, 0, 0] and value == 3 * one
    limbs, bad, value = _check_limb_sum(emu, [2.0 ** 24, -(2.0 ** 24 - 2.0 ** -18)], "l2 = 1, l1 = -(2^42 - 1)")
    assert limbs == [0, -(2 ** 42 - 1), 1] and value == 2.0 ** -18
    limbs, bad, value = _check_limb_sum(emu, [2.0 ** 24, -(2.0 ** 24 - 2.0 ** -18), -one], "... and l0 = -1")
    assert limbs == [-1, -(2 ** 42 - 1), 1] and value == 2.0 ** -18 - one
    # the header's "fewer than 2^11 entries": 2047 entries of the largest accepted magnitude keep every |l_k| < 2^53
    # (asserted in _check_limb_sum), one sign and mixed signs
    limbs, bad, value = _check_limb_sum(emu, [top] * 2047, "2047 largest")
    assert bad == 0 and limbs[2] == 2047 * (2 ** 41 - 1)
    _check_limb_sum(emu, [top if i % 3 else -top for i in range(2047)], "2047 largest, mixed signs")
    _check_limb_sum(emu, [2.0 ** -18 - one] * 2047, "2047 full low limbs")


def _create_layout(desc):
    lib = capi.load_library()
    h = C.c_void_p()
    rc = lib.towr_gpu_create(C.byref(desc), -1, C.byref(h))
    if rc == 0:
        lib.towr_gpu_destroy(h)
    return rc, lib.towr_gpu_last_error(None).decode()


@pytest.mark.parametrize("field,value", [("kind", 9), ("ip0", 6), ("ip1", 2), ("ip2", 3), ("ee", 7)])
def test_bad_cost_terms_rejected(field, value):
    desc = COSTS["anymal_all_costs"]
    d = capi.ProblemDesc.from_buffer_copy(desc)
    c = d.costs[0]   # a NodeCost (forces)
    assert c.kind == capi.COST_NODE
    if field == "kind":
        c.kind = value
    elif field == "ee":
        c.ee = value
    else:
        c.ip[int(field[2])] = value
    rc, msg = _create_layout(d)
    assert rc == capi.TOWR_ERR_INVALID, msg
    rc, _ = _create_layout(desc)
    assert rc == 0
