"""What the LDS emitters (tile_emit.h TileEmit, tiles.hip TileEmitPre, misc_body) take for granted about the tile
tables, on the CPU: tests/host_emu/emu.hip emu_tile_bounds walks every tile of a layout lane by lane as the kernels do
(the slot groups each emitter loads, ring prefetch and preloads included; the position of every candidate; the dummy
slots; the g rows and Dynamic's scratch inside the class's LDS; the small-kind waves back to back) and returns the
number of the first expectation that does not hold. The expectations are restated there from the emitters, not from
build_layout's arithmetic. The emulation's value check (test_shape_sweep.py) drops a dummy-slot store and never looks
at the LDS layout, so until now these held only as far as GPU parity ran a shape.

Seeds 0..199 of the sweep, STAGE_OVERFLOW, the four slot-limit shapes and every parity configuration."""
import ctypes as C

import numpy as np
import pytest

from tests import jp_emu
from tests.configs import anymal_trot_slot_limit, config_descs
from tests.shape_sweep import make
from tests.test_shape_sweep import STAGE_OVERFLOW, _stage_overflow_formulation
from towr2025_amd import TowrGpuProblem, _capi as capi

CONFIGS = config_descs()
SLOT_LIMIT = anymal_trot_slot_limit()
CASES = [f"seed_{s}" for s in range(200)] + [STAGE_OVERFLOW] + sorted(SLOT_LIMIT) + sorted(CONFIGS)
OUT = ("tiles", "lanes", "present", "absent", "direct", "covered", "spare_groups", "lds_end")


def _desc(case):
    if case.startswith("seed_"):
        return make(int(case[5:]))[0].to_desc()
    if case == STAGE_OVERFLOW:
        return _stage_overflow_formulation().to_desc()
    return SLOT_LIMIT[case] if case in SLOT_LIMIT else CONFIGS[case]


def tile_bounds(desc):
    """(return code, message, dict of OUT) of emu_tile_bounds on a description."""
    L = jp_emu.lib()
    L.emu_tile_bounds.argtypes = [C.POINTER(capi.ProblemDesc), C.c_void_p, C.c_char_p, C.c_int]
    out = np.full(len(OUT), -1, dtype=np.int64)
    err = C.create_string_buffer(512)
    rc = L.emu_tile_bounds(C.byref(desc), out.ctypes.data, err, 512)
    return rc, err.value.decode(), dict(zip(OUT, (int(v) for v in out)))


@pytest.mark.parametrize("case", CASES)
def test_tile_tables_are_what_the_emitters_assume(case):
    desc = _desc(case)
    rc, msg, st = tile_bounds(desc)
    assert rc == 0, f"{case}: check {rc}: {msg}"
    p = TowrGpuProblem(desc, device=-1)
    n, m, nnz = p.sizes()
    # the tiles' values are the whole pattern, each position one present candidate; every spare group still there
    assert st["covered"] == nnz and st["present"] == nnz, (case, st, nnz)
    assert st["tiles"] > 0 and st["lanes"] > 0 and st["spare_groups"] >= 0, (case, st)
    assert st["direct"] == 0 or desc.optimize_timings, (case, st)


def test_the_walk_reaches_every_emitter():
    """The case list is worth its minute only while it holds absent candidates (dummy slots), direct ranges (the
    phase-duration tiles), Dynamic tiles with and without the RotVec pre-pass, and layouts whose furthest slot load is
    the last group but three or closer (the ring's depth against kSlotSpare)."""
    absent = direct = 0
    closest = 1 << 30
    for case in ("seed_0", "seed_13", "seed_93", "anymal_trot_2p4s", "anymal_trot_rotvec", "anymal_stairs_gaitopt", "hopper_torque_node"):
        rc, msg, st = tile_bounds(_desc(case))
        assert rc == 0, f"{case}: check {rc}: {msg}"
        absent += st["absent"]
        direct += st["direct"]
        closest = min(closest, st["spare_groups"])
    assert absent > 0 and direct > 0 and closest <= 3, (absent, direct, closest)
