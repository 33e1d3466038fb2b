"""The (case, B) list of the device-batch tests with want_g = 0 or want_jac = 0 (tests/test_gpu_want_flags.py, GPU) and
of the table of launch shapes that list reaches (tests/test_want_flags_cases.py, CPU); not a test.

Cases: the shapes of the seeded sweep that run on the GPU (tests/test_shape_sweep.py GPU_CASES: GPU_SEEDS,
FIXED_GAIT_SEEDS, STAGE_OVERFLOW) and four named parity configurations. Batch sizes: with fixed phase durations 3 and
63, the largest below kSplitBatch = 64 (towr_gpu.hip), ragged whether a block takes 16, 4 or 1 problems; under
phase-duration optimisation also 65, the two- and three-chain path. A layout with fixed phase durations never gets
B >= 64 with a flag off: that is the shape of the open intermittent illegal access, which these tests
stay away from. Every case runs every one of its batch sizes (no subset)."""
import functools

from tests.configs import config_descs
from tests.shape_sweep import make
from tests.test_shape_sweep import GPU_CASES, STAGE_OVERFLOW, _stage_overflow_formulation

NAMED = ["anymal_trot_2p4s", "anymal_trot_rotvec", "anymal_stairs_gaitopt", "anymal_gait_torque"]
CASES = list(GPU_CASES) + NAMED
SPLIT = 64                       # kSplitBatch (towr_gpu.hip)
FIXED_B = (3, SPLIT - 1)
GAIT_B = (3, SPLIT - 1, SPLIT + 1)
TERRAIN_CASES = [("anymal_trot_2p4s", SPLIT - 1), ("anymal_stairs_gaitopt", SPLIT - 1)]   # per-problem terrains


@functools.lru_cache(maxsize=None)
def desc_of(case):
    if case in NAMED:
        return config_descs()[case]
    return _stage_overflow_formulation().to_desc() if case == STAGE_OVERFLOW else make(case)[0].to_desc()


def optimizes(case):
    """Whether the case optimises the phase durations (else: a fixed gait)."""
    return bool(desc_of(case).optimize_timings)


def batch_sizes(case):
    return GAIT_B if optimizes(case) else FIXED_B


CASE_B = [(case, B) for case in CASES for B in batch_sizes(case)]
