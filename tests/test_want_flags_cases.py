"""What the (case, B) list of tests/want_flags_cases.py reaches with want_g = 0 or want_jac = 0, from kernel_path,
kernels() and step_launches() of the layout-only handles of exactly that list (as
test_shape_sweep.test_seed_lists_reach_the_large_batch_launch_shapes does for B = 65 with both flags on), and that no
pair of it sends a flag off to a fixed-gait layout at B >= kSplitBatch. tests/test_gpu_want_flags.py runs the list."""
from tests.test_shape_sweep import DYN, FDISC, ROM, STAGE_OVERFLOW, TQDISC, _large_batch_shapes
from tests.want_flags_cases import CASE_B, CASES, FIXED_B, GAIT_B, NAMED, SPLIT, TERRAIN_CASES, batch_sizes, desc_of, optimizes
from towr2025_amd import TowrGpuProblem

MISC = 4   # the small kinds' launch class
RF = "the fused RangeOfMotion + FDISC launch, then Dynamic and the small kinds on the same stream"
EULER = "per-class Euler launches"
ROTVEC = "the RotVec pre-pass and per-class launches"
SINGLE = "every record part in one launch, the small kinds inside the composer launch"
STREAM_SHAPES = ("FDISC streamed beside RangeOfMotion / Dynamic", "FDISC + TQDISC streamed", "TQDISC streamed without an FDISC grid",
                 "RangeOfMotion / Dynamic streamed alone", "tile-path FDISC or TQDISC beside streamed classes")


def _shapes(case, B):
    """The launch shapes of (case, B) by name (towr_gpu.hip launch_classes / launch_stream_path)."""
    d = desc_of(case)
    p = TowrGpuProblem(d, device=-1)
    pt = [p.kernel_path(k) for k in (DYN, ROM, FDISC, TQDISC)]
    kern = {k: nt for k, _, nt, _ in p.kernels()}
    names = {k: name for k, name, _, _ in p.kernels()}
    launches = p.step_launches()
    large = _large_batch_shapes(bool(d.optimize_timings), d.angular_rep == 1, pt, kern, launches, case)
    if not d.optimize_timings:
        assert B < SPLIT, (case, B)
        fused = [k for k in launches if k >= 5]
        if fused:   # below kSplitBatch a batch with a fusion group runs serially
            assert [names[k] for k in fused] == ["range_of_motion+force_discretized"] and launches[0] == fused[0], case
            assert {DYN, MISC} <= set(launches[1:]) and ROM not in launches and FDISC not in launches, case
            return [RF]
        if d.angular_rep == 1:
            assert DYN in launches and p.kernel_path(DYN) == 0, case
            return [ROTVEC]
        assert DYN in launches and ROM in launches, case
        return [EULER]
    assert any(k == 1 for k in pt), case
    if B >= SPLIT:
        return [f"B = {B}: {sh}" for sh in large]
    assert MISC in kern, case   # below kSplitBatch the small kinds join the composer launch
    return [SINGLE]


def test_case_list_reaches_the_launch_shapes_with_a_flag_off():
    reached = {}
    for case, B in CASE_B:
        for sh in _shapes(case, B):
            reached.setdefault(sh, {}).setdefault(B, []).append(case)
    for sh in sorted(reached):
        print(sh, {B: cases for B, cases in sorted(reached[sh].items())})
    below = SPLIT - 1
    assert {93, STAGE_OVERFLOW, "anymal_trot_2p4s"} <= set(reached[RF][below]) and len(reached[RF][below]) >= 7
    assert reached[RF][3] == reached[RF][below]
    assert len(reached[EULER][below]) >= 2 and reached[EULER][3] == reached[EULER][below]
    assert "anymal_trot_rotvec" in reached[ROTVEC][below] and len(reached[ROTVEC][below]) >= 7
    assert reached[ROTVEC][3] == reached[ROTVEC][below]
    assert {"anymal_stairs_gaitopt", "anymal_gait_torque"} <= set(reached[SINGLE][below]) and len(reached[SINGLE][below]) >= 12
    assert reached[SINGLE][3] == reached[SINGLE][below]
    above = {sh: set(reached.get(f"B = {SPLIT + 1}: {sh}", {}).get(SPLIT + 1, [])) for sh in STREAM_SHAPES}
    assert len(above["FDISC streamed beside RangeOfMotion / Dynamic"]) >= 3
    assert {0, 191} <= above["FDISC + TQDISC streamed"]
    assert {10, 94, 126} <= above["TQDISC streamed without an FDISC grid"]
    assert {45, 83} <= above["RangeOfMotion / Dynamic streamed alone"]
    assert {13, 86, 131} <= above["tile-path FDISC or TQDISC beside streamed classes"]


def test_no_flag_off_on_a_fixed_gait_at_or_above_the_split():
    """By construction over the same list: a fixed-gait layout never meets B >= kSplitBatch, every case runs 3 and 63,
    the phase-duration cases also 65, and the per-problem terrain cases are one of each kind below the split."""
    assert len(set(CASE_B)) == len(CASE_B) and {c for c, _ in CASE_B} == set(CASES) and set(NAMED) <= set(CASES)
    assert max(FIXED_B) < SPLIT <= max(GAIT_B) and SPLIT - 1 in FIXED_B and set(FIXED_B) < set(GAIT_B)
    for case, B in CASE_B + TERRAIN_CASES:
        assert optimizes(case) or B < SPLIT, (case, B)
        assert bool(desc_of(case).optimize_timings) == optimizes(case)
    for case in CASES:
        assert [B for c, B in CASE_B if c == case] == list(batch_sizes(case)) == list(GAIT_B if optimizes(case) else FIXED_B)
    assert [optimizes(c) for c, _ in TERRAIN_CASES] == [False, True] and all(B < SPLIT for _, B in TERRAIN_CASES)
