"""A solvable ANYmal trot beside the default one, which is not.

F.anymal_trot() takes goal = (2.1, 0, 0), and bounds_final_lin_pos_ = {X, Y, Z} pins the last base node's z to that 0,
while BaseHeight and the four feet's RangeOfMotion rows need the base about 0.42 above the feet: the default
configuration has no feasible point. Here the goal's z is the standing height -nominal_stance[0][2], read from the model.
The layout (n, m, the pattern) is anymal_trot_2p4s's, so one handle serves both: the default formulation's variable
bounds travel as another problem's XL / XU rows (TowrGpuProblem.variable_bounds_with), and a batch holds a solvable and
an unsolvable problem side by side. Stance tracking is off, as in tests/gpu_helpers._formulation."""
import functools

import numpy as np

from towr2025_amd import TowrGpuProblem
from towr2025_amd import formulation as F

NAME = "anymal_trot_2p4s"
GOAL_XY = (2.1, 0.0)


def z_stand():
    """The standing height of the model: the base above the nominal stance's feet."""
    return -F.RobotModel(F.RobotModel.Anymal).kinematic_model.nominal_stance[0][2]


def formulation(feasible=True):
    f = F.anymal_trot(goal=GOAL_XY + (z_stand(),)) if feasible else F.anymal_trot()
    f.params_.enable_stance_tracking = False
    return f


def bounds_data(feasible=True):
    """The TOWR_DATA_VAR_BOUNDS side data of the feasible or the default formulation."""
    return formulation(feasible).var_bounds_data()


def problem(device=-1):
    """The handle of the feasible formulation (device -1: layout only)."""
    f = formulation(True)
    return TowrGpuProblem(f.to_desc(), device=device, data=f.var_bounds_data())


@functools.lru_cache(maxsize=None)
def bounds():
    """dict(feasible=(lo, up), default=(lo, up)) on a layout-only handle, n doubles each."""
    h = problem(-1)
    out = dict(feasible=h.variable_bounds(), default=h.variable_bounds_with(bounds_data(False)))
    h.close()
    return out


def bounds_rows(kinds):
    """(XL, XU), (len(kinds), n): row b holds the bounds of kinds[b] in ('feasible', 'default')."""
    b = bounds()
    return np.stack([b[k][0] for k in kinds]), np.stack([b[k][1] for k in kinds])


def start(x0, seed=900):
    """The start of DESIGN 4p's runs: x0 + 0.05 randn(seed)."""
    return x0 + 0.05 * np.random.default_rng(seed).standard_normal(x0.size)
