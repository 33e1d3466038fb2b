"""ifopt::Problem-shaped host API over the HIP engine's C-ABI (include/towr_gpu.h).

Mirrors what IPOPT reaches through ifopt's IpoptAdapter for the hot path:
  GetNumberOfOptimizationVariables / GetNumberOfConstraints / nonzeros  -> sizes()
  GetVariableValues (starting point)                                    -> initial_x()
  EvalConstraints(x)                         (IpoptAdapter::eval_g)     -> eval_g(x)
  GetJacobianOfConstraints structure         (eval_jac_g, values=NULL)  -> jac_structure()
  EvalNonzerosOfJacobian(x)                  (eval_jac_g, values!=NULL) -> eval_jac_values(x)
  EvaluateCostFunction / ...Gradient         (eval_f / eval_grad_f)     -> eval_f(x) / eval_grad_f(x)
  SaveTrajectoryToCSV's samples              (save_data.cpp:9-130)      -> sample_trajectory(x, dt)
plus the batched, device-resident entry points used by bench.py.

Every evaluation runs on the GPU through libtowr_gpu.so; there is no CPU path. A missing or
unloadable extension raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as capi


class TowrGpuError(RuntimeError):
    pass


def _check_tensor(t, what, min_cols, device=None):
    """A device batch operand: float64, on a HIP device (the handle's), rows contiguous (stride(1) == 1),
    at least min_cols columns. The C-ABI sees only a pointer and a leading dimension, so a float32 or
    strided tensor would otherwise be read or written out of bounds."""
    import torch
    if t.dtype != torch.float64:
        raise TowrGpuError(f"{what}: dtype {t.dtype}, expected torch.float64")
    if t.device.type != "cuda":
        raise TowrGpuError(f"{what}: tensor on {t.device}, expected a HIP device tensor")
    if device is not None and t.device.index != device:
        raise TowrGpuError(f"{what}: tensor on {t.device}, the handle is on device {device}")
    if t.dim() == 2:
        if t.shape[1] > 1 and t.stride(1) != 1:
            raise TowrGpuError(f"{what}: stride(1) = {t.stride(1)}, expected 1 (row-major rows)")
        if t.shape[1] < min_cols:
            raise TowrGpuError(f"{what}: {t.shape[1]} columns, needs >= {min_cols}")
        if t.shape[0] > 1 and t.stride(0) < min_cols:
            raise TowrGpuError(f"{what}: leading dimension {t.stride(0)} < {min_cols}")
    elif t.dim() != 1:
        raise TowrGpuError(f"{what}: expected a 1-D or 2-D tensor")


def _opt(t):
    """(pointer, leading dimension) of a 2-D operand, which may be optional: None is (NULL, 0), which the C-ABI never
    touches. Call sites unpack it in place: *_opt(X)."""
    return (C.c_void_p(None), 0) if t is None else (C.c_void_p(t.data_ptr()), t.stride(0))


def _check_per_problem(t, what, B, device):
    """An optional 1-D operand with one entry per problem, such as F: None, or >= B contiguous entries."""
    if t is None:
        return
    _check_tensor(t, what, 1, device)
    if t.dim() != 1 or t.shape[0] < B or (B > 1 and t.stride(0) != 1):
        raise TowrGpuError(f"{what}: expected a contiguous 1-D tensor of >= B entries")


AL_PARAM_DEFAULTS = dict(mem=5, max_inner=50, max_outer=20, c1=1e-4, shrink=0.5, alpha0=1.0, alpha_min=1e-10, curv_eps=1e-8,
                         rho0=10.0, rho_grow=10.0, rho_max=1e8, eta0=0.1, eta_shrink=0.1, eta_star=1e-6,
                         omega0=0.1, omega_shrink=0.1, omega_star=1e-6)


def alsolve_params(**kw) -> capi.AlSolveParams:
    """towr_alsolve_params_t from keywords (AL_PARAM_DEFAULTS for the rest); the C-ABI checks the ranges."""
    unknown = set(kw) - set(AL_PARAM_DEFAULTS)
    if unknown:
        raise TowrGpuError(f"alsolve_params: unknown field(s) {sorted(unknown)}")
    return capi.AlSolveParams(**{**AL_PARAM_DEFAULTS, **kw})


def alsolve_stop_params(acc_eta=0.0, acc_omega=0.0, acc_iters=0, infeas_keep=1.0, infeas_rho=float("inf")) -> capi.AlSolveStop:
    """towr_alsolve_stop_t: the acceptable rule (acc_iters = 0: off) and the infeasible rule (infeas_rho = inf: off); the
    defaults switch both off. The C-ABI checks the ranges."""
    return capi.AlSolveStop(acc_eta=float(acc_eta), acc_omega=float(acc_omega), acc_iters=int(acc_iters), reserved=0,
                            infeas_keep=float(infeas_keep), infeas_rho=float(infeas_rho))


def gn_params(ncg=8, mu=0.0, tol=0.0) -> capi.GnParams:
    """towr_gn_params_t: at most ncg CG steps, the damping mu, the relative residual tolerance tol; the C-ABI checks
    the ranges."""
    return capi.GnParams(ncg=int(ncg), reserved=0, mu=float(mu), tol=float(tol))


class AlSolveState:
    """The tensors of towr_alsolve_state_t (towr_gpu.h) for B problems and `mem` pairs; allocate() makes them (zeros) on
    the problem's device. X holds the starting points and LAM the starting multipliers before alsolve_init."""
    _ROWS = ("X", "GR", "XC", "GRC", "D", "LAM", "LAMP", "HS", "HY", "SCAL", "RSUM", "SSUM", "DSUM", "USUM", "LSUM")
    _VECS = ("ALPHA", "RHO", "FC")

    @classmethod
    def allocate(cls, p, B, mem):
        import torch
        dev = torch.device("cuda", p.device)
        z = lambda r, c: torch.zeros((r, c), dtype=torch.float64, device=dev)
        s = cls()
        s.B, s.mem = B, mem
        for k in ("X", "GR", "XC", "GRC", "D"):
            setattr(s, k, z(B, p.n))
        s.LAM, s.LAMP = z(B, p.m), z(B, p.m)
        s.HS, s.HY = z(B * mem, p.n), z(B * mem, p.n)
        s.HMETA = torch.zeros(2 * B, dtype=torch.int32, device=dev)
        s.ISTATE = torch.zeros(4 * B, dtype=torch.int32, device=dev)
        for k in cls._VECS:
            setattr(s, k, torch.zeros(B, dtype=torch.float64, device=dev))
        s.SCAL, s.LSUM, s.USUM, s.DSUM = z(B, 8), z(B, 8), z(B, 6), z(B, 5)
        s.RSUM, s.SSUM = z(B, 4 + p.desc.n_constraints), z(B, 5 + p.desc.n_varsets)
        return s

    def tensors(self):
        return {k: getattr(self, k) for k in self._ROWS + self._VECS + ("HMETA", "ISTATE")}

    def clone(self):
        s = type(self)()
        s.B, s.mem = self.B, self.mem
        for k, t in self.tensors().items():
            setattr(s, k, t.clone())
        return s


class TowrGpuProblem:
    """`data`: side data of towr_gpu_create_ex, [(towr_data_kind, index, float64 array)]: the matrix M of
    each LinearEqualityConstraint (capi.DATA_LINEAR_M, constraint index, rows x n_set row-major) and the
    wrapped set's bounds of each SoftConstraint term (capi.DATA_SOFT_BOUNDS, cost index, [lower, upper]); optionally
    what the bounds calls need (capi.DATA_BOUNDS, NlpFormulation.bounds_data(); capi.DATA_VAR_BOUNDS, variable set
    index, records (node, deriv, dim, lower, upper), NlpFormulation.var_bounds_data())."""

    def __init__(self, desc: capi.ProblemDesc, device: int = 0, data=None):
        self._lib = capi.load_library()
        self.desc = desc
        self.device = device
        h = C.c_void_p()
        arr, keep = capi.side_data(data)
        rc = self._lib.towr_gpu_create_ex(C.byref(desc), len(data or []), arr, device, C.byref(h))
        if rc != capi.TOWR_OK:
            raise TowrGpuError(f"towr_gpu_create failed ({rc}): {self._lib.towr_gpu_last_error(None).decode()}")
        self._h = h
        self._pinned = {}
        n, m, nnz = C.c_int32(), C.c_int32(), C.c_int64()
        self._check(self._lib.towr_gpu_sizes(h, C.byref(n), C.byref(m), C.byref(nnz)))
        self.n, self.m, self.nnz = n.value, m.value, nnz.value

    def _check(self, rc):
        if rc != capi.TOWR_OK:
            raise TowrGpuError(f"towr_gpu error {rc}: {self._lib.towr_gpu_last_error(self._h).decode()}")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.towr_gpu_destroy(self._h)   # unregisters the registered host arrays
            self._h = None
            self._pinned = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -------------------------------------------------------------------- structure ----------
    def sizes(self):
        return self.n, self.m, self.nnz

    def initial_x(self) -> np.ndarray:
        x = np.zeros(self.n)
        self._check(self._lib.towr_gpu_initial_x(self._h, capi.dptr(x)))
        return x

    def initial_x_for(self, init: capi.InitDesc, terrain: capi.Terrain) -> np.ndarray:
        """x0 of another start/goal/terrain instance on this layout (batch harness)."""
        x = np.zeros(self.n)
        self._check(self._lib.towr_gpu_initial_x_for(self._h, C.byref(init), C.byref(terrain), capi.dptr(x)))
        return x

    def varset_info(self):
        out = []
        for i in range(self.desc.n_varsets):
            k, e, c0, n = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
            self._check(self._lib.towr_gpu_varset_info(self._h, i, C.byref(k), C.byref(e), C.byref(c0), C.byref(n)))
            out.append((k.value, e.value, c0.value, n.value))
        return out

    def constraint_info(self):
        """[(kind, ee, row0, rows)] of the constraint sets in description order; the hard sets tile [0, m), a soft
        set has rows = 0."""
        out = []
        for i in range(self.desc.n_constraints):
            k, e, r0, n = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
            self._check(self._lib.towr_gpu_constraint_info(self._h, i, C.byref(k), C.byref(e), C.byref(r0), C.byref(n)))
            out.append((k.value, e.value, r0.value, n.value))
        return out

    def constraint_bounds(self):
        """(lower, upper), m doubles each: every constraint set's GetBounds() in row order, at the description's x0
        and terrain (IpoptAdapter::get_bounds_info for g). Unbounded sides are +-1e20."""
        lo, up = np.zeros(self.m), np.zeros(self.m)
        self._check(self._lib.towr_gpu_constraint_bounds(self._h, capi.dptr(lo), capi.dptr(up)))
        return lo, up

    def constraint_bounds_for(self, init: capi.InitDesc, terrain: capi.Terrain):
        """The bounds of another start/goal/terrain instance on this layout (they differ on node-Torque rows only)."""
        lo, up = np.zeros(self.m), np.zeros(self.m)
        self._check(self._lib.towr_gpu_constraint_bounds_for(self._h, C.byref(init), C.byref(terrain),
                                                             capi.dptr(lo), capi.dptr(up)))
        return lo, up

    def variable_bounds(self):
        """(lower, upper), n doubles each: the bounds on x in ifopt column order (IpoptAdapter::get_bounds_info for x),
        from the TOWR_DATA_VAR_BOUNDS entries given at creation and, for the schedule sets, bound_phase_duration.
        Unbounded sides are +-1e20."""
        lo, up = np.zeros(self.n), np.zeros(self.n)
        self._check(self._lib.towr_gpu_variable_bounds(self._h, capi.dptr(lo), capi.dptr(up)))
        return lo, up

    def variable_bounds_with(self, data):
        """The bounds of another instance on this layout: `data` as the constructor's, its DATA_VAR_BOUNDS entries used
        instead of the creation's (NlpFormulation.var_bounds_data with that instance's init / terrain)."""
        lo, up = np.zeros(self.n), np.zeros(self.n)
        arr, keep = capi.side_data(data)
        self._check(self._lib.towr_gpu_variable_bounds_with(self._h, len(data or []), arr, capi.dptr(lo), capi.dptr(up)))
        del keep
        return lo, up

    def variable_bounds_batch(self, datas):
        """variable_bounds_with of every entry of `datas`: (lower, upper), (B, n) arrays (the per-problem rows of
        step_batch_device)."""
        lo, up = np.zeros((len(datas), self.n)), np.zeros((len(datas), self.n))
        for b, data in enumerate(datas):
            lo[b], up[b] = self.variable_bounds_with(data)
        return lo, up

    def jac_structure(self):
        r = np.zeros(self.nnz, dtype=np.int32)
        c = np.zeros(self.nnz, dtype=np.int32)
        self._check(self._lib.towr_gpu_jac_structure(self._h, capi.iptr(r), capi.iptr(c)))
        return r, c

    def jac_csr(self):
        rp = np.zeros(self.m + 1, dtype=np.int64)
        c = np.zeros(self.nnz, dtype=np.int32)
        self._check(self._lib.towr_gpu_jac_csr(self._h, capi.lptr(rp), capi.iptr(c)))
        return rp, c

    # -------------------------------------------------------------------- evaluation ---------
    def eval_g(self, x) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float64)
        g = np.zeros(self.m)
        self._check(self._lib.towr_gpu_eval_g(self._h, capi.dptr(x), capi.dptr(g)))
        return g

    def eval_jac_values(self, x) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float64)
        v = np.zeros(self.nnz)
        self._check(self._lib.towr_gpu_eval_jac_values(self._h, capi.dptr(x), capi.dptr(v)))
        return v

    def eval_g_jac(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        g, v = np.zeros(self.m), np.zeros(self.nnz)
        self._check(self._lib.towr_gpu_eval_g_jac(self._h, capi.dptr(x), capi.dptr(g), capi.dptr(v)))
        return g, v

    def eval_g_keep_jac(self, x) -> np.ndarray:
        """g at x, the Jacobian kept on the device for eval_jac_values_kept (IPOPT's eval_g at a new x)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        g = np.zeros(self.m)
        self._check(self._lib.towr_gpu_eval_g_keep_jac(self._h, capi.dptr(x), capi.dptr(g)))
        return g

    def eval_jac_values_kept(self, x) -> np.ndarray:
        """The Jacobian values at x: the kept ones when x is bit-identical to eval_g_keep_jac's, else evaluated."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        v = np.zeros(self.nnz)
        self._check(self._lib.towr_gpu_eval_jac_values_kept(self._h, capi.dptr(x), capi.dptr(v)))
        return v

    def eval_g_jac_into(self, x, g, v):
        """eval_g + eval_jac_g into caller arrays (contiguous float64): with x, g, v registered
        (register_host) the transfers run in place, as an IPOPT driver reusing its buffers would."""
        for a, k in ((x, self.n), (g, self.m), (v, self.nnz)):
            if a.dtype != np.float64 or not a.flags.c_contiguous or a.size < k:
                raise TowrGpuError("eval_g_jac_into: contiguous float64 arrays of n / m / nnz entries expected")
        self._check(self._lib.towr_gpu_eval_g_jac(self._h, capi.dptr(x), capi.dptr(g), capi.dptr(v)))

    def register_host(self, a):
        """Page-lock a contiguous numpy array for in-place host transfers (towr_gpu_register_host)."""
        if not a.flags.c_contiguous:
            raise TowrGpuError("register_host: contiguous array expected")
        self._check(self._lib.towr_gpu_register_host(self._h, C.c_void_p(a.ctypes.data), a.nbytes))
        self._pinned[a.ctypes.data] = a   # keep it alive while registered

    def unregister_host(self, a):
        self._check(self._lib.towr_gpu_unregister_host(self._h, C.c_void_p(a.ctypes.data)))
        self._pinned.pop(a.ctypes.data, None)

    def eval_f(self, x) -> float:
        """Objective (IpoptAdapter::eval_f): the sum of every cost term."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        f = C.c_double()
        self._check(self._lib.towr_gpu_eval_f(self._h, capi.dptr(x), C.byref(f)))
        return f.value

    def eval_grad_f(self, x) -> np.ndarray:
        """Dense objective gradient (IpoptAdapter::eval_grad_f)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        grad = np.zeros(self.n)
        self._check(self._lib.towr_gpu_eval_grad_f(self._h, capi.dptr(x), capi.dptr(grad)))
        return grad

    def eval_cost_batch_device(self, X, F, GRAD=None, stream=None):
        """Device batch objective on torch HIP tensors: X (B, ldx) -> F (B,), GRAD (B, ldgrad) or None."""
        import torch
        B = X.shape[0]
        _check_tensor(X, "X", self.n, self.device)
        _check_per_problem(F, "F", B, self.device)
        if GRAD is not None:
            _check_tensor(GRAD, "GRAD", self.n, self.device)
            if GRAD.shape[0] < B:
                raise TowrGpuError("GRAD: fewer rows than X")
        if stream is None:
            stream = torch.cuda.current_stream(X.device)
        self._check(self._lib.towr_gpu_eval_cost_batch_device(
            self._h, B, *_opt(X), C.c_void_p(F.data_ptr()),
            C.c_void_p(GRAD.data_ptr() if GRAD is not None else 0), GRAD.stride(0) if GRAD is not None else 0,
            C.c_void_p(stream.cuda_stream)))

    def trajectory_size(self, dt: float):
        """(n_samples, n_cols) of the trajectory export at sample period dt."""
        ns, nc = C.c_int32(), C.c_int32()
        self._check(self._lib.towr_gpu_trajectory_size(self._h, dt, C.byref(ns), C.byref(nc)))
        return ns.value, nc.value

    def sample_trajectory(self, x, dt: float = 0.001) -> np.ndarray:
        """SaveTrajectoryToCSV's samples (save_data.cpp:9-130) on the device: (n_samples, 19 + 25 n_ee)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        ns, nc = self.trajectory_size(dt)
        out = np.zeros((ns, nc))
        self._check(self._lib.towr_gpu_sample_trajectory(self._h, capi.dptr(x), dt, capi.dptr(out)))
        return out

    def sample_trajectory_batch_device(self, X, dt, OUT, stream=None):
        """Device batch on torch HIP tensors: X (B, ldx) -> OUT (B, ldo >= n_samples * n_cols)."""
        import torch
        _check_tensor(X, "X", self.n, self.device)
        ns, nc = self.trajectory_size(dt)
        _check_tensor(OUT, "OUT", ns * nc, self.device)
        if OUT.shape[0] < X.shape[0]:
            raise TowrGpuError("OUT: fewer rows than X")
        if stream is None:
            stream = torch.cuda.current_stream(X.device)
        self._check(self._lib.towr_gpu_sample_trajectory_batch_device(
            self._h, X.shape[0], *_opt(X), dt, *_opt(OUT),
            C.c_void_p(stream.cuda_stream)))

    def set_batch_terrain(self, terrains):
        arr = (capi.Terrain * len(terrains))(*terrains)
        self._check(self._lib.towr_gpu_set_batch_terrain(self._h, len(terrains), arr))

    def eval_batch(self, X, G=None, V=None):
        """Host batch: X (B, n) -> G (B, m), V (B, nnz) (new arrays, or the given contiguous ones)."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        B = X.shape[0]
        if G is None:
            G = np.zeros((B, self.m))
        if V is None:
            V = np.zeros((B, self.nnz))
        for a, k, name in ((G, self.m, "G"), (V, self.nnz, "V")):
            if a.dtype != np.float64 or not a.flags.c_contiguous or a.shape != (B, k):
                raise TowrGpuError(f"eval_batch: {name} must be a contiguous float64 array of shape ({B}, {k})")
        self._check(self._lib.towr_gpu_eval_batch(self._h, B, capi.dptr(X), capi.dptr(G), capi.dptr(V)))
        return G, V

    def eval_batch_device(self, X, G, V, want_g=True, want_jac=True, stream=None):
        """Device batch on torch CUDA (HIP) tensors: X (B, ldx), G (B, ldg), V (B, ldv) float64.
        `stream`: a torch.cuda.Stream (default: torch's current stream)."""
        import torch
        B = X.shape[0]
        self._check_batch(X, G, V, want_g, want_jac)
        if stream is None:
            stream = torch.cuda.current_stream(X.device)
        self._check(self._lib.towr_gpu_eval_batch_device(   # (an output that is not wanted may be None)
            self._h, B, *_opt(X), *_opt(G), *_opt(V), int(want_g), int(want_jac), C.c_void_p(stream.cuda_stream)))

    def _check_batch(self, X, G, V, want_g=True, want_jac=True):
        B = X.shape[0]
        _check_tensor(X, "X", self.n, self.device)
        for t, name, cols, want in ((G, "G", self.m, want_g), (V, "V", self.nnz, want_jac)):
            if want or t is not None:
                _check_tensor(t, name, cols, self.device)
                if t.shape[0] < B:
                    raise TowrGpuError(f"{name}: fewer rows than X")

    # -------------------------------------------------------------------- products ------------
    def jac_csc(self):
        """The pattern by column (the transpose view of jac_csr): col_ptr (n + 1), row (nnz), csr_index (nnz)."""
        cp = np.zeros(self.n + 1, dtype=np.int64)
        r = np.zeros(self.nnz, dtype=np.int32)
        k = np.zeros(self.nnz, dtype=np.int32)
        self._check(self._lib.towr_gpu_jac_csc(self._h, capi.lptr(cp), capi.iptr(r), capi.iptr(k)))
        return cp, r, k

    def _check_rows(self, B, *ops):
        """(tensor, name, min columns) operands of a B-problem product call."""
        for t, name, cols in ops:
            _check_tensor(t, name, cols, self.device)
            if t.dim() != 2 or t.shape[0] < B:
                raise TowrGpuError(f"{name}: expected a 2-D tensor of >= {B} rows")

    @staticmethod
    def _stream(stream, t):
        import torch
        return C.c_void_p((stream if stream is not None else torch.cuda.current_stream(t.device)).cuda_stream)

    def jac_vec_batch_device(self, V, P, Y, stream=None):
        """Y[b] = J_b P[b] on torch HIP tensors: V (B, ldv >= nnz) CSR values, P (B, >= n), Y (B, >= m)."""
        B = V.shape[0]
        self._check_rows(B, (V, "V", self.nnz), (P, "P", self.n), (Y, "Y", self.m))
        self._check(self._lib.towr_gpu_jac_vec_batch_device(
            self._h, B, *_opt(V), *_opt(P), *_opt(Y), self._stream(stream, V)))

    def jac_tvec_batch_device(self, V, LAM, Z, accumulate=False, stream=None):
        """Z[b] (+)= J_b^T LAM[b]: V (B, ldv >= nnz), LAM (B, >= m), Z (B, >= n); accumulate adds to what Z holds."""
        B = V.shape[0]
        self._check_rows(B, (V, "V", self.nnz), (LAM, "LAM", self.m), (Z, "Z", self.n))
        self._check(self._lib.towr_gpu_jac_tvec_batch_device(
            self._h, B, *_opt(V), *_opt(LAM), *_opt(Z), int(bool(accumulate)), self._stream(stream, V)))

    def eval_products_batch_device(self, X, G=None, LAM=None, Z=None, P=None, Y=None, accumulate=False, stream=None):
        """Evaluate J_b at X[b] (and g into G when given), then Z[b] (+)= J_b^T LAM[b] and / or Y[b] = J_b P[b]; the
        values stay in handle scratch, set_products_chunk problems at a time."""
        B = X.shape[0]
        ops = [(X, "X", self.n)]
        ops += [(t, name, cols) for t, name, cols in ((G, "G", self.m), (LAM, "LAM", self.m), (Z, "Z", self.n),
                                                       (P, "P", self.n), (Y, "Y", self.m)) if t is not None]
        self._check_rows(B, *ops)
        self._check(self._lib.towr_gpu_eval_products_batch_device(
            self._h, B, *_opt(X), *_opt(G), *_opt(LAM), *_opt(Z), int(bool(accumulate)), *_opt(P), *_opt(Y),
            self._stream(stream, X)))

    # -------------------------------------------------------------------- residuals -----------
    def _box_operands(self, B, lo, up, cols, names):
        """(lower pointer, upper pointer, ldb) of an optional pair of bounds (names: the pair's and its dimension's,
        for messages): both None (the handle's bounds), both 1-D of >= cols entries (one row shared by all problems,
        ldb = 0) or both 2-D (B, >= cols) with one leading dimension."""
        nl, nu, dim = names
        if lo is None and up is None:
            return C.c_void_p(None), C.c_void_p(None), 0
        if lo is None or up is None:
            raise TowrGpuError(f"{nl} and {nu}: give both or neither")
        if lo.dim() != up.dim():
            raise TowrGpuError(f"{nl} and {nu}: one is shared (1-D), the other per problem (2-D)")
        if lo.dim() == 1:
            for t, name in ((lo, nl), (up, nu)):
                _check_tensor(t, name, cols, self.device)
                if t.shape[0] < cols or (t.shape[0] > 1 and t.stride(0) != 1):
                    raise TowrGpuError(f"{name}: expected >= {cols} contiguous entries")
            return C.c_void_p(lo.data_ptr()), C.c_void_p(up.data_ptr()), 0
        self._check_rows(B, (lo, nl, cols), (up, nu, cols))
        if lo.stride(0) != up.stride(0) or lo.stride(0) < cols:
            raise TowrGpuError(f"{nl} and {nu}: they share one leading dimension (>= {dim})")
        return C.c_void_p(lo.data_ptr()), C.c_void_p(up.data_ptr()), lo.stride(0)

    def _bounds_operands(self, B, GL, GU):
        return self._box_operands(B, GL, GU, self.m, ("GL", "GU", "m"))

    def _var_bounds_operands(self, B, XL, XU):
        return self._box_operands(B, XL, XU, self.n, ("XL", "XU", "n"))

    def residual_batch_device(self, G, SUM, GL=None, GU=None, LAM=None, rho=1.0, LAMP=None, stream=None):
        """Per-problem violation summary of G (B, >= m) against the bounds into SUM (B, >= 4 + n_constraints): max,
        sum, arg max, phi, per-set maxima (towr_gpu.h). GL / GU: None (the handle's bounds), 1-D (shared) or (B, >= m).
        With LAMP (B, >= m): the augmented Lagrangian's multipliers for LAM (None = zero) and rho."""
        B = G.shape[0]
        ops = [(G, "G", self.m), (SUM, "SUM", 4 + self.desc.n_constraints)]
        ops += [(t, name, self.m) for t, name in ((LAM, "LAM"), (LAMP, "LAMP")) if t is not None]
        self._check_rows(B, *ops)
        gl, gu, ldb = self._bounds_operands(B, GL, GU)
        self._check(self._lib.towr_gpu_residual_batch_device(
            self._h, B, *_opt(G), gl, gu, ldb, *_opt(LAM), float(rho), *_opt(LAMP), *_opt(SUM), self._stream(stream, G)))

    def eval_auglag_batch_device(self, X, SUM, Z, GL=None, GU=None, LAM=None, rho=1.0, G=None, LAMP=None,
                                 accumulate=False, stream=None):
        """Evaluate g_b, J_b at X[b], then SUM[b] and lam+_b as residual_batch_device, then Z[b] (+)= J_b^T lam+_b; g and
        lam+ are written to G / LAMP when given. The values stay in handle scratch, set_products_chunk problems at a time."""
        B = X.shape[0]
        ops = [(X, "X", self.n), (SUM, "SUM", 4 + self.desc.n_constraints), (Z, "Z", self.n)]
        ops += [(t, name, self.m) for t, name in ((LAM, "LAM"), (G, "G"), (LAMP, "LAMP")) if t is not None]
        self._check_rows(B, *ops)
        gl, gu, ldb = self._bounds_operands(B, GL, GU)
        self._check(self._lib.towr_gpu_eval_auglag_batch_device(
            self._h, B, *_opt(X), gl, gu, ldb, *_opt(LAM), float(rho), *_opt(G), *_opt(LAMP), *_opt(SUM), *_opt(Z),
            int(bool(accumulate)), self._stream(stream, X)))

    # -------------------------------------------------------------------- steps ---------------
    def _alpha_operand(self, B, alpha):
        """(ALPHA pointer, scalar) of a step call: a float, or a contiguous 1-D device tensor of >= B step lengths."""
        if isinstance(alpha, (int, float)):
            return C.c_void_p(None), float(alpha)
        _check_tensor(alpha, "ALPHA", 1, self.device)
        if alpha.dim() != 1 or alpha.shape[0] < B or (alpha.shape[0] > 1 and alpha.stride(0) != 1):
            raise TowrGpuError("ALPHA: expected a contiguous 1-D tensor of >= B entries")
        return C.c_void_p(alpha.data_ptr()), 0.0

    def step_batch_device(self, X, D, SUM, XP=None, alpha=1.0, XL=None, XU=None, stream=None):
        """XP[b] = P_[XL, XU](X[b] - alpha_b D[b]) and the projected step's summary into SUM (B, >= 5 + n_varsets): max
        |s|, sum s^2, sum d s, columns on a bound, how far X is outside its box, per-set max |s| (towr_gpu.h). alpha: a
        float or a 1-D tensor of B step lengths. XL / XU: None (the handle's bounds), 1-D (shared) or (B, >= n). XP
        None: the summary only."""
        B = X.shape[0]
        ops = [(X, "X", self.n), (D, "D", self.n), (SUM, "SUM", 5 + self.desc.n_varsets)]
        if XP is not None:
            ops.append((XP, "XP", self.n))
        self._check_rows(B, *ops)
        xl, xu, ldb = self._var_bounds_operands(B, XL, XU)
        ap, a = self._alpha_operand(B, alpha)
        self._check(self._lib.towr_gpu_step_batch_device(
            self._h, B, *_opt(X), *_opt(D), ap, a, xl, xu, ldb, *_opt(XP), *_opt(SUM), self._stream(stream, X)))

    def auglag_step_batch_device(self, X, XP, SSUM, RSUM, GL=None, GU=None, LAM=None, rho=1.0, alpha=1.0, XL=None, XU=None,
                                 F=None, G=None, LAMP=None, stream=None):
        """One iteration in one call: eval_cost_batch_device's gradient, eval_auglag_batch_device accumulated onto it
        (RSUM its summary; F, G, LAMP optional outputs) and step_batch_device with D = that gradient (XP, SSUM); the
        gradient stays in handle scratch. Bit-identical to the three calls in sequence."""
        B = X.shape[0]
        ops = [(X, "X", self.n), (XP, "XP", self.n), (SSUM, "SSUM", 5 + self.desc.n_varsets),
               (RSUM, "RSUM", 4 + self.desc.n_constraints)]
        ops += [(t, name, self.m) for t, name in ((LAM, "LAM"), (G, "G"), (LAMP, "LAMP")) if t is not None]
        self._check_rows(B, *ops)
        _check_per_problem(F, "F", B, self.device)
        gl, gu, ldgb = self._bounds_operands(B, GL, GU)
        xl, xu, ldxb = self._var_bounds_operands(B, XL, XU)
        ap, a = self._alpha_operand(B, alpha)
        self._check(self._lib.towr_gpu_auglag_step_batch_device(
            self._h, B, *_opt(X), gl, gu, ldgb, *_opt(LAM), float(rho), ap, a, xl, xu, ldxb, _opt(F)[0], *_opt(G), *_opt(LAMP),
            *_opt(RSUM), *_opt(XP), *_opt(SSUM), self._stream(stream, X)))

    # -------------------------------------------------------------------- L-BFGS --------------
    def _history_operands(self, B, mem, HS, HY, HMETA):
        """(HS pointer, HY pointer, ldh, HMETA pointer) of an L-BFGS call: HS and HY 2-D (B * mem, >= n) with one
        leading dimension, row b * mem + k = pair k of problem b; HMETA contiguous int32 of >= 2 B entries
        ({count, next} per problem; zeros = an empty history)."""
        import torch
        if not (isinstance(mem, int) and 1 <= mem <= capi.LBFGS_MAX_MEM):
            raise TowrGpuError(f"mem: expected an int in 1..{capi.LBFGS_MAX_MEM}")
        self._check_rows(B * mem, (HS, "HS", self.n), (HY, "HY", self.n))
        if HS.stride(0) != HY.stride(0) or HS.stride(0) < self.n:
            raise TowrGpuError("HS and HY: they share one leading dimension (>= n)")
        if HMETA.dtype != torch.int32:
            raise TowrGpuError(f"HMETA: dtype {HMETA.dtype}, expected torch.int32")
        if HMETA.device.type != "cuda" or HMETA.device.index != self.device:
            raise TowrGpuError(f"HMETA: tensor on {HMETA.device}, expected the handle's HIP device")
        if not HMETA.is_contiguous() or HMETA.numel() < 2 * B:
            raise TowrGpuError("HMETA: expected a contiguous tensor of >= 2 B entries")
        return C.c_void_p(HS.data_ptr()), C.c_void_p(HY.data_ptr()), HS.stride(0), C.c_void_p(HMETA.data_ptr())

    def lbfgs_update_batch_device(self, X, XN, GR, GRN, HS, HY, HMETA, SUM, mem, curv_eps=0.0, stream=None):
        """Offer the pair s = XN - X, y = GRN - GR of every problem to its history (HS, HY, HMETA, `mem` slots per
        problem): accepted iff sum s y > curv_eps sum y y, then written to slot `next`; a rejected problem's history is
        untouched. SUM (B, >= 6): sy, ss, yy, accepted, count, slot (towr_gpu.h)."""
        B = X.shape[0]
        self._check_rows(B, (X, "X", self.n), (XN, "XN", self.n), (GR, "GR", self.n), (GRN, "GRN", self.n), (SUM, "SUM", 6))
        hs, hy, ldh, hm = self._history_operands(B, mem, HS, HY, HMETA)
        self._check(self._lib.towr_gpu_lbfgs_update_batch_device(
            self._h, B, mem, *_opt(X), *_opt(XN), *_opt(GR), *_opt(GRN), float(curv_eps), hs, hy, ldh, hm, *_opt(SUM),
            self._stream(stream, GR)))

    def lbfgs_direction_batch_device(self, GR, HS, HY, HMETA, D, SUM, mem, X=None, XL=None, XU=None, stream=None):
        """D[b] = the two-loop L-BFGS direction of the gradient GR[b] on the free columns (held columns: D = GR), with
        the columns held where X[b] sits on a bound and the gradient points outward; X None: every column is free.
        XL / XU: None (the handle's bounds), 1-D (shared) or (B, >= n). SUM (B, >= 5): pairs used, gamma, slope
        sum g D, held columns, sum_free g^2 (towr_gpu.h)."""
        B = GR.shape[0]
        ops = [(GR, "GR", self.n), (D, "D", self.n), (SUM, "SUM", 5)]
        if X is not None:
            ops.append((X, "X", self.n))
        self._check_rows(B, *ops)
        hs, hy, ldh, hm = self._history_operands(B, mem, HS, HY, HMETA)
        xl, xu, ldb = self._var_bounds_operands(B, XL, XU)
        self._check(self._lib.towr_gpu_lbfgs_direction_batch_device(
            self._h, B, mem, *_opt(X), *_opt(GR), xl, xu, ldb, hs, hy, ldh, hm, *_opt(D), *_opt(SUM), self._stream(stream, GR)))

    def auglag_lbfgs_step_batch_device(self, X, GR, XP, SSUM, RSUM, DSUM, HS, HY, HMETA, mem, XPREV=None, GRPREV=None,
                                       USUM=None, curv_eps=0.0, GL=None, GU=None, LAM=None, rho=1.0, alpha=1.0, XL=None,
                                       XU=None, F=None, stream=None):
        """One inner iteration in one call: the augmented Lagrangian's gradient at X into GR (RSUM the residual
        summary, F optional), lbfgs_update_batch_device with (XPREV -> X, GRPREV -> GR) into USUM when XPREV / GRPREV
        are given, lbfgs_direction_batch_device at (X, GR) (DSUM) and step_batch_device with that direction (XP,
        SSUM). Bit-identical to the separate calls in sequence."""
        B = X.shape[0]
        ops = [(X, "X", self.n), (GR, "GR", self.n), (XP, "XP", self.n), (SSUM, "SSUM", 5 + self.desc.n_varsets),
               (RSUM, "RSUM", 4 + self.desc.n_constraints), (DSUM, "DSUM", 5)]
        if (XPREV is None) != (GRPREV is None):
            raise TowrGpuError("XPREV and GRPREV: give both or neither")
        if XPREV is not None:
            if USUM is None:
                raise TowrGpuError("USUM: required with XPREV / GRPREV")
            ops += [(XPREV, "XPREV", self.n), (GRPREV, "GRPREV", self.n), (USUM, "USUM", 6)]
        if LAM is not None:
            ops.append((LAM, "LAM", self.m))
        self._check_rows(B, *ops)
        _check_per_problem(F, "F", B, self.device)
        hs, hy, ldh, hm = self._history_operands(B, mem, HS, HY, HMETA)
        gl, gu, ldgb = self._bounds_operands(B, GL, GU)
        xl, xu, ldxb = self._var_bounds_operands(B, XL, XU)
        ap, a = self._alpha_operand(B, alpha)
        self._check(self._lib.towr_gpu_auglag_lbfgs_step_batch_device(
            self._h, B, mem, *_opt(X), *_opt(XPREV), *_opt(GRPREV), gl, gu, ldgb, *_opt(LAM), float(rho), ap, a, xl, xu, ldxb,
            float(curv_eps), hs, hy, ldh, hm, _opt(F)[0], *_opt(GR), *_opt(RSUM), *_opt(USUM if XPREV is not None else None),
            *_opt(DSUM), *_opt(XP), *_opt(SSUM), self._stream(stream, X)))

    # -------------------------------------------------------------------- resident loop -------
    def _alsolve_state(self, st, params):
        """towr_alsolve_state_t of an AlSolveState, after the checks the C-ABI cannot make (dtypes, devices, rows)."""
        import torch
        B, mem = st.B, st.mem
        if mem != params.mem:
            raise TowrGpuError(f"state allocated for mem = {mem}, params.mem = {params.mem}")
        n, m = self.n, self.m
        self._check_rows(B, *[(getattr(st, k), k, n) for k in ("X", "GR", "XC", "GRC", "D")],
                         (st.LAM, "LAM", m), (st.LAMP, "LAMP", m), (st.SCAL, "SCAL", 8), (st.LSUM, "LSUM", 8), (st.USUM, "USUM", 6),
                         (st.DSUM, "DSUM", 5), (st.RSUM, "RSUM", 4 + self.desc.n_constraints),
                         (st.SSUM, "SSUM", 5 + self.desc.n_varsets))
        for a, b in (("X", "GR"), ("X", "XC"), ("X", "GRC"), ("X", "D"), ("LAM", "LAMP")):
            if getattr(st, a).stride(0) != getattr(st, b).stride(0):
                raise TowrGpuError(f"{a} and {b}: they share one leading dimension")
        hs, hy, ldh, hm = self._history_operands(B, mem, st.HS, st.HY, st.HMETA)
        for k in ("ALPHA", "RHO", "FC"):
            _check_per_problem(getattr(st, k), k, B, self.device)
        t = st.ISTATE
        if t.dtype != torch.int32 or t.device.type != "cuda" or t.device.index != self.device or not t.is_contiguous() \
                or t.numel() < 4 * B:
            raise TowrGpuError("ISTATE: expected a contiguous int32 tensor of >= 4 B entries on the handle's device")
        c = capi.AlSolveStateC()
        for k in ("X", "GR", "XC", "GRC", "D", "LAM", "LAMP", "HS", "HY", "HMETA", "ALPHA", "RHO", "FC", "SCAL", "ISTATE",
                  "RSUM", "SSUM", "DSUM", "USUM", "LSUM"):
            setattr(c, k, getattr(st, k).data_ptr())
        c.ldx, c.ldl, c.ldh, c.ldsc = st.X.stride(0), st.LAM.stride(0), ldh, st.SCAL.stride(0)
        c.ldrs, c.ldss, c.ldds, c.ldus, c.ldls = (st.RSUM.stride(0), st.SSUM.stride(0), st.DSUM.stride(0), st.USUM.stride(0),
                                                  st.LSUM.stride(0))
        return c

    def linesearch_batch_device(self, params, st, XL=None, XU=None, stream=None):
        """Keep or reject every problem's candidate st.XC behind an evaluation (st.FC, st.GRC, st.RSUM): the Armijo
        test, the pair offered to the history, the base, ALPHA, the phase and flags, LSUM (towr_gpu.h)."""
        c = self._alsolve_state(st, params)
        xl, xu, ldb = self._var_bounds_operands(st.B, XL, XU)
        self._check(self._lib.towr_gpu_linesearch_batch_device(self._h, st.B, C.byref(params), C.byref(c), xl, xu, ldb,
                                                               self._stream(stream, st.X)))

    def auglag_outer_batch_device(self, params, st, stream=None):
        """The outer update of the problems whose inner loop is done: converged, LAM <- LAMP with tighter tolerances,
        or a larger RHO (towr_gpu.h)."""
        c = self._alsolve_state(st, params)
        self._check(self._lib.towr_gpu_auglag_outer_batch_device(self._h, st.B, C.byref(params), C.byref(c),
                                                                 self._stream(stream, st.X)))

    def alsolve_stop(self, params, stop, st, stream=None):
        """The stop rule alone, between the line search and the outer update: a SEARCH problem whose base stayed
        acceptable for stop.acc_iters iterations becomes ACCEPTABLE, one whose penalty is about to grow again without
        progress becomes INFEASIBLE (towr_gpu.h; SCAL[6..7] are the rule's memory)."""
        c = self._alsolve_state(st, params)
        self._check(self._lib.towr_gpu_alsolve_stop_batch_device(self._h, st.B, C.byref(params), C.byref(stop), C.byref(c),
                                                                 self._stream(stream, st.X)))

    def alsolve_init(self, params, st, XL=None, XU=None, stream=None):
        """Start a solve from st.X (clamped into st.XC) and st.LAM: phases, counters, RHO, ALPHA, tolerances."""
        c = self._alsolve_state(st, params)
        xl, xu, ldb = self._var_bounds_operands(st.B, XL, XU)
        self._check(self._lib.towr_gpu_alsolve_init_batch_device(self._h, st.B, C.byref(params), C.byref(c), xl, xu, ldb,
                                                                 self._stream(stream, st.X)))

    def alsolve_iterate(self, params, st, iters=1, GL=None, GU=None, XL=None, XU=None, stream=None):
        """`iters` complete iterations (evaluation, line search, outer update, direction, step) on the stream, with no
        host synchronisation. Frozen problems are still evaluated; their state no longer changes."""
        c = self._alsolve_state(st, params)
        gl, gu, ldgb = self._bounds_operands(st.B, GL, GU)
        xl, xu, ldxb = self._var_bounds_operands(st.B, XL, XU)
        self._check(self._lib.towr_gpu_alsolve_iterate_batch_device(self._h, st.B, int(iters), C.byref(params), C.byref(c),
                                                                    gl, gu, ldgb, xl, xu, ldxb, self._stream(stream, st.X)))

    def _probe_operands(self, B, probes, PSUM):
        """(towr_alsolve_probe_t, PSUM pointer, ldps) of a probe stage with `probes` trials."""
        if PSUM is None:
            raise TowrGpuError("PSUM: required with probes")
        self._check_rows(B, (PSUM, "PSUM", 8))
        return capi.AlSolveProbe(trials=int(probes)), PSUM.data_ptr(), PSUM.stride(0)

    def alsolve_probe(self, params, st, probes, PSUM, GL=None, GU=None, XL=None, XU=None, stream=None):
        """The probe stage in front of an iteration (towr_gpu.h, towr_gpu_alsolve_probe_batch_device): up to `probes`
        lengths of the line search's ladder are tested with cheap evaluations (f only, g only, the residual kernel) and
        every SEARCH problem's ALPHA, XC and inner counter are left where the sequential loop would stand after the
        rejections found. PSUM (B, >= 8): code, t*, lengths probed, the length, its merit (NaN when untested), gs."""
        c = self._alsolve_state(st, params)
        gl, gu, ldgb = self._bounds_operands(st.B, GL, GU)
        xl, xu, ldxb = self._var_bounds_operands(st.B, XL, XU)
        pr, ps, ldps = self._probe_operands(st.B, probes, PSUM)
        self._check(self._lib.towr_gpu_alsolve_probe_batch_device(self._h, st.B, C.byref(params), C.byref(pr), C.byref(c),
                                                                  gl, gu, ldgb, xl, xu, ldxb, ps, ldps, self._stream(stream, st.X)))

    # -------------------------------------------------------------------- Gauss-Newton -------
    def gn_direction_batch_device(self, gn, V, LAMP, GR, D, SUM, rho=1.0, X=None, XL=None, XU=None, RUN=None, run_stride=1,
                                  stream=None):
        """D[b] = the truncated CG solution of (rho_b (J^T W J)_ff + mu I) d = g on the free columns (held columns:
        D = GR), J_b the CSR values V[b], W the rows whose LAMP is not zero, g = GR[b]; gn: gn_params(...). rho: a float
        or a 1-D tensor of B values. X None: every column is free. XL / XU: None (the handle's bounds), 1-D (shared) or
        (B, >= n). RUN: None, or an int32 tensor; problem b is skipped when RUN[b * run_stride] >= 2. SUM (B, >= 6):
        steps, bb, rr, slope sum g D, held columns, stop code (towr_gpu.h)."""
        B = GR.shape[0]
        ops = [(V, "V", self.nnz), (LAMP, "LAMP", self.m), (GR, "GR", self.n), (D, "D", self.n), (SUM, "SUM", 6)]
        if X is not None:
            ops.append((X, "X", self.n))
        self._check_rows(B, *ops)
        xl, xu, ldb = self._var_bounds_operands(B, XL, XU)
        rp, r, run = self._gn_rho_run(B, rho, RUN, run_stride)
        self._check(self._lib.towr_gpu_gn_direction_batch_device(
            self._h, B, C.byref(gn), *_opt(V), *_opt(LAMP), rp, r, *_opt(X), *_opt(GR), xl, xu, ldb, run, int(run_stride),
            *_opt(D), *_opt(SUM), self._stream(stream, GR)))

    def _gn_rho_run(self, B, rho, RUN, run_stride):
        """(RHO pointer, scalar rho, RUN pointer) of a GN direction call."""
        import torch
        if isinstance(rho, (int, float)):
            rp, r = C.c_void_p(None), float(rho)
        else:
            _check_per_problem(rho, "RHO", B, self.device)
            rp, r = C.c_void_p(rho.data_ptr()), 0.0
        run = C.c_void_p(None)
        if RUN is not None:
            if RUN.dtype != torch.int32 or RUN.device.type != "cuda" or RUN.device.index != self.device or not RUN.is_contiguous() \
                    or run_stride < 1 or RUN.numel() < (B - 1) * run_stride + 1:
                raise TowrGpuError("RUN: expected a contiguous int32 tensor of >= (B - 1) run_stride + 1 entries on the handle's device")
            run = C.c_void_p(RUN.data_ptr())
        return rp, r, run

    def gn_pc_direction_batch_device(self, gn, V, LAMP, GR, D, SUM, PC=None, precond=capi.GN_PC_JACOBI, rho=1.0, X=None, XL=None,
                                     XU=None, RUN=None, run_stride=1, stream=None):
        """gn_direction_batch_device with a preconditioner: capi.GN_PC_JACOBI (the default) runs the CG recursion
        preconditioned by M = rho_b diag(J^T W J) + mu (1 where that is exactly 0), which it writes to PC (B, >= n; 0 on
        held columns); capi.GN_PC_NONE is gn_direction_batch_device bit for bit (PC may be None). SUM (B, >= 8): as
        there, then [6] the final r.z and [7] the number of free columns whose M was replaced by 1 (towr_gpu.h)."""
        B = GR.shape[0]
        ops = [(V, "V", self.nnz), (LAMP, "LAMP", self.m), (GR, "GR", self.n), (D, "D", self.n), (SUM, "SUM", 8)]
        if X is not None:
            ops.append((X, "X", self.n))
        if PC is not None:
            ops.append((PC, "PC", self.n))
        self._check_rows(B, *ops)
        xl, xu, ldb = self._var_bounds_operands(B, XL, XU)
        rp, r, run = self._gn_rho_run(B, rho, RUN, run_stride)
        self._check(self._lib.towr_gpu_gn_direction_pc_batch_device(
            self._h, B, C.byref(gn), int(precond), *_opt(V), *_opt(LAMP), rp, r, *_opt(X), *_opt(GR), xl, xu, ldb, run,
            int(run_stride), *_opt(D), *_opt(SUM), *_opt(PC), self._stream(stream, GR)))

    def alsolve_gn_iterate(self, params, st, gn, DC, GSUM, iters=1, GL=None, GU=None, XL=None, XU=None, stream=None):
        """alsolve_iterate with the Gauss-Newton direction: per iteration the evaluation, the CG solve at the candidate
        into DC (B, the leading dimension of st.X) and GSUM (B, >= 6), the line search, the outer update, the select
        (st.D <- DC on an accepted base, st.GR on the one steepest-descent retry) and the step, with no host
        synchronisation (towr_gpu.h)."""
        c = self._alsolve_state(st, params)
        self._check_rows(st.B, (DC, "DC", self.n), (GSUM, "GSUM", 6))
        if DC.stride(0) != st.X.stride(0):
            raise TowrGpuError("X and DC: they share one leading dimension")
        gl, gu, ldgb = self._bounds_operands(st.B, GL, GU)
        xl, xu, ldxb = self._var_bounds_operands(st.B, XL, XU)
        self._check(self._lib.towr_gpu_alsolve_gn_iterate_batch_device(
            self._h, st.B, int(iters), C.byref(params), C.byref(c), C.byref(gn), C.c_void_p(DC.data_ptr()), *_opt(GSUM),
            gl, gu, ldgb, xl, xu, ldxb, self._stream(stream, st.X)))

    def alsolve_gn_pc_iterate(self, params, st, gn, DC, GSUM, PC=None, precond=capi.GN_PC_JACOBI, iters=1, GL=None, GU=None,
                              XL=None, XU=None, stream=None):
        """alsolve_gn_iterate with the direction of gn_pc_direction_batch_device: PC (B, the leading dimension of st.X)
        takes the preconditioner of every CG solve, GSUM is (B, >= 8). precond = capi.GN_PC_NONE is alsolve_gn_iterate
        bit for bit (towr_gpu.h)."""
        c = self._alsolve_state(st, params)
        ops = [(DC, "DC", self.n), (GSUM, "GSUM", 8)] + ([(PC, "PC", self.n)] if PC is not None else [])
        self._check_rows(st.B, *ops)
        if DC.stride(0) != st.X.stride(0) or (PC is not None and PC.stride(0) != st.X.stride(0)):
            raise TowrGpuError("X, DC and PC: they share one leading dimension")
        gl, gu, ldgb = self._bounds_operands(st.B, GL, GU)
        xl, xu, ldxb = self._var_bounds_operands(st.B, XL, XU)
        self._check(self._lib.towr_gpu_alsolve_gn_pc_iterate_batch_device(
            self._h, st.B, int(iters), C.byref(params), C.byref(c), C.byref(gn), int(precond), C.c_void_p(DC.data_ptr()),
            *_opt(GSUM), C.c_void_p(None if PC is None else PC.data_ptr()), gl, gu, ldgb, xl, xu, ldxb,
            self._stream(stream, st.X)))

    def gn_factor_info(self):
        """The symbolic phase of the direct Gauss-Newton direction (a layout-only handle answers too): dict(ordering
        (capi.GN_ORDER_RCM), pos (n; the permuted position of column j), first (n; the first permuted column of permuted
        row q of the lower triangle of J^T J), envelope, bandwidth, ldw_min (workspace doubles per problem))."""
        pos = np.zeros(self.n, dtype=np.int32)
        first = np.zeros(self.n, dtype=np.int32)
        o = C.c_int32(0)
        env, bw, ldw = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._check(self._lib.towr_gpu_gn_factor_info(self._h, C.byref(o), capi.iptr(pos), capi.iptr(first), C.byref(env),
                                                      C.byref(bw), C.byref(ldw)))
        return dict(ordering=o.value, pos=pos, first=first, envelope=env.value, bandwidth=bw.value, ldw_min=ldw.value)

    def _gn_workspace(self, W, wrows, B):
        """(pointer, ldw, wrows) of a direct direction's workspace W (rows, >= ldw_min): wrows None takes W's rows."""
        _check_tensor(W, "W", 1, self.device)
        if W.dim() != 2 or W.shape[0] < 1:
            raise TowrGpuError("W: expected a 2-D tensor of >= 1 rows")
        wrows = W.shape[0] if wrows is None else int(wrows)
        if wrows > W.shape[0]:
            raise TowrGpuError(f"W: {W.shape[0]} rows, wrows = {wrows}")
        ldw = W.stride(0) if W.shape[0] > 1 else W.shape[1]
        return C.c_void_p(W.data_ptr()), ldw, wrows

    def gn_direct_direction_batch_device(self, gn, V, LAMP, GR, D, SUM, W, wrows=None, rho=1.0, X=None, XL=None, XU=None,
                                         RUN=None, run_stride=1, stream=None):
        """gn_direction_batch_device's system solved exactly: per problem the envelope Cholesky factorisation of
        rho_b (J^T W J)_ff + mu I under gn_factor_info's ordering and two triangular solves; of gn only mu is read. W
        (rows, >= ldw_min) is the workspace: the call runs ceil(B / wrows) launches and problem b uses row b mod wrows
        (wrows None: every row of W). SUM (B, >= 8): solved, bb, smallest pivot, slope sum g D, held columns, code
        (1 solved, 2 breakdown, 3 bb == 0), largest pivot, breakdown column or -1 (towr_gpu.h)."""
        B = GR.shape[0]
        ops = [(V, "V", self.nnz), (LAMP, "LAMP", self.m), (GR, "GR", self.n), (D, "D", self.n), (SUM, "SUM", 8)]
        if X is not None:
            ops.append((X, "X", self.n))
        self._check_rows(B, *ops)
        xl, xu, ldb = self._var_bounds_operands(B, XL, XU)
        rp, r, run = self._gn_rho_run(B, rho, RUN, run_stride)
        wp, ldw, wr = self._gn_workspace(W, wrows, B)
        self._check(self._lib.towr_gpu_gn_direction_direct_batch_device(
            self._h, B, C.byref(gn), *_opt(V), *_opt(LAMP), rp, r, *_opt(X), *_opt(GR), xl, xu, ldb, run, int(run_stride),
            *_opt(D), *_opt(SUM), wp, ldw, wr, self._stream(stream, GR)))

    def alsolve_gn_direct_iterate(self, params, st, gn, DC, GSUM, W, wrows=None, iters=1, GL=None, GU=None, XL=None, XU=None,
                                  stream=None):
        """alsolve_gn_iterate with the direction of gn_direct_direction_batch_device: W / wrows its workspace (wrows
        applies within each products chunk), GSUM is (B, >= 8) (towr_gpu.h)."""
        c = self._alsolve_state(st, params)
        self._check_rows(st.B, (DC, "DC", self.n), (GSUM, "GSUM", 8))
        if DC.stride(0) != st.X.stride(0):
            raise TowrGpuError("X and DC: they share one leading dimension")
        gl, gu, ldgb = self._bounds_operands(st.B, GL, GU)
        xl, xu, ldxb = self._var_bounds_operands(st.B, XL, XU)
        wp, ldw, wr = self._gn_workspace(W, wrows, st.B)
        self._check(self._lib.towr_gpu_alsolve_gn_direct_iterate_batch_device(
            self._h, st.B, int(iters), C.byref(params), C.byref(c), C.byref(gn), C.c_void_p(DC.data_ptr()), *_opt(GSUM),
            wp, ldw, wr, gl, gu, ldgb, xl, xu, ldxb, self._stream(stream, st.X)))

    def gn_tile_info(self):
        """The symbolic phase of the tiled direct Gauss-Newton direction (a layout-only handle answers too): dict(tile
        (capi.GN_TILE), nt (block rows), bfirst (nt; the first stored tile of block row I under gn_factor_info's
        ordering), tiles, ldw_min (workspace doubles per problem: 256 per stored tile))."""
        nt = (self.n + capi.GN_TILE - 1) // capi.GN_TILE
        bfirst = np.zeros(nt, dtype=np.int32)
        t, k = C.c_int32(0), C.c_int32(0)
        tiles, ldw = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.towr_gpu_gn_tile_info(self._h, C.byref(t), C.byref(k), capi.iptr(bfirst), C.byref(tiles),
                                                    C.byref(ldw)))
        return dict(tile=t.value, nt=k.value, bfirst=bfirst, tiles=tiles.value, ldw_min=ldw.value)

    def gn_tiled_direction_batch_device(self, gn, V, LAMP, GR, D, SUM, W, wrows=None, rho=1.0, X=None, XL=None, XU=None,
                                        RUN=None, run_stride=1, stream=None):
        """gn_direct_direction_batch_device's system, arguments, codes and SUM with the factorisation done as a block
        Cholesky on 16 x 16 tiles inside gn_tile_info's tile envelope; W rows hold >= its ldw_min doubles. The bits are
        this entry's own (towr_gpu.h): a function of the problem's operands alone, not the envelope entry's."""
        B = GR.shape[0]
        ops = [(V, "V", self.nnz), (LAMP, "LAMP", self.m), (GR, "GR", self.n), (D, "D", self.n), (SUM, "SUM", 8)]
        if X is not None:
            ops.append((X, "X", self.n))
        self._check_rows(B, *ops)
        xl, xu, ldb = self._var_bounds_operands(B, XL, XU)
        rp, r, run = self._gn_rho_run(B, rho, RUN, run_stride)
        wp, ldw, wr = self._gn_workspace(W, wrows, B)
        self._check(self._lib.towr_gpu_gn_direction_tiled_batch_device(
            self._h, B, C.byref(gn), *_opt(V), *_opt(LAMP), rp, r, *_opt(X), *_opt(GR), xl, xu, ldb, run, int(run_stride),
            *_opt(D), *_opt(SUM), wp, ldw, wr, self._stream(stream, GR)))

    def alsolve_gn_tiled_iterate(self, params, st, gn, DC, GSUM, W, wrows=None, iters=1, GL=None, GU=None, XL=None, XU=None,
                                 stream=None):
        """alsolve_gn_direct_iterate with the direction of gn_tiled_direction_batch_device (W rows of gn_tile_info's
        ldw_min; towr_gpu.h)."""
        c = self._alsolve_state(st, params)
        self._check_rows(st.B, (DC, "DC", self.n), (GSUM, "GSUM", 8))
        if DC.stride(0) != st.X.stride(0):
            raise TowrGpuError("X and DC: they share one leading dimension")
        gl, gu, ldgb = self._bounds_operands(st.B, GL, GU)
        xl, xu, ldxb = self._var_bounds_operands(st.B, XL, XU)
        wp, ldw, wr = self._gn_workspace(W, wrows, st.B)
        self._check(self._lib.towr_gpu_alsolve_gn_tiled_iterate_batch_device(
            self._h, st.B, int(iters), C.byref(params), C.byref(c), C.byref(gn), C.c_void_p(DC.data_ptr()), *_opt(GSUM),
            wp, ldw, wr, gl, gu, ldgb, xl, xu, ldxb, self._stream(stream, st.X)))

    # -------------------------------------------------------------------- the lazy GN loop ----
    def _lazy_operands(self, B, VERDICT, NDIR):
        """towr_alsolve_lazy_t of VERDICT (int32, >= B) and NDIR (int32, >= B, or None)."""
        if VERDICT is None:
            raise TowrGpuError("VERDICT: required")
        return capi.AlSolveLazy(VERDICT=self._int_operand(VERDICT, "VERDICT", B).value,
                                NDIR=None if NDIR is None else self._int_operand(NDIR, "NDIR", B).value)

    def alsolve_verdict(self, params, st, VERDICT, NDIR=None, stream=None):
        """The line search's accept test ahead of it (towr_gpu.h, towr_gpu_alsolve_verdict_batch_device), on st.X, GR, XC,
        FC, SCAL, ISTATE and RSUM as the line search will find them: VERDICT[b] (int32) = 0 where a base will be accepted
        (RESTART, or a SEARCH candidate that passes) and 2 otherwise (frozen rows included); NDIR[b] (int32, optional)
        += 1 on a 0. Nothing else is written."""
        c = self._alsolve_state(st, params)
        lz = self._lazy_operands(st.B, VERDICT, NDIR)
        self._check(self._lib.towr_gpu_alsolve_verdict_batch_device(self._h, st.B, C.byref(params), C.byref(c), lz.VERDICT, lz.NDIR,
                                                                    self._stream(stream, st.X)))

    def alsolve_gn_lazy_iterate(self, params, st, method, gn, DC, GSUM, VERDICT, NDIR=None, PC=None, precond=capi.GN_PC_JACOBI,
                                W=None, wrows=None, iters=1, GL=None, GU=None, XL=None, XU=None, stream=None):
        """`iters` iterations of the GN method's iterate entry (capi.SOLVE_GN, _GN_PC, _GN_DIRECT, _GN_TILED; gn, DC, GSUM,
        PC / precond, W / wrows as that entry takes them) with alsolve_verdict ahead of every direction, which then runs
        only where VERDICT is 0 (towr_gpu.h, towr_gpu_alsolve_gn_lazy_iterate_batch_device). The state is bit for bit that
        entry's; a DC / GSUM / PC row is written only in an iteration whose candidate the line search takes."""
        c = self._alsolve_state(st, params)
        d = self._solve_dir(st, method, gn, DC, GSUM, PC, precond, W, wrows)
        lz = self._lazy_operands(st.B, VERDICT, NDIR)
        gl, gu, ldgb = self._bounds_operands(st.B, GL, GU)
        xl, xu, ldxb = self._var_bounds_operands(st.B, XL, XU)
        self._check(self._lib.towr_gpu_alsolve_gn_lazy_iterate_batch_device(
            self._h, st.B, int(iters), int(method), C.byref(params), C.byref(c), C.byref(d), C.byref(lz), gl, gu, ldgb,
            xl, xu, ldxb, self._stream(stream, st.X)))

    # -------------------------------------------------------------------- solve to completion -
    def _int_operand(self, t, what, count):
        import torch
        if t.dtype != torch.int32 or t.device.type != "cuda" or t.device.index != self.device or not t.is_contiguous() \
                or t.numel() < count:
            raise TowrGpuError(f"{what}: expected a contiguous int32 tensor of >= {count} entries on the handle's device")
        return C.c_void_p(t.data_ptr())

    def alsolve_partition(self, ISTATE, HEAD, PAIRS, B=None, stream=None):
        """The partition plan of a batch by its phases (towr_gpu.h): ISTATE int32 (>= 4 B), HEAD int32 (>= 8) takes
        na, np and the six phase counts, PAIRS int32 (>= 2 (B // 2)) the (frozen row, active row) pairs whose exchange
        puts the active rows in front. B None: ISTATE.numel() // 4."""
        B = ISTATE.numel() // 4 if B is None else int(B)
        self._check(self._lib.towr_gpu_alsolve_partition_batch_device(
            self._h, B, self._int_operand(ISTATE, "ISTATE", 4 * B), self._int_operand(HEAD, "HEAD", 8),
            self._int_operand(PAIRS, "PAIRS", 2 * (B // 2)), self._stream(stream, ISTATE)))

    def _row_descs(self, arrays, what, limit):
        """towr_rows_t descriptors of torch HIP tensors (1-D: rows of one element; 2-D: row-major rows) or of
        (tensor, columns) for only the first `columns` of each row."""
        if len(arrays) > limit:
            raise TowrGpuError(f"{what}: {len(arrays)} arrays, at most {limit}")
        desc = (capi.Rows * max(len(arrays), 1))()
        for k, a in enumerate(arrays):
            t, cols = a if isinstance(a, tuple) else (a, None)
            if t.device.type != "cuda" or t.device.index != self.device or t.dim() not in (1, 2) or \
                    (t.dim() == 2 and t.shape[1] > 1 and t.stride(1) != 1):
                raise TowrGpuError(f"{what}: array {k}: expected a 1-D or row-major 2-D tensor on the handle's device")
            es = t.element_size()
            width = 1 if t.dim() == 1 else t.shape[1]
            cols = width if cols is None else int(cols)
            if cols > width:
                raise TowrGpuError(f"{what}: array {k}: {cols} columns of {width}")
            ld = t.stride(0) if t.shape[0] > 1 else max(width, 1)
            desc[k].base, desc[k].ld_bytes, desc[k].row_bytes = t.data_ptr(), ld * es, cols * es
        return desc

    def alsolve_swap_rows(self, PAIRS, arrays, NP=None, npairs=0, max_pairs=None, stream=None):
        """Exchange rows PAIRS[2 i] and PAIRS[2 i + 1], i < count, of every array in place (towr_gpu.h). `arrays`: torch
        HIP tensors (1-D: rows of one element; 2-D: row-major rows, any padding behind the columns of a view is not
        touched) or (tensor, columns) to exchange only the first `columns` of each row. The count is NP[0] (an int32
        device tensor, e.g. HEAD[1:]; the grid holds max_pairs pairs, default PAIRS.numel() // 2) or, with NP None, the
        host value npairs."""
        desc = self._row_descs(arrays, "alsolve_swap_rows", capi.SWAP_MAX_ARRAYS)
        if NP is None:
            np_, n, mx = C.c_void_p(None), int(npairs), 0
            need = 2 * n
        else:
            mx = PAIRS.numel() // 2 if max_pairs is None else int(max_pairs)
            np_, n = self._int_operand(NP, "NP", 1), 0
            need = 2 * mx
        self._check(self._lib.towr_gpu_alsolve_swap_rows_batch_device(
            self._h, np_, n, mx, self._int_operand(PAIRS, "PAIRS", max(need, 0)), len(arrays), desc, self._stream(stream, PAIRS)))

    def _solve_dir(self, st, method, gn, DC, GSUM, PC, precond, W, wrows):
        """towr_solve_dir_t of a solve on st's rows: what the method's iterate entry takes beside the state."""
        B = st.B
        d = capi.SolveDir()
        if method != capi.SOLVE_LBFGS:
            if gn is None or DC is None or GSUM is None:
                raise TowrGpuError("alsolve_solve: a GN method needs gn, DC and GSUM")
            self._check_rows(B, (DC, "DC", self.n), (GSUM, "GSUM", 6 if method == capi.SOLVE_GN else 8))
            if DC.stride(0) != st.X.stride(0):
                raise TowrGpuError("X and DC: they share one leading dimension")
            d.gn, d.DC, d.GSUM, d.ldgs = C.pointer(gn), DC.data_ptr(), GSUM.data_ptr(), GSUM.stride(0)
        if method == capi.SOLVE_GN_PC:
            d.precond = int(precond)
            if PC is not None:
                self._check_rows(B, (PC, "PC", self.n))
                if PC.stride(0) != st.X.stride(0):
                    raise TowrGpuError("X and PC: they share one leading dimension")
                d.PC = PC.data_ptr()
        if method in (capi.SOLVE_GN_DIRECT, capi.SOLVE_GN_TILED):
            if W is None:
                raise TowrGpuError("alsolve_solve: the direct methods need the workspace W")
            wp, d.ldw, d.wrows = self._gn_workspace(W, wrows, B)
            d.W = wp.value
        return d

    def alsolve_solve(self, params, st, method=capi.SOLVE_GN_TILED, gn=None, DC=None, GSUM=None, PC=None,
                      precond=capi.GN_PC_JACOBI, W=None, wrows=None, max_iters=100, check_every=4, compact=True,
                      GL=None, GU=None, XL=None, XU=None, LOG=None, stream=None, stop=None, ex=None, probes=None, PSUM=None,
                      lazy=False, VERDICT=None, NDIR=None):
        """Run the resident loop to completion (towr_gpu.h, towr_gpu_alsolve_solve_batch_device): rounds of check_every
        iterations of the method's iterate entry (capi.SOLVE_*; gn, DC, GSUM, PC / precond, W / wrows as that entry
        takes them), the host looking at the phases once per round, until every problem is frozen or max_iters
        iterations have run. compact: the frozen problems are moved out of the batch between rounds; every array is
        back in the caller's order at return, and the persistent arrays hold the bits of the plain iterate loop. Per-problem
        GL / GU / XL / XU rows are permuted during the call. The call blocks the host. LOG: int32 (>= 8 + 2 B), allocated
        when None. Returns dict(rounds, iters_run, problem_iters, n_phase (6 counts: phases 0..4, other)). stop (an
        alsolve_stop_params()): the stop rule runs in every iteration (towr_gpu_alsolve_solve_ex_batch_device) and the
        dict also holds n_acceptable and n_infeasible, which n_phase[5] includes. ex: whether the call goes through the
        _ex entry (default: when stop is given); ex=True with stop None passes stop == NULL to it. probes (1..capi.PROBE_MAX)
        with PSUM (B, >= 8): the probe stage runs in front of every iteration (towr_gpu_alsolve_solve_probe_batch_device;
        iters_run then counts probed iterations); probes=0 calls that entry with probe == NULL, which is the _ex entry.
        lazy (a GN method): the solve runs through towr_gpu_alsolve_solve_lazy_batch_device, where every direction waits
        for alsolve_verdict and runs only for a candidate the line search takes, with stop and probes as above; VERDICT
        and NDIR (int32, B each) are allocated (NDIR zeroed) when None, and the dict also holds directions =
        int(NDIR.sum()), the directions computed, beside problem_iters."""
        import torch
        c = self._alsolve_state(st, params)
        B = st.B
        d = self._solve_dir(st, method, gn, DC, GSUM, PC, precond, W, wrows)
        gl, gu, ldgb = self._bounds_operands(B, GL, GU)
        xl, xu, ldxb = self._var_bounds_operands(B, XL, XU)
        if LOG is None:
            LOG = torch.zeros(8 + 2 * B, dtype=torch.int32, device=st.X.device)
        opts = capi.SolveOpts(method=int(method), max_iters=int(max_iters), check_every=int(check_every), compact=int(bool(compact)))
        rep = capi.SolveReport()
        log = self._int_operand(LOG, "LOG", 8 + 2 * B)
        if lazy:
            if VERDICT is None:
                VERDICT = torch.zeros(B, dtype=torch.int32, device=st.X.device)
            if NDIR is None:
                NDIR = torch.zeros(B, dtype=torch.int32, device=st.X.device)
            lz = self._lazy_operands(B, VERDICT, NDIR)
            pr, ps, ldps = self._probe_operands(B, probes, PSUM) if probes else (None, None, 0)
            self._check(self._lib.towr_gpu_alsolve_solve_lazy_batch_device(
                self._h, B, C.byref(opts), C.byref(params), None if stop is None else C.byref(stop),
                None if pr is None else C.byref(pr), C.byref(c), C.byref(d), gl, gu, ldgb, xl, xu, ldxb, ps, ldps,
                log, C.byref(rep), C.byref(lz), self._stream(stream, st.X)))
            out = dict(rounds=rep.rounds, iters_run=rep.iters_run, problem_iters=rep.problem_iters, n_phase=list(rep.n_phase),
                       directions=int(NDIR.sum()))
            if stop is not None:
                out.update(n_acceptable=rep.reserved[0], n_infeasible=rep.reserved[1])
            return out
        if probes is not None:
            pr, ps, ldps = self._probe_operands(B, probes, PSUM) if probes else (None, None, 0)
            self._check(self._lib.towr_gpu_alsolve_solve_probe_batch_device(
                self._h, B, C.byref(opts), C.byref(params), None if stop is None else C.byref(stop),
                None if pr is None else C.byref(pr), C.byref(c), C.byref(d), gl, gu, ldgb, xl, xu, ldxb, ps, ldps,
                log, C.byref(rep), self._stream(stream, st.X)))
            out = dict(rounds=rep.rounds, iters_run=rep.iters_run, problem_iters=rep.problem_iters, n_phase=list(rep.n_phase))
            if stop is not None:
                out.update(n_acceptable=rep.reserved[0], n_infeasible=rep.reserved[1])
            return out
        if not (stop is not None if ex is None else ex):
            if stop is not None:
                raise TowrGpuError("alsolve_solve: stop needs the _ex entry (ex=False was given)")
            self._check(self._lib.towr_gpu_alsolve_solve_batch_device(
                self._h, B, C.byref(opts), C.byref(params), C.byref(c), C.byref(d), gl, gu, ldgb, xl, xu, ldxb,
                log, C.byref(rep), self._stream(stream, st.X)))
            return dict(rounds=rep.rounds, iters_run=rep.iters_run, problem_iters=rep.problem_iters, n_phase=list(rep.n_phase))
        self._check(self._lib.towr_gpu_alsolve_solve_ex_batch_device(
            self._h, B, C.byref(opts), C.byref(params), None if stop is None else C.byref(stop), C.byref(c), C.byref(d),
            gl, gu, ldgb, xl, xu, ldxb,
            log, C.byref(rep), self._stream(stream, st.X)))
        out = dict(rounds=rep.rounds, iters_run=rep.iters_run, problem_iters=rep.problem_iters, n_phase=list(rep.n_phase))
        if stop is not None:
            out.update(n_acceptable=rep.reserved[0], n_infeasible=rep.reserved[1])
        return out

    # -------------------------------------------------------------------- a queue through the slots
    def alsolve_retire_key(self, ISTATE, AGE, KEY, max_age, add=0, B=None, stream=None):
        """The retire key of a batch (towr_gpu.h): KEY[4 b] = 7 for an active row (phase word 0 or 1) whose AGE[b] has
        reached max_age, else the phase word; add > 0 is added to AGE first. ISTATE int32 (>= 4 B, not written), AGE int32
        (>= B), KEY int32 (>= 4 B). B None: ISTATE.numel() // 4."""
        B = ISTATE.numel() // 4 if B is None else int(B)
        self._check(self._lib.towr_gpu_alsolve_retire_key_batch_device(
            self._h, B, self._int_operand(ISTATE, "ISTATE", 4 * B), self._int_operand(AGE, "AGE", B), int(add), int(max_age),
            self._int_operand(KEY, "KEY", 4 * B), self._stream(stream, ISTATE)))

    def alsolve_move_rows(self, ID, slot, out, count, r0=0, reverse=False, stream=None):
        """Copy row r0 + i of every slot array to row ID[r0 + i] of its out array, i < count (reverse: from there into the
        slot row); a negative ID skips its row (towr_gpu.h). `slot`, `out`: equally many arrays as alsolve_swap_rows takes
        them, pairwise with the same row bytes. ID: int32 (>= r0 + count)."""
        if len(slot) != len(out):
            raise TowrGpuError(f"alsolve_move_rows: {len(slot)} slot arrays, {len(out)} out arrays")
        ds = self._row_descs(slot, "alsolve_move_rows", capi.MOVE_MAX_ARRAYS)
        do = self._row_descs(out, "alsolve_move_rows", capi.MOVE_MAX_ARRAYS)
        self._check(self._lib.towr_gpu_alsolve_move_rows_batch_device(
            self._h, self._int_operand(ID, "ID", max(int(r0) + int(count), 0)), int(r0), int(count), len(slot), ds, do,
            int(bool(reverse)), self._stream(stream, ID)))

    def _queue_bounds(self, N, B, lo, up, cols, names, work):
        """(lower, upper, ld, work lower, work upper, work ld, kept tensors) of a queue's bounds: None, 1-D (shared) or
        (N, >= cols) per-problem rows, which need B slot-side work rows (`work`: a pair of tensors, or None to allocate)."""
        import torch
        lp, up_, ld = self._box_operands(N, lo, up, cols, names)
        if ld == 0:
            return lp, up_, 0, None, None, 0, ()
        if work is None:
            work = tuple(torch.empty((B, cols), dtype=torch.float64, device=lo.device) for _ in range(2))
        wl, wu, ldw = self._box_operands(B, work[0], work[1], cols, (names[0] + "W", names[1] + "W", names[2]))
        return lp, up_, ld, wl.value, wu.value, ldw, work

    def alsolve_solve_queue(self, params, st, X0, LAM0=None, method=capi.SOLVE_GN_TILED, gn=None, DC=None, GSUM=None, PC=None,
                            precond=capi.GN_PC_JACOBI, W=None, wrows=None, max_iters=100, check_every=4, GL=None, GU=None,
                            XL=None, XU=None, work=None, ID=None, AGE=None, KEY=None, out=None, LOG=None, stream=None,
                            stop=None):
        """Solve the N = X0.shape[0] problems of a queue through the B = st.B slots of `st` (towr_gpu.h,
        towr_gpu_alsolve_solve_queue_batch_device): a problem leaves its slot when it is frozen or has run max_iters
        iterations (a positive multiple of check_every), and the next one takes the freed row. X0 (N, >= n), LAM0
        (N, >= m) or None (zeros); GL / GU / XL / XU: None, 1-D (shared) or N per-problem rows (only read). st, DC, GSUM, PC
        and W are sized for B; what they hold before and after the call does not matter. work: dict(GLW, GUW, XLW, XUW) of
        B-row tensors for per-problem bounds; ID / AGE (int32, >= B), KEY (int32, >= 4 B), LOG (int32, >= 8 + 2 B) and
        `out` (dict of X_OUT (N, >= n), LAM_OUT (N, >= m), RHO_OUT (N), SCAL_OUT (N, 8), ISTATE_OUT (int32, 4 N),
        ITERS_OUT (int32, N)) are allocated when not given. stop: an alsolve_stop_params(). The call blocks the host.
        Returns dict(rounds, iters_run, problem_iters, n_phase, n_acceptable, n_infeasible) plus the output tensors under
        their names: per problem bit for bit what alsolve_solve leaves for it in one batch of N."""
        import torch
        c = self._alsolve_state(st, params)
        B, N, n, m = st.B, int(X0.shape[0]), self.n, self.m
        dev = st.X.device
        d = self._solve_dir(st, method, gn, DC, GSUM, PC, precond, W, wrows)
        self._check_rows(N, (X0, "X0", n))
        if LAM0 is not None:
            self._check_rows(N, (LAM0, "LAM0", m))
        work = dict(work or {})
        q = capi.SolveQueue(N=N)
        q.X0, q.ldx0 = X0.data_ptr(), X0.stride(0)
        if LAM0 is not None:
            q.LAM0, q.ldl0 = LAM0.data_ptr(), LAM0.stride(0)
        gpair = (work["GLW"], work["GUW"]) if "GLW" in work else None
        xpair = (work["XLW"], work["XUW"]) if "XLW" in work else None
        gl, gu, q.ldgb, q.GLW, q.GUW, q.ldgw, keep_g = self._queue_bounds(N, B, GL, GU, m, ("GL", "GU", "m"), gpair)
        xl, xu, q.ldxb, q.XLW, q.XUW, q.ldxw, keep_x = self._queue_bounds(N, B, XL, XU, n, ("XL", "XU", "n"), xpair)
        q.GL, q.GU, q.XL, q.XU = gl.value, gu.value, xl.value, xu.value
        ints = lambda k: torch.zeros(k, dtype=torch.int32, device=dev)
        ID = ints(B) if ID is None else ID
        AGE = ints(B) if AGE is None else AGE
        KEY = ints(4 * B) if KEY is None else KEY
        LOG = ints(8 + 2 * B) if LOG is None else LOG
        q.ID, q.AGE, q.KEY = (self._int_operand(ID, "ID", B).value, self._int_operand(AGE, "AGE", B).value,
                              self._int_operand(KEY, "KEY", 4 * B).value)
        out = dict(out or {})
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
        for k, make in (("X_OUT", lambda: z(N, n)), ("LAM_OUT", lambda: z(N, m)), ("RHO_OUT", lambda: z(N)),
                        ("SCAL_OUT", lambda: z(N, 8)), ("ISTATE_OUT", lambda: ints(4 * N)), ("ITERS_OUT", lambda: ints(N))):
            if k not in out:
                out[k] = make()
        self._check_rows(N, (out["X_OUT"], "X_OUT", n), (out["LAM_OUT"], "LAM_OUT", m), (out["SCAL_OUT"], "SCAL_OUT", 8))
        if N > 1 and out["SCAL_OUT"].stride(0) != 8:
            raise TowrGpuError("SCAL_OUT: expected contiguous rows of 8")
        _check_per_problem(out["RHO_OUT"], "RHO_OUT", N, self.device)
        q.X_OUT, q.ldxo = out["X_OUT"].data_ptr(), out["X_OUT"].stride(0)
        q.LAM_OUT, q.ldlo = out["LAM_OUT"].data_ptr(), out["LAM_OUT"].stride(0)
        q.RHO_OUT, q.SCAL_OUT = out["RHO_OUT"].data_ptr(), out["SCAL_OUT"].data_ptr()
        q.ISTATE_OUT = self._int_operand(out["ISTATE_OUT"], "ISTATE_OUT", 4 * N).value
        q.ITERS_OUT = self._int_operand(out["ITERS_OUT"], "ITERS_OUT", N).value
        opts = capi.SolveOpts(method=int(method), max_iters=int(max_iters), check_every=int(check_every), compact=1)
        rep = capi.SolveReport()
        self._check(self._lib.towr_gpu_alsolve_solve_queue_batch_device(
            self._h, B, C.byref(opts), C.byref(params), None if stop is None else C.byref(stop), C.byref(c), C.byref(d),
            C.byref(q), self._int_operand(LOG, "LOG", 8 + 2 * (B // 2)), C.byref(rep), self._stream(stream, st.X)))
        del keep_g, keep_x
        res = dict(rounds=rep.rounds, iters_run=rep.iters_run, problem_iters=rep.problem_iters, n_phase=list(rep.n_phase),
                   n_acceptable=rep.reserved[0], n_infeasible=rep.reserved[1])
        res.update(out)
        return res

    def set_products_chunk(self, k: int):
        """Problems per chunk of eval_products_batch_device's values scratch (0 = automatic)."""
        self._check(self._lib.towr_gpu_set_products_chunk(self._h, int(k)))

    def set_cost_grid(self, blocks: int):
        """Blocks of the objective kernel's persistent grid for every launch on this handle (0 = automatic). A launch
        has min(B, blocks) blocks; block k takes problems k, k + blocks, ... The results do not depend on it."""
        self._check(self._lib.towr_gpu_set_cost_grid(self._h, int(blocks)))

    def cost_grid(self, grad: bool = True) -> int:
        """The objective kernel's grid in effect for the gradient (or the f-only) launch."""
        g = self._lib.towr_gpu_cost_grid(self._h, int(bool(grad)))
        if g < 0:
            self._check(g)
        return g

    def step_launches(self):
        """Kernel indices (see kernels()) that one evaluation launches: fusion groups, then the unfused classes."""
        buf = (C.c_int32 * 16)()
        n = self._lib.towr_gpu_step_launches(self._h, buf, 16)
        if n < 0:
            self._check(n)
        return list(buf[:n])

    def kernels(self):
        """[(index, name, n_tiles, algorithmic bytes per problem)] of the launch classes' kernels and the
        fusion groups (index >= 5) this handle uses."""
        out = []
        for k in range(self._lib.towr_gpu_num_kernels()):
            name, nt, by = C.c_char_p(), C.c_int32(), C.c_int64()
            self._check(self._lib.towr_gpu_kernel_info(self._h, k, C.byref(name), C.byref(nt), C.byref(by)))
            if nt.value:
                out.append((k, name.value.decode(), nt.value, by.value))
        return out

    def pattern_outside(self, x) -> int:
        """Reference Jacobian entries at x outside the frozen (x0) pattern: non-zero only on curved terrain,
        where ForceConstraintDiscretized / TorqueConstraintDiscretized blocks appear with x (towr_gpu.h)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        c = C.c_int64()
        self._check(self._lib.towr_gpu_pattern_outside(self._h, x.ctypes.data_as(capi._DP), C.byref(c)))
        return int(c.value)

    def pattern_outside_batch(self, X, counts, stream=None):
        """pattern_outside of every problem of a device batch X (per-problem batch terrains as eval_batch_device)
        into the host int32 array `counts`; synchronous (X is copied to the host and checked there)."""
        import torch
        _check_tensor(X, "X", self.n, self.device)
        if not (isinstance(counts, np.ndarray) and counts.dtype == np.int32 and counts.flags.c_contiguous and counts.size >= X.shape[0]):
            raise TowrGpuError("counts: contiguous int32 numpy array with one entry per problem expected")
        s = stream.cuda_stream if stream is not None else torch.cuda.current_stream(X.device).cuda_stream
        self._check(self._lib.towr_gpu_pattern_outside_batch_device(self._h, X.shape[0], *_opt(X),
                                                                     counts.ctypes.data_as(capi._IP), C.c_void_p(s)))

    def kernel_path(self, kernel: int) -> int:
        """Implementation of launch class `kernel` (0..4): 0 tile kernel, 1 record + stream kernels, -1 unused."""
        rc = self._lib.towr_gpu_kernel_path(self._h, kernel)
        if rc < -1:
            self._check(rc)
        return rc

    def eval_batch_device_kernel(self, kernel, X, G, V, stream):
        """Launch one kernel only: a launch class or a fusion group (roofline accounting)."""
        self._check_batch(X, G, V)
        self._check(self._lib.towr_gpu_eval_batch_device_kernel(
            self._h, kernel, X.shape[0], *_opt(X), *_opt(G), *_opt(V), C.c_void_p(stream.cuda_stream)))

    def set_tiles_per_block(self, t: int):
        self._check(self._lib.towr_gpu_set_tiles_per_block(self._h, t))

    def algorithmic_bytes_per_call(self) -> int:
        return int(self._lib.towr_gpu_algorithmic_bytes_per_call(self._h))
