"""Jacobian-product timings on the GPU box (tool, not product): per call, on one box in one session,
  (a) eval_batch_device (g + J) alone — the yardstick on that box;
  (b) jac_vec_batch_device; (c) jac_tvec_batch_device (overwrite);
  (d) eval_products_batch_device (g, J^T lam and J p) at the automatic chunk and at chunks of 128, 512 and B;
  (e) residual_batch_device (summary and lam+, the handle's bounds): rate = 8 (3 m + 4 + n_constraints) B / time, the
      bytes of G + LAM + LAMP + SUM, beside (f) a device-to-device torch copy moving the same bytes (half read, half
      written);
  (g) eval_auglag_batch_device (g and lam+ in scratch) beside the sum of its parts a + e + c from the same session;
  (h) step_batch_device (XP and the summary, the handle's bounds, scalar step length): rate = 8 (3 n + 5 + n_varsets)
      B / time, the bytes of X + D + XP + SUM, beside (i) a device-to-device torch copy moving the same bytes;
  (j) lbfgs_update_batch_device (every pair accepted): rate = 8 (6 n + 6) B / time, the bytes of X, XN, GR, GRN read and
      the slot of HS and HY written, beside (k) a copy of the same bytes;
  (l) lbfgs_direction_batch_device at mem = MEM (8) with a full history (every pair used, the handle's bounds): rate =
      8 (4 MEM n + 3 n + 5) B / time — the history read twice (2 * 2 * MEM * n), X, GR and D — beside (m) a copy of the
      same bytes and (n) a copy of the bytes with the history counted once (the call's compulsory traffic if the second
      pass were served by a cache);
  (o) auglag_lbfgs_step_batch_device (one inner iteration, mem = MEM) beside the sum of its parts from the same
      session (cost gradient + g auglag + j + l + h) and the share of j + l in it,
  (q) linesearch_batch_device with every problem in SEARCH, its base accepted and its pair stored: rate = 8 (10 n + 30) B /
      time — X, XC, GR, GRC read, the slot of HS and HY written, XC and GRC read again and X, GR written, the scalars —
      beside (r) a copy of the same bytes. The call consumes its operands (X <- XC), so every call is preceded by two
      device copies that restore X and GR; (q0) times those alone and q - q0 is printed;
  (s) auglag_outer_batch_device with every problem's multipliers updated (LAM <- LAMP, 16 m B bytes; ISTATE restored
      before every call: (s0) times that copy alone and s - s0 is printed) beside (u) a copy of the same bytes;
  (t) alsolve_iterate(iters = 1) in a running solve from X (mem = MEM), beside row (o) + (q - q0) + s;
  (v) gn_direction_batch_device at ncg = NCG (8), tol = 0 (every step runs), on the values of (a), lam+ of (e), GR = J^T lam+,
      the handle's bounds: beside NCG (b + c), the same passes by the product kernels (one launch and one LDS staging
      each); (v1) the same call at ncg = 1 (the pass that cannot come from a cache);
  (w) alsolve_gn_iterate(iters = 1) in a running solve of its own from X (ncg = NCG, mu = 1e-2, tol = 1e-3), beside (t),
  (x) gn_pc_direction_batch_device (the Jacobi-preconditioned recursion) on the operands of (v) at ncg = NCG and (x1) at
      ncg = 1, beside v and v1: x1 - v1 is the diagonal pass with the PC row's write, (x - x1) - (v - v1) what the
      division and the PC row's read add to NCG - 1 steps,
  (y) gn_direct_direction_batch_device (the envelope Cholesky solve of the same system, mu = 1e-2) on the operands of (v)
      with a workspace of WROWS rows (default: B), beside x: with NCG=100 ONLY=x,y,z the comparison of DESIGN 4m;
  (z) alsolve_gn_direct_iterate(iters = 1) in a running solve of its own from X (mu = 1e-2), beside (w),
  (yt) gn_tiled_direction_batch_device (the block Cholesky on 16 x 16 tiles) on the operands and with the WROWS of (y), and
  (zt) alsolve_gn_tiled_iterate(iters = 1) in a running solve of its own beside (z): with NCG=100 WROWS=1024
      ONLY=x,y,z,w,yt,zt the comparison of DESIGN 4n (the letters t and u were taken),
for ANYmal trot at B = 4096 and ANYmal stairs with phase-duration optimisation at B = 1024. Each product's achieved
rate is 8 (nnz + n + m) B / time, printed against the 8 TB/s peak. HIP events around windows of REPS calls after a
warm-up of every shape; the windows alternate between the variants and the median and the spread over ROUNDS are
printed. ONLY=b,c,v,v1,x,x1 (a comma list of the letters above) times those variants alone and prints the summary lines
they suffice for. usage: python tools/products_timing.py [anymal|gait|all]"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from towr2025_amd import AlSolveState, TowrGpuProblem, _capi as capi, alsolve_params, gn_params  # noqa: E402
from towr2025_amd import formulation as F  # noqa: E402

REPS = int(os.environ.get("REPS", "20"))
ROUNDS = int(os.environ.get("ROUNDS", "5"))
MEM = int(os.environ.get("MEM", "8"))
NCG = int(os.environ.get("NCG", "8"))
ONLY = set(os.environ.get("ONLY", "").split(",")) - {""}
WROWS = int(os.environ.get("WROWS", "0"))   # rows of the direct direction's workspace (0: B)
PEAK = 8.0e12


def batch_x(p, B, seed=20261019):
    """x0 + noise per variable (phase durations: +-3 % multiplicative), as bench.make_batch perturbs them."""
    rng = np.random.default_rng(seed)
    x0 = p.initial_x()
    sched = np.zeros(p.n, dtype=bool)
    for kind, _ee, c0, n in p.varset_info():
        if kind == capi.VAR_EE_SCHEDULE:
            sched[c0:c0 + n] = True
    X = x0 + 0.02 * rng.standard_normal((B, p.n))
    X[:, sched] = x0[sched] * (1.0 + 0.03 * rng.standard_normal((B, int(sched.sum()))))
    return X


def run(name, f, B):
    dev = torch.device("cuda", 0)
    f.params_.enable_stance_tracking = False   # the start / goal variable bounds (the step kernel's box)
    p = TowrGpuProblem(f.to_desc(), device=0, data=f.var_bounds_data())
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ld = lambda k: (k + 15) // 16 * 16
    X = torch.from_numpy(batch_x(p, B)).to(dev)
    G = torch.empty((B, ld(p.m)), dtype=torch.float64, device=dev)
    V = torch.empty((B, ld(p.nnz)), dtype=torch.float64, device=dev)
    P = torch.randn((B, ld(p.n)), dtype=torch.float64, device=dev)
    LAM = torch.randn((B, ld(p.m)), dtype=torch.float64, device=dev)
    Y, Z = torch.empty_like(LAM), torch.empty_like(P)
    ns = p.desc.n_constraints
    LAMP, SUM = torch.empty_like(LAM), torch.empty((B, ld(4 + ns)), dtype=torch.float64, device=dev)
    bytes_res = 8 * (3 * p.m + 4 + ns) * B
    src = torch.randn(bytes_res // 16, dtype=torch.float64, device=dev)
    dst = torch.empty_like(src)
    rho = 10.0
    nv = p.desc.n_varsets
    XP, SSUM = torch.empty_like(P), torch.empty((B, ld(5 + nv)), dtype=torch.float64, device=dev)
    Xs = torch.zeros_like(P)
    Xs[:, :p.n] = X
    bytes_step = 8 * (3 * p.n + 5 + nv) * B
    src_s = torch.randn(bytes_step // 16, dtype=torch.float64, device=dev)
    dst_s = torch.empty_like(src_s)
    # L-BFGS: a full history of MEM pairs with positive curvature (y = c s, c per column in [0.5, 2]), X -> XN a small move
    mem = MEM
    HS = 0.01 * torch.randn((B * mem, ld(p.n)), dtype=torch.float64, device=dev)
    HY = HS * (0.5 + 1.5 * torch.rand((1, ld(p.n)), dtype=torch.float64, device=dev))
    HMETA = torch.tensor([[mem, 0]] * B, dtype=torch.int32, device=dev)
    XN = Xs + 0.01 * torch.randn_like(Xs)
    GR = torch.randn_like(P)
    GRN = GR + 1.3 * (XN - Xs)
    D, USUM, DSUM = torch.empty_like(P), torch.empty((B, 16), dtype=torch.float64, device=dev), torch.empty((B, 16), dtype=torch.float64, device=dev)
    Fv, GRo = torch.empty(B, dtype=torch.float64, device=dev), torch.empty_like(P)
    RSUM = torch.empty_like(SUM)
    # the fused iteration's own operands: a history of its own, X = Xs + a small move and the true gradient at Xs as
    # GRPREV, so that its pair is a pair of the augmented Lagrangian (the share accepted is printed)
    HS2, HY2, HMETA2 = HS.clone(), HY.clone(), HMETA.clone()
    XN2 = Xs + 1e-4 * torch.randn_like(Xs)
    GRP = torch.empty_like(P)
    p.eval_cost_batch_device(Xs, Fv, GRAD=GRP, stream=stream)
    p.eval_auglag_batch_device(Xs, RSUM, GRP, LAM=LAM, rho=rho, accumulate=True, stream=stream)
    USUM2 = torch.zeros((B, 16), dtype=torch.float64, device=dev)
    bytes_upd = 8 * (6 * p.n + 6) * B
    bytes_dir = 8 * (4 * mem * p.n + 3 * p.n + 5) * B
    bytes_dir1 = 8 * (2 * mem * p.n + 3 * p.n + 5) * B
    copies = {}
    for key, nb in (("k", bytes_upd), ("m", bytes_dir), ("n", bytes_dir1)):
        a = torch.randn(nb // 16, dtype=torch.float64, device=dev)
        copies[key] = (a, torch.empty_like(a))

    # the resident loop: (q) a state whose every problem accepts and stores its pair (MC = -1e300 <= M0 + c1 gs whenever
    # gs <= 0; XC = X - 0.01 GR), X and GR restored before every call; (s) every problem forced into the multiplier
    # update; (t) a running solve of its own
    par = alsolve_params(mem=mem, shrink=0.1, curv_eps=1e-14, alpha_min=1e-16, max_inner=5)
    sq = AlSolveState.allocate(p, B, mem)
    Xq, GRq = Xs[:, :p.n].contiguous(), GR[:, :p.n].contiguous()
    sq.XC.copy_(Xq - 0.01 * GRq)
    sq.GRC.copy_(GRq + 1.3 * (sq.XC - Xq))
    sq.HS.copy_(HS[:, :p.n]); sq.HY.copy_(HY[:, :p.n]); sq.HMETA.copy_(HMETA.flatten())
    sq.FC.fill_(-1e300); sq.ALPHA.fill_(1.0); sq.RHO.fill_(rho)
    sq.SCAL[:, 0] = 1e300
    sq.ISTATE.copy_(torch.tensor([[1, 0, 0, 0]] * B, dtype=torch.int32, device=dev).flatten())
    IS_outer = torch.tensor([[1, 1, 5, 0]] * B, dtype=torch.int32, device=dev).flatten()
    so = AlSolveState.allocate(p, B, mem)
    so.LAMP.copy_(LAM[:, :p.m]); so.RHO.fill_(rho)
    so.SCAL.copy_(torch.tensor([[0.0, 0.5, 0.1, 0.1, 0.0, 0.0, 0.0, 0.0]] * B, dtype=torch.float64, device=dev))
    stt = AlSolveState.allocate(p, B, mem)
    stt.X.copy_(Xs[:, :p.n])
    part = alsolve_params(mem=mem, shrink=0.1, curv_eps=1e-14, alpha_min=1e-16, max_inner=100, max_outer=1000)
    p.alsolve_init(part, stt, stream=stream)
    # the GN direction on (V, lam+ of the residual, GR = J^T lam+) and a running GN solve of its own
    p.eval_batch_device(X, G, V, stream=stream)
    p.residual_batch_device(G, SUM, LAM=LAM, rho=rho, LAMP=LAMP, stream=stream)
    GRg, Dg, GSUM = torch.empty_like(P), torch.empty_like(P), torch.empty((B, 16), dtype=torch.float64, device=dev)
    Dx, PCx, XSUM = torch.empty_like(P), torch.empty_like(P), torch.empty((B, 16), dtype=torch.float64, device=dev)
    p.jac_tvec_batch_device(V, LAMP, GRg, stream=stream)
    gnv, gnv1, gnw = gn_params(ncg=NCG, mu=1e-2, tol=0.0), gn_params(ncg=1, mu=1e-2, tol=0.0), gn_params(ncg=NCG, mu=1e-2, tol=1e-3)
    stg = AlSolveState.allocate(p, B, mem)
    stg.X.copy_(Xs[:, :p.n])
    p.alsolve_init(part, stg, stream=stream)
    DCg, GSg = torch.empty_like(stg.X), torch.empty((B, 8), dtype=torch.float64, device=dev)
    codes_g, steps_g = [], []
    codes = []
    # the direct direction's workspace, its outputs and a running solve of its own
    info = p.gn_factor_info()
    wrows = min(B, WROWS) if WROWS > 0 else B
    Wd = torch.empty((wrows, ld(info["ldw_min"])), dtype=torch.float64, device=dev)
    Dy, YSUM = torch.empty_like(P), torch.empty((B, 16), dtype=torch.float64, device=dev)
    sty = AlSolveState.allocate(p, B, mem)
    sty.X.copy_(Xs[:, :p.n])
    p.alsolve_init(part, sty, stream=stream)
    DCy, GSy = torch.empty_like(sty.X), torch.empty((B, 8), dtype=torch.float64, device=dev)
    codes_y, dcodes_y = [], []
    # the tiled direction's workspace, its outputs and a running solve of its own
    tinfo = p.gn_tile_info()
    Wt = torch.empty((wrows, ld(tinfo["ldw_min"])), dtype=torch.float64, device=dev)
    Dt, TSUM = torch.empty_like(P), torch.empty((B, 16), dtype=torch.float64, device=dev)
    stz = AlSolveState.allocate(p, B, mem)
    stz.X.copy_(Xs[:, :p.n])
    p.alsolve_init(part, stz, stream=stream)
    DCt, GSt = torch.empty_like(stz.X), torch.empty((B, 8), dtype=torch.float64, device=dev)
    codes_t, dcodes_t = [], []
    bytes_ls = 8 * (10 * p.n + 30) * B
    bytes_out = 8 * 2 * p.m * B
    for key, nb in (("r", bytes_ls), ("u", bytes_out)):
        a = torch.randn(nb // 16, dtype=torch.float64, device=dev)
        copies[key] = (a, torch.empty_like(a))

    # the three calls go to the C-ABI directly with their state structs built once: the Python methods' operand checks
    # (some 20 tensors per call) would otherwise be what a 40 us kernel is timed against
    import ctypes as C
    sp = C.c_void_p(stream.cuda_stream)
    cq, co, ct = p._alsolve_state(sq, par), p._alsolve_state(so, par), p._alsolve_state(stt, part)
    ls_call = lambda: p._check(p._lib.towr_gpu_linesearch_batch_device(p._h, B, C.byref(par), C.byref(cq), None, None, 0, sp))
    outer_call = lambda: p._check(p._lib.towr_gpu_auglag_outer_batch_device(p._h, B, C.byref(par), C.byref(co), sp))
    cg = p._alsolve_state(stg, part)
    gn_iter_call = lambda: p._check(p._lib.towr_gpu_alsolve_gn_iterate_batch_device(
        p._h, B, 1, C.byref(part), C.byref(cg), C.byref(gnw), C.c_void_p(DCg.data_ptr()), C.c_void_p(GSg.data_ptr()), GSg.stride(0),
        None, None, 0, None, None, 0, sp))
    cy = p._alsolve_state(sty, part)
    direct_iter_call = lambda: p._check(p._lib.towr_gpu_alsolve_gn_direct_iterate_batch_device(
        p._h, B, 1, C.byref(part), C.byref(cy), C.byref(gnw), C.c_void_p(DCy.data_ptr()), C.c_void_p(GSy.data_ptr()), GSy.stride(0),
        C.c_void_p(Wd.data_ptr()), Wd.stride(0), wrows, None, None, 0, None, None, 0, sp))
    cz = p._alsolve_state(stz, part)
    tiled_iter_call = lambda: p._check(p._lib.towr_gpu_alsolve_gn_tiled_iterate_batch_device(
        p._h, B, 1, C.byref(part), C.byref(cz), C.byref(gnw), C.c_void_p(DCt.data_ptr()), C.c_void_p(GSt.data_ptr()), GSt.stride(0),
        C.c_void_p(Wt.data_ptr()), Wt.stride(0), wrows, None, None, 0, None, None, 0, sp))
    iter_call = lambda: p._check(p._lib.towr_gpu_alsolve_iterate_batch_device(p._h, B, 1, C.byref(part), C.byref(ct), None, None, 0,
                                                                              None, None, 0, sp))

    def restore_q():
        sq.X.copy_(Xq)
        sq.GR.copy_(GRq)

    def fused(chunk):
        def f():
            p.set_products_chunk(chunk)
            p.eval_products_batch_device(X, G=G, LAM=LAM, Z=Z, P=P, Y=Y, stream=stream)
        return f
    variants = [("a eval_batch_device", lambda: p.eval_batch_device(X, G, V, stream=stream)),
                ("b jac_vec", lambda: p.jac_vec_batch_device(V, P, Y, stream=stream)),
                ("c jac_tvec", lambda: p.jac_tvec_batch_device(V, LAM, Z, stream=stream)),
                ("d fused chunk auto", fused(0)), ("d fused chunk 128", fused(128)), ("d fused chunk 512", fused(512)),
                (f"d fused chunk B={B}", fused(B)),
                ("e residual", lambda: p.residual_batch_device(G, SUM, LAM=LAM, rho=rho, LAMP=LAMP, stream=stream)),
                ("f copy, same bytes", lambda: dst.copy_(src)),
                ("g auglag fused auto", lambda: (p.set_products_chunk(0),
                                                 p.eval_auglag_batch_device(X, SUM, Z, LAM=LAM, rho=rho, stream=stream))),
                ("h step", lambda: p.step_batch_device(Xs, P, SSUM, XP=XP, alpha=0.01, stream=stream)),
                ("i copy, step's bytes", lambda: dst_s.copy_(src_s)),
                ("j lbfgs update", lambda: p.lbfgs_update_batch_device(Xs, XN, GR, GRN, HS, HY, HMETA, USUM, mem, stream=stream)),
                ("k copy, update's bytes", lambda: copies["k"][1].copy_(copies["k"][0])),
                (f"l lbfgs direction mem={mem}", lambda: p.lbfgs_direction_batch_device(GR, HS, HY, HMETA, D, DSUM, mem, X=Xs, stream=stream)),
                ("m copy, direction's bytes", lambda: copies["m"][1].copy_(copies["m"][0])),
                ("n copy, history once", lambda: copies["n"][1].copy_(copies["n"][0])),
                ("p cost gradient", lambda: p.eval_cost_batch_device(Xs, Fv, GRAD=GRo, stream=stream)),
                (f"o auglag lbfgs step mem={mem}", lambda: (p.set_products_chunk(0), p.auglag_lbfgs_step_batch_device(
                    XN2, GRo, XP, SSUM, RSUM, DSUM, HS2, HY2, HMETA2, mem, XPREV=Xs, GRPREV=GRP, USUM=USUM2, LAM=LAM, rho=rho,
                    alpha=1e-6, F=Fv, stream=stream))),
                ("q linesearch + restore", lambda: (restore_q(), ls_call())),
                ("q0 restore alone", restore_q),
                ("r copy, linesearch's bytes", lambda: copies["r"][1].copy_(copies["r"][0])),
                ("s outer (lam update)", lambda: (so.ISTATE.copy_(IS_outer), outer_call())),
                ("s0 ISTATE restore alone", lambda: so.ISTATE.copy_(IS_outer)),
                ("u copy, outer's bytes", lambda: copies["u"][1].copy_(copies["u"][0])),
                (f"t alsolve iterate mem={mem}", lambda: (p.set_products_chunk(0), iter_call(),
                                                         codes.append(stt.LSUM[:, 0].clone()))),
                (f"v gn direction ncg={NCG}", lambda: p.gn_direction_batch_device(gnv, V, LAMP, GRg, Dg, GSUM, rho=rho, X=Xs, stream=stream)),
                ("v1 gn direction ncg=1", lambda: p.gn_direction_batch_device(gnv1, V, LAMP, GRg, Dg, GSUM, rho=rho, X=Xs, stream=stream)),
                (f"w alsolve gn iterate ncg={NCG}", lambda: (p.set_products_chunk(0), gn_iter_call(),
                                                            codes_g.append(stg.LSUM[:, 0].clone()), steps_g.append(GSg[:, 0].clone()))),
                (f"x gn pc direction ncg={NCG}", lambda: p.gn_pc_direction_batch_device(gnv, V, LAMP, GRg, Dx, XSUM, PC=PCx, rho=rho, X=Xs,
                                                                                       stream=stream)),
                ("x1 gn pc direction ncg=1", lambda: p.gn_pc_direction_batch_device(gnv1, V, LAMP, GRg, Dx, XSUM, PC=PCx, rho=rho, X=Xs,
                                                                                   stream=stream)),
                (f"y gn direct wrows={wrows}", lambda: p.gn_direct_direction_batch_device(gnv, V, LAMP, GRg, Dy, YSUM, Wd, wrows=wrows, rho=rho,
                                                                                         X=Xs, stream=stream)),
                ("z alsolve gn direct iterate", lambda: (p.set_products_chunk(0), direct_iter_call(),
                                                         codes_y.append(sty.LSUM[:, 0].clone()), dcodes_y.append(GSy[:, 5].clone()))),
                (f"yt gn tiled wrows={wrows}", lambda: p.gn_tiled_direction_batch_device(gnv, V, LAMP, GRg, Dt, TSUM, Wt, wrows=wrows, rho=rho,
                                                                                        X=Xs, stream=stream)),
                ("zt alsolve gn tiled iterate", lambda: (p.set_products_chunk(0), tiled_iter_call(),
                                                         codes_t.append(stz.LSUM[:, 0].clone()), dcodes_t.append(GSt[:, 5].clone())))]
    if ONLY:
        variants = [(k, fn) for k, fn in variants if k.split()[0] in ONLY]
    for _, fn in variants:   # warm-up: every shape, the tables' upload, the scratch at its largest
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k, _ in variants}
    for _ in range(ROUNDS):
        for k, fn in variants:
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(REPS):
                fn()
            z.record(stream)
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(z) / REPS)
    bytes_prod = 8 * (p.nnz + p.n + p.m) * B
    print(f"{name}: B={B} n={p.n} m={p.m} nnz={p.nnz}  product bytes {bytes_prod / 1e9:.3f} GB, V {8 * p.nnz * B / 2**30:.2f} GiB", flush=True)
    for k, _ in variants:
        t = times[k]
        med = statistics.median(t)
        nbytes = (bytes_prod if k[0] in "bc" else bytes_res if k[0] in "ef" else bytes_step if k[0] in "hi" else
                  bytes_upd if k[0] in "jk" else bytes_dir if k[0] in "lm" else bytes_dir1 if k[0] == "n" else
                  bytes_ls if k[:2] in ("q ", "r ") else bytes_out if k[0] in "su" else 0)
        rate = f"  {nbytes / (med * 1e-3) / 1e12:.2f} TB/s = {100 * nbytes / (med * 1e-3) / PEAK:.0f} % of 8 TB/s" if nbytes else ""
        print(f"  {k:22s} {med:.4f} ms  (min {min(t):.4f} max {max(t):.4f}){rate}", flush=True)
    if not ONLY or {"v", "v1", "x", "x1"} <= ONLY:
        mx = {k.split()[0]: statistics.median(times[k]) for k, _ in variants if k.split()[0] in ("v", "v1", "x", "x1")}
        print(f"  gn pc direction ncg={NCG}: x {mx['x']:.4f} ms vs v {mx['v']:.4f} ms, ratio {mx['x'] / mx['v']:.3f}; ncg=1: x1 {mx['x1']:.4f} ms "
              f"vs v1 {mx['v1']:.4f} ms, x1 - v1 {mx['x1'] - mx['v1']:.4f} ms; per step (x - x1) / {NCG - 1} "
              f"{(mx['x'] - mx['x1']) / max(NCG - 1, 1):.4f} ms vs (v - v1) / {NCG - 1} {(mx['v'] - mx['v1']) / max(NCG - 1, 1):.4f} ms; "
              f"columns whose M was replaced {XSUM[:, 7].mean().item():.2f}", flush=True)
    if not ONLY or {"x", "y"} <= ONLY:
        my = {k.split()[0]: statistics.median(times[k]) for k, _ in variants if k.split()[0] in ("x", "y", "z", "w")}
        line = (f"  gn direct: envelope {info['envelope']} entries ({8 * info['envelope'] / 1024:.0f} KiB per problem), bandwidth "
                f"{info['bandwidth']}, wrows {wrows}: y {my['y']:.4f} ms vs x (ncg={NCG}) {my['x']:.4f} ms, ratio {my['y'] / my['x']:.3f}; "
                f"solved {(YSUM[:, 5] == 1).double().mean().item():.3f} of the problems")
        if "z" in my:
            hist_y = torch.bincount(torch.stack(codes_y).flatten().to(torch.int64), minlength=6).tolist()
            line += (f"; direct iteration z {my['z']:.4f} ms" + (f" vs w {my['w']:.4f} ms" if "w" in my else "") +
                     f"; solved per timed iteration {(torch.stack(dcodes_y) == 1).double().mean().item():.3f}; LSUM[0] codes 0..5 {hist_y}")
        print(line, flush=True)
    if not ONLY or {"y", "yt"} <= ONLY:
        mt = {k.split()[0]: statistics.median(times[k]) for k, _ in variants if k.split()[0] in ("y", "z", "yt", "zt")}
        line = (f"  gn tiled: {tinfo['tiles']} tiles ({8 * tinfo['ldw_min'] / 1024:.0f} KiB per problem), wrows {wrows}: yt {mt['yt']:.4f} ms "
                f"vs y {mt['y']:.4f} ms, yt / y {mt['yt'] / mt['y']:.4f}; code 1 on {(TSUM[:, 5] == 1).double().mean().item():.3f} (yt) and "
                f"{(YSUM[:, 5] == 1).double().mean().item():.3f} (y) of the problems")
        if "z" in mt and "zt" in mt:
            hist_t = torch.bincount(torch.stack(codes_t).flatten().to(torch.int64), minlength=6).tolist()
            line += (f"; tiled iteration zt {mt['zt']:.4f} ms vs z {mt['z']:.4f} ms, zt / z {mt['zt'] / mt['z']:.4f}; solved per timed "
                     f"iteration {(torch.stack(dcodes_t) == 1).double().mean().item():.3f}; LSUM[0] codes 0..5 {hist_t}")
        print(line, flush=True)
    if ONLY:
        p.set_products_chunk(0)
        return
    parts = sum(statistics.median(times[k]) for k in ("a eval_batch_device", "e residual", "c jac_tvec"))
    print(f"  residual bytes {bytes_res / 1e9:.3f} GB; auglag parts a + e + c {parts:.4f} ms, fused / parts "
          f"{statistics.median(times['g auglag fused auto']) / parts:.3f}", flush=True)
    med = {k[0]: statistics.median(times[k]) for k, _ in variants if k[0] in "pgjlho"}
    parts = med["p"] + med["g"] + med["j"] + med["l"] + med["h"]
    print(f"  update bytes {bytes_upd / 1e9:.3f} GB, direction bytes {bytes_dir / 1e9:.3f} GB (history once {bytes_dir1 / 1e9:.3f} GB); "
          f"lbfgs step parts p + g + j + l + h {parts:.4f} ms, fused / parts {med['o'] / parts:.3f}, "
          f"update + direction {med['j'] + med['l']:.4f} ms = {100 * (med['j'] + med['l']) / med['o']:.1f} % of the fused iteration; "
          f"accepted: update {USUM[:, 3].mean().item():.2f}, fused {USUM2[:, 3].mean().item():.2f}; pairs used: direction "
          f"{DSUM[:, 0].mean().item():.2f}", flush=True)
    mq = {k.split()[0]: statistics.median(times[k]) for k, _ in variants if k.split()[0] in ("q", "q0", "r", "s", "s0", "u", "t")}
    ls = mq["q"] - mq["q0"]
    mq["s"] -= mq["s0"]
    so.ISTATE.copy_(IS_outer)
    outer_call()   # (the phases printed below are an outer update's)
    hist = torch.bincount(torch.stack(codes).flatten().to(torch.int64), minlength=6).tolist()
    print(f"  linesearch bytes {bytes_ls / 1e9:.3f} GB: q - q0 {ls:.4f} ms = {bytes_ls / (ls * 1e-3) / 1e12:.2f} TB/s, copy / (q - q0) "
          f"{mq['r'] / ls:.2f}; stored {sq.LSUM[:, 6].mean().item():.2f}; outer: s - s0 {mq['s']:.4f} ms, copy / (s - s0) {mq['u'] / mq['s']:.2f}, phases after "
          f"{torch.bincount(so.ISTATE.view(B, 4)[:, 0].to(torch.int64), minlength=5).tolist()}; iteration t {mq['t']:.4f} ms vs "
          f"o + (q - q0) + (s - s0) {med['o'] + ls + mq['s']:.4f} ms, ratio {mq['t'] / (med['o'] + ls + mq['s']):.3f}; LSUM[0] codes 0..5 over the "
          f"timed iterations {hist}", flush=True)
    mv = {k.split()[0]: statistics.median(times[k]) for k, _ in variants if k.split()[0] in ("b", "c", "v", "v1", "w", "t")}
    hist_g = torch.bincount(torch.stack(codes_g).flatten().to(torch.int64), minlength=6).tolist()
    print(f"  gn direction ncg={NCG}: v {mv['v']:.4f} ms vs {NCG} (b + c) {NCG * (mv['b'] + mv['c']):.4f} ms, ratio "
          f"{mv['v'] / (NCG * (mv['b'] + mv['c'])):.3f}; per step (v - v1) / {NCG - 1} {(mv['v'] - mv['v1']) / max(NCG - 1, 1):.4f} ms vs b + c "
          f"{mv['b'] + mv['c']:.4f} ms, first step v1 {mv['v1']:.4f} ms; gn iteration w "
          f"{mv['w']:.4f} ms vs t {mv['t']:.4f} ms, w - t {mv['w'] - mv['t']:.4f} ms; CG steps per timed iteration "
          f"{torch.stack(steps_g).mean().item():.2f}; LSUM[0] codes 0..5 {hist_g}", flush=True)
    p.set_products_chunk(0)


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    if which in ("anymal", "all"):
        run("anymal_trot", F.anymal_trot(), int(os.environ.get("B", "4096")))
    if which in ("gait", "all"):
        run("anymal_stairs_gaitopt", F.anymal_trot(terrain=F.HeightMap.MakeTerrain(F.HeightMap.StairsID), optimize_timings=True),
            int(os.environ.get("B_GAIT", "1024")))
