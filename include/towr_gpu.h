/*
 * towr_gpu.h — C-ABI of the MI355X (gfx950) constraint/Jacobian evaluation engine for towr's NLP.
 *
 * This is the drop-in boundary for the reference's eval_g / eval_jac_g hot path
 * (hexb66/towr2025). In the reference, IPOPT calls ifopt's IpoptAdapter::eval_g /
 * eval_jac_g, which call ifopt::Problem::EvalConstraints / EvalNonzerosOfJacobian, which call
 * every ifopt::ConstraintSet's GetValues() and FillJacobianBlock(var_set, jac)
 * (towr/include/towr/constraints/time_discretization_constraint.h:50-73,
 *  towr/src/constraints/time_discretization_constraint.cc:65-96). Those callbacks are what
 * this library replaces; IPOPT keeps running on the host.
 *
 * Plain C: POD structs, plain pointers and sizes, int status codes (0 = ok, < 0 = error),
 * no exceptions cross the boundary, no torch types. One handle per host thread; calls on a
 * handle are serialised on that handle's HIP stream.
 *
 * Numbers: every value is IEEE binary64, as in the reference (Eigen double throughout).
 * Jacobian layout: CSR in ifopt order — rows = constraint sets in the order given, each set's
 * rows contiguous; columns = variable sets in the order given; within a row, columns ascend
 * (Eigen::SparseMatrix<double,RowMajor> after setFromTriplets/makeCompressed, which is the
 * (iRow, jCol) order ifopt's IpoptAdapter::eval_jac_g emits).
 */
#ifndef TOWR_GPU_H_
#define TOWR_GPU_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TOWR_GPU_ABI_VERSION 4

#define TOWR_MAX_EE          4
#define TOWR_MAX_PHASES      48
#define TOWR_MAX_VARSETS     (2 + 5 * TOWR_MAX_EE)
#define TOWR_MAX_CONSTRAINTS 64
#define TOWR_MAX_COSTS       128

/* ---- status codes ---------------------------------------------------------------------- */
#define TOWR_OK                  0
#define TOWR_ERR_INVALID        -1   /* malformed description / argument                       */
#define TOWR_ERR_UNSUPPORTED    -2   /* valid for the reference, not (yet) for this engine     */
#define TOWR_ERR_HIP            -3   /* HIP runtime failure (message in towr_gpu_last_error)    */
#define TOWR_ERR_NO_DEVICE      -4   /* no gfx950 device / extension not loadable on this host  */

/* ---- terrain: HeightMap::TerrainID (towr/include/towr/terrain/height_map.h:79-86) --------- */
enum towr_terrain_id {
  TOWR_TERRAIN_FLAT       = 0, /* FlatGround   p[0]=height                                  (height_map_examples.h:45-52)  */
  TOWR_TERRAIN_BLOCK      = 1, /* Block        p[0]=block_start p[1]=length p[2]=height p[3]=eps (:57-69)            */
  TOWR_TERRAIN_STAIRS     = 2, /* Stairs       p[0]=first_step_start p[1]=first_step_width
                                  p[2]=height_first_step p[3]=height_second_step p[4]=width_top   (:74-84)           */
  TOWR_TERRAIN_GAP        = 3, /* Gap          p[0]=gap_start p[1]=w p[2]=h                  (:89-112)                */
  TOWR_TERRAIN_SLOPE      = 4, /* Slope        p[0]=slope_start p[1]=up_length p[2]=down_length p[3]=height_center (:117-131) */
  TOWR_TERRAIN_CHIMNEY    = 5, /* Chimney      p[0]=x_start p[1]=length p[2]=y_start p[3]=slope (:136-148)             */
  TOWR_TERRAIN_CHIMNEY_LR = 6, /* ChimneyLR    p[0]=x_start p[1]=length p[2]=y_start p[3]=slope (:153-166)             */
  TOWR_TERRAIN_STEPS      = 7  /* FiveStepStairs of towr/test/hopper_example.cc:53-86:
                                  p[0]=stairs_start p[1]=step_depth p[2]=step_height p[3]=num_steps              */
};

typedef struct {
  int32_t id;              /* towr_terrain_id                                                  */
  int32_t reserved;
  double  friction_coeff;  /* HeightMap::friction_coeff_ = 0.5 (height_map.h:136)             */
  double  p[8];            /* per-type parameters, see enum                                    */
} towr_terrain_t;

/* ---- robot: SingleRigidBodyDynamics + KinematicModel (models/examples/ *.h) ---------------- */
typedef struct {
  double  mass;                       /* DynamicModel::m_                                       */
  double  gravity;                    /* DynamicModel::g_ = 9.80665 (dynamic_model.cc:37)        */
  double  inertia[6];                 /* Ixx Iyy Izz Ixy Ixz Iyz, BuildInertiaTensor convention
                                         (single_rigid_body_dynamics.cc:36-44)                   */
  int32_t n_ee;
  int32_t reserved;
  double  nominal_stance[TOWR_MAX_EE][3];  /* KinematicModel::nominal_stance_                  */
  double  max_dev[TOWR_MAX_EE][3];         /* KinematicModel::max_dev_from_nominal_            */
  double  min_dev[TOWR_MAX_EE][3];         /* KinematicModel::min_dev_from_nominal_            */
} towr_robot_t;

/* ---- variable sets: ids of towr/include/towr/variables/variable_names.h:43-75 ------------- */
enum towr_varset_kind {
  TOWR_VAR_BASE_LIN    = 0,  /* "base-lin"      NodesVariablesAll                              */
  TOWR_VAR_BASE_ANG    = 1,  /* "base-ang"      NodesVariablesAll (Euler ZYX)                  */
  TOWR_VAR_EE_MOTION   = 2,  /* "ee-motion_i"   NodesVariablesEEMotion                         */
  TOWR_VAR_EE_ANG      = 3,  /* "ee-ang_i"      NodesVariablesEEAng                            */
  TOWR_VAR_EE_FORCE    = 4,  /* "ee-force_i"    NodesVariablesEEForce                          */
  TOWR_VAR_EE_TORQUE   = 5,  /* "ee-torque_i"   NodesVariablesEETorque                         */
  TOWR_VAR_EE_SCHEDULE = 6   /* "ee-schedule_i" PhaseDurations (only with optimize_timings)    */
};

typedef struct {
  int32_t kind;  /* towr_varset_kind           */
  int32_t ee;    /* endeffector id (ee sets)   */
} towr_varset_t;

/* ---- constraint sets: Parameters::ConstraintName (parameters.h:141-152) --------------------- */
enum towr_constraint_kind {
  TOWR_C_DYNAMIC          = 0, /* DynamicConstraint            dt; T                  (dynamic_constraint.cc:38-148)             */
  TOWR_C_RANGE_OF_MOTION  = 1, /* RangeOfMotionConstraint      dt; T; ee              (range_of_motion_constraint.cc:37-131)     */
  TOWR_C_FORCE            = 2, /* ForceConstraint (node-based) ee; p[0]=force limit   (force_constraint.cc:37-171)               */
  TOWR_C_FORCE_DISCRETIZED= 3, /* ForceConstraintDiscretized   dt; T; ee; p[0]=limit  (force_constraint_discretized.cc:71-221)   */
  TOWR_C_TERRAIN          = 4, /* TerrainConstraint            ee; p[0]=min p[1]=max  (terrain_constraint.cc:36-111)             */
  TOWR_C_BASE_MOTION      = 5, /* BaseMotionConstraint         dt; T; p[0..5]=ax,ay,lz bounds (base_motion_constraint.cc:38-91)  */
  TOWR_C_SPLINE_ACC       = 6, /* SplineAccConstraint          ee=0 base-lin, ee=1 base-ang (spline_acc_constraint.cc:34-86)     */
  TOWR_C_BASE_HEIGHT      = 7, /* BaseHeightConstraint         p[0]=safety distance   (base_height_constraint.cc:35-110)         */
  TOWR_C_SWING            = 8, /* SwingConstraint              ee; p[0]=t_swing_avg (0.3, swing_constraint.h:68)                  */
  TOWR_C_TOTAL_DURATION   = 9, /* TotalDurationConstraint      ee; T                  (total_duration_constraint.cc:36-72)       */
  TOWR_C_TORQUE_DISCRETIZED = 10, /* TorqueConstraintDiscretized ee; T; dt; p[0..3] = tx_min, tx_max, ty_min, ty_max;
                                     p[4] = k_friction                     (torque_constraint_discretized.cc:69-235) */
  TOWR_C_TORQUE           = 11, /* TorqueConstraint (node-based) ee; p[0..4] as above      (torque_constraint.cc:36-194)  */
  TOWR_C_TERRAIN_HARD     = 12, /* TerrainConstraintHard       ee; T; dt              (terrain_constraint_hard.cc:35-132)       */
  TOWR_C_EE_LINEAR        = 13, /* EELinearConstraint          T; dt; ip[0] = target (0 motion, 1 ang), ip[1] = deriv (0 pos,
                                     1 vel), ip[2] = n_terms (<= 6), ip[3 + i] = ee_i * 3 + dim_i; p[i] = coeff_i;
                                     (ee_linear_constraint.cc:5-48; the bound tolerance is side data TOWR_DATA_BOUNDS)  */
  TOWR_C_LINEAR_EQ        = 14  /* LinearEqualityConstraint    g = M x_set (linear_constraint.cc:35-80): ip[0] = variable set
                                     (index in AddVariableSet order), ip[1] = rows of M; M itself is side data
                                     TOWR_DATA_LINEAR_M (towr_gpu_create_ex). Jacobian = M.sparseView(): the nonzeros of M.
                                     The offset v only enters the bounds (-v): side data TOWR_DATA_BOUNDS            */
};

/* Role of a constraint set in the description:
 *   TOWR_ROLE_HARD: an ifopt constraint set (AddConstraintSet) — its rows are part of g and J;
 *   TOWR_ROLE_SOFT: only wrapped by a SoftConstraint cost term (AddCostSet(SoftConstraint(c)),
 *                   soft_constraint.cc:34-69) — not part of g / J; the cost term evaluates it.       */
enum towr_constraint_role { TOWR_ROLE_HARD = 0, TOWR_ROLE_SOFT = 1 };

typedef struct {
  int32_t kind;   /* towr_constraint_kind                                                       */
  int32_t ee;     /* endeffector id, or spline id for TOWR_C_SPLINE_ACC                        */
  double  T;      /* total horizon the constraint was constructed with                         */
  double  dt;     /* discretisation step of TimeDiscretizationConstraint subclasses            */
  double  p[6];   /* per-kind parameters (see enum)                                            */
  int32_t ip[9];  /* per-kind integer parameters (EELinear, LinearEquality)                     */
  int32_t role;   /* towr_constraint_role (0 = hard)                                            */
} towr_constraint_t;

/* ---- cost terms: NlpFormulation::GetCosts (nlp_formulation.cc:604-680) ------------------------ */
enum towr_cost_kind {
  TOWR_COST_NODE        = 0, /* NodeCost: ip[0] = variable set kind (towr_varset_kind), ee, ip[1] = deriv
                                (0 pos, 1 vel), ip[2] = dim; weight             (node_cost.cc:36-79)       */
  TOWR_COST_ENERGY      = 1, /* EnergyCost: weight, dt, p[0] = torque weight   (energy_cost.cc:36-152)    */
  TOWR_COST_ANG_MOMENTUM= 2, /* AngularMomentumCost: weight, dt                 (angular_momentum_cost.cc:39-208) */
  TOWR_COST_EE_BASE_POS = 3, /* EEBasePosCost: ee, weight, dt, p[0..2] = p_ref_B  (ee_base_pos_cost.cc:38-162) */
  TOWR_COST_BASE_HEIGHT = 4, /* BaseHeightCost of the fork: weight, dt (the reference's default 0.01 must be given),
                                p[0] = target base height above the mean stance-foot height
                                (base_height_cost.cc:36-142, added by hand in test/biped_example.cc:199-203)     */
  TOWR_COST_SOFT        = 5  /* SoftConstraint: 0.5 (g - b)^T (g - b) over constraint set ip[0] (any role), b = mid-point
                                of its bounds, given as side data TOWR_DATA_SOFT_BOUNDS (soft_constraint.cc:34-69);
                                W = identity as in the reference (no weight: `weight` is ignored)                 */
};
typedef struct {
  int32_t kind;    /* towr_cost_kind                                                             */
  int32_t ee;
  double  weight;
  double  dt;
  double  p[4];
  int32_t ip[4];
} towr_cost_t;

/* ---- initial guess (NlpFormulation::MakeBaseVariables etc., nlp_formulation.cc:121-346) ---- */
enum towr_init_mode {
  TOWR_INIT_FORMULATION = 0,  /* NlpFormulation::GetVariableSets initialisation                  */
  TOWR_INIT_PROCEDURAL  = 1   /* plain SetByLinearInterpolation of towr/test/procedural_example.cc:134-166 */
};

typedef struct {
  int32_t mode;                   /* towr_init_mode                                             */
  int32_t reserved;
  double  base_lin_p0[3], base_lin_v0[3], base_ang_p0[3], base_ang_v0[3];  /* initial_base_     */
  double  base_lin_p1[3], base_lin_v1[3], base_ang_p1[3], base_ang_v1[3];  /* final_base_       */
  double  ee_p0[TOWR_MAX_EE][3];  /* initial_ee_W_                                              */
  double  ee_p1[TOWR_MAX_EE][3];  /* procedural mode only: goal footholds                        */
} towr_init_t;

/* ---- full problem description --------------------------------------------------------------- */
typedef struct {
  int32_t        abi_version;               /* TOWR_GPU_ABI_VERSION                                */
  int32_t        angular_rep;               /* 0 = EulerZYX (Parameters::AngularRepresentation)    */
  towr_robot_t   robot;
  towr_terrain_t terrain;
  /* Parameters (parameters.cc:40-105)                                                            */
  double   total_time;                      /* Parameters::GetTotalTime()                          */
  double   duration_base_polynomial;        /* 0.1                                                  */
  int32_t  ee_polynomials_per_swing_phase;  /* 2                                                    */
  int32_t  force_polynomials_per_stance_phase;   /* 3                                               */
  int32_t  torque_polynomials_per_stance_phase;  /* 3                                               */
  int32_t  optimize_timings;                /* Parameters::IsOptimizeTimings()                     */
  double   bound_phase_duration[2];         /* (0.2, 1.0)                                          */
  int32_t  n_phases[TOWR_MAX_EE];
  int32_t  contact_at_start[TOWR_MAX_EE];   /* ee_in_contact_at_start_                              */
  double   phase_durations[TOWR_MAX_EE][TOWR_MAX_PHASES];  /* ee_phase_durations_                 */
  int32_t  n_varsets;                       /* order = ifopt AddVariableSet order                   */
  int32_t  n_constraints;                   /* order = ifopt AddConstraintSet order                 */
  towr_varset_t     varsets[TOWR_MAX_VARSETS];
  towr_constraint_t constraints[TOWR_MAX_CONSTRAINTS];
  towr_init_t       init;
  int32_t           n_costs;                /* order = ifopt AddCostSet order (cost terms)          */
  int32_t           reserved_costs;
  towr_cost_t       costs[TOWR_MAX_COSTS];
} towr_problem_desc_t;

typedef struct towr_gpu_handle_s* towr_gpu_handle;

/* ---- side data: what the POD description cannot hold (towr_gpu_create_ex) --------------------- */
enum towr_data_kind {
  TOWR_DATA_LINEAR_M    = 0, /* index = constraint (TOWR_C_LINEAR_EQ); count = rows * n_set; data = M row-major
                                (LinearEqualityConstraint::M_, linear_constraint.cc:35-45)                       */
  TOWR_DATA_SOFT_BOUNDS = 1, /* index = cost term (TOWR_COST_SOFT); count = 2 * rows of the wrapped set;
                                data = lower[0..rows-1], upper[0..rows-1] = the wrapped set's GetBounds(), from
                                which the engine forms b = (upper + lower) / 2 as SoftConstraint's ctor does  */
  TOWR_DATA_BOUNDS      = 2, /* OPTIONAL; index = constraint; what towr_gpu_constraint_bounds needs beyond the POD:
                                TOWR_C_EE_LINEAR: count = 1, the tolerance (ee_linear_constraint.cc:32-35);
                                TOWR_C_LINEAR_EQ: count = rows, the offset v (linear_constraint.cc:53-64);
                                TOWR_C_RANGE_OF_MOTION: count = 1..3, Parameters::rom_swing_relax_dims_ as doubles
                                (0, 1 or 2; nlp_formulation.cc:433-435); absent = no relaxation.
                                A handle created without them evaluates as ever; only the bounds calls then fail
                                (TOWR_ERR_INVALID) when it holds an EELinear or LinearEquality set                 */
  TOWR_DATA_VAR_BOUNDS  = 3  /* OPTIONAL; index = variable set (AddVariableSet order, a node set); count = 5 * records;
                                data = records (node_id, deriv, dim, lower, upper), each one call of
                                NodesVariables::AddBound(NodeValueInfo(node, deriv, dim), lower, upper)
                                (nodes_variables.cc:234-241; AddBounds / AddStartBound / AddFinalBound reduce to it),
                                applied in order: what the driver bounds on the variables (nlp_formulation.cc:121-346).
                                A record naming a value that is not optimised (deriv 2, a swing node of a force set,
                                a swing z velocity) is a no-op, as in the reference. A set without an entry is
                                unbounded (towr_gpu_variable_bounds)                                                */
};
typedef struct {
  int32_t       kind;    /* towr_data_kind                                                          */
  int32_t       index;   /* constraint, cost or variable-set index in the description               */
  int64_t       count;   /* doubles at `data`                                                       */
  const double* data;    /* host memory, copied at creation                                         */
} towr_data_t;

/* ---- lifecycle ------------------------------------------------------------------------------- */
/* Builds the layout (variable maps, time grids, CSR pattern, per-item slot tables) on the host and
 * uploads it to `device`. device < 0 creates a layout-only handle (sizes, structure, x0; every
 * evaluation entry point then returns TOWR_ERR_NO_DEVICE) — used by host-side structure checks. Replaces NlpFormulation::GetVariableSets/GetConstraints + ifopt
 * Problem::AddVariableSet/AddConstraintSet (nlp_formulation.cc:76-378, hopper_example.cc:154-161). */
int towr_gpu_create(const towr_problem_desc_t* desc, int device, towr_gpu_handle* out);
/* Same, with side data (LinearEqualityConstraint matrices, SoftConstraint bounds); every
 * TOWR_C_LINEAR_EQ set and TOWR_COST_SOFT term needs its entry (else TOWR_ERR_INVALID).            */
int towr_gpu_create_ex(const towr_problem_desc_t* desc, int32_t n_data, const towr_data_t* data, int device,
                       towr_gpu_handle* out);
int towr_gpu_destroy(towr_gpu_handle h);
const char* towr_gpu_last_error(towr_gpu_handle h);   /* h may be NULL: last global error         */
int towr_gpu_abi_version(void);

/* n = ifopt Problem::GetNumberOfOptimizationVariables, m = GetNumberOfConstraints,
 * nnz = nonzeros of GetJacobianOfConstraints (what IpoptAdapter::get_nlp_info reports).          */
int towr_gpu_sizes(towr_gpu_handle h, int32_t* n, int32_t* m, int64_t* nnz);

/* Jacobian structure, 0-based (IpoptAdapter::eval_jac_g with values == NULL; C_STYLE indexing). */
int towr_gpu_jac_structure(towr_gpu_handle h, int32_t* iRow, int32_t* jCol);
/* Same pattern as CSR: row_ptr[m+1], col[nnz].                                                   */
int towr_gpu_jac_csr(towr_gpu_handle h, int64_t* row_ptr, int32_t* col);

/* Starting point x0 = ifopt Problem::GetVariableValues() after NlpFormulation initialisation.    */
int towr_gpu_initial_x(towr_gpu_handle h, double* x0);

/* x0 of another instance that shares this layout (same robot, gait, horizon, constraint list):
 * only the start/goal states and the terrain differ (BASELINE config 5's randomised batch).      */
int towr_gpu_initial_x_for(towr_gpu_handle h, const towr_init_t* init, const towr_terrain_t* terrain, double* x0);
/* Column range of variable set i (AddVariableSet order): kind, ee, first column, size.          */
int towr_gpu_varset_info(towr_gpu_handle h, int32_t i, int32_t* kind, int32_t* ee, int32_t* col0, int32_t* n);

/* Row range of constraint set i (AddConstraintSet order): kind, ee, first row, rows. The hard sets tile [0, m) in
 * order; a TOWR_ROLE_SOFT set is not part of g and reports rows = 0.                              */
int towr_gpu_constraint_info(towr_gpu_handle h, int32_t i, int32_t* kind, int32_t* ee, int32_t* row0, int32_t* rows);
/* The constraint bounds in ifopt row order, lower[m] and upper[m]: every set's GetBounds() with the reference's
 * arithmetic and literals (what IpoptAdapter::get_bounds_info reports for g). Unbounded sides are ifopt's
 * +-1.0e20, not IEEE infinity. Only a node-based TorqueConstraint's third row, (-L, L) with L = k mu (f . n)
 * (torque_constraint.cc:103-127), depends on x and the terrain: towr_gpu_constraint_bounds uses the description's
 * x0 and terrain; _for those of another instance sharing the layout (as towr_gpu_initial_x_for) and differs on
 * those rows only. TOWR_ERR_INVALID (the message names the set) when an EELinear or LinearEquality set's
 * TOWR_DATA_BOUNDS entry was not given at creation. Host calls; they work on layout-only handles.   */
int towr_gpu_constraint_bounds(towr_gpu_handle h, double* lower /* m */, double* upper /* m */);
int towr_gpu_constraint_bounds_for(towr_gpu_handle h, const towr_init_t* init, const towr_terrain_t* terrain,
                                   double* lower, double* upper);
/* The variable bounds in ifopt column order, lower[n] and upper[n] (what IpoptAdapter::get_bounds_info reports for
 * x): every node set starts as ifopt's NoBound (-1.0e20, +1.0e20) and takes its TOWR_DATA_VAR_BOUNDS records in
 * order, later ones overwriting earlier ones; a record bounds the one column its node value maps to (two stance
 * nodes that share a variable share the bound). Every variable of a schedule set gets bound_phase_duration
 * (phase_durations.cc:51,103-110). Unbounded sides are +-1.0e20, never IEEE infinity. towr_gpu_variable_bounds
 * answers for the entries given at creation; _with rebuilds the bounds on this layout from the TOWR_DATA_VAR_BOUNDS
 * entries of `data` instead (another instance of the randomised batch, whose start and goal differ) and changes
 * nothing in the handle. Creation and _with refuse (TOWR_ERR_INVALID, the message names the variable set) a count
 * that is no multiple of 5, a non-integral or out-of-range node, deriv (0..2) or dim (0..2), a NaN, lower > upper,
 * and an index that is not a node set. Host calls; they work on layout-only handles.                           */
int towr_gpu_variable_bounds(towr_gpu_handle h, double* lower /* n */, double* upper /* n */);
int towr_gpu_variable_bounds_with(towr_gpu_handle h, int32_t n_data, const towr_data_t* data,
                                  double* lower, double* upper);

/* ---- single-problem host callbacks (what IpoptAdapter calls) -------------------------------- */
/* g = ifopt Problem::EvalConstraints(x)          (IpoptAdapter::eval_g)                         */
int towr_gpu_eval_g(towr_gpu_handle h, const double* x, double* g);
/* values = ifopt Problem::EvalNonzerosOfJacobian(x)  (IpoptAdapter::eval_jac_g, values != NULL) */
int towr_gpu_eval_jac_values(towr_gpu_handle h, const double* x, double* values);
/* both at once (one fused launch)                                                                */
int towr_gpu_eval_g_jac(towr_gpu_handle h, const double* x, double* g, double* values);
/* IPOPT's callback pair without a second evaluation: eval_g_keep_jac evaluates g and the Jacobian at x
 * into the handle's device staging and returns g; the values stay on the device with a copy of x.
 * eval_jac_values_kept(x) copies them into `values` (a DMA in place when `values` is registered) when x
 * is bit-identical to the kept x, else it evaluates the values as towr_gpu_eval_jac_values does. Any
 * other host-pointer evaluation on the handle drops the kept values. (ifopt IpoptAdapter::eval_g /
 * eval_jac_g, hopper_example.cc:175-180)                                                           */
int towr_gpu_eval_g_keep_jac(towr_gpu_handle h, const double* x, double* g);
int towr_gpu_eval_jac_values_kept(towr_gpu_handle h, const double* x, double* values);
/* Objective (IpoptAdapter::eval_f = Problem::EvaluateCostFunction, the sum of every cost term's
 * GetCost) and its dense gradient (eval_grad_f = Problem::EvaluateCostFunctionGradient). A problem
 * without cost terms has f = 0 and a zero gradient.                                               */
int towr_gpu_eval_f(towr_gpu_handle h, const double* x, double* f);
int towr_gpu_eval_grad_f(towr_gpu_handle h, const double* x, double* grad);
/* Batched objective on the device: F[b], GRAD[b*ldgrad + j]; stream as for eval_batch_device.    */
int towr_gpu_eval_cost_batch_device(towr_gpu_handle h, int32_t B, const double* X, int64_t ldx,
                                    double* F, double* GRAD, int64_t ldgrad, void* stream);
/* The objective kernel's blocks are persistent: a launch has min(B, grid) blocks and block k takes problems k,
 * k + grid, k + 2 grid, ... The automatic grid is what the device holds at once (blocks per CU x CUs, one value
 * for the f-only kernel and one for the gradient kernel). towr_gpu_set_cost_grid replaces it on this handle for
 * every objective launch (f only and gradient alike): blocks >= 1 blocks, 0 = the automatic grid again, negative =
 * TOWR_ERR_INVALID. The kernel has no grid-wide wait (a block never waits for another), so any positive value is
 * safe; the results do not depend on it, bit for bit. A SoftConstraint child's launches are not affected. It is a
 * test and experiment knob, like towr_gpu_set_products_chunk, and needs no device (layout-only handles accept it).
 * towr_gpu_cost_grid returns the grid in effect (>= 1) for the f-only (grad = 0) or the gradient (grad != 0)
 * launch, the automatic one while no override is set (1 on a layout-only handle); TOWR_ERR_INVALID (negative) for
 * a NULL handle.                                                                                                 */
int towr_gpu_set_cost_grid(towr_gpu_handle h, int32_t blocks);
int towr_gpu_cost_grid(towr_gpu_handle h, int32_t grad);

/* ---- trajectory export: SaveTrajectoryToCSV (towr/src/utils/save_data.cpp:9-130) ------------ */
/* Samples at t = 0, dt, 2dt, ... (accumulated) while t <= T + 1e-9, T = the base-linear spline's total
 * time. Row layout, n_cols = 19 + 25 * n_ee doubles:
 *   t | base-lin pos vel acc | base-ang pos vel acc (the raw angular spline: Euler angles or rotation
 *   vector and its derivatives) | per ee: motion pos vel acc | ee-ang pos vel acc | force | torque |
 *   is_contact (1.0 / 0.0)                                                                        */
int towr_gpu_trajectory_size(towr_gpu_handle h, double dt, int32_t* n_samples, int32_t* n_cols);
/* one problem, host buffers: out = n_samples x n_cols row-major                                   */
int towr_gpu_sample_trajectory(towr_gpu_handle h, const double* x, double dt, double* out);
/* B problems on the device: OUT[b * ldo + k * n_cols + c], ldo >= n_samples * n_cols              */
int towr_gpu_sample_trajectory_batch_device(towr_gpu_handle h, int32_t B, const double* X, int64_t ldx, double dt,
                                            double* OUT, int64_t ldo, void* stream);

/* ---- batched evaluation over independent problems that share the layout ---------------------- */
/* Per-problem terrain parameters (the only per-instance input to g/J besides x). `terrains` is a
 * host array of B entries of the description terrain's curvature class (Gap or not; see
 * towr_gpu_pattern_outside for what curved terrain does to the pattern).
 * Once set, every BATCH entry point (eval_batch, eval_batch_device[_kernel], eval_cost_batch_device)
 * uses terrain b for problem b and requires exactly B problems (else TOWR_ERR_INVALID); B = 0 clears
 * the set. The single-problem entry points (eval_g, eval_jac_values, eval_g_jac, eval_f,
 * eval_grad_f, sample_trajectory*) always use the description's terrain.                         */
int towr_gpu_set_batch_terrain(towr_gpu_handle h, int32_t B, const towr_terrain_t* terrains);

/* Frozen-pattern check (curved terrain). On Gap terrain ForceConstraintDiscretized and
 * TorqueConstraintDiscretized add a row's motion block only where its scale is non-zero
 * (force_constraint_discretized.cc:58, torque_constraint_discretized.cc:57), so the reference's
 * Jacobian pattern moves with x; IPOPT's structure, and this engine's CSR, are fixed at x0 (the
 * description's). These return how many entries the reference's Jacobian at x holds OUTSIDE that
 * frozen pattern (0 on terrains without curvature): entries the frozen structure cannot deliver. The
 * values on the frozen pattern are always the reference's, or 0.0 where the reference has no entry.
 * Both are HOST passes, not device kernels: the predicate is a floating-point tie (is a scale exactly
 * 0.0?), so it is evaluated with the reference's own host operations (std::pow, no contraction). Both are
 * synchronous. The batch form ("_device": X lives in HBM) copies X to the host on `stream`, waits for
 * it, evaluates the B problems on up to 16 host threads with the batch terrains like eval_batch_device,
 * and writes counts[B] in host memory (bench.py `pattern_watch` times it on a 4096-problem Gap batch).
 * Layout-only handles answer the single form. */
int towr_gpu_pattern_outside(towr_gpu_handle h, const double* x, int64_t* count);
int towr_gpu_pattern_outside_batch_device(towr_gpu_handle h, int32_t B, const double* X, int64_t ldx,
                                          int32_t* counts, void* stream);

/* Device-resident batch: X[b*ldx + j], G[b*ldg + i], V[b*ldv + k] are DEVICE pointers (HBM);
 * `stream` is the hipStream_t to launch on (NULL = HIP's default stream, as in the HIP API).
 * want_g / want_jac select outputs.
 * Asynchronous with respect to the host. Streams: some layouts evaluate through scratch owned by
 * the handle (the per-instant records of the phase-duration-optimisation kernels, the SoftConstraint
 * child's g / values). A call issued on a different stream than the handle's previous call waits
 * (on the GPU, through an event) for that call's work before it touches the scratch, so calls on one
 * handle never race but serialise across streams; use one handle per stream to overlap them.     */
int towr_gpu_eval_batch_device(towr_gpu_handle h, int32_t B,
                               const double* X, int64_t ldx,
                               double* G, int64_t ldg,
                               double* V, int64_t ldv,
                               int32_t want_g, int32_t want_jac, void* stream);

/* Host batch (H2D of X, D2H of G and V; contiguous lds = n, m, nnz). Outputs move in chunks: the
 * kernels of chunk i overlap the PCIe transfer of chunk i - 1. Arrays inside memory registered with
 * towr_gpu_register_host are transferred in place; others go through the handle's pinned staging.  */
int towr_gpu_eval_batch(towr_gpu_handle h, int32_t B, const double* X, double* G, double* V);

/* Page-locks caller memory [ptr, ptr + bytes) (hipHostRegister) for this handle until
 * towr_gpu_unregister_host or towr_gpu_destroy. Every host-pointer entry point whose x / g / values
 * (or X / G / V) array lies inside a registered range DMAs straight to / from it, without the
 * staging copy: an IPOPT driver registers its x, g and values arrays once (they are reused by every
 * IpoptAdapter callback, hopper_example.cc:175-180). Ranges must not overlap; the memory must stay
 * allocated while registered.                                                                    */
int towr_gpu_register_host(towr_gpu_handle h, void* ptr, int64_t bytes);
int towr_gpu_unregister_host(towr_gpu_handle h, void* ptr);

/* ---- consuming a batch on the device: per-problem products with the evaluated Jacobians ---------- */
/* The pattern by column (the transpose view of towr_gpu_jac_csr): col_ptr[n+1], row[nnz], csr_index[nnz]. The
 * entries of column j are q in [col_ptr[j], col_ptr[j+1]); rows ascend strictly within a column; csr_index[q] is
 * the entry's position in the CSR value array. Works on layout-only handles.                       */
int towr_gpu_jac_csc(towr_gpu_handle h, int64_t* col_ptr /* n+1 */, int32_t* row /* nnz */, int32_t* csr_index /* nnz */);

/* Y[b*ldy + i] = sum_{k in row i} V[b*ldv + k] * P[b*ldp + col[k]]           (J_b p_b, m outputs per problem)
 * Z[b*ldz + j] (+)= sum_{k in column j} V[b*ldv + k] * LAM[b*ldl + row[k]]   (J_b^T lam_b, n outputs per problem)
 * accumulate = 0: Z is overwritten; 1: the sum is added to what Z holds (grad f + J^T lam on top of
 * towr_gpu_eval_cost_batch_device's GRAD). All pointers are DEVICE pointers; V holds CSR values as
 * towr_gpu_eval_batch_device writes them; `stream` as there. ldv >= nnz, ldp, ldz >= n, ldl, ldy >= m.
 * Bit-reproducible: Y[b] is a function of (V_b, P_b) and Z[b] of (V_b, LAM_b, and the old Z_b when accumulating)
 * alone — the same bits for any B, any position in the batch, any stream, run to run: every output is one fixed
 * tree of IEEE additions over exactly its own entries (no atomics, no entry skipped: a NaN or Inf term makes
 * exactly its outputs non-finite). Rows / columns without entries give 0.0; an empty column under accumulate
 * leaves Z_j untouched. V[b*ldv + nnz ..] is never read, Y[b*ldy + m ..] and Z[b*ldz + n ..] never written. The
 * calls use no handle scratch (they neither wait for other calls on the handle nor drop the kept Jacobian). The
 * first product call on a handle uploads the product tables (synchronously); later ones are asynchronous.   */
int towr_gpu_jac_vec_batch_device(towr_gpu_handle h, int32_t B, const double* V, int64_t ldv,
                                  const double* P, int64_t ldp, double* Y, int64_t ldy, void* stream);
int towr_gpu_jac_tvec_batch_device(towr_gpu_handle h, int32_t B, const double* V, int64_t ldv,
                                   const double* LAM, int64_t ldl, double* Z, int64_t ldz,
                                   int32_t accumulate, void* stream);

/* Fused, chunked evaluate-and-apply: for each problem, evaluate J_b at X_b (and g_b when G != NULL), then
 * Z_b (+)= J_b^T LAM_b when LAM != NULL (Z required) and Y_b = J_b P_b when P != NULL (Y required). The values live
 * only in scratch owned by the handle, `chunk` problems at a time (towr_gpu_set_products_chunk; 0 = automatic:
 * equal parts of at most 2 GiB of values each — larger chunks measured faster), so the footprint
 * does not grow with B. Bit-identical to
 * towr_gpu_eval_batch_device followed by the two product calls, whatever the chunk. Batch terrains as
 * towr_gpu_eval_batch_device (exactly B entries). The scratch follows the cross-stream rule stated there; the
 * kept Jacobian of towr_gpu_eval_g_keep_jac is not touched.                                                    */
int towr_gpu_eval_products_batch_device(towr_gpu_handle h, int32_t B, const double* X, int64_t ldx,
                                        double* G, int64_t ldg,
                                        const double* LAM, int64_t ldl, double* Z, int64_t ldz, int32_t accumulate,
                                        const double* P, int64_t ldp, double* Y, int64_t ldy, void* stream);
int towr_gpu_set_products_chunk(towr_gpu_handle h, int32_t problems);   /* 0 = automatic */

/* ---- feasibility of a batch on the device: violation summaries and augmented-Lagrangian multipliers ---------- */
/* Per problem b and row i, with g = G[b*ldg + i], l = GL[b*ldb + i], u = GU[b*ldb + i] (DEVICE pointers; GL = GU = NULL:
 * the handle's description bounds, uploaded synchronously by the first such call; ldb = 0: one bounds row shared by
 * all problems; else ldb >= m):
 *   a side counts only if l > -1e19, respectively u < 1e19 (IPOPT's infinity threshold; IEEE infinities are safe);
 *   violation  v_i = max(l - g, g - u, 0) over the sides that count; a NaN g gives a NaN v_i;
 *   multiplier (LAMP != NULL, rho > 0; LAM NULL = zero multipliers): t = g + lam_i / rho, c = t clamped to the sides
 *              that count, r_i = t - c, LAMP[b*ldlp + i] = rho r_i (Rockafellar's augmented Lagrangian for
 *              l <= g <= u: grad_x = grad f + J^T lam+).
 * SUM[b*lds + ...] holds 4 + n_constraints doubles (lds >= that): [0] max v_i; [1] sum v_i; [2] the lowest row
 * attaining [0] as a double (-1.0 when [0] == 0; the first NaN row when a row is NaN); [3] phi = sum (0.5 rho r_i^2
 * - 0.5 lam_i^2 / rho), 0.0 without LAMP; [4 + s] max v_i over constraint set s in description order (soft sets 0.0).
 * A NaN row makes [0], [1] and its own set's entry NaN and leaves the other sets' entries untouched.
 * One block per problem; every sum is one fixed tree (lane-strided partials, a shuffle tree, a fixed-order combine
 * across waves; no floating-point atomics), so problem b's outputs are a function of its own operands alone: the
 * same bits for any B, any position, any stream, run to run. Nothing beyond m (G, LAM, LAMP) or 4 + n_constraints
 * (SUM) is read or written. No handle scratch is used and the kept Jacobian is not dropped. TOWR_ERR_INVALID before
 * anything runs for: NULL G or SUM, lds < 4 + n_constraints, ldg / ldl / ldlp < m, 0 < ldb < m, rho <= 0 (or NaN)
 * with LAMP, only one of GL / GU.                                                                                */
int towr_gpu_residual_batch_device(towr_gpu_handle h, int32_t B, const double* G, int64_t ldg,
                                   const double* GL, const double* GU, int64_t ldb,
                                   const double* LAM, int64_t ldl, double rho,
                                   double* LAMP, int64_t ldlp, double* SUM, int64_t lds, void* stream);

/* Fused, chunked merit-and-gradient: per chunk of problems (towr_gpu_set_products_chunk, automatic as for
 * towr_gpu_eval_products_batch_device) evaluate g and J at X into handle scratch, run the residual kernel, then
 * Z_b (+)= J_b^T lam+_b. G and LAMP are optional outputs (NULL: they live in handle scratch only); SUM and Z are
 * required, rho > 0. Bit-identical to towr_gpu_eval_batch_device, towr_gpu_residual_batch_device (with LAMP) and
 * towr_gpu_jac_tvec_batch_device in sequence, whatever the chunk. With accumulate = 1 on top of
 * towr_gpu_eval_cost_batch_device's GRAD, Z is the augmented Lagrangian's gradient and F + SUM[3] its value. Batch
 * terrains, the cross-stream scratch rule and the kept Jacobian as for towr_gpu_eval_products_batch_device.       */
int towr_gpu_eval_auglag_batch_device(towr_gpu_handle h, int32_t B, const double* X, int64_t ldx,
                                      const double* GL, const double* GU, int64_t ldb,
                                      const double* LAM, int64_t ldl, double rho,
                                      double* G, int64_t ldg, double* LAMP, int64_t ldlp,
                                      double* SUM, int64_t lds,
                                      double* Z, int64_t ldz, int32_t accumulate, void* stream);

/* ---- taking a step on the device: the projected step and its summary ------------------------------------------ */
/* Per problem b and column j, with x = X[b*ldx + j], d = D[b*ldd + j], l = XL[b*ldb + j], u = XU[b*ldb + j] and the
 * step length a = ALPHA[b] (ALPHA NULL: the scalar alpha). All pointers are DEVICE pointers. XL = XU = NULL: the
 * handle's description bounds (towr_gpu_variable_bounds), uploaded synchronously by the first such call; ldb = 0:
 * one bounds row shared by all problems; else ldb >= n (per-problem rows, towr_gpu_variable_bounds_with):
 *   a side counts only if l > -1e19, respectively u < 1e19 (as towr_gpu_residual_batch_device);
 *   t  = x - a d, a rounded product then a rounded subtraction (never a fused multiply-add);
 *   xp = t clamped to the sides that count, XP[b*ldxp + j] (XP NULL: summary only); a fixed variable (l == u) lands
 *        exactly on l;
 *   s  = xp - x, the projected step.
 * SUM[b*lds + ...] holds 5 + n_varsets doubles (lds >= that): [0] max |s_j| (with a = 1 and d = grad L the
 * projected-gradient stationarity measure); [1] sum s_j^2; [2] sum d_j s_j (the slope of an Armijo test); [3] the
 * number of columns whose xp lies on a side that counts, as a double; [4] max(l - x, x - u, 0) over the sides that
 * count (how far X itself is outside its box); [5 + s] max |s_j| over variable set s (AddVariableSet order).
 * A NaN x, d or a makes [0], [1], [2] and its own set's entry NaN and leaves the other sets' entries untouched.
 * One block per problem; the sums are one fixed tree each (lane-strided partials, a shuffle tree, the waves in
 * order; no floating-point atomics) and the maxima are integer maxima of the bit patterns, so problem b's outputs
 * are a function of its own operands alone: the same bits for any B, any position, any stream, run to run. Nothing
 * beyond n (X, D, XP, XL, XU) or 5 + n_varsets (SUM) is read or written. No handle scratch is used and the kept
 * Jacobian is not dropped. TOWR_ERR_INVALID before anything runs for: NULL X, D or SUM, lds < 5 + n_varsets,
 * ldx / ldd / ldxp < n, 0 < ldb < n, only one of XL / XU, a NaN scalar alpha with ALPHA NULL.                     */
int towr_gpu_step_batch_device(towr_gpu_handle h, int32_t B, const double* X, int64_t ldx,
                               const double* D, int64_t ldd, const double* ALPHA, double alpha,
                               const double* XL, const double* XU, int64_t ldb,
                               double* XP, int64_t ldxp, double* SUM, int64_t lds, void* stream);

/* One call per iteration of a projected first-order method on the augmented Lagrangian: on `stream`,
 *   1. towr_gpu_eval_cost_batch_device with GRAD into handle scratch (F NULL: f into handle scratch as well);
 *   2. towr_gpu_eval_auglag_batch_device with accumulate = 1 onto that gradient (G, LAMP optional, RSUM its SUM);
 *   3. towr_gpu_step_batch_device with D = that gradient (XP and SSUM required).
 * Bit-identical to the three calls in sequence, whatever the products chunk. It exists for the footprint (the
 * gradient, like the values, g and lam+, never leaves handle scratch) and the single call, not for speed: it
 * launches what the three calls launch. Batch terrains, the cross-stream scratch rule and the kept Jacobian as for
 * towr_gpu_eval_products_batch_device. Argument checks as the three calls'.                                      */
int towr_gpu_auglag_step_batch_device(towr_gpu_handle h, int32_t B, const double* X, int64_t ldx,
                                      const double* GL, const double* GU, int64_t ldgb,
                                      const double* LAM, int64_t ldl, double rho,
                                      const double* ALPHA, double alpha,
                                      const double* XL, const double* XU, int64_t ldxb,
                                      double* F, double* G, int64_t ldg, double* LAMP, int64_t ldlp,
                                      double* RSUM, int64_t ldrs,
                                      double* XP, int64_t ldxp, double* SSUM, int64_t ldss, void* stream);

/* ---- a quasi-Newton direction on the device: the L-BFGS history and the two-loop recursion --------------------- */
/* The history is caller-owned DEVICE memory for B problems and `mem` pairs, 1 <= mem <= TOWR_LBFGS_MAX_MEM: pair k
 * of problem b starts at HS + (b*mem + k)*ldh (s) and HY + (b*mem + k)*ldh (y), ldh >= n; HMETA is int32_t[2*B],
 * {count, next} per problem: the number of pairs held (0..mem) and the slot the next accepted pair goes to
 * (0..mem-1). A zeroed HMETA is an empty history — also the way to reset it when lam or rho change (the pairs
 * describe another function then). A problem whose count or next is out of range is treated as empty ({0, 0}); the
 * kernels never index from such a value. All pointers are DEVICE pointers; `stream` as everywhere else.            */
#define TOWR_LBFGS_MAX_MEM 16

/* Per problem: s_j = XN_j - X_j, y_j = GRN_j - GR_j (one rounded subtraction each); sy = sum s y, ss = sum s s,
 * yy = sum y y. The pair is accepted iff sy > curv_eps * yy (L-BFGS-B's curvature test: gamma = sy / yy stays above
 * curv_eps; a NaN anywhere makes the comparison false). Accepted: s and y are written to slot `next`, then
 * next = (next + 1) % mem and count = min(count + 1, mem). Rejected: not one byte of HS, HY or HMETA of that problem
 * changes. SUM[b*lds + ..] holds 6 doubles (lds >= 6): [0] sy; [1] ss; [2] yy; [3] 1.0 accepted / 0.0 rejected;
 * [4] count after the call; [5] the slot written (-1.0 when rejected). Nothing beyond n is read or written in any
 * row, nothing beyond 6 in SUM. The sums are one fixed tree each (as towr_gpu_step_batch_device) and the decision is
 * taken on them: problem b's outputs are a function of its own operands alone. No handle scratch is used and the
 * kept Jacobian is not dropped. TOWR_ERR_INVALID before anything runs for: a NULL pointer, mem outside
 * 1..TOWR_LBFGS_MAX_MEM, ldx / ldxn / ldgr / ldgrn / ldh < n, lds < 6, curv_eps negative or NaN.
 * TOWR_ERR_UNSUPPORTED at the call when n is too large for the kernels' LDS (16 n bytes of 60 KiB).                */
int towr_gpu_lbfgs_update_batch_device(towr_gpu_handle h, int32_t B, int32_t mem,
                                       const double* X, int64_t ldx, const double* XN, int64_t ldxn,
                                       const double* GR, int64_t ldgr, const double* GRN, int64_t ldgrn,
                                       double curv_eps, double* HS, double* HY, int64_t ldh, int32_t* HMETA,
                                       double* SUM, int64_t lds, void* stream);

/* The two-loop recursion on the free columns: D_b ~ H_b g_b, g = GR[b*ldgr + ..]. The bounds as for
 * towr_gpu_step_batch_device (XL = XU = NULL: the handle's; ldb = 0: one shared row; a side counts only within
 * +-1e19); X = NULL: every column is free and the bounds are not read. Column j is held iff its lower side counts,
 * x_j <= l_j and g_j > 0, or its upper side counts, x_j >= u_j and g_j < 0, or both sides count and l_j == u_j (exact
 * comparisons: the step kernel lands a clamped variable exactly on its bound). Every other column is free (a NaN g_j
 * is free). Held entries count as zero in every sum and are never updated:
 *   q = g; for i = 1..count (newest to oldest), slot = (next - i) mod mem: c_i = sum_free s y; the pair is used iff
 *   c_i > 0 (a NaN in a pair makes it unused); if used a_i = (sum_free s q) / c_i, q -= a_i y;
 *   gamma = c / sum_free y y of the newest used pair (1 when none is used); r = gamma q;
 *   for the used pairs, oldest to newest: beta = (sum_free y r) / c_i, r += (a_i - beta) s;
 *   D_j = r_j on free columns, D_j = g_j bit for bit on held ones (the projected step keeps them on their bound).
 * With count == 0, D equals GR bit for bit. A NaN g_j on a free column makes the free columns of that problem's D
 * NaN (when a pair is used) and touches no other problem. SUM[b*lds + ..] holds 5 doubles (lds >= 5): [0] pairs
 * used; [1] gamma; [2] sum_j g_j D_j over all columns (the slope: backtrack through ALPHA or fall back to D = GR
 * when it is not positive); [3] the number of held columns; [4] sum_free g^2. Fixed-tree sums, the used decisions on
 * them: problem b's outputs are a function of its own operands alone. Nothing beyond n (rows) or 5 (SUM) is read
 * or written. No handle scratch, the kept Jacobian is not dropped. TOWR_ERR_INVALID before anything runs for: NULL
 * GR, D, HS, HY, HMETA or SUM, mem outside 1..TOWR_LBFGS_MAX_MEM, ldx / ldgr / ldd / ldh < n, lds < 5, only one
 * of XL / XU, 0 < ldb < n. TOWR_ERR_UNSUPPORTED as for the update.                                                 */
int towr_gpu_lbfgs_direction_batch_device(towr_gpu_handle h, int32_t B, int32_t mem,
                                          const double* X, int64_t ldx, const double* GR, int64_t ldgr,
                                          const double* XL, const double* XU, int64_t ldb,
                                          const double* HS, const double* HY, int64_t ldh, const int32_t* HMETA,
                                          double* D, int64_t ldd, double* SUM, int64_t lds, void* stream);

/* One call per inner iteration of a bound-projected L-BFGS method on the augmented Lagrangian: on `stream`,
 *   1. towr_gpu_eval_cost_batch_device with GRAD = GR (F NULL: f into handle scratch), then
 *      towr_gpu_eval_auglag_batch_device with accumulate = 1 onto GR (g and lam+ in handle scratch, RSUM its SUM).
 *      GR (required, ldgr >= n) must persist: it is the next call's GRPREV;
 *   2. towr_gpu_lbfgs_update_batch_device with (X, XN) = (XPREV, X) and (GR, GRN) = (GRPREV, GR), USUM its SUM, when
 *      XPREV and GRPREV are given; both NULL (the first iteration): no update, USUM is not written;
 *   3. towr_gpu_lbfgs_direction_batch_device at (X, GR) into handle scratch, DSUM its SUM;
 *   4. towr_gpu_step_batch_device with that direction (XP and SSUM required).
 * Bit-identical to those calls in sequence, whatever the products chunk. Batch terrains, the cross-stream scratch
 * rule and the kept Jacobian as for towr_gpu_eval_products_batch_device. Argument checks as those calls', and only
 * one of XPREV / GRPREV is TOWR_ERR_INVALID. Three X buffers and two GR buffers rotate in the caller's loop
 * (INTEGRATION.md).                                                                                              */
int towr_gpu_auglag_lbfgs_step_batch_device(towr_gpu_handle h, int32_t B, int32_t mem,
                                            const double* X, int64_t ldx,
                                            const double* XPREV, int64_t ldxprev,
                                            const double* GRPREV, int64_t ldgrprev,
                                            const double* GL, const double* GU, int64_t ldgb,
                                            const double* LAM, int64_t ldl, double rho,
                                            const double* ALPHA, double alpha,
                                            const double* XL, const double* XU, int64_t ldxb,
                                            double curv_eps, double* HS, double* HY, int64_t ldh, int32_t* HMETA,
                                            double* F, double* GR, int64_t ldgr, double* RSUM, int64_t ldrs,
                                            double* USUM, int64_t ldus, double* DSUM, int64_t ldds,
                                            double* XP, int64_t ldxp, double* SSUM, int64_t ldss, void* stream);

/* ---- a resident solve loop: line search, multiplier / penalty update and whole iterations on the stream -------- */
/* The parameters of the loop (host memory, read at the call). TOWR_ERR_INVALID before anything runs for a NaN or
 * out-of-range field: mem in 1..TOWR_LBFGS_MAX_MEM; max_inner >= 1 (trials per outer iteration before the outer
 * update is forced); max_outer >= 1; c1 and shrink in (0, 1); alpha0 >= alpha_min > 0; curv_eps >= 0; rho0 > 0,
 * rho_grow >= 1, rho_max >= rho0; eta0, eta_shrink in (0, 1], eta_star > 0 (the feasibility tolerance schedule);
 * omega0, omega_shrink in (0, 1], omega_star > 0 (the stationarity tolerance schedule).                          */
typedef struct {
  int32_t mem, max_inner, max_outer, reserved;
  double c1, shrink, alpha0, alpha_min, curv_eps;
  double rho0, rho_grow, rho_max;
  double eta0, eta_shrink, eta_star;
  double omega0, omega_shrink, omega_star;
} towr_alsolve_params_t;

/* The per-problem state: caller-owned DEVICE memory for B problems; the struct itself is host memory, read at the
 * call. Row b of a matrix starts at b*ld.
 *   X, GR, XC, GRC, D (ldx >= n): the base iterate, the augmented Lagrangian's gradient there, the candidate, the
 *     gradient at the candidate, the direction at the base;
 *   LAM, LAMP (ldl >= m): the multipliers, lam+ at the candidate;
 *   HS, HY, ldh, HMETA: the L-BFGS history, as above (`mem` pairs per problem);
 *   ALPHA, RHO, FC (B doubles each, contiguous): the next trial length, the penalty parameter, f at the candidate;
 *   SCAL (ldsc >= 8): [0] M0, the merit at the base; [1] pg at the base; [2] eta; [3] omega; [4] the max violation
 *     at the base; [5] f at the base; [6..7] 0;
 *   ISTATE (int32_t[4*B]): {phase, flags, inner, outer} per problem;
 *   RSUM (ldrs), SSUM (ldss), DSUM (ldds), USUM (ldus >= 6), LSUM (ldls >= 8): the summaries of the residual, step,
 *     direction and update stages (their widths as stated there) and of the line search.
 * Phases: 0 RESTART (the next evaluation defines the base), 1 SEARCH, 2 CONVERGED, 3 STALLED (the trial length fell
 * below alpha_min with an empty history), 4 MAXED (max_outer reached). Any other value counts as frozen, like 2..4;
 * the kernels never index from it. Flags (written by the line search): bit 0 a base was accepted in this iteration,
 * bit 1 the direction must be recomputed, bit 2 the history was reset.                                           */
typedef struct {
  double *X, *GR, *XC, *GRC, *D; int64_t ldx;
  double *LAM, *LAMP; int64_t ldl;
  double *HS, *HY; int64_t ldh; int32_t* HMETA;
  double *ALPHA, *RHO, *FC;
  double* SCAL; int64_t ldsc;
  int32_t* ISTATE;
  double* RSUM; int64_t ldrs;
  double* SSUM; int64_t ldss;
  double* DSUM; int64_t ldds;
  double* USUM; int64_t ldus;
  double* LSUM; int64_t ldls;
} towr_alsolve_state_t;
#define TOWR_AL_RESTART 0
#define TOWR_AL_SEARCH 1
#define TOWR_AL_CONVERGED 2
#define TOWR_AL_STALLED 3
#define TOWR_AL_MAXED 4

/* The line search: keeps or rejects the candidate XC of every problem, behind an evaluation that left FC, GRC and
 * RSUM ([0] max violation, [3] phi). MC = FC[b] + RSUM[b][3], one rounded addition. By the phase read at entry:
 *   frozen (>= 2 or invalid): flags = 0, LSUM[0] = 0; no other byte of the problem changes (LSUM[1..7] included).
 *   RESTART: X <- XC, GR <- GRC, SCAL[0] = MC, SCAL[4] = RSUM[b][0], SCAL[5] = FC[b], HMETA = {0, 0},
 *     ALPHA[b] = alpha0, phase = SEARCH, flags = 1|2|4, inner += 1, LSUM[0] = 1. No pair is offered.
 *   SEARCH: s = XC - X (one rounded subtraction per column), gs = sum_j GR_j s_j. Accepted iff gs <= 0 and
 *     MC <= M0 + c1*gs (a rounded product, a rounded addition; a NaN anywhere makes the test false).
 *     accepted: the pair (XC - X, GRC - GR) is offered exactly as towr_gpu_lbfgs_update_batch_device offers it (the
 *       same sums on the same tree, the same test sy > curv_eps*yy, the same slot rules: HS, HY and HMETA end up
 *       bit for bit as that call leaves them; its six summary values go to USUM); then the base is updated as in
 *       RESTART, except that HMETA keeps what the offer left; flags = 1|2, inner += 1, LSUM[0] = 2.
 *     rejected: a = ALPHA[b]*shrink. a >= alpha_min: ALPHA[b] = a, flags = 0, LSUM[0] = 3 (X, GR, D and the history
 *       untouched). Else, with a pair in the history: HMETA = {0, 0}, ALPHA[b] = alpha0, flags = 2|4, LSUM[0] = 4
 *       (the next direction is GR bit for bit). Else: phase = STALLED, ALPHA[b] = 0, flags = 0, LSUM[0] = 5.
 *       inner += 1 in each case. USUM is not written.
 * When a base was accepted, SCAL[1] = pg = max_j |clamp(x_j - g_j) - x_j| over the new base: the expression of
 * towr_gpu_step_batch_device with a = 1 (sides count within +-1e19), an integer maximum of the bit patterns, NaN on
 * top. XL, XU, ldb as there (NULL: the handle's; ldb = 0: one shared row).
 * LSUM[1..7] (every phase but frozen) = gs, MC, the M0 before, sy, yy, pair stored 1 / 0, pg (gs, sy and yy are 0
 * at a RESTART; pg is SCAL[1] after the call). Fixed-tree sums, decisions on broadcast scalars: problem b's outputs
 * are a function of its own operands alone. Nothing beyond n (rows), 8 (SCAL, LSUM), 6 (USUM) is read or written;
 * of RSUM only [0] and [3] are read. Fields used: X, GR, XC, GRC, ldx, HS, HY, ldh, HMETA, ALPHA, FC, SCAL, ISTATE,
 * RSUM, USUM, LSUM. No handle scratch; the kept Jacobian is not dropped. TOWR_ERR_INVALID before anything runs
 * for: NULL params or state, an invalid params field, a NULL used field, ldx / ldh < n, ldsc < 8, ldrs < 4,
 * ldus < 6, ldls < 8, only one of XL / XU, 0 < ldxb < n. TOWR_ERR_UNSUPPORTED as for the L-BFGS update.          */
int towr_gpu_linesearch_batch_device(towr_gpu_handle h, int32_t B, const towr_alsolve_params_t* params,
                                     const towr_alsolve_state_t* state, const double* XL, const double* XU,
                                     int64_t ldxb, void* stream);

/* The outer update. It acts on problem b only if phase == SEARCH, flag bit 0 is set and (pg <= omega or
 * inner >= max_inner), with pg = SCAL[1], omega = SCAL[3]; otherwise not one byte of the problem changes. With
 * viol = SCAL[4], eta = SCAL[2]:
 *   viol <= eta and viol <= eta_star and pg <= omega_star: phase = CONVERGED, ALPHA[b] = 0, flags = 0;
 *   else viol <= eta: LAM <- LAMP (m values), eta = max(eta*eta_shrink, eta_star),
 *     omega = max(omega*omega_shrink, omega_star) (t = the rounded product; t > star ? t : star);
 *   else (also a NaN viol): RHO[b] = min(RHO[b]*rho_grow, rho_max) (t < rho_max ? t : rho_max); LAM, eta and omega
 *     unchanged;
 *   in the two non-converged cases: outer += 1, inner = 0, HMETA = {0, 0}, ALPHA[b] = 0, flags = 0, phase = MAXED
 *     if outer >= max_outer, else RESTART. With ALPHA[b] = 0 the next step gives XC = X and the next evaluation
 *     defines M0 and GR for the new lam / rho.
 * Everything is a copy, one rounded product or a comparison. Fields used: LAM, LAMP, ldl, HMETA, ALPHA, RHO, SCAL,
 * ISTATE. TOWR_ERR_INVALID before anything runs for: NULL params or state, an invalid params field, a NULL used
 * field, ldl < m, ldsc < 8.                                                                                      */
int towr_gpu_auglag_outer_batch_device(towr_gpu_handle h, int32_t B, const towr_alsolve_params_t* params,
                                       const towr_alsolve_state_t* state, void* stream);

/* Starts a solve: ISTATE = {RESTART, 0, 0, 0}, HMETA = 0, RHO = rho0, ALPHA = 0, SCAL = {0, 0, eta0, omega0, 0, 0,
 * 0, 0}, XC = the caller's X clamped to the sides of (XL, XU) that count, D = 0 (the first step runs with
 * ALPHA = 0 and must not meet a NaN there). LAM holds the caller's starting multipliers and is not touched.
 * Fields used: X, XC, D, ldx, HMETA, ALPHA, RHO, SCAL, ISTATE. Checks as towr_gpu_alsolve_iterate_batch_device's. */
int towr_gpu_alsolve_init_batch_device(towr_gpu_handle h, int32_t B, const towr_alsolve_params_t* params,
                                       const towr_alsolve_state_t* state, const double* XL, const double* XU,
                                       int64_t ldxb, void* stream);

/* `iters` complete iterations on `stream`, with no host synchronisation. One iteration:
 *   1. towr_gpu_eval_cost_batch_device at XC, F = FC and GRAD = GRC;
 *   2. towr_gpu_eval_auglag_batch_device at XC with LAM and problem b's own rho = RHO[b], accumulated onto GRC; its
 *      LAMP and SUM are LAMP and RSUM (g stays in handle scratch);
 *   3. towr_gpu_linesearch_batch_device;
 *   4. towr_gpu_auglag_outer_batch_device;
 *   5. towr_gpu_lbfgs_direction_batch_device at (X, GR) into D, DSUM its SUM — only for the problems whose flag bit 1
 *      is set; the D and DSUM rows of the others are untouched (a rejected trial keeps its direction);
 *   6. towr_gpu_step_batch_device, XC = P(X - ALPHA D), SSUM its SUM.
 * Bit-identical to those calls in sequence (step 2 as B = 1 calls with the scalar rho = RHO[b] where the RHO differ),
 * whatever the products chunk. The batch is not compacted: a frozen problem is still evaluated in every iteration
 * (its ALPHA is 0, so XC = X), but its X, GR, LAM, RHO, SCAL, ISTATE and history never change again. Batch terrains,
 * the cross-stream scratch rule and the kept Jacobian as for towr_gpu_eval_products_batch_device. Every field of
 * `state` is used. TOWR_ERR_INVALID before anything runs for: iters < 0, what the two calls above refuse, a NULL
 * field, ldrs < 4 + n_constraints, ldss < 5 + n_varsets, ldds < 5, only one of GL / GU, 0 < ldgb < m, bounds the
 * description cannot give (GL NULL). TOWR_ERR_UNSUPPORTED as for the L-BFGS kernels.                             */
int towr_gpu_alsolve_iterate_batch_device(towr_gpu_handle h, int32_t B, int32_t iters,
                                          const towr_alsolve_params_t* params, const towr_alsolve_state_t* state,
                                          const double* GL, const double* GU, int64_t ldgb,
                                          const double* XL, const double* XU, int64_t ldxb, void* stream);

/* ---- a Gauss-Newton direction for the resident loop: truncated CG on rho J^T W J + mu I --------------------------- */
/* The CG parameters (host memory, read at the call): at most ncg steps, the damping mu >= 0 (it stands in for a cost
 * Hessian), the relative residual tolerance tol >= 0.                                                              */
typedef struct { int32_t ncg, reserved; double mu, tol; } towr_gn_params_t;

/* Per problem a whole CG solve of H d = g on the free columns, H = rho_b (J^T diag(w) J)_ff + mu I, on the CSR values V
 * (as towr_gpu_eval_batch_device writes them, ldv >= nnz) without forming H. w_i = 1.0 if LAMP[b][i] != 0.0 (lam+ of the
 * residual kernel: the row is active; a NaN counts as active), else 0.0. rho_b = RHO[b], or the scalar rho when RHO is
 * NULL. g = GR[b*ldgr + ..]. The held columns are exactly those of towr_gpu_lbfgs_direction_batch_device (the same
 * comparisons on X, g and the bounds; X = NULL: every column is free and the bounds are not read; XL = XU = NULL: the
 * handle's bounds; ldb = 0: one shared row). From d = 0, r = p = g on free columns (p = 0 on held ones),
 * rr = bb = sum_free g^2; bb == 0 ends at once (code 3); else for it < ncg:
 *   1. stop (code 1) if rr <= tol*tol*bb (the rounded products (tol*tol)*bb; a NaN rr goes on to step 5);
 *   2. t = w .* (J p) over all rows (the product w_i * (J p)_i: a NaN or infinity in an inactive row still gives NaN);
 *   3. Hp = rho_b * (J^T t) + mu * p on free columns (two rounded products, one rounded addition), 0 on held ones;
 *   4. pHp = sum_free p Hp;
 *   5. stop (code 2) unless pHp > 0 (a NaN anywhere — GR, V, rho_b — ends here);
 *   6. a = rr / pHp, d = d + a p, r = r - a Hp, rn = sum_free r r, p = r + (rn / rr) p, rr = rn; one step completed.
 * ncg steps completed: code 0. D_j = d_j on free columns and D_j = g_j bit for bit on held ones; when no step
 * completed D equals GR bit for bit. SUM[b*lds + ..] holds 6 doubles (lds >= 6): [0] steps completed; [1] bb; [2] the
 * final rr; [3] sum_j g_j D_j over all columns (the slope); [4] the number of held columns; [5] the stop code.
 * RUN = NULL: every problem; else problem b is skipped when RUN[b*run_stride] >= 2 (the frozen phases of
 * towr_alsolve_state_t's ISTATE with run_stride = 4): not one byte of its D or SUM row is touched.
 * J p and J^T t are the sums of towr_gpu_jac_vec_batch_device and towr_gpu_jac_tvec_batch_device on the same trees, the
 * dot products one fixed tree each, the stop decisions taken on them: problem b's outputs are a function of its own
 * operands alone (the same bits for any B, position, stream and run). Nothing beyond nnz (V), m (LAMP), n (X, GR, D, the
 * bounds) or 6 (SUM) is read or written in any row. D must not overlap any input. No handle scratch is used and the kept
 * Jacobian is not dropped. All pointers are DEVICE pointers. TOWR_ERR_INVALID before anything runs for: NULL gn, V, LAMP,
 * GR, D or SUM, ncg < 1, mu or tol negative or NaN, rho <= 0 or NaN with RHO == NULL, ldv < nnz, ldlp < m,
 * ldx (with X) / ldgr / ldd < n, lds < 6, only one of XL / XU, 0 < ldb < n. TOWR_ERR_UNSUPPORTED at the call when the
 * kernel's LDS (8 (3 n + m) + 20 KiB + m bytes) does not fit the workgroup's 160 KiB.                                 */
int towr_gpu_gn_direction_batch_device(towr_gpu_handle h, int32_t B, const towr_gn_params_t* gn,
                                       const double* V, int64_t ldv, const double* LAMP, int64_t ldlp,
                                       const double* RHO, double rho, const double* X, int64_t ldx,
                                       const double* GR, int64_t ldgr, const double* XL, const double* XU, int64_t ldb,
                                       const int32_t* RUN, int32_t run_stride, double* D, int64_t ldd,
                                       double* SUM, int64_t lds, void* stream);

/* towr_gpu_alsolve_iterate_batch_device with the Gauss-Newton direction: `iters` complete iterations on `stream`, with
 * no host synchronisation. DC (B rows, ldx) and GSUM (ldgs >= 6) are caller-owned DEVICE memory beside `state`: the
 * direction at the candidate and its summary. One iteration:
 *   1. towr_gpu_eval_cost_batch_device at XC, F = FC and GRAD = GRC;
 *   2. towr_gpu_eval_batch_device at XC (g and the values in handle scratch), towr_gpu_residual_batch_device with LAM
 *      and rho = RHO[b] (LAMP, RSUM), towr_gpu_jac_tvec_batch_device of LAMP accumulated onto GRC, and
 *      towr_gpu_gn_direction_batch_device on those values with (LAMP, RHO, X = XC, GR = GRC), RUN = ISTATE and
 *      run_stride = 4 (frozen problems are skipped), D = DC, SUM = GSUM;
 *   3. towr_gpu_linesearch_batch_device (it still offers pairs to the history, which arms the retry below);
 *   4. towr_gpu_auglag_outer_batch_device;
 *   5. the select, per problem by the flags the line search wrote (the outer update clears them where it acts): bit 0
 *      (a base was accepted: X = XC, GR = GRC) D <- DC; else bit 2 (the trial length fell through alpha_min with a pair
 *      in the history) D <- GR, one steepest-descent retry; else D is untouched. Copies, bit for bit;
 *   6. towr_gpu_step_batch_device, XC = P(X - ALPHA D), SSUM its SUM.
 * Bit-identical to those calls in sequence, whatever the products chunk. HS, HY and HMETA are written by the line search
 * but no direction reads them; DSUM is not written. Frozen problems, batch terrains, the cross-stream scratch rule and
 * the kept Jacobian as for towr_gpu_alsolve_iterate_batch_device. TOWR_ERR_INVALID before anything runs for what that
 * entry refuses, NULL gn, DC or GSUM, ncg < 1, mu or tol negative or NaN, ldgs < 6. TOWR_ERR_UNSUPPORTED as for the
 * L-BFGS kernels and the GN direction.                                                                              */
int towr_gpu_alsolve_gn_iterate_batch_device(towr_gpu_handle h, int32_t B, int32_t iters,
                                             const towr_alsolve_params_t* params, const towr_alsolve_state_t* state,
                                             const towr_gn_params_t* gn, double* DC, double* GSUM, int64_t ldgs,
                                             const double* GL, const double* GU, int64_t ldgb,
                                             const double* XL, const double* XU, int64_t ldxb, void* stream);

/* ---- the Gauss-Newton direction with a Jacobi (diagonal) preconditioner ------------------------------------------ */
#define TOWR_GN_PC_NONE 0
#define TOWR_GN_PC_JACOBI 1

/* towr_gpu_gn_direction_batch_device with a choice of preconditioner. PC (B rows, ldpc >= n) is caller-owned DEVICE
 * memory; lds >= 8. precond = TOWR_GN_PC_NONE launches that entry's kernel: D and SUM[0..5] are its bits, PC (which
 * may be NULL) and SUM[6..7] are not written. precond = TOWR_GN_PC_JACOBI, per problem, with H, w, rho_b, g, the held
 * columns and RUN exactly as above:
 *   dg_j = sum_i w_i * (v_ij * v_ij) over the entries of column j (two rounded products per term; a NaN or infinity in
 *   an inactive row still gives NaN), summed on the by-column tree of towr_gpu_jac_tvec_batch_device: the bits that
 *   entry gives for the values v*v and LAM = w;
 *   M_j = rho_b * dg_j + mu (one rounded product, one rounded addition); M_j == 0.0 exactly is replaced by 1.0 (a
 *   column without active entries at mu = 0); a NaN stays NaN. PC[b*ldpc + j] = M_j on free columns, +0.0 on held ones.
 * From d = 0: r = g and z = r ./ M (a division) on free columns, p = z (0 on held ones), bb = rr = sum_free g^2,
 * rz = sum_free r z; bb == 0 ends at once (code 3; PC, SUM[6] and SUM[7] are written all the same); else for it < ncg:
 *   1. stop (code 1) if rr <= (tol*tol)*bb;
 *   2. t = w .* (J p);   3. Hp = rho_b * (J^T t) + mu * p on free columns;   4. pHp = sum_free p Hp;
 *   5. stop (code 2) unless pHp > 0 (a NaN anywhere ends here);
 *   6. a = rz / pHp, d = d + a p, r = r - a Hp, z = r ./ M, rn = sum_free r r, rzn = sum_free r z,
 *      p = z + (rzn / rz) p, rz = rzn, rr = rn; one step completed.
 * D and SUM[0..5] as above ([2] is the true residual rr, not rz); SUM[6] the final rz; SUM[7] the number of free columns
 * whose M was replaced by 1.0. A problem skipped by RUN has no byte of its D, PC or SUM row touched. The same trees and
 * the same independence of B, position, stream and run as above; nothing beyond n (PC) or 8 (SUM) is read or written in
 * a row. TOWR_ERR_INVALID before anything runs for what the entry above refuses, precond outside {0, 1}, PC NULL with
 * TOWR_GN_PC_JACOBI, ldpc < n (with PC), lds < 8, and a PC that overlaps V, LAMP, X, GR or D. TOWR_ERR_UNSUPPORTED as
 * above: the kernel's LDS is the same (M lives in PC).                                                            */
int towr_gpu_gn_direction_pc_batch_device(towr_gpu_handle h, int32_t B, const towr_gn_params_t* gn, int32_t precond,
                                          const double* V, int64_t ldv, const double* LAMP, int64_t ldlp,
                                          const double* RHO, double rho, const double* X, int64_t ldx,
                                          const double* GR, int64_t ldgr, const double* XL, const double* XU, int64_t ldb,
                                          const int32_t* RUN, int32_t run_stride, double* D, int64_t ldd,
                                          double* SUM, int64_t lds, double* PC, int64_t ldpc, void* stream);

/* towr_gpu_alsolve_gn_iterate_batch_device with that direction: step 2 calls towr_gpu_gn_direction_pc_batch_device
 * with `precond` and PC (B rows, leading dimension ldx; caller-owned DEVICE memory) at the chunk's rows; ldgs >= 8.
 * Everything else is that entry's. Bit-identical to the public calls in sequence, whatever the products chunk, and with
 * precond = TOWR_GN_PC_NONE to that entry (PC may be NULL, GSUM[6..7] is not written). TOWR_ERR_INVALID before anything
 * runs for what that entry refuses, precond outside {0, 1}, PC NULL with TOWR_GN_PC_JACOBI, ldgs < 8, and a PC that
 * overlaps LAMP, XC, GRC or DC.                                                                                    */
int towr_gpu_alsolve_gn_pc_iterate_batch_device(towr_gpu_handle h, int32_t B, int32_t iters,
                                                const towr_alsolve_params_t* params, const towr_alsolve_state_t* state,
                                                const towr_gn_params_t* gn, int32_t precond, double* DC, double* GSUM,
                                                int64_t ldgs, double* PC, const double* GL, const double* GU, int64_t ldgb,
                                                const double* XL, const double* XU, int64_t ldxb, void* stream);

/* ---- a direct Gauss-Newton direction: batched envelope Cholesky of rho J^T W J + mu I ------------------------------- */
#define TOWR_GN_ORDER_RCM 1

/* The symbolic phase, on the host, once per handle (a layout-only handle answers too). The ordering is reverse
 * Cuthill-McKee on the graph of J^T J (two columns are adjacent when a row of the pattern holds both), a function of the
 * pattern alone: connected components in the order of their (degree, index)-smallest column; a breadth-first search that
 * appends a node's unvisited neighbours by ascending (degree, index); the whole sequence reversed. It is run from two
 * starts per component — that column itself, and the George-Liu pseudo-peripheral node found from it — and the ordering
 * with the smaller envelope is kept (the pseudo-peripheral one on a tie). *ordering = TOWR_GN_ORDER_RCM. pos[j] (n ints) is
 * the permuted position of column j; first[q] (n ints) the permuted position of the first entry of permuted row q of
 * the lower triangle, first[q] <= q: every structural nonzero (q, c) of the permuted J^T J has first[q] <= c <= q.
 * *envelope = sum_q (q - first[q] + 1), *bandwidth = max_q (q - first[q]), *ldw_min = the workspace doubles per problem
 * of the entry below (the envelope: everything else the kernel needs lives in LDS). Any output pointer may be NULL.  */
int towr_gpu_gn_factor_info(towr_gpu_handle h, int32_t* ordering, int32_t* pos, int32_t* first, int64_t* envelope,
                            int64_t* bandwidth, int64_t* ldw_min);

/* Per problem an exact solve of H d = g on the free columns, H = rho_b (J^T diag(w) J)_ff + mu I, by a Cholesky
 * factorisation inside the envelope of towr_gpu_gn_factor_info. V, LAMP, w, RHO / rho, X, GR, XL, XU, ldb, the held
 * columns, RUN / run_stride, D as for towr_gpu_gn_direction_batch_device; of gn only mu >= 0 is read (mu = 0 is valid).
 * W is caller-owned DEVICE workspace of min(B, wrows) rows, ldw >= ldw_min, wrows >= 1: the call runs ceil(B / wrows)
 * launches in sequence on the stream and problem b uses row b mod wrows; its contents after the call are unspecified.
 * With q = pos[j], c = pos[k] the permuted positions of columns j, k:
 *   assembly, into the envelope: H_qc = rho_b * a, a = sum_i w_i * (v_ij * v_ik) over the rows i that hold both columns in
 *   ascending row order from 0.0 (two rounded products per term: a NaN or infinity in an inactive row still gives NaN);
 *   the diagonal is rho_b * a + mu; an off-diagonal entry of the envelope whose columns share no row is +0.0; where j or
 *   k is held the entry is 1.0 on the diagonal and 0.0 elsewhere;
 *   factorisation L L^T in place, permuted columns c ascending: piv_c = H_cc - sum_k L_ck^2 (k ascending from first[c],
 *   the sum from 0.0), L_cc = sqrt(piv_c), L_rc = (H_rc - sum_k L_rk L_ck) / L_cc for the rows r > c with first[r] <= c,
 *   k ascending from max(first[r], first[c]) to c - 1, the sum from 0.0. The first column whose pivot is not > 0 (a NaN
 *   counts) ends the problem: code 2, D = GR bit for bit, no other problem is affected;
 *   L y = g~ (g~_q = g_j): y_q = (g~_q - sum_k L_qk y_k) / L_qq, k ascending from first[q], the sum from 0.0;
 *   L^T d~ = y: d~_c = (y_c - sum_r L_rc d~_r) / L_cc over the rows r > c of the envelope in descending r, from 0.0;
 *   D_j = d~_q on free columns, g_j bit for bit on held ones.
 * Every square root and division is IEEE's; no product is contracted with a sum. bb = sum_free g^2 (the sum of the entry
 * above); bb == 0 ends at once with code 3 and D = GR, without factorising. SUM[b*lds + ..] holds 8 doubles (lds >= 8):
 * [0] 1.0 when solved, else 0.0; [1] bb; [2] the smallest and [6] the largest accepted pivot over the free columns
 * (both 0.0 when there is none); [3] sum_j g_j D_j over all columns; [4] the number of held columns; [5] the code: 1
 * solved, 2 breakdown, 3 bb == 0; [7] the permuted index of the breakdown column, or -1.0. A problem skipped by RUN has
 * no byte of its D or SUM row touched. Every sum has one fixed order, so problem b's outputs are a function of its own
 * operands alone: the same bits for any B, position, wrows, stream and run. No handle scratch is used and the kept
 * Jacobian is not dropped. TOWR_ERR_INVALID before anything runs for: NULL gn, V, LAMP, GR, D, SUM or W, mu negative or
 * NaN, rho <= 0 or NaN with RHO == NULL, ldv < nnz, ldlp < m, ldx (with X) / ldgr / ldd < n, lds < 8, only one of
 * XL / XU, 0 < ldb < n, ldw < ldw_min, wrows < 1, and a used W row that overlaps V, LAMP, X, GR, D or SUM.
 * TOWR_ERR_UNSUPPORTED at the call when the envelope has 2^31 entries or more (the kernel's offsets are 32-bit) or the
 * kernel's LDS (32 n + 16 bandwidth + m + n bytes and padding) does not fit the workgroup's 160 KiB less 1 KiB.     */
int towr_gpu_gn_direction_direct_batch_device(towr_gpu_handle h, int32_t B, const towr_gn_params_t* gn,
                                              const double* V, int64_t ldv, const double* LAMP, int64_t ldlp,
                                              const double* RHO, double rho, const double* X, int64_t ldx,
                                              const double* GR, int64_t ldgr, const double* XL, const double* XU, int64_t ldb,
                                              const int32_t* RUN, int32_t run_stride, double* D, int64_t ldd,
                                              double* SUM, int64_t lds, double* W, int64_t ldw, int32_t wrows, void* stream);

/* towr_gpu_alsolve_gn_iterate_batch_device with that direction: step 2 calls towr_gpu_gn_direction_direct_batch_device
 * on the chunk's values with W, ldw and wrows (wrows applies within each products chunk: a chunk of cb problems uses
 * min(cb, wrows) rows); ldgs >= 8. Everything else is that entry's: the select, the line search, the outer update.
 * Bit-identical to the public calls in sequence, whatever the products chunk. TOWR_ERR_INVALID before anything runs for
 * what that entry refuses except gn's ncg and tol (not read), NULL W, ldw < ldw_min, wrows < 1, ldgs < 8, and a used W
 * row that overlaps LAMP, XC, GRC, DC or GSUM. TOWR_ERR_UNSUPPORTED as for the L-BFGS kernels and the direct direction. */
int towr_gpu_alsolve_gn_direct_iterate_batch_device(towr_gpu_handle h, int32_t B, int32_t iters,
                                                    const towr_alsolve_params_t* params, const towr_alsolve_state_t* state,
                                                    const towr_gn_params_t* gn, double* DC, double* GSUM, int64_t ldgs,
                                                    double* W, int64_t ldw, int32_t wrows,
                                                    const double* GL, const double* GU, int64_t ldgb,
                                                    const double* XL, const double* XU, int64_t ldxb, void* stream);

/* ---- the direct Gauss-Newton direction on 16 x 16 tiles: a block Cholesky inside the tile envelope ------------------ */
#define TOWR_GN_TILE 16

/* The tile envelope of towr_gpu_gn_factor_info's ordering, on the host, once per handle (a layout-only handle answers
 * too). *tile = TOWR_GN_TILE, *nt = ceil(n / 16) block rows; bfirst[I] (nt ints) = min over the permuted rows q in
 * [16 I, min(n, 16 I + 16)) of first[q] / 16 (first of towr_gpu_gn_factor_info), bfirst[I] <= I: block row I stores the
 * tiles (I, bfirst[I]) .. (I, I), which cover every entry of the scalar envelope in its rows. *tiles = sum_I (I -
 * bfirst[I] + 1). A block envelope has no fill outside itself, so this is the whole symbolic phase. *ldw_min = 256 *
 * *tiles exactly: the workspace doubles per problem of the entry below are its stored tiles and nothing else (everything
 * else the kernel needs lives in LDS). Permuted rows and columns n .. 16 nt - 1 are padding: the identity on the diagonal,
 * 0 elsewhere, nothing read from V. Any output pointer may be NULL.                                                   */
int towr_gpu_gn_tile_info(towr_gpu_handle h, int32_t* tile, int32_t* nt, int32_t* bfirst, int64_t* tiles, int64_t* ldw_min);

/* towr_gpu_gn_direction_direct_batch_device's system, arguments, held rule, codes and SUM slots, with the factorisation
 * done as a block Cholesky on the stored tiles. Kept from that entry word for word: V, LAMP, w, RHO / rho, X, GR, XL, XU,
 * ldb, RUN / run_stride (a skipped problem has no byte of its D or SUM row touched), mu, the launches (ceil(B / wrows) in
 * sequence, problem b uses row b mod wrows of W, whose contents after the call are unspecified), bb and its sum, bb == 0
 * giving code 3 without factorising, D = GR bit for bit on held columns and on every column under code 2 or 3, SUM[0..7]
 * (pivots of padding columns are not counted in [2] and [6]); [7] is the scalar permuted column (16 J + k) of the first
 * pivot that is not > 0 (a NaN counts), or -1.0.
 *   assembly: every stored entry (q, c), c <= q < n, is the direct entry's H_qc by the same per-entry sum (rows ascending
 *   from 0.0, +0.0 where the columns share no row — also everywhere left of the scalar envelope —, rho_b * a + mu on the
 *   diagonal, the identity where j or k is held): bit-equal to that entry's H wherever both hold the entry. The rows of
 *   every entry's sum are listed once per handle at the first device call: sum over the rows of J of len (len + 1) / 2
 *   terms of 12 bytes of device memory (ANYmal trot: 4 MiB; with phase-duration optimisation: 158 MiB);
 *   factorisation, left-looking by block column J ascending, on tiles A_IJ (I >= J, bfirst[I] <= J):
 *     A_IJ <- H_IJ - sum_K L_IK L_JK^T, tile index K ascending from max(bfirst[I], bfirst[J]) to J - 1, and within a tile
 *     k ascending in groups of four: one v_mfma_f64_16x16x4_f64 per group subtracts its four products from the running
 *     tile (its first operand negated, which is exact), their inner order and rounding the instruction's;
 *     the diagonal tile unblocked, k = 0 .. 15 ascending: piv = A_kk; the first pivot that is not > 0 ends the problem
 *     (code 2); L_kk = sqrt(piv); L_rk = A_rk / L_kk for r > k; then A_rc <- A_rc - L_rk * L_ck for k < c <= r (a
 *     rounded product, then a rounded difference);
 *     the tiles under it, each row on its own: L_rc = (A_rc - L_r0 L_c0 - ... - L_r,c-1 L_c,c-1) / L_cc, c ascending,
 *     the products subtracted one by one in ascending k, each rounded;
 *   L y = g~ by blocks: for block J, s_r = sum over K ascending and k of L_rk y_k in four partial sums (k mod 4; each
 *   from 0.0, k ascending), combined (p0 + p1) + (p2 + p3); t_r = g~_r - s_r; then with the diagonal tile, k ascending:
 *   y_k = t_k / L_kk, t_r <- t_r - L_rk * y_k for r > k;
 *   L^T d~ = y by blocks descending: t_c = y_c - acc_c; k = 15 .. 0: d~_k = t_k / L_kk, t_c <- t_c - L_kc * d~_k for c < k;
 *   then for every stored tile (J, K), K < J: acc_c += sum_r L_rc d~_r, the sum from 0.0 in descending r; acc starts at
 *   0.0 and receives the block rows in descending J;
 *   D_j = d~_q on free columns, g_j bit for bit on held ones.
 * Apart from the v_mfma_f64_16x16x4_f64 no product is contracted with a sum; every square root and division is IEEE's.
 * This order is one fixed order per handle, so problem b's outputs are a function of its own operands alone: the same
 * bits for any B, position, wrows, stream and run. They are NOT promised to equal the direct entry's bits, and no host
 * restatement is promised to match them bit for bit (the instruction's inner order is not stated). No handle scratch is
 * used and the kept Jacobian is not dropped. TOWR_ERR_INVALID as for the direct entry, with ldw_min that of
 * towr_gpu_gn_tile_info. TOWR_ERR_UNSUPPORTED at the call when 256 * tiles or the number of the assembly's terms
 * reaches 2^31 (the kernel's offsets are 32-bit) or the kernel's LDS (16 nt * 17 + 2048 + m bytes and padding: per-column state and one tile; the factor is read from
 * the workspace, not held in LDS) does not fit the workgroup's 160 KiB less 1 KiB.                                    */
int towr_gpu_gn_direction_tiled_batch_device(towr_gpu_handle h, int32_t B, const towr_gn_params_t* gn,
                                             const double* V, int64_t ldv, const double* LAMP, int64_t ldlp,
                                             const double* RHO, double rho, const double* X, int64_t ldx,
                                             const double* GR, int64_t ldgr, const double* XL, const double* XU, int64_t ldb,
                                             const int32_t* RUN, int32_t run_stride, double* D, int64_t ldd,
                                             double* SUM, int64_t lds, double* W, int64_t ldw, int32_t wrows, void* stream);

/* towr_gpu_alsolve_gn_direct_iterate_batch_device with the tiled direction in step 2 (W rows of towr_gpu_gn_tile_info's
 * ldw_min). Bit-identical to the public calls in sequence, whatever the products chunk. The refusals are that entry's,
 * TOWR_ERR_UNSUPPORTED as for the L-BFGS kernels and the tiled direction.                                              */
int towr_gpu_alsolve_gn_tiled_iterate_batch_device(towr_gpu_handle h, int32_t B, int32_t iters,
                                                   const towr_alsolve_params_t* params, const towr_alsolve_state_t* state,
                                                   const towr_gn_params_t* gn, double* DC, double* GSUM, int64_t ldgs,
                                                   double* W, int64_t ldw, int32_t wrows,
                                                   const double* GL, const double* GU, int64_t ldgb,
                                                   const double* XL, const double* XU, int64_t ldxb, void* stream);

/* ---- a solve to completion: the resident loop in rounds, frozen problems compacted out of the batch ----------------- */
/* The partition plan of a batch by its phases. ISTATE is int32_t[4*B] as in towr_alsolve_state_t (only the phase word
 * ISTATE[4 b] is read), HEAD is int32_t[8], PAIRS is int32_t[2*(B/2)]; all DEVICE pointers. Row b is ACTIVE iff its
 * phase word is 0 (RESTART) or 1 (SEARCH); any other value, negative and out-of-range ones included, is FROZEN.
 *   HEAD[0] = na, the number of active rows; HEAD[1] = np, the number of pairs; HEAD[2..6] = the number of rows with
 *   phase 0, 1, 2, 3, 4; HEAD[7] = the number of rows with any other value.
 *   Pair i is (PAIRS[2 i], PAIRS[2 i + 1]) = (f_i, a_i): f_i the i-th frozen row of [0, na), a_i the i-th active row of
 *   [na, B), both ascending. There are equally many of both; np is that number (np <= B / 2).
 * After the rows of every pair have been exchanged, rows [0, na) are all active, rows [na, B) all frozen, and a row that
 * was on its side already has not moved. Nothing of PAIRS beyond 2 np ints is written. One block, integer counts in a
 * fixed order: the outputs are a function of the phase words. B = 0 writes HEAD = 0. No handle scratch; the kept
 * Jacobian is not dropped. TOWR_ERR_INVALID before anything runs for a NULL pointer or B < 0.                          */
int towr_gpu_alsolve_partition_batch_device(towr_gpu_handle h, int32_t B, const int32_t* ISTATE, int32_t* HEAD,
                                            int32_t* PAIRS, void* stream);

/* The rows of an array: row r is bytes [r*ld_bytes, r*ld_bytes + row_bytes) from base (DEVICE memory). */
typedef struct { void* base; int64_t ld_bytes; int64_t row_bytes; } towr_rows_t;
#define TOWR_SWAP_MAX_ARRAYS 32

/* Exchanges rows in place: for every pair i < count and every array k < n_arrays, bytes [0, row_bytes) of rows
 * PAIRS[2 i] and PAIRS[2 i + 1] of array k. Not one byte beyond row_bytes of any row is read or written: the padding up
 * to ld_bytes stays exactly as it was. `arrays` is HOST memory, read at the call; PAIRS (and NP) are DEVICE pointers.
 *   NP != NULL: count = min(NP[0], max_pairs), read on the device (NP is typically the partition's HEAD + 1, so no host
 *   round trip lies between the two calls); the grid holds max_pairs pairs and the blocks beyond count exit; npairs is
 *   not read. NP == NULL: count = npairs, a host value; max_pairs is not read.
 * The pairs must be disjoint (no row in two of them) and index rows every array holds, as the partition's are; a pair
 * with a negative index or two equal ones is skipped. A list of disjoint pairs is an involution: the same call again
 * undoes it. row_bytes is a positive multiple of 4, base and ld_bytes are multiples of 4 and ld_bytes >= row_bytes; 8
 * bytes move per lane where base, ld_bytes and row_bytes are all multiples of 8, else 4. Both rows are read before
 * either is written. No handle scratch; the kept Jacobian is not dropped. TOWR_ERR_INVALID before anything runs for:
 * NULL PAIRS, NULL arrays with n_arrays > 0, npairs < 0 (NP NULL) or max_pairs < 0 (NP given), n_arrays outside
 * 0..TOWR_SWAP_MAX_ARRAYS, a descriptor with a NULL or misaligned base, ld_bytes or row_bytes not a positive multiple of
 * 4, ld_bytes < row_bytes, and two descriptors whose rows 0 share a byte (with equal ld_bytes that is every row of both:
 * one array passed twice, or two views of the same columns; rows of different index cannot be told apart without a row
 * count and are the caller's business).                                                                              */
int towr_gpu_alsolve_swap_rows_batch_device(towr_gpu_handle h, const int32_t* NP, int32_t npairs, int32_t max_pairs,
                                            const int32_t* PAIRS, int32_t n_arrays, const towr_rows_t* arrays,
                                            void* stream);

/* The solve driver's options (host memory, read at the call): the iterate entry that runs the iterations, the most
 * iterations (>= 0), the iterations per round K (>= 1; the host looks at the batch once per round), and whether frozen
 * problems are compacted out of the batch (0 or 1).                                                                  */
#define TOWR_SOLVE_LBFGS 0      /* towr_gpu_alsolve_iterate_batch_device           */
#define TOWR_SOLVE_GN 1         /* towr_gpu_alsolve_gn_iterate_batch_device        */
#define TOWR_SOLVE_GN_PC 2      /* towr_gpu_alsolve_gn_pc_iterate_batch_device     */
#define TOWR_SOLVE_GN_DIRECT 3  /* towr_gpu_alsolve_gn_direct_iterate_batch_device */
#define TOWR_SOLVE_GN_TILED 4   /* towr_gpu_alsolve_gn_tiled_iterate_batch_device  */
typedef struct { int32_t method, max_iters, check_every, compact; } towr_solve_opts_t;
/* What the method's iterate entry takes beside `state` (host memory; the pointers in it are DEVICE pointers): gn,
 * precond and PC (GN_PC), DC, GSUM, ldgs (every GN method), W, ldw, wrows (GN_DIRECT, GN_TILED). Fields the method does
 * not read may be NULL or 0.                                                                                         */
typedef struct {
  const towr_gn_params_t* gn;
  int32_t precond, wrows;
  double *DC, *GSUM; int64_t ldgs;
  double* PC;
  double* W; int64_t ldw;
} towr_solve_dir_t;
/* Written at return (host memory): the rounds run, the iterations run (the same for every problem still in the batch),
 * the sum over the rounds of (rows in the round's batch) x (iterations of the round), and HEAD[2..7] of a final
 * partition over all B rows: the number of problems in phase 0, 1, 2, 3, 4 and with any other phase word.             */
typedef struct { int32_t rounds, iters_run; int64_t problem_iters; int32_t n_phase[6]; int32_t reserved[2]; } towr_solve_report_t;

/* Runs the resident loop until every problem is frozen or max_iters iterations have run. The caller has run
 * towr_gpu_alsolve_init_batch_device (or holds a state that an iterate entry left); this entry does not. With Bcur = B,
 * rounds run while iters_run < max_iters and Bcur > 0. One round, all on `stream`:
 *   1. k = min(check_every, max_iters - iters_run) iterations of the method's iterate entry on rows [0, Bcur), its own
 *      launches and checks;
 *   2. towr_gpu_alsolve_partition_batch_device over rows [0, Bcur): HEAD = LOG[0..7], the pairs behind those of the
 *      rounds before (LOG + 8 + 2 * the pairs so far);
 *   3. with compact = 1, towr_gpu_alsolve_swap_rows_batch_device with NP = LOG + 1 on every per-problem array (below);
 *   4. a copy of HEAD to page-locked host memory and ONE synchronisation of the stream;
 *   5. the host reads na and np: it stops when na == 0, and with compact = 1 sets Bcur = na.
 * With compact = 0, Bcur stays B and no swap is queued: the same rounds on the whole batch. When the loop has ended, the
 * swaps of all rounds are run again in reverse order (host counts, NP = NULL), which puts every array back in the
 * caller's order; then a final partition over all B rows fills `report`, and a last synchronisation. THE ENTRY BLOCKS
 * THE HOST: one synchronisation per round and one before it returns; on return all its work on `stream` has finished.
 * LOG is caller-owned DEVICE memory, int32_t[8 + 2 B]: a frozen row moves at most once (out of the front into the tail
 * of its round, which no later round touches), so the pairs of all rounds number at most B. Its contents after the call
 * are the final partition's HEAD and unspecified pairs.
 *   Arrays exchanged (with the used widths stated for each): every per-problem row of `state` — X, GR, XC, GRC, D (n),
 *   LAM, LAMP (m), HS, HY (a problem's `mem` pairs as one row: (mem - 1) ldh + n doubles at mem ldh, so the padding
 *   between a problem's pairs travels with it), HMETA (2 ints), ALPHA, RHO, FC (1), SCAL (8), ISTATE (4 ints), RSUM
 *   (4 + n_constraints), SSUM (5 + n_varsets), DSUM (5), USUM (6), LSUM (8); DC (n, at ldx) and GSUM (6; 8 for GN_PC,
 *   GN_DIRECT and GN_TILED) for the GN methods; GL / GU (m) and XL / XU (n) when their leading dimension is > 0 — they
 *   are per-problem rows then, are PERMUTED DURING THE CALL AND BACK IN THE CALLER'S ORDER AT RETURN, and are therefore
 *   not const here; a leading dimension of 0 (one shared row) and NULL (the handle's bounds) are not touched. When batch
 *   terrains are set (towr_gpu_set_batch_terrain; exactly B of them), the driver permutes a private device copy and
 *   hands that to the launches: the handle's set is not modified. W and PC are not exchanged; their contents after the
 *   call are unspecified.
 *   Persistent arrays: X, GR, LAM, RHO, SCAL, ISTATE, HS, HY, HMETA, D, ALPHA — those the iterate entries never change
 *   again once a problem is frozen — are at return, for every problem, bit for bit what the method's iterate entry
 *   leaves after iters_run iterations on the whole batch; for compact = 0 and 1 alike, for any check_every that gives the
 *   same iters_run, any products chunk, any wrows (problem b's outputs are a function of its own operands alone, so its
 *   place in the batch does not matter).
 *   Candidate-side and summary rows: XC, GRC, FC, LAMP, RSUM, SSUM, DSUM, USUM, LSUM, DC, GSUM are the iterate entry's
 *   bits for the problems active to the end (and for every problem with compact = 0); for a problem frozen before the
 *   last round they are those of the last iteration in which it was part of the batch.
 *   Failure: if a launch or copy fails after the first swap, the recorded swaps are still run in reverse and the first
 *   error is returned; if that fails too, the row order is unspecified and towr_gpu_last_error says so.
 * Handle scratch, the cross-stream rule and the kept Jacobian as for the iterate entry. TOWR_ERR_INVALID before anything
 * runs for: NULL opts, dir, LOG or report, a method outside 0..4, max_iters < 0, check_every < 1, compact outside
 * {0, 1}, everything the method's iterate entry refuses for these arguments, an array above that fails the swap's
 * checks, and batch terrains set for another number of problems than B. TOWR_ERR_UNSUPPORTED and TOWR_ERR_NO_DEVICE as
 * for that iterate entry.                                                                                            */
int towr_gpu_alsolve_solve_batch_device(towr_gpu_handle h, int32_t B, const towr_solve_opts_t* opts,
                                        const towr_alsolve_params_t* params, const towr_alsolve_state_t* state,
                                        const towr_solve_dir_t* dir, double* GL, double* GU, int64_t ldgb,
                                        double* XL, double* XU, int64_t ldxb, int32_t* LOG, towr_solve_report_t* report,
                                        void* stream);

/* ---- two more stops for the resident loop: an acceptable point, and an infeasible stationary point ----------------- */
/* Two more frozen phases. Every kernel above treats a phase word outside {0, 1} as frozen, so a problem in one of them
 * is skipped by the line search, the directions' RUN masks and the partition like a CONVERGED one.
 *   ACCEPTABLE: the base stayed within (acc_eta, acc_omega) for acc_iters consecutive iterations while the loop could
 *     not reach (eta_star, omega_star): the counterpart of IPOPT's acceptable termination (acceptable_tol,
 *     acceptable_iter).
 *   INFEASIBLE: the penalty is about to grow again although it is already >= infeas_rho and the violation has not
 *     fallen below infeas_keep x its value at the previous growth: a stationary point of the infeasibility.          */
#define TOWR_AL_ACCEPTABLE 5
#define TOWR_AL_INFEASIBLE 6

/* The rule's parameters (host memory, read at the call). acc_iters = 0 switches the acceptable rule off;
 * infeas_rho = +inf switches the infeasible rule off. TOWR_ERR_INVALID before anything runs for: acc_eta, acc_omega or
 * infeas_rho negative or NaN, acc_iters < 0, infeas_keep outside (0, 1] or NaN.                                     */
typedef struct {
  double acc_eta, acc_omega;
  int32_t acc_iters, reserved;
  double infeas_keep, infeas_rho;
} towr_alsolve_stop_t;

/* The stop rule alone, between towr_gpu_linesearch_batch_device and towr_gpu_auglag_outer_batch_device. One thread per
 * problem. It acts on problem b only if phase == SEARCH; of any other problem (RESTART, frozen, any other word) not one
 * byte changes. It keeps its memory in the two spare slots of SCAL, which towr_gpu_alsolve_init_batch_device zeroes:
 * SCAL[6], a run length (a small exact integer held in a double), and SCAL[7], the violation at the previous penalty
 * growth. With viol = SCAL[4], pg = SCAL[1], omega = SCAL[3], eta = SCAL[2], flags and inner as the line search left
 * them, and with acc_iters > 0:
 *   run = (viol <= acc_eta and pg <= acc_omega) ? SCAL[6] + 1 : 0; SCAL[6] = run;
 *   run >= acc_iters: phase = ACCEPTABLE, ALPHA[b] = 0, flags = 0; nothing else.
 * (acc_iters = 0: SCAL[6] is not written and the rule never fires.) Otherwise, with
 *   grow = (flags & 1) and (pg <= omega or inner >= max_inner) and not (viol <= eta),
 * which is exactly the outer update's condition for its RHO branch (a NaN viol included):
 *   grow and SCAL[7] > 0 and viol >= infeas_keep * SCAL[7] (one rounded product) and RHO[b] >= infeas_rho:
 *     phase = INFEASIBLE, ALPHA[b] = 0, flags = 0 (the outer update then does not act on the problem);
 *   grow otherwise: SCAL[7] = viol (the outer update grows RHO behind this call).
 * A NaN operand falls on the NON-STOPPING side of every comparison: a NaN viol or pg resets the run length; a NaN
 * viol, SCAL[7] or RHO[b] never gives INFEASIBLE (a NaN viol is then recorded in SCAL[7], and fails the next test
 * too). Only IEEE comparisons and the one product: problem b's outputs are a function of its own operands. Of `params`
 * only max_inner is used, but the whole struct is checked as in the outer update. Fields used: ALPHA, RHO, SCAL,
 * ISTATE. No handle scratch; the kept Jacobian is not dropped. TOWR_ERR_INVALID before anything runs for: NULL params,
 * state or stop, an invalid params or stop field, NULL ISTATE, SCAL, HMETA, ALPHA or RHO, ldsc < 8, B < 0.           */
int towr_gpu_alsolve_stop_batch_device(towr_gpu_handle h, int32_t B, const towr_alsolve_params_t* params,
                                       const towr_alsolve_stop_t* stop, const towr_alsolve_state_t* state, void* stream);

/* towr_gpu_alsolve_solve_batch_device with the stop rule in every iteration: the method's iterate entry with
 * towr_gpu_alsolve_stop_batch_device between its line search and its outer update (bit-identical to those calls in
 * sequence). Compaction needs nothing more: SCAL rows travel with their problem. report->reserved[0] and [1] hold the
 * number of problems in phase ACCEPTABLE and INFEASIBLE after the final partition (both are also part of n_phase[5],
 * "any other word"). stop == NULL: towr_gpu_alsolve_solve_batch_device itself, its launches and its report
 * (reserved = 0). TOWR_ERR_INVALID before anything runs for what that entry refuses and for an invalid stop field.   */
int towr_gpu_alsolve_solve_ex_batch_device(towr_gpu_handle h, int32_t B, const towr_solve_opts_t* opts,
                                           const towr_alsolve_params_t* params, const towr_alsolve_stop_t* stop,
                                           const towr_alsolve_state_t* state, const towr_solve_dir_t* dir, double* GL,
                                           double* GU, int64_t ldgb, double* XL, double* XU, int64_t ldxb, int32_t* LOG,
                                           towr_solve_report_t* report, void* stream);

/* ---- probing the trial lengths before the expensive iteration ---------------------------------------------------------- */
/* A rejected trial of the loops above pays for a whole iteration (in the GN loops: a direction at the candidate) although
 * the line search only looks at the merit f + phi. The probe stage tests up to `trials` lengths of the line search's own
 * ladder with cheap evaluations (an f-only objective launch, a g-only evaluation and the residual kernel) and leaves the
 * state where the sequential loop would stand after the rejections it found, so that the following iteration runs at a
 * length already known to pass. The bases the loop visits are bit for bit those of the loop without probes.
 * trials = T in 1..TOWR_PROBE_MAX (host memory, read at the call).                                                      */
#define TOWR_PROBE_MAX 8
typedef struct { int32_t trials, reserved; } towr_alsolve_probe_t;

/* The probe stage alone, in front of an iteration. PSUM (DEVICE, ldps >= 8) is its per-problem summary. A problem whose
 * phase word is not SEARCH gets PSUM[b][0] = 0 and not one other byte of it changes (XC and PSUM[b][1..7] included). For
 * a SEARCH problem, with X, D, GR, LAM[b], RHO[b], M0 = SCAL[0] and the bounds as the iteration sees them:
 *   lengths: a_0 = ALPHA[b], a_t = a_{t-1} * shrink (one rounded product each: the bits the line search's rejected branch
 *     produces). v = the number of leading t in 0..T with a_t >= alpha_min (a NaN ends the run); t = 0 always counts.
 *   probes, for t < min(v, T) in ascending order: XT = P(X - a_t D), towr_gpu_step_batch_device's expression;
 *     MC_t = F(XT) + phi(XT; LAM[b], RHO[b]), one rounded addition of the objective kernel's f (its f-only launch, whose F
 *     is the gradient launch's bit for bit) and the residual kernel's SUM[3] at a g-only evaluation: the bits the line
 *     search computes at the same point; gs_t = sum_j GR_j (XT_j - X_j) on the line search's tree;
 *     pass_t = gs_t <= 0 and MC_t <= M0 + c1*gs_t, the line search's test (a NaN anywhere makes it false).
 *   choice: t* = the first passing t. If none passes: t* = T when a_T is valid (the next, untested length), else
 *     t* = v - 1 (the last valid length, known to fail: the following line search takes its code 4 / 5 branch at exactly
 *     the base and counters of the sequential loop).
 *   writes: ALPHA[b] = a_{t*}; XC = P(X - a_{t*} D); ISTATE inner += t* (the outer update's inner >= max_inner sees the
 *     sequential loop's number); PSUM[b] = {code, t*, lengths probed, a_{t*}, MC_{t*} (NaN when untested), gs_{t*}, 0, 0},
 *     code 1: a probed length passed, 2: none passed and an untested length follows, 3: none passed and the last valid
 *     length stays.
 * The candidates, their g, lam+ and summaries live in handle scratch. Fixed-tree sums, decisions on broadcast scalars:
 * problem b's outputs are a function of its own operands alone, for any B, position and stream. Batch terrains,
 * per-problem bounds rows, the cross-stream scratch rule and the kept Jacobian as for
 * towr_gpu_alsolve_iterate_batch_device. TOWR_ERR_INVALID before anything runs for: what that entry refuses, a NULL
 * probe, trials outside 1..TOWR_PROBE_MAX, a NULL PSUM, ldps < 8. TOWR_ERR_UNSUPPORTED as for the L-BFGS kernels.         */
int towr_gpu_alsolve_probe_batch_device(towr_gpu_handle h, int32_t B, const towr_alsolve_params_t* params,
                                        const towr_alsolve_probe_t* probe, const towr_alsolve_state_t* state,
                                        const double* GL, const double* GU, int64_t ldgb, const double* XL,
                                        const double* XU, int64_t ldxb, double* PSUM, int64_t ldps, void* stream);

/* towr_gpu_alsolve_solve_ex_batch_device with the probe stage in front of every iteration of the method's iterate entry
 * (bit-identical to towr_gpu_alsolve_probe_batch_device and that entry with iters = 1 in sequence), for every method and
 * both compact values. PSUM is the last iteration's summary of the rows as they stood in that iteration, not state: it
 * is not exchanged by the compaction. iters_run, max_iters and check_every count probed iterations. The stop rule still
 * runs once per iteration: with acc_iters > 0 its run length counts PROBED ITERATIONS, not the sequential loop's trials,
 * so an ACCEPTABLE stop may come after fewer trials' worth of iterations than without probes. probe == NULL:
 * towr_gpu_alsolve_solve_ex_batch_device itself (PSUM and ldps are not read). TOWR_ERR_INVALID before anything runs for
 * what that entry refuses and, with a probe, for trials outside 1..TOWR_PROBE_MAX, a NULL PSUM or ldps < 8.              */
int towr_gpu_alsolve_solve_probe_batch_device(towr_gpu_handle h, int32_t B, const towr_solve_opts_t* opts,
                                              const towr_alsolve_params_t* params, const towr_alsolve_stop_t* stop,
                                              const towr_alsolve_probe_t* probe, const towr_alsolve_state_t* state,
                                              const towr_solve_dir_t* dir, double* GL, double* GU, int64_t ldgb,
                                              double* XL, double* XU, int64_t ldxb, double* PSUM, int64_t ldps,
                                              int32_t* LOG, towr_solve_report_t* report, void* stream);

/* ---- deciding a trial before its Gauss-Newton direction: the lazy GN loop ------------------------------------------------ */
/* The GN iterate entries compute the direction at the candidate XC of every problem that is not frozen, before the line
 * search has looked at the candidate; after a rejected trial nobody reads the problem's DC or GSUM row. Everything the
 * line search's accept test reads is on the device once the products chunk's residual kernel has run, so the verdict
 * stage restates that test ahead of the direction and the direction runs only where a base will be accepted. The words
 * 0 (run) and 2 (skip) make VERDICT a RUN mask with run_stride = 1 for all four direction entries.
 *
 * The verdict stage alone. Fields of `state` used: X, GR, XC, ldx, FC, SCAL, ISTATE, RSUM (ldsc, ldrs); of `params`: c1.
 * VERDICT is DEVICE memory, int32_t[B]; NDIR is DEVICE memory, int32_t[B], or NULL. Per problem b, with the phase word
 * ISTATE[4 b]:
 *   RESTART: VERDICT[b] = 0 (the line search always takes a RESTART candidate);
 *   SEARCH:  gs = sum_j GR_j (XC_j - X_j) on the line search's tree (the lane's partial in column order j = lane,
 *            lane + 256, ..., then the block's fixed tree), mc = FC[b] + RSUM[b][3], m0 = SCAL[b][0],
 *            take = gs <= 0 and mc <= m0 + c1 gs (a rounded product, then a rounded addition; a NaN anywhere makes it
 *            false): the bits and the test of towr_gpu_linesearch_batch_device on the same operands;
 *            VERDICT[b] = take ? 0 : 2;
 *   any other word (frozen, or garbage): VERDICT[b] = 2.
 * NDIR[b] += 1 when the verdict is 0. Nothing else is written: the line search behind the stage finds exactly what it
 * finds without it. Problem b's outputs are a function of its own operands alone, for any B, position and stream.
 * TOWR_ERR_INVALID before anything runs for: NULL params, state or VERDICT, an invalid params field, a NULL used field,
 * ldx < n, ldsc < 8, ldrs < 4, B < 0. TOWR_ERR_UNSUPPORTED and TOWR_ERR_NO_DEVICE as for the line search.                */
int towr_gpu_alsolve_verdict_batch_device(towr_gpu_handle h, int32_t B, const towr_alsolve_params_t* params,
                                          const towr_alsolve_state_t* state, int32_t* VERDICT, int32_t* NDIR, void* stream);

/* The lazy loop's two arrays (the struct is host memory; the pointers are DEVICE memory, int32_t[B] each; NDIR may be
 * NULL). NDIR is only ever incremented: the caller zeroes it.                                                          */
typedef struct { int32_t* VERDICT; int32_t* NDIR; } towr_alsolve_lazy_t;

/* `iters` iterations of the method's GN iterate entry (method: TOWR_SOLVE_GN, _GN_PC, _GN_DIRECT or _GN_TILED; `dir` as
 * towr_gpu_alsolve_solve_batch_device takes it) with one change inside each products chunk: behind the chunk's J^T lam+
 * product the verdict stage runs on the chunk's rows, and the chunk's direction runs with RUN = those rows of VERDICT,
 * run_stride = 1, in place of RUN = ISTATE, 4. Everything else is launch for launch that entry.
 *   After any number of iterations, for any B, batch position, products chunk, wrows and stream, every field of `state`
 *   (X, GR, XC, GRC, D, LAM, LAMP, HS, HY, HMETA, ALPHA, RHO, FC, SCAL, ISTATE, RSUM, SSUM, USUM, LSUM; DSUM is not
 *   written) is bit for bit what the method's iterate entry leaves: the select step reads DC only where the line search
 *   accepted a base, and there the verdict was 0.
 *   DC, GSUM and, with TOWR_GN_PC_JACOBI, PC (the rows the direction kernel writes): a row is that entry's bits in every
 *   iteration where the problem's verdict was 0; in an iteration where it was 2 not one byte of the row is touched. After
 *   a run a row therefore holds the direction of the last candidate that was taken.
 *   After the iteration's line search VERDICT[b] == 0 exactly when LSUM[b][0] is 1 or 2, and 2 otherwise; flag bit 0 set
 *   implies VERDICT[b] == 0. NDIR[b] grows by the number of iterations with verdict 0 and no longer changes once the
 *   problem is frozen.
 * TOWR_ERR_INVALID before anything runs for: what the method's iterate entry refuses, a NULL dir, TOWR_SOLVE_LBFGS or a
 * method outside 0..4 (L-BFGS has no direction at the candidate), a NULL lazy or lazy->VERDICT. TOWR_ERR_UNSUPPORTED and
 * TOWR_ERR_NO_DEVICE as for that entry.                                                                                */
int towr_gpu_alsolve_gn_lazy_iterate_batch_device(towr_gpu_handle h, int32_t B, int32_t iters, int32_t method,
                                                  const towr_alsolve_params_t* params, const towr_alsolve_state_t* state,
                                                  const towr_solve_dir_t* dir, const towr_alsolve_lazy_t* lazy,
                                                  const double* GL, const double* GU, int64_t ldgb, const double* XL,
                                                  const double* XU, int64_t ldxb, void* stream);

/* towr_gpu_alsolve_solve_probe_batch_device with the lazy iteration above in place of the method's iterate entry, for
 * both compact values and with or without stop and probe, which behave as there. lazy == NULL: that entry itself, launch
 * for launch. With a lazy: every array that entry's contract names — the persistent arrays, the candidate-side and
 * summary rows other than DC and GSUM, and the probe's PSUM — holds that entry's bits (PSUM[b][0] == 1, a probed length
 * passed, implies VERDICT[b] == 0 in that iteration); DC and GSUM rows follow the rule above. With compact = 1, NDIR
 * joins the exchanged per-problem arrays (one int per row; with it the state, DC, GSUM, four bounds arrays and the
 * terrains are 28 descriptors of TOWR_SWAP_MAX_ARRAYS) and is back in the caller's order at return; since it no longer
 * changes once a problem is frozen it is equal under compact = 0 and 1. VERDICT is rewritten in every iteration and is
 * not exchanged, like PSUM: it holds the last iteration's words for the rows as they stood then. TOWR_ERR_INVALID before
 * anything runs for what that entry refuses and, with a lazy, for TOWR_SOLVE_LBFGS and a NULL lazy->VERDICT. The queue
 * entry below takes neither probe nor lazy.                                                                            */
int towr_gpu_alsolve_solve_lazy_batch_device(towr_gpu_handle h, int32_t B, const towr_solve_opts_t* opts,
                                             const towr_alsolve_params_t* params, const towr_alsolve_stop_t* stop,
                                             const towr_alsolve_probe_t* probe, const towr_alsolve_state_t* state,
                                             const towr_solve_dir_t* dir, double* GL, double* GU, int64_t ldgb,
                                             double* XL, double* XU, int64_t ldxb, double* PSUM, int64_t ldps,
                                             int32_t* LOG, towr_solve_report_t* report,
                                             const towr_alsolve_lazy_t* lazy, void* stream);

/* ---- a queue of problems through the resident solve's slots: each leaves when it is done, the next takes its row ---- */
/* The retire key of a batch: which rows leave their slots. ISTATE as in towr_alsolve_state_t (only the phase word
 * ISTATE[4 b] is read; NOT WRITTEN), AGE is int32_t[B] (the iterations a row's problem has run), KEY is int32_t[4*B]
 * (ISTATE's stride; only KEY[4 b] is written); all DEVICE pointers. One thread per row:
 *   add > 0: AGE[b] += add first (add = 0: AGE is only read);
 *   KEY[4 b] = (ISTATE[4 b] is 0 or 1) and AGE[b] >= max_age ? 7 : ISTATE[4 b].
 * towr_gpu_alsolve_partition_batch_device runs on KEY as it does on ISTATE: it treats every word outside {0, 1} as
 * frozen, and 7 is counted in HEAD[7]. A key and not a phase word, so that a problem that ran out of budget keeps its
 * RESTART / SEARCH word. Integer compares only. No handle scratch; the kept Jacobian is not dropped. TOWR_ERR_INVALID
 * before anything runs for a NULL pointer, B < 0 or add < 0.                                                           */
int towr_gpu_alsolve_retire_key_batch_device(towr_gpu_handle h, int32_t B, const int32_t* ISTATE, int32_t* AGE, int32_t add,
                                             int32_t max_age, int32_t* KEY, void* stream);

/* Moves rows between slots and arrays indexed by problem: for every i < count and every pair k < n_arrays, bytes
 * [0, row_bytes) of row r0 + i of slot[k] are copied to row ID[r0 + i] of out[k]; with reverse = 1 from that row of
 * out[k] into the slot row (out[k] is then only read). ID is a DEVICE pointer (int32_t, rows r0 .. r0 + count - 1 are
 * read); a negative ID skips its row. `slot` and `out` are HOST memory, read at the call; slot[k] and out[k] state the
 * same row_bytes. Not one byte beyond row_bytes of any row is read or written. The IDs of a call must be distinct and
 * index rows every out[k] holds, and slot[k] and out[k] must not share a byte; that is the caller's business. Per side
 * the swap's rules: row_bytes a positive multiple of 4, base and ld_bytes multiples of 4, ld_bytes >= row_bytes; 8 bytes
 * move per lane where both bases, both ld_bytes and row_bytes are multiples of 8, else 4. count is a host value; count =
 * 0 or n_arrays = 0 launches nothing. No handle scratch; the kept Jacobian is not dropped. TOWR_ERR_INVALID before
 * anything runs for: NULL ID, r0 or count < 0, reverse outside {0, 1}, n_arrays outside 0..TOWR_MOVE_MAX_ARRAYS, NULL slot
 * or out with n_arrays > 0, two row_bytes that differ, and a descriptor that breaks the rules above.                  */
#define TOWR_MOVE_MAX_ARRAYS 16
int towr_gpu_alsolve_move_rows_batch_device(towr_gpu_handle h, const int32_t* ID, int32_t r0, int32_t count,
                                            int32_t n_arrays, const towr_rows_t* slot, const towr_rows_t* out,
                                            int32_t reverse, void* stream);

/* A queue of N problems for B slots (host memory, read at the call; the pointers in it are DEVICE pointers).
 *   Inputs, indexed by problem and only read: X0 (N rows of n at ldx0 >= n), the starting points; LAM0 (N rows of m at
 *   ldl0 >= m), the starting multipliers, or NULL for zeros; the bounds GL / GU (ldgb) and XL / XU (ldxb): NULL (the
 *   handle's), a leading dimension of 0 (one row shared by all problems) or > 0 (N per-problem rows). Per-problem bounds
 *   need slot-side work rows, B of each: GLW / GUW at ldgw >= m, XLW / XUW at ldxw >= n; they are not read otherwise.
 *   Slot bookkeeping: ID (int32_t[B], the problem in each slot), AGE (int32_t[B], its iterations so far), KEY
 *   (int32_t[4 B], the retire keys).
 *   Outputs, indexed by problem: X_OUT (n at ldxo >= n), LAM_OUT (m at ldlo >= m), RHO_OUT[N], SCAL_OUT[8 N],
 *   ISTATE_OUT[4 N], ITERS_OUT[N] (int32_t).                                                                          */
typedef struct {
  int32_t N, reserved;
  const double* X0; int64_t ldx0;
  const double* LAM0; int64_t ldl0;
  const double *GL, *GU; int64_t ldgb;
  const double *XL, *XU; int64_t ldxb;
  double *GLW, *GUW; int64_t ldgw;
  double *XLW, *XUW; int64_t ldxw;
  int32_t *ID, *AGE, *KEY;
  double* X_OUT; int64_t ldxo;
  double* LAM_OUT; int64_t ldlo;
  double *RHO_OUT, *SCAL_OUT;
  int32_t *ISTATE_OUT, *ITERS_OUT;
} towr_solve_queue_t;

/* Solves the N problems of `queue` through B resident slots: a problem leaves its slot when it is frozen or has run
 * max_iters iterations, and the next problem of the queue takes the freed row. `state`, dir's DC / GSUM / PC / W and the
 * work rows are sized for B as in the solve entries; their contents at entry do not matter. With K = check_every,
 * M = max_iters, `next` the queue's cursor and Bcur the live rows (both start at 0), one round, all on `stream`:
 *   1. admit: c = min(B - Bcur, N - next) problems next .. next + c - 1 into rows [Bcur, Bcur + c): X, LAM (zeros when
 *      LAM0 is NULL), the per-problem bound rows and the batch terrain are copied in by towr_gpu_alsolve_move_rows_batch_
 *      device, ID = the problem, AGE = 0; then towr_gpu_alsolve_init_batch_device's launch on exactly those rows;
 *   2. K iterations of the method's iterate entry on rows [0, Bcur), with the stop rule when `stop` is given, as
 *      towr_gpu_alsolve_solve_ex_batch_device runs them;
 *   3. towr_gpu_alsolve_retire_key_batch_device (add = K, max_age = M), towr_gpu_alsolve_partition_batch_device on KEY
 *      (HEAD = LOG[0..7], the pairs behind it) and towr_gpu_alsolve_swap_rows_batch_device with NP = LOG + 1 on that
 *      entry's arrays plus ID, AGE, the work rows and the private terrain copy;
 *   4. a copy of HEAD to page-locked host memory and ONE synchronisation: the round's only host look;
 *   5. retire: rows [na, Bcur) move out, X, LAM, RHO, SCAL (8) and ISTATE (4) to row ID of the outputs and AGE to
 *      ITERS_OUT; Bcur = na;
 *   6. the loop ends when Bcur == 0 and the queue is empty.
 * THE ENTRY BLOCKS THE HOST: once per round and once before it returns, when all its work on `stream` has finished.
 *   The contract: for every problem and every B >= 1, X_OUT, LAM_OUT, RHO_OUT, SCAL_OUT and ISTATE_OUT are bit for bit
 *   the X, LAM, RHO, SCAL and ISTATE that towr_gpu_alsolve_solve_ex_batch_device leaves for that problem with the same
 *   opts, params, stop and dir, behind towr_gpu_alsolve_init_batch_device, the N problems solved as one batch: problem
 *   b's outputs are a function of its own operands alone, so neither its slot nor its neighbours nor what an earlier
 *   tenant left in the slot can change a bit. A problem that ran out of budget keeps its RESTART / SEARCH word.
 *   ITERS_OUT = K ceil(t / K), t the iteration at which the problem froze, or M. max_iters must be a positive multiple
 *   of check_every: no problem's last round is cut short, as the solve entry's min(K, M - iters_run) schedule would.
 *   opts->compact is not read (0 or 1). No padding byte of an output is written; nothing of the inputs is written; rows
 *   beyond min(N, B) of the slot arrays are not touched. The slot state, DC, GSUM, W, PC, ID, AGE, KEY, LOG and the work
 *   rows are unspecified at return: nothing is put back in any order. When batch terrains are set
 *   (towr_gpu_set_batch_terrain) they must number exactly N; the driver keeps a private B-entry copy that travels with
 *   the rows, and the handle's set is not modified. LOG is int32_t[8 + 2 (B / 2)], DEVICE memory.
 *   `report`: rounds; iters_run = K rounds; problem_iters = the sum over the rounds of Bcur K (= the sum of ITERS_OUT;
 *   rounds >= ceil(problem_iters / (B K))); n_phase[0..5] and reserved[0..1] counted over the N rows of ISTATE_OUT as
 *   the ex entry defines them (reserved = 0 when stop is NULL). N = 0: nothing runs and the report is zero.
 *   Failure: every argument check passes before anything is queued; if a launch or copy fails, the first error is
 *   returned and the outputs of the problems not yet retired are unspecified.
 * Handle scratch, the cross-stream rule and the kept Jacobian as for the iterate entry. TOWR_ERR_INVALID before anything
 * runs for: NULL opts, dir, queue, LOG or report, a method outside 0..4, check_every < 1, max_iters not a positive
 * multiple of check_every, compact outside {0, 1}, N < 0, B < 1 with N > 0, with N > 0 (an empty queue names no array)
 * a NULL X0, ID, AGE, KEY or output, ldx0 or ldxo < n, ldl0 (LAM0 given) or ldlo < m, only one of GL / GU or of XL / XU, a leading dimension of the bounds that is
 * negative or in (0, m) / (0, n), per-problem bounds without their work rows or with ldgw < m / ldxw < n, everything the
 * method's iterate entry refuses for B rows, more per-problem arrays than TOWR_SWAP_MAX_ARRAYS, an array that fails the
 * swap's or the move's checks, and batch terrains set for another number of problems than N. TOWR_ERR_UNSUPPORTED and
 * TOWR_ERR_NO_DEVICE as for that iterate entry, behind all of these.                                                  */
int towr_gpu_alsolve_solve_queue_batch_device(towr_gpu_handle h, int32_t B, const towr_solve_opts_t* opts,
                                              const towr_alsolve_params_t* params, const towr_alsolve_stop_t* stop,
                                              const towr_alsolve_state_t* state, const towr_solve_dir_t* dir,
                                              const towr_solve_queue_t* queue, int32_t* LOG, towr_solve_report_t* report,
                                              void* stream);

/* Launch classes and launches, for roofline accounting. Kernel indices 0..4 are the launch
 * classes: Dynamic, RangeOfMotion, ForceConstraintDiscretized, TorqueConstraintDiscretized and the
 * small kinds (node-value constraints, SplineAcc, BaseMotion, TotalDuration, ...), one kernel each.
 * Indices 5..towr_gpu_num_kernels()-1 are the handle's fusion groups: classes that a step launches
 * together in one kernel (default RangeOfMotion + ForceConstraintDiscretized; environment variable
 * TOWR_GPU_FUSE at handle creation). towr_gpu_kernel_info gives a kernel's name, tiles (or units)
 * per problem (0 = not used by this handle) and algorithmic bytes per problem (CSR values and g rows
 * written + distinct x entries read); towr_gpu_eval_batch_device_kernel launches that kernel alone.
 * towr_gpu_step_launches lists the kernels one evaluation launches (returns their count).       */
int towr_gpu_kernel_info(towr_gpu_handle h, int32_t kernel, const char** name, int32_t* n_tiles,
                         int64_t* bytes_per_problem);
int towr_gpu_eval_batch_device_kernel(towr_gpu_handle h, int32_t kernel, int32_t B,
                                      const double* X, int64_t ldx, double* G, int64_t ldg,
                                      double* V, int64_t ldv, void* stream);
int towr_gpu_num_kernels(void);
int towr_gpu_step_launches(towr_gpu_handle h, int32_t* kernels, int32_t cap);
/* The implementation launch class `kernel` (0..4) uses on this handle: 0 = tile kernel, 1 = record +
 * stream kernels (every CSR unit composed and written once; phase-duration optimisation), -1 = the
 * class is not used. Introspection for tests and profiling.                                      */
int towr_gpu_kernel_path(towr_gpu_handle h, int32_t kernel);

/* Sets the launch geometry (tiles per workgroup); 0 = automatic. For benchmarking.              */
int towr_gpu_set_tiles_per_block(towr_gpu_handle h, int32_t tiles_per_block);

/* Per-launch algorithmic byte count used for the roofline: 8*(n + m + nnz) + terrain bytes.     */
int64_t towr_gpu_algorithmic_bytes_per_call(towr_gpu_handle h);

#ifdef __cplusplus
}
#endif

#endif /* TOWR_GPU_H_ */
