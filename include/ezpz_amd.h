/*
 * ezpz_amd.h -- C ABI of the MI355X-native ezpz constraint-solve path.
 *
 * This is the drop-in boundary for ONE path of KittyCAD/ezpz: the Newton / Levenberg-Marquardt
 * constraint-solve loop.  The reference has no FFI seam of its own (it is a pure-Rust crate); the
 * seam is the public function `ezpz::solve` and, inside it, `solve_inner` -> `Model::new` +
 * `Model::solve_levenberg_marquardt`.  Each entry point below names the reference interface it
 * replaces (paths relative to the reference checkout).  A Rust shim binding these symbols is
 * shown in INTEGRATION.md.
 *
 * Conventions: plain pointers and sizes, caller owns every buffer, nothing throws, return value is
 * 0 (EZPZ_OK) or a negative EzpzError that mirrors `NonLinearSystemError` (ezpz/src/error.rs:35-86).
 * All arithmetic is IEEE fp64.  The library needs a HIP device (gfx950); without one every solve
 * entry point returns EZPZ_ERR_NO_DEVICE -- there is no CPU fallback.
 */
#ifndef EZPZ_AMD_H
#define EZPZ_AMD_H

#ifndef __HIPCC_RTC__
#include <stddef.h>
#include <stdint.h>
#else /* run-time compilation of the device kernels (hiprtc has no system headers) */
typedef unsigned char uint8_t;
typedef unsigned short uint16_t;
typedef unsigned int uint32_t;
typedef unsigned long long uint64_t;
typedef int int32_t;
typedef long long int64_t;
typedef unsigned long long uintptr_t;
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Constraint, ezpz/src/constraints.rs:37-93 (kind = enum declaration order) ------------------ */
enum EzpzKind {
    EZPZ_LINE_TANGENT_TO_CIRCLE = 0,          /* ids: line p0.x p0.y p1.x p1.y, circle c.x c.y radius; tag = EzpzLineSide */
    EZPZ_CIRCLE_TANGENT_TO_CIRCLE = 1,        /* ids: a.cx a.cy a.r b.cx b.cy b.r; tag = EzpzCircleSide */
    EZPZ_DISTANCE = 2,                        /* ids: p0 p1; param = distance */
    EZPZ_DISTANCE_VAR = 3,                    /* ids: p q D */
    EZPZ_VERTICAL_DISTANCE = 4,               /* ids: p0 p1; param */
    EZPZ_HORIZONTAL_DISTANCE = 5,             /* ids: p0 p1; param */
    EZPZ_VERTICAL = 6,                        /* ids: line */
    EZPZ_HORIZONTAL = 7,                      /* ids: line */
    EZPZ_LINES_AT_ANGLE = 8,                  /* ids: line0 line1; tag = EzpzAngleKind; param = angle value */
    EZPZ_FIXED = 9,                           /* ids: var; param = value */
    EZPZ_SCALAR_EQUAL = 10,                   /* ids: a b */
    EZPZ_POINTS_COINCIDENT = 11,              /* ids: p0 p1 */
    EZPZ_CIRCLE_RADIUS = 12,                  /* ids: c.x c.y radius; param */
    EZPZ_LINES_EQUAL_LENGTH = 13,             /* ids: line0 line1 */
    EZPZ_ARC_RADIUS = 14,                     /* ids: arc; param */
    EZPZ_ARC = 15,                            /* ids: arc */
    EZPZ_MIDPOINT = 16,                       /* ids: line, point */
    EZPZ_POINT_LINE_DISTANCE = 17,            /* ids: point, line; param */
    EZPZ_VERTICAL_POINT_LINE_DISTANCE = 18,   /* ids: point, line; param */
    EZPZ_HORIZONTAL_POINT_LINE_DISTANCE = 19, /* ids: point, line; param */
    EZPZ_SYMMETRIC = 20,                      /* ids: line, a, b */
    EZPZ_POINT_ARC_COINCIDENT = 21,           /* ids: arc, point */
    EZPZ_ARC_LENGTH = 22,                     /* ids: arc; param */
    EZPZ_ARC_ANGLE = 23,                      /* ids: arc; tag = EZPZ_ANGLE_OTHER_DEG/RAD; param */
    EZPZ_POINTS_AT_ANGLE = 24,                /* ids: p0 p1 p2; tag = EzpzAngleKind; param */
    EZPZ_NUM_KINDS = 25
};
/* datum id order: point = x,y; line = p0,p1; circle = center,radius; arc = center,start,end
 * (struct field order of ezpz/src/datatypes/inputs.rs). */

enum EzpzLineSide { EZPZ_SIDE_UNDEFINED = 0, EZPZ_LINE_LEFT = 1, EZPZ_LINE_RIGHT = 2 };   /* constraints.rs:109-116 */
enum EzpzCircleSide { EZPZ_CIRCLE_EXTERIOR = 1, EZPZ_CIRCLE_INTERIOR = 2 };             /* constraints.rs:122-129 */
enum EzpzAngleKind {                                                                     /* datatypes.rs:9-29 */
    EZPZ_ANGLE_PARALLEL = 0,
    EZPZ_ANGLE_PERPENDICULAR = 1,
    EZPZ_ANGLE_OTHER_DEG = 2,
    EZPZ_ANGLE_OTHER_RAD = 3
};

/* ConstraintRequest {constraint, priority, weight}, ezpz/src/constraint_request.rs.  56 bytes. */
typedef struct EzpzConstraint {
    uint16_t kind; /* EzpzKind */
    uint8_t tag;
    uint8_t flags; /* reserved, 0 */
    uint32_t priority;
    uint32_t ids[8];
    double param;
    double weight;
} EzpzConstraint;

/* Config, ezpz/src/solver.rs:31-81 */
typedef struct EzpzConfig {
    uint64_t max_iterations;   /* default 35 */
    double residual_tolerance; /* default 1e-8 */
    double step_tolerance;     /* default 1e-12 */
    double initial_lambda;     /* default 1e-9 */
} EzpzConfig;

/* NonLinearSystemError, ezpz/src/error.rs:35-86 (+ library conditions <= -100) */
enum EzpzError {
    EZPZ_OK = 0,
    EZPZ_ERR_NOT_FOUND = -1,
    EZPZ_ERR_WRONG_NUMBER_GUESSES = -2,
    EZPZ_ERR_MISSING_GUESS = -3,
    EZPZ_ERR_MATRIX = -4, /* FaerMatrix: a variable id outside [0, n_vars) */
    EZPZ_ERR_EMPTY_SYSTEM = -8,
    EZPZ_ERR_NO_DEVICE = -100,
    EZPZ_ERR_HIP = -101,
    EZPZ_ERR_TOO_LARGE = -102,
    EZPZ_ERR_INVALID_ARGUMENT = -103,
    EZPZ_ERR_KERNEL_BUDGET = -104,   /* ezpz_system_specialize: the process already holds its 512 specialised kernels */
    EZPZ_ERR_PARSE = -110,           /* textual front end: winnow parse failure */
    EZPZ_ERR_TEXT_MISSING_GUESS = -111,  /* TextualError, error.rs:10-33 */
    EZPZ_ERR_TEXT_UNUSED_GUESSES = -112,
    EZPZ_ERR_TEXT_UNDEFINED_POINT = -113
};

/* Warning / WarningContent, ezpz/src/warnings.rs:8-32 */
enum EzpzWarningContent { EZPZ_WARN_DEGENERATE = 0, EZPZ_WARN_SHOULD_BE_PARALLEL = 1, EZPZ_WARN_SHOULD_BE_PERPENDICULAR = 2 };
typedef struct EzpzWarning {
    int32_t about_constraint;
    int32_t content;
} EzpzWarning;

/* Per-system result of the device LM loop: SuccessfulSolve (solver/newton.rs:18-24) plus what
 * solve_inner derives (lib.rs:305-327).  32 bytes. */
#define EZPZ_ITERATIONS_TEAM_TIMEOUT 0xFFFFFFFFu /* EzpzStatus.iterations: see ezpz_system_solve_batch_device */
typedef struct EzpzStatus {
    uint32_t iterations;
    uint32_t converged;
    uint32_t n_unsatisfied;
    uint32_t n_warnings;       /* Degenerate warnings the model produced (every evaluation, no dedup) */
    double final_residual_inf; /* max |weighted r| at exit */
    double final_lambda;
} EzpzStatus;

/* SolveOutcome (solve_outcome.rs:12-26) / FailureOutcome (:126-136) in flat form. */
typedef struct EzpzOutcome {
    int32_t error; /* EzpzError; != 0 => FailureOutcome */
    int32_t err_constraint_id;
    int64_t err_variable;
    uint64_t iterations;
    int32_t converged;
    uint32_t priority_solved;
    uint64_t n_unsatisfied;
    uint64_t n_warnings;
    uint64_t num_vars;
    uint64_t num_eqs;
    double final_lambda;
    double final_residual_inf;
} EzpzOutcome;

/* Sizes of one analysed topology (host symbolic phase), for roofline accounting. */
typedef struct EzpzSystemInfo {
    uint64_t n_constraints, n_vars, n_rows;
    uint64_t nnz_j;  /* zJ */
    uint64_t nnz_a;  /* zA: nnz(lower(JtJ + lambda I)) */
    uint64_t nnz_l;  /* zL: nnz(L) incl. diagonal */
    uint64_t n_levels;      /* elimination-tree height */
    uint64_t n_components;  /* connected components of the variable graph */
    uint64_t program_bytes; /* device-resident topology program */
    uint64_t workspace_bytes; /* per-system LDS / global workspace */
    uint32_t team_size;     /* lanes cooperating on one system */
    uint32_t workspace_in_lds;
    uint32_t team_mode;     /* 0 sub-wavefront teams, 1 wavefront-partitioned workgroup, 2 barrier workgroup,
                             * 3 component-resident (one lane per connected component; n_partitions = chunks of <= 64
                             * components of one isomorphism class), 4 barrier workgroup whose linear solve is a record
                             * walk (one connected sketch, or a system of up to 127 components: the automatic shapes),
                             * 5 frontal: a tree of dense fronts, one wavefront per front (grid_workgroups = workgroups that
                             * share one system, n_partitions = fronts, n_levels = levels of the tree per workgroup) */
    uint32_t n_partitions;  /* partitions (balanced unions of components), one per wavefront in mode 1 */
    uint32_t program_in_lds;
    uint32_t grid_workgroups; /* workgroups that share one system (grid team: one large system on many CUs), else 1 */
    /* A system created for batches (team_size 0) of one connected sketch also carries the frontal plan (team_mode 5's) and
     * takes it for calls of at most front_max_batch systems -- calls too small to fill the device with one workgroup per
     * system; the fields above then describe the shape of its larger calls.  front_workgroups = workgroups that share one
     * system on that plan (0: no such plan); 0xFFFFFFFF in front_max_batch: every call (the latency shapes). */
    uint32_t front_workgroups, front_max_batch;
} EzpzSystemInfo;

typedef struct EzpzSystem EzpzSystem; /* opaque: one analysed topology, resident on one device */

void ezpz_default_config(EzpzConfig* cfg); /* Config::default(), solver.rs:72-81 */
int ezpz_device_count(void);
/* The calling thread's current HIP device, or -1 without one.  ezpz_solve* keep their cached systems on it. */
int ezpz_current_device(void);
const char* ezpz_error_string(int err);

/* ---- symbolic phase ------------------------------------------------------------------------------
 * Replaces Model::new (ezpz/src/solver.rs:192-300): validate_variables (:142-189), row numbering,
 * Jacobian sparsity, and the symbolic Cholesky of JtJ + lambda I that faer's SymbolicLlt does there.
 * `cs` is one priority tier, already side-resolved, in request order; ids index the value vector
 * directly (Layout::index_of, solver.rs:107-109).  On MissingGuess, err_constraint/err_variable
 * receive the offending position in `cs` and the id.  `team_size` 0 = choose automatically for batch
 * throughput; EZPZ_TEAM_AUTO_LATENCY = choose automatically for the latency of one solve (what ezpz_solve does:
 * a connected sketch of a few hundred variables then runs on a 256-512 lane workgroup with its lists staged in LDS
 * instead of one wavefront / a lean 128-lane workgroup: ~35 % sooner per solve at less than half the batch rate). */
#define EZPZ_TEAM_AUTO_LATENCY 0xFFFFFFFFu
/* automatic choice among the list-walk shapes only (team_mode 0-2, dense phases included): never the component-resident
 * shape, one lane per system or the record walk (A/B runs and tests) */
#define EZPZ_TEAM_AUTO_LISTS 0xFFFFFFFEu
/* automatic, and a connected sketch of more than 20 variables runs one lane per system (lanes across the batch) at every
 * batch size instead of from 64 x 2 x CUs systems per call (A/B runs and tests) */
#define EZPZ_TEAM_BATCH_LANES 0xFFFFFFFDu
/* EZPZ_TEAM_AUTO_LATENCY without the record walk (team_mode 4): one connected sketch then ends its elimination with
 * dense phases on the barrier workgroup (team_mode 2), as every latency shape did before round 3 (A/B runs and tests) */
#define EZPZ_TEAM_LATENCY_PHASES 0xFFFFFFFCu
/* EZPZ_TEAM_AUTO_LATENCY, and a small system (<= 20 variables) runs one solve on one WAVEFRONT per system -- constraint
 * sweeps and the assembly of the normal equations across its lanes, the lane kernel's arithmetic operation for operation
 * -- whenever that form exists; EZPZ_TEAM_AUTO_LATENCY itself takes it only where it pays (>= 8 variables and >= 3
 * constraints of the non-linear kinds: `square` 47 -> 40 us of kernel, `two rectangles dependent` 63 -> 53; a 4-variable
 * linear system loses 12 -> 16) (A/B runs and tests) */
#define EZPZ_TEAM_LATENCY_WAVE 0xFFFFFFFBu
/* the FRONTAL shape (team_mode 5: multifrontal supernodal Cholesky on dense fronts, csrc/fronts.cpp) whatever the size of the
 * system, with the automatic latency shape behind it where the shape does not apply (a front of more than 63 rows ...);
 * EZPZ_TEAM_AUTO_LATENCY takes it from a size on its own (EzpzLaunchPolicy.front_min_vars_one_solve) */
#define EZPZ_TEAM_FRONTS 0xFFFFFFFAu
/* EZPZ_TEAM_AUTO_LATENCY without the frontal shape: one connected sketch then walks records (team_mode 4), as every latency
 * shape did before round 5 (A/B runs and tests) */
#define EZPZ_TEAM_LATENCY_RECORDS 0xFFFFFFF9u
int ezpz_system_create(const EzpzConstraint* cs, size_t n_cs, size_t n_vars, int device, uint32_t team_size,
                       EzpzSystem** out, int32_t* err_constraint, int64_t* err_variable);
void ezpz_system_destroy(EzpzSystem* sys);
int ezpz_system_info(const EzpzSystem* sys, EzpzSystemInfo* info);

/* Host-only analysis (no device needed): the same symbolic phase, sizes only. */
int ezpz_analyze(const EzpzConstraint* cs, size_t n_cs, size_t n_vars, EzpzSystemInfo* info, int32_t* err_constraint,
                 int64_t* err_variable);

/* ---- evaluation only (kernel K1 of the design: residual + Jacobian sweep) -----------------------------
 * Replaces Model::residual + Model::refresh_jacobian (ezpz/src/solver.rs:318-440) for `batch` value
 * vectors: r_out [batch][n_rows] weighted residuals, jv_out [batch][nnz_j] weighted Jacobian values in
 * slot order; ezpz_system_jacobian_pattern gives the (row, col) of every slot.  Host pointers. */
int ezpz_system_eval_batch(EzpzSystem* sys, const double* x, size_t batch, double* r_out, double* jv_out,
                           uint32_t* degenerate_count_out);
int ezpz_system_jacobian_pattern(const EzpzSystem* sys, uint32_t* rows, uint32_t* cols);

/* ---- residual field (ezpz/src/residual_viz.rs, feature `residual-viz`) -----------------------------------
 * The residual magnitude as a 2-D scalar field while two variables of the system sweep a viewport: pixel (px, py) of a
 * width x height image is the point x = x_min + (x_max - x_min) * (px + 0.5) / width, likewise y (residual_viz.rs:58-62;
 * row 0 = y_min), put into variables var_x / var_y of the value vector x_base (n_vars values, caller's numbering).
 * `constraint` is a position in the system's constraint list -- the magnitude is then the absolute value of its residual,
 * or sqrt(r0*r0 + r1*r1) for a kind of two rows (:240, :294) -- or -1 for all constraints: sqrt of the sum of squares, the
 * constraints that use a swept variable summed per pixel in list order onto the sum of all others at x_base, which is
 * computed once per call.  Residuals are unweighted, as the reference draws them; a degenerate guard leaves 0 and the
 * pixel is counted in degenerate_pixels_out (optional; with -1 a guard among the constraints no pixel changes counts
 * every pixel).  Outputs, at least one of them: mag_out [height][width] doubles, rgb_out [height][width][3] bytes of the
 * reference's colour map (:72-81, the function of ezpz_residual_colormap).  The _device form takes device pointers and only
 * enqueues on `stream`; both keep their list of constraints in scratch memory of the EzpzSystem: calls on one system
 * must not overlap in time.  The vector stores need width % 4 == 0, mag on 16 bytes and rgb on 4; anything else is
 * stored pixel by pixel, same values.
 * ezpz_residual_colormap and ezpz_residual_overlay run on the host and need no device: the colour of n magnitudes, and
 * draw_solver_overlay (:186-200) on an rgb image of the viewport's size -- an arrow over half the way from the example point
 * to the solution, a red disc at the example, a green one at the solution. */
typedef struct EzpzViewport {
    double x_min, x_max, y_min, y_max;
    uint32_t width, height;
} EzpzViewport;
int ezpz_system_residual_field(EzpzSystem* sys, const double* x_base, uint32_t var_x, uint32_t var_y, int64_t constraint,
                               const EzpzViewport* viewport, double* mag_out, uint8_t* rgb_out,
                               uint64_t* degenerate_pixels_out);
int ezpz_system_residual_field_device(EzpzSystem* sys, const double* x_base_dev, uint32_t var_x, uint32_t var_y,
                                      int64_t constraint, const EzpzViewport* viewport, double* mag_dev, uint8_t* rgb_dev,
                                      uint64_t* degenerate_pixels_dev, void* stream);
void ezpz_residual_colormap(const double* mag, size_t n, uint8_t* rgb);
int ezpz_residual_overlay(uint8_t* rgb, const EzpzViewport* viewport, double example_x, double example_y,
                          double solution_x, double solution_y);

/* ---- numeric phase -------------------------------------------------------------------------------
 * Replaces Model::solve_levenberg_marquardt (ezpz/src/solver/newton.rs:29-145) followed by the
 * unsatisfied check of solve_inner (ezpz/src/lib.rs:305-327), for `batch` independent systems that
 * share the analysed topology.  x0 / x_out are AoS [batch][n_vars] and may alias -- but a block system of linear constraints
 * with unit weights (massive_parallel_system) is solved ~20 % faster when they do not overlap: its kernel stores a system's
 * values before the verdicts of the LM control are in and re-solves the few systems whose verdicts are not the expected ones
 * from x0 (csrc/jit_kernel.hip.hpp: solve_kernel_fast); with overlapping buffers the loop kernel serves, same results.
 * unsat_mask is optional ([batch][n_cs] bytes, 1 = unsatisfied, indexed by position in `cs`); warn_log is optional
 * ([batch][warn_cap] entries (pass << 32 | position), chronological once sorted).
 * Which kernel serves a call may depend on the call's size (EzpzSystemInfo.front_max_batch: small calls of a connected
 * sketch take the frontal elimination order, larger ones the record walk or the lanes): integer and flag outputs are the
 * reference's either way, coordinates of connected sketches agree to rounding (1e-6 relative on determined coordinates), not
 * bit for bit across call sizes -- a caller who chunks a batch itself and needs identical bits per chunk size creates the system
 * with one shape (team_size: EZPZ_TEAM_*).  Block systems are bitwise the same on every path.
 * The _device form takes device pointers and only enqueues on `stream` (a hipStream_t; NULL = default);
 * the host form copies in, runs, copies out and synchronises.  Launches on one EzpzSystem must not overlap in time
 * when the system uses per-system device scratch (a global workspace or a grid team, see EzpzSystemInfo): enqueue
 * them on one stream, or create one EzpzSystem per stream.
 * Thread safety: the _device form may be called on one EzpzSystem from several threads at once (each enqueueing on its
 * own stream; what a launch creates on first use is created under a lock); the host form serialises its callers per
 * EzpzSystem; ezpz_solve* may be called from any number of threads.
 * Grid teams (EzpzSystemInfo.grid_workgroups > 1) need all their workgroups resident at once; launches are sized to
 * the device's CU count, and should a rendezvous still time out (~1 s: another process occupying the device) the
 * affected systems report iterations == EZPZ_ITERATIONS_TEAM_TIMEOUT, converged == 0 instead of hanging; the host
 * form returns EZPZ_ERR_HIP in that case and the EzpzSystem must be destroyed. */
/* Host buffers a caller reuses across batch calls can be page-locked once (hipHostRegister underneath): when both x0
 * and x_out of an ezpz_system_solve_batch call lie inside registered ranges (and no mask / warning log is asked for) the
 * call streams the batch through three device slots, so that the PCIe copy in, the kernels and the copy out overlap.
 * The caller must unregister a range before freeing it. */
int ezpz_host_register(void* p, size_t bytes);
int ezpz_host_unregister(void* p);

int ezpz_system_solve_batch_device(EzpzSystem* sys, const double* x0_dev, size_t batch, const EzpzConfig* cfg,
                                   double* x_out_dev, EzpzStatus* status_dev, uint8_t* unsat_mask_dev,
                                   uint64_t* warn_log_dev, uint32_t warn_cap, void* stream);
int ezpz_system_solve_batch(EzpzSystem* sys, const double* x0, size_t batch, const EzpzConfig* cfg, double* x_out,
                            EzpzStatus* status, uint8_t* unsat_mask, uint64_t* warn_log, uint32_t warn_cap);

/* ---- batches with per-system constraint parameters (new: driven dimensions -- one sketch, many dimension sets) ------------
 * ezpz_system_solve_batch[_device] with the parameters of some constraints taken per system instead of from the `cs` the
 * system was created with: `positions` (host memory, n_param of them, distinct, any order) are positions in that `cs`, and
 * params[b][j] (AoS [batch][n_param]) replaces cs[positions[j]].param for system b -- in the units of that field: degrees for
 * an angle tagged EZPZ_ANGLE_OTHER_DEG.  A constraint that is not listed keeps its value.  System b gets exactly what
 * ezpz_system_solve_batch[_device] gives on a system created from `cs` with those parameters substituted: values, EzpzStatus,
 * unsatisfied mask, warning log (block systems bit for bit; other systems bit for bit what that system's list-walk teams of
 * the same team_size give).  n_param == 0 is the plain entry.  Only finite parameters are supported.
 * ezpz_constraint_has_param (host only, no device): 1 where the residual of the constraint's kind and tag reads `param` -- the
 * ten kinds documented with "param" above, and the three angle kinds unless tagged parallel or perpendicular -- else 0.
 * EZPZ_ERR_INVALID_ARGUMENT, with nothing enqueued and no output touched: a position >= n_cs, a position listed twice, a
 * position whose constraint has no parameter, n_param > 0 with positions or params NULL -- and a system that one solve spreads
 * over several workgroups (EzpzSystemInfo.grid_workgroups > 1 of its list-walk shape), which this entry declines.
 * The entry has its own route: the component interpreter for block systems, else the list-walk teams; never the run-time
 * compiled kernels (a specialised system is served all the same) or the lanes across the batch -- and the fronts only where
 * the caller asks for them:
 * ezpz_system_set_params_route(sys, EZPZ_PARAMS_ROUTE_FRONTS) makes this entry and the sweeps below run on the FRONTAL shape
 * (team_mode 5) of a system whose frontal plan serves every call (EzpzSystemInfo.front_max_batch == 0xFFFFFFFF: created with
 * EZPZ_TEAM_FRONTS, or with EZPZ_TEAM_AUTO_LATENCY where the planner took the fronts); every other system -- a system created
 * for batches that takes the fronts for its small calls included -- gets EZPZ_ERR_INVALID_ARGUMENT and keeps its route.  On
 * that route system b gets exactly, bit for bit, what ezpz_system_solve_batch gives on a system created with the same team_size
 * from `cs` with those parameters substituted (values, EzpzStatus, mask, warning log), on one workgroup per system or several:
 * the decline of grid_workgroups > 1 above is the list-walk route's alone.  A launch on several workgroups refuses a stream that
 * is being captured (EZPZ_ERR_INVALID_ARGUMENT, nothing enqueued), as the plain entry does.  EZPZ_PARAMS_ROUTE_DEFAULT restores
 * the route described above; it is what every system starts with.  The setter waits for the system's launches of both entries.
 * Thread safety and the aliasing of x0 / x_out: as for ezpz_system_solve_batch_device; launches of this entry on one
 * EzpzSystem run one behind the other whatever streams they were enqueued on.  The _device form only enqueues on
 * `stream`, except that a `positions` list other than the system's last one is turned into its device table first: the call then
 * waits for the system's earlier launches of this entry and copies synchronously (repeat the list, and calls only enqueue). */
#define EZPZ_PARAMS_ROUTE_DEFAULT 0u
#define EZPZ_PARAMS_ROUTE_FRONTS 1u
int ezpz_system_set_params_route(EzpzSystem* sys, uint32_t route);
int ezpz_constraint_has_param(const EzpzConstraint* c);
int ezpz_system_solve_batch_params_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                          const double* params_dev, size_t batch, const EzpzConfig* cfg, double* x_out_dev,
                                          EzpzStatus* status_dev, uint8_t* unsat_mask_dev, uint64_t* warn_log_dev,
                                          uint32_t warn_cap, void* stream);
int ezpz_system_solve_batch_params(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param,
                                   const double* params, size_t batch, const EzpzConfig* cfg, double* x_out, EzpzStatus* status,
                                   uint8_t* unsat_mask, uint64_t* warn_log, uint32_t warn_cap);

/* ---- dimension sweeps: a chain of driven solves per system in one launch -------------------------------------
 * `batch` sweeps of `steps` solves each on one topology: step k of sweep b takes params[k][b][:] for the constraints at
 * `positions` and starts from step k - 1's answer; step 0 starts from x0[b] -- a dragged point, a swept length, an animated linkage
 * staying on its solution branch.  Every per-step array is STEP-MAJOR:
 *     params[steps][batch][n_param]   x_out[steps][batch][n_vars]   status[steps][batch]
 *     unsat_mask[steps][batch][n_cs]  warn_log[steps][batch][warn_cap]            x0[batch][n_vars]
 * so that step k of the whole batch is one contiguous batch in the layout of ezpz_system_solve_batch_params, and the sweep is BY
 * DEFINITION this chain of calls of that entry:
 *     step 0:  solve_batch_params(x0,           params[0]) -> x_out[0], status[0], unsat_mask[0], warn_log[0]
 *     step k:  solve_batch_params(x_out[k - 1], params[k]) -> x_out[k], status[k], unsat_mask[k], warn_log[k]
 * System b at step k gets the values, EzpzStatus, mask and warning log that chain gives, bit for bit, on every route the params
 * entry has.  A step that does not converge changes nothing about the chain: the next step starts from whatever it left (holding
 * the last good answer is the caller's business).  steps == 1 is the params entry, same bits.  steps == 0 or batch == 0: EZPZ_OK,
 * nothing written.  n_param == 0 is legal: `steps` re-solves with the system's own values, each from the one before (the plain
 * entry's, as a chain of launches).
 * EZPZ_ERR_INVALID_ARGUMENT, with nothing enqueued and no output touched: the argument errors of the params entry (a position
 * >= n_cs, listed twice, or whose constraint has no parameter; positions or params NULL with n_param > 0; x_out, status or x0 NULL
 * with work to do) -- and a system that one solve spreads over several workgroups (EzpzSystemInfo.grid_workgroups > 1 of its
 * list-walk shape), which this entry declines like the params entry unless the system's params route is the fronts
 * (ezpz_system_set_params_route: the sweep is then bit for bit the chain of params calls on that route).  Sweeps through ezpz_multi_* and ezpz_mixed_* do not exist.
 * Aliasing: x0 may be exactly x_out (step 0's block), as with the plain entry; any other overlap among the arrays is the caller's
 * error, and the result then undefined.
 * The _device form only enqueues on `stream` -- one launch where the plan says in_kernel, else the chain of `steps` launches --
 * with the params entry's exception: a `positions` list other than the system's last one (of this entry or the params entry, they
 * share the table) is turned into its device table first.  Sweeps and params calls on one EzpzSystem run one behind the other
 * whatever their streams.  The host form stages through the system's buffers, sized steps x batch.
 * ezpz_system_sweep_params_plan (host only): the route a sweep of this list takes and whether it is one launch.  DIAGNOSTIC, like
 * EzpzSensitivityPlan: it follows the kernels and is not part of the stable surface. */
#define EZPZ_SWEEP_INTERPRETER 0u           /* block system: the component interpreter */
#define EZPZ_SWEEP_SUB_WAVEFRONT_TEAMS 1u   /* list-walk teams of 1 .. 64 lanes */
#define EZPZ_SWEEP_PARTITIONED_WORKGROUP 2u /* one workgroup per sweep, a partition per wavefront */
#define EZPZ_SWEEP_BARRIER_WORKGROUP 3u     /* one workgroup per sweep on one partition (workspace in LDS or global memory) */
#define EZPZ_SWEEP_RECORD_WALK 4u           /* ... whose linear solve is a record walk */
/* ... the five routes the entry chooses among by itself; and the one a caller opts into (ezpz_system_set_params_route): the
 * frontal shape, a sweep per slot of its workgroups -- route 5 */
#define EZPZ_SWEEP_FRONTS (EZPZ_SWEEP_RECORD_WALK + 1u)
typedef struct EzpzSweepPlan {
    uint32_t route;         /* EZPZ_SWEEP_* */
    uint32_t in_kernel;     /* 1: one launch, the values never leave the team's workspace; 0: the chain of `steps` launches */
    uint32_t params_in_lds; /* list-walk routes and the fronts: a team stages its step's driven values in LDS */
    uint32_t lds_bytes;     /* dynamic LDS per workgroup of the launch */
} EzpzSweepPlan;
int ezpz_system_sweep_params_plan(EzpzSystem* sys, const uint32_t* positions, size_t n_param, EzpzSweepPlan* out);
int ezpz_system_sweep_params_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                    const double* params_dev, size_t steps, size_t batch, const EzpzConfig* cfg, double* x_out_dev,
                                    EzpzStatus* status_dev, uint8_t* unsat_mask_dev, uint64_t* warn_log_dev, uint32_t warn_cap,
                                    void* stream);
int ezpz_system_sweep_params(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const double* params,
                             size_t steps, size_t batch, const EzpzConfig* cfg, double* x_out, EzpzStatus* status,
                             uint8_t* unsat_mask, uint64_t* warn_log, uint32_t warn_cap);

/* ---- guarded sweeps: the sweep with step control where the values live ---------------------------------------
 * ezpz_system_sweep_params is policy-free; this entry carries one policy: a step that fails, lands on another configuration or
 * moves too far is cut in half and tried again, and a sweep never leaves its last accepted answer.  Sweep b carries the state
 * (x_s, p_s): the last accepted values and the driven values they were solved at; it starts as (x0[b], params0[b]) -- params0
 * [batch][n_param] is required: the system's own values of the driven constraints, or params_reached of an earlier call.  Step k
 * has the target p_b = params[k][b] and is BY DEFINITION:
 *     p_a = p_s; t = 0; h = 1; attempts = 0; accepted = 0
 *     while t < 1 and attempts < max_attempts:
 *         u = t + h                                                    (dyadic, exact)
 *         p_u[j] = p_b[j] if u == 1, else p_a[j] + u * (p_b[j] - p_a[j])   (three operations, each rounded by itself)
 *         (x, status, mask, log) = ezpz_system_solve_batch_params' solve of this system from x_s with p_u      (bit for bit)
 *         attempts += 1
 *         accept iff status.converged == 1 and status.n_unsatisfied == 0
 *                    and (max_move <= 0 or |x[i] - x_s[i]| <= max_move for every i)                        (a NaN rejects)
 *         if accept: x_s = x; p_s = p_u; t = u; accepted += 1
 *         else:      h /= 2; if h < 2^-max_halvings: break
 *     x_out[k][b] = x_s; params_reached[k][b] = p_s; guard[k][b] = {reached = t, attempts, accepted}
 *     status[k][b], unsat_mask[k][b], warn_log[k][b] = those of the LAST attempt, accepted or not
 * h starts at 1 again at every step and never grows within one; a step that stops short leaves (x_s, p_s) where they are and the
 * next step tries to catch up from there.  The state across steps is (x_s, p_s) alone: a sweep of 2K steps equals a sweep of K
 * steps and a second one of K steps from (x_out[K - 1], params_reached[K - 1]).  max_halvings == 0 with max_move == 0 is the plain
 * sweep that holds the last good answer.  Layouts are the sweep's (step-major), with guard[steps][batch] and
 * params_reached[steps][batch][n_param]; of a row of warn_log the first min(status.n_warnings, warn_cap) entries are the last
 * attempt's, the others unspecified.  x0 must not overlap x_out (a later step may read it again).
 * EZPZ_ERR_INVALID_ARGUMENT, with nothing enqueued and no output touched: the argument errors of the sweep entry; n_param == 0; a
 * NULL params0, guard or params_reached with work to do; a guard configuration out of range (max_halvings > 20, max_attempts == 0,
 * a max_move that is not finite).  guard_cfg == NULL: ezpz_default_guard_config's values -- policy defaults, not measurements.
 * The _device form runs in ONE launch -- the team that owns a sweep forms p_u, judges the attempt and gathers the last accepted
 * values again after a reject -- on the sub-wavefront teams, the barrier workgroup (workspace in LDS or in global memory) and the
 * record walk, and declines every other route with EZPZ_ERR_INVALID_ARGUMENT (the component interpreter, the partitioned
 * workgroup, a system whose params route is the fronts; grid teams, like the params entry): ezpz_system_sweep_guarded_plan
 * (host only, diagnostic) reports in_kernel == 0 for them.  The host form serves every route the params entry serves: where
 * in_kernel is 1 it stages and calls the device form, elsewhere it runs the rule from the host as rounds of
 * ezpz_system_solve_batch_params over the whole batch, one attempt per round for every sweep still inside its step -- the same
 * bits either way.  Ordering among launches on one EzpzSystem and the `positions` table: as for ezpz_system_sweep_params. */
typedef struct EzpzGuardConfig {
    uint32_t max_halvings; /* 0 .. 20: a step's fraction h is halved at most this often (4) */
    uint32_t max_attempts; /* >= 1: solves per step at most (12) */
    double max_move;       /* finite; > 0: an attempt that moves a value further than this from the last accepted ones is rejected (0: off) */
} EzpzGuardConfig;
typedef struct EzpzGuardStep {
    double reached;    /* t: the fraction of the step from where it started to its target that was accepted, 0 .. 1 */
    uint32_t attempts; /* solves the step took */
    uint32_t accepted; /* ... and how many of them were accepted */
} EzpzGuardStep;
void ezpz_default_guard_config(EzpzGuardConfig* out);
int ezpz_system_sweep_guarded_plan(EzpzSystem* sys, const uint32_t* positions, size_t n_param, EzpzSweepPlan* out);
int ezpz_system_sweep_guarded_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                     const double* params0_dev, const double* params_dev, size_t steps, size_t batch,
                                     const EzpzConfig* cfg, const EzpzGuardConfig* guard_cfg, double* x_out_dev,
                                     EzpzStatus* status_dev, EzpzGuardStep* guard_dev, double* params_reached_dev,
                                     uint8_t* unsat_mask_dev, uint64_t* warn_log_dev, uint32_t warn_cap, void* stream);
int ezpz_system_sweep_guarded(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const double* params0,
                              const double* params, size_t steps, size_t batch, const EzpzConfig* cfg,
                              const EzpzGuardConfig* guard_cfg, double* x_out, EzpzStatus* status, EzpzGuardStep* guard,
                              double* params_reached, uint8_t* unsat_mask, uint64_t* warn_log, uint32_t warn_cap);

/* ---- dimension sensitivities: dx/d(param) of a batch, on the device ------------------------------------------
 * For system b the caller passes values x_b (normally a solve's answer) and a parameter row p_b.  r(x, p) is the weighted
 * residual vector in the reference's row order with p overlaid exactly as ezpz_system_solve_batch_params overlays it,
 * J = dr/dx, g_j = dr/dp_j (non-zero only on the rows of constraint positions[j]; in the units of the `param` field -- per
 * degree where the tag says degrees; it carries the row's weight).  Then
 *     S_b[j, :] = -(JtJ + lambda I)^-1 Jt g_j            S: AoS [batch][n_param][n_vars], the caller's variable order
 * the linearisation of the first step the reference's loop (solver/newton.rs) takes from x_b after p_j moves: d(solution)/dp_j on a
 * well-determined system, the damped minimum-norm response on an under-determined one.  A constraint that is degenerate at x_b
 * contributes zero rows to J (the Jacobian's guards) and to g (the residual's guards), as the evaluators do; the constraints
 * of the evaluated components whose guard fired are counted in degenerate_count_out[b] (optional).  JtJ + lambda I is block
 * diagonal over the connected components of the variable-constraint graph: only the components that hold a listed constraint
 * are evaluated, and every other entry of S is +0.0.  A factorisation that meets a pivot that is not positive and finite sets
 * status_out[b] = 1 (else 0) and fills the whole S_b with NaN; other systems are unaffected.
 * S is bit-identical from run to run, whatever the batch size and the system's place in the batch.
 * ezpz_constraint_param_derivative (host only, no device): g of one constraint, g_out[row] = weight * d residual_row / d param
 * at the values x (indexed by c->ids); *degenerate (optional) = 1 where the residual's guard fired (g_out is 0 then).  Returns
 * the number of rows (1 or 2), 0 for a constraint without a parameter (ezpz_constraint_has_param) or NULL arguments.
 * params == NULL: the system's own values.  n_param == 0: status (and the host form's degenerate counts) are zeroed, nothing
 * else is written.
 * EZPZ_ERR_INVALID_ARGUMENT, with nothing enqueued and no output touched: the argument errors of the params entries (a position
 * >= n_cs, listed twice, or whose constraint has no parameter; positions NULL with n_param > 0; x, S_out or status_out NULL with
 * batch > 0) -- and, on the default route (ezpz_system_set_sensitivity_route below lifts it), a listed constraint in a component of more than EZPZ_SENSITIVITY_MAX_COMPONENT_VARS variables, or in a
 * component of the workspace shape with so many listed constraints that x, two doubles per listed constraint and 12 bytes per
 * variable exceed 64 KB of LDS (some 2800 listed constraints in a component of 1024 variables).
 * The _device form takes device pointers and only enqueues on `stream`: no host synchronisation and no allocation, except
 * that a `positions` list other than the system's last one is planned and uploaded first (repeat the list, and calls only
 * enqueue).  Launches of this entry on one EzpzSystem run one behind the other whatever their streams (they share the plan's
 * workspace).  ezpz_system_param_sensitivity_plan: which launch shape each component of that list takes (host only).  It is
 * DIAGNOSTIC: the tests use it to prove which shape ran; EzpzSensitivityPlan follows the kernels and may change or grow with
 * them -- it is not part of the stable surface. */
#define EZPZ_SENSITIVITY_MAX_COMPONENT_VARS 1024u
typedef struct EzpzSensitivityPlan {
    uint32_t n_components;       /* connected components of the system */
    uint32_t n_active;           /* ... that hold a listed constraint */
    uint32_t n_small;            /* active components on one lane per (system, component) */
    uint32_t n_lds;              /* ... on one workgroup with the factor in LDS */
    uint32_t n_workspace;        /* ... on one workgroup with the factor in a global-memory workspace */
    uint32_t max_component_vars; /* over the active components */
    uint32_t max_envelope;       /* entries of the largest factor (row envelope, diagonal included) */
    uint32_t lds_bytes;          /* per workgroup of the LDS shape */
    uint64_t workspace_bytes;    /* per resident workgroup of the workspace shape */
    /* ... and with ezpz_system_set_sensitivity_route(sys, EZPZ_SENSITIVITY_ROUTE_FRONTS) (the fields above but n_components are 0 then): */
    uint32_t route;              /* EZPZ_SENSITIVITY_ROUTE_* the call takes */
    uint32_t front_workgroups;   /* workgroups per system of the frontal plan */
    uint32_t rhs_per_item;       /* right-hand sides per work item = per factorisation (for a call of one system) */
    uint32_t items_per_system;   /* work items a system's list is cut into (for a call of one system) */
    uint32_t front_lds_bytes;    /* dynamic LDS of the launch */
} EzpzSensitivityPlan;
/* The fronts as the route of the sensitivity entries: ezpz_system_set_sensitivity_route(sys, EZPZ_SENSITIVITY_ROUTE_FRONTS) makes
 * ezpz_system_param_sensitivity and its _device form run on the FRONTAL plan of a system whose plan serves every call (the
 * condition of ezpz_system_set_params_route: EzpzSystemInfo.front_max_batch == 0xFFFFFFFF); every other system, a NULL system and
 * an unknown route get EZPZ_ERR_INVALID_ARGUMENT and keep their route.  It is a setter of its own: the params route is not
 * touched, and with it unset every call is bit for bit what it was.  On that route
 *   - every listed constraint is served whatever the size of its component (no EZPZ_SENSITIVITY_MAX_COMPONENT_VARS): one
 *     factorisation of JtJ + lambda I on the fronts serves many right-hand sides, the listed constraints of a system are cut into
 *     work items that run side by side (EzpzSensitivityPlan.rhs_per_item; EZPZ_SENS_FRONTS_RHS_PER_ITEM=<n> overrides it);
 *   - S, params, lambda, degenerate_count_out and the argument errors are those described above; S[b, j, :] does not depend on
 *     the rest of the list, its order, the work items or the batch (bit for bit); an entry that is exactly zero is +0.0;
 *   - status[b] = 1 (a pivot was not positive) as above, and status[b] = 2 with S[b] all NaN: a wait between the workgroups of
 *     a system ran out (grid_workgroups > 1 on a device that does not hold them all at once) -- never a hang;
 *   - a system on several workgroups refuses a stream that is being captured (EZPZ_ERR_INVALID_ARGUMENT, nothing enqueued).
 * The results are those of a valid Cholesky factorisation in the fronts' elimination order: at the bar of the numpy reference
 * (tests/sensitivity_ref.py), not bitwise those of the default route.  The setter waits for the system's launches on the route. */
#define EZPZ_SENSITIVITY_ROUTE_DEFAULT 0u
#define EZPZ_SENSITIVITY_ROUTE_FRONTS 1u
int ezpz_system_set_sensitivity_route(EzpzSystem* sys, uint32_t route);
int ezpz_constraint_param_derivative(const EzpzConstraint* c, const double* x, double g_out[2], int* degenerate);
int ezpz_system_param_sensitivity_plan(EzpzSystem* sys, const uint32_t* positions, size_t n_param, EzpzSensitivityPlan* out);
int ezpz_system_param_sensitivity_device(EzpzSystem* sys, const double* x_dev, const uint32_t* positions, size_t n_param,
                                         const double* params_dev, size_t batch, double lambda, double* S_out_dev,
                                         uint32_t* status_dev, uint32_t* degenerate_count_dev, void* stream);
int ezpz_system_param_sensitivity(EzpzSystem* sys, const double* x, const uint32_t* positions, size_t n_param,
                                  const double* params, size_t batch, double lambda, double* S_out, uint32_t* status_out,
                                  uint32_t* degenerate_count_out);

/* ---- solve_inner, ezpz/src/lib.rs:265-356: one tier, one system -----------------------------------
 * lint (warnings.rs:34-60) + Model::new + LM + unsatisfied list.  orig_ids (may be NULL) are the
 * ConstraintEntry.id values reported in `unsat_ids` and lint warnings. */
int ezpz_solve_inner(const EzpzConstraint* cs, const uint64_t* orig_ids, size_t n_cs, const uint32_t* var_ids,
                     const double* guesses, size_t n_guesses, const EzpzConfig* cfg, double* x_out,
                     uint64_t* unsat_ids, EzpzWarning* warn_buf, size_t warn_cap, EzpzOutcome* out);

/* ---- ezpz::solve, ezpz/src/lib.rs:80-87 -> solve_with_priority_inner (:148-263) ---------------------
 * Side inference from the guesses (constraints.rs:146-193), priority tiers, returns the last fully
 * satisfied tier.  guesses are (id, value) pairs exactly as the reference takes them.  x_out has
 * n_guesses entries, unsat_ids up to n_reqs, warn_buf up to warn_cap. */
int ezpz_solve(const EzpzConstraint* reqs, size_t n_reqs, const uint32_t* var_ids, const double* guesses,
               size_t n_guesses, const EzpzConfig* cfg, double* x_out, uint64_t* unsat_ids, EzpzWarning* warn_buf,
               size_t warn_cap, EzpzOutcome* out);

/* ---- FreedomAnalysis (reference ezpz/src/solver/find_dof.rs:14-103, analysis.rs:24-77) ----------
 * ezpz_solve_analysis replaces ezpz::solve_analysis (lib.rs:134-146): ezpz_solve plus, for the tier that is returned,
 * the indices of the underconstrained variables (ascending; under_out has room for n_guesses entries).
 * ezpz_system_freedom_batch[_device] analyse `batch` value vectors of one topology (normally the final values of a
 * batch solve): under_mask [batch][n_vars] gets 1 where the variable is underconstrained, participation
 * [batch][n_vars] (optional) the squared row norms of the orthonormal null-space basis (find_dof.rs:90-95).  The
 * Jacobian is re-evaluated at the values given (the reference reuses the LM loop's last refresh, which is the
 * Jacobian at the final values).  Where the system has a frontal plan (EzpzSystemInfo.front_workgroups) the host entries do not
 * factorise J at all: the projector onto its null space is applied to a few probe vectors by the frontal factorisation and the
 * null vectors are refined by subspace iteration -- the same sets, participation equal to rounding; more
 * than four degrees of freedom, a singular value within 1e-7 ... 3e-6 of J's largest entry, or more than 64 systems per call go
 * to the pivoted QR, like every call of the _device entry.  A large component's QR runs on many workgroups that wait for each other's chunks; should one
 * of them give up waiting (workgroups that never became resident beside another process's or stream's kernels), the host entries
 * run the analysis once more as a chain of launches that wait for nobody (EZPZ_ERR_HIP only if that fails too), and the
 * asynchronous _device entry marks the system: 0xFF in every byte of its mask, 0xFFFFFFFF as its count -- as a timed-out grid
 * team's solve reports EZPZ_ITERATIONS_TEAM_TIMEOUT.  Launches of ezpz_system_freedom_batch[_device] on one system run one behind
 * the other whatever their streams: they share the system's gathered values, Jacobian and workspace. */
int ezpz_solve_analysis(const EzpzConstraint* reqs, size_t n_reqs, const uint32_t* var_ids, const double* guesses,
                        size_t n_guesses, const EzpzConfig* cfg, double* x_out, uint64_t* unsat_ids,
                        EzpzWarning* warn_buf, size_t warn_cap, EzpzOutcome* out, uint32_t* under_out,
                        uint64_t* n_under_out);
int ezpz_system_freedom_batch(EzpzSystem* sys, const double* x, size_t batch, uint8_t* under_mask,
                              double* participation);
int ezpz_system_freedom_batch_device(EzpzSystem* sys, const double* x_dev, size_t batch, uint8_t* under_mask_dev,
                                     double* participation_dev, uint32_t* n_under_dev, void* stream);

/* ---- Redundancy analysis: redundant and conflicting constraints per system (a project extension: the reference has none) ----
 * The row-space counterpart of FreedomAnalysis.  Per system b: values x_b (normally a solve's answer, the caller's variable
 * order) and the tier the system was created from.  J (m x n) is the weighted Jacobian at x_b and r the weighted residual, rows
 * in the reference's order (request order, a constraint's rows consecutive: what ezpz_system_eval_batch returns); w_i is the
 * weight of row i's constraint.  The rows are visited IN THAT ORDER, keeping an orthonormal basis q_1 .. q_p of the rows accepted
 * so far, each q_k with a companion scalar s_k: the same linear combination applied to r.  For row i, a = J[i, :], rho = r_i:
 *   1. ||a|| == 0 exactly (a degeneracy guard fired, or nothing depends on the row at x): the row is ZERO; next row.
 *   2. classical Gram-Schmidt TWICE: per pass h = Q v, v <- v - h^T Q, rho <- rho - h . s, v starting as a.  Every dot product
 *      and every update is a fixed-order sum: results are bit-identical from run to run, whatever the batch or the place in it.
 *   3. tau = ||v|| / ||a||.  tau > rank_tol (and fewer basis vectors than the row's component has variables): INDEPENDENT,
 *      q = v / ||v|| and s = rho / ||v|| join the basis.  Otherwise the row depends on earlier rows: CONFLICTING if
 *      |rho| / w_i > conflict_tol (the linearised system cannot satisfy it together with the earlier rows), else REDUNDANT.
 * Status values: 0 INDEPENDENT, 1 ZERO, 2 REDUNDANT, 3 CONFLICTING; a constraint's status is the maximum over its rows; rank[b]
 * counts the INDEPENDENT rows.  The rule is relative per row, so a constraint's weight does not change its class -- on purpose
 * unlike find_dof.rs, whose rank rule is relative to the largest pivot.  Which of two dependent constraints is flagged is decided
 * by the order of the request: the later one.  rank_tol defaults to 1e-6 (an LM answer meets residual_tolerance 1e-8, so a
 * dependency that holds on the solution set holds at x to that order: two decades of margin), conflict_tol to 1e-4 (the
 * reference's own "satisfied" bar, lib.rs:43).  J is block diagonal over the connected components of its row / variable graph and
 * the procedure runs per component (same result as on the whole matrix).
 * Conflict groups: for focus[0 .. n_focus) (constraint positions, host memory in both entries, none listed twice)
 * group[b][k][c] = 1 when c is focus[k] itself or owns an accepted row a_j that takes part in the expansion a_i = sum c_j a_j of a
 * dependent row i of focus[k]: |c_j| ||a_j|| > group_tol ||a_i|| (group_tol defaults to 1e-6).  All zero when focus[k] has no
 * dependent row.
 * con_status [batch][n_cs]; row_status [batch][n_rows], rank [batch] optional (NULL); group [batch][n_focus][n_cs] uint8.
 * EZPZ_ERR_INVALID_ARGUMENT with nothing enqueued and no output touched: x or con_status NULL with batch > 0, a focus position
 * >= n_cs or listed twice, focus or group NULL with n_focus > 0, a tolerance negative or not finite.  batch == 0: EZPZ_OK, nothing
 * written.  EZPZ_ERR_EMPTY_SYSTEM as for FreedomAnalysis; EZPZ_ERR_TOO_LARGE: a component whose workspace exceeds 2^31 doubles.
 * The _device entry takes device pointers (focus stays a host pointer) and only enqueues on `stream`, like
 * ezpz_system_freedom_batch_device, and follows its stream-capture rules; a call whose buffers have to grow or whose focus list
 * differs from the last call's first waits for the system's previous launch of this entry.  Launches of this entry on one system
 * run one behind the other whatever their streams: they share the plan's workspace.  A component runs on one lane or one
 * workgroup; no workgroup waits for another. */
typedef struct EzpzRedundancyConfig {
    double rank_tol, conflict_tol, group_tol;
} EzpzRedundancyConfig;
#define EZPZ_ROW_INDEPENDENT 0
#define EZPZ_ROW_ZERO 1
#define EZPZ_ROW_REDUNDANT 2
#define EZPZ_ROW_CONFLICTING 3
void ezpz_default_redundancy_config(EzpzRedundancyConfig* cfg); /* 1e-6, 1e-4, 1e-6 */
int ezpz_system_redundancy(EzpzSystem* sys, const double* x, size_t batch, const EzpzRedundancyConfig* cfg /* NULL = default */,
                           uint8_t* con_status, uint8_t* row_status, uint32_t* rank, const uint32_t* focus, size_t n_focus,
                           uint8_t* group);
int ezpz_system_redundancy_device(EzpzSystem* sys, const double* x_dev, size_t batch, const EzpzRedundancyConfig* cfg,
                                  uint8_t* con_status_dev, uint8_t* row_status_dev, uint32_t* rank_dev, const uint32_t* focus,
                                  size_t n_focus, uint8_t* group_dev, void* stream);

/* ---- Reference dimensions: measure, gradient, response to the driving dimensions (a project extension: the reference has none) ----
 * A MEASUREMENT RECORD is an EzpzConstraint of which only kind, tag and ids are read; param, weight, priority and flags are
 * ignored.  It must be MEASURABLE: ezpz_constraint_has_param(record) != 0 -- the ten kinds with a length or a value, and the three
 * angle kinds with tag EZPZ_ANGLE_OTHER_DEG or EZPZ_ANGLE_OTHER_RAD.  Its ids index the system's variables, in the caller's order;
 * it need not be, and normally is not, one of the system's constraints: it is a measurement of the solution, not a condition on it.
 * m(record, x) is the value of `param` at which the record's unweighted residual vanishes at x -- for the two kinds with two rows
 * and one parameter (ArcRadius, ArcLength; PointsAtAngle's rows vanish together) the param that minimises the sum of the squares
 * of the two rows -- in the units of the `param` field: degrees where the tag says degrees.  XV(i) = x[ids[i]]:
 *   Fixed, CircleRadius                   the variable                                                       no guard
 *   VerticalDistance, HorizontalDistance  XV(1) - XV(3), XV(0) - XV(2)                                       no guard
 *   Distance                              mag(p0 - p1)                                                       none on the value
 *   ArcRadius                             (mag(c - start) + mag(c - end)) / 2                                none on the value
 *   PointLineDistance, Vertical..., Horizontal...   the residual's own expression without `- param`          the residual's
 *   LinesAtAngle, ArcAngle, PointsAtAngle theta = atan2(cross(u, v), dot(u, v)) in (-pi, pi], u and v the vectors the residual
 *                                         uses; x 180 / pi for the DEG tag                                   the residual's
 *   ArcLength                             mag(u) * rem_euclid(theta(u, w), 2 pi), u = start - c, w = end - c the residual's (r2 <= EPS^2)
 * in the residual's operand order.  The ArcLength value lies in [0, 2 pi r): an arc runs counter-clockwise from start to end.  A
 * guard is the residual's guard of the kind, same comparison, same operands; where it fires m = 0, every gradient slot is 0 and
 * flag bit 0 is set -- exactly where the residual reports degenerate.  grad[slot] = d m / d x[ids[slot]] for slot < the kind's
 * number of ids; the slots from there up to 7 are +0.0.  Gradient guard, flag bit 1, with m still valid: Distance with dist < EPS,
 * and each row of ArcRadius on its own (the guards of the Jacobian's Distance rows); the guarded row contributes zeros.  The
 * branch cuts are documented, not smoothed: theta = +-pi for the angle kinds (opposite arms give +pi), theta = 0 for ArcLength;
 * an arc whose end lies on its centre has no finite gradient.
 * ezpz_constraint_measure (host only, no device): m, grad[8] and the flags of one record at the values x (indexed by c->ids; each
 * output optional).  Returns the kind's number of ids for a measurable record, 0 otherwise or on NULL c / x.
 * ezpz_system_measure[_device]: `batch` value vectors x (AoS [batch][n_vars], normally a solve's or a sweep's answers) against
 * records[0 .. n_meas): m_out [batch][n_meas]; flags_out [batch][n_meas] bytes and grad_out [batch][n_meas][8] optional (NULL).
 * ezpz_system_measure_response[_device]: with S [batch][n_param][n_vars] as ezpz_system_param_sensitivity_device wrote it,
 *     D[b, i, j] = sum over slot of grad[b, i, slot] * S[b, j, ids_i[slot]]      slots ascending, left to right from the first product
 * D_out [batch][n_meas][n_param]: how reference dimension i answers to driving dimension j.  With tol [n_param] (optional) the
 * tolerance stack-up, worst_out and rss_out [batch][n_meas] (both or neither, only with tol):
 *     worst[b, i] = sum_j |D[b, i, j]| * tol[j]        rss[b, i] = sqrt(sum_j (D[b, i, j] * tol[j])^2)       j ascending from +0.0
 * ezpz_system_measure_vjp[_device]: grad_x_out [batch][n_vars],
 *     grad_x[b, v] = sum of grad_m[b, i] * grad[b, i, slot] over the pairs (i, slot) with ids_i[slot] == v, ascending (i, slot) from +0.0
 * +0.0 for a variable no record names: the vector-Jacobian product that makes measure(solve(...)) differentiable end to end.
 * A flagged measurement contributes zeros.  NaN in S propagates: a system whose sensitivity status was 1 gives NaN responses.
 * m[b, i], grad[b, i, :] and D[b, i, :] depend on x_b, S_b and record i alone: bit-identical from run to run, whatever the batch,
 * the system's place in it, the rest of the list and its order; grad_x depends on the list's order only through the order of its
 * sum.  No sum uses atomics; no workgroup waits for another.
 * EZPZ_ERR_INVALID_ARGUMENT, with nothing enqueued and no output touched: a record that is not measurable, an id >= n_vars,
 * records NULL with n_meas > 0, a required pointer NULL with a non-empty call, worst_out / rss_out without tol or only one of the
 * two, a negative or non-finite tol (host form).  EZPZ_ERR_TOO_LARGE: more than 2^20 records.  batch == 0, n_meas == 0, or
 * n_param == 0 for the response: EZPZ_OK, nothing written -- after the checks above that need no values: a list with a record that
 * is not measurable, an id >= n_vars, worst_out / rss_out without tol, or a bad tol is EZPZ_ERR_INVALID_ARGUMENT even with batch == 0.
 * `records` is host memory in both forms.  The _device forms take device pointers (tol included) and only enqueue on `stream`; a
 * list other than the system's last one is first checked, packed and uploaded behind the last launch that read the tables (repeat
 * the list, and calls only enqueue), as is the vjp's variable -> (i, slot) table the first time a list needs it, and a workspace
 * that has to grow.  Launches of these entries on one EzpzSystem run one behind the other whatever their streams; stream capture
 * follows ezpz_system_redundancy_device.  A row x_b of 512 to 1536 variables is staged in LDS, shorter and longer ones are gathered
 * from global memory; EZPZ_MEASURE_ROUTE=row / direct forces either placement (row: up to 7168 variables) -- same bits.
 * Staging loads 16 bytes per lane: an x_dev that is not 16-byte aligned is gathered from global memory whatever its size and
 * whatever EZPZ_MEASURE_ROUTE says; a grad_out_dev that is not 16-byte aligned is written in 8-byte stores.  Same bits again. */
int ezpz_constraint_measure(const EzpzConstraint* c, const double* x, double* m_out, double grad_out[8], int* flags);
int ezpz_system_measure(EzpzSystem* sys, const EzpzConstraint* records, size_t n_meas, const double* x, size_t batch, double* m_out,
                        uint8_t* flags_out, double* grad_out);
int ezpz_system_measure_device(EzpzSystem* sys, const EzpzConstraint* records, size_t n_meas, const double* x_dev, size_t batch,
                               double* m_out_dev, uint8_t* flags_out_dev, double* grad_out_dev, void* stream);
int ezpz_system_measure_response(EzpzSystem* sys, const EzpzConstraint* records, size_t n_meas, const double* x, const double* S,
                                 size_t n_param, size_t batch, const double* tol, double* D_out, double* worst_out, double* rss_out);
int ezpz_system_measure_response_device(EzpzSystem* sys, const EzpzConstraint* records, size_t n_meas, const double* x_dev,
                                        const double* S_dev, size_t n_param, size_t batch, const double* tol_dev, double* D_out_dev,
                                        double* worst_out_dev, double* rss_out_dev, void* stream);
int ezpz_system_measure_vjp(EzpzSystem* sys, const EzpzConstraint* records, size_t n_meas, const double* x, const double* grad_m,
                            size_t batch, double* grad_x_out);
int ezpz_system_measure_vjp_device(EzpzSystem* sys, const EzpzConstraint* records, size_t n_meas, const double* x_dev,
                                   const double* grad_m_dev, size_t batch, double* grad_x_out_dev, void* stream);

/* ---- Monte-Carlo tolerance analysis: sampled driven solves, measured, with statistics reduced on the device (a project
 * extension) -- the non-linear counterpart of ezpz_system_measure_response's stack-up.  Every driving dimension (the constraints at
 * `positions`, as ezpz_system_solve_batch_params takes them) is drawn from its tolerance distribution `samples` times, every variant
 * is solved from x0, the reference dimensions `records` (measurement records, as ezpz_system_measure takes them) are read off each
 * answer, and what comes back is one EzpzMcStats per record, the totals and an optional histogram: n_meas small records, not
 * samples x n_vars values.  x0 [n_vars] is expected to be the NOMINAL SOLUTION -- the answer for the nominal values: every variant
 * starts from it, and nominal[i] of the statistics is measured on it.
 * THE DRAW.  p[b][j] = nominal[j] + deviation, the deviation of sample b (0-based, 64 bits) for dimension j by dist[j]:
 *   EZPZ_MC_FIXED    p = nominal[j], as given (nothing is added)
 *   EZPZ_MC_UNIFORM  a + (b - a) * u,  a <= b the deviations' ends, u in [0, 1)
 *   EZPZ_MC_NORMAL   a * z,  a = sigma >= 0,  b = the truncation in sigmas: 0 = none, else >= 1
 *   EZPZ_MC_CORNER   bit c of the sample index ? b : a,  c = the rank of j among the CORNER dimensions of the list (at most 20 of them):
 *                    samples 0 .. 2^k - 1 are the 2^k corners of k such dimensions
 * u and z come from Philox4x32-10 with counter (b & 0xffffffff, b >> 32, j, t), t the attempt, and key (seed & 0xffffffff,
 * seed >> 32), whose words w0..w3 give
 *   u = ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53     u1 = ((w0 >> 5) * 2^26 + (w1 >> 6) + 1) * 2^-53     u2 = ((w2 >> 5) * 2^26 + (w3 >> 6)) * 2^-53
 * (each exact in a double).  UNIFORM takes u of attempt 0.  NORMAL: z = sqrt(-2 * log(u1)) * cos(TWO_PI * u2), TWO_PI the double
 * nearest 2 pi and the product TWO_PI * u2 rounded once; with a truncation T the attempts 0 .. 15 are tried in order and the first z
 * with |z| <= T is taken, and if none is, z = copysign(T, z of attempt 15).  No product is contracted into a fused multiply-add, on
 * the host or on the device.  A draw depends on (seed, b, j) and dist[j] alone: never on the batch, the round, the other dimensions.
 * ezpz_mc_sample (host only, no device): params_out [count][n_param] = the draws of the samples first .. first + count - 1, from the
 * sampler's one source.  FIXED, UNIFORM and CORNER draws are bit-identical on the host and on the device; a NORMAL draw can differ
 * there in the last bits of log, cos and sqrt -- the ONLY thing in this section that is not bit-reproducible between the two.
 * EZPZ_ERR_INVALID_ARGUMENT with nothing written: an unknown kind, a non-finite a, b or nominal, a > b for UNIFORM, sigma < 0, a
 * truncation in (0, 1) (or negative), more than 20 CORNER dimensions, dist or nominal NULL with n_param > 0.
 * THE SEQUENCE (a project extension).  Bit 0 of EzpzMcDist.reserved, EZPZ_MC_SEQUENCE, asks for a low-discrepancy
 * draw of that dimension: a Sobol' point with a seed-keyed digital shift in place of the Philox words.  It is read on UNIFORM and
 * NORMAL dimensions and ignored on FIXED and CORNER; the other bits of `reserved` stay ignored; with the bit clear every byte of
 * every draw above is what it was.  For a flagged dimension at list position j and sample b:
 *   g = b ^ (b >> 1);   x = the XOR over the set bits c of g of V[j][c]
 *   V: the 32-bit Joe-Kuo direction numbers (new-joe-kuo-6.21201) of Sobol' dimensions 0 .. 63, bit 31 first (V[j][0] = 2^31) -- with
 *   the Gray-coded index, x of row b is row b of the unscrambled 32-bit Sobol' sequence in its usual order
 *   s = w0 of Philox4x32-10 with counter (0, 0, j, 0xFFFFFFFF) and the seed as key (no plain draw uses the attempt 0xFFFFFFFF)
 *   u = ((x ^ s) + 0.5) * 2^-32, exact in a double and inside (0, 1), open at both ends
 *   UNIFORM  a + (b - a) * u
 *   NORMAL   a * z;  without a truncation z = PHI_INV(u);  with a truncation T:  p = P_lo + (P_hi - P_lo) * u,  P_lo = 0.5 *
 *            erfc(T / sqrt(2)) and P_hi = 1 - P_lo computed once on the host,  z = PHI_INV(p) clamped to [-T, T].  No attempts.
 * PHI_INV is Wichura's algorithm AS 241, routine PPND16 (Applied Statistics 37 (1988) 477-484), evaluated as published, no product
 * contracted.  Its central branch, |p - 0.5| <= 0.425 -- 85 % of the draws -- is a rational polynomial of + - * / alone: those draws,
 * and every flagged UNIFORM draw, are bit-identical on the host and on the device.  Its two tail branches use log and sqrt and fall
 * under the caveat above.  An untruncated flagged NORMAL reaches about +-6.34 sigma and no further: u ends at 2^-33 from 0 and 1.
 * The draw still depends on (seed, b, j) and dist[j] alone, so every reduction below takes it as it takes a plain one.  What it
 * buys: for a smooth response the error of mean and std (and of what is built on them: beta, contrib, cond_mean) falls nearly as
 * 1 / samples where a plain run's falls as 1 / sqrt(samples); it does NOT help yields at a tail limit or extreme quantiles much,
 * and the variance estimates of a plain run (var / n as the error of mean) overstate a flagged run's error.
 * EZPZ_ERR_INVALID_ARGUMENT with nothing written or enqueued: a flagged UNIFORM or NORMAL dimension at a position j >= 64; a
 * flagged dimension with first + count > 2^32 (ezpz_mc_sample) or samples > 2^32 (the runs); ezpz_system_tolerance_sobol[_device]
 * with a flagged dimension -- its matrix B would be matrix A XOR a constant, not an independent matrix, and pick-freeze on the two
 * means nothing (as a CORNER dimension has no second matrix at all).
 * THE RUN.  ezpz_system_tolerance_mc[_device] works in rounds of `chunk` samples (rounded up to a multiple of 256; 0: the library's
 * choice, 65536 or less for a large system), everything on one stream: the sampler writes the round's params, a second kernel its
 * copies of x0, ezpz_system_solve_batch_params_device solves them -- that entry itself: whatever params route the system has, the
 * fronts included, and a system it declines is declined here with the same error -- ezpz_system_measure_device measures the answers
 * (m and flags), and the reduction kernel folds the round into the results.  Memory is bounded by chunk, not by samples.
 * nominal == NULL: the system's own params at `positions`.  n_param == 0 is legal: every sample is the same solve.
 * Sample b is OK when its EzpzStatus has converged != 0 and n_unsatisfied == 0.  It is VALID FOR record i when it is ok, flag bit 0
 * of (b, i) is clear and m is finite.  stats[i], over the samples valid for i, with d = m - nominal[i] and nominal[i] = m(record
 * i, x0) measured once before round 0 (0 where the guard fires):
 *   n_valid;  sum_d = sum of d;  sum_d2 = sum of (d * d), the product rounded, then added;  min, max;  argmin, argmax: the sample
 *   indices, the lowest among equals;  n_in: the count with lim_lo[i] <= m <= lim_hi[i] (n_valid without limits);
 *   mean = nominal + sum_d / n_valid;  var = (sum_d2 - sum_d * sum_d / n_valid) / (n_valid - 1).
 * No valid sample: mean and var NaN, min = +inf, max = -inf, argmin = argmax = UINT64_MAX; one: var NaN.
 * hist [n_meas][hist_bins + 2] (hist_bins > 0): under, the bins, over -- a valid m counts in bin floor((m - hist_lo[i]) * scale_i),
 * scale_i = hist_bins / (hist_hi[i] - hist_lo[i]) computed once on the host; m < hist_lo[i] is under, a bin >= hist_bins over.
 * totals: samples; n_ok, the ok samples; n_all_in, the samples valid for and inside the limits of EVERY record.  Variants that do not
 * assemble are counted (samples - n_ok), never averaged.  The angle kinds' branch cut at +-pi is the measurement's and is not
 * unwrapped: a reference angle that straddles it has samples near both ends, and its mean says little.
 * THE ORDER OF EVERY FLOATING SUM is fixed by this interface.  Block q is the samples [256 q, 256 q + 256).  Inside a block the 256
 * leaves -- +0.0 for a sample that is invalid or past `samples` -- are summed by the adjacent-pair tree: for h = 1, 2, .. 128,
 * v[t] += v[t + h] for every t that is a multiple of 2 h.  The blocks' sums are then added left to right from +0.0.  There are no
 * floating-point atomics (counts and histogram bins are integers).  Therefore every output has the same bits for any chunk, any
 * stream and any device, and the host form gives exactly the device form's bits -- given the same draws and the same answers of
 * the two entries above, which are reproducible themselves.
 * keep_params [samples][n_param], keep_m [samples][n_meas], keep_flags [samples][n_meas], keep_ok [samples] bytes (each optional,
 * NULL): the samples themselves.  m and flags of a sample that is not ok are those of whatever the solve left.
 * EZPZ_ERR_INVALID_ARGUMENT with nothing enqueued and no output touched: every argument error of the params entry (the list, a
 * system it declines, a capture its fronts refuse) and of the measure entry (the records); every error of ezpz_mc_sample;
 * hist_bins > 64; hist_bins > 0 without ranges or with hist_hi <= hist_lo; one limit array without the other, or lim_lo > lim_hi;
 * stats or totals (or x0, or hist with hist_bins > 0) NULL with samples > 0.  samples == 0: EZPZ_OK after those checks, nothing written.
 * The _device form takes device pointers for x0 and every output (keep_* included) and host pointers for positions, dist, nominal,
 * records, limits and ranges.  It enqueues on `stream`; distributions, limits or ranges other than the last run's, or a workspace
 * that has to grow, are first uploaded behind the last run's launches (repeat them, and a run only enqueues -- as far as the two
 * entries do).  Runs on one EzpzSystem go one behind the other whatever their streams.  Stream capture, thread safety and the
 * ordering against other launches on the system: those of the two entries it is made of.  mc == NULL: ezpz_default_mc_config's
 * values (seed 0, chunk 0, hist_bins 0); cfg as for the params entry. */
#define EZPZ_MC_FIXED 0u
#define EZPZ_MC_UNIFORM 1u
#define EZPZ_MC_NORMAL 2u
#define EZPZ_MC_CORNER 3u
#define EZPZ_MC_SEQUENCE 1u /* bit 0 of EzpzMcDist.reserved: THE SEQUENCE */
typedef struct EzpzMcDist { /* 24 bytes */
    uint32_t kind, reserved; /* reserved: EZPZ_MC_SEQUENCE or 0; the other bits are ignored */
    double a, b;
} EzpzMcDist;
typedef struct EzpzMcConfig { /* 16 bytes */
    uint64_t seed;
    uint32_t chunk;     /* samples per round; 0 = the library's choice */
    uint32_t hist_bins; /* 0 .. 64 */
} EzpzMcConfig;
typedef struct EzpzMcStats { /* one per measurement record; 88 bytes */
    uint64_t n_valid, n_in, argmin, argmax;
    double nominal, sum_d, sum_d2, mean, var, min, max;
} EzpzMcStats;
typedef struct EzpzMcTotals { /* 24 bytes */
    uint64_t samples, n_ok, n_all_in;
} EzpzMcTotals;
void ezpz_default_mc_config(EzpzMcConfig* mc);
int ezpz_mc_sample(uint64_t seed, const EzpzMcDist* dist, const double* nominal, size_t n_param, uint64_t first, size_t count,
                   double* params_out);
int ezpz_system_tolerance_mc(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const EzpzMcDist* dist,
                             const double* nominal, const EzpzConstraint* records, size_t n_meas, const double* lim_lo,
                             const double* lim_hi, const double* hist_lo, const double* hist_hi, uint64_t samples,
                             const EzpzMcConfig* mc, const EzpzConfig* cfg, EzpzMcStats* stats, EzpzMcTotals* totals, uint64_t* hist,
                             double* keep_params, double* keep_m, uint8_t* keep_flags, uint8_t* keep_ok);
int ezpz_system_tolerance_mc_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                    const EzpzMcDist* dist, const double* nominal, const EzpzConstraint* records, size_t n_meas,
                                    const double* lim_lo, const double* lim_hi, const double* hist_lo, const double* hist_hi,
                                    uint64_t samples, const EzpzMcConfig* mc, const EzpzConfig* cfg, EzpzMcStats* stats_dev,
                                    EzpzMcTotals* totals_dev, uint64_t* hist_dev, double* keep_params_dev, double* keep_m_dev,
                                    uint8_t* keep_flags_dev, uint8_t* keep_ok_dev, void* stream);

/* ---- Tolerance contributors: which driving dimension causes the spread (a project extension) -- the Monte-Carlo
 * counterpart of D of ezpz_system_measure_response.  The second-moment matrix between the sampled driving dimensions and the measured
 * reference dimensions of a Monte-Carlo run is reduced on the device, with the fixed-order sums of the section above, and a closing
 * step turns it into the covariance, the regression coefficients (effective sensitivities over the tolerance zone), each driving
 * dimension's share of each reference dimension's variance, and the explained fraction r2: 1 - r2 is what non-linearity and
 * interactions cause.  samples x (n_param + n_meas) values come back as K + K (K + 1) / 2 sums.
 * THE SAMPLE VECTOR.  k = n_param, m = n_meas, K = k + m, 1 <= K <= EZPZ_MC_MOMENT_MAX.  For sample b, z [K]:
 *   z[j] = p[b][j] - nominal_p[j], j < k;     z[k + i] = m[b][i] - nominal_m[i], i < m
 * each one rounded subtraction: a FIXED dimension gives exactly +0.0.  In the run nominal_p is the nominal of the draw and nominal_m
 * the statistics' nominal[i].
 * Sample b is COMPLETE when it is ok (the run: the section above's rule; ezpz_mc_moments: ok[b] != 0, ok == NULL: every one) and,
 * for EVERY record i, flag bit 0 of (b, i) is clear (flags == NULL: every one) and m[b][i] is finite.  One rule for the whole matrix
 * (complete cases); per-record validity stays in EzpzMcStats.n_valid.  A caller whose record is always degenerate sees
 * n_complete == 0 and drops that record.
 * THE MOMENTS.  moments [K + K (K + 1) / 2]: first the K sums s[a] = sum of z[a]; then the upper triangle, row-major (a = 0: b = 0 ..
 * K - 1; a = 1: b = 1 .. K - 1; ..): G[a][b] = sum of (z[a] * z[b]), a <= b, the product rounded, then added.  EzpzMcMomentsInfo:
 * samples; n_complete, the complete samples.
 * THE ORDER OF EVERY SUM is the section above's: block q is the samples [256 q, 256 q + 256); a leaf is the sample's z[a], or its
 * rounded product, and +0.0 for a sample that is incomplete or past `samples`; inside a block the 256 leaves are summed by the
 * adjacent-pair tree (for h = 1, 2, .. 128: v[t] += v[t + h] for every t that is a multiple of 2 h); the blocks' sums are added left
 * to right from +0.0.  No floating-point atomics, no product contracted into a fused multiply-add: the same bits for any chunk, any
 * stream and any device.
 * THE CLOSING STEP, ezpz_mc_contributors (host only, no device; the run's kernel has the same body and gives the same bits): a pure
 * function of moments, n_complete, k, m and pivot_rel, from + - * / and comparisons alone, every loop ascending.  n = n_complete as
 * a double.
 *   cov [K][K], full and symmetric: cov[a][b] = (G[a][b] - s[a] * s[b] / n) / (n - 1), evaluated as written for a <= b and mirrored.
 *   n_complete < 2: cov, beta, contrib and r2 are all NaN, dropped is all ones (UINT64_MAX); nothing below applies.
 *   LDL^T of the input block cov[0 .. k)[0 .. k), j ascending.  KEPT(l): dimension l was not dropped.
 *     d_j = cov[j][j], then for every kept l < j, ascending:  t = L[j][l] * d_l;  d_j = d_j - L[j][l] * t
 *     dimension j is kept when cov[j][j] > 0 and d_j > pivot_rel * cov[j][j] (false for NaN), else DROPPED: bit j of `dropped`
 *     kept j, every i > j:  v = cov[i][j], then for every kept l < j, ascending:  t = L[j][l] * d_l;  v = v - L[i][l] * t;
 *                           L[i][j] = v / d_j
 *   A dropped dimension is left out of the factorisation: FIXED dimensions (variance 0), a dimension that repeats an earlier one,
 *   CORNER dimensions aliased by too few samples.  pivot_rel (EzpzMcContribConfig; default 2^-26): below sqrt(epsilon) of its own
 *   variance a dimension is a combination of earlier ones to half the digits, and its coefficient would have none left.
 *   beta [m][k], per record i -- cov[0 .. k)[0 .. k) beta_i = cov[0 .. k)[k + i] over the kept dimensions, 0 for a dropped one:
 *     y_j = cov[j][k + i], then for every kept l < j, ascending: y_j = y_j - L[j][l] * y_l          (j ascending, kept)
 *     w_j = y_j / d_j
 *     beta_j = w_j, then for every kept l > j, ascending: beta_j = beta_j - L[l][j] * beta_l       (j descending, kept)
 *   r2 [m]:  explained_i = +0.0, then for every kept j, ascending: explained_i = explained_i + beta[i][j] * cov[j][k + i];
 *            r2[i] = explained_i / cov[k + i][k + i]
 *   contrib [m][k]:  contrib[i][j] = beta[i][j] * beta[i][j] * cov[j][j] / cov[k + i][k + i] (left to right), +0.0 for a dropped j
 *   A reference dimension whose variance is not > 0 gives NaN for r2[i] and contrib[i][*] (its beta is what the formulas give).
 * The sum of contrib[i][j] over j equals r2[i] only up to the sampled inputs' cross-covariances -- r2[i] - sum_j contrib[i][j] is
 * sum over j != l of beta[i][j] * beta[i][l] * cov[j][l] / cov[k + i][k + i] -- which are O(1 / sqrt(n)) of the variances for the
 * sampler's independent draws.  Correlations need a square root and are left to the caller (cov / sqrt(outer(diag))).
 * ezpz_mc_moments[_device]: the reduction alone on the caller's samples -- params [samples][n_param], m [samples][n_meas], flags
 * [samples][n_meas] bytes, ok [samples] bytes, nominal_p [n_param], nominal_m [n_meas] -- no system involved; useful on the kept
 * samples of any run.  It works in rounds of `chunk` samples (rounded up to a multiple of 256; 0: 65536) on a workspace the library
 * owns per device, as ezpz_branch_cluster's.  The _device form takes device pointers for every array and only enqueues on `stream`
 * (a workspace that has to grow is first allocated behind the last call's launches); calls on one device go one behind the other
 * whatever their streams.
 * ezpz_system_tolerance_mc_contrib[_device]: ezpz_system_tolerance_mc[_device] -- the same arguments, the same run, stats, totals,
 * hist and keep_* byte for byte -- with one more kernel per round, behind the round's reduction, that folds the round's params, m,
 * flags and ok into `moments` and `info`, and one closing kernel behind the last round that fills cov, beta, contrib, r2 and dropped
 * [1] from them.  The _device form takes device pointers for these outputs too.  cc == NULL: ezpz_default_mc_contrib_config's value.
 * EZPZ_ERR_INVALID_ARGUMENT with nothing enqueued and no output touched: K == 0; K > EZPZ_MC_MOMENT_MAX; a negative or non-finite
 * pivot_rel; moments NULL (ezpz_mc_contributors: or an output that has elements NULL); with samples > 0: an output NULL -- moments,
 * info, and for the run cov, dropped, r2 (m > 0), beta and contrib (k m > 0) -- or an input that has elements NULL (flags and ok
 * may be); for the run every argument error of ezpz_system_tolerance_mc.  samples == 0: EZPZ_OK after those checks, nothing written. */
#define EZPZ_MC_MOMENT_MAX 64u
typedef struct EzpzMcContribConfig { /* 16 bytes */
    double pivot_rel; /* >= 0; default 2^-26 */
    uint64_t reserved;
} EzpzMcContribConfig;
typedef struct EzpzMcMomentsInfo { /* 16 bytes */
    uint64_t samples, n_complete;
} EzpzMcMomentsInfo;
void ezpz_default_mc_contrib_config(EzpzMcContribConfig* cc);
int ezpz_mc_contributors(const double* moments, uint64_t n_complete, size_t n_param, size_t n_meas, const EzpzMcContribConfig* cc,
                         double* cov, double* beta, double* contrib, double* r2, uint64_t* dropped);
int ezpz_mc_moments(const double* params, const double* m, const uint8_t* flags, const uint8_t* ok, const double* nominal_p,
                    const double* nominal_m, uint64_t samples, size_t n_param, size_t n_meas, uint32_t chunk, double* moments,
                    EzpzMcMomentsInfo* info);
int ezpz_mc_moments_device(const double* params_dev, const double* m_dev, const uint8_t* flags_dev, const uint8_t* ok_dev,
                           const double* nominal_p_dev, const double* nominal_m_dev, uint64_t samples, size_t n_param, size_t n_meas,
                           uint32_t chunk, double* moments_dev, EzpzMcMomentsInfo* info_dev, void* stream);
int ezpz_system_tolerance_mc_contrib(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const EzpzMcDist* dist,
                                     const double* nominal, const EzpzConstraint* records, size_t n_meas, const double* lim_lo,
                                     const double* lim_hi, const double* hist_lo, const double* hist_hi, uint64_t samples,
                                     const EzpzMcConfig* mc, const EzpzConfig* cfg, EzpzMcStats* stats, EzpzMcTotals* totals,
                                     uint64_t* hist, double* keep_params, double* keep_m, uint8_t* keep_flags, uint8_t* keep_ok,
                                     const EzpzMcContribConfig* cc, double* moments, EzpzMcMomentsInfo* info, double* cov, double* beta,
                                     double* contrib, double* r2, uint64_t* dropped);
int ezpz_system_tolerance_mc_contrib_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                            const EzpzMcDist* dist, const double* nominal, const EzpzConstraint* records, size_t n_meas,
                                            const double* lim_lo, const double* lim_hi, const double* hist_lo, const double* hist_hi,
                                            uint64_t samples, const EzpzMcConfig* mc, const EzpzConfig* cfg, EzpzMcStats* stats_dev,
                                            EzpzMcTotals* totals_dev, uint64_t* hist_dev, double* keep_params_dev, double* keep_m_dev,
                                            uint8_t* keep_flags_dev, uint8_t* keep_ok_dev, const EzpzMcContribConfig* cc,
                                            double* moments_dev, EzpzMcMomentsInfo* info_dev, double* cov_dev, double* beta_dev,
                                            double* contrib_dev, double* r2_dev, uint64_t* dropped_dev, void* stream);

/* ---- Sobol tolerance indices: which driving dimension causes the spread, curvature and interactions included (a
 * project extension) -- the variance-based counterpart of the contributors above.  A regression is blind to a dimension that acts
 * through curvature alone (beta and contrib are 0 by symmetry) and cannot say who is behind 1 - r2.  The first-order index first[i][j]
 * is the share of reference dimension i's variance that driving dimension j causes on its own, the total-effect index total[i][j] the
 * share it causes alone or together with others; total - first is what j's interactions cause.  Both are estimated by pick-freeze
 * sampling: (k' + 2) x samples driven solves for k' sampled dimensions, reduced on the device with the fixed-order sums of the
 * Monte-Carlo section to 4 + 4 k sums per record.
 * THE MATRICES.  k = n_param <= EZPZ_SOBOL_MAX, m = n_meas, 1 <= m <= EZPZ_SOBOL_MAX.  Sample b of matrix A is row b of
 * ezpz_mc_sample(seed, ..): the draws of ezpz_system_tolerance_mc with the same seed.  Matrix B is the same with seed_b
 * (EzpzSobolConfig; ezpz_default_sobol_config: 0x9E3779B97F4A7C15); seed_b == seed is an argument error.  Matrix AB_j is A with
 * column j taken from B.  A FIXED dimension has AB_j == A and is not solved.  A CORNER dimension is an argument error: its draw
 * depends on the sample index alone, so A and B coincide.
 * THE ROWS.  Per sample k + 2 rows of measurements, f [samples][k + 2][m]: row 0 of A, row 1 of B, row 2 + j of AB_j; for a FIXED j
 * the kept row is a copy of row 0.  A row is SOLVED unless it is the row 2 + j of a FIXED j.
 * Sample b is COMPLETE FOR record i when every solved row of b is ok (the run: the Monte-Carlo section's rule; ezpz_mc_sobol_sums:
 * ok[b][r] != 0, ok == NULL: every one) and, in every solved row r, flag bit 0 of (b, r, i) is clear (flags == NULL: every one) and
 * f[b][r][i] is finite.  Per record, not per sample as for the contributors: the records are independent here.
 * THE LEAVES of sample b for record i, each operation rounded once, no product contracted into a fused multiply-add; every leaf is
 * +0.0 for a sample that is incomplete for i or past `samples`:
 *   dA = f[b][0][i] - nominal_m[i];   dB = f[b][1][i] - nominal_m[i];   dj = f[b][2 + j][i] - nominal_m[i];   t = dj - dA
 *   p = dB * t  (first order: Saltelli et al. 2010);   q = t * t  (total effect: Jansen 1999);   p * p;   q * q;
 *   dA;   dB;   dA * dA;   dB * dB
 * THE SUMS.  sums [m][4 + 4 k], per record: sA, sB, sAA, sBB (the sums of dA, dB, dA * dA, dB * dB), then P [k], Q [k], P2 [k], Q2 [k]
 * (the sums of p, q, p * p, q * q per dimension); n_complete [m] uint64: the samples complete for i.  The order of every sum is the
 * Monte-Carlo section's: block q is the samples [256 q, 256 q + 256), the 256 leaves are summed by the adjacent-pair tree (for h =
 * 1, 2, .. 128: v[t] += v[t + h] for every t that is a multiple of 2 h), the blocks' sums are added left to right from +0.0; no
 * floating-point atomics: the same bits for any chunk, any stream and any device, and on the host.  For a FIXED j the four entries
 * are WRITTEN as +0.0, not summed (dB * (+0.0) is -0.0 for a negative dB, and a block of those sums to -0.0).
 * THE CLOSING STEP, ezpz_mc_sobol_indices (host only, no device; the run's kernel has the same body and gives the same bits): a
 * pure function of sums, n_complete, k and m, from + - * / and comparisons alone, per record i, every loop ascending, each line
 * evaluated as written, left to right.  n = n_complete[i] as a double.
 *   n_complete[i] < 2: var[i], first[i][*], total[i][*], first_var[i][*], total_var[i][*] are all NaN; nothing below applies.
 *   n2 = 2 * n;   s = sA + sB;   mean = s / n2;   var[i] = ((sAA + sBB) - s * mean) / (n2 - 1)
 *   var[i] not > 0 (a constant record; NaN): first, total, first_var and total_var of the record are NaN.  Else, j ascending:
 *   pm = P[j] / n;                first[i][j] = pm / var[i];   first_var[i][j] = ((P2[j] / n - pm * pm) / (n - 1)) / (var[i] * var[i])
 *   qm = (Q[j] / 2) / n;          total[i][j] = (Q[j] / n2) / var[i]
 *   total_var[i][j] = (((Q2[j] / 4) / n - qm * qm) / (n - 1)) / (var[i] * var[i])
 * var is the variance of the 2 n values dA and dB pooled.  first_var and total_var are the variances of the two estimates -- the
 * sample variance of the leaves over n, scaled -- and IGNORE the uncertainty of var itself; the standard error is their square root,
 * which is the caller's, as for the correlations.  total - first, what interactions cause, is the caller's subtraction too.  A FIXED
 * dimension's indices are +0.0.  An estimate can leave [0, 1] by its own error; nothing is clamped.
 * ezpz_mc_sobol_sums[_device]: the reduction alone on the caller's rows -- f [samples][k + 2][m], flags (bytes, the same shape, may
 * be NULL), ok [samples][k + 2] bytes (may be NULL), nominal_m [m], fixed_mask (bit j: dimension j is FIXED; bits >= k must be
 * clear) -- no system involved; useful on the kept rows of any run.  The host form computes on the host, with no device, and gives
 * the device form's bits.  The _device form takes device pointers for every array and only enqueues on `stream`, in rounds of `chunk`
 * samples (rounded up to a multiple of 256; 0: 65536) on a workspace the library owns per device (a workspace that has to grow is
 * first allocated behind the last call's launches); calls on one device go one behind the other whatever their streams.
 * ezpz_system_tolerance_sobol[_device]: THE RUN -- the arguments of ezpz_system_tolerance_mc[_device] without limits and
 * histogram (mc->hist_bins must be 0), plus EzpzSobolConfig.  A round of `chunk` samples (0: the largest multiple of 256, at most
 * 65536, whose rows -- chunk x (k + 2) x m doubles -- and whose copies of x0 each stay below 256 MiB) is k' + 2 sub-rounds on the
 * caller's stream, k' the dimensions that are not FIXED: the sampler with the seed chosen per column, the copies of x0,
 * ezpz_system_solve_batch_params_device and ezpz_system_measure_device -- those entries themselves -- into the round's rows; the
 * Monte-Carlo section's reduction follows A's sub-round, so stats [m] and totals are ezpz_system_tolerance_mc's with the same seed,
 * byte for byte; one kernel behind the last sub-round folds the round's rows into sums and n_complete, and one closing kernel behind
 * the last round fills var [m], first, total, first_var and total_var [m][k].  keep_f [samples][k + 2][m], keep_flags (bytes, the
 * same shape), keep_ok [samples][k + 2] bytes (each optional, NULL): the rows themselves; the flags and ok of a FIXED j's row are
 * copies of row 0's too.  The _device form takes device pointers for x0 and every output and enqueues as ezpz_system_tolerance_mc_device
 * does; runs on one EzpzSystem, of either kind, go one behind the other.  sobol == NULL: ezpz_default_sobol_config's value.
 * EZPZ_ERR_INVALID_ARGUMENT with nothing enqueued and no output touched: k > EZPZ_SOBOL_MAX; m == 0 or m > EZPZ_SOBOL_MAX; a CORNER
 * dimension; seed_b == seed; a fixed_mask bit at or above k; with samples > 0 an output NULL -- sums, n_complete, and for the run
 * stats, totals, var, and with k > 0 first, total, first_var, total_var (ezpz_mc_sobol_indices: whatever samples) -- or an input that
 * has elements NULL (flags and ok may be); for the run every argument error of ezpz_system_tolerance_mc.  samples == 0: EZPZ_OK
 * after those checks, nothing written. */
#define EZPZ_SOBOL_MAX 32u
typedef struct EzpzSobolConfig { /* 16 bytes */
    uint64_t seed_b; /* matrix B's seed; default 0x9E3779B97F4A7C15 */
    uint64_t reserved;
} EzpzSobolConfig;
void ezpz_default_sobol_config(EzpzSobolConfig* sobol);
int ezpz_mc_sobol_indices(const double* sums, const uint64_t* n_complete, size_t n_param, size_t n_meas, double* var, double* first,
                          double* total, double* first_var, double* total_var);
int ezpz_mc_sobol_sums(const double* f, const uint8_t* flags, const uint8_t* ok, const double* nominal_m, uint32_t fixed_mask,
                       uint64_t samples, size_t n_param, size_t n_meas, uint32_t chunk, double* sums, uint64_t* n_complete);
int ezpz_mc_sobol_sums_device(const double* f_dev, const uint8_t* flags_dev, const uint8_t* ok_dev, const double* nominal_m_dev,
                              uint32_t fixed_mask, uint64_t samples, size_t n_param, size_t n_meas, uint32_t chunk, double* sums_dev,
                              uint64_t* n_complete_dev, void* stream);
int ezpz_system_tolerance_sobol(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const EzpzMcDist* dist,
                                const double* nominal, const EzpzConstraint* records, size_t n_meas, uint64_t samples,
                                const EzpzMcConfig* mc, const EzpzConfig* cfg, const EzpzSobolConfig* sobol, EzpzMcStats* stats,
                                EzpzMcTotals* totals, double* sums, uint64_t* n_complete, double* var, double* first, double* total,
                                double* first_var, double* total_var, double* keep_f, uint8_t* keep_flags, uint8_t* keep_ok);
int ezpz_system_tolerance_sobol_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                       const EzpzMcDist* dist, const double* nominal, const EzpzConstraint* records, size_t n_meas,
                                       uint64_t samples, const EzpzMcConfig* mc, const EzpzConfig* cfg, const EzpzSobolConfig* sobol,
                                       EzpzMcStats* stats_dev, EzpzMcTotals* totals_dev, double* sums_dev, uint64_t* n_complete_dev,
                                       double* var_dev, double* first_dev, double* total_dev, double* first_var_dev,
                                       double* total_var_dev, double* keep_f_dev, uint8_t* keep_flags_dev, uint8_t* keep_ok_dev,
                                       void* stream);

/* ---- Monte-Carlo quantiles: exact order statistics of a reference dimension, selected on the device (a project
 * extension).  mean and std describe a spread that is symmetric; a tolerance report asks where the 0.135 % and 99.865 % points and the
 * median are, and how sure those figures are at this sample count.  A selection is comparisons and integer counts: it has no floating
 * sum, so its output is the same bytes for any round size, any stream and any device, and on the host, with no order to prescribe.
 * VALIDITY.  Sample b is VALID FOR record i exactly as in the Monte-Carlo section: it is ok (the run: that section's rule;
 * ezpz_mc_quantiles: ok[b] != 0, ok == NULL: every one), flag bit 0 of (b, i) is clear (flags == NULL: every one) and m[b][i] is finite.
 * THE ORDER.  Values are ordered by key(m) = bits(m) ^ (bits(m) >> 63 ? ~0ull : 1ull << 63), compared as uint64: the total order on
 * finite doubles, with -0.0 before +0.0.  Equal keys are indistinguishable, so ties need no rule.  Sorted by key, the valid values of
 * record i are x_0 <= .. <= x_{n-1}, n = n_valid.
 * THE RANKS, for a probability p in [0, 1], each operation rounded once:
 *   h = p * (double)(n - 1);   k = (uint64)floor(h);   g = h - (double)k;   lo = x_k;   hi = x_{min(k + 1, n - 1)}
 *   value = g == 0 ? lo : lo + g * (hi - lo)      the product rounded, then added; no contraction on the host or on the device
 * THE BAND, distribution-free, for a call-wide z >= 0 (EzpzMcQuantileConfig; ezpz_default_mc_quantile_config: 0):
 *   s = sqrt(((double)n * p) * (1 - p));   a = h - z * s;   b = h + z * s
 *   k_lo = a <= 0 ? 0 : (uint64)floor(a);   k_hi = b >= (double)(n - 1) ? n - 1 : (uint64)ceil(b)
 *   band_lo = x_{k_lo};   band_hi = x_{k_hi}
 * THE OUTPUT.  out [n_meas][n_q], one EzpzMcQuantile per (record, probability): n_valid, rank = k, rank_lo = k_lo, rank_hi = k_hi,
 * frac = g, lo, hi, value, band_lo, band_hi.  With n == 0 the ranks are UINT64_MAX and the doubles NaN.
 * LIMITS.  n_q <= EZPZ_MC_QUANTILE_MAX_PROBS, n_meas <= EZPZ_MC_QUANTILE_MAX_MEAS, samples < 2^32.
 * ezpz_mc_quantiles[_device]: the selection alone on any kept rows -- m [samples][n_meas], flags [samples][n_meas] bytes, ok
 * [samples] bytes -- no system involved.  probs [n_q] and the config are host pointers in both forms.  The host form computes on the
 * host, with no device (a sort of the keys).  The _device form takes device pointers for m, flags, ok and out; it only enqueues on
 * `stream` and does not synchronise: a most-significant-digit radix select over the keys, eight digits of eight bits.  Digit pass 0
 * counts every valid key by its top byte, which gives n_valid; a closing kernel per record turns (n, probs, z) into at most four
 * target ranks per probability -- k, k + 1 clamped, k_lo, k_hi -- sorted and made distinct: at most 64 selections a record.  Every
 * digit pass is two launches: a count of the keys that carry a selection's prefix, by their next digit -- in LDS first, then global
 * integer atomics -- and the narrowing of every selection's prefix and rank by that digit.  After the last digit a prefix is the key
 * itself, and the same body as the host form's writes the records.  Nothing floating-point happens before that.  The workspace is
 * the library's, per device (a workspace that has to grow is first allocated behind the last call's launches); calls on one device
 * go one behind the other whatever their streams.
 * ezpz_system_tolerance_mc_quantiles[_device]: ezpz_system_tolerance_mc[_device] -- the same arguments, the same run, stats, totals,
 * hist and keep_* byte for byte -- plus probs, n_q, the config and out.  The run keeps m, flags and ok of EVERY sample on the device,
 * in the caller's keep_* buffers where the _device form is given them and else in the plan's workspace, and the selection follows
 * the last round on the same stream.  THE WORKSPACE COSTS samples x n_meas x 9 + samples BYTES: this is the one entry of the family
 * whose memory grows with `samples`, not with chunk.  The _device form takes a device pointer for out too.
 * EZPZ_ERR_INVALID_ARGUMENT with nothing enqueued and no output touched: a limit exceeded, or n_meas == 0; a p outside [0, 1] or not
 * finite; z negative or not finite; probs or out NULL with n_q > 0; m NULL with samples > 0; for the run every argument error of
 * ezpz_system_tolerance_mc.  samples == 0 or n_q == 0: EZPZ_OK after those checks, nothing written (the run with n_q == 0 is the
 * plain run). */
#define EZPZ_MC_QUANTILE_MAX_PROBS 16u
#define EZPZ_MC_QUANTILE_MAX_MEAS 64u
typedef struct EzpzMcQuantileConfig { /* 16 bytes */
    double z; /* >= 0: the band's half width in standard errors of the rank; default 0 */
    uint64_t reserved;
} EzpzMcQuantileConfig;
typedef struct EzpzMcQuantile { /* one per (record, probability); 80 bytes */
    uint64_t n_valid, rank, rank_lo, rank_hi;
    double frac, lo, hi, value, band_lo, band_hi;
} EzpzMcQuantile;
void ezpz_default_mc_quantile_config(EzpzMcQuantileConfig* qc);
int ezpz_mc_quantiles(const double* m, const uint8_t* flags, const uint8_t* ok, uint64_t samples, size_t n_meas, const double* probs,
                      size_t n_q, const EzpzMcQuantileConfig* qc, EzpzMcQuantile* out);
int ezpz_mc_quantiles_device(const double* m_dev, const uint8_t* flags_dev, const uint8_t* ok_dev, uint64_t samples, size_t n_meas,
                             const double* probs, size_t n_q, const EzpzMcQuantileConfig* qc, EzpzMcQuantile* out_dev, void* stream);
int ezpz_system_tolerance_mc_quantiles(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param,
                                       const EzpzMcDist* dist, const double* nominal, const EzpzConstraint* records, size_t n_meas,
                                       const double* lim_lo, const double* lim_hi, const double* hist_lo, const double* hist_hi,
                                       uint64_t samples, const EzpzMcConfig* mc, const EzpzConfig* cfg, EzpzMcStats* stats,
                                       EzpzMcTotals* totals, uint64_t* hist, double* keep_params, double* keep_m, uint8_t* keep_flags,
                                       uint8_t* keep_ok, const double* probs, size_t n_q, const EzpzMcQuantileConfig* qc,
                                       EzpzMcQuantile* out);
int ezpz_system_tolerance_mc_quantiles_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                              const EzpzMcDist* dist, const double* nominal, const EzpzConstraint* records,
                                              size_t n_meas, const double* lim_lo, const double* lim_hi, const double* hist_lo,
                                              const double* hist_hi, uint64_t samples, const EzpzMcConfig* mc, const EzpzConfig* cfg,
                                              EzpzMcStats* stats_dev, EzpzMcTotals* totals_dev, uint64_t* hist_dev,
                                              double* keep_params_dev, double* keep_m_dev, uint8_t* keep_flags_dev,
                                              uint8_t* keep_ok_dev, const double* probs, size_t n_q, const EzpzMcQuantileConfig* qc,
                                              EzpzMcQuantile* out_dev, void* stream);

/* ---- Monte-Carlo main effects: the conditional mean of a reference dimension per driving dimension, and first-order indices at the
 * price of the plain run (a project extension).  The contributors fit one slope to the curve "mean of reference dimension
 * i as a function of driving dimension j across its tolerance zone", the Sobol first-order index compresses it to one number; this
 * section returns the curve, binned, and from it the correlation ratio: the variance of the bin means over the total variance, which
 * estimates the same first-order index from the samples of the plain run alone -- no extra solves.
 * SHAPES.  k = n_param, m = n_meas, B = bins: 1 <= k, m <= 32; 2 <= B <= EZPZ_MC_EFFECT_MAX_BINS; k * B * m <= EZPZ_MC_EFFECT_MAX_CELLS.
 * THE BIN.  edges [k][B - 1], absolute values, non-decreasing per dimension; +-inf may stand (+inf edges leave the upper bins empty),
 * NaN is refused where the library reads the edges (host memory: every entry but ezpz_mc_effects_device).  bin(b, j) = the number
 * of edges of dimension j that are <= p[b][j]: comparisons alone, a function of the drawn value alone; a value on an edge goes to
 * the upper bin; a NaN p (possible only in ezpz_mc_effects[_device]) lands in bin 0, and so does everything under NaN edges.
 * THE CELLS.  For every (j, c, i) -- dimension, bin, record -- n (uint64), sum_d and sum_d2 over the samples that are VALID FOR
 * record i by the Monte-Carlo section's rule (ok -- ezpz_mc_effects: ok[b] != 0, ok == NULL: every one -- flag bit 0 of (b, i)
 * clear, flags == NULL: every one, and m[b][i] finite) and have bin(b, j) == c, with d = m[b][i] - nominal_m[i], one rounded
 * subtraction, and d * d rounded, then added.  THE ORDER OF EVERY SUM is the Monte-Carlo section's: block q is the samples [256 q,
 * 256 q + 256); a leaf is +0.0 for a sample that does not count for the cell or lies past `samples`; inside a block the 256 leaves
 * are summed by the adjacent-pair tree (for h = 1, 2, .. 128: v[t] += v[t + h] for every t that is a multiple of 2 h); the blocks'
 * sums are added left to right from +0.0.  No floating-point atomics, no product contracted into a fused multiply-add: the same bits
 * for any chunk, any stream and any device, and on the host.  A cell is therefore the sum_d / sum_d2 / n_valid of EzpzMcStats for the
 * run restricted to one bin of one dimension, and for every j the sum over c of n[j][c][i] equals stats[i].n_valid exactly.
 * Layout: sums [k][B][m][2] doubles (sum_d, sum_d2) and counts [k][B][m] uint64.
 * THE CLOSING STEP, ezpz_mc_effect_indices (host only, no device; the run's kernel has the same body and gives the same bits): a
 * pure function of sums, counts and nominal_m, from + - * /, comparisons and integer-to-double conversions alone, each line
 * evaluated as written, left to right; every loop ascends c and skips the empty cells (n_c == 0).  s_c, q_c, n_c: a cell's sum_d,
 * sum_d2 and n.
 *   cond_mean [k][B][m]:  nominal_m[i] + s_c / n_c;  NaN for an empty cell
 *   cond_var  [k][B][m]:  (q_c - s_c * s_c / n_c) / (n_c - 1), n_c - 1 formed as an integer;  NaN for n_c < 2
 *   per (i, j):  N = sum of n_c (an integer);  S = sum of s_c and Q = sum of q_c, each from +0.0;  used = the number of non-empty cells
 *   bins_used [m][k] (uint32) = used.   used < 2 (a FIXED dimension, all +inf edges, no valid sample): eta2 = first = +0.0.  Else:
 *   dbar = S / N;   SST = Q - S * S / N;   SSB = SSW = +0.0, then per non-empty cell:
 *     mu = s_c / n_c;   t = mu - dbar;   SSB = SSB + n_c * (t * t);   w_c = q_c - s_c * s_c / n_c;   SSW = SSW + w_c
 *   SST not > 0 (a constant record; NaN), or N - used < 1:  eta2 = first = NaN.  Else:
 *   eta2  [m][k] = SSB / SST
 *   first [m][k] = (SSB - (used - 1) * (SSW / (N - used))) / SST        N - used and used - 1 formed as integers
 * WHAT THE NUMBERS MEAN.  eta2 is the correlation ratio: the share of record i's sample variance that lies between the bin means of
 * dimension j.  It estimates the first-order Sobol index Var(E[m_i | p_j]) / Var(m_i) with two biases.  THE BINS' BIAS, downward: a
 * bin mean averages the curve over the bin, so the variance inside the bins is lost -- for a linear effect on B equal-width bins of
 * a uniform dimension 1 / B^2 of the index, more where the curve bends inside a bin; more bins lose less.  THE SAMPLING BIAS, upward:
 * the bin means of a dimension with no effect still scatter, by (used - 1) / (N - used) of the within-bin variance -- about
 * (B - 1) / N of the total; `first` subtracts exactly that (the adjusted ratio, (used - 1) mean squares within taken off SSB) and
 * is unbiased for a dimension with no effect.  It is not clamped and can be slightly negative.  More bins trade the first bias for
 * noise in the second's correction; 8 to 16 bins at a few thousand samples are a reasonable start.
 * ezpz_mc_effects[_device]: the reduction alone on any kept rows -- params [samples][n_param], m [samples][n_meas], flags (bytes,
 * the same shape, may be NULL), ok [samples] bytes (may be NULL), nominal_m [m], edges [k][B - 1] -- no system involved.  The host
 * form computes on the host, with no device, and gives the device form's bits; it has no rounds and ignores `chunk`.  The _device
 * form takes device pointers for every array, edges included (which it therefore cannot check: the bin rule holds whatever they
 * are), and only enqueues on `stream`, in rounds of `chunk` samples (rounded up to a multiple of 256; 0: 65536) on a workspace the
 * library owns per device (a workspace that has to grow is first allocated behind the last call's launches); calls on one device go
 * one behind the other whatever their streams.
 * ezpz_system_tolerance_mc_effects[_device]: ezpz_system_tolerance_mc[_device] -- the same arguments, the same run, stats, totals,
 * hist and keep_* byte for byte -- with one more kernel per round, behind the round's reduction, that folds the round's params, m,
 * flags and ok into sums and counts, and one closing kernel behind the last round that fills cond_mean, cond_var, eta2, first and
 * bins_used from them, with nominal_m the statistics' nominal[i].  ec (EzpzMcEffectConfig: bins; NULL: ezpz_default_mc_effect_config's
 * 8) and edges are host pointers in both forms; edges other than the last run's are first uploaded behind the last run's launches.
 * The _device form takes device pointers for the seven outputs too.  Not combined with contributors or quantiles in one call.
 * EZPZ_ERR_INVALID_ARGUMENT with nothing enqueued and no output touched: a shape outside the limits above (k == 0 and m == 0
 * included); an edge that is NaN or below its predecessor (host edges); with samples > 0: an output NULL, or an input NULL (flags and
 * ok may be) -- ezpz_mc_effect_indices: whatever samples --; for the run every argument error of ezpz_system_tolerance_mc.
 * samples == 0: EZPZ_OK after those checks, nothing written. */
#define EZPZ_MC_EFFECT_MAX_BINS 64u
#define EZPZ_MC_EFFECT_MAX_CELLS 4096u
typedef struct EzpzMcEffectConfig { /* 8 bytes */
    uint32_t bins; /* 2 .. 64; default 8 */
    uint32_t reserved;
} EzpzMcEffectConfig;
void ezpz_default_mc_effect_config(EzpzMcEffectConfig* ec);
int ezpz_mc_effect_indices(const double* sums, const uint64_t* counts, const double* nominal_m, size_t n_param, size_t n_meas,
                           uint32_t bins, double* cond_mean, double* cond_var, double* eta2, double* first, uint32_t* bins_used);
int ezpz_mc_effects(const double* params, const double* m, const uint8_t* flags, const uint8_t* ok, const double* nominal_m,
                    const double* edges, uint64_t samples, size_t n_param, size_t n_meas, uint32_t bins, uint32_t chunk, double* sums,
                    uint64_t* counts);
int ezpz_mc_effects_device(const double* params_dev, const double* m_dev, const uint8_t* flags_dev, const uint8_t* ok_dev,
                           const double* nominal_m_dev, const double* edges_dev, uint64_t samples, size_t n_param, size_t n_meas,
                           uint32_t bins, uint32_t chunk, double* sums_dev, uint64_t* counts_dev, void* stream);
int ezpz_system_tolerance_mc_effects(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const EzpzMcDist* dist,
                                     const double* nominal, const EzpzConstraint* records, size_t n_meas, const double* lim_lo,
                                     const double* lim_hi, const double* hist_lo, const double* hist_hi, uint64_t samples,
                                     const EzpzMcConfig* mc, const EzpzConfig* cfg, EzpzMcStats* stats, EzpzMcTotals* totals,
                                     uint64_t* hist, double* keep_params, double* keep_m, uint8_t* keep_flags, uint8_t* keep_ok,
                                     const EzpzMcEffectConfig* ec, const double* edges, double* sums, uint64_t* counts,
                                     double* cond_mean, double* cond_var, double* eta2, double* first, uint32_t* bins_used);
int ezpz_system_tolerance_mc_effects_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                            const EzpzMcDist* dist, const double* nominal, const EzpzConstraint* records, size_t n_meas,
                                            const double* lim_lo, const double* lim_hi, const double* hist_lo, const double* hist_hi,
                                            uint64_t samples, const EzpzMcConfig* mc, const EzpzConfig* cfg, EzpzMcStats* stats_dev,
                                            EzpzMcTotals* totals_dev, uint64_t* hist_dev, double* keep_params_dev, double* keep_m_dev,
                                            uint8_t* keep_flags_dev, uint8_t* keep_ok_dev, const EzpzMcEffectConfig* ec,
                                            const double* edges, double* sums_dev, uint64_t* counts_dev, double* cond_mean_dev,
                                            double* cond_var_dev, double* eta2_dev, double* first_dev, uint32_t* bins_used_dev,
                                            void* stream);

/* ---- Factorial effects: every main effect and every interaction of a 2^k corner run (a project extension).  A run
 * whose driving dimensions are all CORNER or FIXED is a full two-level factorial design: samples 0 .. 2^kc - 1 are the 2^kc corners.
 * One Walsh-Hadamard transform of its measured values gives the coefficient of every subset of dimensions, and from those the exact
 * variance decomposition of the two-point tolerance model -- first-order and total indices with no estimator variance, for the CORNER
 * dimensions ezpz_system_tolerance_sobol refuses -- which pair interacts, and whether the extreme corner is the one the linear signs
 * predict.  No extra solve.
 * SHAPES.  kc = n_corner, the number of CORNER dimensions, 1 <= kc <= EZPZ_MC_FACTORIAL_MAX_CORNERS; N = 2^kc rows; m = n_meas,
 * 1 <= m <= EZPZ_MC_FACTORIAL_MAX_MEAS.  Row b is the corner whose bit c is set when the CORNER dimension of rank c (its place among
 * the CORNER dimensions of the list) is at its b end: the Monte-Carlo section's definition.
 * VALIDITY is the Monte-Carlo section's: row b is VALID FOR record i when it is ok (ezpz_mc_factorial: ok[b] != 0, ok == NULL: every
 * one), flag bit 0 of (b, i) is clear (flags == NULL: every one) and m[b][i] is finite.  n_valid[i] counts the valid rows; record i is
 * COMPLETE when n_valid[i] == N.  For a record that is not complete every floating output of the record is NaN (0x7FF8000000000000),
 * its row of coef included, and its masks are 0.
 * THE VALUES.  y[b] = m[b][i] - nominal_m[i], one rounded subtraction.
 * THE TRANSFORM, in place on the N values w = y, for level l = 0, 1, .. kc - 1 with h = 2^l: for every b with bit l clear
 *   (w[b], w[b + h]) <- (w[b] + w[b + h], w[b + h] - w[b])          each one rounded operation, both on the old pair
 * then coef[S] = w[S] * 2^-kc.  So y(b) = sum over S of coef[S] * prod over c in S of s_c(b), s_c = +1 at the b end and -1 at the a
 * end; coef[0] is the mean deviation and 2 coef[1 << c] the classical main effect.  A butterfly's result depends on its two inputs
 * alone: no tiling, grid or pass structure can change a bit, and a host loop gives the device's bits.
 * THE OUTPUTS per record i:
 *   main [m][kc]          coef[1 << c]
 *   pair [m][kc][kc]      coef[(1 << c) | (1 << e)]; symmetric, the diagonal +0.0
 *   ss_order [m][kc + 1]  ss_order[o] = the sum over S with popcount(S) == o of coef[S] * coef[S], the product rounded, then added
 *   ss_total [m][kc]      the same sum over S with bit c set
 * THE ORDER OF THESE SUMS is the Monte-Carlo section's: the leaves are S = 0 .. N - 1, +0.0 where S is outside the class or past N;
 * block q is the leaves [256 q, 256 q + 256), summed by the adjacent-pair tree (for h = 1, 2, .. 128: v[t] += v[t + h] for every t that
 * is a multiple of 2 h); the blocks' sums are added left to right from +0.0.  No floating-point atomics.
 * THE CLOSING STEP, each line evaluated as written, loops ascending:
 *   var = ss_order[1] + .. + ss_order[kc], left to right from +0.0: the population variance of y over the corners (Parseval)
 *   first [m][kc] = (main[c] * main[c]) / var;   total [m][kc] = ss_total[c] / var;   both +0.0 when var == 0
 *   corner_hi: bit c set iff main[c] > 0;   corner_lo: bit c set iff main[c] < 0
 *   m_hi = m[corner_hi][i];   m_lo = m[corner_lo][i]      the measured values at the corners the linear signs call the maximum and
 *                                                       the minimum: compare with EzpzMcStats' max and min
 * info [m]: one EzpzMcFactorial per record -- n_valid, complete (0 or 1), corner_hi, corner_lo, mean_dev = coef[0], var, m_hi, m_lo.
 * coef [m][N] is optional: NULL, not returned.
 * ezpz_mc_factorial[_device]: the reduction alone on any kept rows -- m [N][n_meas], flags (bytes, the same shape, may be NULL), ok
 * [N] bytes (may be NULL), nominal_m [m] -- no system involved.  The host form computes on the host, with no device, and gives the
 * device form's bits.  The _device form takes device pointers for every array; it only enqueues on `stream` and does not
 * synchronise, on a workspace the library owns per device (n_meas x N doubles and the block sums; a workspace that has to grow is
 * first allocated behind the last call's launches); calls on one device go one behind the other whatever their streams.
 * ezpz_system_tolerance_mc_factorial[_device]: ezpz_system_tolerance_mc[_device] -- the same arguments, the same run, stats, totals,
 * hist and keep_* byte for byte -- plus the outputs above, with nominal_m the statistics' nominal[i].  Every dimension must be CORNER
 * or FIXED and samples must be 2^kc.  The run keeps m, flags and ok of every corner on the device, in the caller's keep_* buffers where
 * the _device form is given them and else in the plan's workspace, as the run with quantiles does, and the transform follows the last
 * round on the same stream.  The _device form takes device pointers for the outputs too.  Not combined with contributors, quantiles
 * or effects in one call.
 * EZPZ_ERR_INVALID_ARGUMENT with nothing enqueued and no output touched: n_corner == 0 or above the limit; n_meas == 0 or above the
 * limit; a required output or input NULL (flags, ok and coef may be); for the run: a dimension that is neither CORNER nor FIXED, no
 * CORNER dimension, samples other than 0 and 2^kc, with samples > 0 a required output NULL, and every argument error of
 * ezpz_system_tolerance_mc.  The run with samples == 0: EZPZ_OK after those checks, nothing written. */
#define EZPZ_MC_FACTORIAL_MAX_CORNERS 20u
#define EZPZ_MC_FACTORIAL_MAX_MEAS 32u
typedef struct EzpzMcFactorial { /* one per record; 56 bytes */
    uint64_t n_valid;
    uint32_t complete, corner_hi, corner_lo, reserved;
    double mean_dev, var, m_hi, m_lo;
} EzpzMcFactorial;
int ezpz_mc_factorial(const double* m, const uint8_t* flags, const uint8_t* ok, const double* nominal_m, uint32_t n_corner, size_t n_meas,
                      EzpzMcFactorial* info, double* main, double* pair, double* ss_order, double* ss_total, double* first,
                      double* total, double* coef);
int ezpz_mc_factorial_device(const double* m_dev, const uint8_t* flags_dev, const uint8_t* ok_dev, const double* nominal_m_dev,
                             uint32_t n_corner, size_t n_meas, EzpzMcFactorial* info_dev, double* main_dev, double* pair_dev,
                             double* ss_order_dev, double* ss_total_dev, double* first_dev, double* total_dev, double* coef_dev,
                             void* stream);
int ezpz_system_tolerance_mc_factorial(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param,
                                       const EzpzMcDist* dist, const double* nominal, const EzpzConstraint* records, size_t n_meas,
                                       const double* lim_lo, const double* lim_hi, const double* hist_lo, const double* hist_hi,
                                       uint64_t samples, const EzpzMcConfig* mc, const EzpzConfig* cfg, EzpzMcStats* stats,
                                       EzpzMcTotals* totals, uint64_t* hist, double* keep_params, double* keep_m, uint8_t* keep_flags,
                                       uint8_t* keep_ok, EzpzMcFactorial* info, double* main, double* pair, double* ss_order,
                                       double* ss_total, double* first, double* total, double* coef);
int ezpz_system_tolerance_mc_factorial_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                              const EzpzMcDist* dist, const double* nominal, const EzpzConstraint* records,
                                              size_t n_meas, const double* lim_lo, const double* lim_hi, const double* hist_lo,
                                              const double* hist_hi, uint64_t samples, const EzpzMcConfig* mc, const EzpzConfig* cfg,
                                              EzpzMcStats* stats_dev, EzpzMcTotals* totals_dev, uint64_t* hist_dev,
                                              double* keep_params_dev, double* keep_m_dev, uint8_t* keep_flags_dev,
                                              uint8_t* keep_ok_dev, EzpzMcFactorial* info_dev, double* main_dev, double* pair_dev,
                                              double* ss_order_dev, double* ss_total_dev, double* first_dev, double* total_dev,
                                              double* coef_dev, void* stream);

/* ---- Dimension targets: solve driving dimensions for measured targets (a project extension) -- the inverse of the
 * entries above: which values of the driving dimensions (the constraints at `positions`, as ezpz_system_solve_batch_params takes
 * them) put the reference dimensions `records` (measurement records, as ezpz_system_measure takes them; host memory in both forms)
 * on targets[b][i]?  A projected Levenberg-Marquardt iteration in parameter space, per system, every system of the batch on its
 * own.  x0 [batch][n_vars]: the starts, normally the current solution; params0 [batch][n_param]; targets [batch][n_meas].
 * EzpzSeekConfig: weight [n_meas] (>= 0; 0: the record is reported, not sought), tol [n_meas] (absolute, in the record's unit),
 * lo, hi [n_param] (+-inf allowed; lo == hi freezes a dimension), scale [n_param] (> 0: the size of a typical change, so degrees and
 * lengths mix) -- each array host memory, NULL = the default for every entry (1, 1e-6, -inf, +inf, 1).  ezpz_default_seek_config
 * fills: the arrays NULL, max_iterations 40, mu0 1e-3, mu_up 10, mu_down 0.1, mu_min 1e-12, mu_max 1e12, step_tol 1e-12, inner =
 * ezpz_default_config, sens_lambda = inner.initial_lambda, chunk 0.  These are POLICY DEFAULTS, not measurements.
 * THE ALGORITHM, for one system; w, t, tol indexed by record i, lo, hi, s (scale) by dimension r.  Only + - * /, comparisons and fabs
 * are used, no product is contracted into a fused multiply-add on either side, every sum runs i ascending from +0.0: the step is
 * the same bits on the host, on the device and in Python floats.  finite(v) is fabs(v) <= DBL_MAX.
 * EVALUATE(x_from, q): x = the solve of ezpz_system_solve_batch_params from x_from with q (cfg->inner); S, sens = the answer of
 *   ezpz_system_param_sensitivity at (x, q) with lambda = sens_lambda; m, flags = ezpz_system_measure at x; D = ezpz_system_
 *   measure_response of (x, S).  It is GOOD iff the solve has converged != 0 and n_unsatisfied == 0, sens == 0, no record with
 *   w > 0 has flag bit 0, and every m[i] and D[i][r] is finite.  e_i = w_i * (t_i - m_i); cost = sum of e_i * e_i; worst = the
 *   largest fabs(t_i - m_i) over the records with w_i > 0 (from +0.0); REACHED(m) iff fabs(t_i - m_i) <= tol_i for each of them.
 * START: p = clamp(params0) (v < lo ? lo : v > hi ? hi : v); EVALUATE(x0, p).  Not good: status START_FAILED, params_out = p, x_out =
 *   the x0 row, m_out NaN, cost0 = cost = worst = NaN, mu = mu0, and the system is finished.  Else commit (x, m, D, cost), cost0 =
 *   cost, mu = mu0, it = 0, and if REACHED(m): status REACHED.  Else go to NEXT.
 * NEXT, from the committed (p, m, D) with mu -- STEP is ezpz_seek_step:
 *   D'[i][r] = (w_i * D[i][r]) * s_r;  A[r][c] = sum_i D'[i][r] * D'[i][c];  g[r] = sum_i D'[i][r] * e_i.
 *   Dimension r is HELD for this step iff lo_r == hi_r, or p_r == lo_r and g_r < 0, or p_r == hi_r and g_r > 0; held dimensions are
 *   taken out of the system (the bound would only clip the step: a step along the others keeps the bound and still descends).
 *   amax = the largest A[r][r] over the free r (from +0.0; a NaN never wins);  f = 1e-2 * amax, raised to 1e-300 if below;
 *   M = A over the free dimensions with M[r][r] = A[r][r] + mu * (A[r][r] > f ? A[r][r] : f).  The relative floor keeps a dimension
 *   whose column of D (nearly) vanishes at this point from taking an unbounded step.
 *   M = L diag(d) L^T without square roots, free k ascending: d_k = M[k][k]; a d_k that is not > 0 or not finite: PIVOT.  Then for the
 *   free i > k and free j > k: M[i][j] = M[i][j] - (M[i][k] * M[j][k]) / d_k (the product first: both triangles keep the same bits).
 *   y = g; free k ascending: y_i = y_i - (M[i][k] / d_k) * y_k for the free i > k.  v_r = y_r / d_r.  Then free i descending:
 *   v_k = v_k - (M[i][k] / d_k) * v_i for the free k < i (M[i][k] as it stood when k was the pivot).  A v_r that is not finite: PIVOT.
 *   delta_r = s_r * v_r (held: +0.0);  q = p_r + delta_r;  p_trial_r = clamp(q) (held: p_r).
 *   MINIMUM iff no dimension is free, or fabs(delta_r) <= step_tol * (fabs(p_r) + step_tol) for every free r, or p_trial == p.
 *   The end tests, in this order: STEP says MINIMUM: status MINIMUM.  `stalled` is set: status STALLED.  it == max_iterations:
 *   status ITERATIONS.  Else it += 1, and on PIVOT the iteration is REJECTED (below) without a trial and NEXT runs again; else
 *   EVALUATE(the committed x, p_trial) and the iteration is ACCEPTED iff it is good and its cost < the committed cost.
 *   ACCEPTED: commit (p_trial, x, m, D, cost, worst); accepted += 1; mu = mu * mu_down, raised to mu_min if below; REACHED(m):
 *   status REACHED.  REJECTED: rejected += 1; if mu >= mu_max: stalled is set, else mu = mu * mu_up, lowered to mu_max if above.
 *   cost_trace[it] = the committed cost after iteration it, either way.  Then NEXT.
 * A seek never leaves its last accepted, assembled answer -- the promise guarded sweeps make: params_out, x_out, m_out are the last
 * commit's.  EzpzSeekInfo (48 bytes): status, iterations (it), accepted, rejected, cost0, cost, worst, mu.  cost_trace_out
 * (optional) [batch][1 + max_iterations]: [0] = cost0, [k] as above for k <= iterations, NaN beyond (all NaN on START_FAILED).
 * A finished system is frozen: later rounds evaluate it again and nothing of it is read, so a system's outputs depend on its own
 * inputs alone -- not on the batch, its place in it, the chunk, the stream, or how many rounds its neighbours need.
 * ezpz_seek_step (host only, no device; the lanes' one __host__ __device__ body, run lane after lane): STEP for p, m, targets and D
 * [n_meas][n_param] as ezpz_system_measure_response writes it, with cfg's weight, lo, hi, scale and step_tol.  Returns
 * EZPZ_SEEK_STEP_TRIAL, _MINIMUM or _PIVOT (on PIVOT p_trial = p and delta = +0.0), or an error; held_out (optional): bit r set
 * where dimension r was held.  Non-finite m, D entries are legal here and end, as the rules say, in PIVOT or a held dimension.
 * THE RUN is rounds on one stream.  A round is ezpz_system_solve_batch_params_device, ezpz_system_param_sensitivity_device,
 * ezpz_system_measure_device and ezpz_system_measure_response_device -- those entries themselves, with their routes (the fronts
 * included), locks, kept tables and ordering; a system the params or the sensitivity entry declines is declined here with the
 * same error before anything is enqueued -- then seek_step_kernel (verdict, bookkeeping, the next STEP; a team of 4, 8 or 16 lanes
 * per system by n_param) and seek_commit_kernel (the accepted rows of x).  The _device form enqueues 1 + max_iterations rounds per
 * chunk with no host read-back between them; the host form reads one counter of unfinished systems per round and stops at zero:
 * the same bytes, because finished systems are frozen.  chunk: systems per pass, rounded up to a multiple of 64 (0: the library's
 * choice, at most 65536 and few enough that S [chunk][n_param][n_vars] stays within 256 MiB); each chunk runs its whole loop.
 * EZPZ_ERR_TOO_LARGE: n_param > EZPZ_SEEK_MAX_PARAMS or n_meas > EZPZ_SEEK_MAX_TARGETS, max_iterations > 65535.  EZPZ_ERR_INVALID_ARGUMENT,
 * nothing enqueued, no output touched: the argument errors of the four entries (the list, the records, a system they decline, a
 * capture the fronts refuse); lo > hi or a NaN bound; a negative or non-finite weight or tol; a scale that is not > 0 and finite; a
 * non-finite target or params0 (host form); mu_up <= 1, mu_down >= 1 or <= 0, mu_min <= 0, mu_min > mu0 or mu0 > mu_max or any of
 * them not finite; a negative or non-finite step_tol or sens_lambda; a required pointer NULL (x0 with n_vars > 0, params0, targets,
 * params_out, x_out, m_out, info_out).  batch == 0, n_param == 0 or n_meas == 0: EZPZ_OK, nothing written, after the checks that need
 * no values.  The _device form takes device pointers for x0, params0, targets and every output (targets are then not checked), host
 * pointers for the rest.  x0 may be x_out itself, nothing else may overlap.  Tables other than the last run's, or a workspace that
 * has to grow, are uploaded behind the last run's launches first.  Runs on one EzpzSystem go one behind the other whatever their
 * streams; stream capture, thread safety and ordering against other launches: those of the four entries.  cfg == NULL: the defaults. */
#define EZPZ_SEEK_MAX_PARAMS 16u
#define EZPZ_SEEK_MAX_TARGETS 64u
#define EZPZ_SEEK_REACHED 0u
#define EZPZ_SEEK_MINIMUM 1u
#define EZPZ_SEEK_ITERATIONS 2u
#define EZPZ_SEEK_STALLED 3u
#define EZPZ_SEEK_START_FAILED 4u
#define EZPZ_SEEK_STEP_TRIAL 0
#define EZPZ_SEEK_STEP_MINIMUM 1
#define EZPZ_SEEK_STEP_PIVOT 2
typedef struct EzpzSeekConfig { /* 136 bytes */
    const double* weight; /* [n_meas] */
    const double* tol;    /* [n_meas] */
    const double* lo;     /* [n_param] */
    const double* hi;     /* [n_param] */
    const double* scale;  /* [n_param] */
    uint32_t max_iterations;
    uint32_t chunk;
    double mu0, mu_up, mu_down, mu_min, mu_max, step_tol, sens_lambda;
    EzpzConfig inner;
} EzpzSeekConfig;
typedef struct EzpzSeekInfo { /* one per system; 48 bytes */
    uint32_t status, iterations, accepted, rejected;
    double cost0, cost, worst, mu;
} EzpzSeekInfo;
void ezpz_default_seek_config(EzpzSeekConfig* cfg);
int ezpz_seek_step(size_t n_param, size_t n_meas, const double* p, const double* m, const double* D, const double* targets,
                   const EzpzSeekConfig* cfg, double mu, double* p_trial_out, double* delta_out, uint32_t* held_out);
int ezpz_system_seek_targets(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const double* params0,
                             const EzpzConstraint* records, size_t n_meas, const double* targets, size_t batch,
                             const EzpzSeekConfig* cfg, double* params_out, double* x_out, double* m_out, EzpzSeekInfo* info_out,
                             double* cost_trace_out);
int ezpz_system_seek_targets_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                    const double* params0_dev, const EzpzConstraint* records, size_t n_meas,
                                    const double* targets_dev, size_t batch, const EzpzSeekConfig* cfg, double* params_out_dev,
                                    double* x_out_dev, double* m_out_dev, EzpzSeekInfo* info_out_dev, double* cost_trace_out_dev,
                                    void* stream);

/* ---- Solution branches: sampled multi-start solves, their answers clustered on the device (a project extension).
 * A sketch usually has several configurations -- a triangle's apex on either side of its base, k such choices, 2^k assemblies -- and
 * a solve returns the one its start leads to.  These entries answer "which configurations exist, and which is nearest to my start":
 * `samples` starts scattered around a base x0 are solved in one launch per round, and what comes back is the B distinct answers
 * with the number of starts that reached each: small records, not samples x n_vars values.
 * THE RULE.  SAME BRANCH: samples i and j lie in one branch when, for every compared variable v,
 *   |x_i[v] - x_j[v]| <= eps_abs + eps_rel * max(|x_i[v]|, |x_j[v]|)
 * with the right side evaluated as written -- the product rounded, then the sum; never contracted into a fused multiply-add.
 * `compare` [n_vars] bytes choose the compared variables (non-zero: compared), NULL means all of them; the mask exists for
 * under-constrained sketches, whose free variables form a continuum.  The rule is comparisons only: there is no floating sum, so
 * nothing depends on an order of addition.  OK: a sample is ok when its flag is set -- its `ok` byte is non-zero (the clustering
 * alone) or its EzpzStatus has converged != 0 and n_unsatisfied == 0 (the run; the Monte-Carlo entry's rule) -- and its compared
 * values are finite.  BRANCHES are those of the SEQUENTIAL LEADER pass over the samples of a base in index order: an ok sample joins
 * the first (lowest-slot) leader whose branch it is in; otherwise it becomes the next leader while fewer than max_branches exist;
 * otherwise it is OVERFLOW.  Slots are in order of discovery, so a leader is the lowest sample index of its branch.  Membership is
 * tested against the LEADER, never against other members: the relation is not transitive, and the pass does not pretend it is.
 * tests/branch_ref.py restates the rule in a dozen lines.
 * EzpzBranchConfig: seed; chunk, the samples per base and round (0: the library's choice, 65536 or fewer where batch x n_vars is
 * large; rounded up to a multiple of 256 as the Monte-Carlo entry rounds its own); max_branches, 1 .. EZPZ_BRANCH_MAX (default 32);
 * eps_abs, eps_rel (default 1e-5 each).  WHERE 1e-5 COMES FROM: on chains of 2, 3 and 5 triangles and on 2 and 3 independent
 * triangle blocks, 256 and 1024 uniform starts each, the answers of one branch differed by at most 1.1e-7 in the max-norm under the
 * default EzpzConfig (the LM loop stops at residual_tolerance 1e-8) and distinct branches by at least 3.87; labels at 1e-6 and 1e-4
 * were identical.  The default is about 100 x that spread.  A looser residual_tolerance wants a looser eps.
 * OUTPUTS.  info [batch]: samples; n_ok; n_branches; n_overflow.  branches [batch][max_branches], one EzpzBranch per slot: first, the
 * leader's sample index; count, the samples in the branch (the leader included); dist_inf, the largest |x_leader[v] - origin[v]| over
 * the compared variables -- a maximum from +0.0, not a sum; a NaN difference never wins -- where the origin is x0[b] for the run and
 * sample 0 of the base for the clustering alone; status, the leader's EzpzStatus (all zero for the clustering alone).  x_branch
 * [batch][max_branches][n_vars]: the leaders' full answers, uncompared variables included.  keep_label [batch][samples] int32
 * (optional, NULL): the sample's slot, EZPZ_BRANCH_NOT_OK (-1) or EZPZ_BRANCH_OVERFLOW (-2).  Slots at and beyond n_branches are
 * zero-filled.  n_ok = the sum of the counts + n_overflow.
 * ezpz_branch_cluster[_device] is the clustering alone on the caller's data, x [batch][samples][n_vars] with ok [batch][samples]
 * bytes (NULL: every flag set) -- no system involved; useful on the kept samples of a Monte-Carlo run.
 * ezpz_system_solve_branches[_device] is THE RUN: every base x0[b] ([batch][n_vars]) gets `samples` starts.  Sample 0 is x0[b]
 * itself, so slot 0 is what the plain solve finds whenever that assembles; sample s >= 1 starts at the draw of (seed, s, v) by dist[v]
 * (EzpzMcDist, the sampler of the Monte-Carlo section) around the nominal x0[b][v]: ezpz_mc_sample(seed, dist, x0[b], n_vars, first,
 * count) reproduces the starts on the host, bitwise for FIXED / UNIFORM / CORNER, and a FIXED variable keeps its value.  Rounds of
 * `chunk` samples per base (round 0 is at most 1024: it meets no leaders) run on one stream: the start kernel,
 * ezpz_system_solve_batch_device on batch x count systems -- that entry itself, whatever kernel serves the system, and an error it
 * returns is returned here -- then the clustering of the round: branch_assign_kernel compares every sample with the leaders known
 * when the round begins, branch_elect_kernel (one workgroup per base) runs the leader pass over what is left.  The leader table
 * persists in `branches` and `x_branch` between rounds: every output has the same bytes for any chunk and any stream, given the same
 * answers of the solve entry (see there for when those depend on a call's size).  Memory is bounded by batch x chunk, not by samples;
 * the host form of the clustering alone holds the caller's x on the device whole.
 * EZPZ_ERR_INVALID_ARGUMENT with nothing enqueued and no output touched: max_branches 0 or above EZPZ_BRANCH_MAX; a negative or
 * non-finite eps; a `compare` that selects nothing (n_vars == 0 included); every error of ezpz_mc_sample for dist (the host form
 * checks it with every x0 row as the nominal, the _device form, which cannot read x0, with zeros); sys NULL; x (or x0), info, branches
 * or x_branch NULL with batch > 0 and samples > 0.  EZPZ_ERR_TOO_LARGE, likewise: samples >= 2^48, batch >= 2^32, or a round of
 * more than 2^40 values (batch x chunk x n_vars; the index arithmetic's bounds).  samples == 0 or batch == 0: EZPZ_OK after those checks, nothing written.
 * The _device forms take device pointers for x, ok, x0 and every output, host pointers for compare, dist and the configs, and only
 * enqueue on `stream` once the tables are the last run's and the workspace is large enough (else those are first uploaded behind the
 * last run's launches).  Runs on one EzpzSystem -- and clusterings on one device, whose workspace is the process's -- go one behind
 * the other whatever their streams.  Stream capture, thread safety and the ordering against other launches on the system: those of
 * the solve entry.  cfg / bcfg == NULL: ezpz_default_branch_config's values; cfg of the run as for the solve entry. */
#define EZPZ_BRANCH_MAX 256u
#define EZPZ_BRANCH_NOT_OK (-1)
#define EZPZ_BRANCH_OVERFLOW (-2)
typedef struct EzpzBranchConfig { /* 32 bytes */
    uint64_t seed;
    uint32_t chunk;        /* samples per base and round; 0 = the library's choice */
    uint32_t max_branches; /* 1 .. EZPZ_BRANCH_MAX */
    double eps_abs, eps_rel;
} EzpzBranchConfig;
typedef struct EzpzBranchInfo { /* one per base; 32 bytes */
    uint64_t samples, n_ok, n_branches, n_overflow;
} EzpzBranchInfo;
typedef struct EzpzBranch { /* one per slot; 56 bytes */
    uint64_t first, count;
    double dist_inf;
    EzpzStatus status;
} EzpzBranch;
void ezpz_default_branch_config(EzpzBranchConfig* bcfg);
int ezpz_branch_cluster(const double* x, const uint8_t* ok, const uint8_t* compare, size_t batch, uint64_t samples, size_t n_vars,
                        const EzpzBranchConfig* cfg, EzpzBranchInfo* info, EzpzBranch* branches, double* x_branch,
                        int32_t* keep_label);
int ezpz_branch_cluster_device(const double* x_dev, const uint8_t* ok_dev, const uint8_t* compare, size_t batch, uint64_t samples,
                               size_t n_vars, const EzpzBranchConfig* cfg, EzpzBranchInfo* info_dev, EzpzBranch* branches_dev,
                               double* x_branch_dev, int32_t* keep_label_dev, void* stream);
int ezpz_system_solve_branches(EzpzSystem* sys, const double* x0, const EzpzMcDist* dist, const uint8_t* compare, size_t batch,
                               uint64_t samples, const EzpzBranchConfig* bcfg, const EzpzConfig* cfg, EzpzBranchInfo* info,
                               EzpzBranch* branches, double* x_branch, int32_t* keep_label);
int ezpz_system_solve_branches_device(EzpzSystem* sys, const double* x0_dev, const EzpzMcDist* dist, const uint8_t* compare,
                                      size_t batch, uint64_t samples, const EzpzBranchConfig* bcfg, const EzpzConfig* cfg,
                                      EzpzBranchInfo* info_dev, EzpzBranch* branches_dev, double* x_branch_dev,
                                      int32_t* keep_label_dev, void* stream);

/* ---- ezpz::solve for a batch (new; SURVEY.md 8f #3: priority tiers + weights end-to-end on device batches) --------
 * `batch` systems share the request list and differ in their guesses (x0 AoS [batch][n_vars], id == index).  Per
 * system exactly the semantics of ezpz_solve: LineSide / CircleSide inferred from that system's own guesses
 * (constraints.rs:146-193; systems are grouped by the inferred sides), cumulative priority tiers each re-solved from
 * the original guesses (lib.rs:215-246), the last fully satisfied tier is returned.  priority_solved [batch] and
 * unsat_mask [batch][n_reqs] (indexed by position in `reqs`) are optional.  Topology-level errors (missing guess ...)
 * in the first tier fail the call; in a later tier every system keeps its previous tier, like the reference. */
int ezpz_solve_batch(const EzpzConstraint* reqs, size_t n_reqs, size_t n_vars, const double* x0, size_t batch,
                     const EzpzConfig* cfg, double* x_out, EzpzStatus* status, uint32_t* priority_solved,
                     uint8_t* unsat_mask, int32_t* err_constraint, int64_t* err_variable);

/* ---- one batch over several devices of a node (new; SURVEY.md 8b last row, 8e) ------------------------------------------
 * The reference's caller is a host loop over independent solves (ezpz-cli/src/main.rs:96-98); independent systems have
 * no exchange step, so a batch shards contiguously over the devices of `device_mask` (bit d = HIP device d; 0 = every
 * device of the node): device index g of G gets systems [g * ceil(batch / G), ...), trailing devices may be short or
 * idle.  One host worker thread and one analysed topology (an EzpzSystem) per device; every shard moves over its own
 * device's host link, straight between the caller's buffers and that device -- no peer copies, no collective -- through
 * the single-device path of ezpz_system_solve_batch (registered caller buffers, ezpz_host_register, are pipelined on
 * every device at once).  Results are those of ezpz_system_solve_batch on each shard: a kernel is chosen by the size of the
 * call it serves (lanes across the batch from 64 x 4 x CUs systems, run-time compilation from 1024), so a shard may run on
 * another kernel of its topology than the whole batch would on one device -- bit-identical for component-resident block
 * systems, equal to rounding (and in iteration counts) for connected sketches.
 * `cs` is one side-resolved tier as for ezpz_system_create.  A handle serves one batch call at a time (calls from
 * several threads queue); ezpz_multi_specialize is ezpz_system_specialize on every device (the smallest state is returned).
 * ezpz_multi_shard tells which systems device index `index` takes of a batch.
 * ezpz_system_solve_batch_multi is the same in one call: the handles live in a small cache keyed by the request bytes
 * and the mask (dropped by ezpz_cache_clear). */
typedef struct EzpzMultiSystem EzpzMultiSystem; /* opaque: one analysed topology resident on several devices */
int ezpz_multi_create(const EzpzConstraint* cs, size_t n_cs, size_t n_vars, uint64_t device_mask, uint32_t team_size,
                      EzpzMultiSystem** out, int32_t* err_constraint, int64_t* err_variable);
void ezpz_multi_destroy(EzpzMultiSystem* multi);
int ezpz_multi_device_count(const EzpzMultiSystem* multi);        /* G */
int ezpz_multi_device(const EzpzMultiSystem* multi, int index);  /* HIP device of device index `index`, -1 out of range */
void ezpz_multi_shard(const EzpzMultiSystem* multi, size_t batch, int index, size_t* first, size_t* count);
int ezpz_multi_specialize(EzpzMultiSystem* multi, int wait);
int ezpz_multi_solve_batch(EzpzMultiSystem* multi, const double* x0, size_t batch, const EzpzConfig* cfg, double* x_out,
                           EzpzStatus* status, uint8_t* unsat_mask);
int ezpz_system_solve_batch_multi(const EzpzConstraint* cs, size_t n_cs, size_t n_vars, uint64_t device_mask,
                                  const double* x0, size_t batch, const EzpzConfig* cfg, double* x_out, EzpzStatus* status);

/* ---- one batch of systems of DIFFERENT topologies (new; SURVEY.md 8b last row) -------------------------------------------
 * The reference's callers loop over arbitrary systems, one solve() after the other (ezpz-cli/src/main.rs:96-98,
 * ezpz-wasm/src/lib.rs:96); this is that loop as one call.  System b of the batch has the topology
 * handles[topology_of_system[b]] (side-resolved tiers, all on the calling thread's current device); the batch is RAGGED:
 * x0 / x_out hold the systems' rows one after the other in batch order, system b's n_vars(b) values at
 * x_offset[b] = sum of n_vars over the systems before it (ezpz_mixed_offsets gives the batch + 1 offsets,
 * ezpz_mixed_total_values their last entry).  Inside, the batch is regrouped by topology -- each topology's rows gathered
 * into one block, solved by that topology's kernels on a stream of its own, scattered back -- and every result is the one
 * ezpz_system_solve_batch gives for that system's topology, bit for bit, in caller order.
 * An EzpzMixedBatch is the grouping of one (handles, topology_of_system) pair, reusable for any number of solves (one at
 * a time; the handles must outlive it); the _device form takes device pointers and only enqueues on `stream`;
 * ezpz_system_solve_batch_mixed is create + solve + destroy in one call.  ezpz_multi_solve_batch_mixed shards the
 * batch contiguously (by systems) over the devices the EzpzMultiSystems share -- multis[t] is topology t on every device
 * of one mask -- each device running its shard through the single-device path over its own host link. */
typedef struct EzpzMixedBatch EzpzMixedBatch;
int ezpz_mixed_create(EzpzSystem* const* handles, size_t n_handles, const uint32_t* topology_of_system, size_t batch,
                      EzpzMixedBatch** out);
void ezpz_mixed_destroy(EzpzMixedBatch* mixed);
size_t ezpz_mixed_total_values(const EzpzMixedBatch* mixed);
void ezpz_mixed_offsets(const EzpzMixedBatch* mixed, uint64_t* x_offset /* batch + 1 */);
int ezpz_mixed_solve_device(EzpzMixedBatch* mixed, const double* x0_dev, const EzpzConfig* cfg, double* x_out_dev,
                            EzpzStatus* status_dev, void* stream);
int ezpz_mixed_solve(EzpzMixedBatch* mixed, const double* x0, const EzpzConfig* cfg, double* x_out, EzpzStatus* status);
int ezpz_system_solve_batch_mixed(EzpzSystem* const* handles, size_t n_handles, const uint32_t* topology_of_system,
                                  const double* x0, size_t batch, const EzpzConfig* cfg, double* x_out, EzpzStatus* status);
int ezpz_multi_solve_batch_mixed(EzpzMultiSystem* const* multis, size_t n_multis, const uint32_t* topology_of_system,
                                 const double* x0, size_t batch, const EzpzConfig* cfg, double* x_out, EzpzStatus* status);

/* Constraint::set_from_initial_values (ezpz/src/constraints.rs:146-193) over a request list, in place: every
 * LineTangentToCircle / CircleTangentToCircle whose side is EZPZ_SIDE_UNDEFINED gets the side the values imply
 * (values by id, id == index).  ezpz_solve / ezpz_solve_batch do this themselves; callers of the handle API
 * (ezpz_system_create takes side-resolved tiers) use this first. */
int ezpz_resolve_sides(EzpzConstraint* cs, size_t n_cs, const double* values, size_t n_vars);

/* ---- class-specialised kernels ------------------------------------------------------------------------------------
 * Systems that run component-resident (EzpzSystemInfo.team_mode 3) can have their kernel compiled at run time
 * (hiprtc) into straight-line code for exactly their classes of components: same operations in the same order,
 * state in registers instead of LDS.  Batch calls of >= 1024 systems start that compilation on a background thread
 * (so do topologies solved more than 256 times, one call after the other: an interactive sketch) and switch to the
 * specialised kernel once it is ready (results are bit-identical either way for component-resident systems; the
 * lane-per-system form sums residuals in request order, i.e. agrees to rounding); EZPZ_JIT=0 in the
 * environment turns it off.  ezpz_system_specialize starts it explicitly and, with wait != 0, returns when it is
 * done: 2 = ready, 1 = still compiling, 0 = this system has no specialised form, negative = compilation failed.
 * Compiled code objects are kept on disk ($EZPZ_JIT_CACHE_DIR, else $XDG_CACHE_HOME/ezpz_amd, else
 * $HOME/.cache/ezpz_amd; EZPZ_JIT_CACHE=0 turns the cache off), keyed by the generated source, the embedded device
 * headers, the compiler options and the hiprtc version: a process that finds its kernel there has it from its first few
 * solves (a system's first launch asks the cache in the background) instead of after 256 solves and a compilation.
 * Budget: a loaded code object is never unloaded, so a process holds at most 512 specialised kernels (distinct
 * topologies; systems with the same generated source share one).  Beyond that ezpz_system_specialize returns
 * EZPZ_ERR_KERNEL_BUDGET and batch calls keep running on the interpreting kernels (same results, lower rate).
 * ezpz_specialized_source (no device needed) writes the generated source of a request into buf (NUL-terminated,
 * truncated to cap) and returns its length, 0 when the request gets no component plan; with compile != 0 it also
 * compiles it for gfx950 (compile == 2: through the on-disk cache, like the solve entry points) and returns a negative
 * error with the compiler's log in buf on failure. */
int ezpz_system_specialize(EzpzSystem* sys, int wait);
long ezpz_specialized_source(const EzpzConstraint* cs, size_t n_cs, size_t n_vars, int compile, char* buf, size_t cap);

/* ezpz_solve, ezpz_solve_analysis, ezpz_solve_inner and ezpz_solve_batch keep one small cache of request plans keyed by
 * the request bytes (tiers, lint, validation, the analysed topology of every tier and choice of inferred sides), so that
 * repeated solves of one problem (ezpz-cli's 100-run loop, main.rs:96-98) skip the symbolic phase.  This drops
 * it, and the handles behind ezpz_system_solve_batch_multi (used to time cold solves). */
void ezpz_cache_clear(void);

/* The launch-shape thresholds (csrc/policy.hpp has each number's measurement): what decides which kernel serves a call,
 * for a device of `compute_units` CUs.  "systems per call that fill the device" scale with the CU count; what belongs to
 * one workgroup or one CU's LDS does not.  ezpz_launch_policy(0, ...) = the full 256-CU MI355X. */
typedef struct EzpzLaunchPolicy {
    uint32_t compute_units;
    /* scaled by the CU count */
    uint64_t lanes_min_systems_small;  /* systems per call from which a connected sketch runs one lane per system (64 x 4 x CUs) */
    uint64_t lanes_min_systems_large;  /* ... a sketch of >= lanes_large_from_vars variables (64 x 2 x CUs) */
    uint32_t lanes_large_from_vars;
    uint64_t jit_lane_min_batch;       /* a call this large starts the run-time compilation at once: one lane per system (16 x CUs) */
    uint64_t jit_comp_min_batch;       /* ... component-resident block systems (4 x CUs) */
    uint64_t jit_comp_min_values;      /* ... or this many variables in the call (8192 x CUs) */
    /* not scaled */
    uint32_t jit_after_launches;       /* smaller calls earn the compilation by repetition */
    uint32_t lane_max_vars, lane_max_constraints;
    uint32_t comp_min_components, comp_max_component_vars, comp_max_component_constraints, comp_max_classes;
    uint32_t rec_min_vars_one_solve, rec_min_vars_batch, rec_one_wavefront_max_vars, rec_max_components;
    uint32_t rec_wide_one_solve_max_vars;
    uint32_t sub_team_max_width, dense8_max_vars;
    uint64_t zero_copy_max_bytes, h2h_piece_min_bytes, h2h_piece_max_bytes;
    uint32_t h2h_pieces_per_call;
    uint32_t one_call_host_mask_max_constraints, one_call_host_log_max_entries;
    /* the frontal shape (team_mode 5): one solve of a connected sketch takes it from this many variables; a system created for
     * batches (team_size 0) carries the plan from that many (0 = never) and takes it for calls of up to
     * EzpzSystemInfo.front_max_batch systems (= the systems the device holds at once, compute units / workgroups per system, times
     * max(1, workgroups per system / front_small_call_wgs_per_round) rounds); one workgroup per system up to
     * front_vars_per_workgroup x 2 variables, then one more per that many */
    uint32_t front_min_vars_one_solve, front_min_vars_batch, front_vars_per_workgroup, front_max_workgroups;
    uint32_t front_small_call_wgs_per_round;
} EzpzLaunchPolicy;
int ezpz_launch_policy(int compute_units, EzpzLaunchPolicy* out);

/* Diagnostic: per-stage time stamps of the calling thread's ezpz_solve* calls.  While `buf` is set, every stage boundary of
 * the one-call path appends an (id, CLOCK_MONOTONIC nanoseconds) pair (ids: csrc/call_trace.hpp, CallStage) up to `cap`
 * words; buf == NULL turns it off.  Returns the number of words written since the previous call
 * (tools/solve_call_breakdown.py -> profiles/r04_solve_call_breakdown.txt). */
size_t ezpz_debug_call_trace(uint64_t* buf, size_t cap);

/* Diagnostic: a device buffer for in-kernel time stamps, NULL to stop (the -DEZPZ_STAMPS builds of the list-walk and frontal
 * kernels: tools/front_stamps.py; the run-time compiled kernel of a system on several workgroups when the process runs with
 * EZPZ_JIT_STAMPS=1: tools/ladder_stamps.py).  Not for production callers. */
void ezpz_debug_set_stamps(unsigned long long* dev_buf);

/* Diagnostic: how this process's FreedomAnalysis calls by null-space probes ended (csrc/freedom.hip: freedom_by_probes): out8[0]
 * systems decided fully constrained by the first eight probes, [1] decided with null vectors found, [2] calls that took the
 * second opinion at lambda / 1000; calls handed to the pivoted QR because [3] an answer was not finite, [4] five or more
 * candidate directions, [5] a direction undecided at both lambdas, [6] an unsettled direction, [7] probes not applicable. */
void ezpz_debug_freedom_exits(unsigned long long* out8);

/* Diagnostic: run-time compilations (hiprtc) this process has performed so far -- a kernel found in the on-disk cache of code
 * objects does not count (tests/test_abi_cpu.py::test_code_object_cache_on_disk). */
unsigned long long ezpz_debug_jit_compilations(void);

/* Diagnostic (host only, no device needed): the symbolic phase of the FRONTAL launch shape (team_mode 5, csrc/fronts.cpp:
 * the supernodal counterpart of faer's SymbolicLlt, solver.rs:289-300) for `wgs` workgroups per system (0 = automatic) on
 * workgroups of `lds_bytes` of LDS.  Copies the plan's device blob into buf (up to cap bytes) and fills info[0..15] =
 * workgroups, scratch chunks, first pivot-flag chunk, verdict chunk, LDS bytes, fronts, levels, largest front's rows /
 * pivots, lanes per workgroup, modelled cycles, panel doubles, update doubles, 0...; returns the blob's size, 0 when the
 * shape does not apply to the system, or a negative EZPZ_ERR_*.  tests/front_ref.py executes the blob in numpy. */
long ezpz_debug_front_plan(const EzpzConstraint* cs, size_t n_cs, size_t n_vars, uint32_t wgs, uint32_t max_wgs,
                           uint64_t lds_bytes, unsigned char* buf, size_t cap, uint64_t* info);
/* Diagnostic (host only): the tables the sensitivity route of the fronts derives from that plan for a `positions` list
 * (csrc/front_sens_types.hpp: the rhs-only assembly streams, the rhs-only extend-add of every front, the home of each listed
 * constraint), as 32-bit words; info[0..3] = workgroups, words, the plan blob's bytes, 0.  Returns the tables' size in bytes, 0
 * when the shape does not apply, or a negative EZPZ_ERR_*.  tests/front_sens_ref.py executes them in numpy. */
long ezpz_debug_front_sens_tables(const EzpzConstraint* cs, size_t n_cs, size_t n_vars, uint32_t wgs, uint32_t max_wgs,
                                  uint64_t lds_bytes, const uint32_t* positions, size_t n_param, unsigned char* buf, size_t cap,
                                  uint64_t* info);

/* ---- textual front end, ezpz/src/textual.rs:43-49 (Problem: FromStr) + executor.rs:40-445 ------------ */
typedef struct EzpzProblem EzpzProblem; /* opaque: parsed + lowered problem text */
int ezpz_problem_parse(const char* text, size_t len, EzpzProblem** out, char* errbuf, size_t errcap);
void ezpz_problem_destroy(EzpzProblem* p);
size_t ezpz_problem_num_constraints(const EzpzProblem* p);
size_t ezpz_problem_num_vars(const EzpzProblem* p);
const EzpzConstraint* ezpz_problem_constraints(const EzpzProblem* p);
const double* ezpz_problem_guesses(const EzpzProblem* p); /* values by id (id == index) */
/* label tables, executor.rs:521-566: kind 0 = points, 1 = circles, 2 = arcs */
size_t ezpz_problem_num_labels(const EzpzProblem* p, int kind);
const char* ezpz_problem_label(const EzpzProblem* p, int kind, size_t index);
/* the `line(p, q)` instructions, in the text's order (parser.rs:46-48, inner_lines), as indices into the point labels (kind 0):
 * what the reference draws as strokes.  A line whose label is no declared point is not kept.  ezpz_problem_line: EZPZ_OK, or
 * EZPZ_ERR_INVALID_ARGUMENT for a NULL argument or i past the last line. */
size_t ezpz_problem_num_lines(const EzpzProblem* p);
int ezpz_problem_line(const EzpzProblem* p, size_t i, size_t* point_a, size_t* point_b);

/* ---- Sketch images: many variants of one drawing list accumulated into an integer image (the counterpart of the
 * reference's ezpz-cli/src/visualize.rs, without its axes, mesh and text) --------------------------------------------------------
 * x [batch][n_vars]: the values of `batch` variants of one sketch -- one solution, the steps of a sweep, the branches, the
 * samples of a tolerance run; ok [batch] or NULL: a variant whose byte is 0 draws nothing.  items [n_items] and view: host memory
 * in every form.  counts [n_layers][height][width], uint32: the number of (variant, item) pairs of that layer that cover the
 * pixel -- two items of one variant on one pixel count twice; row 0 is y_min.  accumulate != 0 adds to what counts and info
 * hold, otherwise both are zeroed first (also with batch == 0 or n_items == 0); a count that wraps over several accumulating calls
 * is the caller's business.
 * THE RULE.  Only + - * /, fabs and comparisons, every operation rounded once in the order written (no unit of the library
 * contracts a product into a fused multiply-add): the host body, the kernel and numpy decide every pixel alike, and the counts
 * are integers, so the bytes do not depend on the batch, the chunk, the stream or the placement.
 * A value pair (x, y) is in pixel space u = (x - x_min) * scale, v = (y - y_min) * scale; the centre of pixel (px, py) is
 * (X, Y) = (px + 0.5, py + 0.5); h = half_width.  ids per kind, unused ones 0:
 *   POINT    x, y.  dx = X - u; dy = Y - v; covered iff dx*dx + dy*dy <= h*h.
 *   SEGMENT  ax, ay, bx, by.  ex = bu - au; ey = bv - av; L2 = ex*ex + ey*ey; wx = X - au; wy = Y - av; t = wx*ex + wy*ey.
 *            L2 == 0 || t <= 0: covered iff wx*wx + wy*wy <= h*h.  Else t >= L2: zx = X - bu; zy = Y - bv; covered iff
 *            zx*zx + zy*zy <= h*h.  Else cr = wx*ey - wy*ex; covered iff cr*cr <= (h*h)*L2.  (A capsule.)
 *   CIRCLE   cx, cy, r.  R = fabs(r) * scale; wx = X - u; wy = Y - v; d2 = wx*wx + wy*wy; R2 = R*R.  With EZPZ_DRAW_FILL: hi =
 *            R + h; covered iff d2 <= hi*hi.  Else the ring: q = (d2 + R2) - h*h; covered iff q <= 0 || q*q <= (4.0*d2)*R2.
 *   ARC      cx, cy, ax, ay, bx, by: the minor arc from a to b about c with the radius |a - c| (visualize.rs:289-302).  px = au -
 *            cu; py = av - cv; qx = bu - cu; qy = bv - cv; R2 = px*px + py*py; wx = X - cu; wy = Y - cv; the ring as for the
 *            circle, and the sector: s = px*qy - py*qx; c1 = px*wy - py*wx; c2 = wx*qy - wy*qx.  s > 0: c1 >= 0 && c2 >= 0.
 *            s < 0: c1 <= 0 && c2 <= 0.  s == 0 with px*qx + py*qy > 0: nothing.  s == 0 otherwise: c1 >= 0 (the half-turn
 *            counter-clockwise from a).  The ends are radial cuts, without caps.
 * An item of a variant is skipped when one of its pixel-space numbers (every u and v, the circle's R) is not finite or above
 * 2^30 in magnitude; the items of a variant that draws nothing are not looked at.
 * EzpzImageInfo: variants -- the batch; masked -- variants whose ok byte is 0; items_skipped; increments -- the sum of everything
 * added to counts, a checksum.
 * ezpz_sketch_image_device: device pointers for x, ok, counts and info, the current device, a hipStream_t; it takes no system.  It
 * enqueues only once the item list is the last call's (another list waits for the earlier launches and is copied).
 * ezpz_sketch_image: the same through host pointers.  ezpz_sketch_image_host: the rule alone, plain loops over every pixel of the
 * view on the host; it needs no device.
 * EZPZ_ERR_INVALID_ARGUMENT with nothing enqueued and no output touched: view, counts or info NULL; items NULL with n_items > 0;
 * x NULL with batch > 0 and n_items > 0; n_layers outside 1 .. 8; width or height outside 1 .. 16384; a scale that is not finite
 * and > 0; x_min or y_min not finite; a kind above EZPZ_DRAW_ARC; a layer >= n_layers; a flag other than EZPZ_DRAW_FILL, or
 * EZPZ_DRAW_FILL on another kind than CIRCLE; a used id >= n_vars; a half_width that is not finite and >= 0.  EZPZ_ERR_TOO_LARGE:
 * batch * n_items >= 2^32. */
#define EZPZ_DRAW_POINT 0
#define EZPZ_DRAW_SEGMENT 1
#define EZPZ_DRAW_CIRCLE 2
#define EZPZ_DRAW_ARC 3
#define EZPZ_DRAW_FILL 1u
#define EZPZ_IMAGE_MAX_LAYERS 8u
#define EZPZ_IMAGE_MAX_SIDE 16384u
typedef struct EzpzImageView { /* 32 bytes; isotropic: a circle stays a circle */
    double x_min, y_min, scale;
    uint32_t width, height;
} EzpzImageView;
typedef struct EzpzDrawItem { /* 40 bytes */
    uint16_t kind;
    uint8_t layer;
    uint8_t flags;
    uint32_t ids[6];
    double half_width; /* pixels; POINT: the disc's radius */
} EzpzDrawItem;
typedef struct EzpzImageInfo { /* 32 bytes */
    uint64_t variants, masked, items_skipped, increments;
} EzpzImageInfo;
int ezpz_sketch_image_device(const double* x_dev, const uint8_t* ok_dev, size_t batch, size_t n_vars, const EzpzDrawItem* items,
                             size_t n_items, const EzpzImageView* view, uint32_t n_layers, int accumulate, uint32_t* counts_dev,
                             EzpzImageInfo* info_dev, void* stream);
int ezpz_sketch_image(const double* x, const uint8_t* ok, size_t batch, size_t n_vars, const EzpzDrawItem* items, size_t n_items,
                      const EzpzImageView* view, uint32_t n_layers, int accumulate, uint32_t* counts, EzpzImageInfo* info);
int ezpz_sketch_image_host(const double* x, const uint8_t* ok, size_t batch, size_t n_vars, const EzpzDrawItem* items, size_t n_items,
                           const EzpzImageView* view, uint32_t n_layers, int accumulate, uint32_t* counts, EzpzImageInfo* info);
/* ezpz_system_tolerance_mc_image[_device]: ezpz_system_tolerance_mc[_device] -- the same arguments, the same run, stats, totals,
 * hist and keep_* byte for byte -- and behind every round's reduction the round's solved variants drawn into counts
 * [n_layers][height][width] with the round's ok bytes: a variant that did not solve draws nothing.  The run zeroes counts and info
 * once; items and view are host memory, counts and info device memory in the _device form.  Not combined with the other kinds in
 * one call.  The argument errors of both entries; with samples == 0: EZPZ_OK after those checks, nothing written. */
int ezpz_system_tolerance_mc_image(EzpzSystem* sys, const double* x0, const uint32_t* positions, size_t n_param, const EzpzMcDist* dist,
                                   const double* nominal, const EzpzConstraint* records, size_t n_meas, const double* lim_lo,
                                   const double* lim_hi, const double* hist_lo, const double* hist_hi, uint64_t samples,
                                   const EzpzMcConfig* mc, const EzpzConfig* cfg, EzpzMcStats* stats, EzpzMcTotals* totals,
                                   uint64_t* hist, double* keep_params, double* keep_m, uint8_t* keep_flags, uint8_t* keep_ok,
                                   const EzpzDrawItem* items, size_t n_items, const EzpzImageView* view, uint32_t n_layers,
                                   uint32_t* counts, EzpzImageInfo* info);
int ezpz_system_tolerance_mc_image_device(EzpzSystem* sys, const double* x0_dev, const uint32_t* positions, size_t n_param,
                                          const EzpzMcDist* dist, const double* nominal, const EzpzConstraint* records, size_t n_meas,
                                          const double* lim_lo, const double* lim_hi, const double* hist_lo, const double* hist_hi,
                                          uint64_t samples, const EzpzMcConfig* mc, const EzpzConfig* cfg, EzpzMcStats* stats_dev,
                                          EzpzMcTotals* totals_dev, uint64_t* hist_dev, double* keep_params_dev, double* keep_m_dev,
                                          uint8_t* keep_flags_dev, uint8_t* keep_ok_dev, const EzpzDrawItem* items, size_t n_items,
                                          const EzpzImageView* view, uint32_t n_layers, uint32_t* counts_dev, EzpzImageInfo* info_dev,
                                          void* stream);
/* ezpz_sketch_compose: counts to colours on the host, integer arithmetic only.  rgb_out [height][width][3] starts as
 * background; per pixel the layers in order: F = full_at, or the layer's largest count where full_at is 0 (1 where that is 0 too);
 * a = count == 0 ? 0 : max(a_min, min(count, F) * 255 / F); a = a * opacity / 255; out_c = (out_c * (255 - a) + rgb_c * a +
 * 127) / 255.  EZPZ_ERR_INVALID_ARGUMENT: a NULL argument, a view or n_layers as above. */
typedef struct EzpzComposeLayer { /* 12 bytes */
    uint8_t rgb[3], opacity, a_min;
    uint32_t full_at;
} EzpzComposeLayer;
int ezpz_sketch_compose(const uint32_t* counts, const EzpzImageView* view, uint32_t n_layers, const EzpzComposeLayer* layers,
                        const uint8_t background[3], uint8_t* rgb_out);

#ifdef __cplusplus
}
#endif
#endif /* EZPZ_AMD_H */
