/* minilp_hip.h — C ABI of the MI355X-native simplex pivot engine (libminilp_hip.so).
 *
 * This is the drop-in boundary for ztlpn/minilp's Problem / Solution API.  The reference has
 * no FFI seam (pure Rust); these are the entry points a `minilp-sys` Rust shim
 * binds.  Each function cites the reference interface it replaces.
 *
 * Conventions
 *   - opaque handles, plain pointers and sizes, no C++/torch types;
 *   - status codes: 0 OK, 1 Infeasible, 2 Unbounded (lib.rs:172-178 `Error`), <0 internal
 *     (-1 invalid argument / reference panic condition, -2 singular basis, -3 HIP error,
 *      -4 no GPU / extension unavailable, -5 the dense nucleus inverse (8 k^2 bytes) does not fit in HBM).
 *     mlp_last_error() returns the message;
 *   - not thread-safe per handle; distinct handles are independent;
 *   - Solution mutators follow the reference's consume-on-error rule (lib.rs:359, 385): on a
 *     non-zero status the solution is freed and *s is set to NULL;
 *   - all solver state (x_B, d, gamma, beta, the basis inverse, A in CSR+CSC) lives in HBM;
 *     only scalars cross the boundary per pivot.
 */
#ifndef MINILP_HIP_H
#define MINILP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mlp_problem mlp_problem;   /* lib.rs:193-200 `Problem`  */
typedef struct mlp_solution mlp_solution; /* lib.rs:313-318 `Solution` (owns the device-resident Solver) */

enum { MLP_MINIMIZE = 0, MLP_MAXIMIZE = 1 };      /* lib.rs:61-68  OptimizationDirection */
enum { MLP_EQ = 0, MLP_LE = 1, MLP_GE = 2 };      /* lib.rs:160-169 ComparisonOp */
enum { MLP_OK = 0, MLP_INFEASIBLE = 1, MLP_UNBOUNDED = 2,
       MLP_EINVAL = -1, MLP_ESINGULAR = -2, MLP_EHIP = -3, MLP_ENOGPU = -4, MLP_ENOMEM = -5 };

/* ABI version of this header: bumped whenever a struct below changes.  From version 4 on mlp_stats only GROWS AT ITS END
 * (fields are appended, never inserted or removed), so a host built against an older version-4+ header reads a valid
 * prefix; mlp_stats_size() is sizeof(mlp_stats) as the LIBRARY was built — a host checks it (and mlp_abi_version())
 * against its own header before trusting the layout. */
/* Version 5: the struct mlp_certificate was added, with the dual-value / reduced-cost entry points below; mlp_stats is unchanged. */
/* Still version 5: the basis-status / ranging entry points further down are purely additive — new functions and one new struct
 * (mlp_ranging_info, with its own mlp_ranging_info_size()); mlp_stats and mlp_certificate are untouched, no existing layout moved. */
/* Still version 5: the cut-round entry points (mlp_solution_add_constraints_csr, mlp_solution_add_gomory_cuts, mlp_cut_info) are
 * additive in the same way. */
/* Still version 5: the tableau entry points (mlp_solution_num_rows, mlp_solution_basis_head, mlp_solution_binv_rows / _binv_cols,
 * mlp_solution_tableau_rows / _tableau_cols, mlp_solution_basis_solve, mlp_tableau_info with its own mlp_tableau_info_size()) are
 * additive in the same way. */
/* Still version 5: the Gomory mixed-integer round (mlp_solution_add_gmi_cuts, mlp_gmi_info with its own mlp_gmi_info_size()) is
 * additive in the same way; mlp_cut_info keeps its 80 bytes. */
/* Still version 5: the branching penalties (mlp_solution_branch_penalties, mlp_branch_info with its own mlp_branch_info_size()) are
 * additive in the same way. */
/* Still version 5: the reduced-cost bounds and the batched fixing (mlp_solution_cutoff_bounds, mlp_solution_fix_vars,
 * mlp_solution_unfix_vars, mlp_fix_info with its own mlp_fix_info_size()) are additive in the same way. */
/* Still version 5: the bound changes (mlp_solution_set_var_bounds, mlp_solution_tighten_by_reduced_cost, mlp_solution_var_bounds,
 * mlp_bounds_info with its own mlp_bounds_info_size()) are additive in the same way. */
/* Still version 5: the bound propagation (mlp_solution_propagate_bounds, mlp_solution_tighten_by_propagation, mlp_propagate_info with
 * its own mlp_propagate_info_size()) is additive in the same way. */
/* Still version 5: the right-hand-side changes (mlp_solution_set_rhs, mlp_solution_constraint_rhs, mlp_solution_rhs_scenarios,
 * mlp_rhs_info with its own mlp_rhs_info_size()) are additive in the same way. */
#define MLP_ABI_VERSION 5u
uint32_t mlp_abi_version(void);
uint64_t mlp_stats_size(void);

const char* mlp_last_error(void);
/* Number of visible HIP devices (0 => every solve returns MLP_ENOGPU; there is no CPU fallback). */
int mlp_device_count(void);
/* Select the HIP device used by solutions created afterwards on this thread (one process per GPU). */
int mlp_set_device(int device);

/* ---- Problem (lib.rs:215-305) ------------------------------------------------------------ */
mlp_problem* mlp_problem_new(int direction);                                   /* Problem::new      lib.rs:217 */
mlp_problem* mlp_problem_clone(const mlp_problem* p);                          /* #[derive(Clone)]  lib.rs:193 */
void mlp_problem_free(mlp_problem* p);
/* returns the Variable index (lib.rs:72, 79) */
uint32_t mlp_problem_add_var(mlp_problem* p, double obj_coeff, double min, double max); /* add_var lib.rs:233 */
uint32_t mlp_problem_num_vars(const mlp_problem* p);
/* duplicate or out-of-range variable => MLP_EINVAL (the reference panics, lib.rs:247-249) */
int mlp_problem_add_constraint(mlp_problem* p, const uint32_t* vars, const double* coeffs, uint64_t k,
                               int cmp_op, double rhs);                        /* add_constraint lib.rs:276 */
/* bulk forms of add_var / add_constraint (same semantics, one call): n variables; m rows in CSR */
int mlp_problem_add_vars(mlp_problem* p, uint64_t n, const double* obj_coeffs, const double* mins, const double* maxs);
int mlp_problem_add_constraints_csr(mlp_problem* p, uint64_t m, const uint64_t* indptr, const uint32_t* vars,
                                    const double* coeffs, const int32_t* cmp_ops, const double* rhs);
int mlp_problem_solve(const mlp_problem* p, mlp_solution** out);               /* solve lib.rs:291 */
/* read-back of the model data (Problem is plain data in the reference too, lib.rs:194-200) */
uint64_t mlp_problem_num_constraints(const mlp_problem* p);
int mlp_problem_var(const mlp_problem* p, uint32_t var, double* obj_coeff, double* min, double* max);
/* returns the number of terms; copies min(terms, cap) of them (sorted by variable) */
uint64_t mlp_problem_constraint(const mlp_problem* p, uint64_t c, uint32_t* vars, double* coeffs, uint64_t cap,
                                int* cmp_op, double* rhs);

/* ---- Solution (lib.rs:332-424) ----------------------------------------------------------- */
mlp_solution* mlp_solution_clone(const mlp_solution* s);  /* #[derive(Clone)] lib.rs:313: deep copy of device state */
void mlp_solution_free(mlp_solution* s);
double mlp_solution_objective(const mlp_solution* s);                          /* objective lib.rs:334 */
uint32_t mlp_solution_num_vars(const mlp_solution* s);
int mlp_solution_var_value(const mlp_solution* s, uint32_t var, double* out);  /* var_value lib.rs:344 / Index lib.rs:426 */
int mlp_solution_values(const mlp_solution* s, double* out, uint32_t n);       /* iter lib.rs:350 (bulk form) */
int mlp_solution_add_constraint(mlp_solution** s, const uint32_t* vars, const double* coeffs, uint64_t k,
                                int cmp_op, double rhs);                       /* add_constraint lib.rs:368 */
int mlp_solution_fix_var(mlp_solution** s, uint32_t var, double val);          /* fix_var lib.rs:390 */
int mlp_solution_unfix_var(mlp_solution** s, uint32_t var, int* was_fixed);    /* unfix_var lib.rs:399 */
int mlp_solution_add_gomory_cut(mlp_solution** s, uint32_t var);               /* add_gomory_cut lib.rs:419 */

/* ---- Engine-level controls (no counterpart in the reference: its pivot loop exposes no
 *      counter; these implement the fixed-pivot-budget measurement of §8d) ---- */
/* Like mlp_problem_solve but stops after `budget` simplex iterations (budget < 0: run to optimality).
 * flags: bit0 = record a pivot trace, bit1 = time the dominant kernels with HIP events (sampled iterations),
 * bit2 = with bit1: every iteration is a sampled one. */
int mlp_problem_solve_ex(const mlp_problem* p, mlp_solution** out, int64_t budget, uint32_t flags);
int mlp_solution_continue(mlp_solution* s, int64_t budget);
/* Basis checkpoint ("pivots from a saved mid-solve basis"; the reference has no basis I/O — its
 * Solver state is solver.rs:14-58).  mlp_solution_save_basis returns the size of the blob and copies it when
 * buf != NULL and cap is large enough (0 on error).  mode 0: basic / non-basic sets (solver.rs:37, 44), non-basic
 * flags and values (solver.rs:45-49); mode 1: + the steepest-edge weights as f32 (they only steer pricing);
 * mode 2: + x_B, d, gamma, beta and the objective as f64 — a solve loaded from a mode-2 blob continues pivot for
 * pivot like the uninterrupted one.  mlp_problem_solve_from_basis builds the same problem (Solver::try_new),
 * installs the basis, re-inverts the nucleus on the device (BasisSolver::reset, solver.rs:1286-1303), recomputes
 * x_B and the reduced costs from the basis (modes 0/1; solver.rs:1177-1231) and continues like mlp_problem_solve_ex.
 * A blob of another model (row / variable counts differ, sets do not partition the variables) => MLP_EINVAL.
 * A sharded solution (mlp_solution_enable_sharding) saves mode 0 only: the partition is what every rank holds in full. */
uint64_t mlp_solution_save_basis(const mlp_solution* s, int mode, void* buf, uint64_t cap);
int mlp_problem_solve_from_basis(const mlp_problem* p, const void* blob, uint64_t len, mlp_solution** out, int64_t budget,
                                 uint32_t flags);
/* flags bit1 (HIP-event timing): 1 = sample EVERY iteration as an eager, event-bracketed one (measurement passes),
 * 0 = the default cadence (every 8th / 4th batch), < 0 = switch the sampling off (until the next call with a value >= 0, which
 * also switches HIP-event timing on for a solution created without flag bit1) */
int mlp_solution_set_sampling(mlp_solution* s, int every_iteration);
int mlp_solution_budget_exhausted(const mlp_solution* s);
/* Recompute the dense nucleus inverse from A (the counterpart of BasisSolver::reset,
 * solver.rs:1286-1303); returns max |W_incremental - W_fresh| through *max_diff when non-NULL.  While the basis is held as the
 * compact factor (mlp_stats.factor_active) there is no incremental inverse to compare with: the factor is rebuilt from the basis
 * and *max_diff is NaN ("nothing compared"), never a false 0. */
int mlp_solution_reinvert(mlp_solution* s, double* max_diff);

/* The objective value and the reduced costs are recomputed for the new point as well (solver.rs:1199-1231).
 * x_B = B^-1 (b - N x_N) recomputed from the basis, with two steps of iterative refinement (the reference's
 * recalc_basic_var_vals, solver.rs:1177-1197, which it leaves unused; here it is the polish step of long runs and is
 * exported for hosts that want it after many warm-start pivots).  A dense-rhs FTRAN: with a large nucleus it is one
 * streaming read of the nucleus inverse (8 k^2 bytes) per step; in profile mode mlp_stats.dense_ftran_* time it. */
int mlp_solution_recompute_basic_values(mlp_solution* s);

/* Column-block sharding of the pricing path across the GPUs of one node (one process per GPU,
 * DESIGN.md §6).  Every rank builds the SAME problem, calls mlp_problem_solve_ex(budget = 0), then
 * this function with its rank, the world size (<= 16) and the name of a POSIX shared-memory object of
 * 896 * world zeroed bytes created by the launcher (the rendezvous), and then the same sequence of
 * mlp_solution_continue calls.  Rank r owns non-basic positions [n*r/world, n*(r+1)/world): its
 * tableau-row sweep, d/gamma update and pricing scan cover only that block; candidates are exchanged once or
 * twice per pivot (primal: pricing all-gather + ratio decision; dual: leaving row, pass-1 minimum, pass-2
 * candidate) from inside the pivot kernels.  Transport: every rank keeps a mailbox in its own HBM, the peers map
 * it through HIP IPC (the handles travel through the rendezvous object) and write their 64-byte records into it
 * over xGMI; polling is local.  MLP_MAILBOX=host selects the older host-memory mailbox (PCIe) instead.  The call
 * returns when every rank has mapped every mailbox (bounded waits: a missing rank is an error, MLP_EHIP).
 * Primal and dual loops; the Solution mutators are refused.  mlp_solution_transport names the transport in use.
 * Deferred sharding (default; MLP_SHARD_DEFER=0 turns it off): while the nucleus is small — the sparse-tableau-row regime, a few
 * hundred pivots from the slack basis, where a pivot is tens of microseconds of latency-bound launches and per-pivot exchanges can
 * only slow it down — the ranks run as bit-identical REPLICAS (the deterministic unsharded iteration on every rank, no exchange);
 * the column blocks and the exchanges go live at the first batch that leaves that regime, at the same pivot on every rank, and
 * stay live.  Nothing changes for the caller: the same calls, the same pivots. */
int mlp_solution_enable_sharding(mlp_solution* s, int rank, int world, const char* shm_name);
/* The same with the transport named by the caller: NULL / "" = the default above (or MLP_TRANSPORT), "peer", "host",
 * "rccl" — north_star's literal transport: the mailbox records of every exchange (16-byte pricing candidates, the ratio decision,
 *          the dual loop's minimum / candidate) are delivered by ncclAllGather over xGMI: the pivot kernels post into and poll their
 *          own device box, and while a batch of pivots is in flight the host pumps stage -> ncclAllGather -> deliver rounds on a
 *          second stream until every rank's batch has drained.  rccl_id = the 128-byte ncclUniqueId made by rank 0
 *          (mlp_rccl_unique_id) and distributed by the launcher; librccl.so is loaded at run time.  Slower per exchange than
 *          the peer stores (a collective per round), so it is the fallback for nodes where the peer mappings do not deliver;
 * "pump" — the rccl transport's protocol with peer copies between IPC-mapped staging buffers in place of the collective (RCCL
 *          refuses two ranks on one device; this is how the protocol is tested on a one-GPU box).
 * The pump transports accept world = 1. */
int mlp_solution_enable_sharding_ex(mlp_solution* s, int rank, int world, const char* shm_name, const char* transport,
                                    const void* rccl_id);
int mlp_rccl_unique_id(void* out128);
const char* mlp_solution_transport(const mlp_solution* s);

typedef struct mlp_stats {
    uint64_t iterations, basis_changes, bound_flips, primal_iters, dual_iters, reinversions;
    uint64_t num_constraints, num_total_vars, nucleus_size, nucleus_capacity, nnz;
    /* algorithmic bytes and HIP-event time of the two dominant kernels */
    double fused_bytes, fused_ms, sweep_bytes, sweep_ms;
    uint64_t fused_launches, sweep_launches;
    double solve_wall_s; /* host wall time spent inside the pivot loops */
    uint64_t kase[5]; /* basis changes by partition case: nucleus->nucleus, singleton->nucleus (grow), nucleus->singleton
                         (shrink), singleton->singleton (column swap), same-row singleton swap */
    double update_ms; uint64_t update_launches; /* K8 (x_B/d/gamma/beta update + next pricing scan), HIP-event time */
    uint64_t banded_sweep;    /* 1 when the tableau-row pass runs as the banded sweep (large m), 0 for the CSC pull */
    uint64_t final_refreshes; /* times optimality was re-examined on recomputed reduced costs (long runs only) */
    double max_pivot_err; /* drift monitor: max |alpha_q[r] - alpha_r[q]| / max(1,|alpha_q[r]|) seen so far */
    /* FTRAN of the entering column (head + gather of the listed columns of the nucleus inverse + F push):
     * algorithmic bytes 8 k |list| + 12 nnz(nucleus columns) + 12 nnz(a_q), HIP-event time of sampled iterations */
    double ftran_bytes, ftran_ms; uint64_t ftran_launches;
    double iter_ms; uint64_t iter_samples; /* whole sampled iterations, first kernel to last (HIP events) */
    uint64_t beta_rebuilds; /* lazy dual steepest edge: exact rebuilds of the dual edge norms from the basis inverse (the primal
                               loop skips their per-pivot recurrence, solver.rs:1153-1174, because nothing reads them there) */
    double fold_bytes, fold_ms; uint64_t fold_launches; /* sampled folds of the pending rank-1 terms into the nucleus inverse (HIP events) */
    double dense_ftran_bytes, dense_ftran_ms; uint64_t dense_ftran_launches; /* dense-rhs FTRAN of mlp_solution_recompute_basic_values /
                              the polish step: algorithmic bytes (8 k^2 per solve) and kernel-exact time of the pass over the nucleus inverse */
    double str_ms; uint64_t str_launches; /* sampled sparse tableau rows (small nucleus: only the columns that meet supp(rho)): HIP-event time */
    uint64_t hyper_iters, hyper_bails; /* iterations run by the hypersparse single-workgroup kernel (support-restricted work, sparse models);
                                          iterations it declined (list overflow / too much work for one workgroup) and handed to the multi-kernel path */
    uint64_t ratio_stalls; /* in-kernel waits of the one-launch Harris tests that timed out (grid not co-resident); each one is
                              retried with the two-launch form, which then stays selected */
    /* ---- appended in ABI version 4 ---- */
    uint64_t reinversion_fallbacks; /* rounds 1-3: re-inversions a library call reported singular and the Gauss-Jordan kernels then
                                       re-examined; always 0 since the blocked inversion is hand-written (kept for the layout);
                                       ratio_stalls also counts a stalled wait of the one-launch small-nucleus form */
    /* compact factor of the basis (a peeled triangular factor + additive eta terms instead of the explicit
     * nucleus inverse; selected by the measured shape of the basis, MLP_FACTOR=1 / 0 forces it on / off) */
    uint64_t factor_active;     /* 1 while B^-1 is held as the compact factor */
    uint64_t factor_refactors;  /* refactorisations (peels of the current basis) so far */
    uint64_t factor_levels;     /* levels of the last peel = dependent steps of one triangular solve */
    uint64_t factor_switches;   /* switches between the two representations */
    uint64_t factor_bump;       /* columns the last peel left over (cycles of the basis graph; their inverse is kept explicitly) */
    uint64_t factor_bump_max;   /* largest bump of any refactorisation so far */
} mlp_stats;
void mlp_solution_stats(const mlp_solution* s, mlp_stats* out);
void mlp_solution_reset_stats(mlp_solution* s);

/* pivot trace (flags bit0): phase 0 primal / 1 dual; row = -1 for a bound flip */
uint64_t mlp_solution_trace_len(const mlp_solution* s);
void mlp_solution_trace_get(const mlp_solution* s, uint64_t i, int32_t* phase, int64_t* col, int64_t* row,
                            int64_t* entering_var, int64_t* leaving_var, double* pivot_coeff, double* obj_after);
/* white-box state for the differential tests (names follow solver.rs:14-58): returns the length,
 * copies min(len, cap) doubles into out when out != NULL; (uint64_t)-1 for an unknown name. */
uint64_t mlp_solution_state(const mlp_solution* s, const char* what, double* out, uint64_t cap);

/* ---- Dual values, reduced costs and a KKT certificate (no counterpart in the reference: minilp 0.2.2 returns the primal point
 *      only; these extend Solution::objective / var_value, lib.rs:334-348, to the other half of the solution) ----------------------
 * Constraint index: 0 .. mlp_solution_num_constraints(s)-1 in the order the constraints were added — mlp_problem_add_constraint
 * (MPS rows in file order), then the rows mlp_solution_add_constraint and mlp_solution_add_gomory_cut appended, in call order.
 * Dual value: pi = B^-T c_B of the current basis, from the user's own objective coefficients (not the negated ones of a Maximize
 * problem, not the artificial costs of the feasibility phase), so pi_c is d objective() / d rhs_c for the current basis, in the
 * user's direction.  At an optimum of a Minimize problem a <= row has pi <= 0 and a >= row pi >= 0; Maximize reverses both; = rows
 * take either sign.  A constraint whose slack is basic, or one without terms, returns exactly 0.0.
 * Reduced cost: r_j = c_j - a_j . pi for every variable, in the user's sense; a basic variable returns exactly 0.0.
 * Defined for any Solution the engine holds (optimum, budget-limited solve, solve_from_basis, after the mutators): at a basis that is
 * not optimal they are the multipliers of that basis and the certificate says how far it is from optimal.  Computed on the device
 * once per solution state and cached (the single-element getters are O(1) after that); every mutator, continue, engine stage and
 * re-inversion drops the cache.  Reading is side-effect free: the Solution continues pivot for pivot, bit for bit, and its mode-2
 * basis blob is unchanged.  Sharded solutions are refused with MLP_EINVAL (like the mutators); a wrong length => MLP_EINVAL. */
uint64_t mlp_solution_num_constraints(const mlp_solution* s);                       /* extends Problem::add_constraint, lib.rs:276 */
int mlp_solution_dual_values(mlp_solution* s, double* out, uint64_t m);   /* m = mlp_solution_num_constraints; bulk form like iter lib.rs:350 */
int mlp_solution_dual_value(mlp_solution* s, uint64_t c, double* out);     /* like var_value lib.rs:344, by constraint */
int mlp_solution_reduced_costs(mlp_solution* s, double* out, uint32_t n);  /* n = mlp_solution_num_vars; bulk form like iter lib.rs:350 */
int mlp_solution_reduced_cost(mlp_solution* s, uint32_t var, double* out); /* like var_value lib.rs:344 */

/* KKT certificate of the current point against the model as the user stated it (with fix_var's fixings), computed on the device from
 * x, pi and r.  dual_objective is the Lagrangian bound b . pi + sum_j r_j l_j over every variable (the slacks included), where l_j
 * is the bound of variable j that minimises r_j x_j in the minimisation sense (the fixed value for a fixed variable); where that
 * bound is infinite the term takes the current x_j and |r_j| counts toward max_dual_infeasibility.  So when max_dual_infeasibility
 * is 0, dual_objective is a valid weak-duality bound for any bounds.  Only grows at its end; mlp_certificate_size() is its size as
 * the library was built. */
typedef struct mlp_certificate {
    double primal_objective;       /* c . x recomputed from x */
    double dual_objective;         /* the Lagrangian bound above */
    double relative_gap;           /* |primal - dual| / max(1, |primal|) */
    double max_row_violation;      /* over the constraints: distance of a . x from its allowed side of rhs */
    int64_t max_row_violation_at;  /* constraint index, -1 when none is violated */
    double max_bound_violation;    /* over the variables */
    int64_t max_bound_violation_at;
    double max_dual_infeasibility; /* max |r_j| where the bound l_j is infinite */
    int64_t max_dual_infeasibility_at; /* < num_vars: a variable; num_vars + i: the slack of row i; -1 when none */
    double btran_residual;         /* max over basic columns of |c_j - a_j . pi| before it is zeroed: the accuracy of pi */
    int64_t btran_residual_at;     /* same numbering as max_dual_infeasibility_at */
    double bytes;                  /* algorithmic bytes of the certificate's own passes (transposed solve + reduced costs + rows) */
    double device_ms;              /* their time on the device (HIP events around the launches) */
} mlp_certificate;
uint64_t mlp_certificate_size(void);
int mlp_solution_certificate(mlp_solution* s, mlp_certificate* out);

/* ---- Basis status, cost ranging and rhs ranging (the other half of a sensitivity report: how far may a cost coefficient or a
 *      right-hand side move before the basis changes and the dual values / reduced costs above stop being valid?) -------------------
 * All of it is stated in the engine's internal minimisation form  min c.x, A x + s = b  (slack s = rhs - activity, bounds by operator:
 * <= [0, inf), >= (-inf, 0], = [0, 0]) at the CURRENT basis, whatever it is; the ranges are meaningful at an optimum and are the same
 * formulas, never an error, on a budget-limited solve.
 * Basis status, per structural variable and per constraint (= its slack): MLP_BASIC, MLP_AT_LOWER, MLP_AT_UPPER, MLP_NB_FREE
 * (non-basic at neither bound), MLP_NB_FIXED (mlp_solution_fix_var, or lo == hi).  A constraint without terms has no row: MLP_BASIC.
 * Cost range [lo_j, hi_j] of variable j, containing c_j: the values of c_j for which every reduced-cost sign condition the basis needs
 * keeps holding.  With r the (internal) reduced costs:
 *   non-basic j: at lower [c_j - r_j, +inf); at upper (-inf, c_j - r_j]; MLP_NB_FREE [c_j, c_j]; MLP_NB_FIXED (-inf, +inf);
 *   basic j at position p: alpha_i = (e_p^T B^-1) a_i over ALL non-basic columns i (slack columns included),
 *     delta+ = min r_i / alpha_i over {i at lower, alpha_i > 0} u {i at upper, alpha_i < 0} u {i MLP_NB_FREE, alpha_i != 0: 0},
 *     delta- = max r_i / alpha_i over the mirrored sets; MLP_NB_FIXED columns impose nothing; an empty set gives -+inf;
 *     the range is [c_j + delta-, c_j + delta+].
 * Rhs range [lo_c, hi_c] of constraint c, containing rhs_c: the values for which x_B stays within [loB, hiB] with the non-basic
 * variables where they are.
 *   slack of the row basic at p: [rhs + (loB_p - xB_p), rhs + (hiB_p - xB_p)];
 *   otherwise h = B^-1 e_row: delta+ = min of (hiB_p - xB_p) / h_p over h_p > 0 and (loB_p - xB_p) / h_p over h_p < 0, delta- mirrored;
 *   a constraint without a row: (-inf, +inf).
 * Tolerances: |alpha_i| <= 1e-8 and |h_p| <= 1e-8 count as zero; a numerator of the wrong sign (r_i = -1e-13 at a lower bound, xB a
 * hair outside its bound) is clamped to 0, hence always lo <= current <= hi.
 * User's sense: for a Maximize problem the internal cost is -c, so the cost range returned is [-hi, -lo]; rhs ranges have no sign turn.
 * Within a rhs range the objective moves by dual_value(c) * delta, within a cost range by var_value(j) * delta.
 * vars / cons == NULL asks for all of them (n must then be mlp_solution_num_vars / mlp_solution_num_constraints); otherwise n indices,
 * duplicates allowed.  The two numbers of a request do not depend on what else is in the call (bit for bit).  Reading is side-effect
 * free like the dual values; sharded solutions, a NULL handle, a wrong length or an index out of range => MLP_EINVAL. */
enum { MLP_BASIC = 0, MLP_AT_LOWER = 1, MLP_AT_UPPER = 2, MLP_NB_FREE = 3, MLP_NB_FIXED = 4 };
int mlp_solution_basis_status(const mlp_solution* s, int32_t* var_status, uint32_t n_vars, int32_t* cons_status, uint64_t n_cons);
int mlp_solution_cost_ranging(const mlp_solution* s, const uint32_t* vars, uint64_t n, double* lo, double* hi);
int mlp_solution_rhs_ranging(const mlp_solution* s, const uint64_t* cons, uint64_t n, double* lo, double* hi);
/* of the last ranging call on this solution (zeros before the first).  Only grows at its end; mlp_ranging_info_size() is its size as
 * the library was built. */
typedef struct mlp_ranging_info {
    uint64_t requests;   /* variables / constraints asked for */
    uint64_t solves;     /* of them: requests that needed a row / a column of B^-1 (basic variables, rows whose slack is non-basic) */
    uint64_t batches;    /* batches of 16 such requests: one pass over A (cost) / over the basic positions (rhs) each */
    double bytes;        /* algorithmic bytes of the batches */
    double device_ms;    /* their time on the device (HIP events around the launches) */
} mlp_ranging_info;
int mlp_solution_ranging_info(const mlp_solution* s, mlp_ranging_info* out);
uint64_t mlp_ranging_info_size(void);

/* ---- A round of cuts in one call (no counterpart in the reference: solver.rs:440-460 and 549-634 take one row at a time) ------------
 * mlp_solution_add_constraints_csr: m x mlp_solution_add_constraint in one call (rows in CSR, same argument meaning as
 *   mlp_problem_add_constraints_csr): all rows are appended to the model, then feasibility is restored ONCE.  The model left behind is
 *   what m calls of mlp_solution_add_constraint in the same order would have left: constraint numbering (dual values, rhs ranging,
 *   mlp_solution_num_constraints), the rows the engine holds, slack bounds by operator; a row without terms gets no row and must be a
 *   tautology (otherwise MLP_INFEASIBLE).  The slack of every new row starts at rhs - a.x at the point the call finds; only the pivot
 *   path of the re-solve differs from the sequential form, so the optimum value is the same.
 * mlp_solution_add_gomory_cuts: one round of Gomory cuts.  For every listed variable (each must be basic; a duplicate, a non-basic or
 *   an out-of-range variable is MLP_EINVAL) the cut of solver.rs:440-460,
 *       sum_j (floor(alpha_pj) - alpha_pj) x_nb(j) <= floor(xB_p) - xB_p,
 *   ALL taken from the basis the call finds, built on the device, appended together, feasibility restored once.  Stored as
 *   mlp_solution_add_gomory_cut stores it: terms on all non-basic columns (slacks included) in variable order, coefficients that are
 *   exactly 0.0 dropped, operator <=.  The row of a variable does not depend on what else is in the round (bit for bit).
 * Both: the solution must be solved (MLP_EINVAL otherwise); MLP_INFEASIBLE => status 1; on every non-zero status the solution is
 *   freed and *s = NULL, as the single forms do.  m == 0 / n == 0 is a successful no-op that leaves the solution untouched.  Sharded
 *   solutions and NULL handles => MLP_EINVAL.  The dual-value / ranging cache is dropped.
 * mlp_cut_info: what the last of these two calls on this solution did (zeros before the first).  Only grows at its end;
 *   mlp_cut_info_size() is its size as the library was built. */
int mlp_solution_add_constraints_csr(mlp_solution** s, uint64_t m, const uint64_t* indptr, const uint32_t* vars,
                                     const double* coeffs, const int32_t* cmp_ops, const double* rhs);
int mlp_solution_add_gomory_cuts(mlp_solution** s, const uint32_t* vars, uint64_t n);
typedef struct mlp_cut_info {
    uint64_t rows;                /* rows appended to the matrix */
    uint64_t rows_without_terms;  /* constraints of the call that have no terms (tautologies): numbered, but no row */
    uint64_t nnz;                 /* terms of the appended rows (slack entries not counted) */
    uint64_t batches;             /* Gomory rounds: batches of 16 cuts, one pass over A each; 0 for add_constraints_csr */
    uint64_t relayouts;           /* re-layouts of the column-major copy of A: 1 for any call that appends a row */
    uint64_t reinversions;        /* from-scratch inversions / refactorisations the call needed: 0 or 1 */
    uint64_t pivots;              /* iterations of the one re-solve */
    double bytes;                 /* algorithmic bytes of the cut generation (0 for add_constraints_csr) */
    double device_ms;             /* its time on the device (HIP events around the generation launches) */
    double wall_ms;               /* the whole call */
} mlp_cut_info;
int mlp_solution_cut_info(const mlp_solution* s, mlp_cut_info* out);
uint64_t mlp_cut_info_size(void);

/* ---- Reading the simplex tableau: rows and columns of B^-1 A, of B^-1, solves with the basis (what GLPK calls glp_eval_tab_row / _col
 *      and glp_ftran / glp_btran; the raw material of mixed-integer cuts, custom ranging and post-optimal analysis) ------------------------
 * Internal form, as for the ranging above: A x + s = b, Abar = [A | I], B = the basic columns of Abar at the CURRENT basis, whatever it is
 * (optimum, budget-limited solve, solve_from_basis, after any mutator).  Nothing here depends on the optimisation direction: there is no
 * sign turn for Maximize.
 * Columns: j < num_vars is structural variable j; num_vars + c is the slack of constraint c, in the constraint numbering of
 *   mlp_solution_dual_values.  A constraint without terms has no row and no slack column: asking for it is MLP_EINVAL, and it never
 *   appears in an output.
 * Vectors "by row" are exchanged BY CONSTRAINT and have length mlp_solution_num_constraints: a constraint without a row reads 0.0 on
 *   output and is ignored on input.
 * Basis positions run 0 .. num_rows - 1, num_rows = mlp_solution_num_rows = the constraints that have a row; basis_head[p] is the column
 *   (numbering above) basic at position p, in the engine's own position order (mlp_solution_state "host_basic_vars").  Vectors "by
 *   position" have length num_rows.
 * mlp_solution_binv_rows:    for each listed BASIC column, rho_p = e_p^T B^-1 of its position p, by constraint: out[n][num_constraints].
 * mlp_solution_binv_cols:    for each listed constraint (it must have a row), h = B^-1 e_row by position: out[n][num_rows].
 * mlp_solution_tableau_rows: for each listed BASIC column, alpha_p = rho_p^T Abar as a sparse row in CSR (indptr[n + 1], indices, values)
 *   over the column numbering: sorted by column, exact zeros dropped (as the Gomory generation drops them), the entry of the requested
 *   column itself exactly 1.0, the other basic columns omitted (they are 0 by definition and are not computed).  The three arrays are
 *   owned by the library and stay valid until the next tableau call, mutator, continue, engine stage, re-inversion or free of that
 *   solution.
 * mlp_solution_tableau_cols: for each listed column j (basic or not), B^-1 abar_j by position: out[n][num_rows]; a basic column gives the
 *   exact unit vector of its position.
 * mlp_solution_basis_solve:  transpose == 0: rhs[n][num_constraints] by constraint -> out[n][num_rows] = B^-1 rhs by position (FTRAN);
 *   transpose != 0: rhs[n][num_rows] by position -> out[n][num_constraints] = B^-T rhs by constraint (BTRAN).
 * The dense forms write into caller buffers; rhs_len / out_len are their lengths in doubles and must be exactly n times the row length
 * stated above.  Lists may hold duplicates, in any order.
 * Guarantees: (1) reading is side-effect free like the dual values — the solution continues pivot for pivot and bit for bit as if nothing
 * had been read, and its mode-2 basis blob is unchanged; (2) the numbers of one request are bit-identical whatever else is in the call, in
 * whatever order, and from run to run (requests are served in batches of 16 that share one pass over the inverse / over A; no sum
 * depends on its place in a batch, no float atomics).
 * Errors, all MLP_EINVAL with the solution still usable: a NULL handle, a sharded solution, a wrong length, an index out of range, the
 * slack of a constraint without terms, a non-basic column given to binv_rows / tableau_rows.  n == 0 is a successful no-op.
 * mlp_tableau_info: counters of the last of these calls on this solution (zeros before the first).  Only grows at its end;
 *   mlp_tableau_info_size() is its size as the library was built. */
uint64_t mlp_solution_num_rows(const mlp_solution* s);
int mlp_solution_basis_head(const mlp_solution* s, uint64_t* head, uint64_t num_rows);
int mlp_solution_binv_rows(const mlp_solution* s, const uint64_t* cols, uint64_t n, double* out, uint64_t out_len);
int mlp_solution_binv_cols(const mlp_solution* s, const uint64_t* constraints, uint64_t n, double* out, uint64_t out_len);
int mlp_solution_tableau_rows(const mlp_solution* s, const uint64_t* cols, uint64_t n, const uint64_t** indptr, const uint32_t** indices,
                              const double** values);
int mlp_solution_tableau_cols(const mlp_solution* s, const uint64_t* cols, uint64_t n, double* out, uint64_t out_len);
int mlp_solution_basis_solve(const mlp_solution* s, int transpose, const double* rhs, uint64_t rhs_len, uint64_t n, double* out,
                             uint64_t out_len);
typedef struct mlp_tableau_info {
    uint64_t requests;   /* rows / columns / right-hand sides asked for */
    uint64_t solves;     /* of them: right-hand sides that needed the device (all but basic columns given to tableau_cols) */
    uint64_t batches;    /* batches of 16 of them: one pass over the inverse (solves) / the rows' block and one pass over A (tableau rows) each */
    uint64_t nnz;        /* terms emitted by tableau_rows (0 for the dense forms) */
    double bytes;        /* algorithmic bytes of the batches */
    double device_ms;    /* their time on the device (HIP events around the launches) */
} mlp_tableau_info;
int mlp_solution_tableau_info(const mlp_solution* s, mlp_tableau_info* out);
uint64_t mlp_tableau_info_size(void);

/* ---- A round of Gomory mixed-integer (GMI) cuts from the tableau, in one call ------------------------------------------------------------
 * The cut of mlp_solution_add_gomory_cuts is valid only when every non-basic column is an integer variable at a zero lower bound and the
 * slacks are integer.  The GMI cut handles bounds, columns non-basic at their upper bound, continuous variables and slacks.
 * Internal form, as for the tableau reads above: A x + s = b.  A request is a BASIC structural variable marked integer, at basis position
 * p; f0 = xB_p - floor(xB_p).  Every non-basic column j (structural or slack) has a status (the codes of mlp_solution_basis_status), a
 * value xN_j and a coefficient alpha_j = (e_p^T B^-1) abar_j.  Per column:
 *   fixed (mlp_solution_fix_var, or lo == hi, which includes the slack of an = row): no term;
 *   at lower: abar = alpha;   at upper: abar = -alpha;
 *   free (non-basic at neither bound): |alpha| <= 1e-8 gives no term; otherwise the request has no valid cut and is skipped;
 *   integer treatment, for a column that is marked integer AND has xN_j == floor(xN_j) exactly (structural columns are marked by
 *     var_is_int, slacks by con_is_int):  f = abar - floor(abar);  g = f / f0 if f <= f0, else (1 - f) / (1 - f0);
 *   continuous treatment, for everything else (a marked column whose value is not integral included, which is always valid):
 *     g = abar / f0 if abar >= 0, else -abar / (1 - f0).
 * The cut is  sum_j g_j y_j >= 1  with y_j = x_j - xN_j at lower and y_j = xN_j - x_j at upper.  It is stored as
 * mlp_solution_add_gomory_cut stores its row: operator <=, terms on the non-basic columns (slacks included) in variable order, exact
 * zeros dropped; stored coefficients c_j = -g_j at lower, +g_j at upper; stored right-hand side rhs = -1 + sum_j c_j xN_j.
 * The cut is valid for the bounds the call finds: a bound tightened by mlp_solution_fix_var makes it LOCAL to that fixing (it need not
 * hold once the variable is unfixed).
 * A request with min(f0, 1 - f0) < away is skipped.  A skipped request appends nothing and takes no constraint number (it is not a
 * "row without terms").  All cuts of a round come from the basis the call finds, are built on the device (16 per pass over A) and
 * appended together: one re-layout, at most one re-inversion, feasibility restored once.  A request's row, rhs and status are bit for
 * bit the same from run to run and whatever else is in the call.
 * Arguments: vars[n] the requests; var_is_int[num_vars] (num_vars must be mlp_solution_num_vars); con_is_int[num_constraints]
 *   (num_constraints must be mlp_solution_num_constraints) or NULL with any num_constraints: all slacks continuous; away in (0, 0.5];
 *   status_out[n] or NULL: 0 emitted, 1 skipped for a fraction within away, 2 skipped for a free non-basic column in the row.
 * MLP_EINVAL: a variable out of range, non-basic, unmarked or listed twice; a mask length that does not fit; away outside (0, 0.5]; an
 *   unsolved model; a sharded solution; NULL handles.  MLP_INFEASIBLE => status 1 (a cut whose terms all vanish reads 0 <= -1: the
 *   marks and the point admit no integer solution).  On every non-zero status the solution is freed and
 *   *s = NULL, as the other mutators do.  n == 0, or a call in which every request is skipped, leaves the solution untouched.  The
 *   dual-value / ranging / tableau caches are dropped.
 * mlp_gmi_info: what the last mlp_solution_add_gmi_cuts call on this solution did (zeros before the first); the call also fills
 *   mlp_cut_info as mlp_solution_add_gomory_cuts does.  Only grows at its end; mlp_gmi_info_size() is its size as the library was built. */
int mlp_solution_add_gmi_cuts(mlp_solution** s, const uint32_t* vars, uint64_t n, const uint8_t* var_is_int, uint32_t num_vars,
                              const uint8_t* con_is_int, uint64_t num_constraints, double away, int32_t* status_out);
typedef struct mlp_gmi_info {
    uint64_t requests;          /* variables asked for */
    uint64_t rows;              /* cuts appended */
    uint64_t skipped_fraction;  /* requests skipped: fraction within away */
    uint64_t skipped_free;      /* requests skipped: a free non-basic column in the row */
    uint64_t nnz;               /* terms of the appended cuts (slack entries of the new rows not counted) */
    uint64_t batches;           /* batches of 16 requests: one pass over A each */
    double bytes;               /* algorithmic bytes of the generation */
    double device_ms;           /* its time on the device (HIP events around the generation launches) */
} mlp_gmi_info;
int mlp_solution_gmi_info(const mlp_solution* s, mlp_gmi_info* out);
uint64_t mlp_gmi_info_size(void);

/* ---- Branching penalties: one-pivot bounds for both branches of a variable (Driebeek-Tomlin) -----------------------------------------------
 * What does it cost to branch on x_j?  The penalty of a branch is the objective change of the FIRST dual-simplex pivot after the bound
 * x_j <= floor(x_j) (down) or x_j >= ceil(x_j) (up) is imposed: a lower bound on the degradation of that child, read from the tableau row
 * of x_j without a re-solve.  The call also names the column that would enter, and it proves a branch infeasible when no column can.
 * Internal form, as for the ranging and the tableau reads above: min c^.x, A x + s = b, with c^ = -c for a Maximize problem.  Columns:
 * j < num_vars is structural variable j, num_vars + c the slack of constraint c.  d are the internal reduced costs of the dual-value read.
 * A request is a structural variable j.
 *   non-basic j: frac = xN_j - floor(xN_j), down = up = 0, both columns -1, status 1.  This is no error: drivers pass whole lists.
 *   basic j at position p: x = xB_p, f_dn = x - floor(x), f_up = ceil(x) - x, frac = f_dn.  If f_dn == 0 exactly: answered as a non-basic
 *     request.  Otherwise status 0, and over every non-basic column i with alpha_i = (e_p^T B^-1) abar_i (|alpha_i| <= 1e-8 counts as
 *     zero) and the numerator |d_i| (a reduced cost of the wrong sign clamped to 0, exactly as the cost ranging does it):
 *       eligible in the down branch (x_j must fall by f_dn): i at lower with alpha_i > 0, or at upper with alpha_i < 0;
 *       eligible in the up branch: the mirror image;
 *       MLP_NB_FREE with alpha_i != 0: eligible both ways with ratio 0;   MLP_NB_FIXED: never eligible;
 *       rho_i = |d_i| / |alpha_i|.
 *     down = f_dn * min rho_i over the down set, up = f_up * min rho_i over the up set; an empty set gives +inf: that branch is infeasible
 *     for the bounds the call finds (a bound tightened by mlp_solution_fix_var counts).  down_col / up_col are the minimising columns;
 *     among exactly equal candidates the lowest column number wins; -1 for an empty set.
 * Tomlin's strengthening (optional): a column that is marked integer (structural columns by var_is_int, slacks by con_is_int, as for
 *   mlp_solution_add_gmi_cuts), whose status is at lower or at upper and whose xN_i == floor(xN_i) exactly must itself move by at least 1
 *   in an integer solution, so it takes the candidate T_i = max(f * rho_i, |d_i|) instead of f * rho_i; the result is min T_i with the same
 *   tie rule.  The strengthened numbers bound the integer-feasible descendants of the branch, NOT the child LP.  var_is_int == NULL:
 *   nothing is strengthened (num_vars is then ignored, and con_is_int must be NULL too).
 * User's sense: both numbers are non-negative DEGRADATIONS and no sign is turned: the child's bound is objective() + down for a Minimize
 *   problem and objective() - down for a Maximize problem.
 * The numbers are those of the CURRENT basis, whatever it is; they are bounds at a dual-feasible basis (an optimum, or the basis a
 *   mutator's re-solve ends in) and the same formulas, never an error, on a budget-limited solve — like the ranging.
 * The six outputs of a request are bit for bit the same alone, anywhere in any call and from run to run (16 requests share one pass over
 *   A; the minimum over the columns is exact).  Duplicates are allowed; n == 0 is a successful no-op.  The call is a read, side-effect
 *   free like the ranging: no solution is freed and no cache is dropped.
 * MLP_EINVAL: a variable out of range, a mask length that does not fit (num_vars != mlp_solution_num_vars with var_is_int given,
 *   num_constraints != mlp_solution_num_constraints with con_is_int given, con_is_int without var_is_int), a sharded solution, NULL
 *   handles or outputs.
 * mlp_branch_info: counters of the last mlp_solution_branch_penalties call on this solution (zeros before the first).  Only grows at its
 *   end; mlp_branch_info_size() is its size as the library was built. */
int mlp_solution_branch_penalties(const mlp_solution* s, const uint32_t* vars, uint64_t n, const uint8_t* var_is_int, uint32_t num_vars,
                                  const uint8_t* con_is_int, uint64_t num_constraints, double* down, double* up, int64_t* down_col,
                                  int64_t* up_col, double* frac, int32_t* status);
typedef struct mlp_branch_info {
    uint64_t requests;   /* variables asked for */
    uint64_t solves;     /* of them: basic fractional requests, which reached the device */
    uint64_t batches;    /* batches of 16 of them: one pass over A each */
    double bytes;        /* algorithmic bytes of the batches */
    double device_ms;    /* their time on the device (HIP events around the launches) */
} mlp_branch_info;
int mlp_solution_branch_info(const mlp_solution* s, mlp_branch_info* out);
uint64_t mlp_branch_info_size(void);

/* ---- Reduced-cost bounds from a cutoff, and fixing many variables in one call ------------------------------------------------------------
 * Once an incumbent exists, the reduced cost of a non-basic column bounds how far the column can move before the objective of this LP
 * passes the incumbent (weak duality).  mlp_solution_cutoff_bounds lists every structural variable whose bound tightens that way;
 * mlp_solution_fix_vars applies such a list — or a dive, or a multi-variable branch — in one call; mlp_solution_unfix_vars releases one.
 *
 * mlp_solution_cutoff_bounds (a read).  Internal form as above: min c^.x with c^ = -c for a Maximize problem.  The gap is
 *   g = cutoff - mlp_solution_objective() for a Minimize problem and mlp_solution_objective() - cutoff for a Maximize problem, formed
 *   exactly, without a tolerance.  g < 0: the node is worse than the cutoff, *pruned = 1, *count = 0, status 0.  g = +inf lists nothing.
 *   d_j is the internal reduced cost of column j as the engine's pricing holds it on the device; it agrees with
 *   mlp_solution_reduced_costs (turned to the internal sense) to rounding.  Structural variables only: a slack has no bound to apply.
 *     basic, MLP_NB_FREE and MLP_NB_FIXED columns impose nothing;
 *     at lower with d_j > 0:  t = g / d_j,   new_hi = lo_j + t;     at upper with d_j < 0:  t = g / |d_j|,   new_lo = hi_j - t;
 *     a reduced cost of the wrong sign (-1e-13 at a lower bound) counts as 0, as in the cost ranging, and gives no entry;
 *     var_is_int[j] != 0 and xN_j == floor(xN_j) exactly (the test of Tomlin's strengthening above): t is replaced by floor(t + 1e-9)
 *       — the 1e-9 can only loosen the bound.  var_is_int == NULL: no variable is integer (num_vars is still checked).
 *   A variable is listed only if the bound strictly tightens (new_hi < hi_j, or new_lo > lo_j).  An entry carries BOTH bounds,
 *   (lo_j, new_hi) or (new_lo, hi_j); a tightened bound that reaches the other bound is clamped to it, so such an entry has
 *   new_lo == new_hi == xN_j: the variable can be fixed.  Bounds are in the user's terms, no sign is turned for Maximize.
 *   Entries come in ascending variable number; *count is always set; cap < *count is MLP_EINVAL with nothing written (cap = num_vars
 *   always suffices).  The list is bit-identical from run to run (one classifying pass, compaction by ballots and prefix counts, no
 *   atomics).  The call is a read, side-effect free like the ranging: the host reads back the count and O(count) entries.
 *   MLP_EINVAL: a solution that is not solved (budget-limited or paused: the bound is false at a dual-infeasible basis), a NaN cutoff,
 *   num_vars != mlp_solution_num_vars, a sharded solution, NULL handle / count / pruned.
 *
 * mlp_solution_fix_vars leaves the model that mlp_solution_fix_var(vars[i], vals[i]) for i = 0, 1, ... would leave; only the pivot path
 *   differs, so the optimum value is the same.  Checked before anything changes: a variable out of range or listed twice is MLP_EINVAL;
 *   a value outside [lo, hi] is status 1 (Infeasible), as for the single form.  Then
 *     1. all requests NON-BASIC at the basis the call finds are served together: r = sum_j (val_j - xN_j) a_j is formed on the device in
 *        an order that does not depend on the order of the list, ONE FTRAN follows, x_B -= B^-1 r, the objective moves by
 *        sum_j (val_j - xN_j) d_j (ascending variable number), xN_j = val_j and the columns become MLP_NB_FIXED.  When every variable
 *        already sits at its value — reduced-cost fixing — there is no solve: only the flags are written, and values and objective keep
 *        their bits;
 *     2. each BASIC request, in list order, leaves the basis by the forced dual pivot of the single form (an Infeasible verdict of that
 *        pivot is status 1); the columns fixed in step 1 cannot enter;
 *     3. feasibility is restored ONCE (status 1 if the fixings are infeasible together).
 * mlp_solution_unfix_vars applies the rule of mlp_solution_unfix_var to every request — a basic or not-fixed variable is skipped (this
 *   includes a second mention), the status of a released one is rebuilt from its value against its bounds — and runs ONE primal re-solve
 *   if any was released; *unfixed (may be NULL) = the released count.  If none was, the solution is left exactly as it is.
 * Both: n == 0 is a successful no-op; any non-zero status frees the solution and sets *s = NULL; a sharded solution is MLP_EINVAL; a
 *   pivot budget is lifted; cached duals and ranges are dropped.
 * mlp_fix_info: what the last of these three calls on this solution did (zeros before the first).  Only grows at its end;
 *   mlp_fix_info_size() is its size as the library was built. */
int mlp_solution_cutoff_bounds(const mlp_solution* s, double cutoff, const uint8_t* var_is_int, uint32_t num_vars, uint32_t* vars,
                               double* new_lo, double* new_hi, uint64_t cap, uint64_t* count, int* pruned);
int mlp_solution_fix_vars(mlp_solution** s, const uint32_t* vars, const double* vals, uint64_t n);
int mlp_solution_unfix_vars(mlp_solution** s, const uint32_t* vars, uint64_t n, uint64_t* unfixed);
typedef struct mlp_fix_info {
    uint64_t requests;       /* fix_vars / unfix_vars: variables listed */
    uint64_t nonbasic;       /* fix_vars: of them non-basic at the basis the call found (served together) */
    uint64_t shifted;        /* ... of them with val != xN */
    uint64_t forced_pivots;  /* fix_vars: basic requests, one forced dual pivot each */
    uint64_t solves;         /* fix_vars: FTRANs of the non-basic requests, 0 or 1 */
    uint64_t unfixed;        /* unfix_vars: variables released */
    uint64_t listed;         /* cutoff_bounds: entries */
    uint64_t listed_fixed;   /* ... of them with new_lo == new_hi */
    uint64_t pivots;         /* iterations of the call: the forced pivots and the re-solve */
    double bytes;            /* algorithmic bytes of the batched device work (without the re-solve) */
    double device_ms;        /* its time on the device (HIP events around the launches) */
    double wall_ms;          /* the whole mutator call on the host, re-solve included (0 for the read) */
} mlp_fix_info;
int mlp_solution_fix_info(const mlp_solution* s, mlp_fix_info* out);
uint64_t mlp_fix_info_size(void);

/* ---- New bounds for the structural variables of a solved model ------------------------------------------------------------------------------
 * mlp_solution_set_var_bounds gives the listed structural variables the bounds [lo[i], hi[i]] (the user's terms: no sign is turned for
 *   Maximize) and re-solves with the dual simplex from the basis it finds.  The model keeps its rows: nothing is appended, nothing is
 *   re-inverted.  It needs a solved model (primal and dual feasible, no exhausted pivot budget), as mlp_solution_cutoff_bounds does: the
 *   path rests on a dual-feasible basis and never re-enters the primal loop.
 *   Checked before anything changes, each MLP_EINVAL: a variable out of range or listed twice; a NaN bound, lo = +inf or hi = -inf; a
 *   column fixed by mlp_solution_fix_var(s) whose value lies outside [lo, hi] (a fixed column otherwise keeps its value and its
 *   MLP_NB_FIXED status, only its bounds change; mlp_solution_unfix_var(s) later rebuilds its status against the new bounds); a
 *   solution that is not solved.  lo > hi is status 1 (Infeasible), like a value outside the bounds in mlp_solution_fix_vars.  Then
 *     1. one classifying pass over the requests (the host sorts them by variable; only private buffers are written).  A BASIC column
 *        gets no target: only its bounds move.  A NON-BASIC, not fixed column keeps its side: at lower -> target lo, at upper -> target
 *        hi, both flags set (lo == hi before the call) -> lower if the internal d_j >= 0, else upper, MLP_NB_FREE ->
 *        clamp(xN_j, lo, hi); diff_j = target_j - xN_j, and the new flags come from the target against lo / hi.
 *        REFUSAL: if the new bound on the side a non-basic column sits at is infinite, the column would have to change sides and the
 *        basis would lose dual feasibility; the dual path cannot serve such a request.  If the pass counts one, the call is MLP_EINVAL
 *        with nothing changed (mlp_last_error says how many).  Unfix or re-solve from a Problem with the new bounds instead.
 *     2. if any diff_j != 0: r = sum_j diff_j a_j is formed on the device in an order that does not depend on the order of the list,
 *        ONE FTRAN follows, x_B -= B^-1 r; the objective moves by sum_j diff_j d_j (ascending variable number, a fixed tree); xN_j,
 *        the flags and the bounds are written.  Two calls with the same list in different orders leave bit-identical state.
 *     3. ONE dual re-solve after a shift, or when a basic value now violates its bounds (an Infeasible verdict is status 1).  When
 *        nothing moved and no basic value violates, values and objective keep their bits and there is no pivot.
 *   A basis blob saved after the call carries no bounds: mlp_problem_solve_from_basis needs a Problem that has the bounds wanted.
 * mlp_solution_tighten_by_reduced_cost is mlp_solution_cutoff_bounds (the same gap, marks, *pruned and refusals) with EVERY entry
 *   applied, without the list leaving the device; the host reads back the count (*tightened) only.  A listed column is non-basic at the
 *   bound that does not move, so nothing shifts: no FTRAN, no re-solve, values and objective keep their bits.  An entry with
 *   new_lo == new_hi keeps its plain at-bound status; it is not marked MLP_NB_FIXED (that is what fix_vars is for).  A second call at
 *   the same cutoff tightens nothing.  *pruned = 1 changes nothing.
 * mlp_solution_var_bounds reads the current bounds of the listed variables (vars == NULL: all of them, n = mlp_solution_num_vars).
 * The two mutators: n == 0 is a successful no-op; any non-zero status frees the solution and sets *s = NULL; a sharded solution is
 *   MLP_EINVAL; a pivot budget is lifted; cached duals and ranges are dropped.
 * mlp_bounds_info: what the last of the two mutators on this solution did (zeros before the first).  Only grows at its end;
 *   mlp_bounds_info_size() is its size as the library was built. */
int mlp_solution_set_var_bounds(mlp_solution** s, const uint32_t* vars, const double* lo, const double* hi, uint64_t n);
int mlp_solution_tighten_by_reduced_cost(mlp_solution** s, double cutoff, const uint8_t* var_is_int, uint32_t num_vars,
                                         uint64_t* tightened, int* pruned);
int mlp_solution_var_bounds(const mlp_solution* s, const uint32_t* vars, uint64_t n, double* lo, double* hi);
typedef struct mlp_bounds_info {
    uint64_t requests;   /* set_var_bounds: variables listed; tighten_by_reduced_cost: entries applied */
    uint64_t basic;      /* of them basic at the basis the call found (only their bounds move) */
    uint64_t nonbasic;   /* of them non-basic */
    uint64_t shifted;    /* ... of them whose value moved with its bound */
    uint64_t solves;     /* FTRANs of the shift, 0 or 1 */
    uint64_t tightened;  /* tighten_by_reduced_cost, tighten_by_propagation: entries applied */
    uint64_t pivots;     /* iterations of the dual re-solve */
    double bytes;        /* algorithmic bytes of the device work (without the re-solve) */
    double device_ms;    /* its time on the device (HIP events around the launches) */
    double wall_ms;      /* the whole call on the host, re-solve included */
} mlp_bounds_info;
int mlp_solution_bounds_info(const mlp_solution* s, mlp_bounds_info* out);
uint64_t mlp_bounds_info_size(void);

/* ---- Bound propagation from row activities (node presolve) --------------------------------------------------------------------------------
 * mlp_solution_propagate_bounds lists the bounds that the rows of the model imply on its structural variables, given the bounds and
 *   the fixings it holds now.  The work is done on the device: two streaming passes over A per round.
 *   THE MODEL is the engine's internal form.  The variables are the columns j of [A | I]: j < num_vars structural, num_vars + r the slack
 *   of row r; their bounds [l_j, u_j] are the ones the solution holds now (mlp_solution_var_bounds; a slack: [0, inf) for '<=',
 *   (-inf, 0] for '>=', [0, 0] for '='); a non-basic column flagged MLP_NB_FIXED by mlp_solution_fix_var(s) is [xN_j, xN_j].  Every row
 *   is the equality sum_j a_rj x_j = rhs_r over ALL its stored entries: its own slack, and the slacks of other rows that a cut row taken
 *   from the tableau carries.  No sign is turned for Maximize.  Basis, values and reduced costs are not read: the result is a property
 *   of the model and the fixed flags, bit-identical whatever the basis, and bit-identical from run to run.
 *   ONE ROUND is a Jacobi sweep: every candidate comes from the bounds at the start of the round.
 *     per row:   minfin_r = the sum of the finite minimal contributions (a l_j for a > 0, a u_j for a < 0), mininf_r = the number of
 *                infinite ones; maxfin_r, maxinf_r mirrored (a u_j for a > 0, a l_j for a < 0).  A stored zero contributes nothing.
 *     per entry (r, j), own = the contribution of j itself:
 *                rest_min = minfin_r - own   if own is finite and mininf_r == 0,
 *                           minfin_r         if own is infinite and mininf_r == 1,
 *                           -inf             otherwise;                              rest_max mirrored (+inf otherwise);
 *                a > 0:  upper candidate (rhs_r - rest_min) / a,  lower candidate (rhs_r - rest_max) / a;   a < 0: the two swap.
 *                An infinite candidate imposes nothing.
 *     per column: u' = the minimum of its upper candidates, l' = the maximum of its lower candidates;
 *                var_is_int[j] != 0 (structural variables only):  u' = floor(u' + 1e-9),  l' = ceil(l' - 1e-9);
 *                u' is accepted if u is infinite and u' finite, or if u' < u - 1e-7 max(1, |u|); l' likewise (l' > l + 1e-7 max(1, |l|));
 *                an accepted l' that exceeds the round's u by at most 1e-9 max(1, |u|) is clamped to u; if it exceeds it by more the
 *                model is INFEASIBLE.  An accepted u' against the round's l: the same, mirrored.
 *   The rounds stop after one that accepts nothing, or after max_rounds (1..64; 10 is a good default).  INFEASIBLE stops the call at
 *   once: *infeasible = 1, *count = 0, status 0.
 *   THE LIST holds the structural variables whose bounds after the last round differ from the bounds at the start, MLP_NB_FIXED columns
 *   excluded, in ascending variable number, each entry with BOTH bounds; new_lo == new_hi: the variable can be fixed.  Slack bounds
 *   tighten too, in the working copy of the call, where they carry information from round to round; they are never listed and never
 *   written to the solution.  *count and *infeasible are always set; cap < *count is MLP_EINVAL with nothing written (cap = num_vars
 *   always suffices).  var_is_int == NULL: no variable is integer (num_vars is still checked).
 *   The call is a read, side-effect free, and works on ANY state of a solution, a budget-limited or paused solve included.
 *   MLP_EINVAL: NULL handle / count / infeasible, num_vars != mlp_solution_num_vars, max_rounds outside 1..64, a sharded solution.
 * mlp_solution_tighten_by_propagation runs that read and applies the WHOLE list through the body of mlp_solution_set_var_bounds: one
 *   classification, at most one FTRAN, at most one dual re-solve; mlp_bounds_info describes the application.  Like set_var_bounds it
 *   needs a solved model (else MLP_EINVAL).  *tightened = the length of the list.  *infeasible = 1 changes nothing and is status 0: the
 *   caller prunes.  A re-solve that ends Infeasible (or a list whose bounds cross) is status 1; like every mutator, any non-zero status
 *   frees the solution and sets *s = NULL.  A pivot budget is lifted; cached duals and ranges are dropped.
 * mlp_propagate_info: what the last of the two calls on this solution did (zeros before the first).  Only grows at its end;
 *   mlp_propagate_info_size() is its size as the library was built. */
int mlp_solution_propagate_bounds(const mlp_solution* s, const uint8_t* var_is_int, uint32_t num_vars, int32_t max_rounds, uint32_t* vars,
                                  double* new_lo, double* new_hi, uint64_t cap, uint64_t* count, int* infeasible);
int mlp_solution_tighten_by_propagation(mlp_solution** s, const uint8_t* var_is_int, uint32_t num_vars, int32_t max_rounds,
                                        uint64_t* tightened, int* infeasible);
typedef struct mlp_propagate_info {
    uint64_t requests;      /* columns of [A | I] scanned per round */
    uint64_t rounds;        /* rounds run (the last one accepted nothing, found the model infeasible, or was round max_rounds) */
    uint64_t accepted;      /* bound changes accepted over all rounds, slacks included */
    uint64_t listed;        /* entries of the list */
    uint64_t listed_fixed;  /* ... of them with new_lo == new_hi */
    double bytes;           /* algorithmic bytes of the device work (without the application) */
    double device_ms;       /* its time on the device (HIP events around the launches, the per-round reads of 8 bytes included) */
} mlp_propagate_info;
int mlp_solution_propagate_info(const mlp_solution* s, mlp_propagate_info* out);
uint64_t mlp_propagate_info_size(void);

/* ---- New right-hand sides for a solved model, and the batched what-if read ---------------------------------------------------------------
 * mlp_solution_set_rhs gives constraint constraints[i] the right-hand side rhs[i] (the user's terms: no sign is turned for Maximize) and
 *   re-solves with the dual simplex from the basis it finds.  Constraints are numbered as mlp_solution_num_constraints counts them:
 *   mlp_problem_add_constraint order, then the rows appended to the solution, cut rows included.  Operators and slack bounds stay as
 *   they are: internally the row stays a.x + s = rhs with s in [0, inf) for '<=', (-inf, 0] for '>=', [0, 0] for '='.  The reduced costs
 *   do not depend on the right-hand side, so the basis stays dual feasible and the primal loop is never entered.  It needs a solved model
 *   (primal and dual feasible, no exhausted pivot budget), as mlp_solution_set_var_bounds does.
 *   Checked before anything changes, each MLP_EINVAL: a NULL handle or a NULL array (n > 0); a constraint out of range or listed twice; a
 *   NaN or infinite value; a solution that is not solved; a solution sharded over several ranks.  (A one-rank pump is accepted, as by
 *   every mutator; mlp_solution_rhs_scenarios below refuses that one too.)
 *   A constraint without terms has no row: its new right-hand side is stored and read back by mlp_solution_constraint_rhs; if 0 op rhs
 *   is then false the call is status 1 (Infeasible), as mlp_problem_solve treats such a row.  Then
 *     1. the host sorts the requests by row, forms delta_r = rhs' - rhs against the vector it holds and drops exact zeros.
 *     2. if any delta is non-zero: the deltas are scattered into a zeroed block, ONE FTRAN y = B^-1 delta follows (the dense
 *        right-hand-side path of whichever representation of B^-1 is live), x_B += y by position, and the objective moves by
 *        sum_p c_B[p] y[p] (c_B: the internal cost of the column basic at p), summed over the positions in a fixed order: bit-identical
 *        from run to run and whatever the order of the list.
 *     3. the host's right-hand-side vector follows; it is the only resident copy, and the certificate, the propagation, the
 *        recomputation of the basic values, the row append and mlp_solution_clone all read it.
 *     4. ONE dual re-solve if a basic value now violates its bounds (an Infeasible verdict is status 1).  Otherwise there is no pivot.
 *   A call whose values all equal the current ones leaves every bit of the state (no FTRAN: mlp_rhs_info.solves == 0).
 *   A basis blob saved after the call carries no right-hand side: it belongs with a Problem that has the same right-hand sides.
 *   n == 0 is a successful no-op on any live handle that is not sharded over several ranks, one that is not solved included: as with
 *   mlp_solution_set_var_bounds, the checks of the model's state run only when something is listed.  Any non-zero status
 *   frees the solution and sets *s = NULL; a pivot budget is lifted; cached duals and ranges are dropped.
 * mlp_solution_constraint_rhs reads the current right-hand sides of the listed constraints (constraints == NULL: all of them,
 *   n = mlp_solution_num_constraints).  A host read that works on any state.  MLP_EINVAL: NULL handle / output, an index out of range.
 * mlp_solution_rhs_scenarios evaluates num_scenarios candidate right-hand sides against the current basis, 16 per batch, on the device.
 *   rhs is [num_scenarios][n], row-major: scenario s gives constraints[i] the right-hand side rhs[s * n + i], every other constraint keeps
 *   its own.  Nothing is changed: only private buffers are written.  It needs a solved model; the refusals are those of set_rhs (like
 *   the tableau reads, whose solve it runs, it also refuses a solution sharding was enabled on, a one-rank pump included), and every
 *   listed constraint must have a row (else MLP_EINVAL).  Per scenario, with y_s = B^-1 (b_s - b):
 *     bound[s]     = mlp_solution_objective as the scenario's basis would report it: internally obj + sum_p c_B[p] y_s[p] (the order of
 *                    set_rhs's sum), turned into the user's sense.  It is the value of the current dual solution at b_s: the scenario's
 *                    optimum where feasible[s] is set, otherwise a bound on it from the dual side (below for Minimize, above for
 *                    Maximize; an infeasible scenario has no optimum).
 *     feasible[s]  = 1 if no position p has x_B[p] + y_s[p] outside [loB[p] - 1e-8, hiB[p] + 1e-8] — the test of the dual pricing, so
 *                    it says "mlp_solution_set_rhs of this scenario would run zero pivots" — else 0.
 *     worst[s]     = the largest such violation (0.0 when feasible).
 *     worst_col[s] = the column basic at the position of that violation, the lowest position on a tie; -1 when feasible.  Column
 *                    numbering of mlp_solution_basis_head.
 *   A scenario's four results are bit-identical whatever else is in the call: its place, its neighbours, num_scenarios and the order of
 *   the constraints do not enter.  n == 0: every scenario is feasible with bound = mlp_solution_objective.  The host reads back four
 *   numbers per scenario, never a block.
 * mlp_rhs_info: what the last of mlp_solution_set_rhs / mlp_solution_rhs_scenarios on this solution did (zeros before the first).  Only
 *   grows at its end; mlp_rhs_info_size() is its size as the library was built. */
int mlp_solution_set_rhs(mlp_solution** s, const uint64_t* constraints, const double* rhs, uint64_t n);
int mlp_solution_constraint_rhs(const mlp_solution* s, const uint64_t* constraints, uint64_t n, double* rhs);
int mlp_solution_rhs_scenarios(const mlp_solution* s, const uint64_t* constraints, uint64_t n, const double* rhs, uint64_t num_scenarios,
                               double* bound, uint8_t* feasible, double* worst, int64_t* worst_col);
typedef struct mlp_rhs_info {
    uint64_t requests;   /* constraints listed */
    uint64_t changed;    /* set_rhs: of them with a right-hand side that differs from the current one (rowless ones included) */
    uint64_t scenarios;  /* rhs_scenarios: scenarios evaluated */
    uint64_t solves;     /* right-hand sides sent through the FTRAN (set_rhs: 0 or 1) */
    uint64_t batches;    /* batches of 16 right-hand sides */
    uint64_t pivots;     /* set_rhs: iterations of the dual re-solve */
    double bytes;        /* algorithmic bytes of the device work (without the re-solve) */
    double device_ms;    /* its time on the device (HIP events around the launches) */
    double wall_ms;      /* the whole call on the host, re-solve included */
} mlp_rhs_info;
int mlp_solution_rhs_info(const mlp_solution* s, mlp_rhs_info* out);
uint64_t mlp_rhs_info_size(void);

/* ---- MPS (mps.rs:39 MpsFile::parse) ------------------------------------------------------ */
typedef struct mlp_mps mlp_mps;
int mlp_mps_parse(const char* text, uint64_t len, int direction, mlp_mps** out);
void mlp_mps_free(mlp_mps* f);
const char* mlp_mps_name(const mlp_mps* f);                 /* MpsFile::problem_name mps.rs:11 */
uint32_t mlp_mps_num_vars(const mlp_mps* f);
const char* mlp_mps_var_name(const mlp_mps* f, uint32_t i); /* MpsFile::variables mps.rs:13 */
int64_t mlp_mps_var_index(const mlp_mps* f, const char* name);
mlp_problem* mlp_mps_problem(const mlp_mps* f);             /* MpsFile::problem mps.rs:15 (a clone) */

/* ---- engine-level stepping (second table) --------------------------------------------
 * The iteration of Solver::optimize / restore_feasibility (solver.rs:487-547) one stage per call, paced
 * by the host: what a host-side Solver would bind instead of BasisSolver::{solve, solve_transp,
 * push_eta_matrix} (solver.rs:1273-1339) and the scans of choose_pivot / pivot.  Every stage runs the
 * same kernels as the replayed graph; vectors stay on the device (read them with mlp_solution_state:
 * "col_coeffs" after FTRAN, "row_coeffs" after ROW, ...); only the scalars below cross the boundary.
 *
 *   mlp_problem_solve_ex(p, &s, 0, 0);                         // set up, no pivot yet
 *   while (mlp_engine_open(s, &info) == MLP_ITER_PIVOT)        // pricing: entering column (primal) / leaving row (dual)
 *       do st = mlp_engine_stage(s, info.next_stage, &info);   // FTRAN, RATIO, BTRAN, BASIS, ROW, APPLY in the phase's order
 *       while (st == MLP_ITER_PIVOT || st == MLP_ITER_FLIP);   // after APPLY the next iteration is already priced
 *
 * mlp_engine_open picks the phase initial_solve would run next (dual loop while primal-infeasible,
 * then recalc_obj_coeffs + primal loop) and returns the status of the pricing decision; a terminal
 * status (OPTIMAL, FEASIBLE, INFEASIBLE, UNBOUNDED) closes the loop, after FEASIBLE call open again.
 * Return values < 0 are errors (mlp_last_error), e.g. a stage called out of order. */
enum { MLP_STAGE_FTRAN = 0, MLP_STAGE_RATIO = 1, MLP_STAGE_BTRAN = 2, MLP_STAGE_BASIS = 3, MLP_STAGE_ROW = 4, MLP_STAGE_APPLY = 5 };
enum { MLP_ITER_PIVOT = 0, MLP_ITER_FLIP = 1, MLP_ITER_OPTIMAL = 2, MLP_ITER_UNBOUNDED = 3, MLP_ITER_FEASIBLE = 4,
       MLP_ITER_INFEASIBLE = 5, MLP_ITER_SINGULAR = 6 };
typedef struct mlp_iter_info {
    int32_t status;      /* MLP_ITER_* of the open iteration (after APPLY: of the next one) */
    int32_t phase;       /* 0 primal (optimize), 1 dual (restore_feasibility) */
    int32_t next_stage;  /* the stage mlp_engine_stage expects next, -1 when no iteration is open */
    int32_t reserved;
    int64_t col, row;    /* entering non-basic position q, leaving basic position r (-1 while undecided) */
    int64_t entering_var, leaving_var;
    double pivot_coeff;  /* alpha_rq (solver.rs:1073) */
    double step;         /* change of the entering variable (solver.rs:828) */
    double objective;    /* cur_obj_val after the decision (solver.rs:1027) */
    uint64_t nucleus_size;
} mlp_iter_info;
int mlp_engine_open(mlp_solution* s, mlp_iter_info* out);
int mlp_engine_stage(mlp_solution* s, int stage, mlp_iter_info* out);

/* ---- driver helper (host only; examples/tsp.rs:437-539) -------------------------------------------
 * Stoer-Wagner global minimum cut of a dense symmetric n x n weight matrix (row-major, zero diagonal):
 * returns the cut weight and marks one side of the cut in side_out[n] (0/1).  Used by the TSP
 * cutting-plane driver to separate subtour-elimination constraints. */
double mlp_util_min_cut(uint32_t n, const double* weights, uint8_t* side_out);

#ifdef __cplusplus
}
#endif
#endif /* MINILP_HIP_H */
