// engine.h — host orchestration of the device-resident revised simplex (the "Solver" of
// solver.rs:14-58 with every vector in HBM and every hot loop a HIP kernel).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>
#include <map>
#include <utility>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/minilp_hip.h"  // the report structs (mlp_cut_info ...) are defined there, once
#include "batch.h"
#include "kernels.h"
#include "settings.h"

namespace mlp {

enum Stage { STAGE_FTRAN = 0, STAGE_RATIO = 1, STAGE_BTRAN = 2, STAGE_BASIS = 3, STAGE_ROW = 4, STAGE_APPLY = 5 };

struct MlpError : std::runtime_error {
    int code;
    MlpError(int c, const std::string& s) : std::runtime_error(s), code(c) {}
};
struct LpFail {  // lib.rs:172-178
    int code;    // 1 infeasible, 2 unbounded
};

#define HIPCHECK(expr)                                                                                   \
    do {                                                                                                 \
        hipError_t e__ = (expr);                                                                         \
        if (e__ != hipSuccess)                                                                           \
            throw ::mlp::MlpError(-3, std::string(#expr) + " failed: " + hipGetErrorString(e__) + " at " + \
                                          __FILE__ + ":" + std::to_string(__LINE__));                    \
    } while (0)

struct Constraint {  // lib.rs:199: (CsVec, ComparisonOp, f64) with sorted unique indices
    std::vector<int> idx;
    std::vector<double> val;
    int op;
    double rhs;
};
struct ProblemData {  // lib.rs:193-200
    int direction = 0;
    std::vector<double> obj, lo, hi;  // obj already negated for Maximize (lib.rs:235-238)
    std::vector<Constraint> cons;
    int add_var(double c, double mn, double mx);
    void add_constraint(const uint32_t* vars, const double* coeffs, uint64_t k, int op, double rhs);
};

// Process-wide cache of small device blocks.  A Solution owns ~50 device arrays; `Solution::clone`
// (one per branch-and-bound node in the TSP driver, lib.rs:313) and `drop` would otherwise pay one
// hipMalloc / hipFree each (hipFree synchronises the device).  Blocks are rounded up to a power of two
// and recycled; large blocks (W) go straight to the runtime.  A block is returned only after the
// owning stream has been synchronised, so the next owner may use it on any stream.
struct DevPool {
    static constexpr size_t kMaxBlock = (size_t)64 << 20;   // larger blocks are not cached
    static constexpr size_t kMaxCached = (size_t)4 << 30;   // total bytes kept in the cache
    static void* get(size_t bytes, size_t* got_bytes, int* device);   // on the current device
    static void* get_raw(size_t bytes, size_t* got_bytes, int* device);
    static void put(void* p, size_t bytes, int device);                // back to the free list of ITS device
    static void trim();  // hipFree everything cached
};

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;        // elements
    size_t bytes = 0;      // size of the block as obtained from the pool
    int dev = 0;           // device the block lives on
    DevBuf() {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) DevPool::put(p, bytes, dev);
        p = nullptr;
        cap = 0;
        bytes = 0;
    }
    // grow to hold n elements, preserving the first `keep` ones
    void ensure(size_t n, size_t keep, hipStream_t st) {
        if (n <= cap) return;
        size_t want = n + n / 2 + 64, got = 0;
        int ndev = 0;
        T* np = static_cast<T*>(DevPool::get(want * sizeof(T), &got, &ndev));
        if (p && keep) HIPCHECK(hipMemcpyAsync(np, p, keep * sizeof(T), hipMemcpyDeviceToDevice, st));
        if (p) {
            HIPCHECK(hipStreamSynchronize(st));
            DevPool::put(p, bytes, dev);
        }
        p = np;
        dev = ndev;
        bytes = got;
        cap = got / sizeof(T);
    }
    void alloc_exact(size_t n) {  // fresh allocation of (at least) n elements (contents undefined)
        release();
        size_t got = 0;
        p = static_cast<T*>(DevPool::get(n * sizeof(T), &got, &dev));
        bytes = got;
        cap = n;
    }
    void upload(const std::vector<T>& h, hipStream_t st) {
        ensure(h.size(), 0, st);
        if (!h.empty()) HIPCHECK(hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st));
    }
    void swap(DevBuf<T>& o) {
        std::swap(p, o.p); std::swap(cap, o.cap); std::swap(bytes, o.bytes); std::swap(dev, o.dev);
    }
    void copy_from(const DevBuf<T>& o, size_t n, hipStream_t st) {
        ensure(n, 0, st);
        if (n) HIPCHECK(hipMemcpyAsync(p, o.p, n * sizeof(T), hipMemcpyDeviceToDevice, st));
    }
};

struct PivotRecord {
    int32_t phase;
    int64_t col, row, entering_var, leaving_var;
    double pivot_coeff, obj_after;
};

struct Stats {
    uint64_t iterations = 0, basis_changes = 0, bound_flips = 0, primal_iters = 0, dual_iters = 0, reinversions = 0;
    double fused_bytes = 0, fused_ms = 0, sweep_bytes = 0, sweep_ms = 0;
    uint64_t fused_launches = 0, sweep_launches = 0, final_refreshes = 0;
    // FTRAN of the entering column (head + gather + F push): HIP-event time and algorithmic bytes
    double ftran_bytes = 0, ftran_ms = 0;
    uint64_t ftran_launches = 0;
    double iter_ms = 0;  // whole sampled iterations (first kernel to last), HIP events
    uint64_t iter_samples = 0;
    double update_ms = 0;
    uint64_t update_launches = 0;
    double solve_wall_s = 0;
    double max_pivot_err = 0;
    uint64_t reinversion_fallbacks = 0;  // (rounds 1-3: rocSOLVER inversions that reported a false zero pivot and were redone; always 0 since the blocked inversion is hand-written)
    double str_ms = 0;  // sampled sparse tableau rows (k_row_touch + k_row_pull, launch-bracketed HIP events)
    uint64_t str_launches = 0;
    uint64_t hyper_bail_reason[10] = {};  // by reason code of the kernel (hyper.inc)
    uint64_t hyper_iters = 0, hyper_bails = 0;  // iterations taken by the hypersparse kernel; iterations it handed back
    uint64_t ratio_stalls = 0;   // in-kernel waits of the fused ratio test that timed out (each one retried with two launches)
    uint64_t beta_rebuilds = 0;  // lazy dual steepest edge: exact rebuilds of beta from the basis inverse
    uint64_t fac_refactors = 0, fac_levels = 0, fac_switches = 0, fac_bump = 0, fac_bump_max = 0, fac_sb_factors = 0, fac_sb_fallbacks = 0, fac_sb_rounds = 0, fac_sb_tail = 0, fac_sb_skipped = 0;  // compact factor: refactorisations (peels), levels of the last one, mode switches
    // dense-rhs FTRAN x_B = B^-1 (b - N x_N) (recalc_basic_vals): the streaming read of the nucleus inverse, kernel-exact
    double dense_ftran_bytes = 0, dense_ftran_ms = 0;
    uint64_t dense_ftran_launches = 0;
    double fold_bytes = 0, fold_ms = 0;  // sampled folds of W0 (HIP events stamped by the kernel): read + write of the matrix
    uint64_t fold_launches = 0;
    uint64_t kase[5] = {0, 0, 0, 0, 0};  // partition-change cases: nuc->nuc, grow, shrink, col swap, same-row
};

// What ONE iteration launches, decided once (Engine::plan_iteration) for a (phase, DevView, Geom) and read by every stage
// (Engine::launch_stage).  Plain values; a plan is never compared and never part of a graph's key (get_graph compares Geom).
enum class IterForm : int { Plain, PrimalHead, SmallBasis, MediumRide, LargeRide, ShardedPull, Factor };  // each one's rule: plan_iteration
enum class FtranEntry : int { Fused, GatherLrh, PrepGather };  // head inside the gather kernel | delayed-update mode: the same | head launch + gather
enum class RowForm : int { Inside, Sparse, Sweep };            // Inside: the update kernel's workgroups pull the touched columns (no launch)
struct IterPlan {
    int phase, pse, dse, lazy, wtau, inl, fac;
    IterForm form;
    FtranEntry ftran;
    int ftran_ys, ftran_fpk;        // gather: + y_S by row (t_K ride) | no blocked push, the product is pulled in the ratio test's launch
    int tk_ride, rk_inside;         // launch_ratio_primal
    int v_ride;                     // ... its riders also form the v partials; the BASIS stage is launch_eta_vtail alone (MediumRide only)
    int btran, btran_rhs;           // a BTRAN launch exists | its with_rhs
    int sb_tk_inside;               // launch_small_basis
    int post_touch, post_rk_ride;   // launch_post_fused
    int basis_lists_touched;        // the BASIS stage (or the head) carries the touched-column list: the sparse row launches no k_row_touch
    RowForm row;
    int row_lists;                  // the dual ROW stage lists the non-zeros of alpha_r: the dual Harris test walks the list
    int pull_inside, with_struct;   // launch_update_pivot (pull_inside also gives k_primal_head its list / applies arguments)
    int fac_fused, fac_rho_part, fac_pair;  // compact factor: single-purpose launches inside the solves | MLP_FACTOR_RHO_PART | paired solves
};

class Engine {
public:
    explicit Engine(const Settings& settings);  // Settings::from_env() for a new Solution, the parent's cfg for a clone
    ~Engine();
    Engine(const Engine&) = delete;

    // Solver::try_new (solver.rs:108-369): throws LpFail{1} for min > max / contradictory empty rows
    void try_new(const ProblemData& pd);
    void initial_solve();                                                   // solver.rs:470-485
    void add_constraint(Constraint c);                     // solver.rs:549-634 (indices < num_total_vars): add_constraints of one row
    void fix_var(int var, double val);                                      // solver.rs:378-415
    bool unfix_var(int var);                                                // solver.rs:418-438
    void add_gomory_cut(int var);                                           // solver.rs:440-460
    // A round of cuts in one call (cuts.inc; include/minilp_hip.h mlp_solution_add_constraints_csr / mlp_solution_add_gomory_cuts): all
    // rows appended with ONE re-layout of the CSC, at most one re-inversion, the edge norms of every new row, ONE re-solve.  The model
    // left behind is that of the single forms called in the same order; only the pivot path of the re-solve differs.
    using CutInfo = mlp_cut_info;  // (the report structs are the public ones: no default initialisers, every declaration value-initialises)
    void add_constraints(std::vector<Constraint> cs, CutInfo& info, bool gomory = false);
    void add_gomory_cuts(const std::vector<int>& vars, CutInfo& info);  // the cut of add_gomory_cut for every listed (basic) variable
    // A round of Gomory mixed-integer cuts (gmi.inc; include/minilp_hip.h mlp_solution_add_gmi_cuts): one cut per listed
    // basic integer variable, all from the basis the call finds, appended through add_constraints.  var_is_int: num_vars marks;
    // con_is_int: num_constraints() marks of the slacks, or nullptr (all slacks continuous); status_out: vars.size() codes (0 emitted,
    // 1 skipped: fraction within away, 2 skipped: free non-basic column in the row), or nullptr.
    using GmiInfo = mlp_gmi_info;
    void add_gmi_cuts(const std::vector<int>& vars, const uint8_t* var_is_int, const uint8_t* con_is_int, double away, int32_t* status_out,
                      CutInfo& info, GmiInfo& gmi);
    double get_value(int var);                                              // solver.rs:371-376
    void get_values(double* out, int n);
    double cur_obj_val();                                                   // solver.rs:51
    Engine* clone();                                                        // #[derive(Clone)] solver.rs:14
    double reinvert(bool replace);  // from-scratch nucleus inversion; returns max |W - W_fresh|
    // Dual values, reduced costs and the KKT certificate of the current basis (duals.inc; include/minilp_hip.h
    // mlp_solution_dual_values ...): pi by CONSTRAINT (0 for a constraint without terms, which has no row), r by structural variable,
    // both in the user's objective sense.  Reads the state only: the solve continues bit for bit as if nothing had been read.
    struct Duals {
        std::vector<double> pi, r;
        double primal_obj = 0, dual_obj = 0, rel_gap = 0;
        double max_row_viol = 0, max_bound_viol = 0, max_dual_inf = 0, btran_residual = 0;
        int64_t row_viol_at = -1, bound_viol_at = -1, dual_inf_at = -1, btran_residual_at = -1;
        double bytes = 0, device_ms = 0;
        std::vector<double> r_int;  // reduced costs of ALL variables (slacks included) in the internal minimisation sense: the ranging's input
    };
    void compute_duals(Duals& out);
    // Basis status and cost / rhs ranging of the current basis (ranging.inc; include/minilp_hip.h mlp_solution_basis_status ...).
    // Status codes: 0 basic, 1 at lower, 2 at upper, 3 non-basic at neither bound, 4 non-basic fixed.  ranging(): kind 0 = cost ranges of
    // the structural variables idx[], kind 1 = rhs ranges of the constraints idx[], both in the user's sense; du = the duals of the same
    // state.  Reads the state only, like compute_duals.
    using RangingInfo = mlp_ranging_info;
    void basis_status(std::vector<int32_t>& vars, std::vector<int32_t>& cons);
    void ranging(int kind, const std::vector<uint64_t>& idx, const Duals& du, double* lo, double* hi, RangingInfo& info);
    // Branching penalties of the current basis (branch.inc; include/minilp_hip.h mlp_solution_branch_penalties): for every
    // listed structural variable the Driebeek–Tomlin bounds of its down and up branch, the columns that would enter (numbering of the
    // tableau reads, -1: none) and its fraction; status 0 = basic and fractional (served on the device, RG_BATCH per pass over A),
    // 1 = non-basic or integral (zeros).  var_is_int == nullptr: plain penalties.  Reads the state only, like ranging.
    using BranchInfo = mlp_branch_info;
    void branch_penalties(const std::vector<int>& vars, const uint8_t* var_is_int, const uint8_t* con_is_int, const Duals& du, double* down,
                          double* up, int64_t* down_col, int64_t* up_col, double* frac, int32_t* status, BranchInfo& info);
    // Reduced-cost bounds from a cutoff and the batched fixing of variables (fixing.inc; include/minilp_hip.h mlp_solution_cutoff_bounds,
    // mlp_solution_fix_vars, mlp_solution_unfix_vars).  FixInfo describes the last of the three calls.
    using FixInfo = mlp_fix_info;
    bool solved() const { return primal_feasible && dual_feasible && !budget_exhausted; }
    // g = cutoff - objective in the internal minimisation sense, exact: no tolerance (g < 0: the node is worse than the cutoff).  Refuses
    // a model that is not solved (the bound is a weak-duality argument: it needs a dual-feasible basis) and a NaN gap, in `who`'s name.
    double cutoff_gap(double cutoff, const std::string& who);
    // g from cutoff_gap (>= 0); var_is_int: num_vars marks or nullptr.  The list comes back in ascending variable number.  Reads the state
    // only, like ranging.
    void cutoff_bounds(double g, const uint8_t* var_is_int, std::vector<uint32_t>& vars, std::vector<double>& lo, std::vector<double>& hi,
                       FixInfo& info);
    // the model that fix_var(vars[i], vals[i]) for i = 0, 1, ... would leave: the requests non-basic at the basis the call finds are
    // served together (one FTRAN, none when nothing moves), the basic ones by one forced dual pivot each, feasibility restored once
    void fix_vars(const std::vector<int>& vars, const std::vector<double>& vals, FixInfo& info);
    uint64_t unfix_vars(const std::vector<int>& vars, FixInfo& info);  // unfix_var's rule per request, ONE optimize(); returns the released count
    // New bounds for structural variables of a solved model (fixing.inc, bounds.inc; include/minilp_hip.h mlp_solution_set_var_bounds,
    // mlp_solution_tighten_by_reduced_cost).  BoundsInfo describes the last of the two mutators.
    using BoundsInfo = mlp_bounds_info;
    // every non-basic request keeps its side and moves with its bound (one FTRAN for all, none when nothing moves), a basic request
    // only gets its bounds; ONE dual re-solve when a value moved or a basic value now violates its bounds
    void set_var_bounds(const std::vector<int>& vars, const std::vector<double>& lo, const std::vector<double>& hi, BoundsInfo& info);
    // cutoff_bounds with every entry applied on the device (g as there); the host reads back the count only
    uint64_t tighten_by_reduced_cost(double g, const uint8_t* var_is_int, BoundsInfo& info);
    void var_bounds(const uint32_t* vars, uint64_t n, double* lo, double* hi);  // vars == nullptr: all num_vars of them
    // Bound propagation from row activities (propagate.inc; include/minilp_hip.h mlp_solution_propagate_bounds,
    // mlp_solution_tighten_by_propagation).  The read works on any state and reads neither basis nor values: Jacobi
    // rounds over the model's rows, the bounds and the fixed flags; the list comes back in ascending variable number, empty when the
    // rounds prove the model infeasible.
    using PropagateInfo = mlp_propagate_info;
    void propagate_bounds(const uint8_t* var_is_int, int max_rounds, std::vector<uint32_t>& vars, std::vector<double>& lo,
                          std::vector<double>& hi, bool& infeasible, PropagateInfo& info);
    // the read, then the whole list through set_var_bounds (binfo describes that application); returns the length of the list
    uint64_t tighten_by_propagation(const uint8_t* var_is_int, int max_rounds, bool& infeasible, PropagateInfo& info, BoundsInfo& binfo);
    // New right-hand sides for a solved model and the batched what-if read (rhs.inc; include/minilp_hip.h mlp_solution_set_rhs,
    // mlp_solution_constraint_rhs, mlp_solution_rhs_scenarios).  RhsInfo describes the last of set_rhs / rhs_scenarios.
    using RhsInfo = mlp_rhs_info;
    // x_B += B^-1 (b' - b) with ONE FTRAN (none when no value differs), h_rhs follows, ONE dual re-solve if a basic value left its bounds
    void set_rhs(const std::vector<uint64_t>& cons, const std::vector<double>& rhs, RhsInfo& info);
    void constraint_rhs(const uint64_t* cons, uint64_t n, double* out) const;  // cons == nullptr: all num_constraints() of them
    // rhs[S][cons.size()]; per scenario the objective its basis would report (user's sense), whether x_B + B^-1 (b_s - b) stays within
    // the bounds, the largest violation and the column (numbering of basis_head, -1: none) basic where it occurs.  Reads the state only.
    void rhs_scenarios(const std::vector<uint64_t>& cons, const double* rhs, size_t S, double* bound, uint8_t* feasible, double* worst,
                       int64_t* worst_col, RhsInfo& info);
    // Reading the tableau of the current basis (tableau.inc; include/minilp_hip.h mlp_solution_binv_rows ...).  Columns:
    // j < num_vars structural, num_vars + c the slack of constraint c; vectors by row are exchanged by CONSTRAINT (0 / ignored for one
    // without a row), vectors by position have length num_rows().  Internal form A x + s = b: no sign turn for Maximize.  Requests are
    // served in batches of RG_BATCH.  Reads the state only, like compute_duals.
    using TableauInfo = mlp_tableau_info;
    int num_rows() const { return m_; }
    void basis_head(std::vector<uint64_t>& out);  // column basic at each position
    void binv_rows(const std::vector<uint64_t>& cols, double* out, TableauInfo& info);  // out[t][constraint] = (e_p^T B^-1), p = position of the basic column
    void binv_cols(const std::vector<uint64_t>& cons, double* out, TableauInfo& info);  // out[t][position] = B^-1 e_row
    void tableau_rows(const std::vector<uint64_t>& cols, std::vector<uint64_t>& indptr, std::vector<uint32_t>& indices, std::vector<double>& values,
                      TableauInfo& info);  // sparse rows e_p^T B^-1 [A | I], sorted by column, exact zeros and the other basic columns dropped
    void tableau_cols(const std::vector<uint64_t>& cols, double* out, TableauInfo& info);  // out[t][position] = B^-1 a_j
    // transpose = false: rhs[n][constraints] -> out[n][positions] = B^-1 rhs; true: rhs[n][positions] -> out[n][constraints] = B^-T rhs
    void basis_solve(bool transpose, const double* rhs, size_t n, double* out, TableauInfo& info);
    size_t num_constraints() const { return h_cons_row.size(); }
    double last_reinvert_scale = 0.0;  // max |W_fresh| of that comparison (state "reinvert_scale")
    // Basis checkpoint (include/minilp_hip.h: mlp_solution_save_basis / mlp_problem_solve_from_basis).
    // mode 0: basic / non-basic sets, flags and x_N; 1: + steepest-edge weights as f32; 2: + x_B, d, gamma,
    // beta, objective as f64 (a loaded solve continues pivot for pivot).
    std::vector<uint8_t> save_basis(int mode);
    void load_basis(const uint8_t* blob, size_t len);  // call after try_new on the same problem
    // column-block pricing across ranks.  transport: nullptr / "" = MLP_TRANSPORT or the default (device mailboxes written by the peers,
    // MLP_TRANSPORT=host for the host mailbox); "rccl" = records delivered by ncclAllGather (rccl_id: the 128-byte ncclUniqueId of
    // rank 0); "pump" = the same pump protocol with peer copies in place of the collective (ranks sharing one GPU: tests)
    void enable_sharding(int rank, int world, const char* shm_name, const char* transport_name = nullptr, const void* rccl_id = nullptr);
    static void rccl_unique_id(void* out128);
    bool sharded() const { return shard_world > 1; }

    const Settings cfg;  // every MLP_* knob, as the environment stood when the Solution was created (settings.h)
    int num_vars = 0;
    int direction = 0;
    int64_t pivot_budget = -1;
    bool budget_exhausted = false;
    bool resume_in_optimize = false;
    bool trace = false, profile = false;
    int sample_every = 0;  // profile mode: 0 = default cadence (every 8th / 4th batch), 1 = every iteration is a sampled eager one
    std::vector<PivotRecord> trace_log;
    Stats stats;
    uint64_t state(const char* what, double* out, uint64_t cap);
    int m() const { return m_; }
    int total_vars() const { return N_; }
    int nucleus() const { return k_; }
    int nucleus_cap() const { return cap_; }
    size_t nnz() const { return h_rcol.size(); }

private:
    // --- host mirror (integer bookkeeping + the matrix for rebuilds)
    int m_ = 0, N_ = 0, k_ = 0, cap_ = 0;
    std::vector<double> h_obj, h_lo, h_hi, h_rhs;
    // tighten_by_reduced_cost writes bounds on the device without the list leaving it: h_lo / h_hi of the structural variables are then
    // read back on first use.  Every host reader of h_lo / h_hi after set-up calls host_bounds() first.
    bool bounds_mirror_stale_ = false;
    void host_bounds();
    struct CutoffRun;  // the private device buffers of one run of launch_cutoff_bounds
    struct BasisRep;    // the representation of B^-1 one call finds, with the compact factor's private vectors (engine.hip)
    struct SolveBlock;  // the one owner of the blocks of a dense solve and of the TabBufs around them (engine.hip)
    double shift_basic_values(BoundBufs& b, SolveBlock& w, DevBuf<double>& delta);  // the shift that fix_vars and set_var_bounds share
    // The body that fix_vars and set_var_bounds share: classify the requests (ascending variable number), shift the basic values if a
    // request moves, commit, follow with the host mirrors.  before_commit sees the counts while nothing has changed yet and may refuse.
    struct Moves {
        int shifted = 0, basic = 0, infinite = 0;  // requests that move, basic requests, requests whose side has an infinite new bound
        uint64_t solves = 0;
        double bytes = 0, device_ms = 0;
    };
    Moves move_nonbasic(const std::vector<int>& var, const std::vector<double>& lo, const std::vector<double>& hi, bool fix,
                        const std::function<void(const Moves&)>& before_commit = nullptr);
    uint64_t release_fixed(const std::vector<int>& vars, FixInfo& info, const char* who);  // the body of unfix_var and unfix_vars
    void cutoff_launch(double g, const uint8_t* var_is_int, CutoffRun& r);
    void cutoff_alloc(const uint8_t* var_is_int, CutoffRun& r);
    // the length of r's list, checked against the number of variables (the error names `who`); vars != nullptr: the list as well
    int cutoff_read(const CutoffRun& r, const char* who, std::vector<uint32_t>* vars = nullptr, std::vector<double>* lo = nullptr,
                    std::vector<double>* hi = nullptr, uint64_t* listed_fixed = nullptr);
    std::vector<int> h_cons_row;  // constraint (Problem / Solution::add_constraint order) -> row; -1 for one without terms (no row)
    // a constraint without terms keeps its operator and right-hand side here, by constraint (h_rhs is by row): set_rhs / constraint_rhs
    struct Rowless {
        int op;
        double rhs;
    };
    std::map<uint64_t, Rowless> h_rowless_;
    // the checks set_rhs and rhs_scenarios share (nothing is written): solved, in range, no constraint twice
    void check_rhs_list(const std::vector<uint64_t>& cons, const char* who) const;
    struct RhsRun;  // the SolveBlock, the scan's partials and the outputs of one set_rhs / rhs_scenarios call
    // variable of [A | I] -> user column (j structural, num_vars + c the slack of constraint c; -1 stays -1), through row -> constraint
    struct ColumnMap {
        int num_vars;
        std::vector<int64_t> cons_of_row;
        int64_t operator()(int v) const { return v < 0 ? -1 : (v < num_vars ? (int64_t)v : (int64_t)num_vars + cons_of_row[v - num_vars]); }
    };
    ColumnMap user_columns() const;
    std::vector<int> h_rptr, h_rcol;
    std::vector<double> h_rval;
    // Host view of the columns: only what the host logic needs — the length of every column and, for singleton
    // columns, their single entry (classification of the basis in rebuild_inverse).  The CSC itself lives on the
    // device only (built there from the uploaded CSR-side arrays at try_new, re-laid out there by add_constraints).
    std::vector<int> h_cptr, h_crow;       // initial build only (try_new); dropped after the first device-side append
    std::vector<double> h_cval;
    int max_col_nnz_ = 0, max_row_nnz_ = 0;   // longest column / row of A (in-kernel stage heads need them to fit an LDS list)
    double amax_ = 0.0;                       // max |A_ij| (incl. the slack identity): scale bound of the deterministic blocked push
    bool force_det_push_ = false;             // set around recalc_basic_vals: the blocked push in its deterministic form
    bool pb_det_default = false;              // unsharded solves: deterministic blocked push by default (set from the measured A/B)
    bool ratio_two;                          // cfg.ratio_two, or latched by an ITER_STALL: two launches for the two Harris passes
    bool ranks_share_device = false;
    // the forms of the small-nucleus iteration, decided per batch (the geometry is baked into the graphs): sparse tableau row, k_small_basis,
    // k_primal_head (primal_head.inc: the batch is cut short so that the nucleus stays within the head's slots)
    // (geom() and sync_view read them; inside run_loop only enter_row_form and fit_head_room write them)
    struct BatchForm {
        bool str = false, sb = false, ph = false;
    } form;
    bool str_clean = false;  // alpha_r / helper are zero outside touched entries
    void leave_sparse_row();  // an iteration outside run_loop: dense tableau row, whatever the last batch used
    DevBuf<int> d_ar_list;   // non-basic positions with alpha_r != 0 (dual iteration, CSC-pull tableau row): the dual Harris test walks the list
    DevBuf<int> d_str_list;
    // hypersparse single-workgroup iteration (hyper.inc)
    static constexpr int hyper_backoff_max = 8;   // after bail-outs in a row the multi-kernel path keeps going for up to 2 << this pivots (swept 2..8 on config 3)
    uint64_t hyper_off_until = 0;            // lifetime pivot count until which the multi-kernel path runs (after bail-outs)
    int hyper_bail_streak = 0;
    DevBuf<int> d_hy_stamp;                  // n + m epoch stamps (alpha_r list / singleton part of the alpha_q list) + the kernel's derived maps
    DevBuf<double> d_hy_score;               // m dual pricing scores (derived by the kernel at every launch)
    size_t hy_stamp_len = 0;
    bool hyper_capable(int phase) const;
    // ---- compact factor of the basis (csrc/factor.inc, HISTORY.md §2.6): B^-1 = (peeled triangular factor of the
    // basis at the last refactorisation)^-1 + at most fac_J_ additive rank-1 terms, instead of the explicit nucleus inverse
    bool fac_on_ = false;
    bool fac_leaving_ = false;               // inside fac_leave: its re-inversion must not switch straight back
    int fac_J_;                              // rank-1 terms the factor has room for: cfg.fac_J, at most the solve's grid (fac_alloc)
    int fac_period_;                         // pivots between refactorisations: cfg.fac_period; in auto 48, or 64 while a refactorisation is expensive (fac_refactor)
    int fac_nlev_ = 0;
    uint64_t fac_tried_at_ = 0;              // lifetime pivot count of the last attempt that found a bump
    bool fac_tried_ = false;
    DevBuf<int> d_fac_pos_of_var, d_fac_var_of_pos, d_fac_prow, d_fac_items, d_fac_lptr, d_fac_meta, d_fac_tmp, d_fac_counters;
    DevBuf<double> d_fac_pval, d_fac_U, d_fac_V, d_fac_rhs, d_fac_x0, d_fac_coef, d_fac_part;
    DevBuf<unsigned> d_fac_bar;
    DevBuf<int> d_fac_bpos, d_fac_brow, d_fac_bslot_of_row, d_fac_irow, d_fac_fptr, d_fac_fidx, d_fac_bptr, d_fac_bidx;
    DevBuf<double> d_fac_ipiv, d_fac_fval, d_fac_bval;
    DevBuf<int> d_fac_lcount;
    DevBuf<double> d_fac_Kd, d_fac_Wtmp, d_fac_gjval;  // bump inversion: K, the work copy of the inverse, partial maxima | scratch
    DevBuf<int> d_fac_gjrow;
    DevBuf<int> d_fac_eslot;  // 2 nz: slots of the targets of the long edge lists (FTRAN | BTRAN)
    DevBuf<int> d_fac_ltslot, d_fac_segs;  // per level: first LDS slot (small levels) | the segments of a solve's walk
    DevBuf<double> d_fac_WbT;               // transpose of the bump inverse
    DevBuf<FacTailRec> d_fac_tprog;  // the tail of the solves as records: FTRAN | BTRAN, FAC_TAIL_CAP each
    DevBuf<int> d_fac_lev3;   // 3 m: level of a position | level of a row's pivot position | reach of a position
    static constexpr bool fac_skip_ = true;    // every solve walks only the levels its right-hand side can reach
    DevBuf<double> d_fac_Wb;   // allocated with the first bump
    static constexpr bool fac_pair_ = true;  // the two solves of a stage share one walk over the levels
    int fac_bump_ = 0;
    // sparse factor of the bump (factor_sb.inc)
    int fac_sb_fail_b_ = 0, fac_sb_fail_skip_ = 0;  // size of the last bump that failed the sparse elimination / refactorisations left before it is tried again
    bool fac_sb_on_ = false;                 // the current factor carries its bump sparsely
    DevBuf<int> d_fac_sb_int;                // integer scratch + outputs of the factorisation (FacSbWork)
    DevBuf<double> d_fac_sb_dbl;
    DevBuf<FacSbRec> d_fac_sb_rec;
    FacSbWork fac_sb_work(int m) const;
    void fac_alloc();
    void fac_fill_view(DevView& v) const;
    bool fac_refactor(int bump_limit = -1);  // the peel + level lists from the current basis; false when it leaves a bump beyond the limit (-1: cfg.fac_bump_max)
    bool fac_enter(int bump_limit = -1);     // switch to the compact factor (false: the basis does not peel; nothing changed)
    void fac_make_room(int need);
    void fac_leave();                        // back to the explicit nucleus inverse (re-inversion from A)
    void ensure_hyper();         // sharded solve with another rank on this GPU (or unknown): same
    // Lazy dual steepest edge: the primal loop never reads beta, so its iterations skip tau = B^-1 rho (solver.rs:1157)
    // and the beta recurrence; beta is rebuilt exactly from the basis inverse (k_exact_beta) when something next needs it
    bool beta_stale = false;
    bool batch_lazy = false;                 // the iterations being recorded skip the beta recurrence
    bool lazy_now(int phase) const { return cfg.lazy_dse && enable_dse && phase == 0 && !stepping && !fac_on_ && max_row_nnz_ <= HEAD_LIST_CAP; }
    void ensure_beta();
    std::vector<int> h_colnnz, h_single_row;
    std::vector<double> h_single_val;
    std::vector<int> h_basic_vars, h_nb_vars, h_var_loc;
    // slot maps live on the device; pulled on demand (reinvert, add_constraint, clone)
    std::vector<int> h_kslot_of_pos, h_srow_of_pos, h_kslot_of_row, h_pos_of_srow, h_pos_of_kslot, h_row_of_kslot;
    std::vector<double> h_sdiag_of_pos;
    std::vector<uint8_t> h_nb_fixed;
    bool enable_pse = false, enable_dse = false, primal_feasible = false, dual_feasible = false;
    size_t nnz_nonbasic = 0;

    // --- device state
    hipStream_t st = nullptr, st2 = nullptr;  // st2: side branch of the iteration graph
    hipEvent_t evFork[3] = {nullptr, nullptr, nullptr}, evJoin[3] = {nullptr, nullptr, nullptr};
    uint64_t batches_run = 0;
    int eager_iters_in_geom = 0;
    DevBuf<int> d_cptr, d_crow, d_rptr, d_rcol;
    DevBuf<double> d_cval, d_rval, d_lo, d_hi, d_obj;
    DevBuf<int> d_var_loc, d_basic_vars, d_nb_vars;
    DevBuf<double> d_xB, d_loB, d_hiB, d_beta, d_d, d_xN, d_gamma;
    DevBuf<uint8_t> d_nbflags;
    DevBuf<int> d_kslot_of_pos, d_srow_of_pos, d_kslot_of_row, d_pos_of_srow, d_pos_of_kslot, d_row_of_kslot;
    DevBuf<RowInfo> d_rowinfo;
    DevBuf<int> d_bptr;             // banded sweep: band-major copy of A
    DevBuf<unsigned short> d_brow;
    DevBuf<double> d_bval;
    DevBuf<double2> d_band_part;
    bool banded_dirty = true;
    // Locality order of the banded sweep: after many pivots nb_vars is a random permutation and the pass over the
    // band-major copy degenerates into 80-byte gathers (PMC: 521 MB per launch at pivot 240 000 against 150 MB at pivot
    // 200).  The pass therefore visits the positions sorted by the variable they hold; the host rebuilds that order from
    // its mirror of var_loc (O(N)) every `order_every` pivots — a stale order only costs locality, never correctness.
    DevBuf<int> d_nb_order;
    // packed non-basic copy of the band-major matrix in the locality order (DevView.pk_*), rebuilt with the order
    DevBuf<int> d_pk_ptr;
    DevBuf<unsigned short> d_pk_row;
    DevBuf<double> d_pk_val;
    DevBuf<unsigned char> d_pk_valid;
    DevBuf<unsigned char> d_fmark;   // det_pull: row marks of the FTRAN pull (zero outside an FTRAN)
    bool use_pack;                  // cfg.use_pack, until a packed copy has not fitted: then the indirect path through the full copy for good
    bool pack_built = false;
    size_t band_total_ = 0;         // entries of the band-major copy (incl. pad entries)
    static constexpr bool use_order = true;  // banded sweep in the locality order (positions sorted by the variable they hold)
    uint64_t order_built_at = 0;    // lifetime pivot count at the last rebuild
    uint64_t lifetime_pivots = 0;   // (stats can be reset by the caller)
    bool order_valid = false;
    bool order_force = false;       // the order from the first pivot instead of after cfg.order_from (loaded bases)
    void refresh_nb_order(bool force);
    bool use_banded() const;        // cfg.banded_mode; auto: m >= 4 bands and >= 2^22 non-zeros (cfg.det_mode auto: <= 2^21 non-zeros)
  public:
    bool banded_active() const { return use_banded(); }
    bool factor_active() const { return fac_on_; }
    void restart_sampling() { batches_run = 0; }
  private:
    void ensure_banded();
    // pulled F product of the large-nucleus primal iteration (fpull.inc): row-major packed copy of the nucleus columns, rebuilt at the
    // start of every solve / continue call and every fpk_every_ pivots (entering columns are appended in between); alpha_K by variable
    DevBuf<int> d_fpk_cnt, d_fpk_var;
    DevBuf<double> d_fpk_val, d_fpk_x, d_fpk_part;
    DevBuf<unsigned char> d_fpk_in;
    bool fpk_valid_ = false;
    uint64_t fpk_built_at_ = 0, fpk_builds_ = 0;
    static constexpr int fpk_every_ = 1024;
    bool fpk_wanted() const;
    void fpk_rebuild();
    DevBuf<int> d_colblk;        // blocked F push (large nucleus): row-block offsets per column
    DevBuf<double> d_push_part;  // ... and its PB_CHUNKS x m partial sums
    bool colblk_dirty = true;
    void ensure_colblk();
    DevBuf<double> d_sdiag_of_pos, d_W, d_U, d_V, d_Ut;
    int pad_for(int cap) const { return (cap >= 8192 || cfg.force_big_tiles) ? cfg.ld_pad : 0; }  // row pitch of a large W = cap + pad: breaks the power-of-two stride
    int ld() const { return cap_ + pad_for(cap_); }
    // delayed-update period: cfg.lr_force, or 32 from capacity 8192 on; 0 on the compact factor (Ctl.nlow counts ITS rank-1 terms)
    int lr_period() const { return fac_on_ ? 0 : (cfg.lr_force >= 0 ? cfg.lr_force : (cap_ >= 8192 ? 32 : 0)); }
    DevBuf<double> d_work;  // alpha_q | tau | rv (2m) | hS  — one memset per batch
    DevBuf<double> d_alpha_r, d_helper;
    DevBuf<int2> d_nb_rng;
    int rt_device = 0;
    void acquire_runtime();  // streams, events, pinned Ctl mirror: recycled across Solutions
    void release_runtime();
    int shard_rank = 0, shard_world = 1;
    // Round 5: DEFERRED sharding.  While the nucleus is small (the sparse-tableau-row regime, a few hundred pivots from the slack basis)
    // a pivot is 40-60 us of latency-bound launches: two or three per-pivot exchanges over xGMI can only slow it down (measured,
    // oversubscribed: 3 665 against 19 095 pivots/s).  Until the tableau row becomes a pass over A the ranks therefore run as
    // bit-identical REPLICAS — the deterministic unsharded iteration on every rank, no exchange — and the column-block sharding goes
    // live at the first batch that leaves that regime (never back).  cfg.shard_defer off: sharded from the first pivot (protocol tests).
    bool shard_live_ = false;
    bool shard_is_live() const { return shard_world > 1 && shard_live_; }
    MailRec* d_mail = nullptr;
    void* mail_host = nullptr;
    bool mail_registered = false;
    void* own_box = nullptr;               // peer transport: this rank's mailbox in its own HBM
    void* peer_box[MAX_WORLD] = {};        // ... and the peers' boxes as mapped through HIP IPC
    int mail_fanout = 1;
    size_t xb_cap_ = 0;                    // doubles per vector slot of the exchange buffer (>= the largest possible nucleus)
    void release_mailboxes();
    // pump transport (MLP_TRANSPORT=rccl | pump): the kernels post into / poll this rank's own device box; while a batch is in flight
    // the host moves the records between the ranks on a second stream: stage -> all-gather -> deliver (kernels.hip: k_mail_stage)
    int pump_backend_ = 0;                 // 0 off, 1 RCCL all-gather, 2 peer copies through HIP IPC + a shared-memory barrier
    hipStream_t st_pump = nullptr;
    void* pump_stage_ = nullptr;           // world x MAIL_PUMP_RECS records
    void* pump_stage_peer_[MAX_WORLD] = {};
    unsigned long long* pump_host_ = nullptr;  // pinned: [0, world) gathered batch words, [world] this rank's word
    unsigned long long pump_seq_ = 0, pump_gen_ = 0;
    uint64_t pump_rounds_ = 0;
    void* rccl_comm_ = nullptr;
    void enable_pump(int rank, int world, void* shm, size_t host_bytes, int backend, const void* rccl_id);
    void pump_until_idle();                // call after enqueueing kernels that contain exchanges, before synchronising the stream
    void pump_round(bool done_local, bool* all_done);
    void shm_barrier();
    bool fac_allowed_under_sharding() const;  // the compact factor shards on distinct devices only (enable_sharding)
    void golive_check();                   // deferred sharding: the ranks compare fingerprints of their replicated state before the switch
    uint64_t golive_seq_ = 0, golive_checks_ = 0;
  public:
    std::string transport = "none";        // human-readable name of the exchange transport
  private:
    size_t mail_bytes = 0;
    DevBuf<double> d_aK, d_rK, d_tK, d_tauK, d_vK, d_klist_a, d_blist_a, d_part_tau, d_part_v;
    DevBuf<int> d_klist_s, d_blist_s;
    DevBuf<double> d_red_key, d_red_key2;
    DevBuf<int> d_rl_cnt, d_rl_pos;    // list form of the primal Harris test: per ratio block its count and its entries (ensure_red)
    DevBuf<double> d_rl_ca, d_rl_q;
    DevBuf<int> d_red_idx;
    DevBuf<unsigned> d_ticket;
    DevBuf<Ctl> d_ctl;
    DevView hview;
    bool view_dirty = true;
    Ctl* h_ctl = nullptr;  // pinned

    // cached x for get_value
    std::vector<double> h_xB, h_xN;
    bool values_dirty = true;

    // --- iteration graphs: [phase][pse]
    // (cfg.batch, round 4: 16 -> 32: one host round trip per 32 replayed iterations; the driver's 20-pivot window is then ONE batch)
    uint64_t iters_since_recalc = 0, iters_since_polish = 0;
    bool basic_values_feasible();
    bool reduced_costs_feasible();
    bool cold_start_ = true;  // the solve started from the slack basis / a loaded basis (try_new, load_basis); add_constraint, fix_var ... clear it:
                              // warm-start re-solves are short and keep the lazy capture policy
    // graph slots: [0] one iteration per graph, [1] cfg.graph_iters iterations per graph (long runs; round 5: 8 -> 10: the driver's 20-pivot window is two graphs)
    hipGraphExec_t gexec[2][2][2] = {};
    hipGraph_t ggraph[2][2][2] = {};
    Geom ggeom[2][2][2];
    uint64_t graph_batches_in_geom = 0;
    hipEvent_t ev[12] = {};  // sweep0/1, W pass0/1, update0/1, ftran0/1, iteration0/1, fold0/1 (kernel-exact: arm_kernel_timing)
    size_t nnz_nucleus_cols();  // non-zeros of the nucleus basic columns (algorithmic bytes of the F products)
    void drop_graphs();
    hipGraphExec_t get_graph(int phase, int multi);

    Geom geom() const;
    DevView* sync_view();
    void build_csc();
    void upload_matrix();
    void alloc_row_buffers(int m_new);
    void ensure_nucleus_cap(int need);
    void ensure_red();
    void flush_lowrank();
    void pull_ctl();
    void pull_maps();
    void push_maps();
    int col_nnz(int var) const { return h_colnnz[var]; }
    DevBuf<int> d_cptr_alt, d_crow_alt, d_col_cnt, d_scan_tmp;  // second CSC buffer set of the device-side append, its per-column counts
    DevBuf<double> d_cval_alt;
    void append_rows_on_device(const std::vector<Constraint>& cs, size_t old_nnz);  // R >= 1 rows, one CSC re-layout

    IterPlan plan_iteration(int phase) const;                       // the ONLY place that combines the launch predicates (kernels.h)
    void record_iteration(const IterPlan& pl, bool with_events);    // enqueue the kernel sequence of ONE iteration
    void launch_stage(const IterPlan& pl, int stage, bool with_events);
  public:
    // engine-level stepping (include/minilp_hip.h: mlp_engine_open / mlp_engine_stage)
    struct StepInfo {
        int32_t status, phase, next_stage;
        int64_t col, row, entering_var, leaving_var;
        double pivot_coeff, step, objective;
        uint64_t nucleus_size;
    };
    int step_phase = 0, step_pos = -1;
    bool stepping = false;
    void recalc_basic_vals();  // x_B recomputed from the basis (polish of long runs)
    // solver.rs:261-270: neither primal nor dual feasible => the feasibility phase runs on an ARTIFICIAL objective (d = +-1 / 0 from
    // try_new); recomputing d from the real costs inside that phase would resume the dual loop on dual-infeasible reduced costs
    bool in_artificial_phase() const { return !primal_feasible && !dual_feasible; }
    void refresh_objective() { recalc_obj_coeffs(); }  // objective + reduced costs of the current point, from the basis (solver.rs:1199-1231)
    int step_open(StepInfo* out);
    int step_stage(int stage, StepInfo* out);
    int step_finish(int phase, int status);
    void fill_step_info(StepInfo* out, int phase) const;

  private:
    int run_loop(int phase);                             // batches of replays until terminal / budget
    // the steps of one batch, in run_loop's order (where the batch is decided)
    void refresh_batch_layout(int phase, bool& fpk_fresh);  // locality order, packed copy of the sweep, packed copy of the nucleus columns
    int run_hyper_batch(int phase);                      // one launch of the hypersparse kernel; the batch's result (ITER_PIVOT: plan the next)
    void shard_go_live_if_due(bool want_sparse_row);
    void enter_row_form(bool want, bool sb);             // form.str / form.sb, the buffers of the sparse row, alpha_r / helper zeroed once per dirty period
    void plan_graphs_now(BatchPlan& plan, int phase, bool long_run);
    void fit_head_room(BatchPlan& plan, int phase);      // form.ph; the batch ends before the nucleus can outgrow the head's slots
    bool fit_factor_room(BatchPlan& plan);               // refactors when due; false: the basis no longer peels, the factor was left (plan again)
    void clear_batch();                                  // reset ring, clear work
    void open_batch(int phase);                          // ... and the pricing launch that opens the first iteration
    void launch_batch(const BatchPlan& plan, int phase);
    struct SampleShapes {                                // what the byte formulas of a sampled iteration read, as it was before the records were processed
        size_t nnz_nonbasic;
        int k;
        size_t nnz_nucleus;
    };
    void account_sample(int phase, const SampleShapes& before);
    void on_ratio_stall();
    int process_records();
    void watch_drift(bool pivoted);  // drift monitor of the inverse, after the records of a batch
    void optimize();              // solver.rs:487-511
    void restore_feasibility();   // solver.rs:513-547
    void warm_resolve();          // restore_feasibility from the current basis with a fresh budget: the tail of every mutator
    void recalc_obj_coeffs();     // solver.rs:1199-1231
    int fix_var_apply(int var, double val);  // fix_var without its re-solve: forced dual pivot (basic) or shift (non-basic), then the fixed flags; returns the column
    void calc_col_coeffs(int col);                          // solver.rs:671-677
    void calc_row_coeffs(int row, bool with_sweep);         // solver.rs:680-693
    void fetch_values();
    void rebuild_inverse();       // BasisSolver::reset counterpart (solver.rs:1286-1303)
    // the dense tableau reads: op 0 rows of B^-1 (req: positions), 1 columns of B^-1 (rows), 2 columns of the tableau (variables), 3 / 4
    // FTRAN / BTRAN of rhs; a request with req < 0 is answered by the caller
    void tab_dense(int op, const std::vector<int>& req, const double* rhs, double* out, TableauInfo& info);
    int tab_internal_col(uint64_t col, const char* what) const;
    // sparse rows out of dense blocks [N][RG_BATCH] for the basic positions pos, RG_BATCH at a time; emit gets each batch as the host read
    // it back.  mode 0: alpha itself (tableau rows); 1: Gomory, f = floor(alpha) - alpha with right-hand sides and, if kept, the primal
    // edge norms; 2: Gomory mixed-integer, as 1 with the coefficients of gmi.inc and a status per request (gmi_mask: the integrality
    // marks by variable on the device)
    struct RowBatch {
        int nreq;           // rows of this batch
        const int* len;     // [RG_BATCH] terms of each row
        const double* rhs;  // [RG_BATCH] right-hand sides (modes 1, 2)
        const int* status;  // [RG_BATCH] mode 2: 0 emitted, 1 / 2 skipped (a skipped row has no terms); else nullptr
        const int* col;     // the rows, request-major, each sorted by variable of [A | I]
        const double* val;
    };
    struct RowBatches {
        size_t nbat = 0, ncnt = 0, nnz = 0;  // batches, counters per batch (RG_BATCH * cut_segments(N)), terms emitted
        double device_ms = 0;                // HIP events around the launches
        double bytes = 0;                    // algorithmic bytes of the generation
    };
    struct ReqContext;  // the padded requests of one batched read, around the BasisRep they are served from (engine.hip)
    std::vector<int> cut_round_positions(const std::vector<int>& vars, const std::string& who, const uint8_t* var_is_int, bool refs) const;
    RowBatches sparse_row_batches(const std::vector<int>& pos, int mode, const std::function<void(size_t, const RowBatch&)>& emit,
                                  const uint8_t* gmi_mask = nullptr, double gmi_away = 0.0);
};

// ---- MPS (mps.rs) on the host side of the product
struct MpsData {
    std::string name;
    std::vector<std::string> var_names;
    ProblemData problem;
};
MpsData parse_mps(const std::string& text, int direction);  // throws MlpError(-1, ..) on syntax errors

}  // namespace mlp
