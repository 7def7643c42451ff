// capi.hip — extern "C" boundary (include/minilp_hip.h).  No C++ exception crosses the ABI.
#include "../../include/minilp_hip.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "engine.h"

using namespace mlp;


struct mlp_problem {
    ProblemData pd;
};
struct mlp_solution {
    Engine* eng = nullptr;
    // dual values / reduced costs / certificate of the current state (mlp_solution_dual_values ...), computed once per state
    bool duals_valid = false;
    Engine::Duals duals;
    Engine::RangingInfo ranging{};  // of the last mlp_solution_cost_ranging / mlp_solution_rhs_ranging call
    Engine::CutInfo cuts{};         // of the last mlp_solution_add_constraints_csr / mlp_solution_add_gomory_cuts call
    Engine::TableauInfo tableau{};  // of the last tableau call
    Engine::GmiInfo gmi{};          // of the last mlp_solution_add_gmi_cuts call
    Engine::BranchInfo branch{};    // of the last mlp_solution_branch_penalties call
    Engine::FixInfo fix{};          // of the last mlp_solution_cutoff_bounds / mlp_solution_fix_vars / mlp_solution_unfix_vars call
    Engine::BoundsInfo bounds{};    // of the last mlp_solution_set_var_bounds / mlp_solution_tighten_by_reduced_cost call
    Engine::PropagateInfo prop{};   // of the last mlp_solution_propagate_bounds / mlp_solution_tighten_by_propagation call
    Engine::RhsInfo rhs{};          // of the last mlp_solution_set_rhs / mlp_solution_rhs_scenarios call
    std::vector<uint64_t> tab_indptr;  // rows of the last mlp_solution_tableau_rows call (library-owned results)
    std::vector<uint32_t> tab_indices;
    std::vector<double> tab_values;
    ~mlp_solution() { delete eng; }
};
struct mlp_mps {
    MpsData d;
};

static thread_local std::string g_err;

template <class F>
static int guarded(F f) {
    try {
        f();
        return MLP_OK;
    } catch (LpFail& e) {
        return e.code;
    } catch (MlpError& e) {
        g_err = e.what();
        return e.code;
    } catch (std::exception& e) {
        g_err = e.what();
        return MLP_EINVAL;
    }
}

// ---- the guards of the entry points ("The boundary"): one per kind
// Every entry point that takes a handle which a failed mutator may have consumed starts here.  `refuse`: which solutions the call is not
// available on, `what`: the subject of that refusal ("the tableau is ").
enum Refuse {
    NOTHING,        // any live handle
    SHARDED,        // a solution sharded over several ranks
    SHARDING_ON,    // any solution sharding was enabled on, a one-rank pump included: its pivots belong to the collective
};
static mlp_solution& live(const mlp_solution* s, Refuse refuse, const char* what) {
    if (!s) throw MlpError(MLP_EINVAL, "NULL solution (consumed by a failed mutator?)");
    if (refuse != NOTHING && (s->eng->sharded() || (refuse == SHARDING_ON && s->eng->transport != "none")))
        throw MlpError(MLP_EINVAL, std::string(what) + "not available on a sharded solution");
    return *const_cast<mlp_solution*>(s);
}
// A mutator (mlp_solution**): f(solution) runs on a live, unsharded handle; any failure frees the solution and clears the handle
// (lib.rs:359, 385).
template <class F>
static int mutate(mlp_solution** s, F f) {
    const int st = guarded([&] { f(live(s ? *s : nullptr, SHARDED, "")); });
    if (st != 0 && s && *s) {
        delete *s;
        *s = nullptr;
    }
    return st;
}
// Whatever can change the state of a solution drops the cached duals; a mutator that is about to re-solve also lifts the pivot budget
// of the initial solve.  Called once the arguments have passed and the call is not a no-op.
static void drop_cached_duals(mlp_solution* s) {
    if (s) s->duals_valid = false;
}
static void begin_change(mlp_solution& s) {
    s.eng->pivot_budget = -1;
    drop_cached_duals(&s);
}
// The engine-level controls (continue, stepping, re-inversion, recomputation): a non-NULL handle, the cached duals dropped.
static Engine* control(mlp_solution* s) {
    if (!s) throw MlpError(MLP_EINVAL, "NULL solution");
    drop_cached_duals(s);
    return s->eng;
}
static const Engine::Duals& duals_of(const mlp_solution* cs) {
    mlp_solution& s = live(cs, SHARDING_ON, "duals are ");
    if (!s.duals_valid) {
        s.eng->compute_duals(s.duals);
        s.duals_valid = true;
    }
    return s.duals;
}
// A report of the last call of its family: a copy of the struct the engine filled (engine.h names the public structs).
template <class T>
static int report(const mlp_solution* s, T mlp_solution::*which, T* out, const char* null_text) {
    return guarded([&] {
        if (!s || !out) throw MlpError(MLP_EINVAL, null_text);
        *out = s->*which;
    });
}
// A list of structural variables as the engine takes it (each index is checked as it is read, nothing is sized by n).
static std::vector<int> var_list(const mlp_solution& s, const uint32_t* vars, uint64_t n, const char* out_of_range) {
    std::vector<int> v;
    for (uint64_t i = 0; i < n; ++i) {
        if (vars[i] >= (uint32_t)s.eng->num_vars) throw MlpError(MLP_EINVAL, out_of_range);
        v.push_back((int)vars[i]);
    }
    return v;
}
// A (vars, lo, hi) list for the caller: the count is always set; a cap below it or a NULL array refuses and writes nothing.
static void copy_bound_list(const std::string& who, const std::vector<uint32_t>& v, const std::vector<double>& lo, const std::vector<double>& hi,
                            uint32_t* vars, double* new_lo, double* new_hi, uint64_t cap, uint64_t* count) {
    *count = (uint64_t)v.size();
    if (cap < *count) throw MlpError(MLP_EINVAL, who + ": cap is below the count (num_vars always suffices)");
    if (*count && (!vars || !new_lo || !new_hi)) throw MlpError(MLP_EINVAL, who + ": NULL output");
    if (*count) {
        std::memcpy(vars, v.data(), sizeof(uint32_t) * v.size());
        std::memcpy(new_lo, lo.data(), sizeof(double) * v.size());
        std::memcpy(new_hi, hi.data(), sizeof(double) * v.size());
    }
}

template <class I>
static int ranging_call(const mlp_solution* cs, int kind, const I* which, uint64_t n, double* lo, double* hi) {
    return guarded([&] {
        const Engine::Duals& d = duals_of(cs);  // (refuses a NULL handle and a sharded solution; the reduced costs come from the cached read)
        mlp_solution* s = const_cast<mlp_solution*>(cs);
        const uint64_t all = kind == 0 ? (uint64_t)s->eng->num_vars : (uint64_t)s->eng->num_constraints();
        if (!which && n != all) throw MlpError(MLP_EINVAL, "ranging: without an index list the length must be the number of variables / constraints");
        if (n && (!lo || !hi)) throw MlpError(MLP_EINVAL, "ranging: NULL output");
        std::vector<uint64_t> idx((size_t)n);
        for (uint64_t i = 0; i < n; ++i) idx[i] = which ? (uint64_t)which[i] : i;
        s->eng->ranging(kind, idx, d, lo, hi, s->ranging);
    });
}

// the tableau reads: refuse a NULL handle and a sharded solution (a one-rank pump included), check the list and the caller's buffer
static mlp_solution* tableau_handle(const mlp_solution* cs) { return &live(cs, SHARDING_ON, "the tableau is "); }
static std::vector<uint64_t> tableau_list(const uint64_t* idx, uint64_t n, const double* out, uint64_t out_len, uint64_t row_len) {
    if (n && !idx) throw MlpError(MLP_EINVAL, "tableau: NULL index list");
    if (out_len != n * row_len || (out_len && !out)) throw MlpError(MLP_EINVAL, "tableau: the output length must be n times the row length");
    return std::vector<uint64_t>(idx, idx + n);
}

extern "C" {

const char* mlp_last_error(void) { return g_err.c_str(); }
int mlp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int mlp_set_device(int device) {
    return guarded([&] { HIPCHECK(hipSetDevice(device)); });
}

mlp_problem* mlp_problem_new(int direction) {
    mlp_problem* p = new mlp_problem();
    p->pd.direction = direction == MLP_MAXIMIZE ? 1 : 0;
    return p;
}
mlp_problem* mlp_problem_clone(const mlp_problem* p) { return new mlp_problem(*p); }
void mlp_problem_free(mlp_problem* p) { delete p; }
uint32_t mlp_problem_add_var(mlp_problem* p, double c, double mn, double mx) { return (uint32_t)p->pd.add_var(c, mn, mx); }
uint32_t mlp_problem_num_vars(const mlp_problem* p) { return (uint32_t)p->pd.obj.size(); }
int mlp_problem_add_constraint(mlp_problem* p, const uint32_t* vars, const double* coeffs, uint64_t k, int op, double rhs) {
    return guarded([&] { p->pd.add_constraint(vars, coeffs, k, op, rhs); });
}
int mlp_problem_add_vars(mlp_problem* p, uint64_t n, const double* obj, const double* mins, const double* maxs) {
    return guarded([&] {
        for (uint64_t i = 0; i < n; ++i) p->pd.add_var(obj[i], mins[i], maxs[i]);
    });
}
int mlp_problem_add_constraints_csr(mlp_problem* p, uint64_t m, const uint64_t* indptr, const uint32_t* vars,
                                    const double* coeffs, const int32_t* ops, const double* rhs) {
    return guarded([&] {
        for (uint64_t i = 0; i < m; ++i)
            p->pd.add_constraint(vars + indptr[i], coeffs + indptr[i], indptr[i + 1] - indptr[i], ops[i], rhs[i]);
    });
}
uint64_t mlp_problem_num_constraints(const mlp_problem* p) { return p->pd.cons.size(); }
int mlp_problem_var(const mlp_problem* p, uint32_t var, double* obj, double* mn, double* mx) {
    return guarded([&] {
        if (var >= p->pd.obj.size()) throw MlpError(MLP_EINVAL, "variable out of range");
        *obj = p->pd.direction == 1 ? -p->pd.obj[var] : p->pd.obj[var];
        *mn = p->pd.lo[var];
        *mx = p->pd.hi[var];
    });
}
uint64_t mlp_problem_constraint(const mlp_problem* p, uint64_t ci, uint32_t* vars, double* coeffs, uint64_t cap, int* op, double* rhs) {
    if (ci >= p->pd.cons.size()) return 0;
    const Constraint& c = p->pd.cons[ci];
    if (op) *op = c.op;
    if (rhs) *rhs = c.rhs;
    for (size_t i = 0; i < c.idx.size() && i < cap; ++i) {
        vars[i] = (uint32_t)c.idx[i];
        coeffs[i] = c.val[i];
    }
    return c.idx.size();
}
int mlp_problem_solve_ex(const mlp_problem* p, mlp_solution** out, int64_t budget, uint32_t flags) {
    *out = nullptr;
    mlp_solution* s = new mlp_solution();
    int st = guarded([&] {
        s->eng = new Engine(Settings::from_env());
        s->eng->pivot_budget = budget;
        s->eng->trace = flags & 1u;
        s->eng->profile = flags & 2u;
        s->eng->sample_every = (flags & 4u) ? 1 : 0;
        s->eng->try_new(p->pd);      // lib.rs:292-297
        s->eng->initial_solve();     // lib.rs:298
    });
    if (st != 0) delete s;
    else *out = s;
    return st;
}
int mlp_problem_solve(const mlp_problem* p, mlp_solution** out) { return mlp_problem_solve_ex(p, out, -1, 0); }
int mlp_problem_solve_from_basis(const mlp_problem* p, const void* blob, uint64_t len, mlp_solution** out, int64_t budget,
                                 uint32_t flags) {
    *out = nullptr;
    mlp_solution* s = new mlp_solution();
    int st = guarded([&] {
        s->eng = new Engine(Settings::from_env());
        s->eng->pivot_budget = budget;
        s->eng->trace = flags & 1u;
        s->eng->profile = flags & 2u;
        s->eng->sample_every = (flags & 4u) ? 1 : 0;
        s->eng->try_new(p->pd);
        s->eng->load_basis(static_cast<const uint8_t*>(blob), (size_t)len);
        s->eng->initial_solve();
    });
    if (st != 0) delete s;
    else *out = s;
    return st;
}
uint64_t mlp_solution_save_basis(const mlp_solution* s, int mode, void* buf, uint64_t cap) {
    uint64_t need = 0;
    int st = guarded([&] {
        if (!s) throw MlpError(MLP_EINVAL, "NULL solution");
        std::vector<uint8_t> b = s->eng->save_basis(mode);
        need = b.size();
        if (buf && cap >= need) std::memcpy(buf, b.data(), b.size());
    });
    return st == 0 ? need : 0;
}
int mlp_solution_set_sampling(mlp_solution* s, int every_iteration) {
    return guarded([&] {
        if (!s) throw MlpError(MLP_EINVAL, "NULL solution");
        if (every_iteration < 0) {  // switch the HIP-event sampling off altogether (long runs after a measurement pass)
            s->eng->profile = false;
            s->eng->sample_every = 0;
        } else {
            s->eng->profile = true;  // (also switches the sampling back on after a `< 0` call)
            s->eng->sample_every = every_iteration ? 1 : 0;
        }
    });
}
int mlp_solution_continue(mlp_solution* s, int64_t budget) {
    return guarded([&] {
        Engine* e = control(s);
        e->pivot_budget = budget;
        e->budget_exhausted = false;
        e->initial_solve();
    });
}
static void copy_info(const Engine::StepInfo& si, mlp_iter_info* out) {
    if (!out) return;
    out->status = si.status; out->phase = si.phase; out->next_stage = si.next_stage; out->reserved = 0;
    out->col = si.col; out->row = si.row; out->entering_var = si.entering_var; out->leaving_var = si.leaving_var;
    out->pivot_coeff = si.pivot_coeff; out->step = si.step; out->objective = si.objective;
    out->nucleus_size = si.nucleus_size;
}
int mlp_engine_open(mlp_solution* s, mlp_iter_info* out) {
    int status = MLP_EINVAL;
    int rc = guarded([&] {
        Engine::StepInfo si{};
        status = control(s)->step_open(&si);
        copy_info(si, out);
    });
    return rc != 0 ? (rc > 0 ? MLP_EINVAL : rc) : status;
}
int mlp_engine_stage(mlp_solution* s, int stage, mlp_iter_info* out) {
    int status = MLP_EINVAL;
    int rc = guarded([&] {
        Engine::StepInfo si{};
        status = control(s)->step_stage(stage, &si);
        copy_info(si, out);
    });
    return rc != 0 ? (rc > 0 ? MLP_EINVAL : rc) : status;
}
int mlp_solution_budget_exhausted(const mlp_solution* s) { return (s && s->eng->budget_exhausted) ? 1 : 0; }
int mlp_solution_reinvert(mlp_solution* s, double* max_diff) {
    return guarded([&] {
        double d = control(s)->reinvert(true);
        if (max_diff) *max_diff = d;
    });
}

int mlp_solution_recompute_basic_values(mlp_solution* s) {
    return guarded([&] {
        // x_B, then the objective of the recomputed point (and the reduced costs with it: solver.rs:1199-1231), so that
        // mlp_solution_objective and the values agree afterwards
        // — except inside the artificial-objective feasibility phase of a budget-paused solve (d = +-1 / 0 there: initial_solve
        // itself never recomputes d on a budget resume); the basic values are recomputed, d and the objective are left alone
        Engine* e = control(s);
        e->recalc_basic_vals();
        if (!e->in_artificial_phase()) e->refresh_objective();
    });
}
uint32_t mlp_abi_version(void) { return MLP_ABI_VERSION; }
uint64_t mlp_certificate_size(void) { return (uint64_t)sizeof(mlp_certificate); }

uint64_t mlp_solution_num_constraints(const mlp_solution* s) { return s ? (uint64_t)s->eng->num_constraints() : 0; }
int mlp_solution_dual_values(mlp_solution* s, double* out, uint64_t m) {
    return guarded([&] {
        const Engine::Duals& d = duals_of(s);
        if (!out || m != d.pi.size()) throw MlpError(MLP_EINVAL, "dual_values: length must be mlp_solution_num_constraints");
        std::memcpy(out, d.pi.data(), sizeof(double) * d.pi.size());
    });
}
int mlp_solution_dual_value(mlp_solution* s, uint64_t c, double* out) {
    return guarded([&] {
        const Engine::Duals& d = duals_of(s);
        if (!out || c >= d.pi.size()) throw MlpError(MLP_EINVAL, "constraint out of range");
        *out = d.pi[c];
    });
}
int mlp_solution_reduced_costs(mlp_solution* s, double* out, uint32_t n) {
    return guarded([&] {
        const Engine::Duals& d = duals_of(s);
        if (!out || n != d.r.size()) throw MlpError(MLP_EINVAL, "reduced_costs: length must be mlp_solution_num_vars");
        std::memcpy(out, d.r.data(), sizeof(double) * d.r.size());
    });
}
int mlp_solution_reduced_cost(mlp_solution* s, uint32_t var, double* out) {
    return guarded([&] {
        const Engine::Duals& d = duals_of(s);
        if (!out || var >= d.r.size()) throw MlpError(MLP_EINVAL, "variable out of range");
        *out = d.r[var];
    });
}
int mlp_solution_certificate(mlp_solution* s, mlp_certificate* out) {
    return guarded([&] {
        const Engine::Duals& d = duals_of(s);
        if (!out) throw MlpError(MLP_EINVAL, "NULL certificate");
        std::memset(out, 0, sizeof(*out));
        out->primal_objective = d.primal_obj; out->dual_objective = d.dual_obj; out->relative_gap = d.rel_gap;
        out->max_row_violation = d.max_row_viol; out->max_row_violation_at = d.row_viol_at;
        out->max_bound_violation = d.max_bound_viol; out->max_bound_violation_at = d.bound_viol_at;
        out->max_dual_infeasibility = d.max_dual_inf; out->max_dual_infeasibility_at = d.dual_inf_at;
        out->btran_residual = d.btran_residual; out->btran_residual_at = d.btran_residual_at;
        out->bytes = d.bytes; out->device_ms = d.device_ms;
    });
}
// ---- basis status, cost / rhs ranging (ranging.inc)
int mlp_solution_basis_status(const mlp_solution* cs, int32_t* var_status, uint32_t n_vars, int32_t* cons_status, uint64_t n_cons) {
    return guarded([&] {
        mlp_solution* s = &live(cs, SHARDING_ON, "the basis status is ");
        if ((int)n_vars != s->eng->num_vars || n_cons != s->eng->num_constraints() || (n_vars && !var_status) || (n_cons && !cons_status))
            throw MlpError(MLP_EINVAL, "basis_status: lengths must be mlp_solution_num_vars and mlp_solution_num_constraints");
        std::vector<int32_t> v, c;
        s->eng->basis_status(v, c);
        if (n_vars) std::memcpy(var_status, v.data(), sizeof(int32_t) * v.size());
        if (n_cons) std::memcpy(cons_status, c.data(), sizeof(int32_t) * c.size());
    });
}
int mlp_solution_cost_ranging(const mlp_solution* s, const uint32_t* vars, uint64_t n, double* lo, double* hi) {
    return ranging_call(s, 0, vars, n, lo, hi);
}
int mlp_solution_rhs_ranging(const mlp_solution* s, const uint64_t* cons, uint64_t n, double* lo, double* hi) {
    return ranging_call(s, 1, cons, n, lo, hi);
}
int mlp_solution_ranging_info(const mlp_solution* s, mlp_ranging_info* out) { return report(s, &mlp_solution::ranging, out, "NULL solution / ranging info"); }
uint64_t mlp_ranging_info_size(void) { return (uint64_t)sizeof(mlp_ranging_info); }
uint64_t mlp_stats_size(void) { return (uint64_t)sizeof(mlp_stats); }

int mlp_solution_enable_sharding(mlp_solution* s, int rank, int world, const char* shm_name) {
    return guarded([&] {
        if (!s || !shm_name) throw MlpError(MLP_EINVAL, "NULL solution / rendezvous name");
        drop_cached_duals(s);
        s->eng->enable_sharding(rank, world, shm_name);
    });
}

int mlp_solution_enable_sharding_ex(mlp_solution* s, int rank, int world, const char* shm_name, const char* transport, const void* rccl_id) {
    return guarded([&] {
        if (!s || !shm_name) throw MlpError(MLP_EINVAL, "NULL solution / rendezvous name");
        drop_cached_duals(s);
        s->eng->enable_sharding(rank, world, shm_name, transport, rccl_id);
    });
}
int mlp_rccl_unique_id(void* out128) {
    return guarded([&] {
        if (!out128) throw MlpError(MLP_EINVAL, "NULL buffer");
        Engine::rccl_unique_id(out128);
    });
}
const char* mlp_solution_transport(const mlp_solution* s) { return s ? s->eng->transport.c_str() : "none"; }

mlp_solution* mlp_solution_clone(const mlp_solution* s) {
    mlp_solution* c = new mlp_solution();
    int st = guarded([&] { c->eng = s->eng->clone(); });
    if (st != 0) {
        delete c;
        return nullptr;
    }
    return c;
}
void mlp_solution_free(mlp_solution* s) { delete s; }
double mlp_solution_objective(const mlp_solution* s) {  // lib.rs:334-339
    if (!s) return std::nan("");
    double v = 0.0;
    if (guarded([&] { v = s->eng->cur_obj_val(); }) != MLP_OK) return std::nan("");  // HIP failure: never a plausible 0
    return s->eng->direction == 1 ? -v : v;
}
uint32_t mlp_solution_num_vars(const mlp_solution* s) { return s ? (uint32_t)s->eng->num_vars : 0; }
int mlp_solution_var_value(const mlp_solution* s, uint32_t var, double* out) {
    return guarded([&] {
        live(s, NOTHING, "");
        if ((int)var >= s->eng->num_vars) throw MlpError(MLP_EINVAL, "variable out of range (lib.rs:345)");
        *out = s->eng->get_value((int)var);
    });
}
int mlp_solution_values(const mlp_solution* s, double* out, uint32_t n) {
    return guarded([&] {
        live(s, NOTHING, "");
        if ((int)n > s->eng->num_vars) throw MlpError(MLP_EINVAL, "too many values requested");
        s->eng->get_values(out, (int)n);
    });
}
int mlp_solution_add_constraint(mlp_solution** h, const uint32_t* vars, const double* coeffs, uint64_t k, int op, double rhs) {
    return mutate(h, [&](mlp_solution& s) {
        ProblemData tmp;
        tmp.obj.resize(s.eng->num_vars);  // lib.rs:376: dimension = num_vars
        tmp.add_constraint(vars, coeffs, k, op, rhs);
        begin_change(s);
        s.eng->add_constraint(tmp.cons[0]);
    });
}
int mlp_solution_fix_var(mlp_solution** h, uint32_t var, double val) {
    return mutate(h, [&](mlp_solution& s) {
        if ((int)var >= s.eng->num_vars) throw MlpError(MLP_EINVAL, "variable out of range (lib.rs:391)");
        begin_change(s);
        s.eng->fix_var((int)var, val);
    });
}
int mlp_solution_unfix_var(mlp_solution** h, uint32_t var, int* was_fixed) {
    return mutate(h, [&](mlp_solution& s) {
        if ((int)var >= s.eng->num_vars) throw MlpError(MLP_EINVAL, "variable out of range (lib.rs:400)");
        begin_change(s);
        *was_fixed = s.eng->unfix_var((int)var) ? 1 : 0;
    });
}
int mlp_solution_add_gomory_cut(mlp_solution** h, uint32_t var) {
    return mutate(h, [&](mlp_solution& s) {
        if ((int)var >= s.eng->num_vars) throw MlpError(MLP_EINVAL, "variable out of range (lib.rs:420)");
        begin_change(s);
        s.eng->add_gomory_cut((int)var);
    });
}

// ---- a round of cuts in one call (cuts.inc)
int mlp_solution_add_constraints_csr(mlp_solution** h, uint64_t m, const uint64_t* indptr, const uint32_t* vars, const double* coeffs,
                                     const int32_t* cmp_ops, const double* rhs) {
    return mutate(h, [&](mlp_solution& s) {
        if (m && (!indptr || !cmp_ops || !rhs)) throw MlpError(MLP_EINVAL, "add_constraints_csr: NULL array");
        ProblemData tmp;
        tmp.obj.resize(s.eng->num_vars);  // lib.rs:376: dimension = num_vars
        for (uint64_t i = 0; i < m; ++i) {
            if (indptr[i + 1] < indptr[i]) throw MlpError(MLP_EINVAL, "add_constraints_csr: indptr must not decrease");
            if (indptr[i + 1] > indptr[i] && (!vars || !coeffs)) throw MlpError(MLP_EINVAL, "add_constraints_csr: NULL array");
            tmp.add_constraint(vars + indptr[i], coeffs + indptr[i], indptr[i + 1] - indptr[i], cmp_ops[i], rhs[i]);
        }
        s.cuts = Engine::CutInfo();
        if (m == 0) return;
        begin_change(s);
        s.eng->add_constraints(std::move(tmp.cons), s.cuts);
    });
}
int mlp_solution_add_gomory_cuts(mlp_solution** h, const uint32_t* vars, uint64_t n) {
    return mutate(h, [&](mlp_solution& s) {
        if (n && !vars) throw MlpError(MLP_EINVAL, "add_gomory_cuts: NULL variable list");
        const std::vector<int> v = var_list(s, vars, n, "variable out of range (lib.rs:420)");
        s.cuts = Engine::CutInfo();
        if (n == 0) return;
        begin_change(s);
        s.eng->add_gomory_cuts(v, s.cuts);
    });
}
int mlp_solution_cut_info(const mlp_solution* s, mlp_cut_info* out) { return report(s, &mlp_solution::cuts, out, "NULL solution / cut info"); }
uint64_t mlp_cut_info_size(void) { return (uint64_t)sizeof(mlp_cut_info); }

// ---- reading the tableau (tableau.inc)
uint64_t mlp_solution_num_rows(const mlp_solution* s) { return s ? (uint64_t)s->eng->num_rows() : 0; }
int mlp_solution_basis_head(const mlp_solution* cs, uint64_t* head, uint64_t num_rows) {
    return guarded([&] {
        mlp_solution* s = tableau_handle(cs);
        if (num_rows != (uint64_t)s->eng->num_rows() || (num_rows && !head)) throw MlpError(MLP_EINVAL, "basis_head: length must be mlp_solution_num_rows");
        std::vector<uint64_t> h;
        s->eng->basis_head(h);
        if (num_rows) std::memcpy(head, h.data(), sizeof(uint64_t) * h.size());
    });
}
int mlp_solution_binv_rows(const mlp_solution* cs, const uint64_t* cols, uint64_t n, double* out, uint64_t out_len) {
    return guarded([&] {
        mlp_solution* s = tableau_handle(cs);
        const std::vector<uint64_t> idx = tableau_list(cols, n, out, out_len, s->eng->num_constraints());
        s->eng->binv_rows(idx, out, s->tableau);
    });
}
int mlp_solution_binv_cols(const mlp_solution* cs, const uint64_t* constraints, uint64_t n, double* out, uint64_t out_len) {
    return guarded([&] {
        mlp_solution* s = tableau_handle(cs);
        const std::vector<uint64_t> idx = tableau_list(constraints, n, out, out_len, (uint64_t)s->eng->num_rows());
        s->eng->binv_cols(idx, out, s->tableau);
    });
}
int mlp_solution_tableau_cols(const mlp_solution* cs, const uint64_t* cols, uint64_t n, double* out, uint64_t out_len) {
    return guarded([&] {
        mlp_solution* s = tableau_handle(cs);
        const std::vector<uint64_t> idx = tableau_list(cols, n, out, out_len, (uint64_t)s->eng->num_rows());
        s->eng->tableau_cols(idx, out, s->tableau);
    });
}
int mlp_solution_tableau_rows(const mlp_solution* cs, const uint64_t* cols, uint64_t n, const uint64_t** indptr, const uint32_t** indices,
                              const double** values) {
    return guarded([&] {
        mlp_solution* s = tableau_handle(cs);
        if ((n && !cols) || !indptr || !indices || !values) throw MlpError(MLP_EINVAL, "tableau_rows: NULL argument");
        // (each index is checked as it is read, nothing is sized by n: a garbage n ends at the first index out of range, not far past
        // the caller's array)
        const uint64_t ncol = (uint64_t)s->eng->num_vars + s->eng->num_constraints();
        std::vector<uint64_t> req;
        for (uint64_t t = 0; t < n; ++t) {
            if (cols[t] >= ncol) throw MlpError(MLP_EINVAL, "tableau_rows: column out of range");
            req.push_back(cols[t]);
        }
        std::vector<uint64_t> ip;
        std::vector<uint32_t> ix;
        std::vector<double> vv;
        s->eng->tableau_rows(req, ip, ix, vv, s->tableau);  // (a refusal leaves the previous rows in place)
        ix.reserve(ix.size() + 1);  // (never a NULL data pointer, also for rows without terms)
        vv.reserve(vv.size() + 1);
        s->tab_indptr.swap(ip); s->tab_indices.swap(ix); s->tab_values.swap(vv);
        *indptr = s->tab_indptr.data(); *indices = s->tab_indices.data(); *values = s->tab_values.data();
    });
}
int mlp_solution_basis_solve(const mlp_solution* cs, int transpose, const double* rhs, uint64_t rhs_len, uint64_t n, double* out,
                             uint64_t out_len) {
    return guarded([&] {
        mlp_solution* s = tableau_handle(cs);
        const uint64_t by_cons = s->eng->num_constraints(), by_pos = (uint64_t)s->eng->num_rows();
        const uint64_t in_row = transpose ? by_pos : by_cons, out_row = transpose ? by_cons : by_pos;
        if (rhs_len != n * in_row || out_len != n * out_row || (rhs_len && !rhs) || (out_len && !out))
            throw MlpError(MLP_EINVAL, "basis_solve: the lengths must be n times num_constraints / num_rows");
        s->eng->basis_solve(transpose != 0, rhs, (size_t)n, out, s->tableau);
    });
}
int mlp_solution_tableau_info(const mlp_solution* s, mlp_tableau_info* out) { return report(s, &mlp_solution::tableau, out, "NULL solution / tableau info"); }
uint64_t mlp_tableau_info_size(void) { return (uint64_t)sizeof(mlp_tableau_info); }

// ---- a round of Gomory mixed-integer cuts (gmi.inc)
int mlp_solution_add_gmi_cuts(mlp_solution** h, const uint32_t* vars, uint64_t n, const uint8_t* var_is_int, uint32_t num_vars,
                              const uint8_t* con_is_int, uint64_t num_constraints, double away, int32_t* status_out) {
    return mutate(h, [&](mlp_solution& s) {
        Engine* e = s.eng;
        if (n && !vars) throw MlpError(MLP_EINVAL, "add_gmi_cuts: NULL variable list");
        if (num_vars != (uint32_t)e->num_vars || (num_vars && !var_is_int)) throw MlpError(MLP_EINVAL, "add_gmi_cuts: var_is_int must have num_vars entries");
        if (con_is_int && num_constraints != (uint64_t)e->num_constraints())
            throw MlpError(MLP_EINVAL, "add_gmi_cuts: con_is_int must have num_constraints entries");
        const std::vector<int> v = var_list(s, vars, n, "add_gmi_cuts: variable out of range");
        s.cuts = Engine::CutInfo();
        s.gmi = Engine::GmiInfo();
        if (n == 0) return;
        begin_change(s);
        e->add_gmi_cuts(v, var_is_int, con_is_int, away, status_out, s.cuts, s.gmi);
    });
}
int mlp_solution_gmi_info(const mlp_solution* s, mlp_gmi_info* out) { return report(s, &mlp_solution::gmi, out, "NULL solution / gmi info"); }
uint64_t mlp_gmi_info_size(void) { return (uint64_t)sizeof(mlp_gmi_info); }

// ---- branching penalties (branch.inc)
int mlp_solution_branch_penalties(const mlp_solution* cs, const uint32_t* vars, uint64_t n, const uint8_t* var_is_int, uint32_t num_vars,
                                  const uint8_t* con_is_int, uint64_t num_constraints, double* down, double* up, int64_t* down_col,
                                  int64_t* up_col, double* frac, int32_t* status) {
    return guarded([&] {
        const Engine::Duals& d = duals_of(cs);  // (refuses a NULL handle and a sharded solution; the reduced costs come from the cached read)
        mlp_solution& s = *const_cast<mlp_solution*>(cs);
        Engine* e = s.eng;
        if (n && !vars) throw MlpError(MLP_EINVAL, "branch_penalties: NULL variable list");
        if (n && (!down || !up || !down_col || !up_col || !frac || !status)) throw MlpError(MLP_EINVAL, "branch_penalties: NULL output");
        if (var_is_int ? num_vars != (uint32_t)e->num_vars : con_is_int != nullptr)
            throw MlpError(MLP_EINVAL, "branch_penalties: var_is_int must have num_vars entries (and con_is_int needs it)");
        if (con_is_int && num_constraints != e->num_constraints())
            throw MlpError(MLP_EINVAL, "branch_penalties: con_is_int must have num_constraints entries");
        const std::vector<int> v = var_list(s, vars, n, "branch_penalties: variable out of range");
        e->branch_penalties(v, var_is_int, con_is_int, d, down, up, down_col, up_col, frac, status, s.branch);
    });
}
int mlp_solution_branch_info(const mlp_solution* s, mlp_branch_info* out) { return report(s, &mlp_solution::branch, out, "NULL solution / branch info"); }
uint64_t mlp_branch_info_size(void) { return (uint64_t)sizeof(mlp_branch_info); }

// ---- reduced-cost bounds from a cutoff, batched fixing (fixing.inc)
int mlp_solution_cutoff_bounds(const mlp_solution* cs, double cutoff, const uint8_t* var_is_int, uint32_t num_vars, uint32_t* vars,
                               double* new_lo, double* new_hi, uint64_t cap, uint64_t* count, int* pruned) {
    return guarded([&] {
        mlp_solution& s = live(cs, SHARDING_ON, "cutoff_bounds is ");
        Engine* e = s.eng;
        if (!count || !pruned) throw MlpError(MLP_EINVAL, "cutoff_bounds: NULL count / pruned");
        *count = 0;
        *pruned = 0;
        if (std::isnan(cutoff)) throw MlpError(MLP_EINVAL, "cutoff_bounds: the cutoff is NaN");
        if (num_vars != (uint32_t)e->num_vars) throw MlpError(MLP_EINVAL, "cutoff_bounds: num_vars must be mlp_solution_num_vars");
        const double g = e->cutoff_gap(cutoff, "cutoff_bounds");
        Engine::FixInfo info{};
        if (g < 0.0) {  // the node is worse than the cutoff
            *pruned = 1;
            s.fix = info;
            return;
        }
        std::vector<uint32_t> v;
        std::vector<double> lo, hi;
        e->cutoff_bounds(g, var_is_int, v, lo, hi, info);
        copy_bound_list("cutoff_bounds", v, lo, hi, vars, new_lo, new_hi, cap, count);
        s.fix = info;
    });
}
int mlp_solution_fix_vars(mlp_solution** h, const uint32_t* vars, const double* vals, uint64_t n) {
    return mutate(h, [&](mlp_solution& s) {
        if (n && (!vars || !vals)) throw MlpError(MLP_EINVAL, "fix_vars: NULL list");
        const std::vector<int> v = var_list(s, vars, n, "fix_vars: variable out of range");
        s.fix = Engine::FixInfo();
        if (n == 0) return;
        begin_change(s);
        s.eng->fix_vars(v, std::vector<double>(vals, vals + n), s.fix);
    });
}
int mlp_solution_unfix_vars(mlp_solution** h, const uint32_t* vars, uint64_t n, uint64_t* unfixed) {
    return mutate(h, [&](mlp_solution& s) {
        if (unfixed) *unfixed = 0;
        if (n && !vars) throw MlpError(MLP_EINVAL, "unfix_vars: NULL list");
        const std::vector<int> v = var_list(s, vars, n, "unfix_vars: variable out of range");
        s.fix = Engine::FixInfo();
        if (n == 0) return;
        begin_change(s);
        const uint64_t k = s.eng->unfix_vars(v, s.fix);
        if (unfixed) *unfixed = k;
    });
}
int mlp_solution_fix_info(const mlp_solution* s, mlp_fix_info* out) { return report(s, &mlp_solution::fix, out, "NULL solution / fix info"); }
uint64_t mlp_fix_info_size(void) { return (uint64_t)sizeof(mlp_fix_info); }

// ---- new bounds for structural variables (bounds.inc)
int mlp_solution_set_var_bounds(mlp_solution** h, const uint32_t* vars, const double* lo, const double* hi, uint64_t n) {
    return mutate(h, [&](mlp_solution& s) {
        if (n && (!vars || !lo || !hi)) throw MlpError(MLP_EINVAL, "set_var_bounds: NULL list");
        const std::vector<int> v = var_list(s, vars, n, "set_var_bounds: variable out of range");
        s.bounds = Engine::BoundsInfo();
        if (n == 0) return;
        begin_change(s);
        s.eng->set_var_bounds(v, std::vector<double>(lo, lo + n), std::vector<double>(hi, hi + n), s.bounds);
    });
}
int mlp_solution_tighten_by_reduced_cost(mlp_solution** h, double cutoff, const uint8_t* var_is_int, uint32_t num_vars, uint64_t* tightened,
                                         int* pruned) {
    return mutate(h, [&](mlp_solution& s) {
        live(&s, SHARDING_ON, "tighten_by_reduced_cost is ");
        Engine* e = s.eng;
        if (!tightened || !pruned) throw MlpError(MLP_EINVAL, "tighten_by_reduced_cost: NULL tightened / pruned");
        *tightened = 0;
        *pruned = 0;
        if (std::isnan(cutoff)) throw MlpError(MLP_EINVAL, "tighten_by_reduced_cost: the cutoff is NaN");
        if (num_vars != (uint32_t)e->num_vars) throw MlpError(MLP_EINVAL, "tighten_by_reduced_cost: num_vars must be mlp_solution_num_vars");
        const double g = e->cutoff_gap(cutoff, "tighten_by_reduced_cost");
        s.bounds = Engine::BoundsInfo();
        if (g < 0.0) {  // the node is worse than the cutoff: nothing changes
            *pruned = 1;
            return;
        }
        begin_change(s);
        *tightened = e->tighten_by_reduced_cost(g, var_is_int, s.bounds);
    });
}
int mlp_solution_var_bounds(const mlp_solution* s, const uint32_t* vars, uint64_t n, double* lo, double* hi) {
    return guarded([&] {
        live(s, NOTHING, "");
        if (!vars && n != (uint64_t)s->eng->num_vars) throw MlpError(MLP_EINVAL, "var_bounds: without a list the length must be the number of variables");
        if (n && (!lo || !hi)) throw MlpError(MLP_EINVAL, "var_bounds: NULL output");
        s->eng->var_bounds(vars, n, lo, hi);
    });
}
int mlp_solution_bounds_info(const mlp_solution* s, mlp_bounds_info* out) { return report(s, &mlp_solution::bounds, out, "NULL solution / bounds info"); }
uint64_t mlp_bounds_info_size(void) { return (uint64_t)sizeof(mlp_bounds_info); }

// ---- bound propagation from row activities (propagate.inc)
int mlp_solution_propagate_bounds(const mlp_solution* cs, const uint8_t* var_is_int, uint32_t num_vars, int32_t max_rounds, uint32_t* vars,
                                  double* new_lo, double* new_hi, uint64_t cap, uint64_t* count, int* infeasible) {
    return guarded([&] {
        mlp_solution& s = live(cs, SHARDING_ON, "propagate_bounds is ");
        if (!count || !infeasible) throw MlpError(MLP_EINVAL, "propagate_bounds: NULL count / infeasible");
        *count = 0;
        *infeasible = 0;
        if (num_vars != (uint32_t)s.eng->num_vars) throw MlpError(MLP_EINVAL, "propagate_bounds: num_vars must be mlp_solution_num_vars");
        Engine::PropagateInfo info{};
        std::vector<uint32_t> v;
        std::vector<double> lo, hi;
        bool inf = false;
        s.eng->propagate_bounds(var_is_int, (int)max_rounds, v, lo, hi, inf, info);
        *infeasible = inf ? 1 : 0;
        copy_bound_list("propagate_bounds", v, lo, hi, vars, new_lo, new_hi, cap, count);
        s.prop = info;
    });
}
int mlp_solution_tighten_by_propagation(mlp_solution** h, const uint8_t* var_is_int, uint32_t num_vars, int32_t max_rounds,
                                        uint64_t* tightened, int* infeasible) {
    return mutate(h, [&](mlp_solution& s) {
        live(&s, SHARDING_ON, "tighten_by_propagation is ");
        if (!tightened || !infeasible) throw MlpError(MLP_EINVAL, "tighten_by_propagation: NULL tightened / infeasible");
        *tightened = 0;
        *infeasible = 0;
        if (num_vars != (uint32_t)s.eng->num_vars) throw MlpError(MLP_EINVAL, "tighten_by_propagation: num_vars must be mlp_solution_num_vars");
        s.bounds = Engine::BoundsInfo();
        s.prop = Engine::PropagateInfo();
        begin_change(s);
        bool inf = false;
        *tightened = s.eng->tighten_by_propagation(var_is_int, (int)max_rounds, inf, s.prop, s.bounds);
        *infeasible = inf ? 1 : 0;
    });
}
int mlp_solution_propagate_info(const mlp_solution* s, mlp_propagate_info* out) { return report(s, &mlp_solution::prop, out, "NULL solution / propagate info"); }
uint64_t mlp_propagate_info_size(void) { return (uint64_t)sizeof(mlp_propagate_info); }

// ---- new right-hand sides and the batched what-if read (rhs.inc)
int mlp_solution_set_rhs(mlp_solution** h, const uint64_t* constraints, const double* rhs, uint64_t n) {
    return mutate(h, [&](mlp_solution& s) {
        if (n && (!constraints || !rhs)) throw MlpError(MLP_EINVAL, "set_rhs: NULL list");
        s.rhs = Engine::RhsInfo();
        if (n == 0) return;  // (the no-op of every mutator: the engine's checks, solved() among them, run only on a list)
        begin_change(s);
        // a constraint index is not narrowed: its range, like a constraint listed twice, is Engine::check_rhs_list's alone
        s.eng->set_rhs(std::vector<uint64_t>(constraints, constraints + n), std::vector<double>(rhs, rhs + n), s.rhs);
    });
}
int mlp_solution_constraint_rhs(const mlp_solution* s, const uint64_t* constraints, uint64_t n, double* rhs) {
    return guarded([&] {
        live(s, NOTHING, "");
        if (!constraints && n != (uint64_t)s->eng->num_constraints())
            throw MlpError(MLP_EINVAL, "constraint_rhs: without a list the length must be the number of constraints");
        if (n && !rhs) throw MlpError(MLP_EINVAL, "constraint_rhs: NULL output");
        s->eng->constraint_rhs(constraints, n, rhs);
    });
}
int mlp_solution_rhs_scenarios(const mlp_solution* cs, const uint64_t* constraints, uint64_t n, const double* rhs, uint64_t num_scenarios,
                               double* bound, uint8_t* feasible, double* worst, int64_t* worst_col) {
    return guarded([&] {
        mlp_solution& s = live(cs, SHARDING_ON, "rhs_scenarios is ");  // (a read through the tableau's solve: refused like the tableau reads)
        if (n && !constraints) throw MlpError(MLP_EINVAL, "rhs_scenarios: NULL constraint list");
        if (n && num_scenarios && !rhs) throw MlpError(MLP_EINVAL, "rhs_scenarios: NULL right-hand sides");
        if (num_scenarios && (!bound || !feasible || !worst || !worst_col)) throw MlpError(MLP_EINVAL, "rhs_scenarios: NULL output");
        s.eng->rhs_scenarios(std::vector<uint64_t>(constraints, constraints + n), rhs, (size_t)num_scenarios, bound, feasible, worst, worst_col,
                             s.rhs);
    });
}
int mlp_solution_rhs_info(const mlp_solution* s, mlp_rhs_info* out) { return report(s, &mlp_solution::rhs, out, "NULL solution / rhs info"); }
uint64_t mlp_rhs_info_size(void) { return (uint64_t)sizeof(mlp_rhs_info); }

void mlp_solution_stats(const mlp_solution* s, mlp_stats* o) {
    if (!o) return;
    if (!s) {
        std::memset(o, 0, sizeof(*o));
        return;
    }
    Engine* e = s->eng;
    const Stats& t = e->stats;
    std::memset(o, 0, sizeof(*o));
    o->iterations = t.iterations; o->basis_changes = t.basis_changes; o->bound_flips = t.bound_flips;
    o->primal_iters = t.primal_iters; o->dual_iters = t.dual_iters; o->reinversions = t.reinversions;
    o->num_constraints = e->m(); o->num_total_vars = e->total_vars();
    o->nucleus_size = e->nucleus(); o->nucleus_capacity = e->nucleus_cap(); o->nnz = e->nnz();
    o->fused_bytes = t.fused_bytes; o->fused_ms = t.fused_ms; o->sweep_bytes = t.sweep_bytes; o->sweep_ms = t.sweep_ms;
    o->fused_launches = t.fused_launches; o->sweep_launches = t.sweep_launches;
    o->update_ms = t.update_ms; o->update_launches = t.update_launches; o->final_refreshes = t.final_refreshes;
    o->banded_sweep = e->banded_active() ? 1 : 0;
    o->solve_wall_s = t.solve_wall_s;
    o->max_pivot_err = t.max_pivot_err;
    o->ftran_bytes = t.ftran_bytes; o->ftran_ms = t.ftran_ms; o->ftran_launches = t.ftran_launches;
    o->iter_ms = t.iter_ms; o->iter_samples = t.iter_samples;
    o->beta_rebuilds = t.beta_rebuilds;
    o->str_ms = t.str_ms; o->str_launches = t.str_launches;
    o->ratio_stalls = t.ratio_stalls; o->hyper_iters = t.hyper_iters; o->hyper_bails = t.hyper_bails;
    o->dense_ftran_bytes = t.dense_ftran_bytes; o->dense_ftran_ms = t.dense_ftran_ms; o->dense_ftran_launches = t.dense_ftran_launches;
    o->fold_bytes = t.fold_bytes; o->fold_ms = t.fold_ms; o->fold_launches = t.fold_launches;
    for (int i = 0; i < 5; ++i) o->kase[i] = t.kase[i];
    o->reinversion_fallbacks = t.reinversion_fallbacks;
    o->factor_active = e->factor_active() ? 1 : 0; o->factor_refactors = t.fac_refactors; o->factor_levels = t.fac_levels;
    o->factor_switches = t.fac_switches; o->factor_bump = t.fac_bump; o->factor_bump_max = t.fac_bump_max;
}
void mlp_solution_reset_stats(mlp_solution* s) {
    s->eng->stats = Stats();
    s->eng->restart_sampling();  // profile mode: the next batch is a sampled one, so a short timed region still has samples
}
uint64_t mlp_solution_trace_len(const mlp_solution* s) { return s->eng->trace_log.size(); }
void mlp_solution_trace_get(const mlp_solution* s, uint64_t i, int32_t* phase, int64_t* col, int64_t* row,
                            int64_t* entering_var, int64_t* leaving_var, double* pivot_coeff, double* obj_after) {
    const PivotRecord& r = s->eng->trace_log[i];
    *phase = r.phase; *col = r.col; *row = r.row; *entering_var = r.entering_var; *leaving_var = r.leaving_var;
    *pivot_coeff = r.pivot_coeff; *obj_after = r.obj_after;
}
uint64_t mlp_solution_state(const mlp_solution* s, const char* what, double* out, uint64_t cap) {
    uint64_t n = (uint64_t)-1;
    guarded([&] { n = s->eng->state(what, out, cap); });
    return n;
}

int mlp_mps_parse(const char* text, uint64_t len, int direction, mlp_mps** out) {
    *out = nullptr;
    mlp_mps* f = new mlp_mps();
    int st = guarded([&] { f->d = parse_mps(std::string(text, len), direction == MLP_MAXIMIZE ? 1 : 0); });
    if (st != 0) delete f;
    else *out = f;
    return st;
}
void mlp_mps_free(mlp_mps* f) { delete f; }
const char* mlp_mps_name(const mlp_mps* f) { return f->d.name.c_str(); }
uint32_t mlp_mps_num_vars(const mlp_mps* f) { return (uint32_t)f->d.var_names.size(); }
const char* mlp_mps_var_name(const mlp_mps* f, uint32_t i) { return f->d.var_names[i].c_str(); }
int64_t mlp_mps_var_index(const mlp_mps* f, const char* name) {
    for (size_t i = 0; i < f->d.var_names.size(); ++i)
        if (f->d.var_names[i] == name) return (int64_t)i;
    return -1;
}
mlp_problem* mlp_mps_problem(const mlp_mps* f) {
    mlp_problem* p = new mlp_problem();
    p->pd = f->d.problem;
    return p;
}

}  // extern "C"
