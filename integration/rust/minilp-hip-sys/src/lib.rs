//! Raw FFI declarations of `include/minilp_hip.h` (one-to-one; see that header for the reference lines each
//! entry replaces).  NOT COMPILED in the build environment of this repository (no Rust toolchain there).
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_double, c_int};

#[repr(C)] pub struct mlp_problem { _p: [u8; 0] }
#[repr(C)] pub struct mlp_solution { _p: [u8; 0] }
#[repr(C)] pub struct mlp_mps { _p: [u8; 0] }

pub const MLP_MINIMIZE: c_int = 0;
pub const MLP_MAXIMIZE: c_int = 1;
pub const MLP_EQ: c_int = 0;
pub const MLP_LE: c_int = 1;
pub const MLP_GE: c_int = 2;
pub const MLP_OK: c_int = 0;
pub const MLP_INFEASIBLE: c_int = 1;
pub const MLP_UNBOUNDED: c_int = 2;

pub const MLP_STAGE_FTRAN: c_int = 0;
pub const MLP_STAGE_RATIO: c_int = 1;
pub const MLP_STAGE_BTRAN: c_int = 2;
pub const MLP_STAGE_BASIS: c_int = 3;
pub const MLP_STAGE_ROW: c_int = 4;
pub const MLP_STAGE_APPLY: c_int = 5;
pub const MLP_ITER_PIVOT: c_int = 0;
pub const MLP_ITER_FLIP: c_int = 1;
pub const MLP_ITER_OPTIMAL: c_int = 2;
pub const MLP_ITER_UNBOUNDED: c_int = 3;
pub const MLP_ITER_FEASIBLE: c_int = 4;
pub const MLP_ITER_INFEASIBLE: c_int = 5;
pub const MLP_ITER_SINGULAR: c_int = 6;

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct mlp_iter_info {
    pub status: i32,
    pub phase: i32,
    pub next_stage: i32,
    pub reserved: i32,
    pub col: i64,
    pub row: i64,
    pub entering_var: i64,
    pub leaving_var: i64,
    pub pivot_coeff: c_double,
    pub step: c_double,
    pub objective: c_double,
    pub nucleus_size: u64,
}

/// Counters of the last tableau call on a solution (only grows at its end; `mlp_tableau_info_size()` is the library's size).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct mlp_tableau_info {
    pub requests: u64,
    pub solves: u64,
    pub batches: u64,
    pub nnz: u64,
    pub bytes: c_double,
    pub device_ms: c_double,
}

extern "C" {
    pub fn mlp_last_error() -> *const c_char;
    pub fn mlp_device_count() -> c_int;
    pub fn mlp_set_device(device: c_int) -> c_int;

    pub fn mlp_problem_new(direction: c_int) -> *mut mlp_problem;
    pub fn mlp_problem_clone(p: *const mlp_problem) -> *mut mlp_problem;
    pub fn mlp_problem_free(p: *mut mlp_problem);
    pub fn mlp_problem_add_var(p: *mut mlp_problem, obj: c_double, min: c_double, max: c_double) -> u32;
    pub fn mlp_problem_add_constraint(p: *mut mlp_problem, vars: *const u32, coeffs: *const c_double, k: u64,
                                      cmp_op: c_int, rhs: c_double) -> c_int;
    pub fn mlp_problem_add_vars(p: *mut mlp_problem, n: u64, obj: *const c_double, mins: *const c_double,
                                maxs: *const c_double) -> c_int;
    pub fn mlp_problem_add_constraints_csr(p: *mut mlp_problem, m: u64, indptr: *const u64, vars: *const u32,
                                           coeffs: *const c_double, cmp_ops: *const i32, rhs: *const c_double) -> c_int;
    pub fn mlp_problem_num_constraints(p: *const mlp_problem) -> u64;
    pub fn mlp_problem_var(p: *const mlp_problem, var: u32, obj_coeff: *mut c_double, min: *mut c_double, max: *mut c_double) -> c_int;
    pub fn mlp_problem_constraint(p: *const mlp_problem, c: u64, vars: *mut u32, coeffs: *mut c_double, cap: u64,
                                  cmp_op: *mut c_int, rhs: *mut c_double) -> u64;
    pub fn mlp_problem_solve(p: *const mlp_problem, out: *mut *mut mlp_solution) -> c_int;
    pub fn mlp_problem_solve_ex(p: *const mlp_problem, out: *mut *mut mlp_solution, pivot_budget: i64, flags: u32) -> c_int;

    pub fn mlp_solution_clone(s: *const mlp_solution) -> *mut mlp_solution;
    pub fn mlp_solution_free(s: *mut mlp_solution);
    pub fn mlp_solution_objective(s: *const mlp_solution) -> c_double;
    pub fn mlp_solution_num_vars(s: *const mlp_solution) -> u32;
    pub fn mlp_solution_var_value(s: *const mlp_solution, var: u32, out: *mut c_double) -> c_int;
    pub fn mlp_solution_values(s: *const mlp_solution, out: *mut c_double, n: u32) -> c_int;
    pub fn mlp_solution_add_constraint(s: *mut *mut mlp_solution, vars: *const u32, coeffs: *const c_double, k: u64,
                                       cmp_op: c_int, rhs: c_double) -> c_int;
    pub fn mlp_solution_fix_var(s: *mut *mut mlp_solution, var: u32, val: c_double) -> c_int;
    pub fn mlp_solution_unfix_var(s: *mut *mut mlp_solution, var: u32, was_fixed: *mut c_int) -> c_int;
    pub fn mlp_solution_add_gomory_cut(s: *mut *mut mlp_solution, var: u32) -> c_int;
    // dual values, reduced costs, KKT certificate (ABI version 5; the certificate struct is read through its size only)
    pub fn mlp_solution_num_constraints(s: *const mlp_solution) -> u64;
    pub fn mlp_solution_dual_values(s: *mut mlp_solution, out: *mut c_double, m: u64) -> c_int;
    pub fn mlp_solution_dual_value(s: *mut mlp_solution, c: u64, out: *mut c_double) -> c_int;
    pub fn mlp_solution_reduced_costs(s: *mut mlp_solution, out: *mut c_double, n: u32) -> c_int;
    pub fn mlp_solution_reduced_cost(s: *mut mlp_solution, var: u32, out: *mut c_double) -> c_int;
    pub fn mlp_solution_certificate(s: *mut mlp_solution, out: *mut std::os::raw::c_void) -> c_int;
    pub fn mlp_certificate_size() -> u64;
    // basis status, cost / rhs ranging (additive: the ABI version stays 5)
    pub fn mlp_solution_basis_status(s: *const mlp_solution, var_status: *mut i32, n_vars: u32, cons_status: *mut i32, n_cons: u64) -> c_int;
    pub fn mlp_solution_cost_ranging(s: *const mlp_solution, vars: *const u32, n: u64, lo: *mut f64, hi: *mut f64) -> c_int;
    pub fn mlp_solution_rhs_ranging(s: *const mlp_solution, cons: *const u64, n: u64, lo: *mut f64, hi: *mut f64) -> c_int;
    pub fn mlp_solution_ranging_info(s: *const mlp_solution, out: *mut std::os::raw::c_void) -> c_int;
    pub fn mlp_ranging_info_size() -> u64;
    // a round of cuts in one call (additive: the ABI version stays 5)
    pub fn mlp_solution_add_constraints_csr(s: *mut *mut mlp_solution, m: u64, indptr: *const u64, vars: *const u32, coeffs: *const f64, cmp_ops: *const i32, rhs: *const f64) -> c_int;
    pub fn mlp_solution_add_gomory_cuts(s: *mut *mut mlp_solution, vars: *const u32, n: u64) -> c_int;
    pub fn mlp_solution_cut_info(s: *const mlp_solution, out: *mut std::os::raw::c_void) -> c_int;
    pub fn mlp_cut_info_size() -> u64;
    pub fn mlp_solution_add_gmi_cuts(s: *mut *mut mlp_solution, vars: *const u32, n: u64, var_is_int: *const u8, num_vars: u32, con_is_int: *const u8, num_constraints: u64, away: f64, status_out: *mut i32) -> c_int;
    pub fn mlp_solution_gmi_info(s: *const mlp_solution, out: *mut std::os::raw::c_void) -> c_int;
    pub fn mlp_gmi_info_size() -> u64;
    pub fn mlp_solution_branch_penalties(s: *const mlp_solution, vars: *const u32, n: u64, var_is_int: *const u8, num_vars: u32, con_is_int: *const u8, num_constraints: u64, down: *mut f64, up: *mut f64, down_col: *mut i64, up_col: *mut i64, frac: *mut f64, status: *mut i32) -> c_int;
    pub fn mlp_solution_branch_info(s: *const mlp_solution, out: *mut std::os::raw::c_void) -> c_int;
    pub fn mlp_branch_info_size() -> u64;
    pub fn mlp_solution_cutoff_bounds(s: *const mlp_solution, cutoff: c_double, var_is_int: *const u8, num_vars: u32, vars: *mut u32, new_lo: *mut f64, new_hi: *mut f64, cap: u64, count: *mut u64, pruned: *mut c_int) -> c_int;
    pub fn mlp_solution_fix_vars(s: *mut *mut mlp_solution, vars: *const u32, vals: *const f64, n: u64) -> c_int;
    pub fn mlp_solution_unfix_vars(s: *mut *mut mlp_solution, vars: *const u32, n: u64, unfixed: *mut u64) -> c_int;
    pub fn mlp_solution_fix_info(s: *const mlp_solution, out: *mut std::os::raw::c_void) -> c_int;
    pub fn mlp_fix_info_size() -> u64;
    pub fn mlp_solution_set_var_bounds(s: *mut *mut mlp_solution, vars: *const u32, lo: *const f64, hi: *const f64, n: u64) -> c_int;
    pub fn mlp_solution_tighten_by_reduced_cost(s: *mut *mut mlp_solution, cutoff: c_double, var_is_int: *const u8, num_vars: u32, tightened: *mut u64, pruned: *mut c_int) -> c_int;
    pub fn mlp_solution_var_bounds(s: *const mlp_solution, vars: *const u32, n: u64, lo: *mut f64, hi: *mut f64) -> c_int;
    pub fn mlp_solution_bounds_info(s: *const mlp_solution, out: *mut std::os::raw::c_void) -> c_int;
    pub fn mlp_bounds_info_size() -> u64;
    pub fn mlp_solution_propagate_bounds(s: *const mlp_solution, var_is_int: *const u8, num_vars: u32, max_rounds: i32, vars: *mut u32, new_lo: *mut f64, new_hi: *mut f64, cap: u64, count: *mut u64, infeasible: *mut c_int) -> c_int;
    pub fn mlp_solution_tighten_by_propagation(s: *mut *mut mlp_solution, var_is_int: *const u8, num_vars: u32, max_rounds: i32, tightened: *mut u64, infeasible: *mut c_int) -> c_int;
    pub fn mlp_solution_propagate_info(s: *const mlp_solution, out: *mut std::os::raw::c_void) -> c_int;
    pub fn mlp_propagate_info_size() -> u64;
    // new right-hand sides and the batched what-if read (additive: the ABI version stays 5)
    pub fn mlp_solution_set_rhs(s: *mut *mut mlp_solution, constraints: *const u64, rhs: *const f64, n: u64) -> c_int;
    pub fn mlp_solution_constraint_rhs(s: *const mlp_solution, constraints: *const u64, n: u64, rhs: *mut f64) -> c_int;
    pub fn mlp_solution_rhs_scenarios(s: *const mlp_solution, constraints: *const u64, n: u64, rhs: *const f64, num_scenarios: u64, bound: *mut f64, feasible: *mut u8, worst: *mut f64, worst_col: *mut i64) -> c_int;
    pub fn mlp_solution_rhs_info(s: *const mlp_solution, out: *mut std::os::raw::c_void) -> c_int;
    pub fn mlp_rhs_info_size() -> u64;
    // reading the tableau: rows / columns of B^-1 A and of B^-1, solves with the basis (additive: the ABI version stays 5)
    pub fn mlp_solution_num_rows(s: *const mlp_solution) -> u64;
    pub fn mlp_solution_basis_head(s: *const mlp_solution, head: *mut u64, num_rows: u64) -> c_int;
    pub fn mlp_solution_binv_rows(s: *const mlp_solution, cols: *const u64, n: u64, out: *mut f64, out_len: u64) -> c_int;
    pub fn mlp_solution_binv_cols(s: *const mlp_solution, constraints: *const u64, n: u64, out: *mut f64, out_len: u64) -> c_int;
    pub fn mlp_solution_tableau_rows(s: *const mlp_solution, cols: *const u64, n: u64, indptr: *mut *const u64, indices: *mut *const u32, values: *mut *const f64) -> c_int;
    pub fn mlp_solution_tableau_cols(s: *const mlp_solution, cols: *const u64, n: u64, out: *mut f64, out_len: u64) -> c_int;
    pub fn mlp_solution_basis_solve(s: *const mlp_solution, transpose: c_int, rhs: *const f64, rhs_len: u64, n: u64, out: *mut f64, out_len: u64) -> c_int;
    pub fn mlp_solution_tableau_info(s: *const mlp_solution, out: *mut mlp_tableau_info) -> c_int;
    pub fn mlp_tableau_info_size() -> u64;
    pub fn mlp_solution_continue(s: *mut mlp_solution, pivot_budget: i64) -> c_int;
    pub fn mlp_solution_budget_exhausted(s: *const mlp_solution) -> c_int;
    pub fn mlp_solution_reinvert(s: *mut mlp_solution, max_diff: *mut c_double) -> c_int;
    pub fn mlp_solution_recompute_basic_values(s: *mut mlp_solution) -> c_int;
    pub fn mlp_solution_save_basis(s: *const mlp_solution, mode: c_int, buf: *mut std::os::raw::c_void, cap: u64) -> u64;
    pub fn mlp_problem_solve_from_basis(p: *const mlp_problem, blob: *const std::os::raw::c_void, len: u64,
                                        out: *mut *mut mlp_solution, pivot_budget: i64, flags: u32) -> c_int;
    pub fn mlp_solution_enable_sharding(s: *mut mlp_solution, rank: c_int, world: c_int, shm_name: *const c_char) -> c_int;
    pub fn mlp_solution_enable_sharding_ex(s: *mut mlp_solution, rank: c_int, world: c_int, shm_name: *const c_char,
                                           transport: *const c_char, rccl_id: *const std::os::raw::c_void) -> c_int;
    pub fn mlp_rccl_unique_id(out128: *mut std::os::raw::c_void) -> c_int;
    pub fn mlp_solution_transport(s: *const mlp_solution) -> *const c_char;
    pub fn mlp_abi_version() -> u32;
    pub fn mlp_stats_size() -> u64;

    pub fn mlp_engine_open(s: *mut mlp_solution, out: *mut mlp_iter_info) -> c_int;
    pub fn mlp_engine_stage(s: *mut mlp_solution, stage: c_int, out: *mut mlp_iter_info) -> c_int;

    pub fn mlp_mps_parse(text: *const c_char, len: u64, direction: c_int, out: *mut *mut mlp_mps) -> c_int;
    pub fn mlp_mps_free(f: *mut mlp_mps);
    pub fn mlp_mps_name(f: *const mlp_mps) -> *const c_char;
    pub fn mlp_mps_num_vars(f: *const mlp_mps) -> u32;
    pub fn mlp_mps_var_name(f: *const mlp_mps, i: u32) -> *const c_char;
    pub fn mlp_mps_var_index(f: *const mlp_mps, name: *const c_char) -> i64;
    pub fn mlp_mps_problem(f: *const mlp_mps) -> *mut mlp_problem;
}
