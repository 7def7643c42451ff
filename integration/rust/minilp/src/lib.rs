//! `minilp`'s public API (ztlpn/minilp 0.2.2, `src/lib.rs:61-464`) over `libminilp_hip.so`.
//!
//! Every public item of the reference crate is here with the same name, signature and error behaviour; the
//! solver behind `Problem::solve` and the `Solution` mutators is the device-resident simplex engine.  A `Problem`
//! is plain host data exactly as in the reference (`lib.rs:193-200`) and is handed to the library at `solve()`;
//! a `Solution` owns an opaque `mlp_solution` (the state of `solver.rs:14-58` in HBM).
//!
//! Differences by construction: a process without a visible GPU gets a panic from `solve()` (there is no CPU
//! fallback); `Solution: Clone` deep-copies device state.
//!
//! NOT COMPILED in this repository (no `cargo` in the build image).  The same C ABI is exercised by the Python
//! `ctypes` mirror (`minilp_amd/api.py`) that the GPU parity tests go through, call for call.
#![deny(missing_docs)]

use minilp_hip_sys as sys;
use std::cell::RefCell;
use std::ffi::CStr;
use std::ptr;

mod mps;
pub use mps::MpsFile;

/// An enum indicating whether to minimize or maximize objective function.  (`lib.rs:62-69`)
#[derive(Clone, Copy, Debug)]
pub enum OptimizationDirection {
    /// Minimize the objective function.
    Minimize,
    /// Maximize the objective function.
    Maximize,
}

/// A reference to a variable in a linear programming problem.  (`lib.rs:71-83`)
#[derive(Clone, Copy, Debug, PartialEq, Eq, PartialOrd, Ord, Hash)]
pub struct Variable(pub(crate) usize);

impl Variable {
    /// Sequence number of the variable.
    pub fn idx(&self) -> usize {
        self.0
    }
}

/// A sum of variables multiplied by constant coefficients.  (`lib.rs:85-114`)
#[derive(Clone, Debug)]
pub struct LinearExpr {
    vars: Vec<usize>,
    coeffs: Vec<f64>,
}

impl LinearExpr {
    /// Creates an empty linear expression.
    pub fn empty() -> Self {
        Self { vars: vec![], coeffs: vec![] }
    }

    /// Add a single term to the linear expression.  Variables can be added only once (checked at
    /// `add_constraint`, like the reference's `CsVec::new` panic).
    pub fn add(&mut self, var: Variable, coeff: f64) {
        self.vars.push(var.0);
        self.coeffs.push(coeff);
    }
}

/// A single `variable * constant` term in a linear expression.  (`lib.rs:116-129`)
#[derive(Clone, Copy, Debug)]
pub struct LinearTerm(Variable, f64);

impl From<(Variable, f64)> for LinearTerm {
    fn from(term: (Variable, f64)) -> Self {
        LinearTerm(term.0, term.1)
    }
}

impl<'a> From<&'a (Variable, f64)> for LinearTerm {
    fn from(term: &'a (Variable, f64)) -> Self {
        LinearTerm(term.0, term.1)
    }
}

impl<I: IntoIterator<Item = impl Into<LinearTerm>>> From<I> for LinearExpr {
    fn from(iter: I) -> Self {
        let mut expr = LinearExpr::empty();
        for term in iter {
            let LinearTerm(var, coeff) = term.into();
            expr.add(var, coeff);
        }
        expr
    }
}

impl std::iter::FromIterator<(Variable, f64)> for LinearExpr {
    fn from_iter<I: IntoIterator<Item = (Variable, f64)>>(iter: I) -> Self {
        let mut expr = LinearExpr::empty();
        for (var, coeff) in iter {
            expr.add(var, coeff);
        }
        expr
    }
}

impl std::iter::Extend<(Variable, f64)> for LinearExpr {
    fn extend<I: IntoIterator<Item = (Variable, f64)>>(&mut self, iter: I) {
        for (var, coeff) in iter {
            self.add(var, coeff);
        }
    }
}

/// An operator specifying the relation between left-hand and right-hand sides of the constraint.  (`lib.rs:161-169`)
#[derive(Clone, Copy, Debug)]
pub enum ComparisonOp {
    /// The == operator (equal to)
    Eq,
    /// The <= operator (less than or equal to)
    Le,
    /// The >= operator (greater than or equal to)
    Ge,
}

impl ComparisonOp {
    fn to_c(self) -> std::os::raw::c_int {
        match self {
            ComparisonOp::Eq => sys::MLP_EQ,
            ComparisonOp::Le => sys::MLP_LE,
            ComparisonOp::Ge => sys::MLP_GE,
        }
    }
}

/// An error encountered while solving a problem.  (`lib.rs:172-190`)
#[derive(Clone, Debug, PartialEq)]
pub enum Error {
    /// Constrains can't simultaneously be satisfied.
    Infeasible,
    /// The objective function is unbounded.
    Unbounded,
}

impl std::fmt::Display for Error {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        let msg = match self {
            Error::Infeasible => "problem is infeasible",
            Error::Unbounded => "problem is unbounded",
        };
        msg.fmt(f)
    }
}

impl std::error::Error for Error {}

fn last_error() -> String {
    unsafe { CStr::from_ptr(sys::mlp_last_error()) }.to_string_lossy().into_owned()
}

/// Status of a C-ABI call -> the reference's behaviour: 0 Ok, 1 / 2 the two `Error`s, negative values are the
/// reference's panics (duplicate variable in an expression, out-of-range `Variable`, Gomory cut on a non-basic
/// variable, singular basis) or a HIP-level failure.
fn check(status: std::os::raw::c_int) -> Result<(), Error> {
    match status {
        sys::MLP_OK => Ok(()),
        sys::MLP_INFEASIBLE => Err(Error::Infeasible),
        sys::MLP_UNBOUNDED => Err(Error::Unbounded),
        code => panic!("minilp (HIP engine) error {}: {}", code, last_error()),
    }
}

/// A specification of a linear programming problem.  (`lib.rs:193-311`)
#[derive(Clone)]
pub struct Problem {
    direction: OptimizationDirection,
    obj_coeffs: Vec<f64>,
    var_mins: Vec<f64>,
    var_maxs: Vec<f64>,
    // rows in CSR form, ready for one bulk FFI crossing at solve()
    row_ptr: Vec<u64>,
    row_vars: Vec<u32>,
    row_coeffs: Vec<f64>,
    row_ops: Vec<i32>,
    row_rhs: Vec<f64>,
}

impl std::fmt::Debug for Problem {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        // (only printing lengths here, like the reference)
        f.debug_struct("Problem")
            .field("direction", &self.direction)
            .field("num_vars", &self.obj_coeffs.len())
            .field("num_constraints", &self.row_rhs.len())
            .finish()
    }
}

impl Problem {
    /// Create a new problem instance.
    pub fn new(direction: OptimizationDirection) -> Self {
        Problem {
            direction,
            obj_coeffs: vec![],
            var_mins: vec![],
            var_maxs: vec![],
            row_ptr: vec![0],
            row_vars: vec![],
            row_coeffs: vec![],
            row_ops: vec![],
            row_rhs: vec![],
        }
    }

    /// Add a new variable to the problem.  `obj_coeff` is its coefficient in the objective, `min` and `max`
    /// may be infinite.  (`lib.rs:233-242`; the library negates the objective for `Maximize` like `lib.rs:235-238`.)
    pub fn add_var(&mut self, obj_coeff: f64, (min, max): (f64, f64)) -> Variable {
        let var = Variable(self.obj_coeffs.len());
        self.obj_coeffs.push(obj_coeff);
        self.var_mins.push(min);
        self.var_maxs.push(max);
        var
    }

    /// Add a linear constraint to the problem.
    ///
    /// # Panics
    ///
    /// Will panic if a variable was added more than once to the left-hand side expression
    /// (`lib.rs:276-289`: `CsVec::new` on unsorted / duplicate indices).
    pub fn add_constraint(&mut self, expr: impl Into<LinearExpr>, cmp_op: ComparisonOp, rhs: f64) {
        let expr = expr.into();
        let mut seen = std::collections::HashSet::with_capacity(expr.vars.len());
        for &v in &expr.vars {
            assert!(v < self.obj_coeffs.len(), "variable {} is not part of this problem", v);
            assert!(seen.insert(v), "variable {} was added more than once to the expression", v);
        }
        self.row_vars.extend(expr.vars.iter().map(|&v| v as u32));
        self.row_coeffs.extend_from_slice(&expr.coeffs);
        self.row_ptr.push(self.row_vars.len() as u64);
        self.row_ops.push(cmp_op.to_c());
        self.row_rhs.push(rhs);
    }

    /// The C-side model: one `mlp_problem` filled with two bulk calls (freed by the caller).
    pub(crate) fn to_c(&self) -> *mut sys::mlp_problem {
        let dir = match self.direction {
            OptimizationDirection::Minimize => sys::MLP_MINIMIZE,
            OptimizationDirection::Maximize => sys::MLP_MAXIMIZE,
        };
        unsafe {
            let p = sys::mlp_problem_new(dir);
            assert!(!p.is_null(), "mlp_problem_new failed: {}", last_error());
            let st = sys::mlp_problem_add_vars(
                p,
                self.obj_coeffs.len() as u64,
                self.obj_coeffs.as_ptr(),
                self.var_mins.as_ptr(),
                self.var_maxs.as_ptr(),
            );
            assert_eq!(st, sys::MLP_OK, "{}", last_error());
            let st = sys::mlp_problem_add_constraints_csr(
                p,
                self.row_rhs.len() as u64,
                self.row_ptr.as_ptr(),
                self.row_vars.as_ptr(),
                self.row_coeffs.as_ptr(),
                self.row_ops.as_ptr(),
                self.row_rhs.as_ptr(),
            );
            assert_eq!(st, sys::MLP_OK, "{}", last_error());
            p
        }
    }

    /// Solve the problem, finding the optimal objective function value and variable values.
    ///
    /// # Errors
    ///
    /// Will return an error, if the problem is infeasible (constraints can't be satisfied)
    /// or if the objective value is unbounded.  (`lib.rs:291-310`)
    pub fn solve(&self) -> Result<Solution, Error> {
        let p = self.to_c();
        let mut s: *mut sys::mlp_solution = ptr::null_mut();
        let st = unsafe { sys::mlp_problem_solve(p, &mut s) };
        unsafe { sys::mlp_problem_free(p) };
        check(st)?;
        Ok(Solution::from_raw(s, self.obj_coeffs.len()))
    }
}

/// A solution of a problem: optimal objective function value and variable values.
///
/// Note that a `Solution` instance contains the whole solver machinery which can require
/// a lot of memory for larger problems (here: device memory).  (`lib.rs:313-424`)
pub struct Solution {
    raw: *mut sys::mlp_solution,
    num_vars: usize,
    // `var_value` and `Index` hand out `&f64` (lib.rs:344, 426): the values are copied from the device once per
    // solved state and cached; every mutator consumes `self`, so the cache can never be stale
    values: RefCell<Option<Box<[f64]>>>,
}

// The handle is used by one thread at a time (each owns its HIP stream and device buffers).
unsafe impl Send for Solution {}

impl Clone for Solution {
    /// `#[derive(Clone)]` of the reference (`lib.rs:313`): an independent deep copy of the solver state.
    fn clone(&self) -> Self {
        let raw = unsafe { sys::mlp_solution_clone(self.raw) };
        assert!(!raw.is_null(), "mlp_solution_clone failed: {}", last_error());
        Solution::from_raw(raw, self.num_vars)
    }
}

impl Drop for Solution {
    fn drop(&mut self) {
        if !self.raw.is_null() {
            unsafe { sys::mlp_solution_free(self.raw) };
            self.raw = ptr::null_mut();
        }
    }
}

impl std::fmt::Debug for Solution {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        // (only printing lengths here, like the reference)
        f.debug_struct("Solution").field("num_vars", &self.num_vars).finish()
    }
}

impl Solution {
    fn from_raw(raw: *mut sys::mlp_solution, num_vars: usize) -> Self {
        Solution { raw, num_vars, values: RefCell::new(None) }
    }

    fn values(&self) -> &[f64] {
        if self.values.borrow().is_none() {
            let mut buf = vec![0.0f64; self.num_vars].into_boxed_slice();
            let st = unsafe { sys::mlp_solution_values(self.raw, buf.as_mut_ptr(), self.num_vars as u32) };
            assert_eq!(st, sys::MLP_OK, "{}", last_error());
            *self.values.borrow_mut() = Some(buf);
        }
        // SAFETY: once filled the box is never replaced or dropped while `self` lives (mutators take `self` by value)
        let b = self.values.borrow();
        let s: &[f64] = b.as_ref().unwrap();
        unsafe { std::slice::from_raw_parts(s.as_ptr(), s.len()) }
    }

    /// Optimal value of the objective function.
    pub fn objective(&self) -> f64 {
        unsafe { sys::mlp_solution_objective(self.raw) }
    }

    /// Value of the variable at optimum.  Note that you can use indexing operations to get variable values.
    pub fn var_value(&self, var: Variable) -> &f64 {
        assert!(var.0 < self.num_vars);
        &self.values()[var.0]
    }

    /// Number of constraints: those of the `Problem` in the order they were added, then the ones `add_constraint` and
    /// `add_gomory_cut` appended, in call order (extension: no counterpart in the reference).
    pub fn num_constraints(&self) -> usize {
        unsafe { sys::mlp_solution_num_constraints(self.raw) as usize }
    }

    /// Dual value (shadow price) of constraint `c` at the current basis: d objective / d rhs_c, in the problem's direction
    /// (extension: no counterpart in the reference).
    pub fn dual_value(&self, c: usize) -> f64 {
        assert!(c < self.num_constraints());
        let mut out = 0.0f64;
        let st = unsafe { sys::mlp_solution_dual_value(self.raw, c as u64, &mut out) };
        assert_eq!(st, sys::MLP_OK, "{}", last_error());
        out
    }

    /// Reduced cost c_j - a_j . pi of a variable (0 for a basic one), in the problem's direction (extension: no counterpart in
    /// the reference).
    pub fn reduced_cost(&self, var: Variable) -> f64 {
        assert!(var.0 < self.num_vars);
        let mut out = 0.0f64;
        let st = unsafe { sys::mlp_solution_reduced_cost(self.raw, var.0 as u32, &mut out) };
        assert_eq!(st, sys::MLP_OK, "{}", last_error());
        out
    }

    /// Range `(lo, hi)` of the objective coefficient of a variable over which the current basis stays optimal, in the problem's
    /// direction; within it the objective moves by `var_value * delta` (extension: no counterpart in the reference).
    pub fn cost_range(&self, var: Variable) -> (f64, f64) {
        assert!(var.0 < self.num_vars);
        let (v, mut lo, mut hi) = (var.0 as u32, 0.0f64, 0.0f64);
        let st = unsafe { sys::mlp_solution_cost_ranging(self.raw, &v, 1, &mut lo, &mut hi) };
        assert_eq!(st, sys::MLP_OK, "{}", last_error());
        (lo, hi)
    }

    /// Branching penalties of the listed variables at the current basis: per variable `(down, up, down_col, up_col, frac)`, the
    /// one-pivot (Driebeek-Tomlin) lower bounds on the objective degradation of the branches `x <= floor(x)` and `x >= ceil(x)`
    /// (`f64::INFINITY`: the branch is infeasible), the columns that would enter (`None`: no column; `num_vars + c` is the slack
    /// of constraint `c`) and the fraction of the variable.  A non-basic or integral variable returns zeros and no columns.
    /// `integer_vars` / `integer_constraints` switch Tomlin's strengthening on: the numbers then bound the integer descendants of
    /// the branch, not the child LP (extension: no counterpart in the reference; semantics in `minilp_hip.h`).
    ///
    /// # Panics
    ///
    /// Will panic if a mask has the wrong length or `integer_constraints` is given without `integer_vars`.
    pub fn branch_penalties(&self, vars: &[Variable], integer_vars: Option<&[bool]>, integer_constraints: Option<&[bool]>) -> Vec<(f64, f64, Option<usize>, Option<usize>, f64)> {
        assert!(vars.iter().all(|x| x.0 < self.num_vars));
        let v: Vec<u32> = vars.iter().map(|x| x.0 as u32).collect();
        let vm: Option<Vec<u8>> = integer_vars.map(|m| m.iter().map(|&b| b as u8).collect());
        let cm: Option<Vec<u8>> = integer_constraints.map(|m| m.iter().map(|&b| b as u8).collect());
        let (vp, vn) = vm.as_ref().map_or((std::ptr::null(), 0u32), |m| (m.as_ptr(), m.len() as u32));
        let (cp, cn) = cm.as_ref().map_or((std::ptr::null(), 0u64), |m| (m.as_ptr(), m.len() as u64));
        let n = v.len();
        let (mut down, mut up, mut frac) = (vec![0.0f64; n], vec![0.0f64; n], vec![0.0f64; n]);
        let (mut dcol, mut ucol, mut status) = (vec![0i64; n], vec![0i64; n], vec![0i32; n]);
        let st = unsafe {
            sys::mlp_solution_branch_penalties(self.raw, v.as_ptr(), n as u64, vp, vn, cp, cn, down.as_mut_ptr(), up.as_mut_ptr(),
                                               dcol.as_mut_ptr(), ucol.as_mut_ptr(), frac.as_mut_ptr(), status.as_mut_ptr())
        };
        assert_eq!(st, sys::MLP_OK, "{}", last_error());
        let col = |c: i64| if c < 0 { None } else { Some(c as usize) };
        (0..n).map(|t| (down[t], up[t], col(dcol[t]), col(ucol[t]), frac[t])).collect()
    }

    /// Bounds that the reduced costs imply once an incumbent of objective value `cutoff` is known: `None` if this LP is already
    /// worse than the cutoff (prune the node), else every variable whose bound tightens as `(variable, lo, hi)` in ascending order;
    /// `lo == hi` means the variable can be fixed ([`fix_vars`](Self::fix_vars)).  `integer_vars` rounds the bound of a marked
    /// variable to whole steps (extension: no counterpart in the reference; semantics in `minilp_hip.h`).
    ///
    /// # Panics
    ///
    /// Will panic if the mask has the wrong length, the cutoff is NaN or the solution is not solved.
    pub fn cutoff_bounds(&self, cutoff: f64, integer_vars: Option<&[bool]>) -> Option<Vec<(Variable, f64, f64)>> {
        let vm: Option<Vec<u8>> = integer_vars.map(|m| m.iter().map(|&b| b as u8).collect());
        let (vp, vn) = vm.as_ref().map_or((std::ptr::null(), self.num_vars as u32), |m| (m.as_ptr(), m.len() as u32));
        let n = self.num_vars;
        let (mut v, mut lo, mut hi) = (vec![0u32; n], vec![0.0f64; n], vec![0.0f64; n]);
        let (mut count, mut pruned): (u64, std::os::raw::c_int) = (0, 0);
        let st = unsafe {
            sys::mlp_solution_cutoff_bounds(self.raw, cutoff, vp, vn, v.as_mut_ptr(), lo.as_mut_ptr(), hi.as_mut_ptr(), n as u64, &mut count,
                                            &mut pruned)
        };
        assert_eq!(st, sys::MLP_OK, "{}", last_error());
        if pruned != 0 {
            return None;
        }
        Some((0..count as usize).map(|t| (Variable(v[t] as usize), lo[t], hi[t])).collect())
    }

    /// Bounds that the rows of the model imply on its variables, given the bounds and fixings it holds now (bound propagation, node
    /// presolve): `None` if the rounds prove the model infeasible (prune the node), else every variable whose bounds tighten as
    /// `(variable, lo, hi)` in ascending order; `lo == hi` means the variable can be fixed.  `integer_vars` rounds the bounds of a
    /// marked variable inwards; at most `max_rounds` (1..=64) Jacobi rounds are run.  Works on any state of a solution (extension:
    /// no counterpart in the reference; semantics in `minilp_hip.h`).
    ///
    /// # Panics
    ///
    /// Will panic if the mask has the wrong length or `max_rounds` is out of range.
    pub fn propagate_bounds(&self, integer_vars: Option<&[bool]>, max_rounds: usize) -> Option<Vec<(Variable, f64, f64)>> {
        let vm: Option<Vec<u8>> = integer_vars.map(|m| m.iter().map(|&b| b as u8).collect());
        let (vp, vn) = vm.as_ref().map_or((std::ptr::null(), self.num_vars as u32), |m| (m.as_ptr(), m.len() as u32));
        let n = self.num_vars;
        let (mut v, mut lo, mut hi) = (vec![0u32; n], vec![0.0f64; n], vec![0.0f64; n]);
        let (mut count, mut infeasible): (u64, std::os::raw::c_int) = (0, 0);
        let st = unsafe {
            sys::mlp_solution_propagate_bounds(self.raw, vp, vn, max_rounds.min(65) as i32, v.as_mut_ptr(), lo.as_mut_ptr(), hi.as_mut_ptr(),
                                               n as u64, &mut count, &mut infeasible)
        };
        assert_eq!(st, sys::MLP_OK, "{}", last_error());
        if infeasible != 0 {
            return None;
        }
        Some((0..count as usize).map(|t| (Variable(v[t] as usize), lo[t], hi[t])).collect())
    }

    /// Range `(lo, hi)` of the right-hand side of a constraint (by index, in the order the constraints were added) over which the
    /// current basis stays feasible; within it the objective moves by `dual_value * delta` (extension).
    pub fn rhs_range(&self, constraint: usize) -> (f64, f64) {
        assert!(constraint < self.num_constraints());
        let (c, mut lo, mut hi) = (constraint as u64, 0.0f64, 0.0f64);
        let st = unsafe { sys::mlp_solution_rhs_ranging(self.raw, &c, 1, &mut lo, &mut hi) };
        assert_eq!(st, sys::MLP_OK, "{}", last_error());
        (lo, hi)
    }

    /// Whether a variable is basic at the current basis (extension).
    pub fn is_basic(&self, var: Variable) -> bool {
        assert!(var.0 < self.num_vars);
        let mut vs = vec![0i32; self.num_vars];
        let mut cs = vec![0i32; self.num_constraints()];
        let st = unsafe { sys::mlp_solution_basis_status(self.raw, vs.as_mut_ptr(), vs.len() as u32, cs.as_mut_ptr(), cs.len() as u64) };
        assert_eq!(st, sys::MLP_OK, "{}", last_error());
        vs[var.0] == 0
    }

    // ---- reading the tableau (extension: no counterpart in the reference; numbering and definitions in include/minilp_hip.h).
    // Columns: j < num_vars is variable j, num_vars + c the slack of constraint c.  Vectors by row are exchanged by constraint
    // (length num_constraints), vectors by position have length num_rows.  Internal form A x + s = b: no sign turn for Maximize.

    /// Number of constraints that have a row (= basis positions).
    pub fn num_rows(&self) -> usize {
        unsafe { sys::mlp_solution_num_rows(self.raw) as usize }
    }

    /// The column basic at each position.
    pub fn basis_head(&self) -> Vec<usize> {
        let mut h = vec![0u64; self.num_rows()];
        let st = unsafe { sys::mlp_solution_basis_head(self.raw, h.as_mut_ptr(), h.len() as u64) };
        assert_eq!(st, sys::MLP_OK, "{}", last_error());
        h.into_iter().map(|c| c as usize).collect()
    }

    /// Row e_p^T B^-1 (by constraint) of the position p at which the given column is basic.
    pub fn binv_row(&self, basic_col: usize) -> Vec<f64> {
        let (c, mut out) = (basic_col as u64, vec![0.0f64; self.num_constraints()]);
        let st = unsafe { sys::mlp_solution_binv_rows(self.raw, &c, 1, out.as_mut_ptr(), out.len() as u64) };
        assert_eq!(st, sys::MLP_OK, "{}", last_error());
        out
    }

    /// Column B^-1 e_row (by position) of the row of the given constraint.
    pub fn binv_col(&self, constraint: usize) -> Vec<f64> {
        let (c, mut out) = (constraint as u64, vec![0.0f64; self.num_rows()]);
        let st = unsafe { sys::mlp_solution_binv_cols(self.raw, &c, 1, out.as_mut_ptr(), out.len() as u64) };
        assert_eq!(st, sys::MLP_OK, "{}", last_error());
        out
    }

    /// Tableau row e_p^T B^-1 [A | I] of a basic column as `(column, coefficient)` pairs sorted by column: exact zeros and the
    /// other basic columns are left out, the column's own coefficient is exactly 1.
    pub fn tableau_row(&self, basic_col: usize) -> Vec<(usize, f64)> {
        let c = basic_col as u64;
        let (mut ip, mut ix, mut dv): (*const u64, *const u32, *const f64) = (ptr::null(), ptr::null(), ptr::null());
        let st = unsafe { sys::mlp_solution_tableau_rows(self.raw, &c, 1, &mut ip, &mut ix, &mut dv) };
        assert_eq!(st, sys::MLP_OK, "{}", last_error());
        // (the three arrays belong to the library until the next tableau call: copied here)
        let n = unsafe { *ip.add(1) } as usize;
        (0..n).map(|e| unsafe { (*ix.add(e) as usize, *dv.add(e)) }).collect()
    }

    /// Tableau column B^-1 a_j (by position) of any column; a basic one gives the unit vector of its position.
    pub fn tableau_col(&self, col: usize) -> Vec<f64> {
        let (c, mut out) = (col as u64, vec![0.0f64; self.num_rows()]);
        let st = unsafe { sys::mlp_solution_tableau_cols(self.raw, &c, 1, out.as_mut_ptr(), out.len() as u64) };
        assert_eq!(st, sys::MLP_OK, "{}", last_error());
        out
    }

    /// B^-1 rhs: `rhs` by constraint, the result by position.
    pub fn ftran(&self, rhs: &[f64]) -> Vec<f64> {
        let mut out = vec![0.0f64; self.num_rows()];
        let st = unsafe { sys::mlp_solution_basis_solve(self.raw, 0, rhs.as_ptr(), rhs.len() as u64, 1, out.as_mut_ptr(), out.len() as u64) };
        assert_eq!(st, sys::MLP_OK, "{}", last_error());
        out
    }

    /// B^-T rhs: `rhs` by position, the result by constraint.
    pub fn btran(&self, rhs: &[f64]) -> Vec<f64> {
        let mut out = vec![0.0f64; self.num_constraints()];
        let st = unsafe { sys::mlp_solution_basis_solve(self.raw, 1, rhs.as_ptr(), rhs.len() as u64, 1, out.as_mut_ptr(), out.len() as u64) };
        assert_eq!(st, sys::MLP_OK, "{}", last_error());
        out
    }

    /// Iterate over the variable-value pairs of the solution.
    pub fn iter(&self) -> SolutionIter {
        SolutionIter { solution: self, var_idx: 0 }
    }

    /// Runs one consuming C call: on a non-zero status the library has already freed the solver
    /// (consume-on-error, the reference drops `self` at `lib.rs:359, 385`).
    fn consume(mut self, f: impl FnOnce(*mut *mut sys::mlp_solution) -> std::os::raw::c_int) -> Result<Self, Error> {
        let mut raw = self.raw;
        self.raw = ptr::null_mut(); // whatever happens, `self` no longer owns it
        let st = f(&mut raw);
        check(st)?; // on Err the library freed and nulled `raw`
        Ok(Solution::from_raw(raw, self.num_vars))
    }

    /// Add another constraint and return the solution to the updated problem.  (`lib.rs:368-388`)
    ///
    /// # Errors
    ///
    /// Will return an error if the problem becomes infeasible with the additional constraint.
    pub fn add_constraint(self, expr: impl Into<LinearExpr>, cmp_op: ComparisonOp, rhs: f64) -> Result<Self, Error> {
        let expr = expr.into();
        let vars: Vec<u32> = expr.vars.iter().map(|&v| v as u32).collect();
        self.consume(|s| unsafe {
            sys::mlp_solution_add_constraint(s, vars.as_ptr(), expr.coeffs.as_ptr(), vars.len() as u64, cmp_op.to_c(), rhs)
        })
    }

    /// Fix the variable to the specified value and return the solution to the updated problem.  (`lib.rs:390-397`)
    ///
    /// # Errors
    ///
    /// Will return an error if the problem becomes infeasible with the additional constraint.
    pub fn fix_var(self, var: Variable, val: f64) -> Result<Self, Error> {
        assert!(var.0 < self.num_vars);
        self.consume(|s| unsafe { sys::mlp_solution_fix_var(s, var.0 as u32, val) })
    }

    /// If the variable was fixed with [`fix_var`](Self::fix_var) before, remove that constraint and return the
    /// solution to the updated problem and a boolean indicating if the variable was really fixed.  (`lib.rs:399-417`)
    pub fn unfix_var(self, var: Variable) -> (Self, bool) {
        assert!(var.0 < self.num_vars);
        let mut was: std::os::raw::c_int = 0;
        let sol = self
            .consume(|s| unsafe { sys::mlp_solution_unfix_var(s, var.0 as u32, &mut was) })
            .expect("unfix_var cannot make the problem infeasible or unbounded (lib.rs:433 unwrap)");
        (sol, was != 0)
    }

    /// [`fix_var`](Self::fix_var) for every `(variable, value)` pair in one call: the variables that are non-basic share one
    /// FTRAN (none at all when each already sits at its value), the basic ones take one forced pivot each, and feasibility is
    /// restored once.  The model left behind is that of the single form called pair by pair (extension: no counterpart in the
    /// reference).
    ///
    /// # Errors
    ///
    /// Will return an error if a value lies outside the bounds of its variable or the problem becomes infeasible.
    ///
    /// # Panics
    ///
    /// Will panic if a variable is listed twice.
    pub fn fix_vars(self, fixings: &[(Variable, f64)]) -> Result<Self, Error> {
        assert!(fixings.iter().all(|x| x.0 .0 < self.num_vars));
        let mut seen: Vec<usize> = fixings.iter().map(|x| x.0 .0).collect();
        seen.sort_unstable();
        assert!(seen.windows(2).all(|w| w[0] != w[1]), "fix_vars: a variable is listed twice");
        let vars: Vec<u32> = fixings.iter().map(|x| x.0 .0 as u32).collect();
        let vals: Vec<f64> = fixings.iter().map(|x| x.1).collect();
        self.consume(|s| unsafe { sys::mlp_solution_fix_vars(s, vars.as_ptr(), vals.as_ptr(), vars.len() as u64) })
    }

    /// [`unfix_var`](Self::unfix_var) for every listed variable with one re-solve; returns the solution and how many of the
    /// variables were really fixed (extension).
    pub fn unfix_vars(self, vars: &[Variable]) -> (Self, usize) {
        assert!(vars.iter().all(|x| x.0 < self.num_vars));
        let v: Vec<u32> = vars.iter().map(|x| x.0 as u32).collect();
        let mut released: u64 = 0;
        let sol = self
            .consume(|s| unsafe { sys::mlp_solution_unfix_vars(s, v.as_ptr(), v.len() as u64, &mut released) })
            .expect("unfix_vars cannot make the problem infeasible or unbounded (lib.rs:433 unwrap)");
        (sol, released as usize)
    }

    /// New bounds `(variable, lo, hi)` for variables of a solved model, then one dual re-solve from the current basis (none when
    /// nothing moves).  A non-basic variable keeps its side and moves with its bound; making that bound infinite is refused
    /// (extension: no counterpart in the reference; semantics in `minilp_hip.h`).
    ///
    /// # Errors
    ///
    /// Will return an error if `lo > hi` for a variable or the problem becomes infeasible with the new bounds.
    ///
    /// # Panics
    ///
    /// Will panic if a variable is listed twice.
    pub fn set_var_bounds(self, bounds: &[(Variable, f64, f64)]) -> Result<Self, Error> {
        assert!(bounds.iter().all(|x| x.0 .0 < self.num_vars));
        let mut seen: Vec<usize> = bounds.iter().map(|x| x.0 .0).collect();
        seen.sort_unstable();
        assert!(seen.windows(2).all(|w| w[0] != w[1]), "set_var_bounds: a variable is listed twice");
        let vars: Vec<u32> = bounds.iter().map(|x| x.0 .0 as u32).collect();
        let lo: Vec<f64> = bounds.iter().map(|x| x.1).collect();
        let hi: Vec<f64> = bounds.iter().map(|x| x.2).collect();
        self.consume(|s| unsafe { sys::mlp_solution_set_var_bounds(s, vars.as_ptr(), lo.as_ptr(), hi.as_ptr(), vars.len() as u64) })
    }

    /// [`cutoff_bounds`](Self::cutoff_bounds) with every entry applied to the bounds on the device; returns the solution, how many
    /// bounds were tightened and whether this LP is already worse than the cutoff (then nothing changes).  Values and objective
    /// keep their bits (extension).
    pub fn tighten_by_reduced_cost(self, cutoff: f64, integer_vars: Option<&[bool]>) -> (Self, usize, bool) {
        let vm: Option<Vec<u8>> = integer_vars.map(|m| m.iter().map(|&b| b as u8).collect());
        let (vp, vn) = vm.as_ref().map_or((std::ptr::null(), self.num_vars as u32), |m| (m.as_ptr(), m.len() as u32));
        let (mut count, mut pruned): (u64, std::os::raw::c_int) = (0, 0);
        let sol = self
            .consume(|s| unsafe { sys::mlp_solution_tighten_by_reduced_cost(s, cutoff, vp, vn, &mut count, &mut pruned) })
            .expect("tighten_by_reduced_cost moves no value: it cannot make the problem infeasible");
        (sol, count as usize, pruned != 0)
    }

    /// [`propagate_bounds`](Self::propagate_bounds) with the whole list applied through the body of
    /// [`set_var_bounds`](Self::set_var_bounds): one dual re-solve at most.  Returns the solution, how many variables were tightened
    /// and whether the rounds proved the model infeasible (then nothing changes: prune the node).  Needs a solved model (extension).
    ///
    /// # Errors
    ///
    /// Will return an error if the re-solve with the tightened bounds finds the problem infeasible.
    pub fn tighten_by_propagation(self, integer_vars: Option<&[bool]>, max_rounds: usize) -> Result<(Self, usize, bool), Error> {
        let vm: Option<Vec<u8>> = integer_vars.map(|m| m.iter().map(|&b| b as u8).collect());
        let (vp, vn) = vm.as_ref().map_or((std::ptr::null(), self.num_vars as u32), |m| (m.as_ptr(), m.len() as u32));
        let (mut count, mut infeasible): (u64, std::os::raw::c_int) = (0, 0);
        let rounds = max_rounds.min(65) as i32;
        let sol = self.consume(|s| unsafe { sys::mlp_solution_tighten_by_propagation(s, vp, vn, rounds, &mut count, &mut infeasible) })?;
        Ok((sol, count as usize, infeasible != 0))
    }

    /// Bounds `(lo, hi)` of a variable as the solution holds them now (extension).
    pub fn var_bounds(&self, var: Variable) -> (f64, f64) {
        assert!(var.0 < self.num_vars);
        let (v, mut lo, mut hi) = (var.0 as u32, 0.0f64, 0.0f64);
        let st = unsafe { sys::mlp_solution_var_bounds(self.raw, &v, 1, &mut lo, &mut hi) };
        assert_eq!(st, sys::MLP_OK, "{}", last_error());
        (lo, hi)
    }

    /// New right-hand sides `(constraint, rhs)` for constraints of a solved model (numbering of
    /// [`num_constraints`](Self::num_constraints)), then one dual re-solve from the current basis (none when every basic value
    /// stays within its bounds).  Operators stay as they are (extension: no counterpart in the reference; semantics in
    /// `minilp_hip.h`).
    ///
    /// # Errors
    ///
    /// Will return an error if the problem becomes infeasible with the new right-hand sides.
    ///
    /// # Panics
    ///
    /// Will panic if a constraint is out of range or listed twice.
    pub fn set_rhs(self, changes: &[(usize, f64)]) -> Result<Solution, Error> {
        let m = self.num_constraints();
        assert!(changes.iter().all(|x| x.0 < m));
        let mut seen: Vec<usize> = changes.iter().map(|x| x.0).collect();
        seen.sort_unstable();
        assert!(seen.windows(2).all(|w| w[0] != w[1]), "set_rhs: a constraint is listed twice");
        let cons: Vec<u64> = changes.iter().map(|x| x.0 as u64).collect();
        let rhs: Vec<f64> = changes.iter().map(|x| x.1).collect();
        self.consume(|s| unsafe { sys::mlp_solution_set_rhs(s, cons.as_ptr(), rhs.as_ptr(), cons.len() as u64) })
    }

    /// Right-hand side of a constraint as the solution holds it now (extension).
    pub fn constraint_rhs(&self, constraint: usize) -> f64 {
        let (c, mut rhs) = (constraint as u64, 0.0f64);
        let st = unsafe { sys::mlp_solution_constraint_rhs(self.raw, &c, 1, &mut rhs) };
        assert_eq!(st, sys::MLP_OK, "{}", last_error());
        rhs
    }

    /// Candidate right-hand sides against the current basis, 16 per batch on the device: scenario `s` gives `constraints[i]` the
    /// right-hand side `rhs[s][i]`.  Per scenario `(bound, feasible, worst, worst_col)`: the objective its basis would report (the
    /// optimum where `feasible`, else a bound from the dual side), whether every basic value stays within its bounds (then
    /// [`set_rhs`](Self::set_rhs) runs no pivot), the largest violation and the column basic where it occurs (numbering of
    /// [`basis_head`](Self::basis_head)).  The solution is left as it is (extension).
    ///
    /// # Panics
    ///
    /// Will panic if a scenario's length differs from the list's, or if the library refuses the call (a constraint out of range,
    /// listed twice or without terms, a model that is not solved).
    pub fn rhs_scenarios(&self, constraints: &[usize], rhs: &[Vec<f64>]) -> Vec<(f64, bool, f64, Option<usize>)> {
        let n = constraints.len();
        assert!(rhs.iter().all(|r| r.len() == n), "rhs_scenarios: every scenario needs one value per listed constraint");
        let cons: Vec<u64> = constraints.iter().map(|&c| c as u64).collect();
        let flat: Vec<f64> = rhs.iter().flat_map(|r| r.iter().copied()).collect();
        let s = rhs.len();
        let (mut bound, mut worst) = (vec![0.0f64; s], vec![0.0f64; s]);
        let (mut feasible, mut col) = (vec![0u8; s], vec![0i64; s]);
        let st = unsafe {
            sys::mlp_solution_rhs_scenarios(self.raw, cons.as_ptr(), n as u64, flat.as_ptr(), s as u64, bound.as_mut_ptr(),
                                            feasible.as_mut_ptr(), worst.as_mut_ptr(), col.as_mut_ptr())
        };
        assert_eq!(st, sys::MLP_OK, "{}", last_error());
        (0..s).map(|i| (bound[i], feasible[i] != 0, worst[i], if col[i] < 0 { None } else { Some(col[i] as usize) })).collect()
    }

    /// Add a Gomory cut constraint to the problem and return the solution.  (`lib.rs:419-423`)
    ///
    /// # Errors
    ///
    /// Will return an error if the problem becomes infeasible with the additional constraint.
    ///
    /// # Panics
    ///
    /// Will panic if the variable is not basic (variable is basic if it has value other than its bounds).
    pub fn add_gomory_cut(self, var: Variable) -> Result<Self, Error> {
        assert!(var.0 < self.num_vars);
        self.consume(|s| unsafe { sys::mlp_solution_add_gomory_cut(s, var.0 as u32) })
    }

    /// Add a whole round of constraints in one call and return the solution to the updated problem: every row is
    /// appended to the model, then feasibility is restored once.  The model left behind is that of
    /// [`add_constraint`](Self::add_constraint) called row by row in the same order (extension: no counterpart in the
    /// reference).
    ///
    /// # Errors
    ///
    /// Will return an error if the problem becomes infeasible with the additional constraints.
    pub fn add_constraints(self, rows: Vec<(LinearExpr, ComparisonOp, f64)>) -> Result<Self, Error> {
        let mut indptr: Vec<u64> = vec![0];
        let mut vars: Vec<u32> = Vec::new();
        let mut coeffs: Vec<f64> = Vec::new();
        let mut ops: Vec<i32> = Vec::new();
        let mut rhs: Vec<f64> = Vec::new();
        for (expr, op, r) in &rows {
            vars.extend(expr.vars.iter().map(|&v| v as u32));
            coeffs.extend_from_slice(&expr.coeffs);
            indptr.push(vars.len() as u64);
            ops.push(op.to_c() as i32);
            rhs.push(*r);
        }
        self.consume(|s| unsafe {
            sys::mlp_solution_add_constraints_csr(s, rhs.len() as u64, indptr.as_ptr(), vars.as_ptr(), coeffs.as_ptr(), ops.as_ptr(), rhs.as_ptr())
        })
    }

    /// Add one round of Gomory cuts, one per listed variable, all taken from the current basis, and return the
    /// solution (extension: the reference adds one cut per call, `lib.rs:419-423`).
    ///
    /// # Errors
    ///
    /// Will return an error if the problem becomes infeasible with the additional constraints.
    ///
    /// # Panics
    ///
    /// Will panic if a variable is listed twice or is not basic.
    pub fn add_gomory_cuts(self, vars: &[Variable]) -> Result<Self, Error> {
        let v: Vec<u32> = vars.iter().map(|x| x.0 as u32).collect();
        assert!(vars.iter().all(|x| x.0 < self.num_vars));
        self.consume(|s| unsafe { sys::mlp_solution_add_gomory_cuts(s, v.as_ptr(), v.len() as u64) })
    }

    /// Add one round of Gomory mixed-integer cuts, one per listed basic integer variable, all taken from the current
    /// basis, and return the solution with a status per request: 0 emitted, 1 skipped (fraction within `away`),
    /// 2 skipped (a free non-basic column in the row).  `integer_vars[j]` marks variable `j` as integer;
    /// `integer_constraints[c]` marks the slack of constraint `c` (`None`: all slacks continuous).  The cuts are valid
    /// for the bounds the call finds (extension: no counterpart in the reference; semantics in `minilp_hip.h`).
    ///
    /// # Errors
    ///
    /// Will return an error if the problem becomes infeasible with the additional constraints.
    ///
    /// # Panics
    ///
    /// Will panic if a variable is listed twice, is not basic or is not marked integer, if a mask has the wrong
    /// length, or if `away` is not in (0, 0.5].
    pub fn add_gmi_cuts(self, vars: &[Variable], integer_vars: &[bool], integer_constraints: Option<&[bool]>, away: f64) -> Result<(Self, Vec<i32>), Error> {
        let v: Vec<u32> = vars.iter().map(|x| x.0 as u32).collect();
        assert!(vars.iter().all(|x| x.0 < self.num_vars));
        let vm: Vec<u8> = integer_vars.iter().map(|&b| b as u8).collect();
        let cm: Option<Vec<u8>> = integer_constraints.map(|m| m.iter().map(|&b| b as u8).collect());
        let (cp, cn) = cm.as_ref().map_or((std::ptr::null(), 0u64), |m| (m.as_ptr(), m.len() as u64));
        let mut status = vec![0i32; v.len()];
        let sp = status.as_mut_ptr();
        let out = self.consume(|s| unsafe {
            sys::mlp_solution_add_gmi_cuts(s, v.as_ptr(), v.len() as u64, vm.as_ptr(), vm.len() as u32, cp, cn, away, sp)
        })?;
        Ok((out, status))
    }

    /// The raw handle, for the engine-level stepping API and the diagnostics of `minilp-hip-sys`
    /// (not part of the reference's API).
    pub fn as_raw(&self) -> *mut sys::mlp_solution {
        self.raw
    }
}

impl std::ops::Index<Variable> for Solution {
    type Output = f64;

    fn index(&self, var: Variable) -> &Self::Output {
        self.var_value(var)
    }
}

/// An iterator over the variable-value pairs of a [`Solution`].  (`lib.rs:435-462`)
#[derive(Debug, Clone)]
pub struct SolutionIter<'a> {
    solution: &'a Solution,
    var_idx: usize,
}

impl<'a> Iterator for SolutionIter<'a> {
    type Item = (Variable, &'a f64);

    fn next(&mut self) -> Option<Self::Item> {
        if self.var_idx < self.solution.num_vars {
            let var_idx = self.var_idx;
            self.var_idx += 1;
            Some((Variable(var_idx), &self.solution.values()[var_idx]))
        } else {
            None
        }
    }
}

impl<'a> IntoIterator for &'a Solution {
    type Item = (Variable, &'a f64);
    type IntoIter = SolutionIter<'a>;

    fn into_iter(self) -> Self::IntoIter {
        self.iter()
    }
}

#[cfg(test)]
mod tests {
    //! The reference's own tests of `lib.rs:466-646`, unchanged in substance: they are the acceptance tests of a
    //! drop-in.  (The same cases run on the GPU box through the ctypes mirror: tests/test_hip_parity.py.)
    use super::*;

    #[test]
    fn optimize() {
        let mut problem = Problem::new(OptimizationDirection::Maximize);
        let v1 = problem.add_var(3.0, (12.0, f64::INFINITY));
        let v2 = problem.add_var(4.0, (5.0, f64::INFINITY));
        problem.add_constraint(&[(v1, 1.0), (v2, 1.0)], ComparisonOp::Le, 20.0);
        problem.add_constraint(&[(v2, -4.0), (v1, 1.0)], ComparisonOp::Ge, -20.0);
        let sol = problem.solve().unwrap();
        assert_eq!(sol[v1], 12.0);
        assert_eq!(sol[v2], 8.0);
        assert_eq!(sol.objective(), 68.0);
    }

    #[test]
    fn fix_unfix_var() {
        let mut problem = Problem::new(OptimizationDirection::Maximize);
        let v1 = problem.add_var(1.0, (0.0, 3.0));
        let v2 = problem.add_var(2.0, (0.0, 3.0));
        problem.add_constraint(&[(v1, 1.0), (v2, 1.0)], ComparisonOp::Le, 4.0);
        problem.add_constraint(&[(v1, 1.0), (v2, 1.0)], ComparisonOp::Ge, 1.0);
        let orig_sol = problem.solve().unwrap();
        let sol = orig_sol.clone().fix_var(v1, 0.5).unwrap();
        assert_eq!(sol[v1], 0.5);
        assert_eq!(sol[v2], 3.0);
        assert_eq!(sol.objective(), 6.5);
        let (sol, was_fixed) = sol.unfix_var(v1);
        assert!(was_fixed);
        assert_eq!(sol[v1], 1.0);
        assert_eq!(sol.objective(), 7.0);
    }

    #[test]
    fn infeasible_constraint_consumes_the_solution() {
        let mut problem = Problem::new(OptimizationDirection::Minimize);
        let v = problem.add_var(1.0, (0.0, 1.0));
        let sol = problem.solve().unwrap();
        assert_eq!(sol.add_constraint(&[(v, 1.0)], ComparisonOp::Ge, 2.0).unwrap_err(), Error::Infeasible);
    }
}
