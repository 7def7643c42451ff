"""ctypes binding of libminilp_hip.so with the reference's names and argument meaning
(lib.rs:61-464: OptimizationDirection, ComparisonOp, Problem, Solution, Error; mps.rs: MpsFile)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libminilp_hip.so")
# the sharded solve maps peer mailboxes through HIP IPC: this driver stack only supports the dmabuf flavour
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

MINIMIZE, MAXIMIZE = 0, 1          # lib.rs:61-68 OptimizationDirection
EQ, LE, GE = 0, 1, 2               # lib.rs:160-169 ComparisonOp


class Infeasible(Exception):       # lib.rs:175 Error::Infeasible
    pass


class Unbounded(Exception):        # lib.rs:177 Error::Unbounded
    pass


class InternalError(Exception):    # where the reference panics (or a HIP error / missing GPU)
    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code = code


class MlpStats(C.Structure):
    _fields_ = ([(n, C.c_uint64) for n in ("iterations", "basis_changes", "bound_flips", "primal_iters", "dual_iters",
                                            "reinversions", "num_constraints", "num_total_vars", "nucleus_size",
                                            "nucleus_capacity", "nnz")]
                + [(n, C.c_double) for n in ("fused_bytes", "fused_ms", "sweep_bytes", "sweep_ms")]
                + [(n, C.c_uint64) for n in ("fused_launches", "sweep_launches")]
                + [("solve_wall_s", C.c_double), ("kase", C.c_uint64 * 5), ("update_ms", C.c_double),
                   ("update_launches", C.c_uint64), ("banded_sweep", C.c_uint64), ("final_refreshes", C.c_uint64), ("max_pivot_err", C.c_double),
                   ("ftran_bytes", C.c_double), ("ftran_ms", C.c_double), ("ftran_launches", C.c_uint64),
                   ("iter_ms", C.c_double), ("iter_samples", C.c_uint64), ("beta_rebuilds", C.c_uint64),
                   ("fold_bytes", C.c_double), ("fold_ms", C.c_double), ("fold_launches", C.c_uint64),
                   ("dense_ftran_bytes", C.c_double), ("dense_ftran_ms", C.c_double), ("dense_ftran_launches", C.c_uint64),
                   ("str_ms", C.c_double), ("str_launches", C.c_uint64),
                   ("hyper_iters", C.c_uint64), ("hyper_bails", C.c_uint64), ("ratio_stalls", C.c_uint64),
                   ("reinversion_fallbacks", C.c_uint64),
                   ("factor_active", C.c_uint64), ("factor_refactors", C.c_uint64), ("factor_levels", C.c_uint64),
                   ("factor_switches", C.c_uint64), ("factor_bump", C.c_uint64), ("factor_bump_max", C.c_uint64)])  # appended in ABI version 4 (the struct only grows at its end from here on)


class MlpCertificate(C.Structure):  # include/minilp_hip.h: mlp_certificate (only grows at its end)
    _fields_ = [("primal_objective", C.c_double), ("dual_objective", C.c_double), ("relative_gap", C.c_double),
                ("max_row_violation", C.c_double), ("max_row_violation_at", C.c_int64),
                ("max_bound_violation", C.c_double), ("max_bound_violation_at", C.c_int64),
                ("max_dual_infeasibility", C.c_double), ("max_dual_infeasibility_at", C.c_int64),
                ("btran_residual", C.c_double), ("btran_residual_at", C.c_int64),
                ("bytes", C.c_double), ("device_ms", C.c_double)]


class MlpRangingInfo(C.Structure):  # include/minilp_hip.h: mlp_ranging_info (only grows at its end)
    _fields_ = [("requests", C.c_uint64), ("solves", C.c_uint64), ("batches", C.c_uint64), ("bytes", C.c_double), ("device_ms", C.c_double)]


class MlpCutInfo(C.Structure):  # include/minilp_hip.h: mlp_cut_info (only grows at its end)
    _fields_ = [("rows", C.c_uint64), ("rows_without_terms", C.c_uint64), ("nnz", C.c_uint64), ("batches", C.c_uint64),
                ("relayouts", C.c_uint64), ("reinversions", C.c_uint64), ("pivots", C.c_uint64),
                ("bytes", C.c_double), ("device_ms", C.c_double), ("wall_ms", C.c_double)]


class MlpTableauInfo(C.Structure):  # include/minilp_hip.h: mlp_tableau_info (only grows at its end)
    _fields_ = [("requests", C.c_uint64), ("solves", C.c_uint64), ("batches", C.c_uint64), ("nnz", C.c_uint64),
                ("bytes", C.c_double), ("device_ms", C.c_double)]


class MlpGmiInfo(C.Structure):  # include/minilp_hip.h: mlp_gmi_info (only grows at its end)
    _fields_ = [("requests", C.c_uint64), ("rows", C.c_uint64), ("skipped_fraction", C.c_uint64), ("skipped_free", C.c_uint64),
                ("nnz", C.c_uint64), ("batches", C.c_uint64), ("bytes", C.c_double), ("device_ms", C.c_double)]


class MlpBranchInfo(C.Structure):  # include/minilp_hip.h: mlp_branch_info (only grows at its end)
    _fields_ = [("requests", C.c_uint64), ("solves", C.c_uint64), ("batches", C.c_uint64), ("bytes", C.c_double), ("device_ms", C.c_double)]


class MlpFixInfo(C.Structure):  # include/minilp_hip.h: mlp_fix_info (only grows at its end)
    _fields_ = [("requests", C.c_uint64), ("nonbasic", C.c_uint64), ("shifted", C.c_uint64), ("forced_pivots", C.c_uint64),
                ("solves", C.c_uint64), ("unfixed", C.c_uint64), ("listed", C.c_uint64), ("listed_fixed", C.c_uint64),
                ("pivots", C.c_uint64), ("bytes", C.c_double), ("device_ms", C.c_double), ("wall_ms", C.c_double)]


class MlpBoundsInfo(C.Structure):  # include/minilp_hip.h: mlp_bounds_info (only grows at its end)
    _fields_ = [("requests", C.c_uint64), ("basic", C.c_uint64), ("nonbasic", C.c_uint64), ("shifted", C.c_uint64), ("solves", C.c_uint64),
                ("tightened", C.c_uint64), ("pivots", C.c_uint64), ("bytes", C.c_double), ("device_ms", C.c_double), ("wall_ms", C.c_double)]


class MlpPropagateInfo(C.Structure):  # include/minilp_hip.h: mlp_propagate_info (only grows at its end)
    _fields_ = [("requests", C.c_uint64), ("rounds", C.c_uint64), ("accepted", C.c_uint64), ("listed", C.c_uint64),
                ("listed_fixed", C.c_uint64), ("bytes", C.c_double), ("device_ms", C.c_double)]


class MlpRhsInfo(C.Structure):  # include/minilp_hip.h: mlp_rhs_info (only grows at its end)
    _fields_ = [("requests", C.c_uint64), ("changed", C.c_uint64), ("scenarios", C.c_uint64), ("solves", C.c_uint64),
                ("batches", C.c_uint64), ("pivots", C.c_uint64), ("bytes", C.c_double), ("device_ms", C.c_double), ("wall_ms", C.c_double)]


# basis status of a variable / of a constraint's slack (include/minilp_hip.h)
MLP_BASIC, MLP_AT_LOWER, MLP_AT_UPPER, MLP_NB_FREE, MLP_NB_FIXED = range(5)

ABI_VERSION = 5  # include/minilp_hip.h: MLP_ABI_VERSION
# (size function of the library, the class here): lib() refuses a library whose struct differs in size
_STRUCT_SIZES = (("mlp_certificate_size", MlpCertificate), ("mlp_ranging_info_size", MlpRangingInfo), ("mlp_cut_info_size", MlpCutInfo),
                 ("mlp_tableau_info_size", MlpTableauInfo), ("mlp_gmi_info_size", MlpGmiInfo), ("mlp_branch_info_size", MlpBranchInfo),
                 ("mlp_fix_info_size", MlpFixInfo), ("mlp_bounds_info_size", MlpBoundsInfo), ("mlp_propagate_info_size", MlpPropagateInfo),
                 ("mlp_rhs_info_size", MlpRhsInfo))


class MlpIterInfo(C.Structure):  # include/minilp_hip.h: mlp_iter_info
    _fields_ = [("status", C.c_int32), ("phase", C.c_int32), ("next_stage", C.c_int32), ("reserved", C.c_int32),
                ("col", C.c_int64), ("row", C.c_int64), ("entering_var", C.c_int64), ("leaving_var", C.c_int64),
                ("pivot_coeff", C.c_double), ("step", C.c_double), ("objective", C.c_double), ("nucleus_size", C.c_uint64)]


STAGE_FTRAN, STAGE_RATIO, STAGE_BTRAN, STAGE_BASIS, STAGE_ROW, STAGE_APPLY = range(6)
ITER_PIVOT, ITER_FLIP, ITER_OPTIMAL, ITER_UNBOUNDED, ITER_FEASIBLE, ITER_INFEASIBLE, ITER_SINGULAR = range(7)

_lib = None


def lib_path():
    return _SO


def lib():
    """Load the HIP extension.  Fails loudly if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise ImportError(f"{_SO} is missing: build it with `python -m minilp_amd.build` (hipcc, gfx950). "
                          "minilp_amd has no CPU fallback.")
    L = C.CDLL(_SO)
    vp, u64, i64, u32, dbl, i32 = C.c_void_p, C.c_uint64, C.c_int64, C.c_uint32, C.c_double, C.c_int
    pu32, pdbl = C.POINTER(C.c_uint32), C.POINTER(C.c_double)

    def sig(name, res, *args):
        f = getattr(L, name)
        f.restype = res
        f.argtypes = list(args)

    sig("mlp_abi_version", u32)
    sig("mlp_stats_size", u64)
    if L.mlp_abi_version() != ABI_VERSION or L.mlp_stats_size() != C.sizeof(MlpStats):
        raise ImportError(f"{_SO} was built from another version of include/minilp_hip.h (ABI {L.mlp_abi_version()}, mlp_stats "
                          f"{L.mlp_stats_size()} bytes; this binding: ABI {ABI_VERSION}, {C.sizeof(MlpStats)} bytes): rebuild it")
    for size_fn, struct in _STRUCT_SIZES:
        sig(size_fn, u64)
        if getattr(L, size_fn)() != C.sizeof(struct):
            raise ImportError(f"{_SO}: {size_fn[:-5]} is {getattr(L, size_fn)()} bytes, this binding {C.sizeof(struct)}: rebuild it")
    sig("mlp_last_error", C.c_char_p)
    sig("mlp_device_count", i32)
    sig("mlp_set_device", i32, i32)
    sig("mlp_problem_new", vp, i32)
    sig("mlp_problem_clone", vp, vp)
    sig("mlp_problem_free", None, vp)
    sig("mlp_problem_add_var", u32, vp, dbl, dbl, dbl)
    sig("mlp_problem_num_vars", u32, vp)
    sig("mlp_problem_add_constraint", i32, vp, pu32, pdbl, u64, i32, dbl)
    sig("mlp_problem_add_vars", i32, vp, u64, pdbl, pdbl, pdbl)
    sig("mlp_problem_add_constraints_csr", i32, vp, u64, C.POINTER(C.c_uint64), pu32, pdbl, C.POINTER(C.c_int32), pdbl)
    sig("mlp_problem_solve", i32, vp, C.POINTER(vp))
    sig("mlp_problem_num_constraints", u64, vp)
    sig("mlp_problem_var", i32, vp, u32, pdbl, pdbl, pdbl)
    sig("mlp_problem_constraint", u64, vp, u64, pu32, pdbl, u64, C.POINTER(i32), pdbl)
    sig("mlp_problem_solve_ex", i32, vp, C.POINTER(vp), i64, u32)
    sig("mlp_solution_continue", i32, vp, i64)
    sig("mlp_solution_save_basis", u64, vp, i32, vp, u64)
    sig("mlp_problem_solve_from_basis", i32, vp, vp, u64, C.POINTER(vp), i64, u32)
    sig("mlp_solution_set_sampling", i32, vp, i32)
    sig("mlp_solution_budget_exhausted", i32, vp)
    sig("mlp_solution_reinvert", i32, vp, pdbl)
    sig("mlp_solution_recompute_basic_values", i32, vp)
    sig("mlp_solution_enable_sharding", i32, vp, i32, i32, C.c_char_p)
    sig("mlp_solution_enable_sharding_ex", i32, vp, i32, i32, C.c_char_p, C.c_char_p, vp)
    sig("mlp_rccl_unique_id", i32, vp)
    sig("mlp_solution_transport", C.c_char_p, vp)
    sig("mlp_solution_clone", vp, vp)
    sig("mlp_solution_free", None, vp)
    sig("mlp_solution_objective", dbl, vp)
    sig("mlp_solution_num_vars", u32, vp)
    sig("mlp_solution_var_value", i32, vp, u32, pdbl)
    sig("mlp_solution_values", i32, vp, pdbl, u32)
    sig("mlp_solution_add_constraint", i32, C.POINTER(vp), pu32, pdbl, u64, i32, dbl)
    sig("mlp_solution_fix_var", i32, C.POINTER(vp), u32, dbl)
    sig("mlp_solution_unfix_var", i32, C.POINTER(vp), u32, C.POINTER(i32))
    sig("mlp_solution_add_gomory_cut", i32, C.POINTER(vp), u32)
    sig("mlp_solution_stats", None, vp, C.POINTER(MlpStats))
    sig("mlp_solution_reset_stats", None, vp)
    sig("mlp_solution_trace_len", u64, vp)
    sig("mlp_solution_trace_get", None, vp, u64, C.POINTER(C.c_int32), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64),
        C.POINTER(i64), pdbl, pdbl)
    sig("mlp_solution_state", u64, vp, C.c_char_p, pdbl, u64)
    sig("mlp_mps_parse", i32, C.c_char_p, u64, i32, C.POINTER(vp))
    sig("mlp_mps_free", None, vp)
    sig("mlp_mps_name", C.c_char_p, vp)
    sig("mlp_mps_num_vars", u32, vp)
    sig("mlp_mps_var_name", C.c_char_p, vp, u32)
    sig("mlp_mps_var_index", i64, vp, C.c_char_p)
    sig("mlp_mps_problem", vp, vp)
    sig("mlp_util_min_cut", C.c_double, u32, pdbl, C.POINTER(C.c_uint8))
    sig("mlp_solution_num_constraints", u64, vp)
    sig("mlp_solution_dual_values", i32, vp, pdbl, u64)
    sig("mlp_solution_dual_value", i32, vp, u64, pdbl)
    sig("mlp_solution_reduced_costs", i32, vp, pdbl, u32)
    sig("mlp_solution_reduced_cost", i32, vp, u32, pdbl)
    sig("mlp_solution_certificate", i32, vp, C.POINTER(MlpCertificate))
    sig("mlp_solution_basis_status", i32, vp, C.POINTER(C.c_int32), u32, C.POINTER(C.c_int32), u64)
    sig("mlp_solution_cost_ranging", i32, vp, pu32, u64, pdbl, pdbl)
    sig("mlp_solution_rhs_ranging", i32, vp, C.POINTER(C.c_uint64), u64, pdbl, pdbl)
    sig("mlp_solution_ranging_info", i32, vp, C.POINTER(MlpRangingInfo))
    sig("mlp_solution_add_constraints_csr", i32, C.POINTER(vp), u64, C.POINTER(C.c_uint64), pu32, pdbl, C.POINTER(C.c_int32), pdbl)
    sig("mlp_solution_add_gomory_cuts", i32, C.POINTER(vp), pu32, u64)
    sig("mlp_solution_cut_info", i32, vp, C.POINTER(MlpCutInfo))
    pu64 = C.POINTER(C.c_uint64)
    sig("mlp_solution_num_rows", u64, vp)
    sig("mlp_solution_basis_head", i32, vp, pu64, u64)
    sig("mlp_solution_binv_rows", i32, vp, pu64, u64, pdbl, u64)
    sig("mlp_solution_binv_cols", i32, vp, pu64, u64, pdbl, u64)
    sig("mlp_solution_tableau_rows", i32, vp, pu64, u64, C.POINTER(pu64), C.POINTER(pu32), C.POINTER(pdbl))
    sig("mlp_solution_tableau_cols", i32, vp, pu64, u64, pdbl, u64)
    sig("mlp_solution_basis_solve", i32, vp, i32, pdbl, u64, u64, pdbl, u64)
    sig("mlp_solution_tableau_info", i32, vp, C.POINTER(MlpTableauInfo))
    pu8 = C.POINTER(C.c_uint8)
    sig("mlp_solution_add_gmi_cuts", i32, C.POINTER(vp), pu32, u64, pu8, u32, pu8, u64, dbl, C.POINTER(C.c_int32))
    sig("mlp_solution_gmi_info", i32, vp, C.POINTER(MlpGmiInfo))
    sig("mlp_solution_branch_penalties", i32, vp, pu32, u64, pu8, u32, pu8, u64, pdbl, pdbl, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
        pdbl, C.POINTER(C.c_int32))
    sig("mlp_solution_branch_info", i32, vp, C.POINTER(MlpBranchInfo))
    sig("mlp_solution_cutoff_bounds", i32, vp, dbl, pu8, u32, pu32, pdbl, pdbl, u64, pu64, C.POINTER(i32))
    sig("mlp_solution_fix_vars", i32, C.POINTER(vp), pu32, pdbl, u64)
    sig("mlp_solution_unfix_vars", i32, C.POINTER(vp), pu32, u64, pu64)
    sig("mlp_solution_fix_info", i32, vp, C.POINTER(MlpFixInfo))
    sig("mlp_solution_set_var_bounds", i32, C.POINTER(vp), pu32, pdbl, pdbl, u64)
    sig("mlp_solution_tighten_by_reduced_cost", i32, C.POINTER(vp), dbl, pu8, u32, pu64, C.POINTER(i32))
    sig("mlp_solution_var_bounds", i32, vp, pu32, u64, pdbl, pdbl)
    sig("mlp_solution_bounds_info", i32, vp, C.POINTER(MlpBoundsInfo))
    sig("mlp_solution_propagate_bounds", i32, vp, pu8, u32, C.c_int32, pu32, pdbl, pdbl, u64, pu64, C.POINTER(i32))
    sig("mlp_solution_tighten_by_propagation", i32, C.POINTER(vp), pu8, u32, C.c_int32, pu64, C.POINTER(i32))
    sig("mlp_solution_propagate_info", i32, vp, C.POINTER(MlpPropagateInfo))
    sig("mlp_solution_set_rhs", i32, C.POINTER(vp), pu64, pdbl, u64)
    sig("mlp_solution_constraint_rhs", i32, vp, pu64, u64, pdbl)
    sig("mlp_solution_rhs_scenarios", i32, vp, pu64, u64, pdbl, u64, pdbl, pu8, pdbl, C.POINTER(C.c_int64))
    sig("mlp_solution_rhs_info", i32, vp, C.POINTER(MlpRhsInfo))
    sig("mlp_engine_open", i32, vp, C.POINTER(MlpIterInfo))
    sig("mlp_engine_stage", i32, vp, i32, C.POINTER(MlpIterInfo))
    _lib = L
    return L


def device_count():
    return lib().mlp_device_count()


def rccl_unique_id():
    """128-byte ncclUniqueId (rank 0 makes it, the launcher distributes it) for Solution.enable_sharding_ex(..., "rccl", id)."""
    buf = (C.c_char * 128)()
    _raise(lib().mlp_rccl_unique_id(C.cast(buf, C.c_void_p)))
    return bytes(buf)


def set_device(device):
    _raise(lib().mlp_set_device(int(device)))


def _raise(st):
    if st == 0:
        return
    if st == 1:
        raise Infeasible("problem is infeasible")
    if st == 2:
        raise Unbounded("problem is unbounded")
    raise InternalError(st, lib().mlp_last_error().decode())


class LinearExpr:
    """lib.rs:84-158: a linear expression, built term by term (`LinearExpr.empty().add(x, 1.0)`) or from any
    iterable of (variable, coefficient) pairs.  Every method that takes an expression accepts either form."""

    def __init__(self, terms=()):
        self.vars, self.coeffs = [], []
        for var, coeff in terms:
            self.add(var, coeff)

    @classmethod
    def empty(cls):  # lib.rs:92
        return cls()

    def add(self, var, coeff):  # lib.rs:98
        self.vars.append(int(var))
        self.coeffs.append(float(coeff))
        return self

    def __iter__(self):
        return iter(zip(self.vars, self.coeffs))

    def __len__(self):
        return len(self.vars)


def _terms(expr):
    pairs = list(expr)
    idx = np.ascontiguousarray([int(p[0]) for p in pairs], dtype=np.uint32)
    val = np.ascontiguousarray([float(p[1]) for p in pairs], dtype=np.float64)
    return idx, val


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def min_cut(weights):
    """Stoer-Wagner global minimum cut of a dense symmetric weight matrix (host helper of the TSP
    driver, include/minilp_hip.h).  Returns (cut weight, boolean side mask)."""
    w = np.ascontiguousarray(weights, dtype=np.float64)
    n = w.shape[0]
    side = np.zeros(n, dtype=np.uint8)
    val = lib().mlp_util_min_cut(n, _p(w, C.c_double), _p(side, C.c_uint8))
    return float(val), side.astype(bool)


class Problem:
    """lib.rs:193-305.  `Problem(direction)`, `add_var(obj_coeff, (min, max)) -> Variable index`,
    `add_constraint(expr, cmp_op, rhs)` with expr an iterable of (variable, coeff), `solve()`."""

    def __init__(self, direction, _h=None):
        self._h = _h if _h is not None else lib().mlp_problem_new(int(direction))
        self.direction = direction

    def __del__(self):
        if getattr(self, "_h", None):
            lib().mlp_problem_free(self._h)
            self._h = None

    def clone(self):
        return Problem(self.direction, lib().mlp_problem_clone(self._h))

    @property
    def num_vars(self):
        return lib().mlp_problem_num_vars(self._h)

    def add_var(self, obj_coeff, bounds):
        return int(lib().mlp_problem_add_var(self._h, obj_coeff, bounds[0], bounds[1]))

    def add_constraint(self, expr, cmp_op, rhs):
        idx, val = _terms(expr)
        _raise(lib().mlp_problem_add_constraint(self._h, _p(idx, C.c_uint32), _p(val, C.c_double), len(idx), cmp_op, rhs))

    def add_constraint_arrays(self, idx, val, cmp_op, rhs):
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        _raise(lib().mlp_problem_add_constraint(self._h, _p(idx, C.c_uint32), _p(val, C.c_double), len(idx), cmp_op, rhs))

    def add_vars_bulk(self, obj_coeffs, mins, maxs):
        """n x add_var in one call; returns the index of the first new variable."""
        first = self.num_vars
        o = np.ascontiguousarray(obj_coeffs, dtype=np.float64)
        a = np.ascontiguousarray(mins, dtype=np.float64)
        b = np.ascontiguousarray(maxs, dtype=np.float64)
        _raise(lib().mlp_problem_add_vars(self._h, len(o), _p(o, C.c_double), _p(a, C.c_double), _p(b, C.c_double)))
        return first

    def add_constraints_csr(self, indptr, indices, data, cmp_ops, rhs):
        """m x add_constraint in one call (rows in CSR form)."""
        ip = np.ascontiguousarray(indptr, dtype=np.uint64)
        ix = np.ascontiguousarray(indices, dtype=np.uint32)
        dv = np.ascontiguousarray(data, dtype=np.float64)
        ops = np.ascontiguousarray(cmp_ops, dtype=np.int32)
        rh = np.ascontiguousarray(rhs, dtype=np.float64)
        _raise(lib().mlp_problem_add_constraints_csr(self._h, len(rh), _p(ip, C.c_uint64), _p(ix, C.c_uint32), _p(dv, C.c_double),
                                                     _p(ops, C.c_int32), _p(rh, C.c_double)))

    def variables(self):
        """[(obj_coeff, min, max)] as given to add_var."""
        o, a, b = C.c_double(), C.c_double(), C.c_double()
        res = []
        for v in range(self.num_vars):
            _raise(lib().mlp_problem_var(self._h, v, C.byref(o), C.byref(a), C.byref(b)))
            res.append((o.value, a.value, b.value))
        return res

    def constraints(self):
        """[(vars, coeffs, cmp_op, rhs)] with terms sorted by variable (sprs CsVec order, lib.rs:279)."""
        res = []
        op, rhs = C.c_int(), C.c_double()
        for c in range(lib().mlp_problem_num_constraints(self._h)):
            k = lib().mlp_problem_constraint(self._h, c, None, None, 0, C.byref(op), C.byref(rhs))
            idx = np.zeros(k, dtype=np.uint32)
            val = np.zeros(k, dtype=np.float64)
            lib().mlp_problem_constraint(self._h, c, _p(idx, C.c_uint32), _p(val, C.c_double), k, C.byref(op), C.byref(rhs))
            res.append((idx, val, op.value, rhs.value))
        return res

    def solve(self, budget=-1, trace=False, profile=False):
        out = C.c_void_p()
        _raise(lib().mlp_problem_solve_ex(self._h, C.byref(out), budget, (1 if trace else 0) | (2 if profile else 0)))
        return Solution(out)

    def solve_from_basis(self, blob, budget=-1, trace=False, profile=False):
        """Build the solver for this problem, install a basis saved by `Solution.save_basis` and continue."""
        blob = bytes(blob)
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        out = C.c_void_p()
        _raise(lib().mlp_problem_solve_from_basis(self._h, C.cast(buf, C.c_void_p), len(blob), C.byref(out), budget,
                                                  (1 if trace else 0) | (2 if profile else 0)))
        return Solution(out)


class Solution:
    """lib.rs:313-424.  Mutators consume self like the Rust receivers and return the new Solution;
    on error the device-resident solver is freed (lib.rs:359, 385)."""

    def __init__(self, h):
        self._h = C.c_void_p(h.value if isinstance(h, C.c_void_p) else h)

    def __del__(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().mlp_solution_free(self._h)
            self._h = C.c_void_p()

    def _take(self):
        h = C.c_void_p(self._h.value)
        self._h = C.c_void_p()
        return h

    def clone(self):
        h = lib().mlp_solution_clone(self._h)
        if not h:
            raise InternalError(-3, lib().mlp_last_error().decode())
        return Solution(C.c_void_p(h))

    def objective(self):
        return lib().mlp_solution_objective(self._h)

    @property
    def num_vars(self):
        return lib().mlp_solution_num_vars(self._h)

    def var_value(self, var):
        out = C.c_double()
        _raise(lib().mlp_solution_var_value(self._h, int(var), C.byref(out)))
        return out.value

    __getitem__ = var_value

    def values(self):
        a = np.zeros(self.num_vars, dtype=np.float64)
        _raise(lib().mlp_solution_values(self._h, _p(a, C.c_double), len(a)))
        return a

    def __iter__(self):  # lib.rs:350 iter()
        return iter(enumerate(self.values()))

    def _report(self, fn, struct):
        """The struct a read fills in, as a dict."""
        r = struct()
        _raise(fn(self._h, C.byref(r)))
        return {n: getattr(r, n) for n, _ in struct._fields_}

    # ---- dual values, reduced costs, KKT certificate (include/minilp_hip.h: mlp_solution_dual_values ...; user's objective sense)
    @property
    def num_constraints(self):
        """Constraints of the model: Problem.add_constraint order, then Solution.add_constraint / add_gomory_cut in call order."""
        return lib().mlp_solution_num_constraints(self._h)

    def dual_values(self):
        """pi = B^-T c_B by constraint: d objective() / d rhs_c at the current basis (0.0 where the slack is basic)."""
        a = np.zeros(self.num_constraints, dtype=np.float64)
        _raise(lib().mlp_solution_dual_values(self._h, _p(a, C.c_double), len(a)))
        return a

    def dual_value(self, c):
        out = C.c_double()
        _raise(lib().mlp_solution_dual_value(self._h, int(c), C.byref(out)))
        return out.value

    def reduced_costs(self):
        """r_j = c_j - a_j . pi by variable (0.0 for a basic variable)."""
        a = np.zeros(self.num_vars, dtype=np.float64)
        _raise(lib().mlp_solution_reduced_costs(self._h, _p(a, C.c_double), len(a)))
        return a

    def reduced_cost(self, var):
        out = C.c_double()
        _raise(lib().mlp_solution_reduced_cost(self._h, int(var), C.byref(out)))
        return out.value

    def certificate(self):
        """KKT certificate of the current point (mlp_certificate) as a dict."""
        return self._report(lib().mlp_solution_certificate, MlpCertificate)

    # ---- basis status, cost / rhs ranging (include/minilp_hip.h: mlp_solution_basis_status ...; definitions there)
    def basis_status(self):
        """(variables, constraints): int32 arrays of MLP_BASIC / MLP_AT_LOWER / MLP_AT_UPPER / MLP_NB_FREE / MLP_NB_FIXED."""
        v = np.zeros(self.num_vars, dtype=np.int32)
        c = np.zeros(self.num_constraints, dtype=np.int32)
        _raise(lib().mlp_solution_basis_status(self._h, _p(v, C.c_int32), len(v), _p(c, C.c_int32), len(c)))
        return v, c

    def _ranging(self, fn, which, n_all, ctype, dtype):
        if which is None:
            n, ptr = n_all, None
        else:
            w = np.ascontiguousarray(which, dtype=np.int64).reshape(-1)
            if len(w) and (w.min() < 0 or w.max() > np.iinfo(dtype).max):
                raise InternalError(-1, "ranging: index out of range")
            w = w.astype(dtype)
            n, ptr = len(w), _p(w, ctype)
        lo, hi = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
        _raise(fn(self._h, ptr, n, _p(lo, C.c_double), _p(hi, C.c_double)))
        return lo, hi

    def cost_ranging(self, vars=None):
        """(lo, hi): the range of each objective coefficient (all variables, or the listed ones) over which the current basis stays optimal."""
        return self._ranging(lib().mlp_solution_cost_ranging, vars, self.num_vars, C.c_uint32, np.uint32)

    def rhs_ranging(self, constraints=None):
        """(lo, hi): the range of each right-hand side (all constraints, or the listed ones) over which the current basis stays feasible."""
        return self._ranging(lib().mlp_solution_rhs_ranging, constraints, self.num_constraints, C.c_uint64, np.uint64)

    def ranging_info(self):
        """Counters of the last cost_ranging / rhs_ranging call (mlp_ranging_info) as a dict."""
        return self._report(lib().mlp_solution_ranging_info, MlpRangingInfo)

    # ---- reading the tableau (include/minilp_hip.h: mlp_solution_binv_rows ...; numbering and definitions there): columns are
    #      j < num_vars structural, num_vars + c the slack of constraint c; vectors by row are exchanged by constraint; internal
    #      form A x + s = b, no sign turn for Maximize
    @property
    def num_rows(self):
        """Constraints that have a row (= basis positions)."""
        return lib().mlp_solution_num_rows(self._h)

    def basis_head(self):
        """int64[num_rows]: the column basic at each position."""
        a = np.zeros(self.num_rows, dtype=np.uint64)
        _raise(lib().mlp_solution_basis_head(self._h, _p(a, C.c_uint64), len(a)))
        return a.astype(np.int64)

    @staticmethod
    def _tab_list(which):
        w = np.asarray(which)
        if w.ndim != 1 and w.size:
            raise InternalError(-1, "tableau: the index list must be one-dimensional")
        w = np.ascontiguousarray(w, dtype=np.int64).reshape(-1)
        if len(w) and w.min() < 0:
            raise InternalError(-1, "tableau: index out of range")
        return w.astype(np.uint64)

    def _tab_dense(self, fn, which, row_len):
        w = self._tab_list(which)
        out = np.zeros((len(w), row_len), dtype=np.float64)
        _raise(fn(self._h, _p(w, C.c_uint64), len(w), _p(out, C.c_double), out.size))
        return out

    def binv_rows(self, cols):
        """float64[n, num_constraints]: e_p^T B^-1 by constraint, p the position of each listed basic column."""
        return self._tab_dense(lib().mlp_solution_binv_rows, cols, self.num_constraints)

    def binv_cols(self, constraints):
        """float64[n, num_rows]: B^-1 e_row by position, for each listed constraint."""
        return self._tab_dense(lib().mlp_solution_binv_cols, constraints, self.num_rows)

    def tableau_cols(self, cols):
        """float64[n, num_rows]: B^-1 abar_j by position, for each listed column (a basic one: the unit vector of its position)."""
        return self._tab_dense(lib().mlp_solution_tableau_cols, cols, self.num_rows)

    def tableau_rows(self, cols):
        """CSR (indptr, indices, data) over the column numbering: alpha_p = e_p^T B^-1 [A | I] for each listed basic column, sorted by
        column, exact zeros and the other basic columns dropped, the column's own entry exactly 1.0."""
        w = self._tab_list(cols)
        ip, ix, dv = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_double)()
        _raise(lib().mlp_solution_tableau_rows(self._h, _p(w, C.c_uint64), len(w), C.byref(ip), C.byref(ix), C.byref(dv)))
        indptr = np.ctypeslib.as_array(ip, shape=(len(w) + 1,)).astype(np.int64)  # (copies: the buffers belong to the library)
        nnz = int(indptr[-1])
        if nnz == 0:
            return indptr, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float64)
        return indptr, np.ctypeslib.as_array(ix, shape=(nnz,)).astype(np.int64), np.ctypeslib.as_array(dv, shape=(nnz,)).copy()

    def basis_solve(self, rhs, transpose=False):
        """rhs [n, num_constraints] by constraint -> B^-1 rhs [n, num_rows] by position; transpose=True: rhs [n, num_rows] by position
        -> B^-T rhs [n, num_constraints] by constraint.  A one-dimensional rhs is one right-hand side and gives a one-dimensional result."""
        r = np.ascontiguousarray(rhs, dtype=np.float64)
        one = r.ndim == 1
        if one:
            r = r.reshape(1, -1)
        n_in, n_out = (self.num_rows, self.num_constraints) if transpose else (self.num_constraints, self.num_rows)
        if r.ndim != 2 or r.shape[1] != n_in:
            raise InternalError(-1, f"basis_solve: rhs must be [n, {n_in}]")
        out = np.zeros((r.shape[0], n_out), dtype=np.float64)
        _raise(lib().mlp_solution_basis_solve(self._h, 1 if transpose else 0, _p(r, C.c_double), r.size, r.shape[0], _p(out, C.c_double),
                                              out.size))
        return out[0] if one else out

    def tableau_info(self):
        """Counters of the last tableau call (mlp_tableau_info) as a dict."""
        return self._report(lib().mlp_solution_tableau_info, MlpTableauInfo)

    def add_constraint(self, expr, cmp_op, rhs):
        idx, val = _terms(expr)
        h = self._take()
        _raise(lib().mlp_solution_add_constraint(C.byref(h), _p(idx, C.c_uint32), _p(val, C.c_double), len(idx), cmp_op, rhs))
        return Solution(h)

    def fix_var(self, var, val):
        h = self._take()
        _raise(lib().mlp_solution_fix_var(C.byref(h), int(var), val))
        return Solution(h)

    def unfix_var(self, var):
        h = self._take()
        was = C.c_int()
        _raise(lib().mlp_solution_unfix_var(C.byref(h), int(var), C.byref(was)))
        return Solution(h), bool(was.value)

    def add_gomory_cut(self, var):
        h = self._take()
        _raise(lib().mlp_solution_add_gomory_cut(C.byref(h), int(var)))
        return Solution(h)

    # ---- a round of cuts in one call (include/minilp_hip.h: mlp_solution_add_constraints_csr ...; semantics there)
    def add_constraints_csr(self, indptr, indices, data, cmp_ops, rhs):
        """m x add_constraint in one call (rows in CSR form): all rows appended, feasibility restored once."""
        ip = np.ascontiguousarray(indptr, dtype=np.uint64)
        ix = np.ascontiguousarray(indices, dtype=np.uint32)
        dv = np.ascontiguousarray(data, dtype=np.float64)
        ops = np.ascontiguousarray(cmp_ops, dtype=np.int32)
        rh = np.ascontiguousarray(rhs, dtype=np.float64)
        if len(ip) != len(rh) + 1 or len(ops) != len(rh) or len(ix) != len(dv) or (len(rh) and int(ip[-1]) != len(ix)):
            raise InternalError(-1, "add_constraints_csr: array lengths do not fit")
        h = self._take()
        _raise(lib().mlp_solution_add_constraints_csr(C.byref(h), len(rh), _p(ip, C.c_uint64), _p(ix, C.c_uint32), _p(dv, C.c_double),
                                                      _p(ops, C.c_int32), _p(rh, C.c_double)))
        return Solution(h)

    def add_constraints(self, rows):
        """add_constraint for every (expr, cmp_op, rhs) of `rows`, in one call."""
        ip, ix, dv, ops, rh = [0], [], [], [], []
        for expr, cmp_op, rhs in rows:
            idx, val = _terms(expr)
            ix.extend(int(i) for i in idx)
            dv.extend(float(v) for v in val)
            ip.append(len(ix))
            ops.append(int(cmp_op))
            rh.append(float(rhs))
        return self.add_constraints_csr(ip, ix, dv, ops, rh)

    def add_gomory_cuts(self, vars):
        """One round of Gomory cuts, one per listed basic variable, all from the current basis; feasibility restored once."""
        v = self._var_list(vars, "add_gomory_cuts")
        h = self._take()
        _raise(lib().mlp_solution_add_gomory_cuts(C.byref(h), _p(v, C.c_uint32), len(v)))
        return Solution(h)

    @staticmethod
    def _int_mask(marks, n):
        """uint8 mask from a bool mask (taken as it is, whatever its length: the library checks it) or a list of indices < n."""
        a = np.asarray(marks)
        if a.dtype == np.bool_:
            return np.ascontiguousarray(a, dtype=np.uint8).ravel()
        idx = a.astype(np.int64).ravel()
        if len(idx) and (idx.min() < 0 or idx.max() >= n):
            raise InternalError(-1, "add_gmi_cuts: integer mark out of range")
        m = np.zeros(n, dtype=np.uint8)
        m[idx] = 1
        return m

    @staticmethod
    def _mask_args(mask, n_without=0):
        """(pointer, length) of an optional uint8 mask; None: a NULL pointer and n_without."""
        return (None, n_without) if mask is None else (_p(mask, C.c_uint8), len(mask))

    def add_gmi_cuts(self, vars, integer_vars, integer_constraints=None, away=0.01):
        """One round of Gomory mixed-integer cuts (mlp_solution_add_gmi_cuts; semantics in the header), one per listed basic integer
        variable, all from the current basis; feasibility restored once.  integer_vars / integer_constraints: a bool mask or a list of
        indices (constraints: the slacks that are integer; None: all slacks continuous).  Returns (Solution, status): status[i] is 0
        emitted, 1 skipped (fraction within away), 2 skipped (free non-basic column in the row)."""
        v = self._var_list(vars, "add_gmi_cuts")
        vm = self._int_mask(integer_vars, self.num_vars)
        cm = None if integer_constraints is None else self._int_mask(integer_constraints, self.num_constraints)
        status = np.zeros(len(v), dtype=np.int32)
        h = self._take()
        _raise(lib().mlp_solution_add_gmi_cuts(C.byref(h), _p(v, C.c_uint32), len(v), _p(vm, C.c_uint8), len(vm), *self._mask_args(cm), float(away),
                                               _p(status, C.c_int32)))
        return Solution(h), status

    def gmi_info(self):
        """Counters of the last add_gmi_cuts call (mlp_gmi_info) as a dict."""
        return self._report(lib().mlp_solution_gmi_info, MlpGmiInfo)

    # ---- branching penalties (include/minilp_hip.h: mlp_solution_branch_penalties; definitions there)
    def branch_penalties(self, vars, integer_vars=None, integer_constraints=None):
        """One-pivot (Driebeek-Tomlin) bounds on the objective degradation of the down and the up branch of every listed structural
        variable, from the current basis.  Returns a dict of arrays: down, up (non-negative, inf: the branch is infeasible), down_col,
        up_col (the column that would enter; -1: none), frac, status (0 basic and fractional, 1 non-basic or integral: zeros).
        integer_vars / integer_constraints: a bool mask or a list of indices, as for add_gmi_cuts; they switch Tomlin's strengthening on
        (the numbers then bound the integer descendants of the branch, not the child LP).  A read: the solution is left as it is."""
        v = self._var_list(vars, "branch_penalties")
        if integer_vars is None and integer_constraints is not None:
            raise InternalError(-1, "branch_penalties: integer_constraints needs integer_vars")
        vm = None if integer_vars is None else self._int_mask(integer_vars, self.num_vars)
        cm = None if integer_constraints is None else self._int_mask(integer_constraints, self.num_constraints)
        n = len(v)
        out = dict(down=np.zeros(n), up=np.zeros(n), down_col=np.zeros(n, dtype=np.int64), up_col=np.zeros(n, dtype=np.int64),
                   frac=np.zeros(n), status=np.zeros(n, dtype=np.int32))
        _raise(lib().mlp_solution_branch_penalties(self._h, _p(v, C.c_uint32), n, *self._mask_args(vm), *self._mask_args(cm),
                                                   _p(out["down"], C.c_double), _p(out["up"], C.c_double),
                                                   _p(out["down_col"], C.c_int64), _p(out["up_col"], C.c_int64),
                                                   _p(out["frac"], C.c_double), _p(out["status"], C.c_int32)))
        return out

    def branch_info(self):
        """Counters of the last branch_penalties call (mlp_branch_info) as a dict."""
        return self._report(lib().mlp_solution_branch_info, MlpBranchInfo)

    # ---- reduced-cost bounds from a cutoff, batched fixing (include/minilp_hip.h: mlp_solution_cutoff_bounds ...; semantics there)
    def cutoff_bounds(self, cutoff, integer_vars=None):
        """Bounds that the reduced costs and the objective value `cutoff` of an incumbent imply.  Returns (vars, lo, hi, pruned): the
        structural variables whose bound tightens, ascending, each with both of its bounds; lo == hi: the variable can be fixed.
        pruned: this LP is already worse than the cutoff (the arrays are empty).  integer_vars: a bool mask or a list of indices; the
        bound of a marked variable is rounded to whole steps.  A read on a solved model: the solution is left as it is."""
        n = self.num_vars
        vm = None if integer_vars is None else self._int_mask(integer_vars, n)
        v, lo, hi = np.zeros(n, dtype=np.uint32), np.zeros(n), np.zeros(n)
        count, pruned = C.c_uint64(), C.c_int()
        _raise(lib().mlp_solution_cutoff_bounds(self._h, float(cutoff), *self._mask_args(vm, n), _p(v, C.c_uint32), _p(lo, C.c_double), _p(hi, C.c_double), n,
                                                C.byref(count), C.byref(pruned)))
        k = int(count.value)
        return v[:k].copy(), lo[:k].copy(), hi[:k].copy(), bool(pruned.value)

    @staticmethod
    def _var_list(vars, who):
        v = np.ascontiguousarray(list(vars), dtype=np.int64).reshape(-1)
        if len(v) and (v.min() < 0 or v.max() > 0xFFFFFFFF):
            raise InternalError(-1, who + ": variable out of range")
        return v.astype(np.uint32)

    def fix_vars(self, vars, vals):
        """fix_var(vars[i], vals[i]) for every i in one call: the non-basic requests share one FTRAN (none when every variable already
        sits at its value), the basic ones take one forced pivot each, feasibility is restored once."""
        v = self._var_list(vars, "fix_vars")
        x = np.ascontiguousarray(list(vals), dtype=np.float64).reshape(-1)
        if len(x) != len(v):
            raise InternalError(-1, "fix_vars: vars and vals differ in length")
        h = self._take()
        _raise(lib().mlp_solution_fix_vars(C.byref(h), _p(v, C.c_uint32), _p(x, C.c_double), len(v)))
        return Solution(h)

    def unfix_vars(self, vars):
        """unfix_var for every listed variable with one re-solve.  Returns (Solution, released count)."""
        v = self._var_list(vars, "unfix_vars")
        h = self._take()
        k = C.c_uint64()
        _raise(lib().mlp_solution_unfix_vars(C.byref(h), _p(v, C.c_uint32), len(v), C.byref(k)))
        return Solution(h), int(k.value)

    def fix_by_reduced_cost(self, cutoff, integer_vars=None):
        """cutoff_bounds, then fix_vars on the entries with lo == hi.  Returns (Solution, fixed variables); a pruned LP fixes nothing."""
        v, lo, hi, _ = self.cutoff_bounds(cutoff, integer_vars)
        sel = lo == hi
        return self.fix_vars(v[sel], lo[sel]), v[sel]

    def fix_info(self):
        """Counters of the last cutoff_bounds / fix_vars / unfix_vars call (mlp_fix_info) as a dict."""
        return self._report(lib().mlp_solution_fix_info, MlpFixInfo)

    # ---- new bounds for structural variables (include/minilp_hip.h: mlp_solution_set_var_bounds ...; semantics there)
    def set_var_bounds(self, vars, lo, hi):
        """New bounds [lo[i], hi[i]] for the listed structural variables of a solved model, then one dual re-solve from the current
        basis (none when nothing moves).  A non-basic variable keeps its side and moves with its bound; making that bound infinite is
        refused.  lo > hi raises Infeasible."""
        v = self._var_list(vars, "set_var_bounds")
        a = np.ascontiguousarray(list(lo), dtype=np.float64).reshape(-1)
        b = np.ascontiguousarray(list(hi), dtype=np.float64).reshape(-1)
        if len(a) != len(v) or len(b) != len(v):
            raise InternalError(-1, "set_var_bounds: vars, lo and hi differ in length")
        h = self._take()
        _raise(lib().mlp_solution_set_var_bounds(C.byref(h), _p(v, C.c_uint32), _p(a, C.c_double), _p(b, C.c_double), len(v)))
        return Solution(h)

    def tighten_by_reduced_cost(self, cutoff, integer_vars=None):
        """cutoff_bounds with every entry applied to the bounds on the device.  Returns (Solution, count, pruned); values and objective
        keep their bits, and a pruned LP is left as it is."""
        n = self.num_vars
        vm = None if integer_vars is None else self._int_mask(integer_vars, n)
        h = self._take()
        count, pruned = C.c_uint64(), C.c_int()
        _raise(lib().mlp_solution_tighten_by_reduced_cost(C.byref(h), float(cutoff), *self._mask_args(vm, n), C.byref(count), C.byref(pruned)))
        return Solution(h), int(count.value), bool(pruned.value)

    def var_bounds(self, vars=None):
        """(lo, hi) of the listed structural variables as the solution holds them now; vars=None: all of them."""
        v = None if vars is None else self._var_list(vars, "var_bounds")
        n = self.num_vars if v is None else len(v)
        lo, hi = np.zeros(n), np.zeros(n)
        _raise(lib().mlp_solution_var_bounds(self._h, None if v is None else _p(v, C.c_uint32), n, _p(lo, C.c_double), _p(hi, C.c_double)))
        return lo, hi

    def bounds_info(self):
        """Counters of the last set_var_bounds / tighten_by_reduced_cost call (mlp_bounds_info) as a dict."""
        return self._report(lib().mlp_solution_bounds_info, MlpBoundsInfo)

    # ---- bound propagation from row activities (include/minilp_hip.h: mlp_solution_propagate_bounds ...; semantics there)
    def propagate_bounds(self, integer_vars=None, max_rounds=10):
        """Bounds that the rows of the model imply on its structural variables, given the bounds and fixings it holds now (node
        presolve).  Returns (vars, lo, hi, infeasible): the variables whose bounds tighten, ascending, each with both bounds;
        lo == hi: the variable can be fixed.  infeasible: the rounds prove that the model has no solution (the arrays are empty).
        integer_vars: a bool mask or a list of indices; the bounds of a marked variable are rounded inwards.  A read that works on any
        state, a budget-limited solve included: the solution is left as it is."""
        n = self.num_vars
        vm = None if integer_vars is None else self._int_mask(integer_vars, n)
        v, lo, hi = np.zeros(n, dtype=np.uint32), np.zeros(n), np.zeros(n)
        count, infeasible = C.c_uint64(), C.c_int()
        _raise(lib().mlp_solution_propagate_bounds(self._h, *self._mask_args(vm, n), int(max_rounds), _p(v, C.c_uint32), _p(lo, C.c_double), _p(hi, C.c_double), n,
                                                   C.byref(count), C.byref(infeasible)))
        k = int(count.value)
        return v[:k].copy(), lo[:k].copy(), hi[:k].copy(), bool(infeasible.value)

    def tighten_by_propagation(self, integer_vars=None, max_rounds=10):
        """propagate_bounds with the whole list applied through set_var_bounds (one dual re-solve at most).  Returns (Solution, count,
        infeasible); infeasible leaves the solution as it is.  Needs a solved model."""
        n = self.num_vars
        vm = None if integer_vars is None else self._int_mask(integer_vars, n)
        h = self._take()
        count, infeasible = C.c_uint64(), C.c_int()
        _raise(lib().mlp_solution_tighten_by_propagation(C.byref(h), *self._mask_args(vm, n), int(max_rounds), C.byref(count), C.byref(infeasible)))
        return Solution(h), int(count.value), bool(infeasible.value)

    def propagate_info(self):
        """Counters of the last propagate_bounds / tighten_by_propagation call (mlp_propagate_info) as a dict."""
        return self._report(lib().mlp_solution_propagate_info, MlpPropagateInfo)

    # ---- new right-hand sides and the batched what-if read (include/minilp_hip.h: mlp_solution_set_rhs ...; semantics there)
    @staticmethod
    def _cons_list(constraints, who):
        c = np.ascontiguousarray(list(constraints), dtype=np.int64).reshape(-1)
        if len(c) and c.min() < 0:
            raise InternalError(-1, who + ": constraint out of range")
        return c.astype(np.uint64)

    def set_rhs(self, constraints, rhs):
        """New right-hand sides rhs[i] for the listed constraints of a solved model (numbering of num_constraints, the user's terms),
        then one dual re-solve from the current basis (none when every basic value stays within its bounds).  Raises Infeasible when
        the changed model has no solution.  Like every mutator it consumes the receiver, also when the library refuses the call; only
        what the binding itself refuses before the call (a negative index, lists of different lengths) leaves the receiver usable."""
        c = self._cons_list(constraints, "set_rhs")
        b = np.ascontiguousarray(list(rhs), dtype=np.float64).reshape(-1)
        if len(b) != len(c):
            raise InternalError(-1, "set_rhs: constraints and rhs differ in length")
        h = self._take()
        _raise(lib().mlp_solution_set_rhs(C.byref(h), _p(c, C.c_uint64), _p(b, C.c_double), len(c)))
        return Solution(h)

    def constraint_rhs(self, constraints=None):
        """The right-hand sides of the listed constraints as the solution holds them now; constraints=None: all of them."""
        c = None if constraints is None else self._cons_list(constraints, "constraint_rhs")
        n = self.num_constraints if c is None else len(c)
        out = np.zeros(n, dtype=np.float64)
        _raise(lib().mlp_solution_constraint_rhs(self._h, None if c is None else _p(c, C.c_uint64), n, _p(out, C.c_double)))
        return out

    def rhs_scenarios(self, constraints, rhs):
        """S candidate right-hand sides against the current basis, 16 per batch on the device: rhs is float64 [S, n], scenario s gives
        constraints[i] the right-hand side rhs[s, i].  Returns a dict of arrays of length S: bound (the objective the scenario's basis
        would report: its optimum where feasible, else a bound from the dual side), feasible (bool: set_rhs of the scenario would run no
        pivot), worst (the largest bound violation of a basic value, 0.0 when feasible), worst_col (the column basic there, numbering of
        basis_head; -1 when feasible).  The solution is left as it is."""
        c = self._cons_list(constraints, "rhs_scenarios")
        r = np.ascontiguousarray(rhs, dtype=np.float64)
        if r.ndim != 2 or r.shape[1] != len(c):
            raise InternalError(-1, f"rhs_scenarios: rhs must be [S, {len(c)}]")
        S = r.shape[0]
        bound, worst = np.zeros(S, dtype=np.float64), np.zeros(S, dtype=np.float64)
        feasible, worst_col = np.zeros(S, dtype=np.uint8), np.zeros(S, dtype=np.int64)
        _raise(lib().mlp_solution_rhs_scenarios(self._h, _p(c, C.c_uint64), len(c), _p(r, C.c_double), S, _p(bound, C.c_double),
                                                _p(feasible, C.c_uint8), _p(worst, C.c_double), _p(worst_col, C.c_int64)))
        return {"bound": bound, "feasible": feasible.astype(bool), "worst": worst, "worst_col": worst_col}

    def rhs_info(self):
        """Counters of the last set_rhs / rhs_scenarios call (mlp_rhs_info) as a dict."""
        return self._report(lib().mlp_solution_rhs_info, MlpRhsInfo)

    def cut_info(self):
        """Counters of the last add_constraints / add_constraints_csr / add_gomory_cuts call (mlp_cut_info) as a dict."""
        return self._report(lib().mlp_solution_cut_info, MlpCutInfo)

    def save_basis(self, mode=2):
        """Basis checkpoint as bytes (include/minilp_hip.h): 0 sets + flags + x_N, 1 + f32 weights, 2 full f64 state."""
        n = lib().mlp_solution_save_basis(self._h, int(mode), None, 0)
        if n == 0:
            raise InternalError(-1, lib().mlp_last_error().decode())
        buf = (C.c_char * n)()
        if lib().mlp_solution_save_basis(self._h, int(mode), C.cast(buf, C.c_void_p), n) != n:
            raise InternalError(-1, lib().mlp_last_error().decode())
        return bytes(buf)

    def set_sampling(self, every_iteration):
        """True: every iteration is an eager, event-bracketed one; False: default cadence; None: sampling off for good."""
        _raise(lib().mlp_solution_set_sampling(self._h, -1 if every_iteration is None else (1 if every_iteration else 0)))

    # --- engine-level controls (fixed pivot budget, stats, trace)
    def continue_solve(self, budget):
        _raise(lib().mlp_solution_continue(self._h, budget))

    @property
    def budget_exhausted(self):
        return bool(lib().mlp_solution_budget_exhausted(self._h))

    def enable_sharding(self, rank, world, shm_name):
        """Column-block sharding of the pricing path (include/minilp_hip.h); see minilp_amd.dist."""
        _raise(lib().mlp_solution_enable_sharding(self._h, int(rank), int(world), shm_name.encode()))

    def enable_sharding_ex(self, rank, world, shm_name, transport, rccl_id=None):
        """enable_sharding with the transport named: "peer", "host", "rccl" (rccl_id: rank 0's 128-byte id) or "pump"."""
        buf = (C.c_char * 128).from_buffer_copy(bytes(rccl_id)) if rccl_id else None
        _raise(lib().mlp_solution_enable_sharding_ex(self._h, int(rank), int(world), shm_name.encode(), transport.encode(),
                                                      C.cast(buf, C.c_void_p) if buf is not None else None))

    def transport(self):
        return lib().mlp_solution_transport(self._h).decode()

    # ---- engine-level stepping (include/minilp_hip.h: mlp_engine_open / mlp_engine_stage)
    def engine_open(self):
        """Pricing decision of the phase initial_solve would run next; returns (status, info dict)."""
        info = MlpIterInfo()
        st = lib().mlp_engine_open(self._h, C.byref(info))
        if st < 0:
            _raise(st)
        return st, {n: getattr(info, n) for n, _ in MlpIterInfo._fields_}

    def engine_stage(self, stage):
        """One stage (STAGE_*) of the open iteration; returns (status, info dict)."""
        info = MlpIterInfo()
        st = lib().mlp_engine_stage(self._h, int(stage), C.byref(info))
        if st < 0:
            _raise(st)
        return st, {n: getattr(info, n) for n, _ in MlpIterInfo._fields_}

    def reinvert(self):
        d = C.c_double()
        _raise(lib().mlp_solution_reinvert(self._h, C.byref(d)))
        return d.value

    def recompute_basic_values(self):
        """x_B = B^-1 (b - N x_N) from the basis, two refinement steps (solver.rs:1177-1197)."""
        _raise(lib().mlp_solution_recompute_basic_values(self._h))

    def stats(self):
        s = MlpStats()
        lib().mlp_solution_stats(self._h, C.byref(s))
        d = {n: getattr(s, n) for n, _ in MlpStats._fields_}
        d["kase"] = list(d["kase"])
        rl = self.state("ratio_list")  # counters of the control block, not of mlp_stats (whose layout stays as it is)
        d["ratio_list_decisions"], d["ratio_list_overflows"] = int(rl[1]), int(rl[2])
        return d

    def reset_stats(self):
        lib().mlp_solution_reset_stats(self._h)

    def trace(self):
        n = lib().mlp_solution_trace_len(self._h)
        out = []
        ph, col, row, ev, lv = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        pc, ob = C.c_double(), C.c_double()
        for i in range(n):
            lib().mlp_solution_trace_get(self._h, i, C.byref(ph), C.byref(col), C.byref(row), C.byref(ev), C.byref(lv),
                                         C.byref(pc), C.byref(ob))
            out.append((ph.value, col.value, row.value, ev.value, lv.value, pc.value, ob.value))
        return out

    def state(self, what):
        n = lib().mlp_solution_state(self._h, what.encode(), None, 0)
        if n == 2 ** 64 - 1:
            raise KeyError(what)
        a = np.zeros(n, dtype=np.float64)
        lib().mlp_solution_state(self._h, what.encode(), _p(a, C.c_double), n)
        return a


class MpsFile:
    """mps.rs:7-16; MpsFile.parse(text, direction) mirrors MpsFile::parse (mps.rs:39)."""

    def __init__(self, text, direction):
        if isinstance(text, str):
            text = text.encode()
        h = C.c_void_p()
        st = lib().mlp_mps_parse(text, len(text), int(direction), C.byref(h))
        if st != 0:
            raise ValueError(lib().mlp_last_error().decode())  # io::ErrorKind::InvalidData
        self._h = h
        self.problem_name = lib().mlp_mps_name(h).decode()
        n = lib().mlp_mps_num_vars(h)
        self.variables = {lib().mlp_mps_var_name(h, i).decode(): i for i in range(n)}
        self.problem = Problem(direction, lib().mlp_mps_problem(h))

    parse = classmethod(lambda cls, text, direction: cls(text, direction))

    def __del__(self):
        if getattr(self, "_h", None):
            lib().mlp_mps_free(self._h)
