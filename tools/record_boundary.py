"""Records what every mlp_solution_* entry point of DESIGN.md §7.1 - §7.9 answers at the C boundary (include/minilp_hip.h), called through
ctypes directly so that NULL pointers can be passed: in three states of two small instances — solved, not solved (a pivot budget of 3),
a one-rank pump — each entry point is called with valid arguments, with n == 0 and with one fault at a time (NULL list, NULL output,
index out of range, index listed twice, wrong num_vars, max_rounds 0 and 65, NaN cutoff, away 0, cap below the count, lo > hi, NULL
handle).  Per call: the status, the text of mlp_last_error() when the status is negative, whether a mutator set the handle to NULL, the
small integer outputs, and — while the handle lives — the integer fields and `bytes` of all eight report structs and the 16 hex digits of
the objective.

    python tools/record_boundary.py [OUT.json]        (default: tests/golden/boundary_parent.json)

The committed file is the output of the commit BEFORE the boundary was consolidated;
tests/test_boundary_golden.py replays `record_case()` on the current tree and asserts equality of every field."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import minilp_amd as M                                                                   # noqa: E402
from minilp_amd import api, dist, lpgen                                                  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "boundary_parent.json")
INSTANCES = {"cover": (lpgen.gen_cover_lp, (70, 90, 5, 5)),                              # Minimize; tools/record_bound_moves.py's
             "sparse-maximize": (lpgen.gen_sparse_lp, (60, 45, 6, 7))}                   # Maximize (the sign of the cutoff gap), smaller
STATES = ("solved", "not-solved", "pump")
CASES = tuple("%s/%s" % (i, s) for i in INSTANCES for s in STATES)
REPORTS = (("ranging", api.MlpRangingInfo), ("cut", api.MlpCutInfo), ("tableau", api.MlpTableauInfo), ("gmi", api.MlpGmiInfo),
           ("branch", api.MlpBranchInfo), ("fix", api.MlpFixInfo), ("bounds", api.MlpBoundsInfo), ("propagate", api.MlpPropagateInfo))
TIMES = ("device_ms", "wall_ms")                                                         # left out: they differ from run to run
NULL_HANDLE = "NULL handle"

u8, u32, u64, i32, i64, f64 = C.c_uint8, C.c_uint32, C.c_uint64, C.c_int32, C.c_int64, C.c_double


def _a(values, ctype):
    return np.ascontiguousarray(values, dtype=np.dtype(ctype))


def _p(a, ctype):
    return None if a is None else a.ctypes.data_as(C.POINTER(ctype))


def _hex(x):
    return np.float64(x).tobytes().hex()


class _State:
    """Fresh handles of one state of one instance, and the lists the valid calls use (taken from the solved model)."""

    def __init__(self, instance, state):
        gen, args = INSTANCES[instance]
        self.lp, self.state, self.L, self.boxes = gen(*args), state, M.lib(), []
        self.prob = lpgen.build_problem(M.Problem, self.lp)
        self.base = self.prob.solve()
        s = self.base
        self.nv, self.nc, self.nr = s.num_vars, s.num_constraints, s.num_rows
        self.x, self.obj, head = s.values(), s.objective(), [int(j) for j in s.basis_head()]
        self.lo, self.hi = s.var_bounds()
        self.basic = [j for j in head if j < self.nv and self.x[j] > 1e-3][:3]
        self.nonbasic = [j for j in range(self.nv) if j not in head][:3]
        assert len(self.basic) == 3 and len(self.nonbasic) == 3, (instance, self.basic, self.nonbasic)
        better = -1.0 if self.lp["direction"] == M.MAXIMIZE else 1.0                    # a cutoff the node beats / one that prunes it
        self.cutoff, self.cutoff_pruning = self.obj + better, self.obj - better

    def fresh(self):
        if self.state == "solved":
            return self.base.clone()._take().value
        s = self.prob.solve(budget=3) if self.state == "not-solved" else self.prob.solve()
        if self.state == "not-solved":
            assert s.budget_exhausted
        else:
            self.boxes.append(dist.create_mailbox(1))
            s.enable_sharding_ex(0, 1, self.boxes[-1], "pump")
        return s._take().value

    def close(self):
        for b in self.boxes:
            dist.remove_mailbox(b)


def _entries(S):
    """[(entry point, 'm' mutator | 'r' read, [(label, call)])]: call(h) -> (status, {output: int}); h is what goes in the handle's place."""
    L, nv, nc, nr, x = S.L, S.nv, S.nc, S.nr, S.x
    B, NB = S.basic, S.nonbasic
    ones, cons0 = _a(np.ones(nv), u8), _a(np.zeros(nc), u8)
    E = []

    def outs(**kw):
        return {k: int(v.value) for k, v in kw.items()}

    # ---- §7.1
    def vec_read(fn, n, ctype=f64):
        def call(h, n_=n, null=False):
            buf = _a(np.zeros(n_ + 1), ctype)
            return fn(h, None if null else _p(buf, ctype), n_), {}
        return [("valid", call), ("NULL output", lambda h: call(h, null=True)), ("wrong length", lambda h: call(h, n + 1)), (NULL_HANDLE, call)]

    def one_read(fn, n):
        def call(h, i=0, null=False):
            out = f64()
            return fn(h, i, None if null else C.byref(out)), {}
        return [("valid", call), ("index out of range", lambda h: call(h, n)), ("NULL output", lambda h: call(h, null=True)), (NULL_HANDLE, call)]

    E.append(("dual_values", "r", vec_read(L.mlp_solution_dual_values, nc)))
    E.append(("dual_value", "r", one_read(L.mlp_solution_dual_value, nc)))
    E.append(("reduced_costs", "r", vec_read(L.mlp_solution_reduced_costs, nv)))
    E.append(("reduced_cost", "r", one_read(L.mlp_solution_reduced_cost, nv)))

    def certificate(h, null=False):
        c = api.MlpCertificate()
        return L.mlp_solution_certificate(h, None if null else C.byref(c)), {}
    E.append(("certificate", "r", [("valid", certificate), ("NULL output", lambda h: certificate(h, True)), (NULL_HANDLE, certificate)]))

    # ---- §7.2
    def basis_status(h, n=nv, null=False):
        v, c = _a(np.zeros(nv + 1), i32), _a(np.zeros(nc + 1), i32)
        return L.mlp_solution_basis_status(h, None if null else _p(v, i32), n, _p(c, i32), nc), {}
    E.append(("basis_status", "r", [("valid", basis_status), ("NULL output", lambda h: basis_status(h, null=True)),
                                    ("wrong num_vars", lambda h: basis_status(h, nv + 1)), (NULL_HANDLE, basis_status)]))

    def ranging(fn, ctype, n_all):
        def call(h, which=(0, 1, 2), n=None, null=False):
            w = None if which is None else _a(which, ctype)
            n = len(which) if n is None else n
            lo, hi = _a(np.zeros(max(n, 1)), f64), _a(np.zeros(max(n, 1)), f64)
            return fn(h, _p(w, ctype), n, None if null else _p(lo, f64), _p(hi, f64)), {}
        return [("valid", call), ("n == 0", lambda h: call(h, (0,), 0)), ("valid, no list", lambda h: call(h, None, n_all)),
                ("NULL list", lambda h: call(h, None, 3)), ("NULL output", lambda h: call(h, null=True)),
                ("index out of range", lambda h: call(h, (0, n_all))), ("index listed twice", lambda h: call(h, (1, 1))), (NULL_HANDLE, call)]
    E.append(("cost_ranging", "r", ranging(L.mlp_solution_cost_ranging, u32, nv)))
    E.append(("rhs_ranging", "r", ranging(L.mlp_solution_rhs_ranging, u64, nc)))

    # ---- §7.3 (and the single forms)
    def rows_csr(h, rows=((((B[0], 1.0), (B[1], 1.0)), M.LE, 1e9), (((B[2], 1.0),), M.LE, 0.5 * x[B[2]])), null=None):
        ip, ix, dv = [0], [], []
        for terms, _, _ in rows:
            ix += [t[0] for t in terms]
            dv += [t[1] for t in terms]
            ip.append(len(ix))
        a = dict(ip=_a(ip, u64), ix=_a(ix + [0], u32), dv=_a(dv + [0.0], f64), ops=_a([r[1] for r in rows] + [0], i32), rhs=_a([r[2] for r in rows] + [0.0], f64))
        if null:
            a[null] = None
        return L.mlp_solution_add_constraints_csr(h, len(rows), _p(a["ip"], u64), _p(a["ix"], u32), _p(a["dv"], f64), _p(a["ops"], i32), _p(a["rhs"], f64)), {}
    E.append(("add_constraints_csr", "m", [
        ("valid", rows_csr), ("n == 0", lambda h: rows_csr(h, ())), ("NULL list", lambda h: rows_csr(h, null="ip")),
        ("NULL variables", lambda h: rows_csr(h, null="ix")), ("index out of range", lambda h: rows_csr(h, ((((0, 1.0), (nv, 1.0)), M.LE, 1e9),))),
        ("index listed twice", lambda h: rows_csr(h, ((((1, 1.0), (1, 1.0)), M.LE, 1e9),))), (NULL_HANDLE, rows_csr)]))

    def add_constraint(h, terms=((B[0], 1.0), (B[1], 1.0)), rhs=None):
        ix, dv = _a([t[0] for t in terms], u32), _a([t[1] for t in terms], f64)
        return L.mlp_solution_add_constraint(h, _p(ix, u32), _p(dv, f64), len(terms), M.LE, 0.5 * (x[B[0]] + x[B[1]]) if rhs is None else rhs), {}
    E.append(("add_constraint", "m", [("valid", add_constraint), ("index out of range", lambda h: add_constraint(h, ((0, 1.0), (nv, 1.0)))),
                                      ("index listed twice", lambda h: add_constraint(h, ((1, 1.0), (1, 1.0)))), (NULL_HANDLE, add_constraint)]))

    def fix_var(h, j=NB[0]):
        return L.mlp_solution_fix_var(h, j, float(x[min(j, nv - 1)])), {}
    E.append(("fix_var", "m", [("valid", fix_var), ("index out of range", lambda h: fix_var(h, nv)), (NULL_HANDLE, fix_var)]))

    def unfix_var(h, j=NB[0]):
        was = C.c_int(-7)
        return L.mlp_solution_unfix_var(h, j, C.byref(was)), outs(was_fixed=was)
    E.append(("unfix_var", "m", [("setup: fix_var", fix_var), ("valid", unfix_var), ("valid, not fixed", lambda h: unfix_var(h, NB[1])),
                                 ("index out of range", lambda h: unfix_var(h, nv)), (NULL_HANDLE, unfix_var)]))

    def gomory_cut(h, j=B[0]):
        return L.mlp_solution_add_gomory_cut(h, j), {}
    E.append(("add_gomory_cut", "m", [("valid", gomory_cut), ("index out of range", lambda h: gomory_cut(h, nv)), (NULL_HANDLE, gomory_cut)]))

    def var_list(fn, valid):
        """The calls of a mutator whose arguments are (handle, uint32 list, n): fn(h, pointer, n)."""
        def call(h, which=valid, n=None, null=False):
            w = _a(list(which) + [0], u32)
            return fn(h, None if null else _p(w, u32), len(which) if n is None else n)
        return [("valid", call), ("n == 0", lambda h: call(h, ())), ("NULL list", lambda h: call(h, null=True)),
                ("index out of range", lambda h: call(h, (valid[0], nv))), ("index listed twice", lambda h: call(h, (valid[1], valid[1]))),
                (NULL_HANDLE, call)]
    E.append(("add_gomory_cuts", "m", var_list(lambda h, p, n: (L.mlp_solution_add_gomory_cuts(h, p, n), {}), B[:2])))

    # ---- §7.4
    def basis_head(h, n=nr, null=False):
        a = _a(np.zeros(nr + 1), u64)
        return L.mlp_solution_basis_head(h, None if null else _p(a, u64), n), {}
    E.append(("basis_head", "r", [("valid", basis_head), ("NULL output", lambda h: basis_head(h, null=True)),
                                  ("wrong length", lambda h: basis_head(h, nr + 1)), (NULL_HANDLE, basis_head)]))

    def tab_dense(fn, valid, row_len, n_all):
        def call(h, which=valid, null_list=False, null_out=False, extra=0):
            w, out = _a(list(which) + [0], u64), _a(np.zeros(len(which) * row_len + 1), f64)
            return fn(h, None if null_list else _p(w, u64), len(which), None if null_out else _p(out, f64), len(which) * row_len + extra), {}
        return [("valid", call), ("n == 0", lambda h: call(h, ())), ("NULL list", lambda h: call(h, null_list=True)),
                ("NULL output", lambda h: call(h, null_out=True)), ("index out of range", lambda h: call(h, (valid[0], n_all))),
                ("index listed twice", lambda h: call(h, (valid[1], valid[1]))), ("wrong length", lambda h: call(h, extra=1)), (NULL_HANDLE, call)]
    E.append(("binv_rows", "r", tab_dense(L.mlp_solution_binv_rows, B[:2], nc, nv + nc)))
    E.append(("binv_cols", "r", tab_dense(L.mlp_solution_binv_cols, (0, 1), nr, nc)))
    E.append(("tableau_cols", "r", tab_dense(L.mlp_solution_tableau_cols, (NB[0], B[0]), nr, nv + nc)))

    def tableau_rows(h, which=tuple(B[:2]), null_list=False, null_out=False):
        w = _a(list(which) + [0], u64)
        ip, ix, dv = C.POINTER(u64)(), C.POINTER(u32)(), C.POINTER(f64)()
        st = L.mlp_solution_tableau_rows(h, None if null_list else _p(w, u64), len(which), None if null_out else C.byref(ip), C.byref(ix), C.byref(dv))
        return st, (dict(nnz=int(ip[len(which)])) if st == 0 and len(which) else {})
    E.append(("tableau_rows", "r", [("valid", tableau_rows), ("n == 0", lambda h: tableau_rows(h, ())), ("NULL list", lambda h: tableau_rows(h, null_list=True)),
                                    ("NULL output", lambda h: tableau_rows(h, null_out=True)), ("index out of range", lambda h: tableau_rows(h, (B[0], nv + nc))),
                                    ("index listed twice", lambda h: tableau_rows(h, (B[1], B[1]))), (NULL_HANDLE, tableau_rows)]))

    def basis_solve(h, transpose=0, n=1, null_rhs=False, null_out=False, extra=0):
        n_in, n_out = (nr, nc) if transpose else (nc, nr)
        rhs, out = _a(np.ones(n * n_in + 1), f64), _a(np.zeros(n * n_out + 1), f64)
        return L.mlp_solution_basis_solve(h, transpose, None if null_rhs else _p(rhs, f64), n * n_in + extra, n, None if null_out else _p(out, f64), n * n_out), {}
    E.append(("basis_solve", "r", [("valid", basis_solve), ("valid, transposed", lambda h: basis_solve(h, 1, 2)), ("n == 0", lambda h: basis_solve(h, n=0)),
                                   ("NULL list", lambda h: basis_solve(h, null_rhs=True)), ("NULL output", lambda h: basis_solve(h, null_out=True)),
                                   ("wrong length", lambda h: basis_solve(h, extra=1)), (NULL_HANDLE, basis_solve)]))

    # ---- §7.5
    def gmi(h, which=tuple(B[:2]), null_list=False, vm=ones, n_vars=nv, cm=None, n_cons=0, away=0.01):
        w, status = _a(list(which) + [0], u32), _a(np.full(len(which) + 1, -7), i32)
        st = L.mlp_solution_add_gmi_cuts(h, None if null_list else _p(w, u32), len(which), _p(vm, u8), n_vars, _p(cm, u8), n_cons, away, _p(status, i32))
        return st, {"status[%d]" % i: int(v) for i, v in enumerate(status[:len(which)])}
    E.append(("add_gmi_cuts", "m", [
        ("valid", gmi), ("valid, integer slacks", lambda h: gmi(h, cm=_a(np.ones(nc), u8), n_cons=nc)), ("n == 0", lambda h: gmi(h, ())),
        ("NULL list", lambda h: gmi(h, null_list=True)), ("NULL mask", lambda h: gmi(h, vm=None)), ("index out of range", lambda h: gmi(h, (B[0], nv))),
        ("index listed twice", lambda h: gmi(h, (B[1], B[1]))), ("wrong num_vars", lambda h: gmi(h, n_vars=nv + 1)),
        ("wrong num_constraints", lambda h: gmi(h, cm=cons0, n_cons=nc + 1)), ("away 0", lambda h: gmi(h, away=0.0)), (NULL_HANDLE, gmi)]))

    # ---- §7.6
    def branch(h, which=tuple(B[:2]), null_list=False, null_out=False, vm=None, n_vars=0, cm=None, n_cons=0):
        n = len(which)
        w = _a(list(which) + [0], u32)
        dn, up, fr = (_a(np.zeros(n + 1), f64) for _ in range(3))
        dc, uc, status = _a(np.zeros(n + 1), i64), _a(np.zeros(n + 1), i64), _a(np.full(n + 1, -7), i32)
        st = L.mlp_solution_branch_penalties(h, None if null_list else _p(w, u32), n, _p(vm, u8), n_vars, _p(cm, u8), n_cons, None if null_out else _p(dn, f64),
                                             _p(up, f64), _p(dc, i64), _p(uc, i64), _p(fr, f64), _p(status, i32))
        return st, {"status[%d]" % i: int(v) for i, v in enumerate(status[:n])}
    E.append(("branch_penalties", "r", [
        ("valid", branch), ("valid, integer marks", lambda h: branch(h, vm=ones, n_vars=nv, cm=cons0, n_cons=nc)), ("n == 0", lambda h: branch(h, ())),
        ("NULL list", lambda h: branch(h, null_list=True)), ("NULL output", lambda h: branch(h, null_out=True)),
        ("index out of range", lambda h: branch(h, (B[0], nv))), ("index listed twice", lambda h: branch(h, (B[1], B[1]))),
        ("wrong num_vars", lambda h: branch(h, vm=ones, n_vars=nv + 1)), ("wrong num_constraints", lambda h: branch(h, vm=ones, n_vars=nv, cm=cons0, n_cons=nc + 1)),
        (NULL_HANDLE, branch)]))

    # ---- §7.7
    def bound_list(fn):
        """The copy-out of a (vars, lo, hi) list: fn(h, vars, lo, hi, cap, count, flag, **kw)."""
        def call(h, null_count=False, null_out=False, cap=nv, **kw):
            v, lo, hi = _a(np.full(nv + 1, 77), u32), _a(np.full(nv + 1, 77.0), f64), _a(np.full(nv + 1, 77.0), f64)
            count, flag = u64(77), C.c_int(77)
            st = fn(h, None if null_out else _p(v, u32), _p(lo, f64), _p(hi, f64), cap, None if null_count else C.byref(count), C.byref(flag), **kw)
            return st, dict(count=int(count.value), flag=int(flag.value), untouched=int((v == 77).sum()))
        return call

    cutoff = bound_list(lambda h, v, lo, hi, cap, count, flag, c=S.cutoff, vm=None, n_vars=nv:
                        L.mlp_solution_cutoff_bounds(h, c, _p(vm, u8), n_vars, v, lo, hi, cap, count, flag))
    E.append(("cutoff_bounds", "r", [
        ("valid", cutoff), ("valid, integer marks", lambda h: cutoff(h, vm=ones)), ("valid, pruned", lambda h: cutoff(h, c=S.cutoff_pruning)),
        ("NULL count", lambda h: cutoff(h, null_count=True)), ("NULL output", lambda h: cutoff(h, null_out=True)),
        ("wrong num_vars", lambda h: cutoff(h, n_vars=nv + 1)), ("NaN cutoff", lambda h: cutoff(h, c=float("nan"))),
        ("cap below the count", lambda h: cutoff(h, cap=0)), (NULL_HANDLE, cutoff)]))

    def fix_vars(h, which=tuple(NB[:2]), null_list=False, null_vals=False, vals=None):
        w = _a(list(which) + [0], u32)
        vals = _a([x[min(j, nv - 1)] for j in which] + [0.0] if vals is None else list(vals) + [0.0], f64)
        return L.mlp_solution_fix_vars(h, None if null_list else _p(w, u32), None if null_vals else _p(vals, f64), len(which)), {}
    E.append(("fix_vars", "m", [
        ("valid", fix_vars), ("valid, a basic variable", lambda h: fix_vars(h, (B[0],), vals=(0.5 * x[B[0]],))), ("n == 0", lambda h: fix_vars(h, ())),
        ("NULL list", lambda h: fix_vars(h, null_list=True)), ("NULL values", lambda h: fix_vars(h, null_vals=True)),
        ("index out of range", lambda h: fix_vars(h, (NB[0], nv))), ("index listed twice", lambda h: fix_vars(h, (NB[1], NB[1]))), (NULL_HANDLE, fix_vars)]))

    def unfix_vars(h, p, n, null_out=False):
        k = u64(77)
        return L.mlp_solution_unfix_vars(h, p, n, None if null_out else C.byref(k)), outs(unfixed=k)
    E.append(("unfix_vars", "m", [("setup: fix_vars", fix_vars)] + var_list(unfix_vars, NB[:2]) +
              [("setup: fix_vars again", fix_vars), ("valid, NULL count", lambda h: unfix_vars(h, _p(_a(NB[:2], u32), u32), 2, True))]))

    # ---- §7.8
    def set_bounds(h, which=(B[0], B[1], NB[0]), null_list=False, null_lo=False, lo=None, hi=None):
        w = _a(list(which) + [0], u32)
        js = [min(j, nv - 1) for j in which]
        lo = _a([S.lo[j] for j in js] + [0.0] if lo is None else list(lo) + [0.0], f64)
        hi = _a([0.5 * x[js[0]]] + [S.hi[j] for j in js[1:]] + [0.0] if hi is None else list(hi) + [0.0], f64)
        return L.mlp_solution_set_var_bounds(h, None if null_list else _p(w, u32), None if null_lo else _p(lo, f64), _p(hi, f64), len(which)), {}
    E.append(("set_var_bounds", "m", [
        ("valid", set_bounds), ("valid, the current bounds", lambda h: set_bounds(h, hi=[S.hi[j] for j in (B[0], B[1], NB[0])])),
        ("n == 0", lambda h: set_bounds(h, (), hi=())), ("NULL list", lambda h: set_bounds(h, null_list=True)), ("NULL bounds", lambda h: set_bounds(h, null_lo=True)),
        ("index out of range", lambda h: set_bounds(h, (B[0], nv))), ("index listed twice", lambda h: set_bounds(h, (B[1], B[1]))),
        ("lo > hi", lambda h: set_bounds(h, (B[0],), lo=(2.0,), hi=(1.0,))), (NULL_HANDLE, set_bounds)]))

    def tighten_rc(h, c=S.cutoff, vm=None, n_vars=nv, null_out=False):
        k, flag = u64(77), C.c_int(77)
        st = L.mlp_solution_tighten_by_reduced_cost(h, c, _p(vm, u8), n_vars, None if null_out else C.byref(k), C.byref(flag))
        return st, outs(tightened=k, flag=flag)
    E.append(("tighten_by_reduced_cost", "m", [
        ("valid", tighten_rc), ("valid, integer marks", lambda h: tighten_rc(h, vm=ones)), ("valid, pruned", lambda h: tighten_rc(h, c=S.cutoff_pruning)),
        ("NULL output", lambda h: tighten_rc(h, null_out=True)), ("wrong num_vars", lambda h: tighten_rc(h, n_vars=nv + 1)),
        ("NaN cutoff", lambda h: tighten_rc(h, c=float("nan"))), (NULL_HANDLE, tighten_rc)]))

    def var_bounds(h, which=(0, 1, 2), n=None, null_out=False):
        w = None if which is None else _a(list(which) + [0], u32)
        n = len(which) if n is None else n
        lo, hi = _a(np.zeros(max(n, 1)), f64), _a(np.zeros(max(n, 1)), f64)
        return L.mlp_solution_var_bounds(h, _p(w, u32), n, None if null_out else _p(lo, f64), _p(hi, f64)), {}
    E.append(("var_bounds", "r", [("valid", var_bounds), ("n == 0", lambda h: var_bounds(h, ())), ("valid, no list", lambda h: var_bounds(h, None, nv)),
                                  ("NULL list", lambda h: var_bounds(h, None, 2)), ("NULL output", lambda h: var_bounds(h, null_out=True)),
                                  ("index out of range", lambda h: var_bounds(h, (0, nv))), (NULL_HANDLE, var_bounds)]))

    # ---- §7.9
    propagate = bound_list(lambda h, v, lo, hi, cap, count, flag, vm=None, n_vars=nv, rounds=10:
                           L.mlp_solution_propagate_bounds(h, _p(vm, u8), n_vars, rounds, v, lo, hi, cap, count, flag))
    E.append(("propagate_bounds", "r", [
        ("valid", propagate), ("valid, integer marks", lambda h: propagate(h, vm=ones)), ("NULL count", lambda h: propagate(h, null_count=True)),
        ("NULL output", lambda h: propagate(h, null_out=True)), ("wrong num_vars", lambda h: propagate(h, n_vars=nv + 1)),
        ("max_rounds 0", lambda h: propagate(h, rounds=0)), ("max_rounds 65", lambda h: propagate(h, rounds=65)),
        ("cap below the count", lambda h: propagate(h, cap=0)), (NULL_HANDLE, propagate)]))

    def tighten_prop(h, vm=None, n_vars=nv, rounds=10, null_out=False):
        k, flag = u64(77), C.c_int(77)
        st = L.mlp_solution_tighten_by_propagation(h, _p(vm, u8), n_vars, rounds, None if null_out else C.byref(k), C.byref(flag))
        return st, outs(tightened=k, flag=flag)
    E.append(("tighten_by_propagation", "m", [
        ("valid", tighten_prop), ("valid, integer marks", lambda h: tighten_prop(h, vm=ones)), ("NULL output", lambda h: tighten_prop(h, null_out=True)),
        ("wrong num_vars", lambda h: tighten_prop(h, n_vars=nv + 1)), ("max_rounds 0", lambda h: tighten_prop(h, rounds=0)),
        ("max_rounds 65", lambda h: tighten_prop(h, rounds=65)), (NULL_HANDLE, tighten_prop)]))

    # ---- the eight reports
    for name, struct in REPORTS:
        fn = getattr(L, "mlp_solution_%s_info" % name)

        def info(h, null_out=False, fn=fn, struct=struct):
            return fn(h, None if null_out else C.byref(struct())), {}
        E.append((name + "_info", "r", [("valid", info), ("NULL output", lambda h, info=info: info(h, True)), (NULL_HANDLE, info)]))
    return E


def _reports(L, h):
    out = {}
    for name, struct in REPORTS:
        r = struct()
        st = getattr(L, "mlp_solution_%s_info" % name)(h, C.byref(r))
        out[name] = dict(status=st, **{f: (getattr(r, f) if f == "bytes" else int(getattr(r, f))) for f, _ in struct._fields_ if f not in TIMES})
    return out


_ZERO = {name: dict(status=0, **{f: 0 for f, _ in struct._fields_ if f not in TIMES}) for name, struct in REPORTS}


def record_case(case):
    """{"entry point: label": record}.  The calls of one entry point run in turn on one handle, a fresh one after a call that consumed
    it; `reports` holds the reports that differ from the previous record of the same handle (all zero on a fresh one)."""
    instance, state = case.split("/")
    S = _State(instance, state)
    L, out = S.L, {}
    try:
        for entry, kind, calls in _entries(S):
            h = None
            for label, call in calls:
                if h is None:
                    h, prev = S.fresh(), _ZERO
                rec = {}
                if label == NULL_HANDLE:
                    hv = C.c_void_p()
                    st, o = call(C.byref(hv) if kind == "m" else hv)
                elif kind == "m":
                    hv = C.c_void_p(h)
                    st, o = call(C.byref(hv))
                    rec["consumed"] = not hv.value
                    h = hv.value                                                         # (None once the library has freed it)
                else:
                    st, o = call(C.c_void_p(h))
                rec["status"] = int(st)
                if st < 0:
                    rec["error"] = L.mlp_last_error().decode()
                if o:
                    rec["outputs"] = o
                if h is not None:
                    cur = _reports(L, C.c_void_p(h))
                    rec["reports"] = {name: r for name, r in cur.items() if r != prev[name]}
                    rec["objective"] = _hex(L.mlp_solution_objective(C.c_void_p(h)))
                    prev = cur
                out["%s: %s" % (entry, label)] = rec
            if h is not None:
                L.mlp_solution_free(C.c_void_p(h))
    finally:
        S.close()
    return out


def record():
    return {case: record_case(case) for case in CASES}


def call_names():
    """The names of the calls of every case: no GPU and no library needed (the lists depend on the model for their arguments only)."""
    import types

    class AnyName:
        def __getattr__(self, name):
            return None
    S = types.SimpleNamespace(L=AnyName(), nv=8, nc=4, nr=4, x=np.ones(8), lo=np.zeros(8), hi=np.ones(8), basic=[0, 1, 2], nonbasic=[3, 4, 5],
                              cutoff=0.0, cutoff_pruning=0.0)
    return ["%s: %s" % (entry, label) for entry, _, calls in _entries(S) for label, _ in calls]


def drop_differences(a, b, path=()):
    """Removes from a (in place) every leaf on which two recordings disagree; returns the paths.  Only objective bits and `bytes` may go:
    statuses, texts, consumed flags and integer counters are deterministic by construction."""
    dropped = []
    assert sorted(a) == sorted(b), (path, sorted(set(a) ^ set(b)))
    for k in list(a):
        if isinstance(a[k], dict) and isinstance(b[k], dict):
            dropped += drop_differences(a[k], b[k], path + (k,))
        elif a[k] != b[k]:
            assert k in ("objective", "bytes"), (path, k, a[k], b[k])
            del a[k]
            dropped.append("/".join(path + (k,)))
    return dropped


def dump(rec, path):
    with open(path, "w") as f:                                                           # one line per call
        f.write("{\n" + ",\n".join("%s: {\n%s\n}" % (json.dumps(case), ",\n".join(
            "%s: %s" % (json.dumps(k), json.dumps(r, sort_keys=True)) for k, r in sorted(calls.items()))) for case, calls in sorted(rec.items())) + "\n}\n")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--merge"]:                                                     # --merge FIRST.json SECOND.json [OUT.json]
        rec, again = json.load(open(sys.argv[2])), json.load(open(sys.argv[3]))
        dropped = drop_differences(rec, again)
        path = sys.argv[4] if len(sys.argv) > 4 else GOLDEN
        print("two recordings disagree on %d fields: %s" % (len(dropped), dropped))
    else:
        path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
        rec = record()
    dump(rec, path)
    print("%d cases, %d calls -> %s" % (len(rec), sum(len(c) for c in rec.values()), path))
