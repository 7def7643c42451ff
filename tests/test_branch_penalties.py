"""Branching penalties (include/minilp_hip.h: mlp_solution_branch_penalties, mlp_branch_info; csrc/branch.inc).

The yardstick is `Ref` below: the formulas of the header in numpy / scipy, float64, on an splu factorisation of the basis the solution
reports (basis_head, basis_status) and the model.  It is built neither from cost_ranging nor from tableau_rows.  The CPU tests run it on
oracle solves (they confirm that the instances of the GPU tests leave at most 2 % of their requests to the zero threshold, that the
plain penalty bounds the child LP and the strengthened one the integer optimum of the branch); the GPU tests compare the engine with it.

Tolerance of a penalty: the relative 1e-7 of tests/test_ranging.py for its ranges (1e-6 at the config-4 basis, as there): a penalty is
f times the same ratio |d_i| / |alpha_i| the cost range is made of.  The entering column is not compared by index: the reference's
candidate at the reported column must equal the reference's minimum within that tolerance.  A request is left out of the comparison
only when some |alpha_i| of its row lies within 1e-12 of the zero threshold 1e-8 (the eligible set itself is then a matter of rounding)."""
import ctypes
import gzip
import itertools
import json
import math
import os
import re

import numpy as np
import pytest

import minilp_amd as M
from minilp_amd import api, build as mbuild, lpgen
from tests.common import OBJ_RTOL, ROOT

INF = math.inf
EPS = 1e-8  # kernels.h: |alpha| at or below it counts as zero
NEW = ["mlp_solution_branch_penalties", "mlp_solution_branch_info", "mlp_branch_info_size"]
MID = os.path.join(ROOT, "tests", "golden", "cfg4_basis_p45000.bin.gz")
INSTANCES = {"mixed": (lpgen.gen_mixed_lp, (300, 400, 6, 3)), "sparse-maximize": (lpgen.gen_sparse_lp, (400, 300, 12, 7)),
             "cover": (lpgen.gen_cover_lp, (70, 90, 5, 5)), "small-mixed": (lpgen.gen_mixed_lp, (40, 30, 6, 9))}
KEYS = ("down", "up", "down_col", "up_col", "frac", "status")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(M.lib_path()):
        mbuild.build(verbose=False)
    return M.lib()


# ------------------------------------------------------------------------------------------------ the yardstick
class Ref:
    """Internal form min c.x, [A | I] x = b.  Af: m x N with the slack identity; c: internal costs (N); basic[p]: column basic at position
    p; status[N]: 0 basic, 1 at lower, 2 at upper, 3 free, 4 fixed; xval[N]: the value of every column."""

    def __init__(self, Af, c, basic, status, xval):
        from scipy.sparse.linalg import splu
        self.Af = Af.tocsc()
        self.AT = self.Af.T.tocsr()
        self.m, self.N = self.Af.shape
        self.basic = np.asarray(basic, dtype=np.int64)
        self.st = np.asarray(status, dtype=np.int64)
        self.xval = np.asarray(xval, dtype=np.float64)
        self.pos = np.full(self.N, -1, dtype=np.int64)
        self.pos[self.basic] = np.arange(self.m)
        assert len(self.basic) == self.m and (self.st[self.basic] == 0).all() and int((self.st == 0).sum()) == self.m
        self.lu = splu(self.Af[:, self.basic].tocsc())
        c = np.asarray(c, dtype=np.float64)
        d = c - self.AT @ self.lu.solve(c[self.basic], trans="T")
        d[self.basic] = 0.0
        self.d = d
        self.num = np.where(self.st == 1, np.maximum(d, 0.0), np.where(self.st == 2, np.maximum(-d, 0.0), 0.0))

    def candidates(self, j, is_int=None, eps=EPS):
        """(down candidates[N], up candidates[N], near): inf outside the eligible set; near: some |alpha| within 1e-12 of eps."""
        st, x = self.st, self.xval[j]
        f_dn, f_up = x - math.floor(x), math.ceil(x) - x
        e = np.zeros(self.m)
        e[self.pos[j]] = 1.0
        alpha = self.AT @ self.lu.solve(e, trans="T")
        live = (st != 0) & (st != 4)
        act = live & (np.abs(alpha) > eps)
        free = act & (st == 3)
        dn = act & (((st == 1) & (alpha > 0)) | ((st == 2) & (alpha < 0)) | free)
        up = act & (((st == 1) & (alpha < 0)) | ((st == 2) & (alpha > 0)) | free)
        with np.errstate(divide="ignore", invalid="ignore"):
            rho = np.where(act, self.num / np.abs(alpha), INF)
        strong = np.zeros(self.N, bool) if is_int is None else (np.asarray(is_int, bool) & ((st == 1) | (st == 2)) & (self.xval == np.floor(self.xval)))
        out = []
        for f, sel in ((f_dn, dn), (f_up, up)):
            c = np.where(sel, f * rho, INF)
            out.append(np.where(sel & strong, np.maximum(c, self.num), c))
        return out[0], out[1], bool((live & (np.abs(np.abs(alpha) - eps) <= 1e-12)).any())

    def penalties(self, js, is_int=None):
        n = len(js)
        out = dict(down=np.zeros(n), up=np.zeros(n), frac=np.zeros(n), status=np.ones(n, dtype=np.int32), cand=[None] * n, near=np.zeros(n, bool))
        for t, j in enumerate(js):
            x = self.xval[j]
            out["frac"][t] = x - math.floor(x)
            if self.pos[j] < 0 or out["frac"][t] == 0.0:
                continue
            cd, cu, near = self.candidates(j, is_int)
            out["status"][t] = 0
            out["down"][t], out["up"][t] = cd.min(), cu.min()
            out["cand"][t] = (cd, cu)
            out["near"][t] = near
        return out


def _model(lp):
    import scipy.sparse as sp
    m, n = lp["m"], lp["n"]
    A = sp.csr_matrix((lp["data"], lp["indices"].astype(np.int64), lp["indptr"].astype(np.int64)), shape=(m, n))
    sg = -1.0 if lp["direction"] == M.MAXIMIZE else 1.0
    return sp.hstack([A, sp.identity(m)], format="csc"), np.concatenate([sg * lp["obj"], np.zeros(m)]), np.asarray(lp["rhs"], float)


def _model_of_state(s):
    """The model as the engine holds it (the rows of a cut round are known to the host only this way); the costs are the internal ones."""
    import scipy.sparse as sp
    ip, ix, dt = s.state("csr_indptr").astype(np.int64), s.state("csr_indices").astype(np.int64), s.state("csr_data")
    c, rhs = s.state("orig_obj_coeffs"), s.state("orig_rhs")
    return sp.csr_matrix((dt, ix, ip), shape=(len(ip) - 1, len(c))).tocsc(), c, rhs


def _with_slack_values(Af, rhs, x, basic):
    """Values of all N columns: a non-basic slack sits on a bound of its row's operator, which is 0, exactly."""
    m, N = Af.shape
    n = N - m
    xval = np.concatenate([x, np.zeros(m)])
    sl = rhs - Af[:, :n] @ x
    bs = basic[basic >= n]
    xval[bs] = sl[bs - n]
    return xval


def _ref_of_engine(s, model):
    Af, c, rhs = model
    m, N = Af.shape
    assert s.num_rows == s.num_constraints == m and s.num_vars == N - m
    basic = np.asarray(s.basis_head(), dtype=np.int64)
    vs, cs = s.basis_status()
    return Ref(Af, c, basic, np.concatenate([vs, cs]), _with_slack_values(Af, rhs, np.asarray(s.values()), basic))


def _ref_of_oracle(o, model):
    Af, c, rhs = model
    m, N = Af.shape
    basic, nb = o.state("basic_vars").astype(np.int64), o.state("nb_vars").astype(np.int64)
    at_min, at_max = o.state("nb_at_min") != 0, o.state("nb_at_max") != 0
    status = np.zeros(N, dtype=np.int64)
    status[nb] = np.where(at_min & at_max, 4, np.where(at_min, 1, np.where(at_max, 2, 3)))
    xval = np.zeros(N)
    xval[basic] = o.state("basic_var_vals")
    xval[nb] = o.state("nb_var_vals")
    return Ref(Af, c, basic, status, xval)


def _close(dev, ref, tol):
    if math.isinf(ref) or math.isinf(dev):
        return dev == ref
    return abs(dev - ref) <= tol * max(1.0, abs(ref))


def _compare(dev, ref, tol=1e-7, label=""):
    """The six outputs of every request against the reference; returns (compared, left out, worst relative deviation)."""
    n = len(ref["status"])
    assert all(len(dev[k]) == n for k in KEYS)
    assert dev["status"].tolist() == ref["status"].tolist(), label
    assert dev["frac"].tobytes() == ref["frac"].tobytes(), label                      # exact
    left = worst = 0
    for t in range(n):
        if ref["status"][t] == 1:
            assert dev["down"][t] == 0.0 and dev["up"][t] == 0.0 and dev["down_col"][t] == -1 and dev["up_col"][t] == -1, (label, t)
            continue
        if ref["near"][t]:
            left += 1
            continue
        for side, (val, col), cand in (("down", (dev["down"][t], dev["down_col"][t]), ref["cand"][t][0]),
                                       ("up", (dev["up"][t], dev["up_col"][t]), ref["cand"][t][1])):
            want = ref[side][t]
            assert val >= 0.0 and _close(val, want, tol), (label, t, side, val, want)
            if math.isinf(want):
                assert col == -1, (label, t, side, col)
            else:
                assert 0 <= col < len(cand) and _close(cand[col], want, tol), (label, t, side, col, cand[col] if 0 <= col < len(cand) else None, want)
                worst = max(worst, abs(val - want) / max(1.0, abs(want)))
    served = int((ref["status"] == 0).sum())
    assert 50 * left <= served, (label, left, served)                                   # at most 2 % left out
    return served - left, left, worst


def _check(s, model, js, int_vars=None, int_cons=None, tol=1e-7, label="", ref=None):
    ref = ref or _ref_of_engine(s, model)
    n = s.num_vars
    is_int = None if int_vars is None else np.concatenate([np.asarray(int_vars, bool), np.zeros(ref.N - n, bool) if int_cons is None else np.asarray(int_cons, bool)])
    want = ref.penalties(js, is_int)
    dev = s.branch_penalties(js, int_vars, int_cons)
    done, left, worst = _compare(dev, want, tol, label)
    info = s.branch_info()
    served = int((want["status"] == 0).sum())
    assert info["requests"] == len(js) and info["solves"] == served and info["batches"] == (served + 15) // 16, info
    fin = int(np.isfinite(want["down"][want["status"] == 0]).sum() + np.isfinite(want["up"][want["status"] == 0]).sum())
    print("%s: %d requests, %d served, %d left out, %d finite of %d penalties, worst relative deviation %.2e, device %.3f ms" %
          (label, len(js), served, left, fin, 2 * served, worst, info["device_ms"]))
    return dev, want


def _frac_basic(s):
    bp = s.branch_penalties(range(s.num_vars))
    return [int(j) for j in np.flatnonzero(bp["status"] == 0)]


def _knapsack(seed, n=11):
    """Pure binary, integer data, 3 <= rows, Maximize."""
    rng = np.random.default_rng(seed)
    a = rng.integers(1, 10, size=(3, n)).astype(float)
    return dict(name="knapsack_%d" % seed, direction=M.MAXIMIZE, m=3, n=n, obj=rng.integers(5, 30, size=n).astype(float), lo=np.zeros(n),
                hi=np.ones(n), indptr=np.arange(0, 3 * n + 1, n, dtype=np.uint64), indices=np.tile(np.arange(n, dtype=np.uint32), 3),
                data=a.ravel(), ops=np.full(3, lpgen.LE, dtype=np.int32), rhs=np.floor(a.sum(axis=1) * np.array([0.45, 0.5, 0.4])))


KNAPSACK_SEEDS = (1, 2, 3, 4)


def _best_integer(lp, j, val):
    """Enumeration: the best objective over the binary points with x_j = val, -inf when there is none."""
    n = lp["n"]
    X = np.array(list(itertools.product((0.0, 1.0), repeat=n)))
    X = X[X[:, j] == val]
    ok = (X @ lp["data"].reshape(3, n).T <= lp["rhs"] + 1e-9).all(axis=1)
    return float((X[ok] @ lp["obj"]).max()) if ok.any() else -INF


def _strengthening_checks(lp, obj, js, plain, strong):
    """(finite branch checks, strictly stronger entries) of one knapsack instance; asserts the bound on every branch."""
    finite = stronger = 0
    for t, j in enumerate(js):
        for side, val in (("down", 0.0), ("up", 1.0)):
            p, q = plain[side][t], strong[side][t]
            assert q >= p, (lp["name"], j, side, p, q)
            stronger += q > p
            best = _best_integer(lp, j, val)
            if math.isinf(q):
                assert best == -INF, (lp["name"], j, side, best)
            else:
                finite += 1
                assert best <= obj - q + OBJ_RTOL * max(1.0, abs(obj)), (lp["name"], j, side, best, obj, q)
    return finite, stronger


def _hand_lp():
    """max x0:  2 x0 + x1 + x2 = 3,  x1 + x3 <= 5,  x2 + x3 <= 5,  0 <= x <= 10.  Optimum x0 = 1.5, basic with both slacks; the row of x0
    is x0 = 1.5 - x1 / 2 - x2 / 2.  Up (x0 >= 2): no column is eligible, 2 x0 <= 3 forbids it.  Down (x0 <= 1): x1 and x2 are eligible,
    the penalty is 0.5 * (0.5 / 0.5) = 0.5, the child's optimum 1.  With x1 and x2 fixed at 0 the down set is empty too."""
    return dict(name="hand_3x4", direction=M.MAXIMIZE, m=3, n=4, obj=np.array([1.0, 0.0, 0.0, 0.0]), lo=np.zeros(4), hi=np.full(4, 10.0),
                indptr=np.array([0, 3, 5, 7], dtype=np.uint64), indices=np.array([0, 1, 2, 1, 3, 2, 3], dtype=np.uint32),
                data=np.array([2.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]), ops=np.array([lpgen.EQ, lpgen.LE, lpgen.LE], dtype=np.int32),
                rhs=np.array([3.0, 5.0, 5.0]))


# ------------------------------------------------------------------------------------------------ CPU
def test_header_library_python_and_rust_have_the_new_names(L):
    hdr = open(os.path.join(ROOT, "include", "minilp_hip.h")).read()
    sys_rs = open(os.path.join(ROOT, "integration", "rust", "minilp-hip-sys", "src", "lib.rs")).read()
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "minilp", "src", "lib.rs")).read()
    api_py = open(os.path.join(ROOT, "minilp_amd", "api.py")).read()
    surface = open(os.path.join(ROOT, "integration", "rust", "API_SURFACE.md")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(ctypes.CDLL(M.lib_path()), n), n
        assert n in api_py, n
        assert re.search(r"pub fn %s\s*\(" % n, sys_rs), n
    assert "typedef struct mlp_branch_info" in hdr
    # the declaration in the sys crate has the header's thirteen arguments in the header's order
    args = re.search(r"pub fn mlp_solution_branch_penalties\s*\(([^)]*)\)", sys_rs).group(1)
    assert [a.split(":")[0].strip() for a in args.split(",")] == ["s", "vars", "n", "var_is_int", "num_vars", "con_is_int", "num_constraints",
                                                                  "down", "up", "down_col", "up_col", "frac", "status"]
    assert re.search(r"pub fn branch_penalties\s*\(&self", lib_rs)
    assert re.search(r"\* `pub fn branch_penalties\(&self, .*`", surface.split("### extensions")[1])
    for n in ("branch_penalties", "branch_info"):
        assert hasattr(M.Solution, n), n


def test_abi_version_is_still_5_and_the_struct_size_matches(L):
    assert L.mlp_abi_version() == 5 == api.ABI_VERSION
    assert L.mlp_branch_info_size() == ctypes.sizeof(api.MlpBranchInfo) == 40
    assert "Still version 5: the branching penalties" in open(os.path.join(ROOT, "include", "minilp_hip.h")).read()


def test_null_handle_is_einval_not_a_crash(L):
    v = np.zeros(2, dtype=np.uint32)
    d, c, st = np.zeros(2), np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int32)
    pd, pc = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), c.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    assert L.mlp_solution_branch_penalties(None, v.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 2, None, 0, None, 0, pd, pd, pc, pc, pd,
                                           st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == -1
    assert L.mlp_solution_branch_penalties(None, None, 0, None, 0, None, 0, None, None, None, None, None, None) == -1
    assert L.mlp_solution_branch_info(None, ctypes.byref(api.MlpBranchInfo())) == -1


@pytest.mark.parametrize("name", list(INSTANCES))
def test_the_instances_stay_under_the_cap_at_the_oracle_basis(name):
    """The reference on the oracle's optimal basis: at most 2 % of the fractional basic variables have an |alpha| at the zero
    threshold, and the instance has penalties to compare at all."""
    from oracle import minilp_oracle as O
    gen, args = INSTANCES[name]
    lp = gen(*args)
    ref = _ref_of_oracle(lpgen.build_problem(O.Problem, lp).solve(), _model(lp))
    out = ref.penalties(list(range(lp["n"])))
    served = out["status"] == 0
    fin = int(np.isfinite(out["down"][served]).sum() + np.isfinite(out["up"][served]).sum())
    print("%s: %d served, %d near the threshold, %d finite penalties" % (name, served.sum(), out["near"].sum(), fin))
    assert served.sum() >= 8 and 50 * int(out["near"].sum()) <= int(served.sum()) and fin >= 8


def test_the_reference_bounds_the_child_lp_on_oracle_solves():
    """The yardstick itself: objective +- plain penalty bounds the oracle's optimum of the child, an empty set means an infeasible child."""
    from oracle import minilp_oracle as O
    for lp in (lpgen.gen_mixed_lp(40, 30, 6, 9), _hand_lp()):
        prob = lpgen.build_problem(O.Problem, lp)
        o = prob.solve()
        ref = _ref_of_oracle(o, _model(lp))
        obj, sg = o.objective(), (-1.0 if lp["direction"] == M.MAXIMIZE else 1.0)
        js = [j for j in range(lp["n"]) if ref.pos[j] >= 0 and ref.xval[j] != math.floor(ref.xval[j])]
        out = ref.penalties(js)
        finite = infeasible = 0
        for t, j in enumerate(js):
            for side, op, bound in (("down", O.LE, math.floor(ref.xval[j])), ("up", O.GE, math.ceil(ref.xval[j]))):
                try:
                    child = o.clone().add_constraint([(j, 1.0)], op, float(bound)).objective()
                except O.Infeasible:
                    child = None
                pen = out[side][t]
                if math.isinf(pen):
                    infeasible += 1
                    assert child is None, (lp["name"], j, side, child)
                elif child is not None:
                    finite += 1
                    assert sg * (child - obj) >= pen - OBJ_RTOL * max(1.0, abs(obj)), (lp["name"], j, side, child, obj, pen)
        print("%s: %d finite checks, %d infeasible branches" % (lp["name"], finite, infeasible))
        assert (finite >= 8) if lp["n"] > 4 else (finite == 1 and infeasible == 1)


def test_the_strengthened_reference_bounds_the_integer_optimum_on_oracle_solves():
    from oracle import minilp_oracle as O
    finite = stronger = 0
    for seed in KNAPSACK_SEEDS:
        lp = _knapsack(seed)
        o = lpgen.build_problem(O.Problem, lp).solve()
        ref = _ref_of_oracle(o, _model(lp))
        js = [j for j in range(lp["n"]) if ref.pos[j] >= 0 and ref.xval[j] != math.floor(ref.xval[j])]
        f, g = _strengthening_checks(lp, o.objective(), js, ref.penalties(js), ref.penalties(js, np.ones(ref.N, bool)))
        finite, stronger = finite + f, stronger + g
    print("knapsacks: %d finite branch checks, %d strictly stronger" % (finite, stronger))
    assert finite >= 4 and stronger >= 1


# ------------------------------------------------------------------------------------------------ 1: against the host reference
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(INSTANCES))
def test_explicit_inverse_at_an_optimum_against_the_host_reference(name):
    """All variables in one call (the non-basic ones are answered with status 1), plain and with every column and slack marked."""
    gen, args = INSTANCES[name]
    lp = gen(*args)
    s = lpgen.build_problem(M.Problem, lp).solve()
    model = _model(lp)
    ref = _ref_of_engine(s, model)
    js = list(range(lp["n"]))
    dev, want = _check(s, model, js, label=name, ref=ref)
    assert int((want["status"] == 0).sum()) >= 8
    _check(s, model, js, np.ones(lp["n"], bool), np.ones(lp["m"], bool), label=name + " strengthened", ref=ref)
    _check(s, model, js, np.ones(lp["n"], bool), None, label=name + " strengthened, slacks continuous", ref=ref)


@pytest.mark.gpu
def test_requested_variables_at_singleton_positions():
    from tests.test_ranging import _singleton_lp
    lp = _singleton_lp()
    s = lpgen.build_problem(M.Problem, lp).solve()
    vs, _ = s.basis_status()
    cn = np.bincount(lp["indices"], minlength=lp["n"])
    dev, want = _check(s, _model(lp), list(range(lp["n"])), np.ones(lp["n"], bool), label="singleton columns")
    served = want["status"] == 0
    assert int((served & (cn == 1)).sum()) >= 3 and int((served & (cn > 1)).sum()) >= 5, (int((served & (cn == 1)).sum()), int((served & (cn > 1)).sum()))


@pytest.mark.gpu
def test_pending_terms_of_the_delayed_update_mode(monkeypatch):
    """The committed config-4 mid basis, budget 0, then pivots that leave pending rank-1 terms (applied by the read, not folded)."""
    monkeypatch.setenv("MLP_LOWRANK", "3")
    lp = lpgen.gen_sparse_lp(100000, 100000, 100, 4)
    with gzip.open(MID, "rb") as f:
        s = lpgen.build_problem(M.Problem, lp).solve_from_basis(f.read(), budget=0)
    s.continue_solve(10)
    for _ in range(3):
        if int(s.state("lowrank_pending")[0]) > 0:
            break
        s.continue_solve(1)
    model = _model(lp)
    ref = _ref_of_engine(s, model)
    pool = np.asarray(_frac_basic(s))
    js = [int(j) for j in np.random.default_rng(5).choice(pool, size=24, replace=False)]
    assert int(s.state("lowrank_pending")[0]) > 0 and s.stats()["nucleus_size"] >= 9000
    dev, want = _check(s, model, js, tol=1e-6, label="config 4 mid + pivots", ref=ref)
    assert int(s.state("lowrank_pending")[0]) > 0                                     # still pending: nothing was folded
    info = s.branch_info()
    assert info["solves"] == 24 and info["batches"] == 2


@pytest.mark.gpu
def test_compact_factor(monkeypatch):
    monkeypatch.setenv("MLP_FACTOR", "1")
    lp = lpgen.gen_transport_lp(600, 700, 4, 5, tight=0.45)
    s = lpgen.build_problem(M.Problem, lp).solve()
    assert s.stats()["factor_active"] == 1
    _check(s, _model(lp), list(range(lp["n"])), label="compact factor, optimum")
    s = lpgen.build_problem(M.Problem, lp).solve(budget=70)
    assert s.stats()["factor_active"] == 1
    dev, want = _check(s, _model(lp), list(range(lp["n"])), np.ones(lp["n"], bool), label="compact factor, 70 pivots")
    assert int((want["status"] == 0).sum()) >= 8


@pytest.mark.gpu
def test_compact_factor_sparse_bump(monkeypatch):
    monkeypatch.setenv("MLP_FACTOR", "1")
    monkeypatch.setenv("MLP_FACTOR_SB_FROM", "1")
    s = lp = None
    for gen, args in ((lpgen.gen_sparse_lp, (400, 300, 12, 7)), (lpgen.gen_mixed_lp, (300, 400, 6, 3)), (lpgen.gen_sparse_lp, (1500, 1400, 12, 9))):
        lp = gen(*args)
        s = lpgen.build_problem(M.Problem, lp).solve()
        if s.stats()["factor_active"] == 1 and s.state("factor_sb")[0] == 1:
            break
    assert s.stats()["factor_active"] == 1 and s.state("factor_sb")[0] == 1
    dev, want = _check(s, _model(lp), list(range(lp["n"])), label="sparse bump")
    assert int((want["status"] == 0).sum()) >= 8


@pytest.mark.gpu
def test_after_fix_var_a_fixed_column_is_never_eligible():
    lp = lpgen.gen_mixed_lp(300, 400, 6, 3)
    s = lpgen.build_problem(M.Problem, lp).solve()
    model = _model(lp)
    frac = _frac_basic(s)
    x = s.values()
    fixed = frac[:3]
    for j in fixed:
        s = s.fix_var(j, float(math.floor(x[j])))
    vs, _ = s.basis_status()
    assert all(vs[j] == M.MLP_NB_FIXED for j in fixed)
    ref = _ref_of_engine(s, model)
    dev, want = _check(s, model, list(range(lp["n"])), label="after fix_var", ref=ref)
    # the fixed columns do meet requested rows (so the rule decides something), and none of them is ever reported
    hit = 0
    for j in np.flatnonzero(want["status"] == 0)[:40]:
        e = np.zeros(ref.m)
        e[ref.pos[j]] = 1.0
        hit += bool((np.abs(ref.AT[fixed] @ ref.lu.solve(e, trans="T")) > EPS).any())
    assert hit >= 1
    assert not (set(dev["down_col"].tolist()) | set(dev["up_col"].tolist())) & set(fixed)
    assert all(dev["status"][j] == 1 and dev["down"][j] == 0.0 and dev["up"][j] == 0.0 for j in fixed)


@pytest.mark.gpu
def test_after_a_gomory_round_the_slacks_of_cut_rows_take_part():
    """(On gen_mixed_lp(300, 400, 6, 3) the cuts of a round end with basic slacks, which take part in nothing; here some stay tight.)"""
    lp = lpgen.gen_sparse_lp(400, 300, 12, 7)
    s = lpgen.build_problem(M.Problem, lp).solve()
    s = s.add_gomory_cuts(_frac_basic(s)[:20])
    assert s.num_constraints == lp["m"] + 20
    model = _model_of_state(s)
    assert np.array_equal(model[1][:lp["n"]], -lp["obj"])                              # internal costs: a Maximize problem
    ref = _ref_of_engine(s, model)
    dev, want = _check(s, model, list(range(lp["n"])), label="after add_gomory_cuts", ref=ref)
    first = lp["n"] + lp["m"]                                                          # the first slack column of a cut row
    meets = sum(1 for c in want["cand"] if c is not None and (np.isfinite(c[0][first:]).any() or np.isfinite(c[1][first:]).any()))
    print("non-basic slacks of cut rows: %d, eligible in %d requested rows" % (int((ref.st[first:] != 0).sum()), meets))
    assert meets >= 1, "no slack of a cut row is eligible in any requested row"


# ------------------------------------------------------------------------------------------------ 2: the bound is a bound
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small-mixed", "cover", "sparse-maximize"])
def test_the_plain_penalty_bounds_the_child_lp(name):
    gen, args = INSTANCES[name]
    lp = gen(*args)
    s = lpgen.build_problem(M.Problem, lp).solve()
    obj, sg = s.objective(), (-1.0 if lp["direction"] == M.MAXIMIZE else 1.0)
    js = _frac_basic(s)[:12]
    bp = s.branch_penalties(js)
    x = s.values()
    finite = infeasible = 0
    for t, j in enumerate(js):
        for side, op, bound in (("down", M.LE, math.floor(x[j])), ("up", M.GE, math.ceil(x[j]))):
            try:
                child = s.clone().add_constraint([(j, 1.0)], op, float(bound)).objective()
            except M.Infeasible:
                child = None
            pen = bp[side][t]
            if math.isinf(pen):
                infeasible += 1
                assert child is None, (name, j, side, child)
            elif child is not None:
                finite += 1
                assert sg * (child - obj) >= pen - OBJ_RTOL * max(1.0, abs(obj)), (name, j, side, child, obj, pen)
    print("%s: %d finite checks, %d branches proved infeasible" % (name, finite, infeasible))
    assert finite >= 8


@pytest.mark.gpu
def test_an_empty_set_is_an_infeasible_branch_by_hand():
    lp = _hand_lp()
    s = lpgen.build_problem(M.Problem, lp).solve()
    assert abs(s.objective() - 1.5) <= 1e-12
    bp = s.branch_penalties([0, 1, 2, 3])
    assert bp["status"].tolist() == [0, 1, 1, 1] and bp["frac"][0] == 0.5
    assert bp["down"][0] == 0.5 and bp["down_col"][0] == 1 and math.isinf(bp["up"][0]) and bp["up_col"][0] == -1   # the lowest of the tied columns 1, 2
    assert abs(s.clone().add_constraint([(0, 1.0)], M.LE, 1.0).objective() - 1.0) <= 1e-12
    with pytest.raises(M.Infeasible):
        s.clone().add_constraint([(0, 1.0)], M.GE, 2.0)
    t = s.clone().fix_var(1, 0.0)
    bp = t.branch_penalties([0])
    assert bp["down"][0] == 0.5 and bp["down_col"][0] == 2
    t = t.fix_var(2, 0.0)                                                            # every eligible column of the down branch is fixed now
    bp = t.branch_penalties([0])
    assert bp["status"][0] == 0 and math.isinf(bp["down"][0]) and math.isinf(bp["up"][0]) and bp["down_col"][0] == -1 and bp["up_col"][0] == -1
    for op, bound in ((M.LE, 1.0), (M.GE, 2.0)):
        with pytest.raises(M.Infeasible):
            t.clone().add_constraint([(0, 1.0)], op, bound)


# ------------------------------------------------------------------------------------------------ 3: strengthening
@pytest.mark.gpu
def test_strengthened_penalties_bound_the_integer_optimum_of_each_branch():
    finite = stronger = 0
    for seed in KNAPSACK_SEEDS:
        lp = _knapsack(seed)
        s = lpgen.build_problem(M.Problem, lp).solve()
        js = _frac_basic(s)
        plain = s.branch_penalties(js)
        none = s.branch_penalties(js, None, None)
        unmarked = s.branch_penalties(js, np.zeros(lp["n"], bool), np.zeros(3, bool))
        assert all(plain[k].tobytes() == none[k].tobytes() == unmarked[k].tobytes() for k in KEYS)
        strong = s.branch_penalties(js, np.ones(lp["n"], bool), np.ones(3, bool))
        _check(s, _model(lp), js, np.ones(lp["n"], bool), np.ones(3, bool), label=lp["name"])
        f, g = _strengthening_checks(lp, s.objective(), js, plain, strong)
        finite, stronger = finite + f, stronger + g
    print("knapsacks: %d finite branch checks, %d strictly stronger" % (finite, stronger))
    assert finite >= 4 and stronger >= 1


# ------------------------------------------------------------------------------------------------ 4: batch independence, determinism
@pytest.mark.gpu
@pytest.mark.parametrize("budget", [300, -1])
def test_batch_independence_and_determinism(budget):
    lp = lpgen.gen_mixed_lp(300, 400, 6, 3)
    n = lp["n"]
    s = lpgen.build_problem(M.Problem, lp).solve(budget=budget)
    marks = (np.ones(n, bool), np.ones(lp["m"], bool)) if budget < 0 else (None, None)
    full = s.branch_penalties(range(n), *marks)
    again = s.branch_penalties(range(n), *marks)
    assert all(full[k].tobytes() == again[k].tobytes() for k in KEYS)
    served = np.flatnonzero(full["status"] == 0)
    assert len(served) >= 36, len(served)
    rng = np.random.default_rng(3)
    req = np.concatenate([rng.choice(served, size=36, replace=False), np.flatnonzero(full["status"] == 1)[:4]])
    assert len(req) == 40
    for j in req:
        one = s.branch_penalties([int(j)], *marks)
        assert all(one[k].tobytes() == full[k][j:j + 1].tobytes() for k in KEYS), j      # bit for bit
    lst = np.concatenate([req, req[:5]])                                              # duplicates are allowed
    rng.shuffle(lst)
    mixed = s.branch_penalties(lst, *marks)
    assert all(mixed[k].tobytes() == full[k][lst].tobytes() for k in KEYS)
    clone = s.clone().branch_penalties(lst, *marks)                                  # a clone that never read
    assert all(mixed[k].tobytes() == clone[k].tobytes() for k in KEYS)


# ------------------------------------------------------------------------------------------------ 5: no side effects
def _bits(s, n0):
    return [tuple(np.float64(v).tobytes() if isinstance(v, float) else v for v in t) for t in s.trace()[n0:]], np.float64(s.objective()).tobytes()


def _blob(s):
    b = s.save_basis(2)
    return b[:48] + b[56:]  # (header bytes 48..56: the solution's pivot counter, which a clone starts from zero)


@pytest.mark.gpu
def test_reading_has_no_side_effects():
    lp = lpgen.gen_mixed_lp(300, 400, 6, 3)
    n = lp["n"]
    a = lpgen.build_problem(M.Problem, lp).solve(budget=150, trace=True)
    b = a.clone()
    blob = a.save_basis(2)
    r0 = a.reduced_costs().tobytes()
    a.branch_penalties(range(n))
    a.branch_penalties(range(n), np.ones(n, bool), np.ones(lp["m"], bool))
    a.branch_info()
    assert a.save_basis(2) == blob and _blob(a) == _blob(b) and a.reduced_costs().tobytes() == r0
    na, nb = len(a.trace()), len(b.trace())
    a.continue_solve(40)
    b.continue_solve(40)
    assert _bits(a, na) == _bits(b, nb) and len(a.trace()) > na
    a.branch_penalties(range(n))
    na, nb = len(a.trace()), len(b.trace())
    a.continue_solve(-1)
    b.continue_solve(-1)
    assert _bits(a, na) == _bits(b, nb) and _blob(a) == _blob(b)
    x = a.values()
    j = _frac_basic(a)[0]
    na, nb = len(a.trace()), len(b.trace())
    a, b = a.fix_var(j, float(math.floor(x[j]))), b.fix_var(j, float(math.floor(x[j])))
    assert _bits(a, na) == _bits(b, nb) and _blob(a) == _blob(b)


# ------------------------------------------------------------------------------------------------ 6: refusals and trivial requests
@pytest.mark.gpu
def test_refusals_and_trivial_requests():
    from minilp_amd import dist as md
    lp = lpgen.gen_mixed_lp(40, 30, 6, 9)
    n, m = lp["n"], lp["m"]
    prob = lpgen.build_problem(M.Problem, lp)
    s = prob.solve()

    def refused(f):
        with pytest.raises(M.InternalError) as e:
            f()
        assert e.value.code == -1

    refused(lambda: s.branch_penalties([0, n]))                                       # out of range
    refused(lambda: s.branch_penalties([0, -1]))
    refused(lambda: s.branch_penalties([0], np.ones(n - 1, bool)))                    # mask lengths that do not fit
    refused(lambda: s.branch_penalties([0], np.ones(n + 1, bool)))
    refused(lambda: s.branch_penalties([0], np.ones(n, bool), np.ones(m + 1, bool)))
    refused(lambda: s.branch_penalties([0], None, np.ones(m, bool)))                  # slack marks without variable marks
    L = M.lib()
    buf, col, st = np.zeros(1), np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int32)
    v, cm = np.zeros(1, dtype=np.uint32), np.ones(m, dtype=np.uint8)
    pd, pc = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), col.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    assert L.mlp_solution_branch_penalties(s._h, v.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 1, None, 0,
                                           cm.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), m, pd, pd, pc, pc, pd,
                                           st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == -1
    s.objective()                                                                      # the solution is still usable: a read frees nothing
    # n == 0 is a no-op; non-basic and integral requests are answered with status 1 and zeros
    out = s.branch_penalties([])
    assert all(len(out[k]) == 0 for k in KEYS) and s.branch_info()["requests"] == 0
    vs, _ = s.basis_status()
    x = s.values()
    trivial = [j for j in range(n) if vs[j] != M.MLP_BASIC or x[j] == math.floor(x[j])]
    assert any(vs[j] != M.MLP_BASIC for j in trivial)
    out = s.branch_penalties(trivial)
    assert (out["status"] == 1).all() and not out["down"].any() and not out["up"].any() and (out["down_col"] == -1).all() and (out["up_col"] == -1).all()
    assert out["frac"].tobytes() == (x[trivial] - np.floor(x[trivial])).tobytes()
    info = s.branch_info()
    assert info["requests"] == len(trivial) and info["solves"] == 0 and info["batches"] == 0
    # like the other reads (cost_ranging, tableau_rows) the call accepts any basis the engine holds: at the slack basis of an unsolved
    # model no structural variable is basic
    s0 = prob.solve(budget=0)
    out = s0.branch_penalties(range(n))
    assert (out["status"] == 1).all()
    box = md.create_mailbox(1)
    try:
        s0.enable_sharding_ex(0, 1, box, "pump")
        refused(lambda: s0.branch_penalties([0]))                                     # sharded
    finally:
        md.remove_mailbox(box)


# ------------------------------------------------------------------------------------------------ 7: the example driver
TSP_SEED, TSP_CITIES = 108, 14   # (branching is needed: 18 nodes with the most fractional variable)


@pytest.mark.gpu
def test_tsp_example_reaches_the_same_tour_cost_with_penalty_branching():
    import importlib.util
    spec = importlib.util.spec_from_file_location("tsp_example_bp", os.path.join(ROOT, "examples", "tsp.py"))
    tsp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tsp)
    pts = np.random.default_rng(TSP_SEED).uniform(0.0, 100.0, size=(TSP_CITIES, 2))
    plain, pen = tsp.TspSolver(M, pts), tsp.TspSolver(M, pts, branching="penalties")
    c0, t0 = plain.solve()
    c1, t1 = pen.solve()
    print("most fractional: %s; penalties: %s" % (plain.stats, pen.stats))
    assert abs(c0 - c1) <= 1e-9 * max(1.0, abs(c0)) and abs(pen.tour_cost(t1) - c1) <= 1e-7 and sorted(t1) == list(range(TSP_CITIES))
    assert "penalty_calls" in pen.stats and "skipped_sides" in pen.stats and "penalty_calls" not in plain.stats


@pytest.mark.gpu
def test_solve_mps_example_prints_the_table(tmp_path, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("solve_mps_example_bp", os.path.join(ROOT, "examples", "solve_mps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lp = lpgen.gen_mixed_lp(40, 30, 6, 9)
    path = tmp_path / "mixed.mps"
    path.write_text(lpgen.to_mps(lp))
    assert mod.run(M, str(path), branch_penalties=True, continuous=["X3"]) == 0
    out = capsys.readouterr().out
    k = int(re.search(r"branch penalties of (\d+) fractional basic variables", out).group(1))
    assert k >= 8 and "'solves': %d" % k in out and out.count("slack(row ") + out.count(", X") >= 1
    assert mod.run(M, str(path), branch_penalties=True, continuous=["NOPE"]) == 1


# ------------------------------------------------------------------------------------------------ 8: device time against the cost ranging
@pytest.mark.gpu
def test_device_time_against_cost_ranging():
    """device_ms of branch_penalties against cost_ranging — the parent's own pass over the same bytes — on the same 64 basic requests of
    gen_mixed_lp(6000, 10000, 4, 3): median of 5 after one warm-up, one process.  The sweep reads the same data; the allowance of 1.5 is
    for the head launch, the wider partials and the per-column classification.  Written to profiles/branch_penalties.json when
    MLP_WRITE_PROFILES=1; the recorded run: 0.130 ms against 0.112 ms, ratio 1.16."""
    lp = lpgen.gen_mixed_lp(6000, 10000, 4, 3)
    s = lpgen.build_problem(M.Problem, lp).solve()
    req = _frac_basic(s)[:64]
    assert len(req) == 64
    bp, rg = [], []
    for rep in range(6):
        s.branch_penalties(req)
        bi = s.branch_info()
        s.cost_ranging(req)
        ri = s.ranging_info()
        assert bi["solves"] == ri["solves"] == 64 and bi["batches"] == ri["batches"] == 4
        if rep:
            bp.append(bi["device_ms"])
            rg.append(ri["device_ms"])
    rec = dict(instance="gen_mixed_lp(6000, 10000, 4, 3)", requests=64, batches=4, branch_device_ms=float(np.median(bp)),
               ranging_device_ms=float(np.median(rg)), branch_us_per_request=float(np.median(bp)) * 1e3 / 64,
               ranging_us_per_request=float(np.median(rg)) * 1e3 / 64, ratio=float(np.median(bp) / np.median(rg)),
               branch_bytes=bi["bytes"], ranging_bytes=ri["bytes"])
    print("BRANCH_PENALTIES " + json.dumps(rec))
    if os.environ.get("MLP_WRITE_PROFILES") == "1":
        with open(os.path.join(ROOT, "profiles", "branch_penalties.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    assert rec["ratio"] <= 1.5, rec
