"""Reading the simplex tableau of a Solution (include/minilp_hip.h: mlp_solution_num_rows, mlp_solution_basis_head, mlp_solution_binv_rows,
mlp_solution_binv_cols, mlp_solution_tableau_rows, mlp_solution_tableau_cols, mlp_solution_basis_solve, mlp_solution_tableau_info;
csrc/tableau.inc).

CPU: the entry points exist in the header, the library, the Python mirror and the Rust crates; the ABI version is still 5; a NULL handle is
MLP_EINVAL.  GPU: a known answer in exact rational arithmetic, a host reference (Abar = [A | I] in scipy CSC, B = Abar[:, basis_head()],
splu) on every representation of B^-1, batch edges and bit-for-bit independence of a request from the rest of its call, agreement with the
dual values, the cost ranging and the Gomory cuts the engine already reports, no side effects through every mutator, warm starts,
residuals on models with more than 524 288 rows / columns, and the refusals.

Tolerance against the host reference: |dev - ref| <= 1e-7 max(1, |ref vector|_inf) per vector (the default of check_against_host of
tests/test_ranging.py, on the same instances).  Every basis_solve call below counts every right-hand side as a solve (an all-zero one
included); a basic column given to tableau_cols is answered on the host and is no solve."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import minilp_amd as M
from minilp_amd import api, build as mbuild, lpgen
from tests.common import ROOT

INF = math.inf
TOL = 1e-7
NEW = ["mlp_solution_num_rows", "mlp_solution_basis_head", "mlp_solution_binv_rows", "mlp_solution_binv_cols", "mlp_solution_tableau_rows",
       "mlp_solution_tableau_cols", "mlp_solution_basis_solve", "mlp_solution_tableau_info", "mlp_tableau_info_size"]
PD = ctypes.POINTER(ctypes.c_double)
PU64 = ctypes.POINTER(ctypes.c_uint64)
PU32 = ctypes.POINTER(ctypes.c_uint32)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(M.lib_path()):
        mbuild.build(verbose=False)
    return M.lib()


# ------------------------------------------------------------------------------------------------ CPU
def test_header_library_python_and_rust_have_the_new_names(L):
    hdr = open(os.path.join(ROOT, "include", "minilp_hip.h")).read()
    sys_rs = open(os.path.join(ROOT, "integration", "rust", "minilp-hip-sys", "src", "lib.rs")).read()
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "minilp", "src", "lib.rs")).read()
    surface = open(os.path.join(ROOT, "integration", "rust", "API_SURFACE.md")).read()
    api_py = open(os.path.join(ROOT, "minilp_amd", "api.py")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(ctypes.CDLL(M.lib_path()), n), n
        assert n in api_py, n
        assert re.search(r"pub fn %s\s*\(" % n, sys_rs), n
    assert "typedef struct mlp_tableau_info" in hdr and "pub struct mlp_tableau_info" in sys_rs
    for n in ("basis_head", "binv_row", "binv_col", "tableau_row", "tableau_col", "ftran", "btran"):
        assert re.search(r"pub fn %s\s*\(" % n, lib_rs), n
        assert n in surface, n
    for n in ("num_rows", "basis_head", "binv_rows", "binv_cols", "tableau_rows", "tableau_cols", "basis_solve", "tableau_info"):
        assert hasattr(M.Solution, n), n


def test_abi_version_is_still_5_and_the_struct_size_matches(L):
    assert L.mlp_abi_version() == 5 == api.ABI_VERSION
    assert L.mlp_tableau_info_size() == ctypes.sizeof(api.MlpTableauInfo) == 48


def test_null_solution_is_einval_not_a_crash(L):
    buf = np.zeros(4)
    idx = np.zeros(4, dtype=np.uint64)
    pd, pi = buf.ctypes.data_as(PD), idx.ctypes.data_as(PU64)
    assert L.mlp_solution_num_rows(None) == 0
    assert L.mlp_solution_basis_head(None, pi, 4) == -1
    assert L.mlp_solution_binv_rows(None, pi, 1, pd, 4) == -1
    assert L.mlp_solution_binv_cols(None, pi, 1, pd, 4) == -1
    assert L.mlp_solution_tableau_cols(None, pi, 1, pd, 4) == -1
    a, b, c = PU64(), PU32(), PD()
    assert L.mlp_solution_tableau_rows(None, pi, 1, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == -1
    assert L.mlp_solution_basis_solve(None, 0, pd, 4, 1, pd, 4) == -1
    assert L.mlp_solution_basis_solve(None, 1, pd, 4, 1, pd, 4) == -1
    assert L.mlp_solution_tableau_info(None, ctypes.byref(api.MlpTableauInfo())) == -1


# ------------------------------------------------------------------------------------------------ host reference
class Ref:
    """Abar = [A | I] by row of the engine, B = Abar[:, basis_head()], splu.  cons_row: constraint -> row (-1: no terms, no row)."""

    def __init__(self, A, s, cons_row=None, factor=True):
        import scipy.sparse as sp
        self.m, self.n = A.shape
        self.Abar = sp.hstack([sp.csr_matrix(A), sp.identity(self.m)], format="csc")
        self.cons_row = np.arange(self.m) if cons_row is None else np.asarray(cons_row, dtype=np.int64)
        self.ncons = len(self.cons_row)
        self.has = self.cons_row >= 0
        self.head = s.basis_head()
        assert self.head.dtype == np.int64 and len(self.head) == self.m == s.num_rows and self.ncons == s.num_constraints
        self.hvar = self.var_of(self.head)
        self.pos = np.full(self.n + self.m, -1, dtype=np.int64)
        self.pos[self.hvar] = np.arange(self.m)
        assert (self.pos[self.hvar] == np.arange(self.m)).all()              # no column twice
        self.B = self.Abar[:, self.hvar].tocsc()
        self.col_of_var = np.concatenate([np.arange(self.n), self.n + np.flatnonzero(self.has)])
        if factor:
            from scipy.sparse.linalg import splu
            self.lu = splu(self.B)

    @classmethod
    def from_lp(cls, lp, s, **kw):
        import scipy.sparse as sp
        return cls(sp.csr_matrix((lp["data"], lp["indices"], lp["indptr"]), shape=(lp["m"], lp["n"])), s, **kw)

    def var_of(self, cols):
        cols = np.asarray(cols, dtype=np.int64)
        return np.where(cols < self.n, cols, self.n + self.cons_row[np.maximum(cols - self.n, 0)])

    def by_cons(self, V):      # [rows, k] by row -> [k, constraints]
        out = np.zeros((V.shape[1], self.ncons))
        out[:, self.has] = V[self.cons_row[self.has]].T
        return out

    def binv_rows(self, cols):
        E = np.zeros((self.m, len(cols)))
        E[self.pos[self.var_of(cols)], np.arange(len(cols))] = 1.0
        return self.lu.solve(E, trans="T")                                    # rho by row, one column per request

    def tableau_rows(self, cols):
        return np.asarray(self.Abar.T @ self.binv_rows(cols)).T               # [k, variables]

    def binv_cols(self, cons):
        E = np.zeros((self.m, len(cons)))
        E[self.cons_row[np.asarray(cons)], np.arange(len(cons))] = 1.0
        return self.lu.solve(E).T

    def tableau_cols(self, cols):
        return self.lu.solve(self.Abar[:, self.var_of(cols)].toarray()).T

    def ftran(self, rhs):      # [k, constraints] -> [k, positions]
        X = np.zeros((self.m, rhs.shape[0]))
        X[self.cons_row[self.has]] = rhs[:, self.has].T
        return self.lu.solve(X).T

    def btran(self, rhs):      # [k, positions] -> [k, constraints]
        return self.by_cons(self.lu.solve(np.ascontiguousarray(rhs.T), trans="T"))


def _near(dev, ref, tol=TOL, what=""):
    dev, ref = np.atleast_2d(dev), np.atleast_2d(ref)
    assert dev.shape == ref.shape, (what, dev.shape, ref.shape)
    if dev.size == 0:
        return 0.0
    scale = np.maximum(1.0, np.abs(ref).max(axis=1))
    err = (np.abs(dev - ref).max(axis=1) / scale).max()
    assert err <= tol, (what, err)
    return err


def _dense_rows(ref, ip, ix, dv):
    out = np.zeros((len(ip) - 1, ref.n + ref.ncons))
    for t in range(len(ip) - 1):
        out[t, ix[ip[t]:ip[t + 1]]] = dv[ip[t]:ip[t + 1]]
    return out


def check_rows_structure(ref, cols, ip, ix, dv):
    """sorted, no stored zero, own entry == 1.0, no other basic column"""
    assert ip[0] == 0 and len(ip) == len(cols) + 1 and ip[-1] == len(ix) == len(dv) and (dv != 0.0).all()
    isb = np.zeros(ref.n + ref.ncons, dtype=bool)
    isb[ref.head] = True
    for t, j in enumerate(cols):
        cc, vv = ix[ip[t]:ip[t + 1]], dv[ip[t]:ip[t + 1]]
        assert (np.diff(cc) > 0).all() and (cc < ref.n + ref.ncons).all()
        bas = cc[isb[cc]]
        assert list(bas) == [j] and vv[cc == j][0] == 1.0, (t, j, bas)
        if (~ref.has).any():
            assert not np.isin(cc, ref.n + np.flatnonzero(~ref.has)).any()


def _rhs(rng, k, width):
    """seeded dense right-hand sides; one column all zero, one a unit vector (when there is room)"""
    r = rng.standard_normal((k, width))
    if k >= 2:
        r[k - 1] = 0.0
    if k >= 3:
        r[k - 2] = 0.0
        r[k - 2, width // 3] = 1.0
    return r


def check_ops(ref, s, rng, n_req=None, tol=TOL, label="", solves=(1, 16, 17)):
    """All seven operations against the host reference: everything (n_req None) or n_req seeded requests per operation."""
    n, ncons, m = ref.n, ref.ncons, ref.m
    head = ref.head
    nonbasic = np.setdiff1d(ref.col_of_var, head)
    withrow = np.flatnonzero(ref.has)
    pick = (lambda a: a) if n_req is None else (lambda a: rng.choice(a, size=min(n_req, len(a)), replace=False))
    errs = {}
    cols = pick(head)
    errs["binv_rows"] = _near(s.binv_rows(cols), ref.by_cons(ref.binv_rows(cols)), tol, label + " binv_rows")
    ip, ix, dv = s.tableau_rows(cols)
    info = s.tableau_info()
    assert info["requests"] == info["solves"] == len(cols) and info["batches"] == -(-len(cols) // 16) and info["nnz"] == len(ix)
    assert len(cols) == 0 or (info["device_ms"] > 0 and info["bytes"] > 0)
    check_rows_structure(ref, cols, ip, ix, dv)
    want = np.zeros((len(cols), n + ncons))
    want[:, ref.col_of_var] = ref.tableau_rows(cols)
    errs["tableau_rows"] = _near(_dense_rows(ref, ip, ix, dv), want, tol, label + " tableau_rows")
    cons = pick(withrow)
    errs["binv_cols"] = _near(s.binv_cols(cons), ref.binv_cols(cons), tol, label + " binv_cols")
    assert s.tableau_info()["batches"] == -(-len(cons) // 16)
    tc = np.concatenate([rng.choice(nonbasic, size=min(40, len(nonbasic)), replace=False), rng.choice(head, size=min(3, m), replace=False)])
    got = s.tableau_cols(tc)
    assert s.tableau_info()["solves"] == min(40, len(nonbasic)) and s.tableau_info()["requests"] == len(tc)
    errs["tableau_cols"] = _near(got, ref.tableau_cols(tc), tol, label + " tableau_cols")
    for t in range(min(40, len(nonbasic)), len(tc)):                          # a basic column: the exact unit vector of its position
        e = np.zeros(m)
        e[ref.pos[ref.var_of(tc[t:t + 1])[0]]] = 1.0
        assert got[t].tobytes() == e.tobytes()
    for k in solves:
        r = _rhs(rng, k, ncons)
        out = s.basis_solve(r)
        assert s.tableau_info()["solves"] == k and s.tableau_info()["batches"] == -(-k // 16)
        errs["ftran%d" % k] = _near(out, ref.ftran(r), tol, label + " basis_solve")
        r = _rhs(rng, k, m)
        errs["btran%d" % k] = _near(s.basis_solve(r, transpose=True), ref.btran(r), tol, label + " basis_solve^T")
        if k >= 2:
            assert not out[k - 1].any()                                          # the all-zero right-hand side
    print(label, {k: "%.1e" % v for k, v in errs.items()})
    return errs


# ------------------------------------------------------------------------------------------------ GPU
def _frac_inverse(B):
    k = len(B)
    a = [[Fraction(int(B[i][j])) for j in range(k)] + [Fraction(int(i == j)) for j in range(k)] for i in range(k)]
    for c in range(k):
        p = next(i for i in range(c, k) if a[i][c] != 0)
        a[c], a[p] = a[p], a[c]
        a[c] = [v / a[c][c] for v in a[c]]
        for i in range(k):
            if i != c and a[i][c] != 0:
                a[i] = [v - a[i][c] * w for v, w in zip(a[i], a[c])]
    return [row[k:] for row in a]


def _known(direction):
    sg = 1.0 if direction == M.MAXIMIZE else -1.0
    p = M.Problem(direction)
    x = [p.add_var(sg * c, (0.0, INF)) for c in (3.0, 2.0, 4.0, 1.0)]
    rows = [[1, 1, 2, 1], [2, 0, 3, 1], [2, 1, 3, 0]]
    for row, op, b in zip(rows, (M.LE, M.LE, M.LE), (4.0, 5.0, 7.0)):
        p.add_constraint([(x[j], float(v)) for j, v in enumerate(row) if v], op, b)
    return p, rows


@pytest.mark.gpu
def test_known_answer_in_rational_arithmetic():
    outs = []
    for direction in (M.MAXIMIZE, M.MINIMIZE):
        p, rows = _known(direction)
        s = p.solve()
        assert s.objective() == pytest.approx(10.5 if direction == M.MAXIMIZE else -10.5)
        m, n = 3, 4
        Abar = [[Fraction(v) for v in row] + [Fraction(int(i == c)) for c in range(m)] for i, row in enumerate(rows)]
        head = s.basis_head()
        assert s.num_rows == 3 and sorted(set(head)) == sorted(head) and (head < n + m).all()
        assert (head == s.state("host_basic_vars")).all()
        Binv = _frac_inverse([[Abar[i][j] for j in head] for i in range(m)])
        fl = lambda M_: np.array([[float(v) for v in r] for r in M_])
        BI = fl(Binv)
        T = fl([[sum(Binv[p_][i] * Abar[i][j] for i in range(m)) for j in range(n + m)] for p_ in range(m)])
        assert np.abs(s.binv_rows(head) - BI).max() <= 1e-12
        assert np.abs(s.binv_cols([0, 1, 2]) - BI.T).max() <= 1e-12
        ip, ix, dv = s.tableau_rows(head)
        nb = np.setdiff1d(np.arange(n + m), head)
        dense = np.zeros((m, n + m))
        for t in range(m):
            dense[t, ix[ip[t]:ip[t + 1]]] = dv[ip[t]:ip[t + 1]]
            assert dense[t, head[t]] == 1.0 and set(ix[ip[t]:ip[t + 1]]) <= set(nb) | {head[t]}
        assert np.abs(dense[:, nb] - T[:, nb]).max() <= 1e-12
        assert np.abs(s.tableau_cols(np.arange(n + m)) - T.T).max() <= 1e-12
        r = np.array([[1.0, 2.0, 3.0], [0.0, -1.0, 5.0]])
        assert np.abs(s.basis_solve(r) - r @ BI.T).max() <= 1e-12
        assert np.abs(s.basis_solve(r, transpose=True) - r @ BI).max() <= 1e-12
        assert np.abs(s.basis_solve(r[0]) - BI @ r[0]).max() <= 1e-12         # one-dimensional form
        outs.append((head, s.binv_rows(head), ip, ix, dv, s.tableau_cols(np.arange(n + m))))
    for a, b in zip(*outs):                                                     # no sign turn for Maximize: the tableau is identical
        assert np.array_equal(a, b)


def _singleton_lp():
    """gen_mixed_lp(300, 400, 6, 3) with 60 extra columns of ONE entry each, built like _singleton_lp of tests/test_ranging.py."""
    lp = lpgen.gen_mixed_lp(300, 400, 6, 3)
    m, n, k = lp["m"], lp["n"], 60
    rng = np.random.default_rng(11)
    rows = rng.choice(m, size=k, replace=False)
    coef = rng.uniform(0.5, 2.0, size=k)
    sgn = 1.0 if lp["direction"] == M.MAXIMIZE else -1.0
    ip, ix, dt = lp["indptr"], lp["indices"], lp["data"]
    nip, nix, ndt = [0], [], []
    extra = {int(r): (n + t, float(coef[t])) for t, r in enumerate(rows)}
    for i in range(m):
        nix.extend(ix[ip[i]:ip[i + 1]]); ndt.extend(dt[ip[i]:ip[i + 1]])
        if i in extra:
            nix.append(extra[i][0]); ndt.append(extra[i][1])
        nip.append(len(nix))
    return dict(lp, n=n + k, indptr=np.asarray(nip, dtype=ip.dtype), indices=np.asarray(nix, dtype=ix.dtype), data=np.asarray(ndt, dtype=float),
                obj=np.concatenate([lp["obj"], sgn * rng.uniform(0.05, 0.4, size=k)]), lo=np.concatenate([lp["lo"], np.zeros(k)]),
                hi=np.concatenate([lp["hi"], rng.uniform(0.5, 3.0, size=k)]), name="mixed_with_singletons")


@pytest.mark.gpu
@pytest.mark.parametrize("family,args", [("mixed", (300, 400, 6, 3)), ("sparse", (400, 300, 12, 7)), ("cover", (2000, 3000, 6, 5)),
                                         ("twophase", (300, 260, 8, 6)), ("singleton", ())],
                         ids=["mixed", "sparse", "hypersparse-cover", "twophase", "singleton-columns"])
def test_host_reference_everything_requested(family, args):
    gen = {"mixed": lpgen.gen_mixed_lp, "sparse": lpgen.gen_sparse_lp, "cover": lpgen.gen_cover_lp, "twophase": lpgen.gen_twophase_lp,
           "singleton": _singleton_lp}[family]
    lp = gen(*args)
    s = lpgen.build_problem(M.Problem, lp).solve()
    ref = Ref.from_lp(lp, s)
    assert (ref.hvar == s.state("host_basic_vars")).all()
    vs, cs = s.basis_status()
    isb = np.zeros(ref.n + ref.ncons, dtype=bool)
    isb[ref.head] = True
    assert ((vs == M.MLP_BASIC) == isb[:ref.n]).all() and ((cs == M.MLP_BASIC) == isb[ref.n:]).all()
    check_ops(ref, s, np.random.default_rng(5), label=family)
    if family == "cover":
        assert s.stats()["hyper_iters"] > 0
    if family == "singleton":
        cn = np.diff(ref.B.indptr)                                              # every basic column is requested: both kinds of position
        assert (cn == 1).sum() >= 5 and (cn > 1).sum() >= 5 and ((ref.hvar < ref.n) & (cn == 1)).sum() >= 5


def _extend(lp, idx, val, op, rhs):
    q = dict(lp)
    q["indptr"] = np.append(lp["indptr"], lp["indptr"][-1] + len(idx))
    q["indices"] = np.append(lp["indices"], np.asarray(idx, dtype=lp["indices"].dtype))
    q["data"] = np.append(lp["data"], val)
    q["ops"] = np.append(lp["ops"], op).astype(lp["ops"].dtype)
    q["rhs"] = np.append(lp["rhs"], rhs)
    q["m"] = lp["m"] + 1
    return q


def _pending(s):
    return int(s.state("lowrank_pending")[0])


def _with_pending_terms(lp):
    """A solved solution that holds pending rank-1 terms of the delayed-update mode (MLP_LOWRANK=3 set by the caller), and its model: the
    dual pivots of a warm-start re-solve leave them pending, so single violated bound rows are added until one does."""
    s = lpgen.build_problem(M.Problem, lp).solve()
    for t in range(1, 9):
        x = s.values()
        j = int(np.argsort(x)[-t])
        assert x[j] > 1e-3
        s = s.add_constraint([(j, 0.7)], M.LE, float(x[j]) * 0.35)
        lp = _extend(lp, [j], [0.7], lpgen.LE, float(x[j]) * 0.35)
        if _pending(s) > 0 and t >= 2:
            break
    assert _pending(s) > 0
    return s, lp


def _big(monkeypatch):
    for k, v in (("MLP_LOWRANK", "3"), ("MLP_BIGTILE", "1"), ("MLP_LDPAD", "16")):
        monkeypatch.setenv(k, v)


@pytest.mark.gpu
def test_delayed_mode_with_pending_terms(monkeypatch):
    _big(monkeypatch)
    s, lp = _with_pending_terms(lpgen.gen_sparse_lp(400, 300, 12, 7))
    before = _pending(s)
    assert before > 0
    ref = Ref.from_lp(lp, s)
    check_ops(ref, s, np.random.default_rng(8), n_req=40, label="pending terms")
    assert _pending(s) == before


@pytest.mark.gpu
@pytest.mark.parametrize("budget", [-1, 70])
def test_compact_factor(monkeypatch, budget):
    monkeypatch.setenv("MLP_FACTOR", "1")
    lp = lpgen.gen_transport_lp(600, 700, 4, 5, tight=0.45)
    s = lpgen.build_problem(M.Problem, lp).solve(budget=budget)
    assert s.stats()["factor_active"] == 1
    check_ops(Ref.from_lp(lp, s), s, np.random.default_rng(9), n_req=40, label="compact factor, budget %d" % budget)
    assert s.stats()["factor_active"] == 1


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
    check_ops(Ref.from_lp(lp, s), s, np.random.default_rng(10), n_req=40, label="sparse bump")


def _same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def _rows_of(res, t):
    ip, ix, dv = res
    return ix[ip[t]:ip[t + 1]], dv[ip[t]:ip[t + 1]]


def batch_independence(s, rng):
    """Request counts 1, 15, 16, 17, 33 with duplicates, shuffled: every request bit-identical alone, inside 33 and across two runs."""
    head = s.basis_head()
    n, ncons, m = s.num_vars, s.num_constraints, s.num_rows
    nonbasic = np.setdiff1d(np.arange(n + ncons), head)
    for name, fn, pool in (("binv_rows", s.binv_rows, head), ("binv_cols", s.binv_cols, np.arange(ncons)),
                           ("tableau_cols", s.tableau_cols, nonbasic)):
        pool = rng.choice(pool, size=33, replace=False)
        full = fn(pool)
        assert s.tableau_info()["solves"] == 33 and s.tableau_info()["batches"] == 3
        assert full.tobytes() == fn(pool).tobytes(), name                       # run to run
        for t in (0, 16, 32):
            assert fn(pool[t:t + 1]).tobytes() == full[t:t + 1].tobytes(), (name, t)      # alone
        for size in (1, 15, 16, 17, 33):
            at = rng.choice(33, size=size, replace=False)
            at = np.concatenate([at, at[:2]]) if size > 1 else at              # duplicates
            rng.shuffle(at)
            assert fn(pool[at]).tobytes() == full[at].tobytes(), (name, size)
            info = s.tableau_info()
            assert info["solves"] == len(at) and info["batches"] == -(-len(at) // 16), (name, size, info)
    pool = rng.choice(head, size=33, replace=False)
    full = s.tableau_rows(pool)
    assert _same(full, s.tableau_rows(pool))
    for t in (0, 16, 32):
        assert _same(_rows_of(s.tableau_rows(pool[t:t + 1]), 0), _rows_of(full, t)), t
    for size in (1, 15, 16, 17, 33):
        at = rng.choice(33, size=size, replace=False)
        at = np.concatenate([at, at[:2]]) if size > 1 else at
        rng.shuffle(at)
        got = s.tableau_rows(pool[at])
        assert s.tableau_info()["batches"] == -(-len(at) // 16)
        for q, t in enumerate(at):
            assert _same(_rows_of(got, q), _rows_of(full, t)), (size, q)
    for transpose, width in ((False, ncons), (True, m)):
        r = _rhs(rng, 33, width)
        full = s.basis_solve(r, transpose=transpose)
        assert full.tobytes() == s.basis_solve(r, transpose=transpose).tobytes()
        for t in (0, 16, 31, 32):
            assert s.basis_solve(r[t:t + 1], transpose=transpose).tobytes() == full[t:t + 1].tobytes(), (transpose, t)
        for size in (1, 15, 16, 17, 33):
            at = rng.choice(33, size=size, replace=False)
            at = np.concatenate([at, at[:2]]) if size > 1 else at
            rng.shuffle(at)
            assert s.basis_solve(r[at], transpose=transpose).tobytes() == full[at].tobytes(), (transpose, size)
            info = s.tableau_info()
            assert info["solves"] == len(at) and info["batches"] == -(-len(at) // 16)


@pytest.mark.gpu
@pytest.mark.parametrize("rep", ["explicit", "pending", "factor"])
def test_batch_edges_and_independence(monkeypatch, rep):
    if rep == "pending":
        _big(monkeypatch)
        s, _ = _with_pending_terms(lpgen.gen_sparse_lp(400, 300, 12, 7))
        before = _pending(s)
    elif rep == "factor":
        monkeypatch.setenv("MLP_FACTOR", "1")
        s = lpgen.build_problem(M.Problem, lpgen.gen_transport_lp(600, 700, 4, 5, tight=0.45)).solve()
        assert s.stats()["factor_active"] == 1
    else:
        s = lpgen.build_problem(M.Problem, lpgen.gen_sparse_lp(400, 300, 12, 7)).solve()
        assert s.stats()["factor_active"] == 0
    batch_independence(s, np.random.default_rng(3))
    if rep == "pending":
        assert _pending(s) == before > 0


def _gomory_round_from_tableau_rows(s, on_self, before_call=None):
    """17 basic variables (two batches): what add_gomory_cuts stores for each must be, bit for bit, floor(a) - a of the row tableau_rows
    returns for it, exact zeros dropped, and its right-hand side floor(x) - x of the variable's value.  Returns the rows compared."""
    from tests.test_cut_rounds import _stored_rows
    n = s.num_vars
    assert s.num_rows == s.num_constraints                          # every constraint has a row: slack columns number alike in both
    vs, _ = s.basis_status()
    x = s.values()
    basic = [j for j in range(n) if vs[j] == M.MLP_BASIC]
    frac = [j for j in basic if abs(x[j] - round(x[j])) > 1e-6]
    req = (frac + [j for j in basic if j not in set(frac)])[:17]
    assert len(req) == 17 and len(frac) >= 10, (len(req), len(frac))
    ip, ix, dv = s.tableau_rows(req)
    assert s.tableau_info()["batches"] == 2
    m0 = len(s.state("csr_indptr")) - 1
    t = s if on_self else s.clone()
    if before_call:
        before_call(t)
    t = t.add_gomory_cuts(req)
    info = t.cut_info()
    assert info["batches"] == 2, info
    stored = iter(_stored_rows(t, m0))
    compared = terms = 0
    for q, j in enumerate(req):
        a = dv[ip[q]:ip[q + 1]]
        f = np.floor(a) - a
        keep = f != 0.0
        if not keep.any():
            continue                                                # (a row without terms is not stored: counted below)
        cols, vals, rhs = next(stored)
        assert cols.tobytes() == ix[ip[q]:ip[q + 1]][keep].astype(np.int64).tobytes(), (q, j)
        assert vals.tobytes() == f[keep].tobytes(), (q, j)
        assert np.float64(rhs).tobytes() == np.float64(math.floor(x[j]) - x[j]).tobytes(), (q, j, rhs, x[j])
        compared += 1
        terms += int(keep.sum())
    assert next(stored, None) is None
    assert compared + info["rows_without_terms"] == len(req) and compared >= 10, (compared, info)
    print("gomory round against tableau rows: %d rows, %d terms, bit-identical" % (compared, terms))
    return compared


@pytest.mark.gpu
@pytest.mark.parametrize("rep", ["explicit", "pending", "factor", (40, 30, 6, 9), (200, 150, 8, 3), (600, 500, 10, 5)], ids=str)
def test_a_gomory_round_is_the_tableau_rows_bit_for_bit(monkeypatch, rep):
    """The Gomory round and the tableau rows form alpha = rho . a_j with ONE accumulator (csc_block_dot) over the same block of rows of
    B^-1: on the three representations of test_batch_edges_and_independence and on the instances of test_cut_rounds'
    test_gomory_rows_against_a_host_reference.  With pending terms the round is added to the solution itself: a clone folds them."""
    check = None
    if rep == "pending":
        _big(monkeypatch)
        s, _ = _with_pending_terms(lpgen.gen_sparse_lp(400, 300, 12, 7))

        def check(t):
            assert _pending(t) > 0
    elif rep == "factor":
        monkeypatch.setenv("MLP_FACTOR", "1")
        s = lpgen.build_problem(M.Problem, lpgen.gen_transport_lp(600, 700, 4, 5, tight=0.45)).solve()
        assert s.stats()["factor_active"] == 1
    else:
        s = lpgen.build_problem(M.Problem, lpgen.gen_sparse_lp(*((400, 300, 12, 7) if rep == "explicit" else rep))).solve()
        assert s.stats()["factor_active"] == 0
    _gomory_round_from_tableau_rows(s, on_self=rep == "pending", before_call=check)


@pytest.fixture(scope="module")
def mixed():
    lp = lpgen.gen_mixed_lp(300, 400, 6, 3)
    return lp, lpgen.build_problem(M.Problem, lp).solve()


def _internal_duals(lp, s):
    sg = -1.0 if lp["direction"] == M.MAXIMIZE else 1.0
    return sg, sg * s.dual_values(), sg * s.reduced_costs()


@pytest.mark.gpu
def test_btran_of_the_basic_costs_is_the_dual_values(mixed):
    lp, s = mixed
    sg, pi, _ = _internal_duals(lp, s)
    head = s.basis_head()
    cB = np.where(head < lp["n"], (sg * lp["obj"])[np.minimum(head, lp["n"] - 1)], 0.0)
    y = s.basis_solve(cB, transpose=True)
    assert np.abs(y - pi).max() <= 1e-9 * max(1.0, np.abs(pi).max())


@pytest.mark.gpu
def test_cost_ranges_recomputed_from_the_tableau_rows(mixed):
    lp, s = mixed
    n, m = lp["n"], lp["m"]
    sg, pi, r = _internal_duals(lp, s)
    vs, cs = s.basis_status()
    st = np.concatenate([vs, cs])
    rr = np.concatenate([r, -pi])                                               # reduced cost of a slack: 0 - e_row . y
    js = np.flatnonzero(vs == M.MLP_BASIC)
    ip, ix, dv = s.tableau_rows(js)
    lo_d, hi_d = s.cost_ranging(js)
    for t, j in enumerate(js):
        dp, dm = INF, -INF
        for i, a in zip(ix[ip[t]:ip[t + 1]], dv[ip[t]:ip[t + 1]]):
            if i == j or not abs(a) > 1e-8 or st[i] == M.MLP_NB_FIXED:
                continue
            if st[i] == M.MLP_NB_FREE:
                dp, dm = min(dp, 0.0), max(dm, 0.0)
                continue
            q = (max(rr[i], 0.0) if st[i] == M.MLP_AT_LOWER else min(rr[i], 0.0)) / a
            if (st[i] == M.MLP_AT_LOWER) == (a > 0.0):
                dp = min(dp, q)
            else:
                dm = max(dm, q)
        c = sg * lp["obj"][j]
        lo, hi = (c + dm, c + dp) if sg > 0 else (-(c + dp), -(c + dm))
        for dev, want in ((lo_d[t], lo), (hi_d[t], hi)):
            assert dev == want if math.isinf(want) or math.isinf(dev) else abs(dev - want) <= 1e-9 * max(1.0, abs(want)), (j, dev, want)


@pytest.mark.gpu
def test_gomory_cut_built_on_the_host_from_a_tableau_row(mixed):
    import scipy.sparse as sp
    lp, s = mixed
    n, m = lp["n"], lp["m"]
    A = sp.csr_matrix((lp["data"], lp["indices"], lp["indptr"]), shape=(m, n))
    x = s.values()
    vs, _ = s.basis_status()
    frac = [j for j in range(n) if vs[j] == M.MLP_BASIC and abs(x[j] - round(x[j])) > 1e-6][:5]
    assert len(frac) == 5
    for j in frac:
        ip, ix, dv = s.tableau_rows([j])
        keep = ix != j
        f = np.floor(dv[keep]) - dv[keep]
        cols = ix[keep]
        # sum f_i x_i + sum f_c s_c <= f0 with s_c = rhs_c - a_c . x
        sl = cols >= n
        row = np.zeros(n)
        row[cols[~sl]] = f[~sl]
        row -= A[cols[sl] - n].T @ f[sl]
        rhs = (math.floor(x[j]) - x[j]) - float(f[sl] @ lp["rhs"][cols[sl] - n])
        nz = np.flatnonzero(row)
        a = s.clone().add_constraints([([(int(i), float(row[i])) for i in nz], M.LE, rhs)])
        b = s.clone().add_gomory_cuts([j])
        assert abs(a.objective() - b.objective()) <= 1e-9 * max(1.0, abs(b.objective())), (j, a.objective(), b.objective())


def _bits(s, n0):
    return [tuple(np.float64(v).tobytes() if isinstance(v, float) else v for v in t) for t in s.trace()[n0:]], np.float64(s.objective()).tobytes()


def _blob(s):
    b = s.save_basis(2)
    return b[:48] + b[56:]  # (header bytes 48..56: the solution's pivot counter, which a clone starts from zero)


def _same_step(a, b, f):
    na, nb = len(a.trace()), len(b.trace())
    a, b = f(a), f(b)
    assert _bits(a, na) == _bits(b, nb)
    return a, b


def _read_all(s, rng):
    head = s.basis_head()
    ncons, m = s.num_constraints, s.num_rows
    s.binv_rows(head); s.tableau_rows(head); s.binv_cols(np.arange(ncons)); s.tableau_cols(np.arange(s.num_vars + ncons))
    s.basis_solve(_rhs(rng, 17, ncons)); s.basis_solve(_rhs(rng, 17, m), transpose=True); s.tableau_info()


def _through_every_mutator(a, b, lp, rng):
    blob = a.save_basis(2)
    _read_all(a, rng)
    assert a.save_basis(2) == blob and _blob(a) == _blob(b)
    a, b = _same_step(a, b, lambda s: (s.continue_solve(-1), s)[1])
    _read_all(a, rng)
    x = a.values()
    vs, _ = a.basis_status()
    frac = [i for i in range(lp["n"]) if vs[i] == M.MLP_BASIC and np.isfinite(x[i]) and abs(x[i] - round(x[i])) > 1e-6][:2]
    assert frac
    a, b = _same_step(a, b, lambda s: s.add_gomory_cuts(frac))
    _read_all(a, rng)
    x = a.values()
    rhs = float(x[0] + x[1]) - 0.25
    a, b = _same_step(a, b, lambda s: s.add_constraint([(0, 1.0), (1, 1.0)], M.LE, rhs))
    _read_all(a, rng)
    x = a.values()
    vs, _ = a.basis_status()
    j = next(i for i in range(lp["n"]) if vs[i] == M.MLP_BASIC and np.isfinite(lp["lo"][i]) and np.isfinite(lp["hi"][i]))
    v = float(x[j])
    a, b = _same_step(a, b, lambda s: s.fix_var(j, v))
    _read_all(a, rng)
    a, b = _same_step(a, b, lambda s: s.unfix_var(j)[0])
    assert _blob(a) == _blob(b)


@pytest.mark.gpu
def test_reading_has_no_side_effects_through_every_mutator():
    lp = lpgen.gen_mixed_lp(300, 400, 6, 3)
    a = lpgen.build_problem(M.Problem, lp).solve(budget=300, trace=True)
    _through_every_mutator(a, a.clone(), lp, np.random.default_rng(4))


def _pending_steps(a):
    """continue_solve, add_constraint, fix_var / unfix_var and add_gomory_cuts, each chosen from the solution that is read (the twin has the
    same bits): step(s) -> s."""
    x = a.values()
    vs, _ = a.basis_status()
    n = a.num_vars
    frac = [i for i in range(n) if vs[i] == M.MLP_BASIC and abs(x[i] - round(x[i])) > 1e-6][:2]
    j = next(i for i in range(n) if vs[i] == M.MLP_BASIC and x[i] > 1e-3)         # bounds [0, inf): half its value is inside them
    rhs = float(x[0] + x[1]) - 0.25
    assert frac
    return {"continue_solve": lambda s: (s.continue_solve(-1), s)[1],
            "add_constraint": lambda s: s.add_constraint([(0, 1.0), (1, 1.0)], M.LE, rhs),
            "fix_var-unfix_var": lambda s: s.fix_var(j, 0.5 * float(x[j])).unfix_var(j)[0],
            "add_gomory_cuts": lambda s: s.add_gomory_cuts(frac)}


@pytest.mark.gpu
@pytest.mark.parametrize("step", ["continue_solve", "add_constraint", "fix_var-unfix_var", "add_gomory_cuts"])
def test_reading_with_pending_terms_has_no_side_effects(monkeypatch, step):
    """A clone folds the pending terms, so the untouched twin is built by the same (deterministic) steps instead, one pair per mutator:
    every step starts from a solution that was read while it held pending terms and still holds them."""
    _big(monkeypatch)
    base = lpgen.gen_sparse_lp(400, 300, 12, 7)

    def make():
        s = lpgen.build_problem(M.Problem, base).solve(trace=True)
        for t in range(1, 9):
            x = s.values()
            j = int(np.argsort(x)[-t])
            s = s.add_constraint([(j, 0.7)], M.LE, float(x[j]) * 0.35)
            if _pending(s) > 0 and t >= 2:
                break
        return s
    a, b = make(), make()
    before = _pending(a)
    assert before > 0 and _pending(b) == before
    blob_a, blob_b = a.save_basis(2), b.save_basis(2)
    assert blob_a == blob_b
    _read_all(a, np.random.default_rng(4))
    assert _pending(a) == before                                                # applied, not folded
    assert a.save_basis(2) == blob_a                                            # its own blob, before and after the reads
    assert a.save_basis(2) == b.save_basis(2)                                   # and the twin that was never read
    f = _pending_steps(a)[step]
    assert _pending(a) == before == _pending(b)                                 # the step starts with the terms still pending
    a, b = _same_step(a, b, f)
    assert a.save_basis(2) == b.save_basis(2)


@pytest.mark.gpu
def test_warm_starts_follow_the_definitions():
    lp = lpgen.gen_mixed_lp(300, 400, 6, 3)
    n = lp["n"]
    s = lpgen.build_problem(M.Problem, lp).solve()
    m0 = s.num_constraints
    rng = np.random.default_rng(6)
    x = s.values()
    s = s.add_constraint([(0, 1.0), (1, 1.0)], M.LE, float(x[0] + x[1]) - 0.5)
    lp = _extend(lp, [0, 1], [1.0, 1.0], lpgen.LE, float(x[0] + x[1]) - 0.5)
    assert s.num_constraints == s.num_rows == m0 + 1
    check_ops(Ref.from_lp(lp, s), s, rng, n_req=40, label="add_constraint")
    x = s.values()
    rows = [([(2, 1.0), (3, 1.0)], M.LE, float(x[2] + x[3]) + 1.0), ([(4, 1.0)], M.LE, float(x[4]) + 2.0), ([(5, 1.0), (6, -1.0)], M.GE, float(x[5] - x[6]) - 1.0)]
    s = s.add_constraints(rows)
    for e, op, b in rows:
        lp = _extend(lp, [i for i, _ in e], [v for _, v in e], {M.LE: lpgen.LE, M.GE: lpgen.GE}[op], b)
    assert s.num_constraints == s.num_rows == m0 + 4
    check_ops(Ref.from_lp(lp, s), s, rng, n_req=40, label="add_constraints")
    vs, _ = s.basis_status()
    x = s.values()
    j = next(j for j in range(n) if vs[j] == M.MLP_BASIC and lp["lo"][j] < x[j] < lp["hi"][j])
    s = s.fix_var(j, float(x[j]) + 0.25 if x[j] + 0.25 <= lp["hi"][j] else float(x[j]) - 0.25)
    assert j not in s.basis_head()
    check_ops(Ref.from_lp(lp, s), s, rng, n_req=40, label="fix_var")
    # a constraint without terms: numbered, but no row, no slack column, no position
    b7 = float(s.values()[7]) + 1.0
    s = s.add_constraints([([], M.LE, 1.0), ([(7, 1.0)], M.LE, b7)])
    lp = _extend(lp, [7], [1.0], lpgen.LE, b7)
    assert s.num_constraints == m0 + 6 and s.num_rows == m0 + 5
    cons_row = np.concatenate([np.arange(m0 + 4), [-1, m0 + 4]])
    ref = Ref.from_lp(lp, s, cons_row=cons_row)
    head = s.basis_head()
    assert len(head) == m0 + 5 and (n + m0 + 4) not in head
    assert s.binv_rows(head[:3]).shape == (3, m0 + 6) and s.binv_cols([0, m0 + 5]).shape == (2, m0 + 5)
    assert s.tableau_cols([0, n + m0 + 5]).shape == (2, m0 + 5)
    assert (s.binv_rows(head)[:, m0 + 4] == 0.0).all()                          # reads 0.0 on output
    r = _rhs(rng, 3, m0 + 6)
    r2 = r.copy()
    r2[:, m0 + 4] = 123.0                                                       # ignored on input
    assert s.basis_solve(r).tobytes() == s.basis_solve(r2).tobytes()
    assert (s.basis_solve(_rhs(rng, 3, m0 + 5), transpose=True)[:, m0 + 4] == 0.0).all()
    for bad in (lambda: s.tableau_cols([n + m0 + 4]), lambda: s.binv_cols([m0 + 4])):
        with pytest.raises(M.InternalError):
            bad()
    check_ops(ref, s, rng, n_req=40, label="constraint without terms")


CAP = 4 * 256 * 512   # elements one trip of a 512-block grid with four elements per thread covers: 524 288


def _residuals(lp, s, cols_rows, cols_any, label):
    """Residuals by sparse mat-vecs against Abar only (no factorisation): |B h - abar_j|, |B^T rho - e_p|, |alpha - Abar^T rho|, each
    <= 1e-8 max(1, |solution|_inf)."""
    ref = Ref.from_lp(lp, s, factor=False)
    Bt = ref.B.T.tocsr()
    rho = s.binv_rows(cols_rows)
    ip, ix, dv = s.tableau_rows(cols_rows)
    check_rows_structure(ref, cols_rows, ip, ix, dv)
    for t, j in enumerate(cols_rows):
        p = ref.pos[ref.var_of([j])[0]]
        e = np.zeros(ref.m)
        e[p] = 1.0
        res = np.abs(Bt @ rho[t] - e).max()
        alpha = np.zeros(ref.n + ref.m)
        alpha[ix[ip[t]:ip[t + 1]]] = dv[ip[t]:ip[t + 1]]
        res_a = np.abs(alpha - ref.Abar.T @ rho[t]).max()
        bound = 1e-8 * max(1.0, np.abs(rho[t]).max())
        print(f"{label}: column {j} position {p}: |B^T rho - e| {res:.2e}, |alpha - Abar^T rho| {res_a:.2e}, bound {bound:.2e}")
        assert res <= bound and res_a <= 1e-8 * max(1.0, np.abs(alpha).max())
    h = s.tableau_cols(cols_any)
    for t, j in enumerate(cols_any):
        aj = np.asarray(ref.Abar[:, ref.var_of([j])[0]].todense()).ravel()
        res = np.abs(ref.B @ h[t] - aj).max()
        print(f"{label}: column {j}: |B h - a_j| {res:.2e}")
        assert res <= 1e-8 * max(1.0, np.abs(h[t]).max())
    hc = s.binv_cols(cols_any[:3] % ref.m)
    for t, c in enumerate(cols_any[:3] % ref.m):
        e = np.zeros(ref.m)
        e[c] = 1.0
        assert np.abs(ref.B @ hc[t] - e).max() <= 1e-8 * max(1.0, np.abs(hc[t]).max())
    rng = np.random.default_rng(12)
    r = rng.standard_normal((3, ref.m))
    y = s.basis_solve(r)
    z = s.basis_solve(r, transpose=True)
    for t in range(3):
        assert np.abs(ref.B @ y[t] - r[t]).max() <= 1e-8 * max(1.0, np.abs(y[t]).max())
        assert np.abs(Bt @ z[t] - r[t]).max() <= 1e-8 * max(1.0, np.abs(z[t]).max())
    return ref


@pytest.mark.gpu
def test_more_than_524288_rows():
    lp = lpgen.gen_sparse_lp(700000, 60000, 4, 51)
    s = lpgen.build_problem(M.Problem, lp).solve(budget=300)
    head = s.basis_head()
    n, m = lp["n"], lp["m"]
    assert m > CAP and len(head) == m
    structural = np.flatnonzero(head < n)
    assert len(structural) >= 1
    high = np.flatnonzero(np.arange(m) > CAP)
    cols_rows = np.array([head[structural[-1]], head[high[len(high) // 2]], head[high[-1]]])     # positions above 524 288 among them
    nonbasic = np.setdiff1d(np.arange(n + m), head)
    cols_any = np.array([nonbasic[0], nonbasic[nonbasic > CAP][0], nonbasic[-1]])               # columns above 524 288 among them
    ref = _residuals(lp, s, cols_rows, cols_any, "tall")
    assert (ref.pos[ref.var_of(cols_rows)] > CAP).sum() >= 2 and (cols_any > CAP).sum() >= 2


@pytest.mark.gpu
def test_more_than_524288_columns():
    lp = lpgen.gen_cover_lp(60000, 700000, 12, 52)
    s = lpgen.build_problem(M.Problem, lp).solve(budget=300)
    head = s.basis_head()
    n, m = lp["n"], lp["m"]
    assert n > CAP
    hs = np.sort(head[head < n])
    assert len(hs) >= 2
    cols_rows = np.array([hs[0], hs[-1], head[np.flatnonzero(head >= n)[-1]]])
    nonbasic = np.setdiff1d(np.arange(n + m), head)
    cols_any = np.array([nonbasic[0], nonbasic[(nonbasic > CAP) & (nonbasic < n)][0], nonbasic[nonbasic < n][-1]])
    _residuals(lp, s, cols_rows, cols_any, "wide")
    assert (cols_rows > CAP).sum() >= 1 and (cols_any > CAP).sum() >= 2


@pytest.mark.gpu
def test_refusals():
    lp = lpgen.gen_sparse_lp(400, 300, 12, 7)
    s = lpgen.build_problem(M.Problem, lp).solve()
    ref = Ref.from_lp(lp, s)
    n, m = lp["n"], lp["m"]
    head = s.basis_head()
    nonbasic = np.setdiff1d(np.arange(n + m), head)
    good = s.binv_rows(head[:2]).copy()
    Lb = M.lib()
    buf = np.zeros(4 * m)
    idx = np.array([head[0], head[1]], dtype=np.uint64)
    pd, pi = buf.ctypes.data_as(PD), idx.ctypes.data_as(PU64)

    def still_fine():
        assert s.binv_rows(head[:2]).tobytes() == good.tobytes()

    for bad in (lambda: s.tableau_rows([nonbasic[0]]), lambda: s.binv_rows([nonbasic[0]]),           # a non-basic column
                lambda: s.tableau_rows([n + m]), lambda: s.binv_rows([n + m]), lambda: s.tableau_cols([n + m]), lambda: s.binv_cols([m]),   # out of range
                lambda: s.tableau_cols([-1]), lambda: s.basis_solve(np.zeros((2, m + 1))), lambda: s.basis_solve(np.zeros((2, m - 1)), transpose=True),
                lambda: s.basis_solve(np.zeros((2, 2, m))), lambda: s.binv_rows(np.zeros((2, 2), dtype=np.int64))):   # wrong shapes
        with pytest.raises(M.InternalError) as e:
            bad()
        assert e.value.code == -1
        still_fine()
    assert Lb.mlp_solution_binv_rows(s._h, pi, 2, pd, 2 * m + 1) == -1            # wrong lengths at the C boundary
    assert Lb.mlp_solution_binv_cols(s._h, pi, 2, pd, m) == -1
    assert Lb.mlp_solution_tableau_cols(s._h, pi, 2, pd, 3 * m) == -1
    assert Lb.mlp_solution_basis_solve(s._h, 0, pd, 2 * m, 2, pd, 2 * m - 1) == -1
    assert Lb.mlp_solution_basis_head(s._h, pi, m - 1) == -1
    far = np.array([head[0], head[1], 2 ** 63], dtype=np.uint64)                  # a garbage n: refused at the first index out of range
    pa, pb, pc = PU64(), PU32(), PD()
    assert Lb.mlp_solution_tableau_rows(s._h, far.ctypes.data_as(PU64), 2 ** 40, ctypes.byref(pa), ctypes.byref(pb), ctypes.byref(pc)) == -1
    still_fine()
    t = s.clone().add_constraints([([], M.LE, 1.0)])                                    # the slack of a constraint without terms
    tref = Ref.from_lp(lp, t, cons_row=np.concatenate([np.arange(m), [-1]]))
    th = t.basis_head()[:2]
    for bad in (lambda: t.tableau_cols([n + m]), lambda: t.tableau_rows([n + m]), lambda: t.binv_rows([n + m])):
        with pytest.raises(M.InternalError) as e:
            bad()
        assert e.value.code == -1
        got = t.binv_rows(th)
        assert got.shape == (2, m + 1)
        _near(got, tref.by_cons(tref.binv_rows(th)), what="after a refusal on the slack of a constraint without terms")
    for fn, shape in ((t.binv_rows, (0, m + 1)), (t.binv_cols, (0, m)), (t.tableau_cols, (0, m))):   # n == 0: a successful no-op
        assert fn([]).shape == shape
    ip, ix, dv = t.tableau_rows([])
    assert list(ip) == [0] and len(ix) == 0 and len(dv) == 0
    assert t.basis_solve(np.zeros((0, m + 1))).shape == (0, m)
    _near(s.binv_rows(head[:2]), ref.by_cons(ref.binv_rows(head[:2])), what="after the refusals")
