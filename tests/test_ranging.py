"""Basis status, cost ranging and rhs ranging of a Solution (include/minilp_hip.h: mlp_solution_basis_status, mlp_solution_cost_ranging,
mlp_solution_rhs_ranging, mlp_solution_ranging_info; csrc/ranging.inc).

CPU: the entry points exist in the header, the library, the Python mirror and the Rust crates; the ABI version is still 5.  GPU: the known
answer of the lib.rs doc example, a host reference (scipy splu of the basis, the definitions of the header applied to every variable and
constraint), the behaviour of the oracle's optimum inside and outside the ranges, every representation of B^-1, warm starts, no side
effects, determinism and batch independence, refusals, and a measurement at config-4 size.

Definitions (internal minimisation form, current basis; include/minilp_hip.h has the full text): |alpha| <= 1e-8 and |h| <= 1e-8 count as
zero, numerators of the wrong sign are clamped to 0, a Maximize problem's cost range is [-hi, -lo].

Two notes on the cases of the config-4 tests:
  * config 4 (gen_sparse_lp(100000, 100000, 100, 4)) has no structural column with fewer than 59 entries, so every basic structural variable
    of its bases sits at a NUCLEUS position and every row with a non-basic slack is a NUCLEUS row: "nucleus and singleton positions both
    present" cannot be asserted for the 24 requested variables there.  What config 4 does exercise of the singleton side is the pull of
    h over the ~90 000 basic slacks and the slack columns of the sweep.  Singleton POSITIONS among the requested variables (the sparse
    combination of stored rows) are asserted on `_singleton_lp` below, in the same host-reference test as the other instances.
  * the host solve of the late basis (nucleus 20 493) is the dense LU (scipy.linalg.lu_factor) of the nucleus after the singleton columns
    are split off on the host, not splu of the whole basis: SuperLU's fill on that nucleus is the dense factor anyway, at a fraction of
    LAPACK's speed."""
import ctypes
import gzip
import json
import math
import os
import re

import numpy as np
import pytest

import minilp_amd as M
from minilp_amd import api, build as mbuild, lpgen
from tests.common import ROOT

INF = math.inf
MID = os.path.join(ROOT, "tests", "golden", "cfg4_basis_p45000.bin.gz")
LATE = os.path.join(ROOT, "tests", "golden", "cfg4_basis_p240000.bin.gz")
NEW = ["mlp_solution_basis_status", "mlp_solution_cost_ranging", "mlp_solution_rhs_ranging", "mlp_solution_ranging_info",
       "mlp_ranging_info_size"]
PD = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(M.lib_path()):
        mbuild.build(verbose=False)
    return M.lib()


# ------------------------------------------------------------------------------------------------ CPU
def test_header_library_python_and_rust_have_the_five_symbols(L):
    hdr = open(os.path.join(ROOT, "include", "minilp_hip.h")).read()
    sys_rs = open(os.path.join(ROOT, "integration", "rust", "minilp-hip-sys", "src", "lib.rs")).read()
    api_py = open(os.path.join(ROOT, "minilp_amd", "api.py")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(ctypes.CDLL(M.lib_path()), n), n
        assert n in api_py, n
        assert re.search(r"pub fn %s\s*\(" % n, sys_rs), n
    assert "typedef struct mlp_ranging_info" in hdr
    for n in ("MLP_BASIC = 0", "MLP_AT_LOWER = 1", "MLP_AT_UPPER = 2", "MLP_NB_FREE = 3", "MLP_NB_FIXED = 4"):
        assert n in hdr, n
    assert (M.MLP_BASIC, M.MLP_AT_LOWER, M.MLP_AT_UPPER, M.MLP_NB_FREE, M.MLP_NB_FIXED) == (0, 1, 2, 3, 4)
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "minilp", "src", "lib.rs")).read()
    for n in ("cost_range", "rhs_range", "is_basic"):
        assert re.search(r"pub fn %s\s*\(" % n, lib_rs), n
    for n in ("basis_status", "cost_ranging", "rhs_ranging", "ranging_info"):
        assert hasattr(M.Solution, n), n


def test_abi_version_is_still_5_and_the_struct_size_matches(L):
    assert L.mlp_abi_version() == 5 == api.ABI_VERSION
    assert L.mlp_ranging_info_size() == ctypes.sizeof(api.MlpRangingInfo) == 40


def test_null_solution_is_einval_not_a_crash(L):
    buf = np.zeros(4)
    ib = np.zeros(4, dtype=np.int32)
    pi = ctypes.POINTER(ctypes.c_int32)
    assert L.mlp_solution_basis_status(None, ib.ctypes.data_as(pi), 4, ib.ctypes.data_as(pi), 4) == -1
    assert L.mlp_solution_cost_ranging(None, None, 4, buf.ctypes.data_as(PD), buf.ctypes.data_as(PD)) == -1
    assert L.mlp_solution_rhs_ranging(None, None, 4, buf.ctypes.data_as(PD), buf.ctypes.data_as(PD)) == -1
    assert L.mlp_solution_ranging_info(None, ctypes.byref(api.MlpRangingInfo())) == -1


# ------------------------------------------------------------------------------------------------ host reference
class HostRef:
    """The definitions of include/minilp_hip.h applied on the host to a basis: A with the slack identity, B from the basic variables,
    scipy solves.  Everything internal (minimisation form) until the last step."""

    def __init__(self, Af, c_int, lo, hi, rhs, bv, x, n, direction, fixed=(), dense_split=False):
        import scipy.sparse as sp
        self.Af = sp.csc_matrix(Af)
        self.m, self.N = self.Af.shape
        self.n, self.c, self.lo, self.hi, self.rhs = n, np.asarray(c_int, float), np.asarray(lo, float), np.asarray(hi, float), np.asarray(rhs, float)
        self.bv = np.asarray(bv, dtype=np.int64)
        self.direction = direction
        m, N = self.m, self.N
        assert len(self.bv) == m
        self.pos = np.full(N, -1, dtype=np.int64)
        self.pos[self.bv] = np.arange(m)
        A = self.Af[:, :n]
        xs = self.rhs - A @ x
        self.xall = np.concatenate([x, xs])
        st = np.zeros(N, dtype=np.int32)
        nb = self.pos < 0
        fx = np.zeros(N, dtype=bool)
        fx[list(fixed)] = True
        xa, lo_, hi_ = self.xall, self.lo, self.hi
        s_struct = np.where(fx | (lo_ == hi_), 4, np.where(xa == lo_, 1, np.where(xa == hi_, 2, 3)))
        s_slack = np.where(lo_ == hi_, 4, np.where(np.isfinite(lo_), 1, 2))       # a non-basic slack sits at its only finite bound
        st[nb] = np.where(np.arange(N) < n, s_struct, s_slack)[nb]
        self.st = st
        self.nb = np.flatnonzero(nb)
        self.B = self.Af[:, self.bv].tocsc()
        self._split = dense_split
        self._factor()
        y = self.solve_t(self.c[self.bv][:, None])[:, 0]
        self.y = y
        r = self.c - self.Af.T @ y
        r[self.bv] = 0.0
        self.r = r
        self.xB = self.xall[self.bv]

    @classmethod
    def from_lp(cls, lp, s, fixed=(), **kw):
        import scipy.sparse as sp
        m, n = lp["m"], lp["n"]
        A = sp.csr_matrix((lp["data"], lp["indices"], lp["indptr"]), shape=(m, n))
        Af = sp.hstack([A, sp.identity(m)], format="csc")
        sg = -1.0 if lp["direction"] == M.MAXIMIZE else 1.0
        ops = lp["ops"]
        slo = np.where(ops == lpgen.GE, -INF, 0.0)
        shi = np.where(ops == lpgen.LE, INF, 0.0)
        bv = s.state("host_basic_vars")
        return cls(Af, np.concatenate([sg * lp["obj"], np.zeros(m)]), np.concatenate([lp["lo"], slo]), np.concatenate([lp["hi"], shi]),
                   lp["rhs"], bv, s.values(), n, lp["direction"], fixed, **kw)

    @classmethod
    def from_state(cls, s, direction, fixed=()):
        """The model as the engine holds it (after add_gomory_cut, whose row the host does not know otherwise)."""
        import scipy.sparse as sp
        ip, ix, dt = s.state("csr_indptr").astype(np.int64), s.state("csr_indices").astype(np.int64), s.state("csr_data")
        lo, hi, c, rhs = s.state("orig_var_mins"), s.state("orig_var_maxs"), s.state("orig_obj_coeffs"), s.state("orig_rhs")
        m, N = len(ip) - 1, len(lo)
        Af = sp.csr_matrix((dt, ix, ip), shape=(m, N)).tocsc()
        return cls(Af, c, lo, hi, rhs, s.state("host_basic_vars"), s.values(), N - m, direction, fixed)

    def _factor(self):
        if not self._split:
            from scipy.sparse.linalg import splu
            self.lu = splu(self.B)
            return
        # singleton columns split off (B = [[D, F], [0, K]] in a row / column order of the host's own), dense LU of K
        import scipy.linalg as sl
        Bc = self.B
        cn = np.diff(Bc.indptr)
        self.ps = np.flatnonzero(cn == 1)
        self.pk = np.flatnonzero(cn != 1)
        self.rs = Bc.indices[Bc.indptr[self.ps]]
        self.D = Bc.data[Bc.indptr[self.ps]]
        isk = np.ones(self.m, dtype=bool)
        isk[self.rs] = False
        self.rk = np.flatnonzero(isk)
        Br = Bc.tocsr()
        self.K = sl.lu_factor(Br[self.rk][:, self.pk].toarray())
        self.F = Br[self.rs][:, self.pk].tocsr()

    def solve(self, R):      # B^-1 R, by position
        if not self._split:
            return self.lu.solve(np.ascontiguousarray(R))
        import scipy.linalg as sl
        X = np.zeros_like(R)
        X[self.pk] = sl.lu_solve(self.K, R[self.rk])
        X[self.ps] = (R[self.rs] - self.F @ X[self.pk]) / self.D[:, None]
        return X

    def solve_t(self, C):    # B^-T C, by row
        if not self._split:
            return self.lu.solve(np.ascontiguousarray(C), trans="T")
        import scipy.linalg as sl
        Y = np.zeros_like(C)
        Y[self.rs] = C[self.ps] / self.D[:, None]
        Y[self.rk] = sl.lu_solve(self.K, C[self.pk] - self.F.T @ Y[self.rs], trans=1)
        return Y

    def status(self, cons_row=None):
        cr = np.arange(self.m) if cons_row is None else np.asarray(cons_row)
        return self.st[:self.n].copy(), np.where(cr < 0, 0, self.st[self.n + np.maximum(cr, 0)])

    def cost(self, js, eps=1e-8):
        js = np.asarray(js, dtype=np.int64)
        lo, hi = np.empty(len(js)), np.empty(len(js))
        c, r, st = self.c, self.r, self.st
        for t, j in enumerate(js):
            if self.pos[j] < 0:
                s = st[j]
                lo[t] = c[j] - max(r[j], 0.0) if s == 1 else (c[j] if s == 3 else -INF)
                hi[t] = c[j] - min(r[j], 0.0) if s == 2 else (c[j] if s == 3 else INF)
        bas = np.flatnonzero(self.pos[js] >= 0)
        nb, stn = self.nb, st[self.nb]
        num = np.where(stn == 1, np.maximum(r[nb], 0.0), np.minimum(r[nb], 0.0))
        AN = self.Af[:, nb].T.tocsr()
        for b0 in range(0, len(bas), 256):
            tt = bas[b0:b0 + 256]
            E = np.zeros((self.m, len(tt)))
            E[self.pos[js[tt]], np.arange(len(tt))] = 1.0
            AL = AN @ self.solve_t(E)                                     # |nb| x batch
            for q, t in enumerate(tt):
                a = AL[:, q]
                act = np.abs(a) > eps
                with np.errstate(divide="ignore", invalid="ignore"):
                    ratio = num / a
                plus = act & (((stn == 1) & (a > 0)) | ((stn == 2) & (a < 0)))
                minus = act & (((stn == 1) & (a < 0)) | ((stn == 2) & (a > 0)))
                free = act & (stn == 3)
                dp = min(ratio[plus].min(initial=INF), 0.0 if free.any() else INF)
                dm = max(ratio[minus].max(initial=-INF), 0.0 if free.any() else -INF)
                lo[t], hi[t] = c[js[t]] + dm, c[js[t]] + dp
        if self.direction == M.MAXIMIZE:
            lo, hi = -hi, -lo
        return lo + 0.0, hi + 0.0

    def rhs_range(self, rows, eps=1e-8):
        rows = np.asarray(rows, dtype=np.int64)
        lo, hi = np.empty(len(rows)), np.empty(len(rows))
        up, dn = np.maximum(self.hi[self.bv] - self.xB, 0.0), np.minimum(self.lo[self.bv] - self.xB, 0.0)
        need = []
        for t, i in enumerate(rows):
            if i < 0:
                lo[t], hi[t] = -INF, INF
                continue
            p = self.pos[self.n + i]
            if p >= 0:
                lo[t], hi[t] = self.rhs[i] + dn[p], self.rhs[i] + up[p]
            else:
                need.append(t)
        need = np.asarray(need, dtype=np.int64)
        for b0 in range(0, len(need), 256):
            tt = need[b0:b0 + 256]
            E = np.zeros((self.m, len(tt)))
            E[rows[tt], np.arange(len(tt))] = 1.0
            Hh = self.solve(E)
            for q, t in enumerate(tt):
                h = Hh[:, q]
                with np.errstate(divide="ignore", invalid="ignore"):
                    ru, rd = up / h, dn / h
                P, N_ = h > eps, h < -eps
                dp = min(ru[P].min(initial=INF), rd[N_].min(initial=INF))
                dm = max(rd[P].max(initial=-INF), ru[N_].max(initial=-INF))
                lo[t], hi[t] = self.rhs[rows[t]] + dm, self.rhs[rows[t]] + dp
        return lo, hi


def _close(dev, ref, tol):
    """|dev - ref| <= tol max(1, |ref|), infinities exactly."""
    dev, ref = np.asarray(dev, float), np.asarray(ref, float)
    inf = np.isinf(ref)
    ok = np.where(inf, dev == ref, np.abs(dev - np.where(inf, 0.0, ref)) <= tol * np.maximum(1.0, np.abs(np.where(inf, 0.0, ref))))
    return ok & ~(np.isinf(dev) & ~inf)


def check_against_host(ref, s, tol=1e-7, vars_=None, rows=None, cons_row=None, label=""):
    """Status arrays equal; every range end equal to tol, except where the host reference itself is unstable (its value differs between
    the zero-thresholds 0.5e-8 and 2e-8): at most 5 % of the ends."""
    n = ref.n
    if vars_ is None:
        vs, cs = s.basis_status()
        hv, hc = ref.status(cons_row)
        assert (vs == hv).all() and (cs == hc).all(), (label, np.flatnonzero(vs != hv)[:5], np.flatnonzero(cs != hc)[:5])
    js = np.arange(n) if vars_ is None else np.asarray(vars_)
    cr = (np.arange(ref.m) if cons_row is None else np.asarray(cons_row))
    cidx = np.arange(len(cr)) if rows is None else np.asarray(rows)
    out = {}
    for name, dev, fn, arg in (("cost", s.cost_ranging(None if vars_ is None else js), ref.cost, js),
                               ("rhs", s.rhs_ranging(None if rows is None else cidx), ref.rhs_range, cr[cidx])):
        a = fn(arg, 1e-8)
        b = fn(arg, 0.5e-8)
        c = fn(arg, 2e-8)
        ends_dev = np.concatenate(dev)
        ends = np.concatenate(a)
        unstable = (np.concatenate(b) != ends) | (np.concatenate(c) != ends)
        assert unstable.mean() <= 0.05, (label, name, unstable.mean())
        ok = _close(ends_dev, ends, tol) | unstable
        bad = np.flatnonzero(~ok)
        with np.errstate(invalid="ignore"):
            rel = np.where(np.isfinite(ends) & np.isfinite(ends_dev), np.abs(ends_dev - ends) / np.maximum(1, np.abs(ends)), 0.0)
        print(f"{label} {name}: {len(ends)} ends, {int(np.isfinite(ends).sum())} finite, {int(unstable.sum())} unstable, {len(bad)} off; "
              f"max rel dev {rel.max(initial=0.0):.2e}")
        assert len(bad) == 0, (label, name, bad[:8], ends_dev[bad[:8]], ends[bad[:8]])
        assert (dev[0] <= dev[1]).all()
        out[name] = dev
    return out


# ------------------------------------------------------------------------------------------------ GPU
def _doc_example(direction):
    p = M.Problem(direction)
    x = p.add_var(1.0, (0.0, INF))
    y = p.add_var(2.0, (0.0, 3.0))
    p.add_constraint([(x, 1.0), (y, 1.0)], M.LE, 4.0)
    p.add_constraint([(x, 2.0), (y, 1.0)], M.GE, 2.0)
    return p


@pytest.mark.gpu
def test_lib_rs_doc_example_known_answer():
    s = _doc_example(M.MAXIMIZE).solve()
    assert s.objective() == pytest.approx(7.0)
    vs, cs = s.basis_status()
    assert vs.dtype == np.int32 and list(vs) == [M.MLP_BASIC, M.MLP_AT_UPPER] and list(cs) == [M.MLP_AT_LOWER, M.MLP_BASIC]
    lo, hi = s.cost_ranging()
    assert np.allclose(lo, [0.0, 1.0], atol=1e-12, rtol=0) and abs(hi[0] - 2.0) <= 1e-12 and hi[1] == INF
    lo, hi = s.rhs_ranging()
    assert abs(lo[0] - 3.0) <= 1e-12 and hi[0] == INF and lo[1] == -INF and abs(hi[1] - 5.0) <= 1e-12
    info = s.ranging_info()
    assert info["requests"] == 2 and info["solves"] == 1 and info["batches"] == 1 and info["device_ms"] > 0
    # Minimize twin of test_duals.py: min x + 2y, -x - y = -4, 2x + y >= 2 -> x = 4, y = 0: x basic, y at lower, row 0 fixed, row 1 basic
    p = M.Problem(M.MINIMIZE)
    x = p.add_var(1.0, (0.0, INF))
    y = p.add_var(2.0, (0.0, 3.0))
    p.add_constraint([(x, -1.0), (y, -1.0)], M.EQ, -4.0)
    p.add_constraint([(x, 2.0), (y, 1.0)], M.GE, 2.0)
    s = p.solve()
    assert s.objective() == pytest.approx(4.0)
    vs, cs = s.basis_status()
    assert list(vs) == [M.MLP_BASIC, M.MLP_AT_LOWER] and list(cs) == [M.MLP_NB_FIXED, M.MLP_BASIC]
    lo, hi = s.cost_ranging()
    # x: alpha_y = 1 (y at lower, r_y = 1): delta+ = 1; the fixed slack imposes nothing: delta- = -inf.  y: [c - r, inf) = [1, inf)
    assert lo[0] == -INF and abs(hi[0] - 2.0) <= 1e-12 and abs(lo[1] - 1.0) <= 1e-12 and hi[1] == INF
    lo, hi = s.rhs_ranging()
    # row 0 (x = -rhs): x >= 0 -> rhs <= 0; the basic slack of row 1, s = 2 - 2x <= 0 -> x >= 1 -> rhs <= -1.  row 1: s = rhs - 8 <= 0
    assert lo[0] == -INF and abs(hi[0] + 1.0) <= 1e-12 and lo[1] == -INF and abs(hi[1] - 8.0) <= 1e-12


def _singleton_lp():
    """gen_mixed_lp(300, 400, 6, 3) with 60 extra columns of ONE entry each (cost that makes most of them basic): singleton positions among
    the basic structural variables, so that the rows of B^-1 that are sparse combinations of stored rows are requested."""
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
    q = dict(lp, n=n + k, indptr=np.asarray(nip, dtype=ip.dtype), indices=np.asarray(nix, dtype=ix.dtype), data=np.asarray(ndt, dtype=float),
             obj=np.concatenate([lp["obj"], sgn * rng.uniform(0.05, 0.4, size=k)]), lo=np.concatenate([lp["lo"], np.zeros(k)]),
             hi=np.concatenate([lp["hi"], rng.uniform(0.5, 3.0, size=k)]), name="mixed_with_singletons")
    return q


@pytest.mark.gpu
@pytest.mark.parametrize("family,args", [("mixed", (300, 400, 6, 3)), ("sparse", (400, 300, 12, 7)), ("cover", (2000, 3000, 6, 5)),
                                         ("twophase", (300, 260, 8, 6)), ("singleton", ())],
                         ids=["mixed", "sparse", "hypersparse-cover", "twophase", "singleton-columns"])
def test_host_reference_all_variables_and_constraints(family, args):
    gen = {"mixed": lpgen.gen_mixed_lp, "sparse": lpgen.gen_sparse_lp, "cover": lpgen.gen_cover_lp, "twophase": lpgen.gen_twophase_lp,
           "singleton": _singleton_lp}[family]
    lp = gen(*args)
    s = lpgen.build_problem(M.Problem, lp).solve()
    ref = HostRef.from_lp(lp, s)
    check_against_host(ref, s, label=family)
    if family == "cover":
        assert s.stats()["hyper_iters"] > 0
    if family == "singleton":
        cn = np.diff(ref.B.indptr)
        bs = ref.bv < ref.n
        assert (bs & (cn == 1)).sum() >= 5 and (bs & (cn > 1)).sum() >= 5, ((bs & (cn == 1)).sum(), (bs & (cn > 1)).sum())


def _oracle_obj(lp, O):
    try:
        return lpgen.build_problem(O.Problem, lp).solve().objective()
    except Exception:
        return None


def _highs_obj(lp):
    """Second referee for the one thing the oracle cannot do: like the reference it reports Unbounded for some bounded models in which a
    FREE variable has a non-zero cost (mixed (60, 80, 5, 3), variable 79 at cost 0.03: HiGHS solves it, optimum = the linear prediction)."""
    import scipy.sparse as sp
    from scipy.optimize import linprog
    A = sp.csr_matrix((lp["data"], lp["indices"], lp["indptr"]), shape=(lp["m"], lp["n"]))
    ops, sg = lp["ops"], (-1.0 if lp["direction"] == M.MAXIMIZE else 1.0)
    le, ge, eq = ops == lpgen.LE, ops == lpgen.GE, ops == lpgen.EQ
    r = linprog(sg * lp["obj"], A_ub=sp.vstack([A[le], -A[ge]]), b_ub=np.concatenate([lp["rhs"][le], -lp["rhs"][ge]]),
                A_eq=A[eq] if eq.any() else None, b_eq=lp["rhs"][eq] if eq.any() else None, bounds=list(zip(lp["lo"], lp["hi"])), method="highs",
                options={"primal_feasibility_tolerance": 1e-10, "dual_feasibility_tolerance": 1e-10})
    return sg * r.fun if r.status == 0 else None


def behaviour_against_oracle(lp, O, obj, x, pi, cost, rhs, js, cs):
    """Inside a range the oracle's optimum is the linear prediction; beyond a finite end it leaves it on the concave (cost) / convex (rhs)
    side in the minimisation sense, or the model turns infeasible (rhs).  Returns (ends tested, ends that showed the deviation)."""
    tol = 1e-9 * max(1.0, abs(obj))
    sg = -1.0 if lp["direction"] == M.MAXIMIZE else 1.0
    tested = shown = 0
    for kind, idx, (lo, hi), key, slope in (("cost", js, cost, "obj", x), ("rhs", cs, rhs, "rhs", pi)):
        for t, i in enumerate(idx):
            cur = float(lp[key][i])
            assert lo[t] <= cur <= hi[t]
            a = lo[t] if np.isfinite(lo[t]) else cur - 1.0
            b = hi[t] if np.isfinite(hi[t]) else cur + 1.0
            for f in (0.25, 0.75):
                v = a + f * (b - a)
                q = dict(lp, **{key: lp[key].copy()})
                q[key][i] = v
                got = _oracle_obj(q, O)
                if got is None and kind == "cost" and lp["lo"][i] == -INF and lp["hi"][i] == INF:
                    got = _highs_obj(q)
                assert got is not None and abs(got - (obj + (v - cur) * slope[i])) <= tol, (kind, i, v, got, obj + (v - cur) * slope[i])
            for end, sgn in ((lo[t], -1.0), (hi[t], 1.0)):
                if not np.isfinite(end):
                    continue
                v = end + sgn * (0.5 * abs(end - cur) + 0.1)
                q = dict(lp, **{key: lp[key].copy()})
                q[key][i] = v
                got = _oracle_obj(q, O)
                if got is None and kind == "cost" and lp["lo"][i] == -INF and lp["hi"][i] == INF:
                    got = _highs_obj(q)
                lin = obj + (v - cur) * slope[i]
                tested += 1
                if kind == "rhs":
                    shown += got is None or sg * (got - lin) > tol
                else:
                    shown += got is not None and sg * (lin - got) > tol
    return tested, shown


@pytest.mark.gpu
@pytest.mark.parametrize("family,args", [("mixed", (60, 80, 5, 3)), ("sparse", (400, 300, 12, 7)), ("cover", (70, 90, 5, 5))])
def test_behaviour_against_the_oracle(family, args):
    from oracle import minilp_oracle as O
    gen = {"mixed": lpgen.gen_mixed_lp, "sparse": lpgen.gen_sparse_lp, "cover": lpgen.gen_cover_lp}[family]
    lp = gen(*args)
    s = lpgen.build_problem(M.Problem, lp).solve()
    rng = np.random.default_rng(7)
    js = rng.choice(lp["n"], size=min(20, lp["n"]), replace=False)
    cs = rng.choice(lp["m"], size=min(20, lp["m"]), replace=False)
    tested, shown = behaviour_against_oracle(lp, O, s.objective(), s.values(), s.dual_values(), s.cost_ranging(js), s.rhs_ranging(cs), js, cs)
    print(f"{family}: {shown} of {tested} finite ends show the deviation")
    assert shown >= 0.8 * tested, (shown, tested)


@pytest.fixture(scope="module")
def cfg4():
    lp = lpgen.gen_sparse_lp(100000, 100000, 100, 4)
    return lp, lpgen.build_problem(M.Problem, lp)


def _load(prob, path, **kw):
    with gzip.open(path, "rb") as f:
        return prob.solve_from_basis(f.read(), budget=0, **kw)


def _pick(ref, s, k, seed):
    """k basic structural variables and k constraints whose slack is non-basic, drawn with a fixed seed."""
    rng = np.random.default_rng(seed)
    vs, cs = s.basis_status()
    bas, nbr = np.flatnonzero(vs == M.MLP_BASIC), np.flatnonzero(cs != M.MLP_BASIC)
    return rng.choice(bas, size=min(k, len(bas)), replace=False), rng.choice(nbr, size=min(k, len(nbr)), replace=False)


@pytest.mark.gpu
def test_delayed_mode_pending_terms_against_splu(cfg4):
    lp, prob = cfg4
    a = _load(prob, MID)
    a.continue_solve(10)                                               # pending rank-1 terms of the delayed-update mode
    assert a.stats()["nucleus_size"] >= 9000
    ref = HostRef.from_lp(lp, a)
    js, cs = _pick(ref, a, 24, 5)
    assert len(js) == 24 and len(cs) == 24
    cn = np.diff(ref.B.indptr)
    assert (cn[ref.pos[js]] > 1).all() and (cn == 1).sum() >= 80000     # nucleus positions requested; the singleton side is the basic slacks
    check_against_host(ref, a, tol=1e-6, vars_=js, rows=cs, label="config 4 mid + 10 pivots")
    a.cost_ranging(js)
    info = a.ranging_info()
    assert info["solves"] == 24 and info["batches"] == 2 and info["requests"] == 24
    a.rhs_ranging(cs)
    assert a.ranging_info()["solves"] == 24


@pytest.mark.gpu
def test_compact_factor_at_the_optimum_and_with_pending_terms(monkeypatch):
    monkeypatch.setenv("MLP_FACTOR", "1")
    lp = lpgen.gen_transport_lp(600, 700, 4, 5, tight=0.45)
    s = lpgen.build_problem(M.Problem, lp).solve()
    assert s.stats()["factor_active"] == 1
    check_against_host(HostRef.from_lp(lp, s), s, label="compact factor, optimum")
    s = lpgen.build_problem(M.Problem, lp).solve(budget=70)
    assert s.stats()["factor_active"] == 1
    ref = HostRef.from_lp(lp, s)
    js, cs = _pick(ref, s, 40, 3)
    check_against_host(ref, s, vars_=js, rows=cs, label="compact factor, 70 pivots")
    assert s.ranging_info()["solves"] == len(cs)


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
    ref = HostRef.from_lp(lp, s)
    js, cs = _pick(ref, s, 40, 3)
    check_against_host(ref, s, vars_=js, rows=cs, label="sparse bump")


def _extend(lp, idx, val, op, rhs):
    q = dict(lp)
    q["indptr"] = np.append(lp["indptr"], lp["indptr"][-1] + len(idx))
    q["indices"] = np.append(lp["indices"], np.asarray(idx, dtype=lp["indices"].dtype))
    q["data"] = np.append(lp["data"], val)
    q["ops"] = np.append(lp["ops"], op).astype(lp["ops"].dtype)
    q["rhs"] = np.append(lp["rhs"], rhs)
    q["m"] = lp["m"] + 1
    return q


@pytest.mark.gpu
def test_warm_starts_grow_the_arrays_and_keep_the_host_reference():
    lp = lpgen.gen_mixed_lp(300, 400, 6, 3)
    s = lpgen.build_problem(M.Problem, lp).solve()
    m0 = s.num_constraints
    x = s.values()
    s = s.add_constraint([(0, 1.0), (1, 1.0)], M.LE, float(x[0] + x[1]) - 0.5)
    assert s.num_constraints == m0 + 1 and len(s.rhs_ranging()[0]) == m0 + 1 and len(s.basis_status()[1]) == m0 + 1
    lp2 = _extend(lp, [0, 1], [1.0, 1.0], lpgen.LE, float(x[0] + x[1]) - 0.5)
    check_against_host(HostRef.from_lp(lp2, s), s, label="add_constraint")
    x = s.values()
    vs, _ = s.basis_status()
    frac = [j for j in range(lp["n"]) if vs[j] == M.MLP_BASIC and abs(x[j] - round(x[j])) > 1e-6]
    assert frac
    s = s.add_gomory_cut(frac[0])
    assert s.num_constraints == m0 + 2 and len(s.rhs_ranging()[0]) == m0 + 2 and len(s.basis_status()[1]) == m0 + 2
    check_against_host(HostRef.from_state(s, lp["direction"]), s, label="add_gomory_cut")
    s = lpgen.build_problem(M.Problem, lp).solve()
    x = s.values()
    vs, _ = s.basis_status()
    j = next(j for j in range(lp["n"]) if vs[j] == M.MLP_BASIC and lp["lo"][j] < x[j] < lp["hi"][j])
    s = s.fix_var(j, float(x[j]) + 0.25 if x[j] + 0.25 <= lp["hi"][j] else float(x[j]) - 0.25)
    vs, _ = s.basis_status()
    lo, hi = s.cost_ranging([j])
    assert vs[j] == M.MLP_NB_FIXED and lo[0] == -INF and hi[0] == INF
    check_against_host(HostRef.from_lp(lp, s, fixed=[j]), s, label="fix_var")


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


def _read_all(s):
    s.basis_status(); s.cost_ranging(); s.rhs_ranging(); s.ranging_info()


@pytest.mark.gpu
def test_reading_has_no_side_effects_through_every_mutator():
    lp = lpgen.gen_mixed_lp(300, 400, 6, 3)
    a = lpgen.build_problem(M.Problem, lp).solve(budget=150, trace=True)
    b = a.clone()
    blob = a.save_basis(2)
    _read_all(a)
    assert a.save_basis(2) == blob and _blob(a) == _blob(b)
    a, b = _same_step(a, b, lambda s: (s.continue_solve(40), s)[1])
    _read_all(a)
    a, b = _same_step(a, b, lambda s: (s.continue_solve(-1), s)[1])
    _read_all(a)
    x = a.values()
    vs, _ = a.basis_status()
    basic = [j for j in range(lp["n"]) if vs[j] == M.MLP_BASIC and abs(x[j] - round(x[j])) > 1e-6]
    a, b = _same_step(a, b, lambda s: s.add_gomory_cut(basic[0]))
    _read_all(a)
    rhs = float(x[0] + x[1]) - 0.25
    a, b = _same_step(a, b, lambda s: s.add_constraint([(0, 1.0), (1, 1.0)], M.LE, rhs))
    _read_all(a)
    j = int(np.argmax(np.abs(a.values())))
    v = float(a.values()[j])
    a, b = _same_step(a, b, lambda s: s.fix_var(j, v))
    assert _blob(a) == _blob(b)


@pytest.mark.gpu
def test_delayed_mode_reading_has_no_side_effects(cfg4):
    lp, prob = cfg4
    a = _load(prob, MID, trace=True)
    a.continue_solve(10)
    b = a.clone()
    blob0 = a.save_basis(2)
    vs, cs = a.basis_status()
    js, rs = np.flatnonzero(vs == 0)[:20], np.flatnonzero(cs != 0)[:20]
    a.cost_ranging(js); a.rhs_ranging(rs); a.ranging_info()
    assert a.save_basis(2) == blob0 and _blob(a) == _blob(b)
    a, b = _same_step(a, b, lambda s: (s.continue_solve(40), s)[1])
    assert _blob(a) == _blob(b)


@pytest.mark.gpu
@pytest.mark.parametrize("budget", [300, -1])
def test_determinism_and_batch_independence(budget):
    lp = lpgen.gen_sparse_lp(1500, 1400, 12, 9)
    s = lpgen.build_problem(M.Problem, lp).solve(budget=budget)
    t = s.clone()
    c_all, r_all = s.cost_ranging(), s.rhs_ranging()
    for u in (s, t):                                                    # a second read, and a clone that never read
        c2, r2 = u.cost_ranging(), u.rhs_ranging()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(c_all + r_all, c2 + r2))
    vs, cs = s.basis_status()
    assert all(x.tobytes() == y.tobytes() for x, y in zip((vs, cs), t.basis_status()))
    rng = np.random.default_rng(3)
    for kind, full, pool, fn in (("cost", c_all, np.flatnonzero(vs == M.MLP_BASIC), s.cost_ranging),
                                 ("rhs", r_all, np.flatnonzero(cs != M.MLP_BASIC), s.rhs_ranging)):
        assert len(pool) >= 40, (kind, len(pool))
        for j in pool[:3]:
            lo, hi = fn([j])
            assert lo.tobytes() == full[0][j:j + 1].tobytes() and hi.tobytes() == full[1][j:j + 1].tobytes()
        for size in (1, 15, 17, 33):
            lst = rng.choice(pool, size=size, replace=False)
            lst = np.concatenate([lst, lst[:2]])                        # duplicates are allowed
            rng.shuffle(lst)
            lo, hi = fn(lst)
            assert lo.tobytes() == full[0][lst].tobytes() and hi.tobytes() == full[1][lst].tobytes(), (kind, size)


@pytest.mark.gpu
def test_refusals():
    from minilp_amd import dist as md
    lp = lpgen.gen_sparse_lp(400, 300, 12, 7)
    prob = lpgen.build_problem(M.Problem, lp)
    s = prob.solve()
    L = M.lib()
    buf = np.zeros(8)
    pd = lambda a: a.ctypes.data_as(PD)
    assert L.mlp_solution_cost_ranging(s._h, None, 3, pd(buf), pd(buf)) == -1                      # wrong length
    assert L.mlp_solution_rhs_ranging(s._h, None, 3, pd(buf), pd(buf)) == -1
    ib = np.zeros(3, dtype=np.int32)
    pi = ctypes.POINTER(ctypes.c_int32)
    assert L.mlp_solution_basis_status(s._h, ib.ctypes.data_as(pi), 3, ib.ctypes.data_as(pi), 3) == -1
    for fn, n in ((s.cost_ranging, lp["n"]), (s.rhs_ranging, lp["m"])):
        with pytest.raises(M.InternalError) as e:
            fn([0, n])                                                                             # index >= n
        assert e.value.code == -1
    assert len(s.cost_ranging([])[0]) == 0
    s2 = prob.solve(budget=0)
    box = md.create_mailbox(1)
    try:
        s2.enable_sharding_ex(0, 1, box, "pump")
        for fn in (s2.basis_status, s2.cost_ranging, s2.rhs_ranging):
            with pytest.raises(M.InternalError) as e:
                fn()
            assert e.value.code == -1
    finally:
        md.remove_mailbox(box)


@pytest.mark.gpu
def test_config4_scale_measurement(cfg4):
    """Per-request device time of a 64-request ranging call against ONE certificate read at the same basis (k = 20 493); the issue asks for
    at most a quarter.  The figures are printed (one RANGING_CFG4_LATE line); profiles/ranging_cfg4_late.json and DESIGN 7.2 record a run:
    cost 124 us per request (0.114 of the 1.09 ms certificate read), rhs 53 us per request (0.049)."""
    lp, prob = cfg4
    s = _load(prob, LATE)
    assert s.stats()["nucleus_size"] == 20493
    vs, cs = s.basis_status()
    rng = np.random.default_rng(9)
    js = rng.choice(np.flatnonzero(vs == M.MLP_BASIC), size=64, replace=False)
    rs = rng.choice(np.flatnonzero(cs != M.MLP_BASIC), size=64, replace=False)
    s.cost_ranging(js[:16]); s.rhs_ranging(rs[:16])                     # warm-up reads (the certificate read is cached by now)
    clo, chi = s.cost_ranging(js)
    ci = s.ranging_info()
    rlo, rhi = s.rhs_ranging(rs)
    ri = s.ranging_info()
    sg = -1.0
    assert not np.isnan(clo).any() and not np.isnan(chi).any() and (clo <= lp["obj"][js]).all() and (lp["obj"][js] <= chi).all()
    assert not np.isnan(rlo).any() and not np.isnan(rhi).any() and (rlo <= lp["rhs"][rs]).all() and (lp["rhs"][rs] <= rhi).all()
    assert ci["solves"] == 64 and ci["batches"] == 4 and ri["solves"] == 64 and ri["batches"] == 4
    s.continue_solve(0)                                                 # drops the cached duals: the certificate is read again
    s.certificate()
    s.continue_solve(0)
    cert = s.certificate()
    rec = {"k": 20493, "certificate_ms": cert["device_ms"], "certificate_bytes": cert["bytes"]}
    for name, inf in (("cost", ci), ("rhs", ri)):
        us = inf["device_ms"] * 1e3 / inf["solves"]
        rec[name] = {"requests": int(inf["solves"]), "batches": int(inf["batches"]), "bytes": inf["bytes"], "device_ms": inf["device_ms"],
                     "us_per_request": us, "GBps": inf["bytes"] / (inf["device_ms"] * 1e-3) / 1e9,
                     "ratio_to_certificate": us * 1e-3 / cert["device_ms"]}
    print("RANGING_CFG4_LATE " + json.dumps(rec))
    ref = HostRef.from_lp(lp, s, dense_split=True)
    check_against_host(ref, s, tol=1e-6, vars_=js[:4], rows=rs[:4], label="config 4 late")
    assert rec["cost"]["ratio_to_certificate"] <= 0.25 and rec["rhs"]["ratio_to_certificate"] <= 0.25, rec
