"""A round of Gomory mixed-integer cuts in one call (include/minilp_hip.h: mlp_solution_add_gmi_cuts, mlp_gmi_info; csrc/gmi.inc;
DESIGN.md §7.5).

The yardstick is `gmi_reference` below: the formula of the header in numpy, on a dense solve with the basis.  The CPU tests run it on
oracle solves and check the cuts themselves (the planted integer point of the generator satisfies every row, the LP optimum misses every
row by exactly 1, every arm of the formula occurs); the GPU tests compare the rows the engine stores with it.

Tolerance of a stored coefficient: the project's agreement on a tableau entry alpha is 1e-9 (tests/test_cut_rounds.py).  The GMI
coefficient is continuous in alpha, with slope at most 1 / min(f0, 1 - f0) in every arm, and the integer arm takes the fraction of
alpha, whose error relative to g matters once |g| > 1: 1e-9 / min(f0, 1 - f0) * max(1, |g|) per entry, and the same for the rhs (a sum of
entries times bounds of magnitude O(1) on these instances)."""
import ctypes
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
EPS = 1e-8  # ranging.inc: |alpha| at or below it counts as zero on a free column
NEW = ["mlp_solution_add_gmi_cuts", "mlp_solution_gmi_info", "mlp_gmi_info_size"]
INSTANCES = [(40, 30, 6, 9), (200, 150, 8, 3), (600, 500, 10, 5)]
ARMS = ("integer", "continuous", "lower", "upper", "f_le_f0", "f_gt_f0", "abar_ge_0", "abar_lt_0", "slack_at_upper", "fixed_dropped")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(M.lib_path()):
        mbuild.build(verbose=False)
    return M.lib()


# ------------------------------------------------------------------------------------------------ the yardstick
def gmi_reference(A, basic, status, xval, is_int, requests, away, arms=None):
    """The GMI cuts of the header, dense numpy.  A: [A | I] (m x N); basic[p]: column basic at position p; status[N]: 0 basic, 1 at
    lower, 2 at upper, 3 free, 4 fixed; xval[N]: value of every column; is_int[N]: integrality marks; requests: basic columns.
    Returns [(status, c[N], rhs, f0)] per request (status 0 emitted, 1 fraction within away, 2 free column; c = 0, rhs = nan when
    skipped); arms: a dict of counters of the arms taken by columns with alpha != 0 of emitted cuts."""
    m, N = A.shape
    pos = np.full(N, -1)
    pos[basic] = np.arange(m)
    E = np.zeros((m, len(requests)))
    for t, v in enumerate(requests):
        assert pos[v] >= 0 and is_int[v]
        E[pos[v], t] = 1.0
    RHO = np.linalg.solve(A[:, basic].T, E)  # rows of B^-1, as columns
    out = []
    for t, v in enumerate(requests):
        f0 = xval[v] - math.floor(xval[v])
        if min(f0, 1.0 - f0) < away:
            out.append((1, np.zeros(N), math.nan, f0))
            continue
        alpha = RHO[:, t] @ A
        c = np.zeros(N)
        free_hit = False
        took = dict.fromkeys(ARMS, 0)
        for j in range(N):
            st = status[j]
            if st == 0:
                continue
            if st == 4:
                took["fixed_dropped"] += alpha[j] != 0.0
                continue
            if st == 3:
                if abs(alpha[j]) > EPS:
                    free_hit = True
                    break
                continue
            abar = alpha[j] if st == 1 else -alpha[j]
            if is_int[j] and xval[j] == math.floor(xval[j]):
                f = abar - math.floor(abar)
                g = f / f0 if f <= f0 else (1.0 - f) / (1.0 - f0)
                arm = ("integer", "f_le_f0" if f <= f0 else "f_gt_f0")
            else:
                g = abar / f0 if abar >= 0.0 else -abar / (1.0 - f0)
                arm = ("continuous", "abar_ge_0" if abar >= 0.0 else "abar_lt_0")
            c[j] = -g if st == 1 else g
            if alpha[j] != 0.0:
                for a in arm + ("lower" if st == 1 else "upper",):
                    took[a] += 1
                took["slack_at_upper"] += st == 2 and j >= N - m
        if free_hit:
            out.append((2, np.zeros(N), math.nan, f0))
            continue
        if arms is not None:
            for a in ARMS:
                arms[a] = arms.get(a, 0) + int(took[a])
        out.append((0, c, -1.0 + float(c @ xval), f0))
    return out


def _dense(lp):
    m, n = lp["m"], lp["n"]
    A = np.zeros((m, n + m))
    ip, ix, dt = lp["indptr"], lp["indices"], lp["data"]
    for i in range(m):
        A[i, ix[ip[i]:ip[i + 1]]] = dt[ip[i]:ip[i + 1]]
        A[i, n + i] = 1.0
    return A


def _planted(m, n, k, seed):
    """The feasible integer point gen_mixed_lp builds its rows around (lpgen.gen_mixed_lp: x0)."""
    x0 = np.floor(4.0 * lpgen.uniform01(lpgen._stream(seed, 22), n))
    kind = (lpgen.splitmix64(lpgen._stream(seed, 23), n) % np.uint64(10)).astype(np.int64)
    return np.where((kind < 6) | (kind == 9), np.maximum(x0, 0.0), x0)


def _with_slacks(lp, A, x):
    return np.concatenate([x, lp["rhs"] - A[:, :lp["n"]] @ x])


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
    assert "typedef struct mlp_gmi_info" in hdr
    assert re.search(r"pub fn add_gmi_cuts\s*\(self", lib_rs)
    assert re.search(r"\* `pub fn add_gmi_cuts\(self, .*-> Result<\(Self, Vec<i32>\), Error>`", surface.split("### extensions")[1])
    for n in ("add_gmi_cuts", "gmi_info"):
        assert hasattr(M.Solution, n), n


def test_abi_version_is_still_5_and_the_struct_sizes_match(L):
    assert L.mlp_abi_version() == 5 == api.ABI_VERSION
    assert L.mlp_gmi_info_size() == ctypes.sizeof(api.MlpGmiInfo) == 64
    assert L.mlp_cut_info_size() == ctypes.sizeof(api.MlpCutInfo) == 80


def test_null_handles_are_einval_not_a_crash(L):
    null = ctypes.c_void_p()
    v = np.zeros(2, dtype=np.uint32)
    mk = np.ones(4, dtype=np.uint8)
    pv, pm = v.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), mk.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert L.mlp_solution_add_gmi_cuts(None, pv, 2, pm, 4, None, 0, 0.01, None) == -1
    assert L.mlp_solution_add_gmi_cuts(ctypes.byref(null), pv, 2, pm, 4, None, 0, 0.01, None) == -1
    assert L.mlp_solution_add_gmi_cuts(ctypes.byref(null), None, 0, None, 0, None, 0, 0.01, None) == -1
    assert L.mlp_solution_gmi_info(None, ctypes.byref(api.MlpGmiInfo())) == -1
    assert not null.value


def _oracle_state(lp, o):
    """(basic, status, xval) of an oracle solution in the column numbering of [A | I]."""
    N = lp["n"] + lp["m"]
    basic = o.state("basic_vars").astype(np.int64)
    nb = o.state("nb_vars").astype(np.int64)
    at_min, at_max = o.state("nb_at_min") != 0, o.state("nb_at_max") != 0
    status = np.zeros(N, dtype=np.int64)
    status[nb] = np.where(at_min & at_max, 4, np.where(at_min, 1, np.where(at_max, 2, 3)))
    xval = np.zeros(N)
    xval[basic] = o.state("basic_var_vals")
    xval[nb] = o.state("nb_var_vals")
    return basic, status, xval


def _frac_of(xval, basic, n, tol=1e-6):
    return [int(j) for j in np.sort(basic) if j < n and abs(xval[j] - round(xval[j])) > tol]


def test_the_reference_formula_on_oracle_solves():
    """The yardstick itself: with every column and slack integer the planted integer point satisfies every cut, the LP optimum misses
    every cut by exactly 1, the cuts stay valid with the slacks continuous, and every arm of the formula occurs."""
    from oracle import minilp_oracle as O
    arms, counts, minslack = {}, [], []
    for args in INSTANCES:
        lp = lpgen.gen_mixed_lp(*args)
        A = _dense(lp)
        o = lpgen.build_problem(O.Problem, lp).solve()
        basic, status, xval = _oracle_state(lp, o)
        n, N = lp["n"], lp["n"] + lp["m"]
        z = _with_slacks(lp, A, _planted(*args))
        assert np.all(z == np.floor(z))
        frac = _frac_of(xval, basic, n)
        for slack_int in (True, False):
            is_int = np.concatenate([np.ones(n, bool), np.full(lp["m"], slack_int)])
            cuts = gmi_reference(A, basic, status, xval, is_int, frac, 0.01, arms)
            emitted = [c for c in cuts if c[0] == 0]
            assert all(c[0] != 2 for c in cuts)
            for st, c, rhs, f0 in emitted:
                assert c @ z <= rhs + 1e-9 * max(1.0, np.abs(c).sum())           # the planted point is kept
                assert abs(c @ xval - rhs - 1.0) <= 1e-9                          # the vertex is cut off by exactly 1
            if slack_int:
                counts.append(len(emitted))
                minslack.append(min(rhs - c @ z for st, c, rhs, f0 in emitted))
    print("cuts", counts, "min slack of the planted point", minslack, "arms", arms)
    assert all(k > 0 for k in counts) and all(s > 0 for s in minslack)
    for a in ARMS:
        assert arms[a] > 0, (a, arms)


# ------------------------------------------------------------------------------------------------ GPU helpers
def _model(s):
    return tuple(s.state(k).tobytes() for k in ("csr_indptr", "csr_indices", "csr_data", "orig_rhs", "orig_var_mins", "orig_var_maxs",
                                                "orig_obj_coeffs"))


def _stored_rows(s, first):
    """Rows first.. of the engine's CSR without their slack entry: [(cols, vals, rhs)]."""
    ip, ix, dt = s.state("csr_indptr").astype(np.int64), s.state("csr_indices").astype(np.int64), s.state("csr_data")
    rhs = s.state("orig_rhs")
    m = len(ip) - 1
    nv = s.num_vars
    out = []
    for i in range(first, m):
        c, v = ix[ip[i]:ip[i + 1]], dt[ip[i]:ip[i + 1]]
        assert c[-1] == nv + i and v[-1] == 1.0                      # the slack of the row, last
        out.append((c[:-1].copy(), v[:-1].copy(), float(rhs[i])))
    return out


def _bits(rows):
    return [(c.tobytes(), v.tobytes(), np.float64(r).tobytes()) for c, v, r in rows]


def _engine_state(lp, s):
    """(basic, status, xval) of an engine solution whose constraints all have rows.  A non-basic slack sits on a bound of its row's
    operator, which is 0: its value is exact, not rhs - a.x."""
    n, m = lp["n"], lp["m"]
    vs, cs = s.basis_status()
    assert len(vs) == n and len(cs) == m
    status = np.concatenate([vs, cs]).astype(np.int64)
    basic = np.asarray(s.basis_head(), dtype=np.int64)
    x = np.asarray(s.values())
    xval = np.concatenate([x, np.zeros(m)])
    A = _dense(lp)
    sl = lp["rhs"] - A[:, :n] @ x
    bs = basic[basic >= n]
    xval[bs] = sl[bs - n]
    return A, basic, status, xval


def _frac_basic(s, n, tol=1e-6):
    x = s.values()
    vs, _ = s.basis_status()
    return [j for j in range(n) if vs[j] == M.MLP_BASIC and abs(x[j] - round(x[j])) > tol]


def _compare(rows, ref, status, N):
    """The rows the engine stored (emitted requests, in request order) and the statuses it returned against the reference."""
    assert [int(x) for x in status] == [r[0] for r in ref]
    emitted = [r for r in ref if r[0] == 0]
    assert len(rows) == len(emitted)
    worst = 0.0
    for (cols, vals, rhs), (st, c, rhs_ref, f0) in zip(rows, emitted):
        assert np.all(np.diff(cols) > 0), "terms sorted by variable"
        assert np.all(vals != 0.0), "no stored zero"
        assert len(cols) == 0 or cols.max() < N
        dev = np.zeros(N)
        dev[cols] = vals
        unit = 1e-9 / min(f0, 1.0 - f0)
        tol = unit * np.maximum(1.0, np.abs(c))
        d = np.abs(dev - c)
        worst = max(worst, float((d / tol).max()))
        assert np.all(d <= tol), (np.flatnonzero(d > tol)[:5], d[d > tol][:5], f0)
        gmax = float(np.abs(c).max())
        worst = max(worst, abs(rhs - rhs_ref) / (unit * max(1.0, gmax)))
        assert abs(rhs - rhs_ref) <= unit * max(1.0, gmax), (rhs, rhs_ref, f0)
    return worst


def _against_host(lp, s, vars_, con_int, away=0.01, on_self=False, before_call=None, arms=None):
    """One round on a clone of s (or on s itself) against gmi_reference at the basis of s; returns (solution, status, reference)."""
    n, m = lp["n"], lp["m"]
    A, basic, status, xval = _engine_state(lp, s)
    is_int = np.concatenate([np.ones(n, bool), np.full(m, bool(con_int))])
    ref = gmi_reference(A, basic, status, xval, is_int, vars_, away, arms)
    m0 = len(s.state("csr_indptr")) - 1
    assert m0 == m
    t = s if on_self else s.clone()
    if before_call:
        before_call(t)
    t, st = t.add_gmi_cuts(vars_, np.ones(n, bool), np.ones(m, bool) if con_int else None, away)
    rows = _stored_rows(t, m0)
    worst = _compare(rows, ref, st, n + m)
    g, c = t.gmi_info(), t.cut_info()
    nemit = sum(1 for r in ref if r[0] == 0)
    assert g["requests"] == len(vars_) and g["rows"] == nemit == c["rows"] and c["rows_without_terms"] == 0
    assert g["skipped_fraction"] == sum(1 for r in ref if r[0] == 1) and g["skipped_free"] == sum(1 for r in ref if r[0] == 2)
    assert g["batches"] == c["batches"] == (len(vars_) + 15) // 16 and c["relayouts"] == (1 if nemit else 0) and c["reinversions"] <= 1
    assert g["nnz"] == sum(len(r[0]) for r in rows) == c["nnz"]
    assert t.num_constraints == m + nemit
    print("gmi round: %d requests, %d emitted, worst error / tolerance %.3g, device %.3f ms, %d pivots" %
          (len(vars_), nemit, worst, g["device_ms"], c["pivots"]))
    return t, st, ref


# ------------------------------------------------------------------------------------------------ 1: rows against the host reference
@pytest.mark.gpu
def test_rows_against_the_host_reference():
    """All variables marked, the slacks marked in one round and unmarked in another (the continuous arms need unmarked columns: every
    bound of these instances is an integer)."""
    arms = {}
    for args in INSTANCES:
        lp = lpgen.gen_mixed_lp(*args)
        s = lpgen.build_problem(M.Problem, lp).solve()
        frac = _frac_basic(s, lp["n"])
        assert len(frac) >= 10
        for slack_int in (True, False):
            t, st, ref = _against_host(lp, s, frac, slack_int, arms=arms)
            skipped = int((st != 0).sum())
            assert 10 * skipped <= len(frac), (skipped, len(frac))
    print("arms", arms)
    for a in ARMS:
        assert arms[a] > 0, (a, arms)


# ------------------------------------------------------------------------------------------------ 2: validity over rounds
@pytest.mark.gpu
@pytest.mark.parametrize("args", INSTANCES[:2], ids=str)
def test_rounds_keep_the_planted_point_and_raise_the_bound(args):
    lp = lpgen.gen_mixed_lp(*args)
    n, m0 = lp["n"], lp["m"]
    A = _dense(lp)
    z = list(_with_slacks(lp, A, _planted(*args)))       # the planted point with the slack of every row, cut rows appended below
    upper = float(lp["obj"] @ np.asarray(z[:n]))
    s = lpgen.build_problem(M.Problem, lp).solve()
    assert lp["direction"] == M.MINIMIZE
    prev = s.objective()
    scale = max(1.0, float(np.abs(lp["obj"]).max()))
    for rnd in range(3):
        frac = _frac_basic(s, n)
        assert frac
        mk = s.num_constraints
        cm = np.zeros(mk, bool)
        cm[:m0] = True                                   # the slacks of the original rows are integer, those of cut rows continuous
        s, st = s.add_gmi_cuts(frac, np.ones(n, bool), cm, 0.01)
        rows = _stored_rows(s, mk)
        assert len(rows) == int((st == 0).sum()) >= 1
        for cols, vals, rhs in rows:
            lhs = float(np.dot(vals, np.asarray(z)[cols]))
            assert lhs <= rhs + 1e-7 * max(1.0, float(np.abs(vals).sum())), (rnd, lhs, rhs)
            z.append(rhs - lhs)
        obj = s.objective()
        print("round %d: %d cuts, bound %.12g (planted point %.12g)" % (rnd + 1, len(rows), obj, upper))
        assert obj >= prev - 1e-9 * max(1.0, abs(prev)) and obj <= upper + 1e-9 * max(1.0, abs(upper))
        prev = obj
        c = s.certificate()
        assert c["btran_residual"] <= 1e-9 * scale and c["max_dual_infeasibility"] <= 1e-9 * scale and c["relative_gap"] <= 1e-9, c
        assert c["max_row_violation"] <= 1e-7 and c["max_bound_violation"] <= 1e-7, c


# ------------------------------------------------------------------------------------------------ 3: a free non-basic column
def _free_lp():
    return dict(name="free_column", direction=M.MAXIMIZE, m=2, n=3, obj=np.array([1.0, 0.0, 0.0]), lo=np.array([0.0, 0.0, -INF]),
                hi=np.array([10.0, INF, INF]), indptr=np.array([0, 1, 4], dtype=np.uint64), indices=np.array([0, 0, 1, 2], dtype=np.uint32),
                data=np.array([2.0, 1.0, 1.0, 1.0]), ops=np.array([lpgen.LE, lpgen.EQ], dtype=np.int32), rhs=np.array([3.0, 100.2]))


@pytest.mark.gpu
def test_a_free_column_in_the_row_skips_the_request():
    lp = _free_lp()
    s = lpgen.build_problem(M.Problem, lp).solve()
    vs, cs = s.basis_status()
    x = s.values()
    assert list(vs) == [M.MLP_BASIC, M.MLP_BASIC, M.MLP_NB_FREE] and abs(x[0] - 1.5) <= 1e-12 and abs(x[1] - 98.7) <= 1e-9, (vs, x)
    t, st, _ = _against_host(lp, s, [1], False)
    assert list(st) == [2] and t.num_constraints == 2 and t.gmi_info()["skipped_free"] == 1
    t, st, _ = _against_host(lp, s, [0], False)
    assert list(st) == [0] and t.num_constraints == 3
    for req, want in (([0, 1], [0, 2]), ([1, 0], [2, 0])):
        t, st, _ = _against_host(lp, s, req, False)
        assert list(st) == want and t.num_constraints == 3 and len(_stored_rows(t, 2)) == 1


# ------------------------------------------------------------------------------------------------ 4: batch independence, determinism
@pytest.mark.gpu
def test_batch_independence_and_determinism():
    lp = lpgen.gen_mixed_lp(200, 150, 8, 3)
    n, m0 = lp["n"], lp["m"]
    s = lpgen.build_problem(M.Problem, lp).solve()
    frac = [j for j in _frac_basic(s, n)]
    mk, cm = np.ones(n, bool), np.ones(m0, bool)
    ok = [j for j, st in zip(frac, s.clone().add_gmi_cuts(frac, mk, cm)[1]) if st == 0][:17]
    assert len(ok) == 17                                  # 16 + 1: across a batch edge

    def rows_of(req):
        t, st = s.clone().add_gmi_cuts(req, mk, cm)
        assert np.all(st == 0)
        return _bits(_stored_rows(t, m0))

    one = rows_of(ok)
    assert one == rows_of(ok)                             # two clones
    perm = [ok[i] for i in np.random.default_rng(5).permutation(17)]
    again = rows_of(perm)
    for t, v in enumerate(ok):
        assert rows_of([v])[0] == one[t] == again[perm.index(v)], v


# ------------------------------------------------------------------------------------------------ 5: every representation of B^-1
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


def _solved_with_pending_terms(lp, want):
    """A solved solution that holds pending rank-1 terms of the delayed-update mode, and the model it solves (the recipe of
    tests/test_cut_rounds.py: single violated bound rows until the warm-start re-solve ends with pending terms)."""
    s = lpgen.build_problem(M.Problem, lp).solve()
    bounded = []
    for t in range(1, 9):
        x = s.values()
        j = int(np.argsort(x)[-t])
        assert x[j] > 1e-3
        s = s.add_constraint([(j, 0.7)], M.LE, float(x[j]) * 0.35)
        lp = _extend(lp, [j], [0.7], lpgen.LE, float(x[j]) * 0.35)
        bounded.append(j)
        if (_pending(s) > 0) == want and t >= 2:
            break
    return s, lp, bounded


@pytest.mark.gpu
@pytest.mark.parametrize("lowrank", ["0", "3"])
def test_eager_inverse_and_pending_terms_of_the_delayed_update_mode(monkeypatch, lowrank):
    """The call is made on the solution itself: a clone has no pending terms (Engine::clone folds them first)."""
    monkeypatch.setenv("MLP_LOWRANK", lowrank)
    want = lowrank != "0"

    def check(t):
        assert int(t.state("lowrank_pending")[1]) == int(lowrank)
        assert (_pending(t) > 0) == want, _pending(t)

    s, q, bounded = _solved_with_pending_terms(lpgen.gen_sparse_lp(200, 150, 8, 3), want)
    frac = [j for j in _frac_basic(s, q["n"]) if j not in bounded]
    assert len(frac) >= 10
    _, st, _ = _against_host(q, s, frac, True, on_self=True, before_call=check)
    assert int((st == 0).sum()) >= 5


def _singleton_lp():
    """gen_mixed_lp(300, 400, 6, 3) with 60 extra columns of ONE entry each, most of them basic at the optimum (tests/test_cut_rounds.py)."""
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
def test_requested_variables_at_singleton_positions():
    lp = _singleton_lp()
    s = lpgen.build_problem(M.Problem, lp).solve()
    vs, _ = s.basis_status()
    cn = np.bincount(lp["indices"], minlength=lp["n"])
    fr = set(_frac_basic(s, lp["n"]))
    single = [j for j in range(lp["n"]) if vs[j] == M.MLP_BASIC and cn[j] == 1]
    nucleus = [j for j in range(lp["n"]) if vs[j] == M.MLP_BASIC and cn[j] > 1 and j in fr][:12]
    assert len(single) >= 3 and len(nucleus) >= 5, (len(single), len(nucleus))
    _, st, _ = _against_host(lp, s, single + nucleus, True)
    assert int((st[:len(single)] == 0).sum()) >= 1 and int((st[len(single):] == 0).sum()) >= 5, st


@pytest.mark.gpu
def test_compact_factor(monkeypatch):
    monkeypatch.setenv("MLP_FACTOR", "1")
    lp = lpgen.gen_transport_lp(600, 700, 4, 5, tight=0.45)
    s = lpgen.build_problem(M.Problem, lp).solve()
    assert s.stats()["factor_active"] == 1
    vs, _ = s.basis_status()
    basic = [j for j in range(lp["n"]) if vs[j] == M.MLP_BASIC]
    frac = _frac_basic(s, lp["n"])
    req = (frac + [j for j in basic if j not in set(frac)])[:20]
    t, st, _ = _against_host(lp, s, req, True)
    assert int((st == 0).sum()) >= 1 and t.cut_info()["reinversions"] == 1


# ------------------------------------------------------------------------------------------------ 6: refusals and no-ops
@pytest.mark.gpu
def test_refusals_and_no_ops():
    from minilp_amd import dist as md
    lp = lpgen.gen_mixed_lp(200, 150, 8, 3)
    n, m = lp["n"], lp["m"]
    prob = lpgen.build_problem(M.Problem, lp)
    s = prob.solve()
    vs, _ = s.basis_status()
    basic = _frac_basic(s, n)
    nonbasic = [j for j in range(n) if vs[j] != M.MLP_BASIC]
    mk = np.ones(n, bool)

    def refused(f, t=None):
        t = s.clone() if t is None else t
        with pytest.raises(M.InternalError) as e:
            f(t)
        assert e.value.code == -1
        assert not t._h.value                                        # consumed, as the other mutators do

    refused(lambda t: t.add_gmi_cuts([basic[0], n], mk))                        # out of range
    refused(lambda t: t.add_gmi_cuts([basic[0], nonbasic[0]], mk))              # not basic
    unmarked = mk.copy()
    unmarked[basic[1]] = False
    refused(lambda t: t.add_gmi_cuts([basic[0], basic[1]], unmarked))           # not marked integer
    refused(lambda t: t.add_gmi_cuts([basic[0], basic[1], basic[0]], mk))       # duplicate
    refused(lambda t: t.add_gmi_cuts([basic[0]], np.ones(n - 1, bool)))         # mask lengths that do not fit
    refused(lambda t: t.add_gmi_cuts([basic[0]], np.ones(n + 1, bool)))
    refused(lambda t: t.add_gmi_cuts([basic[0]], mk, np.ones(m + 1, bool)))
    for away in (0.0, -0.1, 0.51, math.nan):
        refused(lambda t: t.add_gmi_cuts([basic[0]], mk, None, away))
    refused(lambda t: t.add_gmi_cuts([0], mk), prob.solve(budget=5))            # not solved
    s2 = prob.solve(budget=0)
    box = md.create_mailbox(1)
    try:
        s2.enable_sharding_ex(0, 1, box, "pump")
        refused(lambda t: t.add_gmi_cuts([basic[0]], mk), s2)                   # sharded
    finally:
        md.remove_mailbox(box)
    # no-ops: n == 0, and a call in which every request is skipped
    x = s.values()
    near = [j for j in basic if min(x[j] - math.floor(x[j]), math.ceil(x[j]) - x[j]) < 0.3]
    assert len(near) >= 2
    for req, away in (([], 0.01), (near, 0.3)):
        t = s.clone()
        before = (_model(t), np.float64(t.objective()).tobytes(), list(t.basis_head()))
        t, st = t.add_gmi_cuts(req, mk, None, away)
        assert (_model(t), np.float64(t.objective()).tobytes(), list(t.basis_head())) == before
        assert np.all(st == 1) and len(st) == len(req)
        g, c = t.gmi_info(), t.cut_info()
        assert c["relayouts"] == 0 and c["rows"] == 0 and g["rows"] == 0 and g["skipped_fraction"] == len(req) == g["requests"]
        assert t.num_constraints == m
    t, st = s.clone().add_gmi_cuts(basic, mk, None, 0.49)
    assert int((st == 1).sum()) > len(basic) // 2 and not np.any(st == 2), st   # most fractions are within 0.49 of an integer
    assert t.gmi_info()["skipped_fraction"] == int((st == 1).sum()) and t.num_constraints == m + int((st == 0).sum())


# ------------------------------------------------------------------------------------------------ 7: the generation has no side effects
@pytest.mark.gpu
def test_generation_leaves_other_solutions_alone():
    lp = lpgen.gen_mixed_lp(200, 150, 8, 3)
    n, m = lp["n"], lp["m"]
    s = lpgen.build_problem(M.Problem, lp).solve(trace=True)
    frac = _frac_basic(s, n)
    x = s.values()
    j, val = frac[0], math.floor(x[frac[0]])
    twin = s.clone().fix_var(j, val)                       # what a clone does when no GMI call was ever made
    want = (twin.trace(), np.float64(twin.objective()).tobytes())
    assert len(want[0]) > 0
    keep, again = s.clone(), s.clone()                     # taken before the call
    ip0, ix0, dv0 = keep.tableau_rows(frac)
    n0 = len(s.trace())
    s, st = s.add_gmi_cuts(frac, np.ones(n, bool), np.ones(m, bool))
    assert int((st == 0).sum()) >= 10
    ip1, ix1, dv1 = keep.tableau_rows(frac)
    assert ip0.tobytes() == ip1.tobytes() and ix0.tobytes() == ix1.tobytes() and dv0.tobytes() == dv1.tobytes()
    keep = keep.fix_var(j, val)
    assert (keep.trace(), np.float64(keep.objective()).tobytes()) == want
    # and the same round on the other clone: the same rows, the same re-solve
    k0 = len(again.trace())
    again, st2 = again.add_gmi_cuts(frac, np.ones(n, bool), np.ones(m, bool))
    assert list(st2) == list(st) and _bits(_stored_rows(again, m)) == _bits(_stored_rows(s, m))
    assert again.trace()[k0:] == s.trace()[n0:] and np.float64(again.objective()).tobytes() == np.float64(s.objective()).tobytes()


# ------------------------------------------------------------------------------------------------ 8: a measurement (recorded, not asserted)
@pytest.mark.gpu
def test_generation_time_against_the_gomory_round():
    """device_ms per cut of add_gmi_cuts against add_gomory_cuts on the same 64 requests of gen_mixed_lp(6000, 10000, 4, 3): median of 5
    after a warm-up, one process.  Written to profiles/gmi_cuts.json when MLP_WRITE_PROFILES=1; nothing is asserted on the times."""
    lp = lpgen.gen_mixed_lp(6000, 10000, 4, 3)
    n, m = lp["n"], lp["m"]
    s = lpgen.build_problem(M.Problem, lp).solve()
    vs, _ = s.basis_status()
    frac = _frac_basic(s, n)
    req = (frac + [j for j in range(n) if vs[j] == M.MLP_BASIC and j not in set(frac)])[:64]   # (the requests of tests/test_cut_rounds.py)
    assert len(req) == 64
    mk = np.ones(n, bool)
    gmi, gom, emitted = [], [], 0
    for rep in range(6):
        t, st = s.clone().add_gmi_cuts(req, mk, np.ones(m, bool))
        u = s.clone().add_gomory_cuts(req)
        if rep:
            gmi.append(t.gmi_info()["device_ms"])
            gom.append(u.cut_info()["device_ms"])
        emitted = int((st == 0).sum())
    rec = dict(instance="gen_mixed_lp(6000, 10000, 4, 3)", requests=64, emitted=emitted, batches=4,
               gmi_device_ms=float(np.median(gmi)), gomory_device_ms=float(np.median(gom)),
               gmi_us_per_cut=float(np.median(gmi)) * 1e3 / 64, gomory_us_per_cut=float(np.median(gom)) * 1e3 / 64,
               ratio=float(np.median(gmi) / np.median(gom)), bytes=t.gmi_info()["bytes"])
    print("gmi generation:", json.dumps(rec))
    assert emitted >= 1 and rec["gmi_device_ms"] > 0 and rec["gomory_device_ms"] > 0
    if os.environ.get("MLP_WRITE_PROFILES") == "1":
        with open(os.path.join(ROOT, "profiles", "gmi_cuts.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


# ------------------------------------------------------------------------------------------------ the example driver
@pytest.mark.gpu
def test_solve_mps_example_runs_gmi_rounds(tmp_path, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("solve_mps_example_gmi", os.path.join(ROOT, "examples", "solve_mps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lp = lpgen.gen_mixed_lp(40, 30, 6, 9)
    path = tmp_path / "mixed.mps"
    path.write_text(lpgen.to_mps(lp))
    plain = lpgen.build_problem(M.Problem, lp).solve().objective()
    assert mod.run(M, str(path), gmi_rounds=2, continuous=["X3", "X7"]) == 0
    out = capsys.readouterr().out
    rounds = re.findall(r"gmi round (\d+): (\d+) cuts emitted, (\d+) skipped \(fraction\) \+ (\d+) skipped \(free column\), bound (\S+),", out)
    assert [r[0] for r in rounds] == ["1", "2"] and int(rounds[0][1]) >= 10, out
    assert float(rounds[0][4]) >= plain - 1e-9 * abs(plain) and float(rounds[1][4]) >= float(rounds[0][4]) - 1e-9 * abs(plain)
    assert "'skipped_free'" in out and "'relayouts': 1" in out
    assert mod.run(M, str(path), gmi_rounds=1, continuous=["NOPE"]) == 1
