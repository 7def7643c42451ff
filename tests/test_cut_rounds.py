"""A round of cuts in one call (include/minilp_hip.h: mlp_solution_add_constraints_csr, mlp_solution_add_gomory_cuts, mlp_cut_info;
csrc/cuts.inc).

CPU: the entry points exist in the header, the library, the Python mirror and the Rust crates; the ABI version is still 5.  GPU: a batch
leaves the model of the sequential form and reaches the oracle's optimum; the Gomory rows of a round against a host reference (dense solve
of the basis); a round of one against the single cut; validity of whole rounds; every representation of B^-1; determinism and batch
independence; refusals; the TSP subtour bound; a measurement.

Rule for a Gomory coefficient (the cut's known discontinuity, tests/test_hip_parity.py::test_gomory_cuts_are_valid_cuts): device and host
agree to 1e-9, OR the host's alpha is within 1e-9 of an integer and the difference is within 1e-9 of 0 or +-1.  On the three instances of
the host-reference test no entry other than those the host computes as exactly 0 may take the second arm.

"Computes as exactly 0": many tableau entries of these instances are zero by cancellation, not by pattern, and a floating-point host
returns +-1e-16 .. 1e-33 for them (measured on the MI355X run of this test with a sparse LU on the host: e.g. host alpha -6.96e-18 against
device f -1.05e-17, host alpha 5.45e-16 against device f -1; every second-arm entry seen was of this kind, none larger than 1.6e-15 in
|alpha|).  The host therefore sets to 0 what lies within the rounding error of its own solve and dot product,
64 eps |rho|_inf |a_j|_1 (~1.4e-14 times the magnitude of the terms): a bound from the reference's own arithmetic, far below the 4.8e-6
distance to an integer of the nearest genuine coefficient."""
import ctypes
import json
import math
import os
import re
import time

import numpy as np
import pytest

import minilp_amd as M
from minilp_amd import api, build as mbuild, lpgen
from tests.common import ROOT, X_ATOL, check_feasible, obj_close, objective_of

INF = math.inf
NEW = ["mlp_solution_add_constraints_csr", "mlp_solution_add_gomory_cuts", "mlp_solution_cut_info", "mlp_cut_info_size"]
GOMORY_INSTANCES = [(40, 30, 6, 9), (200, 150, 8, 3), (600, 500, 10, 5)]


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
    api_py = open(os.path.join(ROOT, "minilp_amd", "api.py")).read()
    surface = open(os.path.join(ROOT, "integration", "rust", "API_SURFACE.md")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(ctypes.CDLL(M.lib_path()), n), n
        assert n in api_py, n
        assert re.search(r"pub fn %s\s*\(" % n, sys_rs), n
    assert "typedef struct mlp_cut_info" in hdr
    for n in ("add_constraints", "add_gomory_cuts"):
        assert re.search(r"pub fn %s\s*\(self" % n, lib_rs), n
        assert re.search(r"\* `pub fn %s\(self, .*-> Result<Self, Error>`" % n, surface.split("### extensions")[1]), n
    for n in ("add_constraints", "add_constraints_csr", "add_gomory_cuts", "cut_info"):
        assert hasattr(M.Solution, n), n


def test_abi_version_is_still_5_and_the_struct_size_matches(L):
    assert L.mlp_abi_version() == 5 == api.ABI_VERSION
    assert L.mlp_cut_info_size() == ctypes.sizeof(api.MlpCutInfo) == 80


def test_null_handles_are_einval_not_a_crash(L):
    null = ctypes.c_void_p()
    v = np.zeros(2, dtype=np.uint32)
    assert L.mlp_solution_add_constraints_csr(None, 0, None, None, None, None, None) == -1
    assert L.mlp_solution_add_constraints_csr(ctypes.byref(null), 0, None, None, None, None, None) == -1
    assert L.mlp_solution_add_gomory_cuts(None, v.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 2) == -1
    assert L.mlp_solution_add_gomory_cuts(ctypes.byref(null), v.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 2) == -1
    assert L.mlp_solution_cut_info(None, ctypes.byref(api.MlpCutInfo())) == -1
    assert not null.value


# ------------------------------------------------------------------------------------------------ helpers
def _model(s):
    """The model as the engine holds it: CSR with the slack entries, right-hand sides, bounds and costs of all variables."""
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


def _singleton_lp():
    """gen_mixed_lp(300, 400, 6, 3) with 60 extra columns of ONE entry each, most of them basic at the optimum (tests/test_ranging.py)."""
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


def _second_feasible_point(lp, x):
    """Another vertex of the feasible set: the optimum of a perturbed objective (oracle)."""
    from oracle import minilp_oracle as O
    for seed in range(8):
        rng = np.random.default_rng(100 + seed)
        q = dict(lp, obj=lp["obj"] * rng.uniform(0.2, 3.0, size=lp["n"]))
        try:
            z = lpgen.build_problem(O.Problem, q).solve().values()
        except Exception:
            continue
        if np.abs(z - x).max() > 1e-3:
            return z
    raise AssertionError("no second feasible point found")


def _violated_rows(lp, x, z, R, seed, prefer=()):
    """R random rows violated at x and satisfied by w = x + 0.3 (z - x) (feasible by convexity, so the batch is feasible): mixed
    <= / >= / =, plus one row without terms that is a tautology (placed second when R >= 2)."""
    rng = np.random.default_rng(seed)
    w = x + 0.3 * (z - x)
    moved = np.flatnonzero(np.abs(w - x) > 1e-6)
    rows = []
    t = 0
    while len(rows) < R:
        t += 1
        k = int(rng.integers(2, 7))
        idx = set(int(j) for j in rng.choice(lp["n"], size=k, replace=False))
        idx.add(int(rng.choice(moved)))
        if len(prefer) and t % 2 == 0:
            idx.add(int(rng.choice(prefer)))
        idx = sorted(idx)
        a = np.round(rng.uniform(-2.0, 2.0, size=len(idx)), 3)
        a[a == 0.0] = 1.0
        ax, aw = float(a @ x[idx]), float(a @ w[idx])
        if abs(ax - aw) < 1e-4:
            continue
        kind = t % 5
        op = M.EQ if kind == 0 else (M.LE if aw < ax else M.GE)
        rows.append((list(zip(idx, a.tolist())), op, aw))
    if R >= 2:
        rows.insert(1, ([], M.LE, 1.0))
    return rows


def _unique_optimum(s):
    """No non-basic variable or slack (other than fixed ones) has a zero reduced cost / dual value: the optimal vertex is the only optimum."""
    vs, cs = s.basis_status()
    r, pi = np.asarray(s.reduced_costs()), np.asarray(s.dual_values())
    nbv = (vs != M.MLP_BASIC) & (vs != M.MLP_NB_FIXED)
    nbc = (cs != M.MLP_BASIC) & (cs != M.MLP_NB_FIXED)
    return bool(np.all(np.abs(r[nbv]) > 1e-7) and np.all(np.abs(pi[nbc]) > 1e-7))


def _frac_basic(s, n):
    x = s.values()
    vs, _ = s.basis_status()
    return [j for j in range(n) if vs[j] == M.MLP_BASIC and abs(x[j] - round(x[j])) > 1e-6]


def _host_cuts(lp, s, vars_):
    """Rows of the Gomory cuts of `vars_` at the basis of s, dense numpy solve: {var: (alpha[N], f[N] (0 on basic), rhs)}."""
    m, n = lp["m"], lp["n"]
    A = np.zeros((m, n + m))
    ip, ix, dt = lp["indptr"], lp["indices"], lp["data"]
    for i in range(m):
        A[i, ix[ip[i]:ip[i + 1]]] = dt[ip[i]:ip[i + 1]]
        A[i, n + i] = 1.0
    bv = s.state("host_basic_vars").astype(np.int64)
    pos = np.full(n + m, -1)
    pos[bv] = np.arange(m)
    B = A[:, bv]
    x = s.values()
    xall = np.concatenate([x, lp["rhs"] - A[:, :n] @ x])
    E = np.zeros((m, len(vars_)))
    for t, v in enumerate(vars_):
        assert pos[v] >= 0
        E[pos[v], t] = 1.0
    import scipy.sparse as sp
    from scipy.sparse.linalg import splu
    RHO = splu(sp.csc_matrix(B.T)).solve(E)   # rows of B^-1, as columns (a sparse LU keeps the structural zeros exact)
    out = {}
    for t, v in enumerate(vars_):
        alpha = RHO[:, t] @ A
        # what the host itself cannot tell from 0: the rounding error of its own solve and dot product.  A backward-stable solve leaves
        # every component of rho with an error of at least eps |rho|_inf (times the condition number), so alpha_j carries
        # eps |rho|_inf |a_j|_1; the factor 64 covers the length of the sums and the conditioning of these bases (eps = 2^-52)
        alpha[np.abs(alpha) <= 64.0 * 2.0 ** -52 * np.abs(RHO[:, t]).max() * np.abs(A).sum(axis=0)] = 0.0
        f = np.floor(alpha) - alpha
        f[bv] = 0.0
        alpha[bv] = 0.0
        xb = xall[v]
        out[v] = (alpha, f, math.floor(xb) - xb)
    return out


def _compare_row(row, ref, N, strict):
    """One stored cut against the host's; returns the number of entries that needed the second arm and are no exact host zeros."""
    cols, vals, rhs = row
    alpha, f, rhs_ref = ref
    assert np.all(np.diff(cols) > 0), "terms sorted by variable"
    assert np.all(vals != 0.0), "no stored zero"
    assert abs(rhs - rhs_ref) <= 1e-9
    dev = np.zeros(N)
    dev[cols] = vals
    diff = dev - f
    ok = np.abs(diff) <= 1e-9
    near_int = np.abs(alpha - np.round(alpha)) <= 1e-9
    arm2 = ~ok & near_int & ((np.abs(diff - 1.0) <= 1e-9) | (np.abs(diff + 1.0) <= 1e-9))
    assert np.all(ok | arm2), (np.flatnonzero(~(ok | arm2))[:5], diff[~(ok | arm2)][:5])
    taken = int((arm2 & (alpha != 0.0)).sum())
    for j in np.flatnonzero(arm2 & (alpha != 0.0))[:5]:
        print("   second arm: variable %d host alpha %.17g host f %.17g device f %.17g" % (j, alpha[j], f[j], dev[j]))
    if strict:
        assert taken == 0, taken
    return taken


def _rows_close(a, b, N):
    """Two stored rows under the same rule, without a host alpha: equal to 1e-9, or off by +-1 where one of them is within 1e-9 of 0 / -1."""
    da, db = np.zeros(N), np.zeros(N)
    da[a[0]] = a[1]
    db[b[0]] = b[1]
    d = da - db
    ok = np.abs(d) <= 1e-9
    edge = (np.minimum(np.abs(da), np.abs(da + 1.0)) <= 1e-9) | (np.minimum(np.abs(db), np.abs(db + 1.0)) <= 1e-9)
    assert np.all(ok | (edge & (np.abs(np.abs(d) - 1.0) <= 1e-9))), d[~ok][:5]
    assert abs(a[2] - b[2]) <= 1e-9


# ------------------------------------------------------------------------------------------------ 1: batch == sequential == oracle
def _batch_vs_sequential(lp, R, seed, prefer=(), check_oracle=True, expect_unique=False, prepared=None, before_call=None):
    """prepared: two identically prepared solutions of lp (the batch runs on the first ITSELF, not on a clone: Engine::clone folds the
    pending rank-1 terms); before_call(solution) asserts the state the case is about right before the batched call."""
    from oracle import minilp_oracle as O
    if prepared is None:
        s0 = lpgen.build_problem(M.Problem, lp).solve()
        a, b = s0.clone(), s0.clone()
    else:
        s0, b = prepared
        a = s0
    x = s0.values()
    z = _second_feasible_point(lp, x)
    rows = _violated_rows(lp, x, z, R, seed, prefer)
    m0 = s0.num_constraints
    if before_call:
        before_call(a)
    a = a.add_constraints(rows)
    info = a.cut_info()
    for e, op, r in rows:
        b = b.add_constraint(e, op, r)
    print("R=%d  batch obj %.12g pivots %d reinv %d wall %.2f ms | sequential obj %.12g" %
          (R, a.objective(), info["pivots"], info["reinversions"], info["wall_ms"], b.objective()))
    assert obj_close(a.objective(), b.objective())
    assert a.num_constraints == b.num_constraints == m0 + len(rows)
    assert len(a.dual_values()) == len(b.dual_values()) == m0 + len(rows)
    assert _model(a) == _model(b)
    cert = a.certificate()
    assert abs(cert["relative_gap"]) <= 1e-7 and max(cert["max_row_violation"], cert["max_bound_violation"],
                                                     cert["max_dual_infeasibility"]) <= 1e-7, cert
    assert info["rows"] == R and info["relayouts"] == 1 and info["reinversions"] <= 1, info
    assert info["rows_without_terms"] == (1 if R >= 2 else 0)
    if check_oracle:
        o = lpgen.build_problem(O.Problem, lp).solve()
        for e, op, r in rows:
            if e:
                o = o.add_constraint(e, op, r)
        assert obj_close(a.objective(), o.objective()) and obj_close(b.objective(), o.objective())
        unique = _unique_optimum(a)
        assert unique or not expect_unique          # (the comparison of x below must run on the families whose optimum is unique)
        if unique:                                  # (|dx| <= 1e-7 is the contract on unique optima)
            assert np.abs(a.values() - o.values()).max() <= X_ATOL
        else:
            print("   optimum not unique (a non-basic variable with a zero reduced cost): x not compared")
    return a, info


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 2, 16, 17, 40])
@pytest.mark.parametrize("family,args", [("sparse", (400, 300, 12, 7)), ("dense", (60, 50, 2)), ("mixed", (300, 400, 6, 3)),
                                         ("twophase", (300, 260, 8, 6)), ("cover", (70, 90, 5, 5)), ("singleton", ())],
                         ids=["sparse", "dense", "mixed", "twophase", "cover", "singleton-columns"])
def test_batch_is_the_sequential_model_and_the_oracles_optimum(family, args, R):
    gen = {"sparse": lpgen.gen_sparse_lp, "dense": lpgen.gen_dense_lp, "mixed": lpgen.gen_mixed_lp, "twophase": lpgen.gen_twophase_lp,
           "cover": lpgen.gen_cover_lp, "singleton": _singleton_lp}[family]
    lp = gen(*args)
    prefer = np.arange(lp["n"] - 60, lp["n"]) if family == "singleton" else ()
    # x is compared with the oracle's on unique optima only; on these four families the optimum IS unique, so the comparison must run
    _, info = _batch_vs_sequential(lp, R, 7 * R + 1, prefer, expect_unique=family in ("sparse", "dense", "twophase", "cover"))
    if family == "singleton" and R >= 16:
        assert info["reinversions"] == 1          # some row touched a basic singleton column: one re-inversion for the whole batch


@pytest.mark.gpu
def test_an_infeasible_batch_raises_and_consumes():
    lp = lpgen.gen_sparse_lp(400, 300, 12, 7)
    s = lpgen.build_problem(M.Problem, lp).solve()
    x = s.values()
    j = int(np.argmax(x))
    with pytest.raises(M.Infeasible):
        t = s.clone()
        t.add_constraints([([(j, 1.0)], M.GE, float(x[j]) + 1.0), ([(j, 1.0)], M.LE, float(x[j]) - 1.0)])
    assert not t._h.value
    with pytest.raises(M.Infeasible):               # the first row alone is feasible, the third is not
        t = s.clone()
        t.add_constraints([([(j, 1.0)], M.LE, float(x[j]) * 0.5), ([(0, 1.0), (1, 1.0)], M.LE, 1e6), ([(j, 1.0)], M.LE, lp["lo"][j] - 1.0)])
    assert not t._h.value
    with pytest.raises(M.Infeasible):               # a row without terms that is no tautology
        t = s.clone()
        t.add_constraints([([(j, 1.0)], M.LE, float(x[j]) * 0.5), ([], M.GE, 1.0)])
    assert not t._h.value
    assert s.add_constraints([([(j, 1.0)], M.LE, float(x[j]) * 0.5)]).cut_info()["rows"] == 1


# ------------------------------------------------------------------------------------------------ 2: Gomory rows against the host
def _gomory_against_host(lp, s, vars_, strict, on_self=False, before_call=None):
    """on_self: the round is added to s itself (consumed), not to a clone — Engine::clone folds the pending rank-1 terms."""
    ref = _host_cuts(lp, s, vars_)
    m0 = len(s.state("csr_indptr")) - 1
    N = lp["n"] + lp["m"]
    t = s if on_self else s.clone()
    if before_call:
        before_call(t)
    t = t.add_gomory_cuts(vars_)
    rows = _stored_rows(t, m0)
    info = t.cut_info()
    assert len(rows) + info["rows_without_terms"] == len(vars_)
    assert info["rows_without_terms"] == 0 and info["batches"] == (len(vars_) + 15) // 16 and info["relayouts"] == 1, info
    taken = 0
    ncoef = 0
    for v, row in zip(vars_, rows):
        assert len(row[0]) == 0 or row[0].max() < N               # terms on the variables of the model the call found
        taken += _compare_row(row, ref[v], N, strict)
        ncoef += lp["n"]
    print("gomory rows: %d cuts, %d coefficients, %d second-arm entries, device %.3f ms, %d pivots" %
          (len(vars_), ncoef, taken, info["device_ms"], info["pivots"]))
    return t, info


@pytest.mark.gpu
@pytest.mark.parametrize("args", GOMORY_INSTANCES, ids=str)
def test_gomory_rows_against_a_host_reference(args):
    lp = lpgen.gen_sparse_lp(*args)
    s = lpgen.build_problem(M.Problem, lp).solve()
    frac = _frac_basic(s, lp["n"])
    assert len(frac) >= 10, len(frac)
    _, info = _gomory_against_host(lp, s, frac, strict=True)
    assert info["rows"] == len(frac) and info["reinversions"] == 0


# ------------------------------------------------------------------------------------------------ 3: a round of one is the single cut
@pytest.mark.gpu
@pytest.mark.parametrize("args", GOMORY_INSTANCES, ids=str)
def test_a_round_of_one_is_the_single_cut(args):
    lp = lpgen.gen_sparse_lp(*args)
    s = lpgen.build_problem(M.Problem, lp).solve()
    m0 = lp["m"]
    N = lp["n"] + m0
    for v in _frac_basic(s, lp["n"])[:4]:
        a = s.clone().add_gomory_cuts([v])
        b = s.clone().add_gomory_cut(v)
        ra, rb = _stored_rows(a, m0), _stored_rows(b, m0)
        assert len(ra) == len(rb) == 1
        _rows_close(ra[0], rb[0], N)
        assert obj_close(a.objective(), b.objective())
        assert a.num_constraints == b.num_constraints == m0 + 1


# ------------------------------------------------------------------------------------------------ 4: validity of a round
@pytest.mark.gpu
def test_rounds_of_gomory_cuts_are_valid_cuts():
    lp = lpgen.gen_sparse_lp(40, 30, 6, 9)
    s = lpgen.build_problem(M.Problem, lp).solve()
    n, m0 = lp["n"], lp["m"]
    y = np.floor(s.values() + 1e-9)
    check_feasible(lp, y)
    lower = objective_of(lp, y)
    prev = s.objective()
    rounds = 0
    for _ in range(3):
        x = s.values()
        frac = _frac_basic(s, n)
        if not frac:
            break
        s = s.add_gomory_cuts(frac)
        rounds += 1
        assert s.objective() <= prev + 1e-9 * abs(prev)                     # (a Maximize family: the bound never improves)
        assert s.objective() >= lower - 1e-9 * abs(lower)                   # the integer point floor(x*) is kept by every cut
        assert np.abs(s.values() - x).max() > 1e-9                          # the fractional vertex was cut off
        check_feasible(lp, s.values())
        prev = s.objective()
    assert rounds >= 1
    assert lp["direction"] == M.MAXIMIZE


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
    """A SOLVED solution that holds pending rank-1 terms of the delayed-update mode, and the model it solves.  After a primal solve the
    lazily kept dual weights are stale, and the first thing a warm start does (ensure_beta) folds the pending terms to rebuild them; the
    dual pivots of a warm-start re-solve keep the weights current, so what THEY leave pending stays until the next call.  Hence: solve,
    then add single violated bound rows (the existing single form) until the re-solve ends with pending terms.  Deterministic: two calls
    return the same state.  want = False (MLP_LOWRANK=0): the same steps, and there are never pending terms."""
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
def test_pending_terms_of_the_delayed_update_mode(monkeypatch, lowrank):
    """Items 1 (R = 17) and 2 with MLP_LOWRANK in {0, 3}.  The calls are made on the solution itself: a clone has no pending terms
    (Engine::clone folds them first).  Under MLP_LOWRANK=3 the state read `lowrank_pending` must show pending terms right before each
    batched call, so the rows of B^-1 are taken through their rank-1 terms (rg_w with nlow > 0) and not from a folded inverse."""
    monkeypatch.setenv("MLP_LOWRANK", lowrank)
    want = lowrank != "0"

    def check(t):
        cap = int(t.state("lowrank_pending")[1])
        assert cap == int(lowrank)
        assert (_pending(t) > 0) == want, (_pending(t), cap)

    s, q, bounded = _solved_with_pending_terms(lpgen.gen_sparse_lp(200, 150, 8, 3), want)
    # (a variable held by a one-term row has a tableau row of one entry: its cut has no fractional part to work with)
    frac = [j for j in _frac_basic(s, q["n"]) if j not in bounded]
    assert len(frac) >= 10
    _gomory_against_host(q, s, frac, strict=True, on_self=True, before_call=check)
    base = lpgen.gen_sparse_lp(400, 300, 12, 7)
    a, q, _ = _solved_with_pending_terms(base, want)
    b, _, _ = _solved_with_pending_terms(base, want)
    _batch_vs_sequential(q, 17, 5, prepared=(a, b), before_call=check)


@pytest.mark.gpu
def test_requested_variables_at_singleton_positions():
    lp = _singleton_lp()
    s = lpgen.build_problem(M.Problem, lp).solve()
    vs, _ = s.basis_status()
    cn = np.bincount(lp["indices"], minlength=lp["n"])
    single = [j for j in range(lp["n"]) if vs[j] == M.MLP_BASIC and cn[j] == 1]
    nucleus = [j for j in range(lp["n"]) if vs[j] == M.MLP_BASIC and cn[j] > 1][:12]
    assert len(single) >= 3 and len(nucleus) >= 5, (len(single), len(nucleus))
    _gomory_against_host(lp, s, single + nucleus, strict=False)


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
    single = s.clone().add_gomory_cut(req[0])
    t, info = _gomory_against_host(lp, s, req, strict=False)
    assert info["reinversions"] == 1
    if single.stats()["factor_active"] == 1:
        assert t.stats()["factor_active"] == 1
    a, info = _batch_vs_sequential(lp, 17, 3)
    assert a.stats()["factor_active"] == 1 and info["reinversions"] == 1


# ------------------------------------------------------------------------------------------------ 6: determinism, independence, no-op
def _bits(rows):
    return [(c.tobytes(), v.tobytes(), np.float64(r).tobytes()) for c, v, r in rows]


def _blob(s):
    b = s.save_basis(2)
    return b[:48] + b[56:]  # (header bytes 48..56: the solution's pivot counter, which a clone starts from zero)


@pytest.mark.gpu
def test_determinism_batch_independence_and_the_empty_call():
    lp = lpgen.gen_sparse_lp(600, 500, 10, 5)
    s = lpgen.build_problem(M.Problem, lp).solve(trace=True)
    m0 = lp["m"]
    frac = _frac_basic(s, lp["n"])
    assert len(frac) >= 33
    one = _bits(_stored_rows(s.clone().add_gomory_cuts(frac), m0))
    two = _bits(_stored_rows(s.clone().add_gomory_cuts(frac), m0))
    assert one == two
    v, others = frac[20], frac[:16]
    alone = _bits(_stored_rows(s.clone().add_gomory_cuts([v]), m0))[0]
    first = _bits(_stored_rows(s.clone().add_gomory_cuts([v] + others), m0))[0]
    last = _bits(_stored_rows(s.clone().add_gomory_cuts(others + [v]), m0))[16]
    assert alone == first == last == one[20]
    # the empty call: the checkpoint is byte-identical, and the solution continues pivot for pivot like an untouched clone
    a = lpgen.build_problem(M.Problem, lp).solve(budget=150, trace=True)
    b = a.clone()
    blob = a.save_basis(2)
    with pytest.raises(M.InternalError):
        a.clone().add_gomory_cuts([0])            # (not solved: refused, checked here so that the empty call below is seen to differ)
    u = s.clone()
    ublob = u.save_basis(2)
    u = u.add_gomory_cuts([]).add_constraints([]).add_constraints_csr([0], [], [], [], [])
    assert u.save_basis(2) == ublob
    assert u.cut_info()["rows"] == 0
    a = a.add_gomory_cuts([]).add_constraints([])
    assert a.save_basis(2) == blob and _blob(a) == _blob(b)
    na, nb = len(a.trace()), len(b.trace())
    a.continue_solve(200); b.continue_solve(200)
    assert a.trace()[na:] == b.trace()[nb:] and np.float64(a.objective()).tobytes() == np.float64(b.objective()).tobytes()


# ------------------------------------------------------------------------------------------------ 7: refusals
@pytest.mark.gpu
def test_refusals():
    from minilp_amd import dist as md
    lp = lpgen.gen_sparse_lp(400, 300, 12, 7)
    prob = lpgen.build_problem(M.Problem, lp)
    s = prob.solve()
    vs, _ = s.basis_status()
    basic = [j for j in range(lp["n"]) if vs[j] == M.MLP_BASIC]
    nonbasic = [j for j in range(lp["n"]) if vs[j] != M.MLP_BASIC]

    def refused(f):
        t = s.clone()
        with pytest.raises(M.InternalError) as e:
            f(t)
        assert e.value.code == -1
        assert not t._h.value                                        # consumed, as the single forms do

    refused(lambda t: t.add_gomory_cuts([basic[0], nonbasic[0]]))     # not basic
    refused(lambda t: t.add_gomory_cuts([basic[0], basic[1], basic[0]]))  # duplicate
    refused(lambda t: t.add_gomory_cuts([basic[0], lp["n"]]))         # out of range
    refused(lambda t: t.add_constraints([([(0, 1.0)], M.LE, 1e9), ([(1, 1.0), (1, 2.0)], M.LE, 1e9)]))   # duplicate variable in a row
    refused(lambda t: t.add_constraints([([(0, 1.0)], M.LE, 1e9), ([(lp["n"], 1.0)], M.LE, 1e9)]))      # out of range
    u = prob.solve(budget=5)
    assert u.budget_exhausted
    with pytest.raises(M.InternalError):
        u.add_constraints([([(0, 1.0)], M.LE, 1e9)])
    u = prob.solve(budget=5)
    with pytest.raises(M.InternalError):
        u.add_gomory_cuts([0])
    s2 = prob.solve(budget=0)
    box = md.create_mailbox(1)
    try:
        s2.enable_sharding_ex(0, 1, box, "pump")
        with pytest.raises(M.InternalError) as e:
            s2.add_constraints([([(0, 1.0)], M.LE, 1e9)])
        assert e.value.code == -1
    finally:
        md.remove_mailbox(box)


# ------------------------------------------------------------------------------------------------ 8: TSP
@pytest.mark.gpu
def test_tsp_subtour_bound_with_batched_cuts():
    import importlib.util
    spec = importlib.util.spec_from_file_location("tsp_example_cut_rounds", os.path.join(ROOT, "examples", "tsp.py"))
    tsp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tsp)
    _, pts = tsp.read_tsplib(os.path.join(ROOT, "tests", "golden", "bn130.tsp"))
    out = {}
    for batch in (False, True):
        t = tsp.TspSolver(M, pts, batch_cuts=batch)
        sol = t.relaxation()
        out[batch] = (sol.objective(), dict(t.stats))
    print("tsp bn130 subtour relaxation:", out)
    assert obj_close(out[True][0], out[False][0])
    assert out[True][1]["lp_solves"] < out[False][1]["lp_solves"]


# ------------------------------------------------------------------------------------------------ 9: measurement
def _median(xs):
    return float(np.median(np.asarray(xs)))


@pytest.mark.gpu
def test_generation_of_a_round_against_the_single_forms_row():
    """64 Gomory rows (57 on config 2, which has no more basic structural variables at its optimum): generation time per cut of the
    batched call (cut_info().device_ms / requests, median of 5 after one warm-up) against what
    the single form spends per cut before it appends and re-solves (wall of add_gomory_cut minus the stats' solve_wall_s delta, which
    covers add_constraint: the tableau row, its copy to the host and the host loop remain).  The two are not like for like (device time
    against host wall time), so the batched call's wall time by the same yardstick — wall of add_gomory_cuts minus the solve_wall_s
    delta: launches, syncs, buffer allocation, the copies of lengths and sparse rows — is recorded next to them.  Asserted: 4 batches, and the batched
    generation per cut is below the single form's on both instances.  Numbers go to profiles/cut_rounds.json when MLP_WRITE_PROFILES=1."""
    res = {}
    for name, lp in (("config2_dense_1000x1000", lpgen.gen_dense_lp(1000, 1000, 2)), ("config3_mixed_6000x10000", lpgen.gen_mixed_lp(6000, 10000, 4, 3))):
        s = lpgen.build_problem(M.Problem, lp).solve()
        vs, _ = s.basis_status()
        frac = _frac_basic(s, lp["n"])
        basic = [j for j in range(lp["n"]) if vs[j] == M.MLP_BASIC]
        req = (frac + [j for j in basic if j not in set(frac)])[:64]
        assert 49 <= len(req) <= 64           # (config 2 has 57 basic structural variables at its optimum: all of them, still 4 batches)
        gen_ms, gen_wall = [], []
        for it in range(6):
            c = s.clone()
            w0 = c.stats()["solve_wall_s"]
            t0 = time.perf_counter()
            t = c.add_gomory_cuts(req)
            wall = time.perf_counter() - t0
            info = t.cut_info()
            assert info["batches"] == 4 and info["relayouts"] == 1
            if it:
                gen_ms.append(info["device_ms"])
                gen_wall.append((wall - (t.stats()["solve_wall_s"] - w0)) * 1e3)   # the same yardstick as the single form's below
        single = []
        for it in range(6):
            c = s.clone()
            w0 = c.stats()["solve_wall_s"]
            t0 = time.perf_counter()
            c = c.add_gomory_cut(req[it])
            wall = time.perf_counter() - t0
            if it:
                single.append((wall - (c.stats()["solve_wall_s"] - w0)) * 1e3)
        per_cut, one = _median(gen_ms) / len(req), _median(single)
        res[name] = {"batched_generation_ms_per_cut": per_cut, "requests": len(req), "batched_generation_ms_round": _median(gen_ms),
                     "single_form_row_ms_per_cut": one, "ratio_single_over_batched": one / per_cut,
                     "batched_generation_wall_ms_per_cut": _median(gen_wall) / len(req),
                     "ratio_single_over_batched_wall": one / (_median(gen_wall) / len(req)), "bytes": info["bytes"],
                     "cut_nnz": info["nnz"], "resolve_pivots": info["pivots"]}
        print(name, res[name])
        assert per_cut < one, res[name]
    # recorded, not asserted: 16 general rows in one call against one at a time (config 3)
    lp = lpgen.gen_mixed_lp(6000, 10000, 4, 3)
    s = lpgen.build_problem(M.Problem, lp).solve()
    x = s.values()
    rng = np.random.default_rng(1)
    rows = []
    nz = np.flatnonzero(x > 1e-3)
    for _ in range(16):
        idx = sorted(set(int(j) for j in rng.choice(nz, size=4, replace=False)))
        rows.append(([(j, 1.0) for j in idx], M.LE, float(x[idx].sum()) * 0.9))
    for rep in range(2):
        a = s.clone()
        t0 = time.perf_counter()
        a = a.add_constraints(rows)
        wa = (time.perf_counter() - t0) * 1e3
        b = s.clone()
        i0 = b.stats()["iterations"]
        t0 = time.perf_counter()
        for e, op, r in rows:
            b = b.add_constraint(e, op, r)
        wb = (time.perf_counter() - t0) * 1e3
    assert obj_close(a.objective(), b.objective())
    res["config3_16_general_rows"] = {"batched_wall_ms": wa, "batched_pivots": a.cut_info()["pivots"], "sequential_wall_ms": wb,
                                      "sequential_pivots": int(b.stats()["iterations"] - i0)}
    print(res["config3_16_general_rows"])
    if os.environ.get("MLP_WRITE_PROFILES") == "1":
        with open(os.path.join(ROOT, "profiles", "cut_rounds.json"), "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
