"""Dual values, reduced costs and the KKT certificate of a Solution (include/minilp_hip.h: mlp_solution_dual_values ...).

CPU: the entry points exist in the header, the library, the Python mirror and the Rust crates.  GPU: the known answer of the
lib.rs doc example, finite differences of the oracle's objective, a host KKT check in every representation of B^-1, the committed
certificate fixture, no side effects of a read (bit for bit, delayed-update mode included), warm starts, determinism, refusal on a
sharded solution, and a measurement at config-4 size."""
import ctypes
import gzip
import math
import os
import re
import time

import numpy as np
import pytest

import minilp_amd as M
from minilp_amd import api, build as mbuild, lpgen
from tests.common import ROOT

INF = math.inf
MID = os.path.join(ROOT, "tests", "golden", "cfg4_basis_p45000.bin.gz")
LATE = os.path.join(ROOT, "tests", "golden", "cfg4_basis_p240000.bin.gz")
NEW = ["mlp_solution_num_constraints", "mlp_solution_dual_values", "mlp_solution_dual_value", "mlp_solution_reduced_costs",
       "mlp_solution_reduced_cost", "mlp_solution_certificate", "mlp_certificate_size"]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(M.lib_path()):
        mbuild.build(verbose=False)
    return M.lib()


# ------------------------------------------------------------------------------------------------ CPU
def test_header_declares_and_library_exports_the_new_entry_points(L):
    hdr = open(os.path.join(ROOT, "include", "minilp_hip.h")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(ctypes.CDLL(M.lib_path()), n), n
    assert "typedef struct mlp_certificate" in hdr
    assert L.mlp_abi_version() == 5 == api.ABI_VERSION
    assert L.mlp_certificate_size() == ctypes.sizeof(api.MlpCertificate)


def test_python_solution_has_the_new_methods():
    for n in ("num_constraints", "dual_values", "dual_value", "reduced_costs", "reduced_cost", "certificate"):
        assert hasattr(M.Solution, n), n


def test_rust_crates_declare_and_call_the_new_functions():
    sys_rs = open(os.path.join(ROOT, "integration", "rust", "minilp-hip-sys", "src", "lib.rs")).read()
    for n in NEW:
        assert re.search(r"pub fn %s\s*\(" % n, sys_rs), n
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "minilp", "src", "lib.rs")).read()
    for n in ("mlp_solution_num_constraints", "mlp_solution_dual_value", "mlp_solution_reduced_cost"):
        assert re.search(r"sys::%s\s*\(" % n, lib_rs), n
    for n in ("num_constraints", "dual_value", "reduced_cost"):
        assert re.search(r"pub fn %s\s*\(" % n, lib_rs), n


def test_null_solution_is_einval_not_a_crash(L):
    d = ctypes.c_double()
    buf = np.zeros(4)
    assert L.mlp_solution_num_constraints(None) == 0
    assert L.mlp_solution_dual_values(None, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 4) == -1
    assert L.mlp_solution_dual_value(None, 0, ctypes.byref(d)) == -1
    assert L.mlp_solution_reduced_costs(None, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 4) == -1
    assert L.mlp_solution_reduced_cost(None, 0, ctypes.byref(d)) == -1
    c = api.MlpCertificate()
    assert L.mlp_solution_certificate(None, ctypes.byref(c)) == -1


# ------------------------------------------------------------------------------------------------ host reference of the KKT terms
def _csr(lp):
    import scipy.sparse as sp
    A = sp.csr_matrix((lp["data"], lp["indices"], lp["indptr"]), shape=(lp["m"], lp["n"]))
    return A


def host_kkt(lp, s, fixed=()):
    """Host check of (x, pi, r): returns a dict of the certificate's terms computed with scipy, in the user's sense."""
    x, pi, r = s.values(), s.dual_values(), s.reduced_costs()
    A = _csr(lp)
    c, b, lo, hi, ops = lp["obj"], lp["rhs"], lp["lo"].copy(), lp["hi"].copy(), lp["ops"]
    for j in fixed:
        lo[j] = hi[j] = x[j]
    sg = -1.0 if lp["direction"] == M.MAXIMIZE else 1.0
    r_host = c - A.T @ pi
    act = A @ x
    sx = b - act                                               # slack values
    slo = np.where(ops == lpgen.LE, 0.0, np.where(ops == lpgen.GE, -INF, 0.0))
    shi = np.where(ops == lpgen.LE, INF, 0.0)
    rs = -pi                                                    # reduced costs of the slacks (cost 0, coefficient +1)

    def lag(rm, l_lo, l_hi, xv):
        ell = np.where(rm > 0, l_lo, np.where(rm < 0, l_hi, xv))
        inf = np.isinf(ell)
        ell = np.where(inf, xv, ell)
        return float(np.sum(np.where(rm == 0, 0.0, rm * ell))), float(np.max(np.where(inf & (rm != 0), np.abs(rm), 0.0), initial=0.0))

    t1, i1 = lag(sg * r, lo, hi, x)
    t2, i2 = lag(sg * rs, slo, shi, sx)
    primal = float(c @ x)
    dual = sg * (float(b @ (sg * pi)) + t1 + t2)
    viol = np.maximum(np.maximum(slo - sx, sx - shi), 0.0)
    return dict(x=x, pi=pi, r=r, r_host=r_host, primal=primal, dual=dual, dual_inf=max(i1, i2), row_viol=float(viol.max(initial=0.0)),
                gap=abs(primal - dual) / max(1.0, abs(primal)))


def check_kkt(lp, s, optimal=True, fixed=(), tol=1e-9):
    h = host_kkt(lp, s, fixed)
    cert = s.certificate()
    scale = max(1.0, float(np.abs(lp["obj"]).max()))
    basic = h["r"] == 0.0
    # r matches c - A^T pi (non-basic: the same number; basic: zero up to the accuracy of pi)
    assert np.abs(h["r"] - np.where(basic, 0.0, h["r_host"])).max() <= 1e-9 * scale
    assert np.abs(h["r_host"][basic]).max(initial=0.0) <= cert["btran_residual"] + 1e-12 * scale
    # the device certificate agrees with the host's formula
    assert abs(cert["primal_objective"] - h["primal"]) <= 1e-10 * max(1.0, abs(h["primal"]))
    assert abs(cert["dual_objective"] - h["dual"]) <= 1e-10 * max(1.0, abs(h["dual"])), (cert, h["dual"])
    assert abs(cert["max_dual_infeasibility"] - h["dual_inf"]) <= 1e-10 * scale
    assert cert["max_row_violation"] <= h["row_viol"] + 1e-9 and h["row_viol"] <= cert["max_row_violation"] + 1e-9
    if optimal:
        assert cert["btran_residual"] <= 1e-9 * scale
        assert cert["max_dual_infeasibility"] <= tol * scale and cert["relative_gap"] <= tol, cert
        assert h["gap"] <= tol
        sg = -1.0 if lp["direction"] == M.MAXIMIZE else 1.0
        pm = sg * h["pi"]
        assert (pm[lp["ops"] == lpgen.LE] <= tol * scale).all() and (pm[lp["ops"] == lpgen.GE] >= -tol * scale).all()
    return cert


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
    assert s.num_constraints == 2
    assert np.allclose(s.dual_values(), [1.0, 0.0], atol=1e-12, rtol=0)
    assert s.dual_values()[1] == 0.0                                     # basic slack: exactly zero
    assert np.allclose(s.reduced_costs(), [0.0, 1.0], atol=1e-12, rtol=0)
    assert s.reduced_cost(0) == 0.0 and s.dual_value(0) == pytest.approx(1.0)
    c = s.certificate()
    assert c["relative_gap"] <= 1e-12 and c["max_dual_infeasibility"] == 0.0 and c["max_row_violation"] <= 1e-12
    assert c["primal_objective"] == pytest.approx(7.0) and c["dual_objective"] == pytest.approx(7.0)
    # Minimize twin with an '=' row whose dual is negative: min x + 2y, -x - y = -4, 2x + y >= 2 -> x = 4, y = 0, objective 4
    p = M.Problem(M.MINIMIZE)
    x = p.add_var(1.0, (0.0, INF))
    y = p.add_var(2.0, (0.0, 3.0))
    p.add_constraint([(x, -1.0), (y, -1.0)], M.EQ, -4.0)
    p.add_constraint([(x, 2.0), (y, 1.0)], M.GE, 2.0)
    s = p.solve()
    assert s.objective() == pytest.approx(4.0)
    pi = s.dual_values()
    assert pi[0] == pytest.approx(-1.0) and pi[1] == 0.0                 # d obj / d rhs_0 = -1 (rhs -4 -> -3: x = 3)
    assert np.allclose(s.reduced_costs(), [0.0, 1.0], atol=1e-12, rtol=0)
    assert s.certificate()["relative_gap"] <= 1e-12


def _oracle_obj(lp, O):
    try:
        return lpgen.build_problem(O.Problem, lp).solve().objective()
    except Exception:
        return None


@pytest.mark.gpu
@pytest.mark.parametrize("family,args", [("mixed", (60, 80, 5, 3)), ("sparse", (400, 300, 12, 7)), ("cover", (70, 90, 5, 5))])
def test_finite_differences_against_the_oracle(family, args):
    from oracle import minilp_oracle as O
    gen = {"mixed": lpgen.gen_mixed_lp, "sparse": lpgen.gen_sparse_lp, "cover": lpgen.gen_cover_lp}[family]
    lp = gen(*args)
    s = lpgen.build_problem(M.Problem, lp).solve()
    pi, r, x = s.dual_values(), s.reduced_costs(), s.values()
    f0 = _oracle_obj(lp, O)
    assert abs(f0 - s.objective()) <= 1e-9 * max(1.0, abs(f0))
    h = 1e-5
    rng = np.random.default_rng(7)
    rows = rng.choice(lp["m"], size=min(20, lp["m"]), replace=False)
    ok = 0
    for i in rows:
        vals = []
        for sgn in (1, -1):
            q = dict(lp, rhs=lp["rhs"].copy())
            q["rhs"][i] += sgn * h
            vals.append(_oracle_obj(q, O))
        if None in vals:
            continue
        fwd, bwd = (vals[0] - f0) / h, (f0 - vals[1]) / h
        if abs(fwd - bwd) > 1e-6 * max(1.0, abs(fwd)):
            continue                                                        # a basis change inside [rhs - h, rhs + h]
        ok += 1
        assert abs((vals[0] - vals[1]) / (2 * h) - pi[i]) <= 1e-6 * max(1.0, abs(pi[i])), (i, pi[i], fwd, bwd)
    assert ok >= 0.8 * len(rows), (ok, len(rows))
    # reduced costs of non-basic variables: move the bound they sit at (central difference; skipped where the basis changes)
    nb = [j for j in range(lp["n"]) if r[j] != 0.0 and (x[j] == lp["lo"][j] or x[j] == lp["hi"][j]) and lp["lo"][j] < lp["hi"][j]]
    ok = tried = 0
    for j in nb[:10]:
        key = "lo" if x[j] == lp["lo"][j] else "hi"
        vals = []
        for sgn in (1, -1):
            q = dict(lp, lo=lp["lo"].copy(), hi=lp["hi"].copy())
            q[key][j] += sgn * h
            vals.append(_oracle_obj(q, O))
        tried += 1
        if None in vals or abs((vals[0] - f0) - (f0 - vals[1])) > 1e-6 * h * max(1.0, abs(r[j])):
            continue
        ok += 1
        assert abs((vals[0] - vals[1]) / (2 * h) - r[j]) <= 1e-6 * max(1.0, abs(r[j])), (j, r[j])
    assert ok >= 0.8 * tried, (ok, tried)


@pytest.mark.gpu
@pytest.mark.parametrize("family,args", [("mixed", (300, 400, 6, 3)), ("sparse", (400, 300, 12, 7)), ("cover", (2000, 3000, 6, 5))],
                         ids=["explicit-mixed", "explicit-sparse", "hypersparse-cover"])
def test_host_kkt_explicit_and_hypersparse(family, args):
    gen = {"mixed": lpgen.gen_mixed_lp, "sparse": lpgen.gen_sparse_lp, "cover": lpgen.gen_cover_lp}[family]
    lp = gen(*args)
    s = lpgen.build_problem(M.Problem, lp).solve()
    check_kkt(lp, s)
    if family == "cover":
        assert s.stats()["hyper_iters"] > 0


@pytest.mark.gpu
def test_host_kkt_compact_factor(monkeypatch):
    monkeypatch.setenv("MLP_FACTOR", "1")
    lp = lpgen.gen_transport_lp(600, 700, 4, 5, tight=0.45)
    s = lpgen.build_problem(M.Problem, lp).solve()
    assert s.stats()["factor_active"] == 1
    check_kkt(lp, s)
    # mid-solve on the factor, with pending rank-1 terms
    s = lpgen.build_problem(M.Problem, lp).solve(budget=70)
    assert s.stats()["factor_active"] == 1
    check_kkt(lp, s, optimal=False)
    assert s.certificate()["btran_residual"] <= 1e-9


@pytest.fixture(scope="module")
def cfg4():
    lp = lpgen.gen_sparse_lp(100000, 100000, 100, 4)
    return lp, lpgen.build_problem(M.Problem, lp)


def _load(prob, path, **kw):
    with gzip.open(path, "rb") as f:
        return prob.solve_from_basis(f.read(), budget=0, **kw)


@pytest.mark.gpu
def test_delayed_mode_pending_terms_kkt_and_no_side_effects(cfg4):
    lp, prob = cfg4
    a = _load(prob, MID, trace=True)
    a.continue_solve(10)                                               # pending rank-1 terms of the delayed-update mode
    assert a.stats()["nucleus_size"] >= 9000
    b = a.clone()
    blob0 = a.save_basis(2)
    cert = check_kkt(lp, a, optimal=False)
    assert cert["btran_residual"] <= 1e-7 * max(1.0, float(np.abs(lp["obj"]).max())), cert
    assert a.save_basis(2) == blob0 and _blob(a) == _blob(b)
    a, b = _same_step(a, b, lambda s: (s.continue_solve(40), s)[1])
    assert _blob(a) == _blob(b)


@pytest.mark.gpu
def test_committed_fixture_duals():
    z = np.load(os.path.join(ROOT, "tests", "golden", "cfg_small_certificate.npz"))
    lp = lpgen.gen_sparse_lp(2000, 2000, 20, 4)
    s = lpgen.build_problem(M.Problem, lp).solve()
    y = np.zeros(lp["m"])
    y[z["y_idx"]] = z["y_val"]
    assert np.abs(s.dual_values() - y).max() <= 1e-8
    c = s.certificate()
    assert c["relative_gap"] <= 1e-12 and c["max_dual_infeasibility"] <= 1e-9, c
    check_kkt(lp, s)


def _bits(s, n0):
    """Pivots recorded since index n0 and the objective, as bits."""
    return [tuple(np.float64(v).tobytes() if isinstance(v, float) else v for v in t) for t in s.trace()[n0:]], np.float64(s.objective()).tobytes()


def _blob(s):
    b = s.save_basis(2)
    return b[:48] + b[56:]  # (header bytes 48..56: the solution's pivot counter, which a clone starts from zero)


def _same_step(a, b, f):
    """Apply the same mutator to both solutions; the pivots it takes and the objective must be bit-identical."""
    na, nb = len(a.trace()), len(b.trace())
    a, b = f(a), f(b)
    assert _bits(a, na) == _bits(b, nb)
    return a, b


@pytest.mark.gpu
def test_reading_has_no_side_effects_through_every_mutator():
    lp = lpgen.gen_mixed_lp(300, 400, 6, 3)
    a = lpgen.build_problem(M.Problem, lp).solve(trace=True)
    b = a.clone()
    blob = a.save_basis(2)
    a.dual_values(); a.reduced_costs(); a.certificate()
    assert a.save_basis(2) == blob and _blob(a) == _blob(b)
    x = a.values()
    basic = [j for j in range(lp["n"]) if a.reduced_cost(j) == 0.0 and abs(x[j] - round(x[j])) > 1e-6]
    a, b = _same_step(a, b, lambda s: s.add_gomory_cut(basic[0]))
    a.certificate()
    rhs = float(x[0] + x[1]) - 0.25
    a, b = _same_step(a, b, lambda s: s.add_constraint([(0, 1.0), (1, 1.0)], M.LE, rhs))
    a.dual_values()
    j = int(np.argmax(np.abs(a.values())))
    v = float(a.values()[j])
    a, b = _same_step(a, b, lambda s: s.fix_var(j, v))
    assert _blob(a) == _blob(b)


@pytest.mark.gpu
def test_warm_start_grows_the_dual_vector_and_keeps_kkt():
    lp = lpgen.gen_mixed_lp(300, 400, 6, 3)
    s = lpgen.build_problem(M.Problem, lp).solve()
    m0 = s.num_constraints
    assert m0 == lp["m"] and len(s.dual_values()) == m0
    x = s.values()
    s = s.add_constraint([(0, 1.0), (1, 1.0)], M.LE, float(x[0] + x[1]) - 0.5)
    assert s.num_constraints == m0 + 1 and len(s.dual_values()) == m0 + 1
    lp2 = _extend(lp, [0, 1], [1.0, 1.0], lpgen.LE, float(x[0] + x[1]) - 0.5)
    check_kkt(lp2, s)
    x = s.values()
    frac = [j for j in range(lp["n"]) if s.reduced_cost(j) == 0.0 and abs(x[j] - round(x[j])) > 1e-6]
    if frac:
        s = s.add_gomory_cut(frac[0])
        assert s.num_constraints == m0 + 2 and len(s.dual_values()) == m0 + 2
        c = s.certificate()
        assert c["relative_gap"] <= 1e-9 and c["max_dual_infeasibility"] <= 1e-9 and c["max_row_violation"] <= 1e-7, c
    # fix_var: the fixed variable has a finite reduced cost, KKT holds with its bounds closed
    s = lpgen.build_problem(M.Problem, lp).solve()
    x = s.values()
    j = next(j for j in range(lp["n"]) if s.reduced_cost(j) == 0.0 and lp["lo"][j] < x[j] < lp["hi"][j])
    s = s.fix_var(j, float(x[j]) + 0.25 if x[j] + 0.25 <= lp["hi"][j] else float(x[j]) - 0.25)
    assert math.isfinite(s.reduced_cost(j))
    check_kkt(lp, s, fixed=[j])


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
def test_reads_are_deterministic_and_sharded_solutions_are_refused():
    from minilp_amd import dist as md
    lp = lpgen.gen_sparse_lp(1500, 1400, 12, 9)
    prob = lpgen.build_problem(M.Problem, lp)
    s = prob.solve(budget=300)
    t = s.clone()
    assert s.dual_values().tobytes() == t.dual_values().tobytes()
    assert s.reduced_costs().tobytes() == t.reduced_costs().tobytes()
    c1, c2 = s.certificate(), t.certificate()
    for k in c1:
        if k != "device_ms":
            assert np.float64(c1[k]).tobytes() == np.float64(c2[k]).tobytes(), k
    s2 = prob.solve(budget=0)
    box = md.create_mailbox(1)
    try:
        s2.enable_sharding_ex(0, 1, box, "pump")
        with pytest.raises(M.InternalError) as e:
            s2.dual_values()
        assert e.value.code == -1
        with pytest.raises(M.InternalError):
            s2.certificate()
    finally:
        md.remove_mailbox(box)
    buf = np.zeros(3)
    assert M.lib().mlp_solution_dual_values(s._h, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 3) == -1  # wrong length


@pytest.mark.gpu
def test_config4_scale_measurement(cfg4):
    lp, prob = cfg4
    s = _load(prob, LATE)
    assert s.stats()["nucleus_size"] == 20493
    t = time.perf_counter()
    pi = s.dual_values()
    wall = time.perf_counter() - t
    c = s.certificate()
    assert len(pi) == lp["m"] and np.isfinite(pi).all()
    assert c["btran_residual"] <= 1e-6 * max(1.0, float(np.abs(lp["obj"]).max())), c
    gbs = c["bytes"] / (c["device_ms"] * 1e-3) / 1e9
    print(f"config 4, k = 20 493: certificate {c['bytes'] / 1e9:.3f} GB in {c['device_ms']:.3f} ms on the device = {gbs:.0f} GB/s "
          f"({gbs / 6300:.2f} of 6.3 TB/s); dual_values() wall {wall * 1e3:.1f} ms; btran residual {c['btran_residual']:.2e}")
