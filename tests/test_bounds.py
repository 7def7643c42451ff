"""New bounds for the structural variables of a solved model (include/minilp_hip.h: mlp_solution_set_var_bounds,
mlp_solution_tighten_by_reduced_cost, mlp_solution_var_bounds, mlp_bounds_info; csrc/bounds.inc).

The yardstick of set_var_bounds is the cold solve of the model with the new bounds: the oracle's (status, objective to OBJ_RTOL, x to
X_ATOL where the optimum is unique) and scipy's HiGHS (objective to HIGHS_RTOL).  gen_mixed_lp has alternative optima: there the point
must be feasible for the new bounds and carry the objective.  The bound lists are built by `bound_list` from a solved point and its
basis statuses: the CPU tests build them from the oracle's optimum and check the two yardsticks against each other; the GPU tests build
them from the engine's optimum (the same vertex wherever the optimum is unique) and hold the engine to both yardsticks.  The host KKT
check of tests/test_degenerate.py is written for Minimize instances; sparse-maximize is held to the certificate alone.

A refused call (MLP_EINVAL) frees the handle like every mutator of the library: "left bit-identical" is checked on the solution the
refused clone was taken from.  The refusal of a request that makes infinite the bound a non-basic column sits at is not pinned here."""
import ctypes
import importlib.util
import json
import math
import os
import re
import time

import numpy as np
import pytest

import minilp_amd as M
from minilp_amd import api, build as mbuild, lpgen
from tests.bounded_lp import gen_bounded_lp
from tests.common import HIGHS_RTOL, OBJ_RTOL, ROOT, X_ATOL, check_feasible, obj_close
from tests.test_branch_penalties import INSTANCES, KNAPSACK_SEEDS, _blob, _hand_lp, _knapsack
from tests.test_fixing import _gap_and_cutoff
from tests.test_ranging import _highs_obj

INF = math.inf
NEW = ["mlp_solution_set_var_bounds", "mlp_solution_tighten_by_reduced_cost", "mlp_solution_var_bounds", "mlp_solution_bounds_info",
       "mlp_bounds_info_size"]
BOUND_INSTANCES = {"mixed": INSTANCES["mixed"], "sparse-maximize": INSTANCES["sparse-maximize"], "cover": INSTANCES["cover"],
                   "bounded": (gen_bounded_lp, (300, 400, 6, 3))}
UNIQUE = ("cover", "sparse-maximize", "bounded")
KINDS = ("floor", "ceil", "inward", "outward", "narrow", "widen", "free", "mixed")
LENGTHS = (0, 1, 16, 17, 64, 257)
KKT_TOL = 1e-7


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(M.lib_path()):
        mbuild.build(verbose=False)
    return M.lib()


def _lp(name):
    gen, args = BOUND_INSTANCES[name]
    return gen(*args)


# ------------------------------------------------------------------------------------------------ the bound lists
def bound_list(lp, x, vs, kind, k):
    """(vars, lo, hi): at most k requests of one kind at the point x with variable statuses vs (MLP_BASIC ...).
    floor / ceil   basic fractional columns: the upper bound down to floor(x), the lower bound up to ceil(x)
    inward         the bound a non-basic column sits at moved into its range (the column moves with it)
    outward        ... moved out of its range by 0.5 (finite)
    narrow         a box of half width 0.01 around a basic value, inside the old bounds (nothing moves)
    widen          the finite bounds of a column moved out by 1 (basic and non-basic columns, lo == hi columns included)
    free           columns without any bound get the box [x + 0.25, x + 2]: a non-basic one is clamped, a basic one violates
    mixed          all of the above in turn: basic and non-basic requests, columns at upper bounds and free columns in one list (two
                   branches of each direction at most: a long list of branches is infeasible on every instance)"""
    n, lo, hi = lp["n"], lp["lo"], lp["hi"]
    frac = [j for j in range(n) if vs[j] == 0 and abs(x[j] - round(x[j])) > 1e-3]
    atb = [j for j in range(n) if vs[j] in (1, 2) and lo[j] < hi[j]]
    atb = [j for j in atb if vs[j] == 2] + [j for j in atb if vs[j] == 1]              # the columns at upper bounds first
    step = lambda j: 1e-3 * (min(1.0, hi[j] - lo[j]) if math.isfinite(hi[j] - lo[j]) else 1.0)
    one = {
        "floor": ([j for j in frac if math.floor(x[j]) >= lo[j]], lambda j: (lo[j], float(math.floor(x[j])))),
        "ceil": ([j for j in frac if math.ceil(x[j]) <= hi[j]], lambda j: (float(math.ceil(x[j])), hi[j])),
        "inward": (atb, lambda j: (lo[j] + step(j), hi[j]) if vs[j] == 1 else (lo[j], hi[j] - step(j))),
        "outward": (atb, lambda j: (lo[j] - 0.5, hi[j]) if vs[j] == 1 else (lo[j], hi[j] + 0.5)),
        "narrow": ([j for j in range(n) if vs[j] == 0], lambda j: (max(lo[j], x[j] - 0.01), min(hi[j], x[j] + 0.01))),
        "widen": ([j for j in range(n) if math.isfinite(lo[j]) or math.isfinite(hi[j])], lambda j: (lo[j] - 1.0, hi[j] + 1.0)),
        "free": ([j for j in range(n) if math.isinf(lo[j]) and math.isinf(hi[j])], lambda j: (x[j] + 0.25, x[j] + 2.0)),
    }
    js, los, his = [], [], []
    if kind != "mixed":
        pool, f = one[kind]
        js = pool[:k]
        los, his = [f(j)[0] for j in js], [f(j)[1] for j in js]
    else:
        order = ("floor", "inward", "widen", "ceil", "outward", "free", "narrow")
        used, t, dry = set(), 0, 0
        while len(js) < k and dry < len(order):
            kd = order[t % len(order)]
            pool, f = one[kd]
            t += 1
            if kd in ("floor", "ceil") and t > 2 * len(order):
                pool = []
            left = [j for j in pool if j not in used]
            if not left:
                dry += 1
                continue
            dry = 0
            j = left[len(left) // 2] if t % 2 else left[0]
            used.add(j)
            js.append(j)
            los.append(f(j)[0])
            his.append(f(j)[1])
    return [int(j) for j in js], [float(a) for a in los], [float(b) for b in his]


def _with_bounds(lp, js, los, his):
    lo, hi = np.array(lp["lo"], dtype=float), np.array(lp["hi"], dtype=float)
    lo[js], hi[js] = los, his
    return dict(lp, lo=lo, hi=hi)


_COLD = {}


def _cold(lp2, key):
    """(oracle solution or None when Infeasible, HiGHS objective or None) of the model with the new bounds, computed once per key."""
    from oracle import minilp_oracle as O
    if key not in _COLD:
        try:
            o = lpgen.build_problem(O.Problem, lp2).solve()
        except O.Infeasible:
            o = None
        _COLD[key] = (o, _highs_obj(lp2))
    return _COLD[key]


def _oracle_status(o, lp):
    n, x = lp["n"], o.values()
    basic = set(int(v) for v in o.state("basic_vars"))
    return np.array([0 if j in basic else (1 if x[j] == lp["lo"][j] else (2 if x[j] == lp["hi"][j] else 3)) for j in range(n)])


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
    assert "typedef struct mlp_bounds_info" in hdr and "Still version 5: the bound changes" in hdr
    args = re.search(r"pub fn mlp_solution_tighten_by_reduced_cost\s*\(([^)]*)\)", sys_rs).group(1)
    assert [a.split(":")[0].strip() for a in args.split(",")] == ["s", "cutoff", "var_is_int", "num_vars", "tightened", "pruned"]
    assert re.search(r"pub fn set_var_bounds\s*\(self", lib_rs) and re.search(r"pub fn tighten_by_reduced_cost\s*\(self", lib_rs)
    assert re.search(r"pub fn var_bounds\s*\(&self", lib_rs)
    ext = surface.split("### extensions")[1]
    for n in ("set_var_bounds", "tighten_by_reduced_cost", "var_bounds"):
        assert re.search(r"\* `pub fn %s\(&?self, .*`" % n, ext), n
    for n in ("set_var_bounds", "tighten_by_reduced_cost", "var_bounds", "bounds_info"):
        assert hasattr(M.Solution, n), n
    assert "infinite" in hdr.split("mlp_solution_set_var_bounds gives")[1].split("*/")[0]        # the refusal is written into the header


def test_abi_version_is_still_5_and_the_struct_size_matches(L):
    assert L.mlp_abi_version() == 5 == api.ABI_VERSION
    assert L.mlp_bounds_info_size() == ctypes.sizeof(api.MlpBoundsInfo) == 80
    assert L.mlp_fix_info_size() == 96                                                  # no existing struct grew


def test_null_handle_is_einval_not_a_crash(L):
    h = ctypes.c_void_p()
    v, a, b = np.zeros(1, dtype=np.uint32), np.zeros(1), np.ones(1)
    pu, pd = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_double)
    pv, pa, pb = v.ctypes.data_as(pu), a.ctypes.data_as(pd), b.ctypes.data_as(pd)
    cnt, pr = ctypes.c_uint64(7), ctypes.c_int(7)
    assert L.mlp_solution_set_var_bounds(ctypes.byref(h), pv, pa, pb, 1) == -1
    assert L.mlp_solution_set_var_bounds(None, pv, pa, pb, 0) == -1
    assert L.mlp_solution_tighten_by_reduced_cost(ctypes.byref(h), 1.0, None, 0, ctypes.byref(cnt), ctypes.byref(pr)) == -1
    assert L.mlp_solution_tighten_by_reduced_cost(None, 1.0, None, 0, ctypes.byref(cnt), ctypes.byref(pr)) == -1
    assert L.mlp_solution_var_bounds(None, pv, 1, pa, pb) == -1
    assert L.mlp_solution_bounds_info(None, ctypes.byref(api.MlpBoundsInfo())) == -1


@pytest.mark.parametrize("name", list(BOUND_INSTANCES))
def test_the_two_yardsticks_agree_on_every_bound_list(name):
    """The oracle's cold solve of the model with the new bounds and HiGHS: the same verdict, the objective to HIGHS_RTOL — on every
    kind of list at 16 requests and on the mixed list at every length, built from the oracle's optimum."""
    from oracle import minilp_oracle as O
    lp = _lp(name)
    o = lpgen.build_problem(O.Problem, lp).solve()
    x, vs = o.values(), _oracle_status(o, lp)
    optimal = infeasible = 0
    for kind, k in [(kd, 16) for kd in KINDS] + [("mixed", k) for k in LENGTHS]:
        js, los, his = bound_list(lp, x, vs, kind, k)
        assert len(js) == len(set(js)) and all(a <= b for a, b in zip(los, his)), (name, kind, k)
        if kind == "mixed":
            assert len(js) == min(k, len(js)) and (len(js) == k or name == "cover"), (name, k, len(js))
        oc, hg = _cold(_with_bounds(lp, js, los, his), ("cpu", name, kind, k))
        assert (oc is None) == (hg is None), (name, kind, k, oc is None, hg)
        if oc is None:
            infeasible += 1
        else:
            optimal += 1
            assert obj_close(oc.objective(), hg, HIGHS_RTOL), (name, kind, k, oc.objective(), hg)
    print("%s: %d lists optimal, %d infeasible by both" % (name, optimal, infeasible))
    assert optimal >= 6


def test_the_mixed_list_mixes_what_it_should():
    """One list holds basic and non-basic requests, columns at upper bounds and free columns (gen_mixed_lp), and the bounded instance
    offers lo == hi columns to the widening."""
    from oracle import minilp_oracle as O
    lp = _lp("mixed")
    o = lpgen.build_problem(O.Problem, lp).solve()
    x, vs = o.values(), _oracle_status(o, lp)
    js, los, his = bound_list(lp, x, vs, "mixed", 64)
    assert len(js) == 64
    assert any(vs[j] == 0 for j in js) and any(vs[j] == 1 for j in js) and any(vs[j] == 2 for j in js)
    assert any(math.isinf(lp["lo"][j]) and math.isinf(lp["hi"][j]) for j in js)
    lb = _lp("bounded")
    assert any(lb["lo"][j] == lb["hi"][j] for j in bound_list(lb, np.zeros(lb["n"]), np.zeros(lb["n"], int), "widen", 64)[0])


# ------------------------------------------------------------------------------------------------ GPU: shared state
_SOLVED = {}


def _solved(name):
    if name not in _SOLVED:
        lp = _lp(name)
        _SOLVED[name] = (lp, lpgen.build_problem(M.Problem, lp).solve())
    return _SOLVED[name]


def _bits(s):
    return np.float64(s.objective()).tobytes(), s.values().tobytes(), _blob(s)


def _host_kkt_is_clean(lp2, t, label):
    from tests.test_degenerate import TERMS, host_kkt
    if lp2["direction"] != M.MINIMIZE:
        return
    vs, cs = t.basis_status()
    k = host_kkt(lp2, t.values(), t.dual_values(), t.reduced_costs(), vs, cs)
    assert all(float(k[term]) <= KKT_TOL for term in TERMS), (label, {term: float(k[term]) for term in TERMS})


def _check_after(lp, t, js, los, his, label, unique, key, explicit_inverse=True):
    """Everything section 1 of the issue asks of a solution after set_var_bounds (t is None: the call said Infeasible)."""
    lp2 = _with_bounds(lp, js, los, his)
    oc, hg = _cold(lp2, key)
    assert (t is None) == (oc is None) == (hg is None), (label, t is None, oc is None, hg)
    if t is None:
        return False
    assert obj_close(t.objective(), oc.objective()) and obj_close(t.objective(), hg, HIGHS_RTOL), (label, t.objective(), oc.objective(), hg)
    x = t.values()
    check_feasible(lp2, x)
    assert obj_close(float(np.dot(lp["obj"], x)), t.objective(), 1e-8), label
    if unique:
        assert np.abs(x - oc.values()).max() <= X_ATOL, (label, float(np.abs(x - oc.values()).max()))
    _host_kkt_is_clean(lp2, t, label)
    c = t.certificate()
    assert c["relative_gap"] <= 1e-9 and c["max_dual_infeasibility"] <= 1e-9 and c["max_row_violation"] <= 1e-7 and c["max_bound_violation"] <= 1e-7, (label, c)
    vs, _ = t.basis_status()
    open_ = lp2["lo"] < lp2["hi"]
    assert (x[(vs == 1) & open_] == lp2["lo"][(vs == 1) & open_]).all() and (x[(vs == 2) & open_] == lp2["hi"][(vs == 2) & open_]).all(), label
    blo, bhi = t.var_bounds()
    assert blo.tobytes() == lp2["lo"].tobytes() and bhi.tobytes() == lp2["hi"].tobytes(), label
    assert t.state("orig_var_mins")[:lp["n"]].tobytes() == lp2["lo"].tobytes() and t.state("orig_var_maxs")[:lp["n"]].tobytes() == lp2["hi"].tobytes()
    if js:
        sub = t.var_bounds(js[:3])
        assert sub[0].tolist() == list(los[:3]) and sub[1].tolist() == list(his[:3])
    if explicit_inverse:
        assert t.reinvert() < 1e-8, label
    return True


def _apply(s, js, los, his):
    try:
        return s.set_var_bounds(js, los, his)
    except M.Infeasible:
        return None


# ------------------------------------------------------------------------------------------------ 1: against the cold solve
@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", [(nm, kd) for nm in BOUND_INSTANCES for kd in KINDS if kd != "free" or nm == "mixed"])     # (free columns: gen_mixed_lp only)
def test_set_var_bounds_against_the_cold_solve(name, kind):
    lp, s = _solved(name)
    x0 = s.values()
    vs, _ = s.basis_status()
    js, los, his = bound_list(lp, x0, vs, kind, 16)
    assert len(js) >= 4, (name, kind, len(js))
    t = _apply(s.clone(), js, los, his)
    ok = _check_after(lp, t, js, los, his, "%s %s" % (name, kind), name in UNIQUE, ("gpu", name, kind, 16))
    if ok:
        info = t.bounds_info()
        nb = sum(1 for j in js if vs[j] != 0)
        assert info["requests"] == len(js) and info["nonbasic"] == nb and info["basic"] == len(js) - nb, (name, kind, info)
        assert info["solves"] == (1 if info["shifted"] else 0), info
        if kind in ("inward", "outward"):
            assert info["shifted"] == len(js), info
        if kind == "narrow":                                                             # nothing moves: the same bits, no pivot
            assert info["shifted"] == 0 and info["pivots"] == 0 and info["solves"] == 0, info
            assert np.float64(t.objective()).tobytes() == np.float64(s.objective()).tobytes() and t.values().tobytes() == x0.tobytes()
        print("%s %s: %s" % (name, kind, info))
    else:
        print("%s %s: infeasible, as the oracle and HiGHS say" % (name, kind))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed", "bounded"])
def test_the_mixed_list_at_every_length(name):
    lp, s = _solved(name)
    vs, _ = s.basis_status()
    feasible = 0
    for k in LENGTHS:
        js, los, his = bound_list(lp, s.values(), vs, "mixed", k)
        assert len(js) == k, (name, k, len(js))
        t = _apply(s.clone(), js, los, his)
        feasible += _check_after(lp, t, js, los, his, "%s mixed %d" % (name, k), name in UNIQUE, ("gpu", name, "mixed", k))
        if t is not None:
            assert t.bounds_info()["requests"] == len(js)
            if k >= 16:
                assert t.bounds_info()["basic"] >= 1 and t.bounds_info()["nonbasic"] >= 1
    assert feasible >= 5, (name, feasible)


# ------------------------------------------------------------------------------------------------ 2: against what the parent can do
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed", "sparse-maximize", "cover"])
def test_a_bound_is_a_singleton_row_and_a_closed_box_is_a_fixing(name):
    lp, s = _solved(name)
    x = s.values()
    vs, _ = s.basis_status()
    frac = [j for j in range(lp["n"]) if vs[j] == 0 and abs(x[j] - round(x[j])) > 1e-3][:4]
    assert len(frac) == 4
    done = 0
    for j in frac:
        u = float(math.floor(x[j]))
        a = _apply(s.clone(), [j], [float(lp["lo"][j])], [u])
        try:
            b = s.clone().add_constraint([(j, 1.0)], M.LE, u)
        except M.Infeasible:
            b = None
        assert (a is None) == (b is None), (name, j)
        if a is not None:
            assert obj_close(a.objective(), b.objective()), (name, j, a.objective(), b.objective())
            done += 1
        v = float(math.ceil(x[j]))
        if not lp["lo"][j] <= v <= lp["hi"][j]:
            continue
        a = _apply(s.clone(), [j], [v], [v])
        try:
            b = s.clone().fix_var(j, v)
        except M.Infeasible:
            b = None
        assert (a is None) == (b is None), (name, j)
        if a is not None:
            assert obj_close(a.objective(), b.objective()), (name, j, a.objective(), b.objective())
            done += 1
    assert done >= 4


# ------------------------------------------------------------------------------------------------ 3: order and batch independence
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BOUND_INSTANCES))
def test_the_order_of_the_list_changes_no_bit(name):
    lp, s = _solved(name)
    vs, _ = s.basis_status()
    js, los, his = bound_list(lp, s.values(), vs, "mixed", 17)
    rng = np.random.default_rng(11)
    outs = []
    for rep in range(3):
        p = np.arange(len(js)) if rep == 0 else rng.permutation(len(js))
        t = _apply(s.clone(), [js[i] for i in p], [los[i] for i in p], [his[i] for i in p])
        outs.append(None if t is None else _bits(t) + (t.var_bounds()[0].tobytes(), t.var_bounds()[1].tobytes()))
    assert outs[0] == outs[1] == outs[2]


@pytest.mark.gpu
def test_one_call_of_64_and_64_single_calls():
    lp, s = _solved("mixed")
    vs, _ = s.basis_status()
    js, los, his = [], [], []
    for kind, k in (("widen", 24), ("outward", 16), ("narrow", 16), ("inward", 64)):      # relaxations first: the list stays feasible
        for j, a, b in zip(*bound_list(lp, s.values(), vs, kind, k)):
            if j not in js and len(js) < 64:
                js.append(j); los.append(a); his.append(b)
    js, los, his = js[:64], los[:64], his[:64]
    assert len(js) == 64
    one = s.clone().set_var_bounds(js, los, his)
    seq = s.clone()
    for j, a, b in zip(js, los, his):
        seq = seq.set_var_bounds([j], [a], [b])
    assert obj_close(one.objective(), seq.objective()), (one.objective(), seq.objective())
    assert one.var_bounds()[0].tobytes() == seq.var_bounds()[0].tobytes() and one.var_bounds()[1].tobytes() == seq.var_bounds()[1].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BOUND_INSTANCES))
def test_the_current_bounds_change_nothing(name):
    lp, s = _solved(name)
    t = s.clone()
    before = _bits(t)
    js = list(range(0, lp["n"], 3))                                                     # basic and non-basic columns
    t = t.set_var_bounds(js, lp["lo"][js], lp["hi"][js])
    info = t.bounds_info()
    assert _bits(t) == before and info["pivots"] == 0 and info["solves"] == 0 and info["shifted"] == 0 and info["requests"] == len(js), info
    assert info["basic"] >= 1 and info["nonbasic"] >= 1
    t = t.set_var_bounds([], [], [])                                                   # n == 0: a successful no-op
    assert _bits(t) == before and t.bounds_info()["requests"] == 0


# ------------------------------------------------------------------------------------------------ 4: tighten_by_reduced_cost
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed", "sparse-maximize", "cover"])
def test_tighten_by_reduced_cost_applies_the_list_of_the_read(name):
    lp, s = _solved(name)
    n, obj = lp["n"], s.objective()
    lo0, hi0 = s.var_bounds()
    assert lo0.tobytes() == np.asarray(lp["lo"], float).tobytes() and hi0.tobytes() == np.asarray(lp["hi"], float).tobytes()
    for frac in (0.0, 0.01, 0.1):
        _, cutoff = _gap_and_cutoff(obj, lp["direction"], frac)
        for marks in (None, np.ones(n, bool)):
            v, lo, hi, pruned = s.cutoff_bounds(cutoff, marks)
            assert not pruned and len(v) >= 1
            t = s.clone()
            before = _bits(t)
            t, count, pruned = t.tighten_by_reduced_cost(cutoff, marks)
            info = t.bounds_info()
            assert count == len(v) == info["tightened"] and not pruned and info["pivots"] == 0 and info["solves"] == 0 and info["shifted"] == 0, info
            blo, bhi = t.var_bounds()
            assert blo[v].tobytes() == lo.tobytes() and bhi[v].tobytes() == hi.tobytes()
            rest = np.setdiff1d(np.arange(n), v)
            assert blo[rest].tobytes() == lo0[rest].tobytes() and bhi[rest].tobytes() == hi0[rest].tobytes()
            assert _bits(t)[:2] == before[:2] and _bits(t) == before                    # objective, values and the whole blob
            assert (t.basis_status()[0] == s.basis_status()[0]).all()                  # lo == hi entries keep their plain status
            c = t.certificate()
            assert c["relative_gap"] <= 1e-9 and c["max_bound_violation"] <= 1e-7, c
            t, again, _ = t.tighten_by_reduced_cost(cutoff, marks)                     # nothing new the second time
            assert again == 0 and t.bounds_info()["tightened"] == 0 and _bits(t) == before
            assert t.var_bounds()[0].tobytes() == blo.tobytes() and t.var_bounds()[1].tobytes() == bhi.tobytes()
            u = t.clone()                                                              # a clone carries the tightened bounds
            assert u.var_bounds()[0].tobytes() == blo.tobytes() and u.var_bounds()[1].tobytes() == bhi.tobytes()
    # a pruned cutoff changes nothing
    _, worse = _gap_and_cutoff(obj, lp["direction"], -0.01)
    t = s.clone()
    before = _bits(t)
    t, count, pruned = t.tighten_by_reduced_cost(worse)
    assert pruned and count == 0 and _bits(t) == before and t.var_bounds()[0].tobytes() == lo0.tobytes() and t.var_bounds()[1].tobytes() == hi0.tobytes()


def _branch_and_bound(lp, tighten):
    """Depth-first branch and bound of a Maximize binary knapsack over set_var_bounds branches; with `tighten` every node applies the
    reduced-cost bounds of the incumbent first.  Returns (best objective, nodes)."""
    n = lp["n"]
    marks = np.ones(n, bool)
    best, nodes = -INF, 0
    stack = [lpgen.build_problem(M.Problem, lp).solve()]
    while stack:
        node = stack.pop()
        nodes += 1
        if node.objective() <= best + 1e-9:
            continue
        if tighten and best > -INF:
            node, _, pruned = node.tighten_by_reduced_cost(best, marks)
            if pruned:
                continue
        x = node.values()
        frac = [j for j in range(n) if abs(x[j] - round(x[j])) > 1e-6]
        if not frac:
            best = max(best, node.objective())
            continue
        j = frac[0]
        lo, hi = node.var_bounds([j])
        for a, b in ((float(lo[0]), float(math.floor(x[j]))), (float(math.ceil(x[j])), float(hi[0]))):
            try:
                stack.append(node.clone().set_var_bounds([j], [a], [b]))
            except M.Infeasible:
                pass
    return best, nodes


@pytest.mark.gpu
def test_branch_and_bound_reaches_the_integer_optimum_with_and_without_tightening():
    import itertools
    for seed in KNAPSACK_SEEDS:
        lp = _knapsack(seed)
        n = lp["n"]
        X = np.array(list(itertools.product((0.0, 1.0), repeat=n)))
        X = X[(X @ lp["data"].reshape(3, n).T <= lp["rhs"] + 1e-9).all(axis=1)]
        want = float((X @ lp["obj"]).max())
        plain, n0 = _branch_and_bound(lp, False)
        tight, n1 = _branch_and_bound(lp, True)
        print("%s: optimum %g, %d nodes plain, %d with tightening" % (lp["name"], want, n0, n1))
        assert abs(plain - want) <= 1e-7 and abs(tight - want) <= 1e-7, (seed, want, plain, tight)


# ------------------------------------------------------------------------------------------------ 5: every representation of B^-1
def _two_lists(lp, s):
    vs, _ = s.basis_status()
    x = s.values()
    shifted = bound_list(lp, x, vs, "inward", 16)
    basic = bound_list(lp, x, vs, "floor", 16)
    assert len(shifted[0]) >= 8 and len(basic[0]) >= 4
    return shifted, basic


def _check_representation(lp, s, label, engaged, twin=None, explicit_inverse=True):
    """One shifted list and one basic-violating list against the cold solve; engaged(t) asserts that the forced form ran.  twin: a second
    solution in the same state for the second list (a clone would fold the pending terms of its source)."""
    shifted, basic = _two_lists(lp, s)
    unique = lp["name"].startswith("sparse")                                             # (transport and mixed instances have alternative optima)
    for which, (js, los, his), src in (("shifted", shifted, s), ("basic", basic, twin if twin is not None else s)):
        t = _apply(src if twin is not None else src.clone(), js, los, his)
        ok = _check_after(lp, t, js, los, his, "%s %s" % (label, which), unique, ("rep", label, which), explicit_inverse)
        if ok:
            info = t.bounds_info()
            assert (info["shifted"] == len(js) and info["solves"] == 1) if which == "shifted" else (info["basic"] == len(js) and info["solves"] == 0), (label, info)
            engaged(t)
        print("%s %s: %s" % (label, which, "infeasible" if t is None else t.bounds_info()))


@pytest.mark.gpu
def test_default_representation():
    lp, s = _solved("sparse-maximize")
    _check_representation(lp, s, "default", lambda t: None)


@pytest.mark.gpu
def test_pending_terms_of_the_delayed_update_mode(monkeypatch):
    from tests.test_gmi_cuts import _pending, _solved_with_pending_terms
    monkeypatch.setenv("MLP_LOWRANK", "3")
    s, lp, _ = _solved_with_pending_terms(lpgen.gen_sparse_lp(200, 150, 8, 3), True)
    twin, _, _ = _solved_with_pending_terms(lpgen.gen_sparse_lp(200, 150, 8, 3), True)
    assert _bits(s)[:2] == _bits(twin)[:2]
    for t in (s, twin):
        assert int(t.state("lowrank_pending")[1]) == 3 and _pending(t) > 0
    _check_representation(lp, s, "pending terms", lambda t: None, twin=twin)


@pytest.mark.gpu
def test_compact_factor(monkeypatch):
    monkeypatch.setenv("MLP_FACTOR", "1")
    lp = lpgen.gen_transport_lp(600, 700, 4, 5, tight=0.45)
    s = lpgen.build_problem(M.Problem, lp).solve()
    assert s.stats()["factor_active"] == 1

    def engaged(t):
        assert t.stats()["factor_active"] == 1

    _check_representation(lp, s, "compact factor", engaged, explicit_inverse=False)


@pytest.mark.gpu
def test_compact_factor_sparse_bump(monkeypatch):
    monkeypatch.setenv("MLP_FACTOR", "1")
    monkeypatch.setenv("MLP_FACTOR_SB_FROM", "2")
    s = lp = None
    for gen, args in ((lpgen.gen_sparse_lp, (400, 300, 12, 7)), (lpgen.gen_mixed_lp, (300, 400, 6, 3)), (lpgen.gen_sparse_lp, (1500, 1400, 12, 9))):
        lp = gen(*args)
        s = lpgen.build_problem(M.Problem, lp).solve()
        if s.stats()["factor_active"] == 1 and s.state("factor_sb")[0] == 1:
            break
    assert s.stats()["factor_active"] == 1 and s.state("factor_sb")[0] == 1

    def engaged(t):
        assert t.stats()["factor_active"] == 1 and t.state("factor_sb")[0] == 1

    _check_representation(lp, s, "sparse bump", engaged, explicit_inverse=False)


@pytest.mark.gpu
def test_hypersparse_re_solve(monkeypatch):
    monkeypatch.setenv("MLP_HYPER", "1")
    lp = lpgen.gen_sparse_lp(400, 300, 12, 7)
    s = lpgen.build_problem(M.Problem, lp).solve()
    h0 = s.stats()["hyper_iters"]

    def engaged(t):
        assert t.bounds_info()["pivots"] == 0 or t.stats()["hyper_iters"] > 0, (h0, t.stats()["hyper_iters"], t.bounds_info())

    _check_representation(lp, s, "hypersparse", engaged)


# ------------------------------------------------------------------------------------------------ 6: refusals and verdicts
@pytest.mark.gpu
def test_refusals_and_verdicts():
    from oracle import minilp_oracle as O
    lp, s = _solved("mixed")
    n = lp["n"]
    x = s.values()
    vs, _ = s.basis_status()
    before = _bits(s)
    lo, hi = lp["lo"], lp["hi"]
    j = next(j for j in range(n) if vs[j] == 1 and math.isfinite(hi[j]) and lo[j] < hi[j])
    # lo' > hi': Infeasible, the handle is consumed
    t = s.clone()
    with pytest.raises(M.Infeasible):
        t.set_var_bounds([j], [1.0], [0.5])
    assert not t._h.value
    # a column fixed by fix_var whose value falls outside the new bounds; inside them it keeps value and status, and unfix_var rebuilds
    fixed = s.clone().fix_var(j, float(lo[j]))
    fb = _bits(fixed)
    refusals = [(s, lambda t: t.set_var_bounds([j, 3 if j != 3 else 4, j], [lo[j]] * 3, [hi[j]] * 3)),              # listed twice
                (s, lambda t: t.set_var_bounds([0, n], [0.0, 0.0], [1.0, 1.0])),                                   # out of range
                (s, lambda t: t.set_var_bounds([j], [math.nan], [1.0])),
                (s, lambda t: t.set_var_bounds([j], [0.0], [math.nan])),
                (s, lambda t: t.set_var_bounds([j], [INF], [INF])),
                (s, lambda t: t.set_var_bounds([j], [-INF], [-INF])),
                (fixed, lambda t: t.set_var_bounds([j], [float(lo[j]) + 0.25], [float(hi[j]) + 1.0]))]
    for src, bad in refusals:
        t = src.clone()
        with pytest.raises(M.InternalError) as e:
            bad(t)
        assert e.value.code == -1 and not t._h.value
    assert _bits(s) == before and _bits(fixed) == fb
    with pytest.raises(M.InternalError):
        s.clone().set_var_bounds([0, 1], [0.0], [1.0, 1.0])                              # lengths differ (caught by the binding)
    # an unsolved (budget-limited) solution
    prob = lpgen.build_problem(M.Problem, lp)
    for call in (lambda t: t.set_var_bounds([j], [float(lo[j])], [float(hi[j])]), lambda t: t.tighten_by_reduced_cost(1e9)):
        t = prob.solve(budget=5)
        with pytest.raises(M.InternalError) as e:
            call(t)
        assert e.value.code == -1
    # a fixed column inside the new bounds
    t = fixed.clone().set_var_bounds([j], [float(lo[j]) - 1.0], [float(hi[j]) + 1.0])
    assert t.basis_status()[0][j] == M.MLP_NB_FIXED and t.values()[j] == lo[j] and _bits(t)[:2] == fb[:2]
    assert t.bounds_info()["shifted"] == 0 and t.bounds_info()["pivots"] == 0
    # unfix_var after it rebuilds the status against the NEW bounds.  (On sparse-maximize: on gen_mixed_lp the reference's own primal
    # re-entry of unfix_var leaves a NaN objective behind, as tests/test_fixing.py documents.)  Fixed at 0 = the old lower bound: with
    # [0, 5] the released column is at lower, with [-1, 5] it would sit strictly inside
    sp, q = _solved("sparse-maximize")
    sv, _ = q.basis_status()
    k = next(k for k in range(sp["n"]) if sv[k] == 1)
    assert sp["lo"][k] == 0.0 and math.isinf(sp["hi"][k])
    t = q.clone().fix_var(k, 0.0).set_var_bounds([k], [0.0], [5.0])
    assert t.basis_status()[0][k] == M.MLP_NB_FIXED
    t, was = t.unfix_var(k)
    assert was and t.var_bounds([k])[1][0] == 5.0 and t.basis_status()[0][k] == M.MLP_AT_LOWER and t.values()[k] == 0.0
    assert obj_close(t.objective(), q.objective())
    # bounds that are infeasible together: Infeasible, as the oracle says, and the handle is consumed
    hand = _hand_lp()
    with pytest.raises(O.Infeasible):
        lpgen.build_problem(O.Problem, _with_bounds(hand, [1, 2], [10.0, 10.0], [10.0, 10.0])).solve()
    q = lpgen.build_problem(M.Problem, hand).solve()
    with pytest.raises(M.Infeasible):
        q.set_var_bounds([1, 2], [10.0, 10.0], [10.0, 10.0])                           # 2 x0 + x1 + x2 = 3 with x0 >= 0
    assert not q._h.value
    cover, c = _solved("cover")
    with pytest.raises(O.Infeasible):
        lpgen.build_problem(O.Problem, dict(cover, hi=np.zeros(cover["n"]))).solve()
    q = c.clone()
    with pytest.raises(M.Infeasible):
        q.set_var_bounds(range(cover["n"]), cover["lo"], np.zeros(cover["n"]))
    assert not q._h.value


# ------------------------------------------------------------------------------------------------ 7: clone independence
@pytest.mark.gpu
def test_a_clone_keeps_its_parent_untouched():
    lp = _lp("sparse-maximize")
    parent, twin = (lpgen.build_problem(M.Problem, lp).solve() for _ in range(2))
    assert _bits(parent) == _bits(twin)
    vs, _ = parent.basis_status()
    js, los, his = bound_list(lp, parent.values(), vs, "mixed", 17)
    _, cutoff = _gap_and_cutoff(parent.objective(), lp["direction"], 0.01)
    child = _apply(parent.clone(), js, los, his)
    child2, count, _ = parent.clone().tighten_by_reduced_cost(cutoff)
    assert count >= 1 and child2.var_bounds()[1].tobytes() != parent.var_bounds()[1].tobytes()
    assert child is None or child.var_bounds()[0].tobytes() != parent.var_bounds()[0].tobytes() or child.var_bounds()[1].tobytes() != parent.var_bounds()[1].tobytes()
    assert _bits(parent) == _bits(twin)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(parent.var_bounds(), twin.var_bounds()))
    fj, flo, fhi = bound_list(lp, parent.values(), vs, "floor", 4)
    a, b = _apply(parent, fj, flo, fhi), _apply(twin, fj, flo, fhi)                     # the same re-solve on both, bit for bit
    assert (a is None) == (b is None) and (a is None or _bits(a) == _bits(b))


# ------------------------------------------------------------------------------------------------ 8: the example
@pytest.mark.gpu
def test_solve_mps_example_applies_the_tightened_bounds(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("solve_mps_bounds", os.path.join(ROOT, "examples", "solve_mps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lp = lpgen.gen_mixed_lp(40, 30, 6, 9)
    path = tmp_path / "mixed.mps"
    path.write_text(lpgen.to_mps(lp))
    obj = lpgen.build_problem(M.Problem, lp).solve().objective()
    assert mod.run(M, str(path), cutoff=obj + 0.05 * abs(obj), continuous=["X3"]) == 0
    assert "tightened:" not in capsys.readouterr().out                                   # without the flag: as before
    assert mod.run(M, str(path), cutoff=obj + 0.05 * abs(obj), continuous=["X3"], tighten=True) == 0
    out = capsys.readouterr().out
    k = int(re.search(r"cutoff \S+: (\d+) variables tightened, (\d+) of them fixed", out).group(1))
    assert k >= 1 and "'listed': %d" % k in out
    m = re.search(r"tightened: (\d+) bounds applied on the device, objective (\S+) unchanged", out)
    assert m and int(m.group(1)) == k and m.group(2) == "%.12g" % obj
    assert out.index("variables tightened") < out.index("tightened:")
    assert mod.run(M, str(path), cutoff=obj - 1.0, tighten=True) == 0 and "tightened:" not in capsys.readouterr().out      # pruned


# ------------------------------------------------------------------------------------------------ 9: measurement
@pytest.mark.gpu
def test_64_bounds_in_one_call_are_not_slower_than_64_singleton_rows():
    """gen_mixed_lp(6000, 10000, 4, 3), median of 5 after one warm-up, one process: 64 upper-bound branches (basic fractional columns
    nearest to their floor, down to it) by one set_var_bounds against one add_constraints of the same 64 singleton rows on a clone of the same state;
    tighten_by_reduced_cost against cutoff_bounds plus set_var_bounds of the list it returns.  Asserts only that the new call is not
    slower than the rows.  Written to profiles/bounds.json when MLP_WRITE_PROFILES=1; the recorded run is in DESIGN.md §7.8."""
    lp = lpgen.gen_mixed_lp(6000, 10000, 4, 3)
    s = lpgen.build_problem(M.Problem, lp).solve()
    x = s.values()
    vs, _ = s.basis_status()
    # the 64 basic fractional columns nearest to their floor, as a dive would take them (64 arbitrary floor branches are infeasible together)
    frac = [j for j in range(lp["n"]) if vs[j] == 0 and abs(x[j] - round(x[j])) > 1e-3 and math.floor(x[j]) >= lp["lo"][j]]
    js = sorted(frac, key=lambda j: x[j] - math.floor(x[j]))[:64]
    los, his = [float(lp["lo"][j]) for j in js], [float(math.floor(x[j])) for j in js]
    assert len(js) == 64
    _, cutoff = _gap_and_cutoff(s.objective(), lp["direction"], 0.01)
    marks = np.ones(lp["n"], bool)
    tb, tr, tt, tc = [], [], [], []
    binfo = rinfo = tinfo = None
    for rep in range(6):
        a, b, c, d = s.clone(), s.clone(), s.clone(), s.clone()
        t0 = time.perf_counter()
        a = a.set_var_bounds(js, los, his)
        t1 = time.perf_counter()
        b = b.add_constraints([([(j, 1.0)], M.LE, u) for j, u in zip(js, his)])
        t2 = time.perf_counter()
        c, count, _ = c.tighten_by_reduced_cost(cutoff, marks)
        t3 = time.perf_counter()
        v, lo, hi, _ = d.cutoff_bounds(cutoff, marks)
        d = d.set_var_bounds(v, lo, hi)
        t4 = time.perf_counter()
        binfo, rinfo, tinfo = a.bounds_info(), b.cut_info(), c.bounds_info()
        assert obj_close(a.objective(), b.objective()) and count == len(v) and d.bounds_info()["shifted"] == 0
        if rep:
            tb.append((t1 - t0) * 1e3); tr.append((t2 - t1) * 1e3); tt.append((t3 - t2) * 1e3); tc.append((t4 - t3) * 1e3)
    rec = dict(instance="gen_mixed_lp(6000, 10000, 4, 3)", requests=64, set_var_bounds_wall_ms=float(np.median(tb)),
               singleton_rows_wall_ms=float(np.median(tr)), ratio=float(np.median(tr) / np.median(tb)), set_var_bounds_device_ms=binfo["device_ms"],
               set_var_bounds_pivots=binfo["pivots"], singleton_rows_pivots=rinfo.get("pivots"), tighten_wall_ms=float(np.median(tt)),
               read_and_round_trip_wall_ms=float(np.median(tc)), tighten_device_ms=tinfo["device_ms"], tightened=tinfo["tightened"])
    print("BOUNDS " + json.dumps(rec))
    if os.environ.get("MLP_WRITE_PROFILES") == "1":
        with open(os.path.join(ROOT, "profiles", "bounds.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    assert rec["ratio"] >= 1.0, rec
