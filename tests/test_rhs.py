"""New right-hand sides for a solved model and the batched what-if read (include/minilp_hip.h: mlp_solution_set_rhs,
mlp_solution_constraint_rhs, mlp_solution_rhs_scenarios, mlp_rhs_info; csrc/rhs.inc).

The yardstick of set_rhs is the cold solve of the model with the new right-hand sides: the oracle's (verdict, objective to OBJ_RTOL, x
to X_ATOL where the optimum is unique) and scipy's HiGHS (objective to HIGHS_RTOL).  The lists are built by `rhs_list` from a solved
point and the basis statuses of the slacks: the CPU tests build them from the oracle's optimum, check the two yardsticks against each
other and pin which lists are Infeasible; the GPU tests build them from the engine's optimum and hold the engine to both yardsticks.
The yardstick of rhs_scenarios is the host route it replaces: basis_solve of the dense change and numpy on values / basis_head.

A refused call (MLP_EINVAL) frees the handle like every mutator of the library: "left bit-identical" is checked on the solution the
refused clone was taken from."""
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
from tests.test_bounds import KKT_TOL, UNIQUE
from tests.test_branch_penalties import INSTANCES, _blob, _frac_basic, _hand_lp, _model_of_state
from tests.test_ranging import _highs_obj

INF = math.inf
EPS = 1e-8  # kernels.h: the feasibility tolerance of the dual pricing
NEW = ["mlp_solution_set_rhs", "mlp_solution_constraint_rhs", "mlp_solution_rhs_scenarios", "mlp_solution_rhs_info", "mlp_rhs_info_size"]
RHS_INSTANCES = dict(INSTANCES, bounded=(gen_bounded_lp, (300, 400, 6, 3)), hand=(_hand_lp, ()))
KINDS = ("tighten", "relax", "loose-in", "loose-beyond", "eq+", "eq-", "mixed")
LENGTHS = (0, 1, 16, 17, 64, 257)
# (instance, kind, k) of the lists that BOTH the oracle and HiGHS find Infeasible at k = 16 and k = 64, built from the oracle's optimum
# (test_the_two_yardsticks_agree_on_every_rhs_list recomputes and compares the whole set); every other list there is feasible
PINNED_INFEASIBLE = {("mixed", "loose-beyond", 64), ("sparse-maximize", "loose-beyond", 64), ("small-mixed", "loose-beyond", 16),
                     ("small-mixed", "loose-beyond", 64), ("bounded", "loose-beyond", 64), ("hand", "loose-beyond", 16),
                     ("hand", "loose-beyond", 64), ("hand", "mixed", 16), ("hand", "mixed", 64)}
# the instances by generator; gen_cover_lp is the one family without an Infeasible list: its variables have no upper bound, so rows of
# non-negative coefficients that ask for more can always be covered
FAMILIES = {"gen_mixed_lp": ("mixed", "small-mixed"), "gen_sparse_lp": ("sparse-maximize",), "gen_bounded_lp": ("bounded",), "hand": ("hand",),
            "gen_cover_lp": ("cover",)}


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(M.lib_path()):
        mbuild.build(verbose=False)
    return M.lib()


def _lp(name):
    gen, args = RHS_INSTANCES[name]
    lp = gen(*args)
    return dict(lp, indptr=np.asarray(lp["indptr"], dtype=np.int64), indices=np.asarray(lp["indices"], dtype=np.int64))  # (the hand LP: unsigned)


# ------------------------------------------------------------------------------------------------ the right-hand-side lists
def _activity(lp, x):
    return np.add.reduceat(lp["data"] * np.asarray(x)[lp["indices"].astype(np.int64)], lp["indptr"][:-1].astype(np.int64))


def rhs_list(lp, x, cons_status, kind, k):
    """(constraints, rhs): at most k requests of one kind at the point x with the statuses cons_status of the slacks (0: basic).  The
    step is 0.05 max(1, |b|); a row is tight when its slack is non-basic.
    tighten / relax  tight inequality rows moved against / with their operator
    loose-in         inequality rows with a basic slack moved half-way to their activity (no basic value leaves its bounds)
    loose-beyond     the same rows moved past their activity by the step
    eq+ / eq-        equality rows shifted up / down
    mixed            all of the above in turn"""
    m, ops, b = lp["m"], lp["ops"], np.asarray(lp["rhs"], dtype=float)
    act = _activity(lp, x)
    step = 0.05 * np.maximum(1.0, np.abs(b))
    away = np.where(ops == lpgen.LE, 1.0, -1.0)                                          # the direction that relaxes an inequality row
    ineq = [i for i in range(m) if ops[i] != lpgen.EQ]
    tight = [i for i in ineq if cons_status[i] != 0]
    loose = [i for i in ineq if cons_status[i] == 0 and abs(act[i] - b[i]) > 1e-6]
    eq = [i for i in range(m) if ops[i] == lpgen.EQ]
    one = {
        "tighten": (tight, lambda i: b[i] - away[i] * step[i]),
        "relax": (tight, lambda i: b[i] + away[i] * step[i]),
        "loose-in": (loose, lambda i: b[i] + 0.5 * (act[i] - b[i])),
        "loose-beyond": (loose, lambda i: act[i] - away[i] * step[i]),
        "eq+": (eq, lambda i: b[i] + step[i]),
        "eq-": (eq, lambda i: b[i] - step[i]),
    }
    cs, vals = [], []
    if kind != "mixed":
        pool, f = one[kind]
        cs = pool[:k]
        vals = [f(i) for i in cs]
    else:
        order = ("relax", "loose-in", "eq+", "tighten", "loose-beyond", "eq-")
        used, t, dry = set(), 0, 0
        while len(cs) < k and dry < len(order):
            pool, f = one[order[t % len(order)]]
            t += 1
            left = [i for i in pool if i not in used]
            if not left:
                dry += 1
                continue
            dry = 0
            i = left[len(left) // 2] if t % 2 else left[0]
            used.add(i)
            cs.append(i)
            vals.append(f(i))
    return [int(i) for i in cs], [float(v) for v in vals]


def feasible_mix(lp, x, cons_status, k):
    """relax and loose-in requests in turn: a list that is feasible whatever its length."""
    a, b = rhs_list(lp, x, cons_status, "relax", k), rhs_list(lp, x, cons_status, "loose-in", k)
    cs, vals = [], []
    for t in range(max(len(a[0]), len(b[0]))):
        for src in (a, b):
            if t < len(src[0]) and len(cs) < k:
                cs.append(src[0][t])
                vals.append(src[1][t])
    return cs, vals


def _with_rhs(lp, cs, vals):
    rhs = np.array(lp["rhs"], dtype=float)
    rhs[cs] = vals
    return dict(lp, rhs=rhs)


_COLD = {}


def _cold(lp2, key):
    """(oracle solution or None when Infeasible, HiGHS objective or None) of the model with the new right-hand sides, once per key."""
    from oracle import minilp_oracle as O
    if key not in _COLD:
        try:
            o = lpgen.build_problem(O.Problem, lp2).solve()
        except O.Infeasible:
            o = None
        _COLD[key] = (o, _highs_obj(lp2))
    return _COLD[key]


def _oracle_cons_status(o, lp):
    basic = set(int(v) for v in o.state("basic_vars"))
    return np.array([0 if lp["n"] + i in basic else 1 for i in range(lp["m"])])


_ORACLE = {}


def _oracle_point(name):
    from oracle import minilp_oracle as O
    if name not in _ORACLE:
        lp = _lp(name)
        o = lpgen.build_problem(O.Problem, lp).solve()
        _ORACLE[name] = (lp, o.values(), _oracle_cons_status(o, lp), o.objective())
    return _ORACLE[name]


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
    assert "typedef struct mlp_rhs_info" in hdr and "Still version 5: the right-hand-side changes" in hdr
    args = re.search(r"pub fn mlp_solution_rhs_scenarios\s*\(([^)]*)\)", sys_rs).group(1)
    assert [a.split(":")[0].strip() for a in args.split(",")] == ["s", "constraints", "n", "rhs", "num_scenarios", "bound", "feasible", "worst",
                                                                 "worst_col"]
    assert re.search(r"pub fn set_rhs\s*\(self", lib_rs) and re.search(r"pub fn constraint_rhs\s*\(&self", lib_rs)
    assert re.search(r"pub fn rhs_scenarios\s*\(&self", lib_rs)
    ext = surface.split("### extensions")[1]
    for n in ("set_rhs", "constraint_rhs", "rhs_scenarios"):
        assert re.search(r"\* `pub fn %s\(&?self, .*`" % n, ext), n
    for n in ("set_rhs", "constraint_rhs", "rhs_scenarios", "rhs_info"):
        assert hasattr(M.Solution, n), n
    block = hdr.split("mlp_solution_set_rhs gives")[1].split("*/")[0]
    assert "same right-hand sides" in block and "zero pivots" in block                     # the blob note and the meaning of `feasible`


def test_abi_version_is_still_5_and_the_struct_size_matches(L):
    assert L.mlp_abi_version() == 5 == api.ABI_VERSION
    L.mlp_rhs_info_size.restype = ctypes.c_uint64
    assert L.mlp_rhs_info_size() == ctypes.sizeof(api.MlpRhsInfo) == 72
    assert ("mlp_rhs_info_size", api.MlpRhsInfo) in api._STRUCT_SIZES
    assert L.mlp_bounds_info_size() == 80 and L.mlp_propagate_info_size() == 56          # no existing struct grew


def test_null_handle_is_einval_not_a_crash(L):
    h = ctypes.c_void_p()
    c, b = np.zeros(1, dtype=np.uint64), np.zeros(1)
    out, feas, col = np.zeros(1), np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.int64)
    pu, pd = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)
    pc, pb, po = c.ctypes.data_as(pu), b.ctypes.data_as(pd), out.ctypes.data_as(pd)
    assert L.mlp_solution_set_rhs(ctypes.byref(h), pc, pb, 1) == -1
    assert L.mlp_solution_set_rhs(None, pc, pb, 0) == -1
    assert L.mlp_solution_constraint_rhs(None, pc, 1, po) == -1
    assert L.mlp_solution_rhs_scenarios(None, pc, 1, pb, 1, po, feas.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), po,
                                        col.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) == -1
    assert L.mlp_solution_rhs_info(None, ctypes.byref(api.MlpRhsInfo())) == -1


@pytest.mark.parametrize("family", list(FAMILIES))
def test_the_two_yardsticks_agree_on_every_rhs_list(family):
    """The oracle's cold solve of the model with the new right-hand sides and HiGHS: the same verdict, the objective to HIGHS_RTOL — on
    every kind of list at 1, 16 and 64 requests, built from the oracle's optimum.  The Infeasible lists at 16 and 64 are exactly the
    pinned ones: the GPU tests compare verdicts, and these pins keep that comparison from being empty."""
    changed = infeasible = 0
    for name in FAMILIES[family]:
        lp, x, st, obj = _oracle_point(name)
        found = set()
        for kind in KINDS:
            for k in (1, 16, 64):
                cs, vals = rhs_list(lp, x, st, kind, k)
                assert len(cs) == len(set(cs)) <= k, (name, kind, k)
                if not cs:
                    continue
                oc, hg = _cold(_with_rhs(lp, cs, vals), ("cpu", name, kind, k))
                assert (oc is None) == (hg is None), (name, kind, k, oc is None, hg)
                if oc is None:
                    found.add((name, kind, k))
                else:
                    assert obj_close(oc.objective(), hg, HIGHS_RTOL), (name, kind, k, oc.objective(), hg)
                    changed += not obj_close(oc.objective(), obj, 1e-6)
                if kind == "loose-in":                                                   # nothing may pivot: the optimum stays
                    assert oc is not None and obj_close(oc.objective(), obj), (name, k)
        assert {f for f in found if f[2] != 1} == {p for p in PINNED_INFEASIBLE if p[0] == name}, (name, sorted(found))
        infeasible += len(found)
    assert changed >= 1 and (infeasible >= 1 or family == "gen_cover_lp"), (family, changed, infeasible)


def test_the_feasible_mix_is_feasible_at_every_length():
    for name, want in (("mixed", (0, 1, 16, 17, 64, 231)), ("bounded", LENGTHS)):
        lp, x, st, obj = _oracle_point(name)
        for k, n in zip(LENGTHS, want):
            cs, vals = feasible_mix(lp, x, st, k)
            assert len(cs) == n == len(set(cs)), (name, k, len(cs))
            oc, hg = _cold(_with_rhs(lp, cs, vals), ("cpu", name, "feasible-mix", k))
            assert oc is not None and obj_close(oc.objective(), hg, HIGHS_RTOL), (name, k)


# ------------------------------------------------------------------------------------------------ GPU: shared state
_SOLVED = {}


def _solved(name):
    if name not in _SOLVED:
        lp = _lp(name)
        _SOLVED[name] = (lp, lpgen.build_problem(M.Problem, lp).solve())
    return _SOLVED[name]


def _bits(s):
    return np.float64(s.objective()).tobytes(), s.values().tobytes(), _blob(s), s.constraint_rhs().tobytes()


def _apply(s, cs, vals):
    try:
        return s.set_rhs(cs, vals)
    except M.Infeasible:
        return None


def _check_after(lp, t, cs, vals, label, unique, key):
    """Everything section 1 of the issue asks of a solution after set_rhs (t is None: the call said Infeasible)."""
    lp2 = _with_rhs(lp, cs, vals)
    oc, hg = _cold(lp2, key)
    assert (t is None) == (oc is None) == (hg is None), (label, t is None, oc is None, hg)
    if t is None:
        return False
    assert obj_close(t.objective(), oc.objective()) and obj_close(t.objective(), hg, HIGHS_RTOL), (label, t.objective(), oc.objective(), hg)
    x = t.values()
    check_feasible(lp2, x)
    assert obj_close(float(np.dot(lp["obj"], x)), t.objective()), (label, float(np.dot(lp["obj"], x)), t.objective())
    if unique:
        assert np.abs(x - oc.values()).max() <= X_ATOL, (label, float(np.abs(x - oc.values()).max()))
    c = t.certificate()
    assert max(c["relative_gap"], c["max_dual_infeasibility"], c["max_row_violation"], c["max_bound_violation"]) <= KKT_TOL, (label, c)
    assert t.constraint_rhs().tobytes() == lp2["rhs"].tobytes() and t.state("orig_rhs").tobytes() == lp2["rhs"].tobytes(), label
    if cs:
        assert t.constraint_rhs(cs[:3]).tolist() == list(vals[:3])
    return True


def _kinds_of(name):
    lp = _lp(name)
    has_eq = bool((lp["ops"] == lpgen.EQ).any())
    return [kd for kd in KINDS if (has_eq or not kd.startswith("eq")) and (name != "hand" or kd not in ("tighten", "relax"))]


# ------------------------------------------------------------------------------------------------ 1: against the cold solve
@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", [(nm, kd) for nm in RHS_INSTANCES for kd in _kinds_of(nm)])
def test_set_rhs_against_the_cold_solve(name, kind):
    lp, s = _solved(name)
    _, cst = s.basis_status()
    cs, vals = rhs_list(lp, s.values(), cst, kind, 16)
    assert len(cs) >= (1 if name == "hand" else 4), (name, kind, len(cs))
    t = _apply(s.clone(), cs, vals)
    ok = _check_after(lp, t, cs, vals, "%s %s" % (name, kind), name in UNIQUE, ("gpu", name, kind, 16))
    if name in UNIQUE or name == "hand":                                                 # the engine's vertex is the oracle's: the pins hold here too
        assert ok == ((name, kind, 16) not in PINNED_INFEASIBLE), (name, kind, ok)
    if ok:
        info = t.rhs_info()
        assert info["requests"] == len(cs) and info["changed"] == len(cs) and info["solves"] == 1 and info["batches"] == 1, (name, kind, info)
        if kind == "loose-in":                                                           # only basic slacks move, inside their bounds
            assert info["pivots"] == 0 and t.values().tobytes() == s.values().tobytes(), info
            assert np.float64(t.objective()).tobytes() == np.float64(s.objective()).tobytes()
        if kind == "loose-beyond":
            assert info["pivots"] >= 1, info
        print("%s %s: %s" % (name, kind, info))
    else:
        print("%s %s: infeasible, as the oracle and HiGHS say" % (name, kind))


# ------------------------------------------------------------------------------------------------ 2: inside the range
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sparse-maximize", "cover", "mixed"])
def test_inside_its_range_a_right_hand_side_moves_no_basis(name):
    """0.5 of the distance to the nearer finite end of rhs_ranging (+-1 where both ends are infinite): no pivot, the basis head stays, the
    objective moves by dual_value * delta.  2 x the distance, past that end: a pivot or Infeasible, as the cold solve says.  Ends nearer
    than 1e-3 are left out (a degenerate vertex has ranges of width 0), and no value lies between 0.9 x and 1.1 x of an end."""
    lp, s = _solved(name)
    _, cst = s.basis_status()
    b, pi, head = s.constraint_rhs(), s.dual_values(), s.basis_head()
    tight = [i for i in range(lp["m"]) if cst[i] != 0]
    lo, hi = s.rhs_ranging(tight)
    done = past = 0
    for i, l, h in zip(tight, lo, hi):
        dl, dh = b[i] - l, h - b[i]
        ends = [d for d in ((-dl, dl), (dh, dh)) if math.isfinite(d[1])]
        if not ends:
            step, finite = 1.0, False
        else:
            step, finite = min(ends, key=lambda d: d[1])[0], True
        if finite and abs(step) < 1e-3:
            continue
        t = s.clone().set_rhs([i], [b[i] + 0.5 * step])
        info = t.rhs_info()
        assert info["pivots"] == 0 and info["solves"] == 1 and (t.basis_head() == head).all(), (name, i, info)
        assert obj_close(t.objective(), s.objective() + pi[i] * 0.5 * step), (name, i, t.objective(), s.objective(), pi[i], step)
        done += 1
        if finite and past < 4:
            u = _apply(s.clone(), [i], [b[i] + 2.0 * step])
            ok = _check_after(lp, u, [i], [b[i] + 2.0 * step], "%s past the range of %d" % (name, i), False, ("range", name, i))
            assert not ok or u.rhs_info()["pivots"] >= 1, (name, i, u.rhs_info())
            past += 1
        if done >= 8:
            break
    assert done >= 4 and past >= 2, (name, done, past)


# ------------------------------------------------------------------------------------------------ 3: h_rhs really moved
@pytest.mark.gpu
def test_every_reader_of_the_right_hand_side_sees_the_new_one():
    lp, s = _solved("sparse-maximize")
    _, cst = s.basis_status()
    cs, vals = rhs_list(lp, s.values(), cst, "mixed", 16)
    before = _bits(s)
    t = s.clone().set_rhs(cs, vals)
    want = _with_rhs(lp, cs, vals)["rhs"]
    x, obj = t.values(), t.objective()
    assert not np.array_equal(x, s.values())
    t.recompute_basic_values()                                                           # x_B = B^-1 (b - N x_N) from the host's vector
    assert np.abs(t.values() - x).max() <= 1e-9 and obj_close(t.objective(), obj)
    t.reinvert()
    assert np.abs(t.values() - x).max() <= 1e-9
    u = t.clone()                                                                        # a clone carries the new vector
    assert u.constraint_rhs().tobytes() == want.tobytes() and _bits(u)[:2] == _bits(t)[:2]
    u = u.add_constraint([(j, 1.0) for j in range(lp["n"])], M.LE, float(x.sum()) + 10.0)  # a slack row: the matrix is laid out again
    assert obj_close(u.objective(), obj) and u.constraint_rhs()[:lp["m"]].tobytes() == want.tobytes()
    assert u.constraint_rhs()[lp["m"]] == float(x.sum()) + 10.0
    u.recompute_basic_values()
    assert np.abs(u.values() - x).max() <= 1e-9
    v = u.set_rhs([lp["m"]], [float(x.sum()) + 20.0])                                   # the appended row has a right-hand side too
    assert v.rhs_info()["pivots"] == 0 and obj_close(v.objective(), obj)
    c = t.certificate()
    assert c["max_row_violation"] <= KKT_TOL and c["relative_gap"] <= KKT_TOL, c         # the certificate reads the new vector
    assert _bits(s) == before                                                            # the parent of a changed clone keeps its own


# ------------------------------------------------------------------------------------------------ 4: every bit
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed", "sparse-maximize", "cover", "bounded"])
def test_the_current_values_change_nothing_and_the_order_changes_no_bit(name):
    lp, s = _solved(name)
    t = s.clone()
    before = _bits(t)
    cs = list(range(0, lp["m"], 3))                                                      # rows with basic and with non-basic slacks
    t = t.set_rhs(cs, lp["rhs"][cs])
    info = t.rhs_info()
    assert _bits(t) == before and info["pivots"] == 0 and info["solves"] == 0 and info["changed"] == 0 and info["requests"] == len(cs), info
    t = t.set_rhs([], [])                                                                # n == 0: a successful no-op
    assert _bits(t) == before and t.rhs_info()["requests"] == 0 and t.rhs_info()["solves"] == 0
    _, cst = s.basis_status()
    cs, vals = rhs_list(lp, s.values(), cst, "mixed", 17)
    rng = np.random.default_rng(11)
    outs = []
    for rep in range(3):
        p = np.arange(len(cs)) if rep == 0 else rng.permutation(len(cs))
        u = _apply(s.clone(), [cs[i] for i in p], [vals[i] for i in p])
        outs.append(None if u is None else _bits(u))
    assert outs[0] is not None and outs[0] == outs[1] == outs[2]


# ------------------------------------------------------------------------------------------------ 5: lengths
# the length of the feasible mix at the engine's own vertex (the engine is deterministic): gen_mixed_lp(300, 400, 6, 3) has 232 inequality
# rows, and a row whose slack is basic at zero belongs to neither kind
ENGINE_MIX_LENGTHS = {"mixed": (0, 1, 16, 17, 64, 231), "bounded": LENGTHS}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ENGINE_MIX_LENGTHS))
def test_the_feasible_mix_at_every_length(name):
    """relax + loose-in in turn at 0, 1, 16, 17, 64, 257 requests: exactly that many, and the objective of the cold solve.
    gen_mixed_lp(300, 400, 6, 3) has fewer inequality rows than 257: there the list has the pinned length of ENGINE_MIX_LENGTHS (231 at
    the oracle's vertex, pinned in the CPU test)."""
    lp, s = _solved(name)
    _, cst = s.basis_status()
    for k, want in zip(LENGTHS, ENGINE_MIX_LENGTHS[name]):
        cs, vals = feasible_mix(lp, s.values(), cst, k)
        print("%s feasible mix: %d asked, %d listed" % (name, k, len(cs)))
        assert len(cs) == want == len(set(cs)), (name, k, len(cs))
        u = _apply(s.clone(), cs, vals)
        assert _check_after(lp, u, cs, vals, "%s feasible mix %d" % (name, k), name in UNIQUE, ("gpu", name, "feasible-mix", k))
        assert u.rhs_info()["requests"] == len(cs) and u.rhs_info()["solves"] == (1 if cs else 0)


# ------------------------------------------------------------------------------------------------ 6: scenarios against basis_solve
def _scenarios(lp, s, S, k=16):
    """(constraints, rhs[S, n]): the mixed list scaled by 0.5 and 2 on rotating subsets; scenario 0 moves loose rows half-way only."""
    _, cst = s.basis_status()
    b = s.constraint_rhs()
    cs, vals = rhs_list(lp, s.values(), cst, "mixed", k)
    loose_in = set(rhs_list(lp, s.values(), cst, "loose-in", lp["m"])[0])
    d = np.array(vals) - b[cs]
    out = np.tile(b[cs], (S, 1))
    for t in range(S):
        if t % 4 == 0:
            mask = np.array([i in loose_in for i in cs])
            scale = 0.5
        elif t % 4 == 1:
            mask, scale = np.ones(len(cs), bool), 2.0
        else:
            mask = np.array([(q + t) % 3 != 0 for q in range(len(cs))])
            scale = 0.5 if t % 4 == 2 else 2.0
        out[t] += scale * (1.0 + 0.01 * (t // 4)) * mask * d
    return cs, out


def _slack_bounds(lp):
    """Bounds of the slack of every constraint of the Problem, from its operator."""
    ops = lp["ops"]
    lo = np.where(ops == lpgen.GE, -INF, 0.0)
    hi = np.where(ops == lpgen.LE, INF, 0.0)
    return lo, hi


def _host_scenarios(s, lp, cs, rhs, floor=False):
    """The host route: basis_solve of the dense changes, numpy on values / basis_head / var_bounds.  floor=True adds "floor": what this
    route itself rounds at most.  It rebuilds a slack's value as b - a.x in double from values(), (nnz + 2) u (|b| + sum |a x|) off per
    row at the worst, and rounds x_B + y once more, u |x_B + y|; u = 2^-53."""
    n, m = lp["n"], s.num_constraints
    b, x, head = s.constraint_rhs(), s.values(), s.basis_head()
    db = np.zeros((len(rhs), m))
    db[:, cs] = rhs - b[cs]
    y = s.basis_solve(db) if len(rhs) else np.zeros((0, m))
    vlo, vhi = s.var_bounds()
    slo, shi = _slack_bounds(lp)
    xall = np.concatenate([x, b - _activity(lp, x)])
    lo, hi = np.concatenate([vlo, slo])[head], np.concatenate([vhi, shi])[head]
    val = xall[head][None, :] + y
    viol = np.where(val < lo - EPS, lo - val, np.where(val > hi + EPS, val - hi, 0.0))
    worst = viol.max(axis=1) if len(rhs) else np.zeros(0)
    feasible = worst == 0.0
    col = np.where(feasible, -1, head[viol.argmax(axis=1)] if len(rhs) else 0)
    bound = s.objective() + db @ s.dual_values()
    out = dict(bound=bound, feasible=feasible, worst=worst, worst_col=col)
    if floor:
        ptr, idx = lp["indptr"].astype(np.int64), lp["indices"].astype(np.int64)
        size = np.abs(b) + np.add.reduceat(np.abs(lp["data"] * x[idx]), ptr[:-1])
        out["floor"] = 2.0 ** -53 * ((int(np.diff(ptr).max()) + 2) * float(size.max()) + (float(np.abs(val).max()) if len(rhs) else 0.0))
    return out


def _check_scenarios(s, lp, cs, rhs, label):
    got, want = s.rhs_scenarios(cs, rhs), _host_scenarios(s, lp, cs, rhs, floor=True)
    floor = want.pop("floor")
    S = len(rhs)
    info = s.rhs_info()
    assert info["scenarios"] == S and info["requests"] == len(cs) and info["solves"] == S and info["batches"] == (S + 15) // 16, (label, info)
    for key in got:
        assert len(got[key]) == S
    for t in range(S):
        print("%s scenario %d: feasible %s worst %.3e col %d bound %.12g | host %s %.3e %d %.12g" % (
            label, t, got["feasible"][t], got["worst"][t], got["worst_col"][t], got["bound"][t], want["feasible"][t], want["worst"][t],
            want["worst_col"][t], want["bound"][t]))
    assert not ((want["worst"] > 0.5e-8) & (want["worst"] < 2e-8)).any(), label                # no scenario sits at the tolerance
    assert (got["feasible"] == want["feasible"]).all() and (got["worst_col"] == want["worst_col"]).all(), label
    off = np.abs(got["worst"] - want["worst"])
    print("%s: worst is off by %.3e at the most, %.3e relative; the host route's own rounding is %.3e" % (
        label, off.max(initial=0.0), (off / np.maximum(want["worst"], 1e-300)).max(initial=0.0), floor))
    assert (off <= 1e-9 * np.abs(want["worst"]) + floor).all(), label                          # 1e-9 relative, above the reference's own rounding
    assert (got["worst"][got["feasible"]] == 0.0).all() and (got["worst_col"][got["feasible"]] == -1).all()
    assert all(obj_close(g, w) for g, w in zip(got["bound"], want["bound"])), (label, got["bound"], want["bound"])
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed", "sparse-maximize", "small-mixed"])
def test_scenarios_against_the_host_route(name):
    lp, s = _solved(name)
    before = _bits(s)
    seen = set()
    for S in (0, 1, 16, 17, 33):
        cs, rhs = _scenarios(lp, s, S)
        got = _check_scenarios(s, lp, cs, rhs, "%s S=%d" % (name, S))
        seen |= set(bool(f) for f in got["feasible"])
    assert seen == {True, False}, (name, seen)
    # one scenario alone, in another place, among other neighbours, under another order of the constraints: the same bits
    cs, rhs = _scenarios(lp, s, 33)
    full = s.rhs_scenarios(cs, rhs)
    perm = np.random.default_rng(5).permutation(len(cs))
    for t in (0, 1, 7, 16, 32):
        alone = s.rhs_scenarios(cs, rhs[t:t + 1])
        moved = s.rhs_scenarios(cs, np.vstack([rhs[20:25], rhs[t:t + 1], rhs[2:4]]))
        turned = s.rhs_scenarios([cs[i] for i in perm], rhs[t:t + 1][:, perm])
        for key in full:
            a = np.asarray(full[key][t]).tobytes()
            assert a == np.asarray(alone[key][0]).tobytes() == np.asarray(moved[key][5]).tobytes() == np.asarray(turned[key][0]).tobytes(), (name, t, key)
    # n == 0: the current point
    got = s.rhs_scenarios([], np.zeros((5, 0)))
    assert got["feasible"].all() and (got["bound"] == s.objective()).all() and (got["worst"] == 0.0).all() and (got["worst_col"] == -1).all()
    assert s.rhs_info()["solves"] == 0
    assert _bits(s) == before                                                            # a read: nothing changed


# ------------------------------------------------------------------------------------------------ 7: scenario and mutator agree
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed", "sparse-maximize"])
def test_a_scenario_says_what_set_rhs_does(name):
    lp, s = _solved(name)
    cs, rhs = _scenarios(lp, s, 17)
    got = s.rhs_scenarios(cs, rhs)
    sg = -1.0 if lp["direction"] == M.MAXIMIZE else 1.0
    quiet = pivoted = refused = 0
    for t in range(len(rhs)):
        u = _apply(s.clone(), cs, rhs[t])
        if got["feasible"][t]:
            assert u is not None and u.rhs_info()["pivots"] == 0 and obj_close(u.objective(), got["bound"][t]), (name, t, got["bound"][t])
            quiet += 1
        else:
            assert u is None or u.rhs_info()["pivots"] >= 1, (name, t)
            pivoted += u is not None
            refused += u is None
        if u is not None:                                                                # weak duality: the bound is on the dual side
            tol = OBJ_RTOL * max(1.0, abs(got["bound"][t]), abs(u.objective()))
            assert sg * u.objective() >= sg * got["bound"][t] - tol, (name, t, u.objective(), got["bound"][t])
    print("%s: %d scenarios without a pivot, %d with pivots, %d infeasible" % (name, quiet, pivoted, refused))
    assert quiet >= 1 and pivoted + refused >= 1


# ------------------------------------------------------------------------------------------------ 8: every representation of B^-1
def _check_representation(lp, s, label, engaged):
    """One batch of 17 scenarios against the host route, then one set_rhs that must pivot against the cold solve, on s itself (a clone
    would fold the pending terms of its source); engaged(t) asserts that the forced form ran."""
    cs, rhs = _scenarios(lp, s, 17)
    _check_scenarios(s, lp, cs, rhs, label)
    _, cst = s.basis_status()
    pick = None
    for kind, k in (("loose-beyond", 4), ("loose-beyond", 1), ("tighten", 16), ("eq+", 4), ("eq-", 4), ("tighten", 64)):
        cs, vals = rhs_list(lp, s.values(), cst, kind, k)                                # the first list that the cold solve finds feasible
        if cs and _cold(_with_rhs(lp, cs, vals), ("rep", label, kind, k))[0] is not None and not s.rhs_scenarios(cs, [vals])["feasible"][0]:
            pick = (kind, k, cs, vals)                                                   # ... and that moves a basic value out of its bounds
            break
    assert pick is not None, label
    kind, k, cs, vals = pick
    t = _apply(s, cs, vals)
    assert _check_after(lp, t, cs, vals, label, lp["name"].startswith("sparse"), ("rep", label, kind, k))
    assert t.rhs_info()["pivots"] >= 1 and t.rhs_info()["solves"] == 1, (label, t.rhs_info())
    engaged(t)
    print("%s: %s %d, %s" % (label, kind, k, t.rhs_info()))


@pytest.mark.gpu
def test_default_representation():
    lp = _lp("sparse-maximize")
    _check_representation(lp, lpgen.build_problem(M.Problem, lp).solve(), "default", lambda t: None)


@pytest.mark.gpu
def test_pending_terms_of_the_delayed_update_mode(monkeypatch):
    from tests.test_gmi_cuts import _pending, _solved_with_pending_terms
    monkeypatch.setenv("MLP_LOWRANK", "3")
    s, lp, _ = _solved_with_pending_terms(lpgen.gen_sparse_lp(200, 150, 8, 3), True)
    assert int(s.state("lowrank_pending")[1]) == 3 and _pending(s) > 0
    _check_representation(lp, s, "pending terms", lambda t: None)


@pytest.mark.gpu
def test_compact_factor(monkeypatch):
    monkeypatch.setenv("MLP_FACTOR", "1")
    lp = lpgen.gen_transport_lp(600, 700, 4, 5, tight=0.45)
    s = lpgen.build_problem(M.Problem, lp).solve()
    assert s.stats()["factor_active"] == 1

    def engaged(t):
        assert t.stats()["factor_active"] == 1

    _check_representation(lp, s, "compact factor", engaged)


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

    _check_representation(lp, s, "sparse bump", engaged)


@pytest.mark.gpu
def test_hypersparse_re_solve(monkeypatch):
    monkeypatch.setenv("MLP_HYPER", "1")
    lp = lpgen.gen_sparse_lp(400, 300, 12, 7)
    s = lpgen.build_problem(M.Problem, lp).solve()

    def engaged(t):
        assert t.stats()["hyper_iters"] > 0, (t.stats()["hyper_iters"], t.rhs_info())

    _check_representation(lp, s, "hypersparse", engaged)


# ------------------------------------------------------------------------------------------------ 9: after a cut round
@pytest.mark.gpu
def test_a_cut_row_relaxed_after_a_gomory_round():
    """The cut rows of a round on gen_sparse_lp(400, 300, 12, 7) stay tight; one of them gets a right-hand side relaxed by the step.
    The yardstick is the oracle's cold solve of the engine's own matrix (read through state("csr_*")) in its equality form, every
    column of [A | I] a variable with the bounds the engine holds."""
    from oracle import minilp_oracle as O
    lp = _lp("sparse-maximize")
    s = lpgen.build_problem(M.Problem, lp).solve()
    s = s.add_gomory_cuts(_frac_basic(s)[:20])
    n, m = lp["n"], lp["m"]
    assert s.num_constraints == m + 20
    _, cst = s.basis_status()
    lo, hi = s.state("orig_var_mins"), s.state("orig_var_maxs")
    c = next(c for c in range(m, m + 20) if cst[c] != 0)
    b = s.constraint_rhs()
    away = 1.0 if math.isinf(hi[n + c]) else -1.0                                        # slack in [0, inf): a larger right-hand side relaxes
    assert (lo[n + c], hi[n + c]) in ((0.0, INF), (-INF, 0.0))
    new = b[c] + away * 0.05 * max(1.0, abs(b[c]))
    before = s.objective()
    t = s.set_rhs([c], [new])
    assert t.constraint_rhs()[c] == new and t.rhs_info()["solves"] == 1
    assert t.objective() >= before - OBJ_RTOL * max(1.0, abs(before))                   # Maximize: a relaxation makes nothing worse
    Af, cost, rhs = _model_of_state(t)
    assert rhs[c] == new
    A = Af.tocsr()
    eqlp = dict(name="engine", direction=M.MINIMIZE, m=A.shape[0], n=A.shape[1], obj=cost, lo=t.state("orig_var_mins"), hi=t.state("orig_var_maxs"),
                indptr=A.indptr.astype(np.uint64), indices=A.indices.astype(np.uint32), data=A.data, ops=np.full(A.shape[0], lpgen.EQ, dtype=np.int32),
                rhs=rhs)
    oc = lpgen.build_problem(O.Problem, eqlp).solve()
    assert obj_close(-oc.objective(), t.objective()), (oc.objective(), t.objective())    # (internal costs: the Maximize problem negated)
    print("cut row %d relaxed: objective %.12g -> %.12g, %s" % (c, before, t.objective(), t.rhs_info()))


# ------------------------------------------------------------------------------------------------ 10: refusals and verdicts
@pytest.mark.gpu
def test_refusals_and_verdicts():
    """Every refusal leaves the solution the refused clone was taken from bit-identical.  (A solution sharded over several ranks needs
    several processes; what one process can build, a one-rank pump, is refused by rhs_scenarios like every read through the tableau.)
    The hand LP  max x0: 2 x0 + x1 + x2 = b, x1 + x3 <= 5, x2 + x3 <= 5, 0 <= x <= 10  has the optimum x0 = b / 2 while b <= 20: 1.75 at
    b = 3.5.  The left-hand side is at most 2 * 10 + 10 + 10 = 40: b = 45 is Infeasible."""
    from minilp_amd import dist as md
    from oracle import minilp_oracle as O
    lp, s = _solved("mixed")
    m = lp["m"]
    before = _bits(s)
    b = s.constraint_rhs()
    refusals = [lambda t: t.set_rhs([3, 5, 3], [b[3], b[5], b[3]]),                      # listed twice
                lambda t: t.set_rhs([0, m], [b[0], 1.0]),                                # out of range
                lambda t: t.set_rhs([2], [math.nan]),
                lambda t: t.set_rhs([2], [INF]),
                lambda t: t.set_rhs([2], [-INF])]
    for bad in refusals:
        t = s.clone()
        with pytest.raises(M.InternalError) as e:
            bad(t)
        assert e.value.code == -1 and not t._h.value
    t = s.clone()                                                                        # NULL arrays with n > 0
    h = t._take()
    assert M.lib().mlp_solution_set_rhs(ctypes.byref(h), None, None, 2) == -1 and not h.value
    reads = [lambda: s.rhs_scenarios([3, 5, 3], np.zeros((2, 3))), lambda: s.rhs_scenarios([0, m], np.zeros((2, 2))),
             lambda: s.rhs_scenarios([2], np.array([[math.nan]])), lambda: s.rhs_scenarios([2], np.array([[1.0], [INF]])),
             lambda: s.constraint_rhs([m])]
    for bad in reads:
        with pytest.raises(M.InternalError) as e:
            bad()
        assert e.value.code == -1
    with pytest.raises(M.InternalError):
        s.clone().set_rhs([0, 1], [1.0])                                                 # lengths differ (caught by the binding)
    with pytest.raises(M.InternalError):
        s.rhs_scenarios([0, 1], np.zeros((2, 3)))
    assert _bits(s) == before and s._h.value
    # an unsolved (budget = 0) solution: the mutator and the what-if read refuse, the host read works
    prob = lpgen.build_problem(M.Problem, lp)
    for call in (lambda t: t.set_rhs([2], [b[2]]), lambda t: t.rhs_scenarios([2], np.array([[b[2]]]))):
        t = prob.solve(budget=0)
        with pytest.raises(M.InternalError) as e:
            call(t)
        assert e.value.code == -1 and "not solved" in str(e.value)
    t = prob.solve(budget=0)
    assert t.constraint_rhs().tobytes() == lp["rhs"].tobytes()
    bt = _bits(t)
    t = t.set_rhs([], [])                                                                # nothing listed: the no-op of every mutator, on any state
    assert _bits(t) == bt and t.budget_exhausted and t.rhs_info()["requests"] == 0
    # a one-rank pump
    t = prob.solve(budget=0)
    box = md.create_mailbox(1)
    try:
        t.enable_sharding_ex(0, 1, box, "pump")
        with pytest.raises(M.InternalError) as e:
            t.rhs_scenarios([2], np.array([[b[2]]]))
        assert e.value.code == -1 and "sharded" in str(e.value)
    finally:
        md.remove_mailbox(box)
    # a constraint without terms has no row: its right-hand side is stored, and 0 op rhs must stay true
    p = lpgen.build_problem(M.Problem, _hand_lp())
    p.add_constraint([], M.LE, 2.0)
    q = p.solve()
    assert q.num_constraints == 4 and q.constraint_rhs()[3] == 2.0
    bq = _bits(q)[:3]
    q = q.set_rhs([3], [0.5])                                                            # 0 <= 0.5: still a tautology
    assert q.constraint_rhs()[3] == 0.5 and q.constraint_rhs([3, 0]).tolist() == [0.5, 3.0] and _bits(q)[:3] == bq
    assert q.rhs_info()["solves"] == 0 and q.rhs_info()["changed"] == 1 and q.clone().constraint_rhs()[3] == 0.5
    with pytest.raises(M.InternalError):
        q.rhs_scenarios([3], np.array([[1.0]]))                                          # no row: nothing to evaluate
    with pytest.raises(M.Infeasible):
        q.set_rhs([3], [-1.0])                                                           # 0 <= -1
    assert not q._h.value
    # the pinned Infeasible lists, built from the oracle's optimum (a verdict is a property of the list alone)
    for name, kind, k in sorted(PINNED_INFEASIBLE):
        olp, x, st, _ = _oracle_point(name)
        cs, vals = rhs_list(olp, x, st, kind, k)
        t = _solved(name)[1].clone()
        with pytest.raises(M.Infeasible):
            t.set_rhs(cs, vals)
        assert not t._h.value
    # the equality row of the hand LP
    hand = _hand_lp()
    q = lpgen.build_problem(M.Problem, hand).solve()
    assert abs(q.objective() - 1.5) <= 1e-12
    t = q.clone().set_rhs([0], [3.5])
    assert abs(t.objective() - 1.75) <= 1e-12 and abs(t.values()[0] - 1.75) <= 1e-12
    assert obj_close(lpgen.build_problem(O.Problem, _with_rhs(hand, [0], [3.5])).solve().objective(), 1.75)
    with pytest.raises(O.Infeasible):
        lpgen.build_problem(O.Problem, _with_rhs(hand, [0], [45.0])).solve()
    t = q.clone()
    with pytest.raises(M.Infeasible):
        t.set_rhs([0], [45.0])
    assert not t._h.value
    got = q.rhs_scenarios([0], np.array([[3.5], [45.0]]))
    assert got["feasible"].tolist() == [True, False] and abs(got["bound"][0] - 1.75) <= 1e-12 and got["worst_col"][1] == 0   # x0 = 22.5 > 10


# ------------------------------------------------------------------------------------------------ 11: the example
@pytest.mark.gpu
def test_solve_mps_example_sweeps_a_right_hand_side(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("solve_mps_rhs", os.path.join(ROOT, "examples", "solve_mps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lp = _lp("small-mixed")
    path = tmp_path / "mixed.mps"
    path.write_text(lpgen.to_mps(lp))
    s = lpgen.build_problem(M.Problem, lp).solve()
    _, cst = s.basis_status()
    row = next(i for i in range(lp["m"]) if cst[i] != 0 and lp["ops"][i] != lpgen.EQ)
    b = float(lp["rhs"][row])
    lo, hi = b, b + (1.0 if lp["ops"][row] == lpgen.LE else -1.0)                        # a relaxation: every step is feasible
    assert mod.run(M, str(path), rhs_sweep="%d:%r:%r:5" % (row, lo, hi)) == 0
    out = capsys.readouterr().out
    what_if = re.findall(r"what-if +row %d = (\S+): bound (\S+) (feasible|pivots needed)" % row, out)
    chain = re.findall(r"set_rhs +row %d = (\S+): (?:optimum (\S+), (\d+) pivots|infeasible)" % row, out)
    assert len(what_if) == 5 == len(chain), out
    assert [float(w[0]) for w in what_if] == [float(c[0]) for c in chain] and float(chain[0][0]) == lo and float(chain[-1][0]) == hi
    assert np.allclose([float(c[0]) for c in chain], np.linspace(lo, hi, 5), rtol=0, atol=1e-12)
    assert what_if[0][2] == "feasible" and int(chain[0][2]) == 0                         # the first step is the model as it stands
    want = lpgen.build_problem(M.Problem, _with_rhs(lp, [row], [hi])).solve().objective()
    assert obj_close(float(chain[-1][1]), want, 1e-9), (chain[-1], want)                 # (printed with 12 digits)
    assert mod.run(M, str(path), rhs_sweep="%d:0:1" % row) == 1                           # a malformed request


# ------------------------------------------------------------------------------------------------ measurement
TIGHTEN_K = 64  # the largest of 64, 16, 4, 1 at which HiGHS finds the tighten list of gen_mixed_lp(6000, 10000, 4, 3) feasible (it finds all four
                # feasible: 5227.779 at 64 against 5219.425), built from the oracle's optimum on the CPU


@pytest.mark.gpu
def test_warm_against_cold_and_scenarios_against_the_host_route():
    """gen_mixed_lp(6000, 10000, 4, 3), median of 5 after one warm-up, one process, wall clock.
    (a) set_rhs of the tighten list of TIGHTEN_K rows on a clone against Problem.solve() of the changed model: the warm call must not be
        slower.
    (b) 64 scenarios of 16 constraints through rhs_scenarios against the same 64 dense vectors through basis_solve and the numpy
        evaluation: the device route must not be slower.  device_ms of both is recorded, not asserted.
    Written to profiles/rhs.json when MLP_WRITE_PROFILES=1; the recorded run is in DESIGN.md §7.10."""
    lp = lpgen.gen_mixed_lp(6000, 10000, 4, 3)
    s = lpgen.build_problem(M.Problem, lp).solve()
    _, cst = s.basis_status()
    cs, vals = rhs_list(lp, s.values(), cst, "tighten", TIGHTEN_K)
    assert len(cs) == TIGHTEN_K
    prob2 = lpgen.build_problem(M.Problem, _with_rhs(lp, cs, vals))
    sc, rhs = _scenarios(lp, s, 64)
    assert len(sc) == 16
    warm, cold, dev, host = [], [], [], []
    winfo = cstats = dinfo = hinfo = None
    for rep in range(6):
        a = s.clone()
        t0 = time.perf_counter()
        a = a.set_rhs(cs, vals)
        t1 = time.perf_counter()
        c = prob2.solve()
        t2 = time.perf_counter()
        got = s.rhs_scenarios(sc, rhs)
        t3 = time.perf_counter()
        dinfo = s.rhs_info()
        t4 = time.perf_counter()
        want = _host_scenarios(s, lp, sc, rhs)
        t5 = time.perf_counter()
        hinfo = s.tableau_info()
        winfo, cstats = a.rhs_info(), c.stats()
        assert obj_close(a.objective(), c.objective()), (a.objective(), c.objective())
        assert (got["feasible"] == want["feasible"]).all()
        if rep:
            warm.append((t1 - t0) * 1e3); cold.append((t2 - t1) * 1e3); dev.append((t3 - t2) * 1e3); host.append((t5 - t4) * 1e3)
    rec = dict(instance="gen_mixed_lp(6000, 10000, 4, 3)", tighten_k=TIGHTEN_K, set_rhs_wall_ms=float(np.median(warm)),
               cold_solve_wall_ms=float(np.median(cold)), warm_ratio=float(np.median(cold) / np.median(warm)), set_rhs_pivots=winfo["pivots"],
               cold_solve_pivots=cstats["iterations"], set_rhs_device_ms=winfo["device_ms"], scenarios=64, constraints=16,
               rhs_scenarios_wall_ms=float(np.median(dev)), host_route_wall_ms=float(np.median(host)),
               scenario_ratio=float(np.median(host) / np.median(dev)), rhs_scenarios_device_ms=dinfo["device_ms"],
               basis_solve_device_ms=hinfo["device_ms"], rhs_scenarios_bytes=dinfo["bytes"], basis_solve_bytes=hinfo["bytes"])
    print("RHS " + json.dumps(rec))
    if os.environ.get("MLP_WRITE_PROFILES") == "1":
        with open(os.path.join(ROOT, "profiles", "rhs.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    assert rec["warm_ratio"] >= 1.0 and rec["scenario_ratio"] >= 1.0, rec
