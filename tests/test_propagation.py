"""GPU: bound propagation from row activities (include/minilp_hip.h: mlp_solution_propagate_bounds,
mlp_solution_tighten_by_propagation, mlp_propagate_info; csrc/propagate.inc).

The reference library has no counterpart.  The yardstick of the read is tests/propagation_ref.py, the numpy restatement of the rules in
the header: on integer data every sum is exact and every candidate is one IEEE division, so the device's list must equal it with ==;
on continuous data the bounds agree to 1e-9 max(1, |bound|) and the listed sets and the number of rounds are equal
(tests/test_propagation_ref.py shows that no acceptance of these instances sits near its threshold).  The yardstick of the mutator is the
cold solve of the model with the listed bounds, on the oracle and HiGHS, as in tests/test_bounds.py.

A model that three fixings make infeasible cannot be reached through fix_vars (its re-solve says Infeasible and frees the solution):
those states are set up as a Problem with the closed bounds and solve(budget=0), which the read serves like any other state."""
import importlib.util
import math
import os

import numpy as np
import pytest

import minilp_amd as M
from minilp_amd import lpgen
from tests import degenerate_lp as D
from tests.bounded_lp import gen_bounded_lp
from tests.common import HIGHS_RTOL, OBJ_RTOL, ROOT, X_ATOL, check_feasible, obj_close
from tests.propagation_ref import internal_form, propagate
from tests.test_bounds import _cold, _with_bounds
from tests.test_branch_penalties import INSTANCES, KNAPSACK_SEEDS, _blob, _knapsack
from tests.test_propagation_ref import chain_lp, hand, row_vars

pytestmark = pytest.mark.gpu

INF = math.inf
CONTINUOUS = {"mixed": INSTANCES["mixed"], "small-mixed": INSTANCES["small-mixed"], "sparse-maximize": INSTANCES["sparse-maximize"],
              "cover": INSTANCES["cover"], "bounded": (gen_bounded_lp, (300, 400, 6, 3))}
UNIQUE = ("cover", "sparse-maximize", "bounded")
INTEGER = {"two_matching": lambda: D.two_matching(D.grid_points(4, 4)), "assignment": lambda: D.assignment(6, 1),
           "unit_packing": lambda: D.unit_packing(30, 40, 4, 1), "unit_cover": lambda: D.unit_cover(30, 40, 4, 1)}
INTEGER.update({"knapsack_%d" % s: (lambda s=s: _knapsack(s)) for s in KNAPSACK_SEEDS})


def _solve(lp, **kw):
    return lpgen.build_problem(M.Problem, lp).solve(**kw)


def form_of(s):
    """The internal form as the solution holds it (rows appended by cuts included), and the columns its flags fix."""
    st = lambda k: np.asarray(s.state(k))
    form = (st("csr_indptr").astype(np.int64), st("csr_indices").astype(np.int64), st("csr_data"), st("orig_rhs"), st("orig_var_mins"),
            st("orig_var_maxs"))
    flags, nbv, xn = st("nb_flags").astype(np.int64), st("nb_vars").astype(np.int64), st("nb_var_vals")
    return form, {int(nbv[c]): float(xn[c]) for c in np.flatnonzero(flags & 4)}


def _ref_of(s, marks=None, max_rounds=10):
    form, fixed = form_of(s)
    return propagate(form, s.num_vars, fixed, marks, max_rounds)


def _same_exactly(dev, ref, label):
    v, lo, hi, inf = dev
    assert inf == ref["infeasible"], (label, inf)
    assert v.tolist() == ref["vars"].tolist(), (label, v.tolist(), ref["vars"].tolist())
    assert lo.tobytes() == ref["lo"].tobytes() and hi.tobytes() == ref["hi"].tobytes(), (label, lo, ref["lo"], hi, ref["hi"])


def _info_matches(s, dev, ref, label):
    info = s.propagate_info()
    assert info["rounds"] == ref["rounds"] and info["listed"] == len(dev[0]) and info["listed_fixed"] == int((dev[1] == dev[2]).sum()), (label, info)
    assert info["requests"] == len(np.asarray(s.state("orig_var_mins"))) and info["bytes"] > 0 and info["device_ms"] > 0, (label, info)
    if not ref["infeasible"]:
        assert info["accepted"] == ref["accepted"], (label, info, ref["accepted"])


# ------------------------------------------------------------------------------------------------ integer data: exact equality
@pytest.mark.parametrize("name", list(INTEGER))
def test_integer_data_equals_the_reference_exactly(name):
    lp = INTEGER[name]()
    n = lp["n"]
    assert form_of(_solve(lp, budget=0))[0][2].tobytes() == internal_form(lp)[2].tobytes()          # the two ways to the model agree
    base = _solve(lp)
    seen = dict(feasible=0, infeasible=0, listed=0)
    for k in (0, 1, 2, 3):
        js = row_vars(lp, 0, k)
        s = None
        if k:
            try:
                s = base.clone().fix_vars(js, [1.0] * k)
            except M.Infeasible:
                closed = _with_bounds(lp, js, [1.0] * k, [1.0] * k)                                   # the LP with the fixings is infeasible:
                s = _solve(closed, budget=0)                                                         # closed bounds, no pivot
        else:
            s = base
        for marks in (None, np.ones(n, bool)):
            label = (name, k, marks is not None)
            ref = _ref_of(s, marks)
            dev = s.propagate_bounds(marks)
            _same_exactly(dev, ref, label)
            _info_matches(s, dev, ref, label)
            seen["infeasible" if dev[3] else "feasible"] += 1
            seen["listed"] += len(dev[0])
    print(name, seen)
    assert seen["feasible"] >= 2


def test_the_figures_of_the_design_document():
    tm = INTEGER["two_matching"]()
    s = _solve(tm).fix_vars(row_vars(tm, 0, 2), [1.0, 1.0])
    v, lo, hi, inf = s.propagate_bounds()
    assert len(v) == 13 and (lo == 0.0).all() and (hi == 0.0).all() and not inf and s.propagate_info()["listed_fixed"] == 13
    js = row_vars(tm, 0, 3)
    v, lo, hi, inf = _solve(_with_bounds(tm, js, [1.0] * 3, [1.0] * 3), budget=0).propagate_bounds()
    assert inf and len(v) == 0
    a = INTEGER["assignment"]()
    s = _solve(a).fix_vars(row_vars(a, 0, 1), [1.0])
    v, lo, hi, inf = s.propagate_bounds(np.ones(36, bool))
    assert (len(v), int((lo == hi).sum()), inf) == (35, 10, False)
    b = gen_bounded_lp(300, 400, 6, 3)
    s = _solve(b)
    assert len(s.propagate_bounds()[0]) == 189
    v, _, _, inf = s.propagate_bounds(np.ones(400, bool))
    assert inf and len(v) == 0 and s.propagate_info()["rounds"] == 1


# ------------------------------------------------------------------------------------------------ continuous data
def _bounds_after(s, dev):
    lo, hi = s.var_bounds()
    lo[dev[0]], hi[dev[0]] = dev[1], dev[2]
    return lo, hi


def _close(a, b):
    fin = np.isfinite(b)
    return (np.isfinite(a) == fin).all() and (a[~fin] == b[~fin]).all() and (np.abs(a[fin] - b[fin]) <= 1e-9 * np.maximum(1.0, np.abs(b[fin]))).all()


@pytest.mark.parametrize("name", list(CONTINUOUS))
def test_continuous_data_agrees_with_the_reference(name):
    gen, args = CONTINUOUS[name]
    lp = gen(*args)
    n = lp["n"]
    s = _solve(lp)
    ref = propagate(internal_form(lp), n)
    dev = s.propagate_bounds()
    assert not dev[3] and not ref["infeasible"]
    assert dev[0].tolist() == ref["vars"].tolist(), name
    lo, hi = _bounds_after(s, dev)
    assert _close(lo, ref["lo_all"][:n]) and _close(hi, ref["hi_all"][:n]), name
    assert s.propagate_info()["rounds"] == ref["rounds"] and s.propagate_info()["accepted"] == ref["accepted"], (name, s.propagate_info())
    for rounds in (1, 3):
        ref = propagate(internal_form(lp), n, max_rounds=rounds)
        dev = s.propagate_bounds(max_rounds=rounds)
        assert dev[0].tolist() == ref["vars"].tolist() and s.propagate_info()["rounds"] == ref["rounds"], (name, rounds)


# ------------------------------------------------------------------------------------------------ shapes that can go wrong
def test_a_dense_row_over_1500_columns():
    lp = _knapsack(5, n=1500)                                                                # 3 rows x 1500: more entries than one group trip covers
    for s in (_solve(lp, budget=0), _solve(lp)):
        for marks in (None, np.ones(1500, bool)):
            _same_exactly(s.propagate_bounds(marks), propagate(internal_form(lp), 1500, is_int=marks), "dense row")
    s = _solve(dict(lp, hi=np.full(1500, 1e4)), budget=0)                                   # ... and bounds that the rows do tighten
    dev = s.propagate_bounds(np.ones(1500, bool))
    _same_exactly(dev, _ref_of(s, np.ones(1500, bool)), "dense row, wide boxes")
    assert len(dev[0]) == 1500


def test_a_dense_column_through_1500_rows():
    m, n = 1500, 40
    rows = [([0, 1 + r % (n - 1)], [1.0 + r % 3, 2.0], lpgen.LE, float(8 + r % 5)) for r in range(m)]
    lp = hand(np.zeros(n), np.full(n, 100.0), rows, lpgen.MAXIMIZE)
    s = _solve(lp, budget=0)
    dev = s.propagate_bounds()
    _same_exactly(dev, propagate(internal_form(lp), n), "dense column")
    assert 0 in dev[0].tolist() and dev[2][0] == 8.0 / 3.0


def test_a_constraint_without_terms_and_maximize():
    lp = hand([0, 0, 0], [10, 10, 10], [([0, 1], [1.0, 1.0], lpgen.LE, 4.0), ([], [], lpgen.LE, 1.0), ([1, 2], [2.0, -1.0], lpgen.GE, 2.0)],
              lpgen.MAXIMIZE)
    for s in (_solve(lp, budget=0), _solve(lp)):
        assert s.num_constraints == 3 and len(np.asarray(s.state("orig_rhs"))) == 2
        dev = s.propagate_bounds()
        _same_exactly(dev, propagate(internal_form(lp), 3), "no terms")
        _same_exactly(dev, _ref_of(s), "no terms, from the state")
        assert dev[0].tolist() == [0, 1, 2] and dev[1].tolist() == [0.0, 1.0, 0.0] and dev[2].tolist() == [3.0, 4.0, 6.0]


def test_the_chain_lists_one_more_variable_per_round():
    lp = chain_lp(12)
    s = _solve(lp, budget=0)
    for rounds, want in ((1, [11]), (10, list(range(2, 12))), (64, list(range(12)))):
        dev = s.propagate_bounds(max_rounds=rounds)
        _same_exactly(dev, propagate(internal_form(lp), 13, max_rounds=rounds), rounds)
        assert dev[0].tolist() == want and (dev[1] == 1.0).all()
    assert s.propagate_info()["rounds"] == 13


def test_appended_rows_and_gomory_cut_rows_with_foreign_slacks():
    lp = _knapsack(2)
    n = lp["n"]
    s = _solve(lp)
    s = s.add_constraints([([(0, 1.0), (1, 1.0), (2, 1.0)], lpgen.LE, 2.0), ([(3, 2.0), (4, -1.0)], lpgen.GE, -1.0)])
    x = s.values()
    vs, _ = s.basis_status()
    frac = [j for j in range(n) if vs[j] == 0 and abs(x[j] - round(x[j])) > 1e-6]
    assert frac
    s = s.add_gomory_cuts(frac[:2])
    form, fixed = form_of(s)
    nrows = len(form[3])
    assert nrows == 5 + len(frac[:2])
    foreign = [int(j) for r in range(5, nrows) for j in form[1][form[0][r]:form[0][r + 1]] if j >= n and j != n + r]
    print("cut row terms on the slacks of other rows:", foreign)
    assert foreign                                                                            # the cut rows carry slacks of other rows
    for marks in (None, np.ones(n, bool)):
        dev = s.propagate_bounds(marks)
        ref = propagate(form, n, fixed, marks)
        assert dev[3] == ref["infeasible"] and dev[0].tolist() == ref["vars"].tolist()
        assert _close(dev[1], ref["lo"]) and _close(dev[2], ref["hi"])
        if marks is None and not dev[3]:                                                      # every listed bound holds at the LP optimum
            x = s.values()
            assert (x[dev[0]] >= dev[1] - 1e-7).all() and (x[dev[0]] <= dev[2] + 1e-7).all()


def test_past_the_grid_cap():
    """600 000 rows x_i + x_{i+1} <= 1 on 600 001 non-negative variables: more rows and columns than 524 288."""
    n = 600001
    idx = np.stack((np.arange(n - 1), np.arange(1, n)), axis=1).reshape(-1).astype(np.uint32)
    lp = dict(name="chain", direction=lpgen.MAXIMIZE, m=n - 1, n=n, obj=np.ones(n), lo=np.zeros(n), hi=np.full(n, INF),
              indptr=np.arange(0, 2 * n - 1, 2, dtype=np.uint64), indices=idx, data=np.ones(2 * (n - 1)),
              ops=np.full(n - 1, lpgen.LE, dtype=np.int32), rhs=np.ones(n - 1))
    s = _solve(lp, budget=0)
    v, lo, hi, inf = s.propagate_bounds()
    info = s.propagate_info()
    assert not inf and len(v) == n and (v == np.arange(n)).all() and (lo == 0.0).all() and (hi == 1.0).all(), (len(v), info)
    assert info["listed"] == n and info["rounds"] == 2 and info["accepted"] == n + (n - 1), info    # (every slack gets the upper bound 1 too)


# ------------------------------------------------------------------------------------------------ independence of the basis
@pytest.mark.parametrize("name", ["mixed", "bounded", "sparse-maximize"])
def test_the_read_is_independent_of_the_basis_and_has_no_side_effects(name):
    gen, args = CONTINUOUS[name]
    lp = gen(*args)
    cold, mid, done = _solve(lp, budget=0), _solve(lp, budget=25), _solve(lp)
    blob, obj, x = _blob(done), done.objective(), done.values().tobytes()
    reads = [t.propagate_bounds() for t in (cold, mid, done, done)]
    for r in reads[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(r[:3], reads[0][:3])) and r[3] == reads[0][3]
    assert _blob(done) == blob and done.objective() == obj and done.values().tobytes() == x
    marks = np.zeros(lp["n"], bool)
    marks[::3] = True
    a, b = cold.propagate_bounds(marks, 4), done.propagate_bounds(marks, 4)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a[:3], b[:3])) and a[3] == b[3]
    mid.continue_solve(-1)                                                                    # the read left the paused solve intact
    assert obj_close(mid.objective(), obj)


# ------------------------------------------------------------------------------------------------ the mutator
@pytest.mark.parametrize("name", list(CONTINUOUS))
def test_without_marks_at_an_optimum_nothing_moves(name):
    gen, args = CONTINUOUS[name]
    lp = gen(*args)
    s = _solve(lp)
    obj, x = s.objective(), s.values()
    t, count, inf = s.clone().tighten_by_propagation()                                        # the default: 10 rounds
    assert not inf and count == len(s.propagate_bounds()[0]) and t.bounds_info()["shifted"] == 0 and t.bounds_info()["pivots"] == 0
    # 64 rounds reach the fixed point on every instance (the default stops mixed, small-mixed and bounded while bounds still move, so a
    # second call at the default goes on where the first one stopped); after the fixed point a second call finds nothing
    want = s.propagate_bounds(max_rounds=64)
    assert s.propagate_info()["rounds"] < 64
    t, count, inf = s.clone().tighten_by_propagation(max_rounds=64)
    info = t.bounds_info()
    assert not inf and count == len(want[0]) == t.propagate_info()["listed"]
    assert info["shifted"] == 0 and info["pivots"] == 0 and info["requests"] == count, info
    assert obj_close(t.objective(), obj) and np.abs(t.values() - x).max() <= X_ATOL
    lo, hi = t.var_bounds()
    assert lo[want[0]].tobytes() == want[1].tobytes() and hi[want[0]].tobytes() == want[2].tobytes()
    t, again, inf = t.tighten_by_propagation(max_rounds=64)
    assert again == 0 and not inf
    print(name, "tightened", count, info)


def _marked_cases():
    yield "mixed", CONTINUOUS["mixed"][0](*CONTINUOUS["mixed"][1])
    yield "bounded", CONTINUOUS["bounded"][0](*CONTINUOUS["bounded"][1])
    for seed in KNAPSACK_SEEDS:
        lp = _knapsack(seed)
        yield "knapsack_%d" % seed, dict(lp, hi=np.full(11, 3.0), indptr=lp["indptr"].astype(np.int64))   # (boxes that the rows do tighten)


@pytest.mark.parametrize("name,lp", list(_marked_cases()), ids=[c[0] for c in _marked_cases()])
def test_with_marks_against_the_cold_solve(name, lp):
    n = lp["n"]
    marks = np.ones(n, bool)
    s = _solve(lp)
    v, lo, hi, inf = s.propagate_bounds(marks)
    before = (s.objective(), s.values().tobytes(), _blob(s))
    try:
        t, count, inf2 = s.clone().tighten_by_propagation(marks)
    except M.Infeasible:
        t, count, inf2 = None, len(v), False
    assert inf2 == inf and (s.objective(), s.values().tobytes(), _blob(s)) == before
    if inf:                                                                                   # left as it is
        assert count == 0 and t.objective() == before[0] and t.values().tobytes() == before[1] and _blob(t) == before[2]
        assert t.var_bounds()[0].tobytes() == s.var_bounds()[0].tobytes() and t.var_bounds()[1].tobytes() == s.var_bounds()[1].tobytes()
        print(name, "infeasible by propagation")
        return
    assert count == len(v)
    lp2 = _with_bounds(lp, v.astype(np.int64), lo, hi)
    oc, hg = _cold(lp2, ("propagation", name))
    assert (t is None) == (oc is None) == (hg is None), (name, t is None, oc is None, hg)
    if t is None:
        return
    assert obj_close(t.objective(), oc.objective()) and obj_close(t.objective(), hg, HIGHS_RTOL), (name, t.objective(), oc.objective(), hg)
    check_feasible(lp2, t.values())
    if name in UNIQUE:
        assert np.abs(t.values() - oc.values()).max() <= X_ATOL
    print(name, "tightened", count, t.bounds_info())


def _branch_and_bound(lp, propagate_at_nodes):
    """tests/test_bounds.py's depth-first search over set_var_bounds branches; with propagation every node tightens first."""
    n = lp["n"]
    marks = np.ones(n, bool)
    best, nodes = -INF, 0
    stack = [_solve(lp)]
    while stack:
        node = stack.pop()
        nodes += 1
        if node.objective() <= best + 1e-9:
            continue
        if propagate_at_nodes:
            try:
                node, _, inf = node.tighten_by_propagation(marks)
            except M.Infeasible:
                continue
            if inf or node.objective() <= best + 1e-9:
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


def test_branch_and_bound_reaches_the_integer_optimum_with_and_without_propagation():
    import itertools
    for seed in KNAPSACK_SEEDS:
        lp = _knapsack(seed)
        n = lp["n"]
        X = np.array(list(itertools.product((0.0, 1.0), repeat=n)))
        X = X[(X @ lp["data"].reshape(3, n).T <= lp["rhs"] + 1e-9).all(axis=1)]
        want = float((X @ lp["obj"]).max())
        plain, n0 = _branch_and_bound(lp, False)
        prop, n1 = _branch_and_bound(lp, True)
        print("%s: optimum %g, %d nodes plain, %d with propagation" % (lp["name"], want, n0, n1))
        assert abs(plain - want) <= 1e-7 and abs(prop - want) <= 1e-7, (seed, want, plain, prop)


def test_tsp_example_with_propagation_returns_the_same_tour():
    from tests.test_fixing import TSP_CITIES, TSP_SEED, _load_example
    tsp = _load_example("tsp")
    pts = np.random.default_rng(TSP_SEED).uniform(0.0, 100.0, size=(TSP_CITIES, 2))
    plain, prop = tsp.TspSolver(M, pts), tsp.TspSolver(M, pts, propagate=True)
    c0, t0 = plain.solve()
    c1, t1 = prop.solve()
    print("14 cities: plain %s; --propagate %s" % (plain.stats, prop.stats))
    assert abs(c0 - c1) <= 1e-9 * max(1.0, abs(c0)) and abs(prop.tour_cost(t1) - c1) <= 1e-7 and sorted(t1) == list(range(TSP_CITIES))
    cyc = lambda t: min(tuple(t[i:] + t[:i]) for i in (t.index(0),))                          # the same tour, whichever way round
    assert cyc(t1) == cyc(t0) or cyc(t1) == cyc(t0[::-1]), (t0, t1)
    assert prop.stats["prop_calls"] >= 1 and "prop_calls" not in plain.stats


# ------------------------------------------------------------------------------------------------ every representation of B^-1
def _check_application(lp, s, label, engaged):
    n = lp["n"]
    marks = np.ones(n, bool)
    v, lo, hi, inf = s.propagate_bounds(marks)
    assert not inf and len(v) > 0, label
    try:
        t, count, _ = s.tighten_by_propagation(marks)
    except M.Infeasible:
        t = None
    oc, hg = _cold(_with_bounds(lp, v.astype(np.int64), lo, hi), ("propagation rep", label))
    assert (t is None) == (oc is None) == (hg is None), label
    if t is not None:
        assert obj_close(t.objective(), oc.objective()) and obj_close(t.objective(), hg, HIGHS_RTOL), (label, t.objective(), oc.objective(), hg)
        check_feasible(_with_bounds(lp, v.astype(np.int64), lo, hi), t.values())
        engaged(t)
        print(label, t.bounds_info())


def _wide_sparse():
    return lpgen.gen_sparse_lp(200, 150, 8, 3)


def test_default_representation():
    lp = _wide_sparse()
    _check_application(lp, _solve(lp), "default", lambda t: None)


def test_pending_terms_of_the_delayed_update_mode(monkeypatch):
    from tests.test_gmi_cuts import _pending, _solved_with_pending_terms
    monkeypatch.setenv("MLP_LOWRANK", "3")
    s, lp, _ = _solved_with_pending_terms(_wide_sparse(), True)
    assert int(s.state("lowrank_pending")[1]) == 3 and _pending(s) > 0
    _check_application(lp, s, "pending terms", lambda t: None)


def test_compact_factor(monkeypatch):
    monkeypatch.setenv("MLP_FACTOR", "1")
    lp = lpgen.gen_transport_lp(600, 700, 4, 5, tight=0.45)
    s = _solve(lp)
    assert s.stats()["factor_active"] == 1

    def engaged(t):
        assert t.stats()["factor_active"] == 1

    _check_application(lp, s, "compact factor", engaged)


def test_compact_factor_sparse_bump(monkeypatch):
    monkeypatch.setenv("MLP_FACTOR", "1")
    monkeypatch.setenv("MLP_FACTOR_SB_FROM", "2")
    s = lp = None
    for gen, args in ((lpgen.gen_sparse_lp, (400, 300, 12, 7)), (lpgen.gen_mixed_lp, (300, 400, 6, 3)), (lpgen.gen_sparse_lp, (1500, 1400, 12, 9))):
        lp = gen(*args)
        s = _solve(lp)
        if s.stats()["factor_active"] == 1 and s.state("factor_sb")[0] == 1:
            break
    assert s.stats()["factor_active"] == 1 and s.state("factor_sb")[0] == 1

    def engaged(t):
        assert t.stats()["factor_active"] == 1 and t.state("factor_sb")[0] == 1

    _check_application(lp, s, "sparse bump", engaged)


def test_hypersparse_re_solve(monkeypatch):
    monkeypatch.setenv("MLP_HYPER", "1")
    lp = lpgen.gen_sparse_lp(400, 300, 12, 7)

    def engaged(t):
        assert t.bounds_info()["pivots"] == 0 or t.stats()["hyper_iters"] > 0, (t.stats()["hyper_iters"], t.bounds_info())

    _check_application(lp, _solve(lp), "hypersparse", engaged)


# ------------------------------------------------------------------------------------------------ refusals, clones
def test_refusals():
    import ctypes as C
    lp = lpgen.gen_mixed_lp(40, 30, 6, 9)
    n = lp["n"]
    s = _solve(lp)
    before = (s.objective(), s.values().tobytes(), _blob(s))
    for bad in (lambda t: t.propagate_bounds(max_rounds=0), lambda t: t.propagate_bounds(max_rounds=65), lambda t: t.propagate_bounds(max_rounds=-1)):
        with pytest.raises(M.InternalError) as e:
            bad(s)
        assert e.value.code == -1
    for bad in (lambda t: t.tighten_by_propagation(max_rounds=0), lambda t: t.tighten_by_propagation(max_rounds=65)):
        t = s.clone()
        with pytest.raises(M.InternalError) as e:
            bad(t)
        assert e.value.code == -1 and not t._h.value
    L = M.lib()
    pu, pd, pb = C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    v, lo, hi, mask = np.zeros(n, dtype=np.uint32), np.zeros(n), np.zeros(n), np.ones(n + 1, dtype=np.uint8)
    cnt, inf = C.c_uint64(), C.c_int()
    args = lambda nv, cap: (s._h, mask.ctypes.data_as(pb), nv, 10, v.ctypes.data_as(pu), lo.ctypes.data_as(pd), hi.ctypes.data_as(pd), cap,
                            C.byref(cnt), C.byref(inf))
    assert L.mlp_solution_propagate_bounds(*args(n + 1, n)) == -1 and L.mlp_solution_propagate_bounds(*args(n - 1, n)) == -1   # the mask's length
    want = s.propagate_bounds(np.ones(n, bool))
    assert len(want[0]) >= 2
    assert L.mlp_solution_propagate_bounds(*args(n, len(want[0]) - 1)) == -1 and cnt.value == len(want[0])                     # cap too small
    assert L.mlp_solution_propagate_bounds(*args(n, len(want[0]))) == 0 and v[:cnt.value].tolist() == want[0].tolist()
    assert L.mlp_solution_propagate_bounds(s._h, None, n, 10, None, None, None, n, None, C.byref(inf)) == -1
    assert (s.objective(), s.values().tobytes(), _blob(s)) == before
    t = lpgen.build_problem(M.Problem, lp).solve(budget=5)                                     # the mutator needs a solved model ...
    t.propagate_bounds()                                                                       # (... the read does not)
    with pytest.raises(M.InternalError) as e:
        t.tighten_by_propagation()
    assert e.value.code == -1


def test_a_sharded_solution_is_refused():
    from minilp_amd import dist as md
    prob = lpgen.build_problem(M.Problem, lpgen.gen_mixed_lp(40, 30, 6, 9))
    box = md.create_mailbox(1)
    try:
        for call in (lambda t: t.propagate_bounds(), lambda t: t.tighten_by_propagation()):
            t = prob.solve()
            t.enable_sharding_ex(0, 1, box, "pump")
            with pytest.raises(M.InternalError) as e:
                call(t)
            assert e.value.code == -1
    finally:
        md.remove_mailbox(box)


def test_a_clone_keeps_its_parent_untouched():
    lp = lpgen.gen_mixed_lp(300, 400, 6, 3)
    parent, twin = _solve(lp), _solve(lp)
    bits = lambda s: (s.objective(), s.values().tobytes(), _blob(s), s.var_bounds()[0].tobytes(), s.var_bounds()[1].tobytes())
    assert bits(parent) == bits(twin)
    child, count, inf = parent.clone().tighten_by_propagation()
    assert count == 200 and not inf and child.var_bounds()[1].tobytes() != parent.var_bounds()[1].tobytes()
    assert bits(parent) == bits(twin)


# ------------------------------------------------------------------------------------------------ the example, the measurement
def test_solve_mps_example_prints_the_count_and_the_info(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("solve_mps_propagate", os.path.join(ROOT, "examples", "solve_mps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lp = lpgen.gen_mixed_lp(40, 30, 6, 9)
    path = tmp_path / "mixed.mps"
    path.write_text(lpgen.to_mps(lp))
    assert mod.run(M, str(path)) == 0
    assert "propagation" not in capsys.readouterr().out                                       # without the flag: as before
    assert mod.run(M, str(path), propagate=True) == 0
    out = capsys.readouterr().out
    assert "propagation: 17 variables tightened" in out and "'rounds': 10" in out and "'shifted': 0" in out, out


def test_a_round_costs_no_more_than_twice_the_certificate():
    """gen_mixed_lp(6000, 10000, 4, 3): the certificate is one CSR pass and one CSC pass over the same matrix plus a BTRAN; a round is the
    same two passes plus two bound vectors.  Medians of 5 after a warm-up; MLP_WRITE_PROFILES=1 records them in profiles/propagate.json."""
    import json
    lp = lpgen.gen_mixed_lp(6000, 10000, 4, 3)
    s = _solve(lp)
    per_round, cert, rounds, nbytes = [], [], 0, 0.0
    for rep in range(6):
        s.propagate_bounds()
        info = s.propagate_info()
        t = s.clone()                                                                          # (a solution caches its duals: a clone computes them afresh)
        c = t.certificate()
        if rep:
            per_round.append(info["device_ms"] / info["rounds"])
            cert.append(c["device_ms"])
        rounds, nbytes = info["rounds"], info["bytes"]
    a, b = float(np.median(per_round)), float(np.median(cert))
    print("propagation: %.4f ms per round over %d rounds, certificate %.4f ms, %.3g bytes per round (%.1f GB/s)"
          % (a, rounds, b, nbytes / rounds, nbytes / rounds / (a * 1e-3) / 1e9))
    if os.environ.get("MLP_WRITE_PROFILES") == "1":
        with open(os.path.join(ROOT, "profiles", "propagate.json"), "w") as f:
            json.dump(dict(instance="gen_mixed_lp(6000, 10000, 4, 3)", rounds=rounds, ms_per_round=a, certificate_ms=b,
                           bytes_per_round=nbytes / rounds, gb_per_s=nbytes / rounds / (a * 1e-3) / 1e9, hbm_peak_gb_per_s=8000.0,
                           per_round_samples=per_round, certificate_samples=cert), f, indent=1)
            f.write("\n")
    assert a <= 2.0 * b, (a, b)
