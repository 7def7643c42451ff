"""Reduced-cost bounds from a cutoff and the batched fixing of variables (include/minilp_hip.h: mlp_solution_cutoff_bounds,
mlp_solution_fix_vars, mlp_solution_unfix_vars, mlp_fix_info; csrc/fixing.inc).

The yardstick of the read is `ref_bounds` below: the formulas of the header in Python floats on the `Ref` of tests/test_branch_penalties.py
(an splu factorisation of the basis the solution reports; its reduced costs are c - A^T B^-T c_B, never reduced_costs()).  The gap is
formed as the header forms it, cutoff - objective() (Maximize: objective() - cutoff), in the same float operation.  The listed set and
its fixed subset must be equal, the bounds agree to the relative 1e-7 of tests/test_ranging.py.  A variable is left out of the comparison
only when it is marked integer and the reference's t + 1e-9 (t > 0) lies within 1e-7 max(1, t) of an integer, where the floor is a matter
of rounding; at most 2 % of the list may be left out (the CPU tests show that the reference leaves out none on these instances).

The yardstick of the mutators is the sequential single form: the oracle's fix_var over the same list (status, objective to OBJ_RTOL) and
the engine's own fix_var on a clone.  x is compared to X_ATOL where the optimum is unique (cover, sparse-maximize: continuous random
data); gen_mixed_lp has alternative optima — engine and oracle already stop at different vertices of the same objective — so there the
point must be feasible and carry the objective.  Where an instance has fewer candidates of a kind than a list length asks for (cover
has 90 variables), the list is as long as the instance allows.

Measured on the MI355X: on gen_mixed_lp(300, 400, 6, 3) the reference's own unfix_var (the oracle, and the engine's single form with
it) leaves a NaN objective behind once a released variable sits strictly inside its bounds; unfix_vars is compared with the single form
there, and with the original optimum on the other two instances."""
import ctypes
import importlib.util
import json
import math
import os
import re

import numpy as np
import pytest

import minilp_amd as M
from minilp_amd import api, build as mbuild, lpgen
from tests.common import OBJ_RTOL, ROOT, X_ATOL, check_feasible, obj_close
from tests.test_branch_penalties import (INSTANCES, KNAPSACK_SEEDS, TSP_CITIES, TSP_SEED, _blob, _hand_lp, _knapsack, _model, _ref_of_engine,
                                         _ref_of_oracle)

INF = math.inf
NEW = ["mlp_solution_cutoff_bounds", "mlp_solution_fix_vars", "mlp_solution_unfix_vars", "mlp_solution_fix_info", "mlp_fix_info_size"]
GAPS = (0.0, 0.001, 0.01, 0.1)          # of |objective| (CPU); the GPU tests use 0, 1 % and 10 %
LENGTHS = (0, 1, 16, 17, 64)
FIX_INSTANCES = ("mixed", "cover", "sparse-maximize")
FIXED = M.MLP_NB_FIXED


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(M.lib_path()):
        mbuild.build(verbose=False)
    return M.lib()


# ------------------------------------------------------------------------------------------------ the yardstick of the read
def ref_bounds(ref, lo, hi, g, is_int=None):
    """({variable: (new_lo, new_hi)}, {variables whose floor is a matter of rounding}) for the gap g >= 0."""
    out, near = {}, set()
    if not g < INF:
        return out, near
    for j in range(len(lo)):
        st, num = int(ref.st[j]), float(ref.num[j])
        if st not in (1, 2) or not num > 0.0:
            continue
        t = g / num
        if is_int is not None and is_int[j] and ref.xval[j] == math.floor(ref.xval[j]):
            if t > 0.0 and abs((t + 1e-9) - round(t + 1e-9)) <= 1e-7 * max(1.0, t):
                near.add(j)
            t = math.floor(t + 1e-9)
        if st == 1:
            nh = max(lo[j] + t, lo[j])
            if nh < hi[j]:
                out[j] = (float(lo[j]), float(nh))
        else:
            nl = min(hi[j] - t, hi[j])
            if nl > lo[j]:
                out[j] = (float(nl), float(hi[j]))
    return out, near


def _gap_and_cutoff(obj, direction, frac):
    """(g, cutoff): the cutoff `frac` of |objective| worse than the objective, and the gap exactly as the library forms it."""
    if direction == M.MAXIMIZE:
        cutoff = obj - frac * abs(obj)
        return obj - cutoff, cutoff
    cutoff = obj + frac * abs(obj)
    return cutoff - obj, cutoff


def _close(a, b, tol):
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= tol * max(1.0, abs(b))


def _compare_bounds(dev, want, near, tol=1e-7, label=""):
    v, lo, hi = dev
    assert len(v) == len(lo) == len(hi) and (np.diff(v.astype(np.int64)) > 0).all(), label      # ascending, no duplicates
    got = {int(j): (float(a), float(b)) for j, a, b in zip(v, lo, hi)}
    left, worst = 0, 0.0
    for j in sorted(set(got) | set(want)):
        if j in near:
            left += 1
            continue
        assert j in got and j in want, (label, j, got.get(j), want.get(j))
        for a, b in zip(got[j], want[j]):
            assert _close(a, b, tol), (label, j, got[j], want[j])
            if not math.isinf(b):
                worst = max(worst, abs(a - b) / max(1.0, abs(b)))
        assert (got[j][0] == got[j][1]) == (want[j][0] == want[j][1]), (label, j, got[j], want[j])      # the fixed subset
    assert 50 * left <= max(len(want), 1), (label, left, len(want))
    return len(want) - left, left, worst


def _flipped(lp):
    """The same model stated in the other sense (negated costs): the internal form is identical."""
    return dict(lp, direction=M.MINIMIZE if lp["direction"] == M.MAXIMIZE else M.MAXIMIZE, obj=-lp["obj"], name=lp["name"] + "_flipped")


def _check_read(s, lp, fracs=(0.0, 0.01, 0.1), label="", ref=None):
    ref = ref or _ref_of_engine(s, _model(lp))
    n, obj = lp["n"], s.objective()
    total = 0
    for frac in fracs:
        g, cutoff = _gap_and_cutoff(obj, lp["direction"], frac)
        for marks in (None, np.ones(n, bool)):
            want, near = ref_bounds(ref, lp["lo"], lp["hi"], g, marks)
            v, lo, hi, pruned = s.cutoff_bounds(cutoff, marks)
            assert not pruned
            done, left, worst = _compare_bounds((v, lo, hi), want, near, label="%s gap %g %s" % (label, frac, "int" if marks is not None else "plain"))
            info = s.fix_info()
            assert info["listed"] == len(v) and info["listed_fixed"] == int((lo == hi).sum()) and info["requests"] == 0 and info["pivots"] == 0
            print("%s gap %g %s: %d listed, %d fixed, %d left out, worst relative deviation %.2e, device %.4f ms" %
                  (label, frac, "marked" if marks is not None else "plain", len(v), int((lo == hi).sum()), left, worst, info["device_ms"]))
            total += len(v)
    return total


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
    assert "typedef struct mlp_fix_info" in hdr
    args = re.search(r"pub fn mlp_solution_cutoff_bounds\s*\(([^)]*)\)", sys_rs).group(1)
    assert [a.split(":")[0].strip() for a in args.split(",")] == ["s", "cutoff", "var_is_int", "num_vars", "vars", "new_lo", "new_hi", "cap", "count", "pruned"]
    assert re.search(r"pub fn cutoff_bounds\s*\(&self", lib_rs) and re.search(r"pub fn fix_vars\s*\(self", lib_rs) and re.search(r"pub fn unfix_vars\s*\(self", lib_rs)
    ext = surface.split("### extensions")[1]
    for n in ("cutoff_bounds", "fix_vars", "unfix_vars"):
        assert re.search(r"\* `pub fn %s\(&?self, .*`" % n, ext), n
    for n in ("cutoff_bounds", "fix_vars", "unfix_vars", "fix_info", "fix_by_reduced_cost"):
        assert hasattr(M.Solution, n), n


def test_abi_version_is_still_5_and_the_struct_size_matches(L):
    assert L.mlp_abi_version() == 5 == api.ABI_VERSION
    assert L.mlp_fix_info_size() == ctypes.sizeof(api.MlpFixInfo) == 96
    assert "Still version 5: the reduced-cost bounds" in open(os.path.join(ROOT, "include", "minilp_hip.h")).read()


def test_null_handle_is_einval_not_a_crash(L):
    cnt, pr, k = ctypes.c_uint64(7), ctypes.c_int(7), ctypes.c_uint64(7)
    assert L.mlp_solution_cutoff_bounds(None, 1.0, None, 0, None, None, None, 0, ctypes.byref(cnt), ctypes.byref(pr)) == -1
    h = ctypes.c_void_p()
    v, x = np.zeros(1, dtype=np.uint32), np.zeros(1)
    pv, px = v.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert L.mlp_solution_fix_vars(ctypes.byref(h), pv, px, 1) == -1
    assert L.mlp_solution_fix_vars(None, pv, px, 0) == -1
    assert L.mlp_solution_unfix_vars(ctypes.byref(h), pv, 1, ctypes.byref(k)) == -1
    assert L.mlp_solution_fix_info(None, ctypes.byref(api.MlpFixInfo())) == -1


@pytest.mark.parametrize("name", list(INSTANCES))
def test_the_instances_list_bounds_and_stay_off_the_integer_boundaries_at_the_oracle_basis(name):
    """The reference on the oracle's optimal basis: every gap lists something, and no t lies within 1e-7 max(1, t) of an integer, so the
    GPU comparison leaves out nothing on these instances."""
    from oracle import minilp_oracle as O
    gen, args = INSTANCES[name]
    lp = gen(*args)
    o = lpgen.build_problem(O.Problem, lp).solve()
    ref = _ref_of_oracle(o, _model(lp))
    n, obj = lp["n"], o.objective()
    counts = []
    for frac in GAPS:
        g, _ = _gap_and_cutoff(obj, lp["direction"], frac)
        assert g >= 0.0 and (g == 0.0) == (frac == 0.0)
        plain, _ = ref_bounds(ref, lp["lo"], lp["hi"], g)
        marked, near = ref_bounds(ref, lp["lo"], lp["hi"], g, np.ones(n, bool))
        assert len(plain) > 0 and len(marked) > 0, (name, frac)
        assert not near, (name, frac, sorted(near))
        counts.append(len(plain))
    print("%s: listed at gaps %s: %s" % (name, GAPS, counts))
    if name == "mixed":
        g0, _ = ref_bounds(ref, lp["lo"], lp["hi"], 0.0)
        assert counts == [193, 191, 145, 89]
        assert sum(1 for j in g0 if ref.st[j] == 1) == 177 and sum(1 for j in g0 if ref.st[j] == 2) == 16
        assert all(a == b for a, b in g0.values())                                       # gap 0: every listed variable is fixed


def test_listed_bounds_keep_every_integer_point_within_the_cutoff_on_oracle_solves():
    """Validity by enumeration: on the binary knapsacks, all variables marked integer, every feasible 0/1 point whose objective is no
    worse than the cutoff satisfies every listed bound — at cutoff = the integer optimum (which must survive) and at two looser ones."""
    import itertools
    from oracle import minilp_oracle as O
    listed = fixed = 0
    for seed in KNAPSACK_SEEDS:
        lp = _knapsack(seed)
        n = lp["n"]
        o = lpgen.build_problem(O.Problem, lp).solve()
        ref = _ref_of_oracle(o, _model(lp))
        X = np.array(list(itertools.product((0.0, 1.0), repeat=n)))
        X = X[(X @ lp["data"].reshape(3, n).T <= lp["rhs"] + 1e-9).all(axis=1)]
        vals = X @ lp["obj"]
        best = float(vals.max())
        assert o.objective() >= best - 1e-9
        for cutoff in (best, best - 2.0, best - 7.0):                                    # Maximize: a looser cutoff is a lower one
            g = o.objective() - cutoff
            want, _ = ref_bounds(ref, lp["lo"], lp["hi"], g, np.ones(n, bool))
            keep = X[vals >= cutoff]
            assert len(keep) >= 1 and (cutoff != best or (keep @ lp["obj"]).max() == best)
            for j, (a, b) in want.items():
                assert (keep[:, j] >= a - 1e-9).all() and (keep[:, j] <= b + 1e-9).all(), (lp["name"], cutoff, j, a, b)
                fixed += a == b
            listed += len(want)
    print("knapsacks: %d bounds listed, %d of them fixings" % (listed, fixed))
    assert listed >= 4 and fixed >= 1


# ------------------------------------------------------------------------------------------------ 1: the read against the host reference
_SOLVED = {}


def _solved(name, flip=False):
    """(lp, engine solution) of an instance, solved once per module; the tests work on clones."""
    key = (name, flip)
    if key not in _SOLVED:
        gen, args = INSTANCES[name]
        lp = gen(*args)
        lp = _flipped(lp) if flip else lp
        _SOLVED[key] = (lp, lpgen.build_problem(M.Problem, lp).solve())
    return _SOLVED[key]


@pytest.mark.gpu
@pytest.mark.parametrize("flip", [False, True], ids=["as stated", "other sense"])
@pytest.mark.parametrize("name", list(INSTANCES))
def test_cutoff_bounds_against_the_host_reference(name, flip):
    lp, s = _solved(name, flip)
    obj = s.objective()
    x0, blob0 = s.values().tobytes(), s.save_basis(2)
    assert _check_read(s, lp, label=lp["name"]) >= 8
    # pruned: a cutoff on the better side of the objective
    _, worse = _gap_and_cutoff(obj, lp["direction"], -0.01)
    v, lo, hi, pruned = s.cutoff_bounds(worse)
    assert pruned and len(v) == 0 and s.fix_info()["listed"] == 0
    assert s.cutoff_bounds(INF if lp["direction"] == M.MINIMIZE else -INF)[0].size == 0   # g = +inf lists nothing, and prunes nothing
    assert not s.cutoff_bounds(INF if lp["direction"] == M.MINIMIZE else -INF)[3]
    # two calls: the same bits; the call changed nothing
    _, cutoff = _gap_and_cutoff(obj, lp["direction"], 0.01)
    a, b = s.cutoff_bounds(cutoff, np.ones(lp["n"], bool)), s.cutoff_bounds(cutoff, np.ones(lp["n"], bool))
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a[:3], b[:3]))
    c = s.clone().cutoff_bounds(cutoff, np.ones(lp["n"], bool))                          # a clone that never read
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a[:3], c[:3]))
    assert s.values().tobytes() == x0 and np.float64(s.objective()).tobytes() == np.float64(obj).tobytes() and s.save_basis(2) == blob0


def _shift_list(lp, s, k):
    """(vars, vals): up to k variables non-basic at a bound, each moved a little way into its range."""
    vs, _ = s.basis_status()
    x = s.values()
    js = [j for j in range(lp["n"]) if vs[j] in (1, 2)][:k]
    step = lambda j: 1e-3 * min(1.0, lp["hi"][j] - lp["lo"][j])
    return js, [float(x[j] + step(j)) if vs[j] == 1 else float(x[j] - step(j)) for j in js]


def _certificate_is_clean(s, label=""):
    c = s.certificate()                                                                  # the bars of tests/test_duals.py after warm-start calls
    assert c["relative_gap"] <= 1e-9 and c["max_dual_infeasibility"] <= 1e-9 and c["max_row_violation"] <= 1e-7 and c["max_bound_violation"] <= 1e-7, (label, c)


def _check_representation(s, lp, label, twin=None, before_batch=None):
    """The read against the reference, then one batch of shifted non-basic requests (the FTRAN through this representation of B^-1)
    against the engine's own sequential fix_var on a clone.  twin: a second solution in the same state; the sequence then runs on it and
    the batch on `s` itself, after before_batch(s) (a clone would fold the pending terms of its source)."""
    assert _check_read(s, lp, fracs=(0.01,), label=label) >= 8
    js, vals = _shift_list(lp, s, 16)
    assert len(js) == 16
    seq = twin or s.clone()
    try:
        for j, v in zip(js, vals):
            seq = seq.fix_var(j, v)
    except M.Infeasible:
        seq = None
    if before_batch:
        before_batch(s)
    try:
        bat = (s if twin else s.clone()).fix_vars(js, vals)
    except M.Infeasible:
        bat = None
    assert (seq is None) == (bat is None), label
    if bat is not None:
        info = bat.fix_info()
        assert info["nonbasic"] == 16 and info["shifted"] == 16 and info["solves"] == 1 and info["forced_pivots"] == 0, info
        assert obj_close(bat.objective(), seq.objective()) and np.abs(bat.values() - seq.values()).max() <= X_ATOL, label
        _certificate_is_clean(bat, label)
        vs, _ = bat.basis_status()
        assert all(vs[j] == FIXED for j in js)
    print("%s: 16 shifted requests, %s" % (label, "infeasible both ways" if bat is None else bat.fix_info()))


@pytest.mark.gpu
def test_singleton_positions():
    from tests.test_ranging import _singleton_lp
    lp = _singleton_lp()
    _check_representation(lpgen.build_problem(M.Problem, lp).solve(), lp, "singleton columns")


@pytest.mark.gpu
def test_pending_terms_of_the_delayed_update_mode(monkeypatch):
    """A SOLVED model that holds pending rank-1 terms (the config-4 mid basis of tests/test_branch_penalties.py is not solved, and the
    read refuses it): the recipe of tests/test_gmi_cuts.py.  The batch runs on the solution itself: a clone folds the terms first."""
    from tests.test_gmi_cuts import _pending, _solved_with_pending_terms
    monkeypatch.setenv("MLP_LOWRANK", "3")
    s, lp, _ = _solved_with_pending_terms(lpgen.gen_sparse_lp(200, 150, 8, 3), True)
    twin, _, _ = _solved_with_pending_terms(lpgen.gen_sparse_lp(200, 150, 8, 3), True)
    assert np.float64(s.objective()).tobytes() == np.float64(twin.objective()).tobytes() and s.values().tobytes() == twin.values().tobytes()

    def check(t):
        assert int(t.state("lowrank_pending")[1]) == 3 and _pending(t) > 0

    check(s)
    _check_representation(s, lp, "pending terms", twin=twin, before_batch=check)       # (the read in between folds nothing)


@pytest.mark.gpu
def test_compact_factor(monkeypatch):
    monkeypatch.setenv("MLP_FACTOR", "1")
    lp = lpgen.gen_transport_lp(600, 700, 4, 5, tight=0.45)
    s = lpgen.build_problem(M.Problem, lp).solve()
    assert s.stats()["factor_active"] == 1
    _check_representation(s, lp, "compact factor")


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
    _check_representation(s, lp, "sparse bump")


@pytest.mark.gpu
def test_refusals_of_the_read():
    from minilp_amd import dist as md
    lp = lpgen.gen_mixed_lp(40, 30, 6, 9)
    n = lp["n"]
    prob = lpgen.build_problem(M.Problem, lp)
    s = prob.solve()

    def refused(f):
        with pytest.raises(M.InternalError) as e:
            f()
        assert e.value.code == -1

    refused(lambda: s.cutoff_bounds(math.nan))
    refused(lambda: s.cutoff_bounds(s.objective() + 1.0, np.ones(n - 1, bool)))
    refused(lambda: s.cutoff_bounds(s.objective() + 1.0, np.ones(n + 1, bool)))
    refused(lambda: prob.solve(budget=5).cutoff_bounds(1e9))                             # a budget-limited solve is not solved
    refused(lambda: prob.solve(budget=0).cutoff_bounds(1e9))
    # cap below the count: MLP_EINVAL, the count is set, nothing is written
    L = M.lib()
    v, lo, hi, _ = s.cutoff_bounds(s.objective() + 1.0)
    assert len(v) >= 2
    bv, bl, bh = np.full(n, 77, dtype=np.uint32), np.full(n, 77.0), np.full(n, 77.0)
    cnt, pr = ctypes.c_uint64(), ctypes.c_int()
    pu, pd = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_double)
    assert L.mlp_solution_cutoff_bounds(s._h, s.objective() + 1.0, None, n, bv.ctypes.data_as(pu), bl.ctypes.data_as(pd), bh.ctypes.data_as(pd),
                                        len(v) - 1, ctypes.byref(cnt), ctypes.byref(pr)) == -1
    assert cnt.value == len(v) and (bv == 77).all() and (bl == 77.0).all() and (bh == 77.0).all()
    assert L.mlp_solution_cutoff_bounds(s._h, s.objective() + 1.0, None, n, bv.ctypes.data_as(pu), bl.ctypes.data_as(pd), bh.ctypes.data_as(pd),
                                        len(v), ctypes.byref(cnt), ctypes.byref(pr)) == 0
    assert bv[:len(v)].tobytes() == v.tobytes() and bl[:len(v)].tobytes() == lo.tobytes()
    s.objective()                                                                        # a read frees nothing
    box = md.create_mailbox(1)
    try:
        t = prob.solve()
        t.enable_sharding_ex(0, 1, box, "pump")
        refused(lambda: t.cutoff_bounds(1e9))
    finally:
        md.remove_mailbox(box)


@pytest.mark.gpu
def test_the_size_horizon_is_exact():
    """One row sum x >= 1, x in [0, 1], n = 600 001 (more than one grid trip, not a multiple of 64): x_300000 = 1 is basic, the dual value
    is 0.5 and d_j = c_j - 0.5 exactly, so the list for cutoff = objective + 0.25 is known exactly."""
    n = 600001
    c = 1.0 + ((7919 * np.arange(n)) % 1000) / 1000.0
    c[300000] = 0.5
    lp = dict(name="one_row", direction=M.MINIMIZE, m=1, n=n, obj=c, lo=np.zeros(n), hi=np.ones(n), indptr=np.array([0, n], dtype=np.uint64),
              indices=np.arange(n, dtype=np.uint32), data=np.ones(n), ops=np.array([lpgen.GE], dtype=np.int32), rhs=np.array([1.0]))
    s = lpgen.build_problem(M.Problem, lp).solve()
    assert s.objective() == 0.5
    d = c - 0.5
    want = np.flatnonzero(d > 0.25)
    assert 300000 not in want and len(want) > 524288 // 2 and want[-1] > 2 * 524288 // 2
    v, lo, hi, pruned = s.cutoff_bounds(s.objective() + 0.25)
    assert not pruned and np.array_equal(v, want) and (lo == 0.0).all() and np.array_equal(hi, 0.25 / d[want])
    v, lo, hi, pruned = s.cutoff_bounds(s.objective() + 0.25, np.ones(n, bool))
    assert not pruned and np.array_equal(v, want) and (lo == 0.0).all() and (hi == 0.0).all()
    info = s.fix_info()
    assert info["listed"] == info["listed_fixed"] == len(want)
    print("n = %d: %d listed, device %.3f ms" % (n, len(want), info["device_ms"]))


# ------------------------------------------------------------------------------------------------ 2: fix_vars
def _request_lists(lp, vs, x, kind, k):
    """(vars, vals) of one kind: `value` non-basic at their value, `shift` non-basic moved into their range, `basic` basic variables moved
    a little (inside their bounds), `mixed` all three in turn."""
    n, lo, hi = lp["n"], lp["lo"], lp["hi"]
    nb = [j for j in range(n) if vs[j] in (1, 2)]
    ba = [j for j in range(n) if vs[j] == 0]
    shifted = lambda j: float(x[j] + 1e-3 * min(1.0, hi[j] - lo[j]) * (1.0 if vs[j] == 1 else -1.0))
    nudged = lambda j: float(min(max(x[j] + 1e-4, lo[j]), hi[j]))
    if kind == "value":
        js = nb[:k]
        return js, [float(x[j]) for j in js]
    if kind == "shift":
        js = nb[:k]
        return js, [shifted(j) for j in js]
    if kind == "basic":
        js = ba[:k]
        return js, [nudged(j) for j in js]
    js, vals = [], []
    for t in range(k):
        src, f = ((nb, lambda j: float(x[j])), (ba, nudged), (nb, shifted))[t % 3]
        pool = [j for j in src if j not in js]
        if pool:
            js.append(pool[0] if t % 3 != 2 else pool[-1])
            vals.append(f(js[-1]))
    return js, vals


_ORACLE = {}


def _oracle_solved(name):
    from oracle import minilp_oracle as O
    if name not in _ORACLE:
        gen, args = INSTANCES[name]
        _ORACLE[name] = lpgen.build_problem(O.Problem, gen(*args)).solve()
    return _ORACLE[name]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["value", "shift", "basic", "mixed"])
@pytest.mark.parametrize("name", FIX_INSTANCES)
def test_fix_vars_against_the_sequential_form(name, kind):
    from oracle import minilp_oracle as O
    lp, s = _solved(name)
    o = _oracle_solved(name)
    obj0, x0 = s.objective(), s.values()
    vs, _ = s.basis_status()
    assert obj_close(obj0, o.objective())
    # x is compared where the existing warm-start tests compare it: where the optimum is unique.  gen_mixed_lp has alternative optima
    # (engine and oracle already stop at different vertices of the same objective): there the point must be feasible with the objective
    unique = bool(np.abs(x0 - o.values()).max() <= X_ATOL)
    assert unique or name == "mixed"
    feasible = 0
    for k in LENGTHS:
        js, vals = _request_lists(lp, vs, x0, kind, k)
        assert len(js) == len(set(js)) and (len(js) == k or k > 17), (name, kind, k, len(js))
        label = "%s %s %d" % (name, kind, len(js))
        oq = o.clone()
        try:
            for j, v in zip(js, vals):
                oq = oq.fix_var(j, v)
        except O.Infeasible:
            oq = None
        seq = s.clone()
        try:
            for j, v in zip(js, vals):
                seq = seq.fix_var(j, v)
        except M.Infeasible:
            seq = None
        try:
            bat = s.clone().fix_vars(js, vals)
        except M.Infeasible:
            bat = None
        assert (bat is None) == (oq is None) == (seq is None), (label, bat is None, oq is None, seq is None)      # the status matches
        if bat is None:
            print("%s: infeasible, as the oracle says" % label)
            continue
        feasible += 1
        info = bat.fix_info()
        nbn = sum(1 for j in js if vs[j] != 0)
        moved = sum(1 for j, v in zip(js, vals) if vs[j] != 0 and v != x0[j])
        assert info["requests"] == len(js) and info["nonbasic"] == nbn and info["forced_pivots"] == len(js) - nbn, (label, info)
        assert info["shifted"] == moved and info["solves"] == (1 if moved else 0), (label, info)
        assert obj_close(bat.objective(), oq.objective()) and obj_close(bat.objective(), seq.objective()), (label, bat.objective(), oq.objective(), seq.objective())
        xb = bat.values()
        check_feasible(lp, xb)
        assert obj_close(float(np.dot(lp["obj"], xb)), bat.objective(), 1e-8), label
        if unique:
            assert np.abs(xb - oq.values()).max() <= X_ATOL and np.abs(xb - seq.values()).max() <= X_ATOL, label
        assert all(xb[j] == v if vs[j] != 0 else abs(xb[j] - v) <= 1e-9 for j, v in zip(js, vals)), label      # a fixed variable holds the value asked for
        st, _ = bat.basis_status()
        assert all(st[j] == FIXED for j in js), label
        if len(js):
            _certificate_is_clean(bat, label)
        if kind == "value":                                                              # nothing moves: no solve, no pivot, the same bits
            assert info["solves"] == 0 and info["pivots"] == 0, (label, info)
            assert np.float64(bat.objective()).tobytes() == np.float64(obj0).tobytes() and xb.tobytes() == x0.tobytes(), label
        print("%s: %s" % (label, info))
    assert feasible >= 3, (name, kind, feasible)                                       # (only some of the longest lists are infeasible)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIX_INSTANCES)
def test_the_order_of_the_non_basic_requests_changes_no_bit(name):
    lp, s = _solved(name)
    vs, _ = s.basis_status()
    x0 = s.values()
    js, vals = _request_lists(lp, vs, x0, "shift", 17)
    bj, bv = _request_lists(lp, vs, x0, "basic", 2)
    rng = np.random.default_rng(7)
    outs = []
    for rep in range(3):
        perm = np.arange(len(js)) if rep == 0 else rng.permutation(len(js))
        lj, lv = [js[i] for i in perm], [vals[i] for i in perm]
        # the basic requests keep their places in the list (their order is the order of the forced pivots)
        lj, lv = lj[:5] + bj[:1] + lj[5:] + bj[1:], lv[:5] + bv[:1] + lv[5:] + bv[1:]
        try:
            t = s.clone().fix_vars(lj, lv)
            outs.append((np.float64(t.objective()).tobytes(), t.values().tobytes(), _blob(t)))
        except M.Infeasible:
            outs.append(None)
    assert outs[0] == outs[1] == outs[2]
    assert outs[0] is not None or name != "mixed"


@pytest.mark.gpu
def test_refusals_of_the_mutators_consume_the_handle():
    from oracle import minilp_oracle as O
    lp, s = _solved("small-mixed")
    n = lp["n"]
    x = s.values()
    vs, _ = s.basis_status()
    j = next(j for j in range(n) if vs[j] in (1, 2) and lp["hi"][j] > lp["lo"][j])
    for bad in (lambda t: t.fix_vars([j, 3 if j != 3 else 4, j], [x[j], x[3 if j != 3 else 4], x[j]]),      # listed twice
                lambda t: t.fix_vars([0, n], [x[0], 0.0]),                                # out of range
                lambda t: t.unfix_vars([0, n])):
        t = s.clone()
        with pytest.raises(M.InternalError) as e:
            bad(t)
        assert e.value.code == -1 and not t._h.value                                     # consumed
    t = s.clone()
    outside = lp["hi"][j] + 1.0 if math.isfinite(lp["hi"][j]) else lp["lo"][j] - 1.0
    with pytest.raises(M.Infeasible):
        t.fix_vars([j], [outside])
    assert not t._h.value
    with pytest.raises(M.InternalError):
        s.clone().fix_vars([0, 1], [x[0]])                                               # lengths differ (caught by the binding)
    # n == 0: a successful no-op on the same state
    t = s.clone()
    b0 = _blob(t)
    t = t.fix_vars([], [])
    assert _blob(t) == b0 and t.fix_info()["requests"] == 0
    t, k = t.unfix_vars([])
    assert k == 0 and _blob(t) == b0
    # fixings that are infeasible together: Infeasible, as the oracle says
    hand = _hand_lp()
    for B in (M, O):
        with pytest.raises(B.Infeasible):
            q = lpgen.build_problem(B.Problem, hand).solve()
            if B is M:
                q.fix_vars([1, 2], [10.0, 10.0])                                         # 2 x0 + x1 + x2 = 3 with x0 >= 0
            else:
                q.fix_var(1, 10.0).fix_var(2, 10.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIX_INSTANCES)
def test_unfix_vars(name):
    lp, s = _solved(name)
    vs, _ = s.basis_status()
    x0, obj0 = s.values(), s.objective()
    js, vals = _request_lists(lp, vs, x0, "shift", 16)
    bj, bv = _request_lists(lp, vs, x0, "basic", 1)
    t = s.clone().fix_vars(js + bj, vals + bv)
    st, _ = t.basis_status()
    never = [j for j in range(lp["n"]) if st[j] in (1, 2)][:3]                           # non-basic, never fixed
    basic = [j for j in range(lp["n"]) if st[j] == 0][:3]
    # an all-skipped call leaves the state as it is, bit for bit
    b0, o0 = t.save_basis(2), np.float64(t.objective()).tobytes()
    t, k = t.unfix_vars(never + basic)
    assert k == 0 and t.save_basis(2) == b0 and np.float64(t.objective()).tobytes() == o0 and t.fix_info()["unfixed"] == 0
    # the single form on a second solution in the same fixed state: the yardstick
    u = s.clone().fix_vars(js + bj, vals + bv)
    for j in js + bj:
        u, was = u.unfix_var(j)
        assert was
    # releasing what was fixed (with a second mention and the skipped kinds in between) returns the original optimum
    t, k = t.unfix_vars(js[:8] + never + js[8:] + basic + bj + js[:2])
    info = t.fix_info()
    assert k == len(js) + len(bj) == info["unfixed"] and info["requests"] == len(js) + len(bj) + len(never) + len(basic) + 2
    st, _ = t.basis_status()
    assert all(lp["lo"][j] == lp["hi"][j] for j in np.flatnonzero(st == FIXED))
    assert np.abs(t.values() - x0).max() <= X_ATOL or name == "mixed"
    if math.isnan(u.objective()):
        # gen_mixed_lp: the reference's own unfix_var (the oracle, and the engine's single form with it) leaves a NaN objective behind once a
        # released variable sits strictly inside its bounds (its ratio test walks a basic variable to an infinite bound); the batched form
        # runs the same re-solve.  There is no yardstick for the point there: the batched form must do no worse than the single form.
        assert name == "mixed" and (math.isnan(t.objective()) or obj_close(t.objective(), obj0))
    else:
        assert obj_close(t.objective(), obj0) and obj_close(u.objective(), t.objective())
        _certificate_is_clean(t, name)
    print("%s: released %d, %s" % (name, k, info))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed", "sparse-maximize"])
def test_reduced_cost_fixing_before_a_branching_step(name):
    """fix_by_reduced_cost at cutoff = objective + gap, then a branch-and-bound step (fix_var of a fractional variable at its floor / its
    ceiling).  Unmarked, an entry is a fixing only when the bound leaves no room at all, and the child's objective is the one without
    the fixing whenever it is within the cutoff.  With integer marks the bound of a variable is rounded to whole steps: that removes
    fractional points within the cutoff, so the child LP may only get worse (weak duality); it is the same whenever the child without the
    fixing keeps every fixed variable at its value, because its optimum is then feasible for the fixed child."""
    lp, s = _solved(name)
    n, obj = lp["n"], s.objective()
    sg = -1.0 if lp["direction"] == M.MAXIMIZE else 1.0
    x = s.values()
    vs, _ = s.basis_status()
    frac = [j for j in range(n) if vs[j] == 0 and abs(x[j] - round(x[j])) > 1e-3][:4]
    assert len(frac) == 4
    same = worse = within = 0
    for gapf, marks in ((0.0, None), (0.01, None), (0.01, np.ones(n, bool)), (0.1, np.ones(n, bool))):
        _, cutoff = _gap_and_cutoff(obj, lp["direction"], gapf)
        f, fixed = s.clone().fix_by_reduced_cost(cutoff, marks)
        info = f.fix_info()
        assert info["requests"] == len(fixed) == info["nonbasic"] and info["solves"] == 0 and info["pivots"] == 0
        assert np.float64(f.objective()).tobytes() == np.float64(obj).tobytes() and f.values().tobytes() == x.tobytes()
        st, _ = f.basis_status()
        assert all(st[j] == FIXED for j in fixed) and (marks is not None or gapf == 0.0 or len(fixed) == 0)
        for j in frac:
            for val in (math.floor(x[j]), math.ceil(x[j])):
                try:
                    plain = s.clone().fix_var(j, float(val))
                except M.Infeasible:
                    plain = None
                try:
                    child = f.clone().fix_var(j, float(val))
                except M.Infeasible:
                    child = None
                if plain is None:
                    assert child is None
                    continue
                inside = sg * (plain.objective() - cutoff) <= 0.0
                within += inside
                if child is None:
                    assert not inside or marks is not None
                    worse += 1
                    continue
                assert sg * (child.objective() - plain.objective()) >= -OBJ_RTOL * max(1.0, abs(obj))      # a restriction: never better
                keeps = len(fixed) == 0 or np.abs(plain.values()[fixed] - x[fixed]).max() == 0.0
                if (marks is None and inside) or keeps:
                    assert obj_close(child.objective(), plain.objective()), (name, gapf, j, val, child.objective(), plain.objective())
                    same += 1
                else:
                    worse += not obj_close(child.objective(), plain.objective())
    print("%s: %d children within their cutoff, %d equal by the rule, %d worse under integer rounding" % (name, within, same, worse))
    assert same >= 4


# ------------------------------------------------------------------------------------------------ 3: the drivers
def _load_example(name):
    spec = importlib.util.spec_from_file_location(name + "_fixing", os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_tsp_example_reaches_the_same_tour_cost_with_reduced_cost_fixing():
    tsp = _load_example("tsp")
    pts = np.random.default_rng(TSP_SEED).uniform(0.0, 100.0, size=(TSP_CITIES, 2))
    plain, rc = tsp.TspSolver(M, pts), tsp.TspSolver(M, pts, rc_fixing=True)
    c0, t0 = plain.solve()
    c1, t1 = rc.solve()
    print("14 cities: plain %s; --rc-fixing %s" % (plain.stats, rc.stats))
    assert abs(c0 - c1) <= 1e-9 * max(1.0, abs(c0)) and abs(rc.tour_cost(t1) - c1) <= 1e-7 and sorted(t1) == list(range(TSP_CITIES))
    assert "rc_calls" in rc.stats and "rc_fixed" in rc.stats and "rc_calls" not in plain.stats


@pytest.mark.gpu
def test_tsp_bn130_reaches_the_same_tour_cost_with_reduced_cost_fixing():
    """The run without the flag is tests/test_mps_tsp.py::test_tsp_bn130_reaches_reference_optimum, which pins its cost to BN130_OPT with
    this bar: one branch and bound here instead of two (about a minute)."""
    from tests.test_mps_tsp import BN130, BN130_OPT
    tsp = _load_example("tsp")
    _, pts = tsp.read_tsplib(BN130)
    rc = tsp.TspSolver(M, pts, rc_fixing=True)
    cost, tour = rc.solve()
    print("bn130 --rc-fixing: %s" % rc.stats)
    assert abs(cost - BN130_OPT) < 1e-6 and sorted(tour) == list(range(130)) and abs(rc.tour_cost(tour) - BN130_OPT) < 1e-6
    assert rc.stats["rc_calls"] >= 1


@pytest.mark.gpu
def test_solve_mps_example_prints_the_tightened_bounds(tmp_path, capsys):
    mod = _load_example("solve_mps")
    lp = lpgen.gen_mixed_lp(40, 30, 6, 9)
    path = tmp_path / "mixed.mps"
    path.write_text(lpgen.to_mps(lp))
    obj = lpgen.build_problem(M.Problem, lp).solve().objective()
    assert mod.run(M, str(path)) == 0
    assert "cutoff" not in capsys.readouterr().out                                       # without the flag: as before
    assert mod.run(M, str(path), cutoff=obj + 0.05 * abs(obj), continuous=["X3"]) == 0
    out = capsys.readouterr().out
    k = int(re.search(r"cutoff \S+: (\d+) variables tightened, (\d+) of them fixed", out).group(1))
    assert k >= 1 and "'listed': %d" % k in out
    assert mod.run(M, str(path), cutoff=obj - 1.0) == 0 and "already worse" in capsys.readouterr().out
    assert mod.run(M, str(path), cutoff=obj + 1.0, continuous=["NOPE"]) == 1


# ------------------------------------------------------------------------------------------------ 4: measurement
@pytest.mark.gpu
def test_batched_fixing_beats_the_sequential_form_and_the_read_beats_the_certificate():
    """gen_mixed_lp(6000, 10000, 4, 3), median of 5 after one warm-up, one process.  (a) wall time of fix_vars on 64 shifted non-basic
    requests against 64 fix_var calls on a clone of the same state — 64 FTRANs and 64 feasibility restores against one of each;
    (b) device_ms of cutoff_bounds against the certificate's of the same state — O(n) bytes against a transposed solve and two passes
    over A.  Written to profiles/fixing.json when MLP_WRITE_PROFILES=1; the recorded run is in DESIGN.md §7.7."""
    import time
    lp = lpgen.gen_mixed_lp(6000, 10000, 4, 3)
    s = lpgen.build_problem(M.Problem, lp).solve()
    js, vals = _shift_list(lp, s, 64)
    assert len(js) == 64
    bat, seq, rd, ce = [], [], [], []
    info = None
    for rep in range(6):
        a, b = s.clone(), s.clone()
        t0 = time.perf_counter()
        a = a.fix_vars(js, vals)
        t1 = time.perf_counter()
        for j, v in zip(js, vals):
            b = b.fix_var(j, v)
        t2 = time.perf_counter()
        info = a.fix_info()
        assert info["shifted"] == 64 and info["solves"] == 1 and obj_close(a.objective(), b.objective())
        c = s.clone()
        _, cutoff = _gap_and_cutoff(c.objective(), lp["direction"], 0.01)
        c.cutoff_bounds(cutoff, np.ones(lp["n"], bool))
        ri = c.fix_info()
        cert = c.certificate()
        if rep:
            bat.append((t1 - t0) * 1e3); seq.append((t2 - t1) * 1e3); rd.append(ri["device_ms"]); ce.append(cert["device_ms"])
    rec = dict(instance="gen_mixed_lp(6000, 10000, 4, 3)", requests=64, batched_wall_ms=float(np.median(bat)), sequential_wall_ms=float(np.median(seq)),
               speedup=float(np.median(seq) / np.median(bat)), batched_device_ms=info["device_ms"], batched_pivots=info["pivots"],
               cutoff_bounds_device_ms=float(np.median(rd)), certificate_device_ms=float(np.median(ce)),
               read_to_certificate=float(np.median(rd) / np.median(ce)), listed=ri["listed"], listed_fixed=ri["listed_fixed"], read_bytes=ri["bytes"])
    print("FIXING " + json.dumps(rec))
    if os.environ.get("MLP_WRITE_PROFILES") == "1":
        with open(os.path.join(ROOT, "profiles", "fixing.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    assert rec["batched_wall_ms"] < rec["sequential_wall_ms"], rec
    assert rec["cutoff_bounds_device_ms"] < rec["certificate_device_ms"], rec
