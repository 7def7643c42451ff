"""CPU: the yardstick of the bound propagation (tests/propagation_ref.py, the numpy restatement of the rules in include/minilp_hip.h:
mlp_solution_propagate_bounds) on hand-written rows with hand-computed answers and on the committed generators with the counts that
DESIGN.md §7.9 records; the new names in the header, the library, Python and Rust; the ABI."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import minilp_amd as M
from minilp_amd import api, build as mbuild, lpgen
from tests import degenerate_lp as D
from tests.bounded_lp import gen_bounded_lp
from tests.common import ROOT
from tests.propagation_ref import ACCEPT_RTOL, internal_form, propagate

INF = math.inf
NEW = ["mlp_solution_propagate_bounds", "mlp_solution_tighten_by_propagation", "mlp_solution_propagate_info", "mlp_propagate_info_size"]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(M.lib_path()):
        mbuild.build(verbose=False)
    return M.lib()


def hand(lo, hi, rows, direction=lpgen.MINIMIZE):
    """An instance from rows [(indices, coefficients, op, rhs)]; a row may have no terms."""
    n = len(lo)
    indptr = np.concatenate(([0], np.cumsum([len(r[0]) for r in rows]))).astype(np.uint64)
    return dict(name="hand", direction=direction, m=len(rows), n=n, obj=np.ones(n), lo=np.asarray(lo, dtype=np.float64),
                hi=np.asarray(hi, dtype=np.float64), indptr=indptr,
                indices=np.asarray([j for r in rows for j in r[0]], dtype=np.uint32),
                data=np.asarray([a for r in rows for a in r[1]], dtype=np.float64),
                ops=np.asarray([r[2] for r in rows], dtype=np.int32), rhs=np.asarray([r[3] for r in rows], dtype=np.float64))


def chain_lp(k=12):
    """x_i - x_{i+1} >= 0 for i < k, x in [0, 10], x_k >= 1: one more variable tightens per round."""
    lo, hi = np.zeros(k + 1), np.full(k + 1, 10.0)
    lo[k] = 1.0
    return hand(lo, hi, [([i, i + 1], [1.0, -1.0], lpgen.GE, 0.0) for i in range(k)])


def row_vars(lp, r, k):
    """The first k variables of constraint r."""
    b = int(lp["indptr"][r])
    return [int(j) for j in lp["indices"][b:b + k]]


def _run(lp, **kw):
    return propagate(internal_form(lp), lp["n"], **kw)


def _list(r):
    return r["vars"].tolist(), r["lo"].tolist(), r["hi"].tolist()


# ------------------------------------------------------------------------------------------------ hand-computed answers
def test_le_row():
    r = _run(hand([0, 0], [10, 10], [([0, 1], [1.0, 1.0], lpgen.LE, 4.0)]))              # x0 + x1 + s = 4, s >= 0: each x <= 4
    assert _list(r) == ([0, 1], [0.0, 0.0], [4.0, 4.0]) and not r["infeasible"]
    assert r["rounds"] == 2 and r["accepted"] == 3 and r["accepted_struct"] == [2, 0]      # (the slack's upper bound 4 is the third)
    assert r["hi_all"][2] == 4.0


def test_ge_row():
    r = _run(hand([0, 0], [1, 10], [([0, 1], [1.0, 1.0], lpgen.GE, 3.0)]))              # x1 >= 3 - max(x0) = 2; x0 >= 3 - 10: nothing
    assert _list(r) == ([1], [2.0], [10.0])


def test_eq_row_with_a_negative_coefficient():
    r = _run(hand([0, 0], [5, 3], [([0, 1], [2.0, -1.0], lpgen.EQ, 1.0)]))              # 2 x0 = 1 + x1 in [1, 4]
    assert _list(r) == ([0], [0.5], [2.0])


def test_exactly_one_infinite_contribution_tightens_only_that_variable():
    r = _run(hand([1, 2, -INF], [2, 3, 10], [([0, 1, 2], [1.0, 1.0, 1.0], lpgen.LE, 5.0)]))   # x2 <= 5 - 1 - 2
    assert _list(r) == ([2], [-INF], [2.0]) and r["accepted"] == 1


def test_two_infinite_contributions_tighten_nothing():
    r = _run(hand([-INF, -INF], [10, 10], [([0, 1], [1.0, 1.0], lpgen.LE, 5.0)]))
    assert _list(r) == ([], [], []) and r["rounds"] == 1 and r["accepted"] == 0


def test_a_free_variable_gets_both_bounds():
    r = _run(hand([-INF, 1], [INF, 2], [([0, 1], [1.0, -1.0], lpgen.EQ, 0.0)]))         # x0 = x1
    assert _list(r) == ([0], [1.0], [2.0])


def test_integer_rounding():
    lp = hand([0, 0], [10, 10], [([0, 1], [2.0, 3.0], lpgen.LE, 7.0)])
    assert _list(_run(lp)) == ([0, 1], [0.0, 0.0], [3.5, 7.0 / 3.0])
    assert _list(_run(lp, is_int=[True, True])) == ([0, 1], [0.0, 0.0], [3.0, 2.0])
    assert _list(_run(lp, is_int=[False, True])) == ([0, 1], [0.0, 0.0], [3.5, 2.0])
    lp = hand([0, 0], [10, 10], [([0, 1], [2.0, 3.0], lpgen.GE, 31.0)])                  # x0 >= 0.5 -> 1, x1 >= 11 / 3 -> 4
    assert _list(_run(lp, is_int=[True, True], max_rounds=1)) == ([0, 1], [1.0, 4.0], [10.0, 10.0])


def test_the_clamp_and_the_infeasible_stop():
    rows = lambda rhs: [([0, 1], [1.0, 1.0], lpgen.GE, rhs)]
    r = _run(hand([0, 0], [1, 0], rows(1.0 + 5e-10)))                                    # x0 >= 1 + 5e-10 against x0 <= 1: clamped
    assert _list(r) == ([0], [1.0], [1.0]) and not r["infeasible"]
    r = _run(hand([0, 0], [1, 0], rows(1.5)))
    assert r["infeasible"] and _list(r) == ([], [], []) and r["rounds"] == 1
    assert _run(hand([0, 0], [1, 0], rows(1.0 + 5e-8)))["infeasible"]                     # beyond the clamp: 5e-8 > 1e-9
    r = _run(hand([1, 0], [1, 1], rows(1.0 + 5e-8)))                                     # x1 >= 5e-8: below the acceptance threshold
    assert not r["infeasible"] and _list(r) == ([], [], [])
    r = _run(hand([1, 0], [2, 5], [([0, 1], [1.0, 1.0], lpgen.LE, 0.5)]))                # an upper candidate below a lower bound
    assert r["infeasible"]


def test_a_fixed_column_counts_at_its_value_and_is_not_listed():
    lp = hand([0, 0, 0], [1, 1, 1], [([0, 1, 2], [1.0, 1.0, 1.0], lpgen.LE, 1.0)])
    assert _list(_run(lp)) == ([], [], [])
    r = _run(lp, fixed={0: 1.0})
    assert _list(r) == ([1, 2], [0.0, 0.0], [0.0, 0.0])
    assert _run(lp, fixed={0: 1.0, 1: 1.0})["infeasible"]


def test_a_constraint_without_terms_has_no_row():
    lp = hand([0, 0], [10, 10], [([0, 1], [1.0, 1.0], lpgen.LE, 4.0), ([], [], lpgen.LE, 1.0), ([1], [2.0], lpgen.LE, 2.0)])
    form = internal_form(lp)
    assert len(form[3]) == 2 and form[1].tolist() == [0, 1, 2, 1, 3]
    assert _list(propagate(form, 2)) == ([0, 1], [0.0, 0.0], [4.0, 1.0])


def test_the_chain_moves_one_variable_per_round():
    lp = chain_lp(12)
    r = _run(lp, max_rounds=10)
    assert r["vars"].tolist() == list(range(2, 12)) and (r["lo"] == 1.0).all() and (r["hi"] == 10.0).all()
    assert r["rounds"] == 10 and r["accepted_struct"] == [1] * 10
    for k in (1, 3):
        assert _run(lp, max_rounds=k)["vars"].tolist() == list(range(12 - k, 12))
    r = _run(lp, max_rounds=64)
    assert r["vars"].tolist() == list(range(12)) and r["rounds"] == 13 and r["accepted_struct"] == [1] * 12 + [0]


# ------------------------------------------------------------------------------------------------ the generators
def _counts(r):
    return len(r["vars"]), int((r["lo"] == r["hi"]).sum()), r["infeasible"]


def test_counts_on_the_generators():
    """The figures of DESIGN.md §7.9."""
    r = _run(lpgen.gen_mixed_lp(300, 400, 6, 3))
    assert _counts(r) == (200, 0, False) and r["accepted_struct"] == [121, 90, 55, 37, 33, 36, 25, 23, 14, 8] and r["rounds"] == 10
    r = _run(lpgen.gen_sparse_lp(400, 300, 12, 7))
    assert _counts(r) == (300, 0, False) and r["accepted_struct"] == [300, 0] and np.isfinite(r["hi"]).all()
    assert _counts(_run(lpgen.gen_cover_lp(70, 90, 5, 5))) == (0, 0, False)
    assert _counts(_run(lpgen.gen_mixed_lp(40, 30, 6, 9))) == (17, 0, False)
    b = gen_bounded_lp(300, 400, 6, 3)
    assert _counts(_run(b)) == (189, 0, False)
    r = _run(b, is_int=np.ones(400, bool))
    assert r["infeasible"] and r["rounds"] == 1
    tm = D.two_matching(D.grid_points(4, 4))
    assert _counts(_run(tm)) == (0, 0, False)
    r = _run(tm, fixed={j: 1.0 for j in row_vars(tm, 0, 2)})
    assert _counts(r) == (13, 13, False) and (r["lo"] == 0.0).all() and (r["hi"] == 0.0).all()
    r = _run(tm, fixed={j: 1.0 for j in row_vars(tm, 0, 3)})
    assert r["infeasible"] and r["rounds"] == 1
    a = D.assignment(6, 1)
    assert _counts(_run(a)) == (36, 0, False)
    assert _counts(_run(a, fixed={row_vars(a, 0, 1)[0]: 1.0}, is_int=np.ones(36, bool))) == (35, 10, False)
    p = D.unit_packing(30, 40, 4, 1)
    assert _counts(_run(p)) == (40, 0, False)
    assert _counts(_run(p, fixed={row_vars(p, 0, 1)[0]: 1.0}, is_int=np.ones(40, bool))) == (39, 6, False)


@pytest.mark.parametrize("name,gen,args", [("mixed", lpgen.gen_mixed_lp, (300, 400, 6, 3)), ("small-mixed", lpgen.gen_mixed_lp, (40, 30, 6, 9)),
                                           ("sparse-maximize", lpgen.gen_sparse_lp, (400, 300, 12, 7)), ("cover", lpgen.gen_cover_lp, (70, 90, 5, 5)),
                                           ("bounded", gen_bounded_lp, (300, 400, 6, 3))])
def test_no_acceptance_sits_on_the_threshold(name, gen, args):
    """The comparison of the device with this yardstick on continuous data must not hang on a rounding error: no improvement of a
    finite bound that the yardstick sees lies between 0.5 and 2 times the acceptance threshold."""
    r = _run(gen(*args))
    ratios = np.asarray(r["ratios"], dtype=float)
    near = ratios[(ratios > 0.5) & (ratios < 2.0)]
    above = ratios[ratios >= 2.0]
    print("%s: %d improvements, nearest above the threshold %.3g x" % (name, len(ratios), above.min() if len(above) else INF))
    assert len(near) == 0, near
    assert ACCEPT_RTOL == 1e-7


# ------------------------------------------------------------------------------------------------ names and ABI
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
    assert "typedef struct mlp_propagate_info" in hdr and "Still version 5: the bound propagation" in hdr
    args = re.search(r"pub fn mlp_solution_propagate_bounds\s*\(([^)]*)\)", sys_rs).group(1)
    assert [a.split(":")[0].strip() for a in args.split(",")] == ["s", "var_is_int", "num_vars", "max_rounds", "vars", "new_lo", "new_hi", "cap",
                                                                  "count", "infeasible"]
    assert re.search(r"pub fn propagate_bounds\s*\(&self", lib_rs) and re.search(r"pub fn tighten_by_propagation\s*\(self", lib_rs)
    ext = surface.split("### extensions")[1]
    for n in ("propagate_bounds", "tighten_by_propagation"):
        assert re.search(r"\* `pub fn %s\(&?self, .*`" % n, ext), n
    for n in ("propagate_bounds", "tighten_by_propagation", "propagate_info"):
        assert hasattr(M.Solution, n), n


def test_abi_version_is_still_5_and_the_struct_size_matches(L):
    assert L.mlp_abi_version() == 5 == api.ABI_VERSION
    assert L.mlp_propagate_info_size() == ctypes.sizeof(api.MlpPropagateInfo) == 56
    assert L.mlp_bounds_info_size() == 80 and L.mlp_fix_info_size() == 96                 # no existing struct grew


def test_null_handle_is_einval_not_a_crash(L):
    h = ctypes.c_void_p()
    v, a, b = np.zeros(1, dtype=np.uint32), np.zeros(1), np.ones(1)
    pu, pd = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_double)
    pv, pa, pb = v.ctypes.data_as(pu), a.ctypes.data_as(pd), b.ctypes.data_as(pd)
    cnt, inf = ctypes.c_uint64(7), ctypes.c_int(7)
    assert L.mlp_solution_propagate_bounds(None, None, 0, 10, pv, pa, pb, 1, ctypes.byref(cnt), ctypes.byref(inf)) == -1
    assert L.mlp_solution_tighten_by_propagation(ctypes.byref(h), None, 0, 10, ctypes.byref(cnt), ctypes.byref(inf)) == -1
    assert L.mlp_solution_tighten_by_propagation(None, None, 0, 10, ctypes.byref(cnt), ctypes.byref(inf)) == -1
    assert L.mlp_solution_propagate_info(None, ctypes.byref(api.MlpPropagateInfo())) == -1
