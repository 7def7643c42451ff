"""CPU: the bounded-variable family (tests/bounded_lp.py) and the oracle-side preconditions tests/test_bounded.py relies on, checked
without a GPU.  Per instance: the oracle terminates Optimal and reaches HiGHS' objective (HIGHS_RTOL); it takes dual pivots, primal
pivots and at least four bound flips; its optimum leaves columns of every bounded kind non-basic at a finite upper bound and at a
negative lower bound; no column is free, every kind of bound and every row operator occurs; and the relabelling check: the instance
with rows and columns in reverse order, where every row sum rounds differently, gives the same sequence of (phase, entering variable,
leaving variable) over the whole trace, i.e. no decision of the sequence lies within rounding of a tie.

The 40 x 30 instance has too few columns for every kind to end at a bound: it is held to everything else.  The one-loop variants
(primal_start, dual_start) are held to their own start conditions and to the relabelling check."""
import numpy as np
import pytest
import scipy.sparse as sp

from minilp_amd import lpgen
from oracle import minilp_oracle as O
from tests import bounded_lp as B
from tests.common import GEN, X_ATOL, obj_close

ALL = [B.SMALL] + B.CASES
VARIANTS = B.PRIMAL_START_CASES + B.DUAL_START_CASES
# (args) -> (trace, pivots, flips, primal iterations, dual iterations, objective): the oracle's numbers the family was chosen by
EXPECTED = {
    (40, 30, 6, 9): (33, 29, 4, 11, 22, 1.264292186),
    (120, 160, 6, 11): (144, 136, 8, 64, 80, -10.629244079),
    (300, 400, 6, 3): (377, 364, 13, 182, 195, -15.551622630),
    (300, 260, 8, 6): (462, 453, 9, 204, 258, -8.090595520),
    (400, 300, 12, 7): (643, 639, 4, 238, 405, -7.770549418),
    (700, 600, 12, 6): (1628, 1619, 9, 751, 877, -12.615895122),
}


@pytest.mark.parametrize("case", ALL, ids=B.case_id)
def test_a_seed_pins_the_instance(case):
    a, b = B.gen_bounded_lp(*case), GEN["bounded"](*case)
    assert a["name"] == b["name"] == "bounded_%dx%d_k%d_s%d" % case
    assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("obj", "lo", "hi", "indptr", "indices", "data", "ops", "rhs"))
    base = lpgen.gen_sparse_lp(*case)
    assert np.array_equal(a["indices"], base["indices"]) and np.array_equal(a["indptr"], base["indptr"])      # gen_sparse_lp's pattern
    assert a["direction"] == lpgen.MINIMIZE and (a["data"] != 0).all() and (np.abs(a["data"]) >= 0.1).all() and (np.abs(a["data"]) < 1.0).all()


@pytest.mark.parametrize("case", ALL, ids=B.case_id)
def test_every_kind_of_bound_and_every_operator_occurs(case):
    lp = B.gen_bounded_lp(*case)
    lo, hi, kinds = lp["lo"], lp["hi"], B.column_kinds(lp["n"], case[3])
    assert not (np.isinf(lo) & np.isinf(hi)).any()                                     # no free column (module docstring of bounded_lp)
    assert (lo <= hi).all() and not np.isnan(lo).any() and not np.isnan(hi).any()
    for kind in range(6):
        assert (kinds == kind).any(), B.KIND_NAMES[kind]
    sel = lambda kind: kinds == kind
    assert (lo[sel(B.NONNEG)] == 0).all() and np.isinf(hi[sel(B.NONNEG)]).all()
    assert (lo[sel(B.NARROW)] == 0).all() and (hi[sel(B.NARROW)] > 0).all() and (hi[sel(B.NARROW)] <= 0.02 * 1.5).all()
    assert (hi[sel(B.WIDE)] - lo[sel(B.WIDE)] >= 0.3 - 1e-12).all() and np.isfinite(lo[sel(B.WIDE)]).all()
    assert (lo[sel(B.UPPER_ONLY)] == -np.inf).all() and np.isfinite(hi[sel(B.UPPER_ONLY)]).all()
    assert np.isfinite(lo[sel(B.LOWER_ONLY)]).all() and np.isinf(hi[sel(B.LOWER_ONLY)]).all()
    assert (lo[sel(B.FIXED)] == hi[sel(B.FIXED)]).all()
    if case != B.SMALL:                                                                # lower bounds of either sign
        for kind in (B.WIDE, B.LOWER_ONLY):
            assert (lo[sel(kind)] < 0).any() and (lo[sel(kind)] > 0).any(), B.KIND_NAMES[kind]
    for op in (lpgen.EQ, lpgen.LE, lpgen.GE):
        assert (lp["ops"] == op).any(), op


@pytest.mark.parametrize("case", ALL, ids=B.case_id)
def test_oracle_side_preconditions(case):
    ref = B.reference(case)                                   # (asserts Optimal, a feasible x and HiGHS' objective; see its docstring)
    lp, st, trace, kinds = ref["lp"], ref["stats"], ref["trace"], ref["kinds"]
    flips = [t for t in trace if t[2] == -1]
    print(f"{B.case_id(case)}: trace {len(trace)}, pivots {st['pivots']}, flips {st['bound_flips']}, primal / dual {st['primal_iters']} / "
          f"{st['dual_iters']}, objective {ref['objective']!r} (HiGHS {ref['highs']!r}); non-basic at upper by kind "
          f"{[int((ref['nb_upper'] & (kinds == q)).sum()) for q in range(6)]}, at a negative lower bound "
          f"{[int((ref['nb_lower'] & (kinds == q) & (lp['lo'] < 0)).sum()) for q in range(6)]}")
    assert st["primal_iters"] > 0 and st["dual_iters"] > 0 and st["bound_flips"] >= 4
    assert len(flips) == st["bound_flips"] and len(trace) == st["pivots"] + st["bound_flips"]
    assert all(kinds[t[3]] in (B.NARROW, B.WIDE) for t in flips)                       # only a boxed column can flip
    want = EXPECTED[tuple(case)]
    assert (len(trace), st["pivots"], st["bound_flips"], st["primal_iters"], st["dual_iters"]) == want[:5]
    assert abs(ref["objective"] - want[5]) <= 1e-9
    # the optimum rests on upper bounds and on negative lower bounds: x is exactly the bound there
    up, low = ref["nb_upper"] & (lp["lo"] < lp["hi"]), ref["nb_lower"] & (lp["lo"] < 0) & (lp["lo"] < lp["hi"])
    assert (ref["x"][up] == lp["hi"][up]).all() and (ref["x"][low] == lp["lo"][low]).all()
    assert up.any() and low.any()
    if case != B.SMALL:
        for kind in (B.NARROW, B.WIDE, B.UPPER_ONLY):
            assert (up & (kinds == kind)).any(), B.KIND_NAMES[kind]
        for kind in (B.WIDE, B.LOWER_ONLY):
            assert (low & (kinds == kind)).any(), B.KIND_NAMES[kind]


@pytest.mark.parametrize("case", VARIANTS, ids=B.case_id)
def test_one_loop_variants(case):
    """primal_start: the start point is strictly feasible and the solve is the primal loop alone, with bound flips; dual_start: the
    start point is dual feasible, the solve the dual loop alone.  Both keep the columns, the matrix and the bounds of the family, are
    feasible and bounded (reference() asserts Optimal and HiGHS' objective) and end with columns of every bounded kind at a bound."""
    ref = B.reference(case)
    lp, st, kinds, base = ref["lp"], ref["stats"], ref["kinds"], B.gen_bounded_lp(*case[1:])
    assert all(np.array_equal(lp[k], base[k]) for k in ("lo", "hi", "indptr", "indices", "data"))
    assert not (np.isinf(lp["lo"]) & np.isinf(lp["hi"])).any()
    print(f"{B.case_id(case)}: trace {len(ref['trace'])}, pivots {st['pivots']}, flips {st['bound_flips']}, primal / dual {st['primal_iters']} / "
          f"{st['dual_iters']}, objective {ref['objective']!r} (HiGHS {ref['highs']!r})")
    xs = B._start_point(lp)
    lhs = np.add.reduceat(lp["data"] * xs[lp["indices"]], lp["indptr"][:-1])
    if case[0] == "primal":
        assert np.array_equal(lp["obj"], base["obj"]) and not (lp["ops"] == lpgen.EQ).any()
        assert (np.where(lp["ops"] == lpgen.LE, lp["rhs"] - lhs, lhs - lp["rhs"]) >= 0.05 - 1e-12).all()     # strictly feasible start
        assert st["dual_iters"] == 0 and st["primal_iters"] > 0 and st["bound_flips"] >= 4
    else:
        assert np.array_equal(lp["ops"], base["ops"]) and np.array_equal(lp["rhs"], base["rhs"])
        at_hi = xs == lp["hi"]
        assert (lp["obj"][~at_hi] >= 0).all() and (lp["obj"][at_hi & (lp["lo"] < lp["hi"])] <= 0).all()       # dual feasible start
        viol = np.where(lp["ops"] == lpgen.LE, lhs - lp["rhs"], np.where(lp["ops"] == lpgen.GE, lp["rhs"] - lhs, np.abs(lhs - lp["rhs"])))
        assert viol.max() > 1e-3                                                                              # and primal infeasible
        assert st["primal_iters"] == 0 and st["dual_iters"] > 0 and st["bound_flips"] == 0
    up, low = ref["nb_upper"] & (lp["lo"] < lp["hi"]), ref["nb_lower"] & (lp["lo"] < 0) & (lp["lo"] < lp["hi"])
    for kind in (B.NARROW, B.WIDE, B.UPPER_ONLY):
        assert (up & (kinds == kind)).any(), B.KIND_NAMES[kind]
    for kind in (B.WIDE, B.LOWER_ONLY):
        assert (low & (kinds == kind)).any(), B.KIND_NAMES[kind]


@pytest.mark.parametrize("case", ALL + VARIANTS, ids=B.case_id)
def test_relabelling_rows_and_columns_keeps_the_sequence(case):
    ref = B.reference(case)
    lp = ref["lp"]
    m, n = lp["m"], lp["n"]
    twin = B.relabelled(lp)
    csr = lambda q: sp.csr_matrix((q["data"], q["indices"], q["indptr"]), shape=(m, n))
    assert np.array_equal(csr(twin).toarray(), csr(lp).toarray()[::-1, ::-1]) and csr(twin).has_sorted_indices
    assert all(np.array_equal(twin[k], lp[k][::-1]) for k in ("obj", "lo", "hi", "ops", "rhs"))
    st =lpgen.build_problem(O.Problem, twin).solve(trace=True)
    a = [(t[0], t[3], t[4]) for t in ref["trace"]]
    b = [(t[0], B.relabel_var(t[3], m, n), B.relabel_var(t[4], m, n)) for t in st.trace()]
    first = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), None)
    assert a == b, (first, len(a), len(b), a[first] if first is not None else None, b[first] if first is not None else None)
    assert obj_close(st.objective(), ref["objective"]) and np.abs(st.values()[::-1] - ref["x"]).max() <= X_ATOL
