"""CPU: the degenerate integer-data generators (tests/degenerate_lp.py) and the oracle-side preconditions a comparison of the engine
with the oracle on them relies on — checked here without a GPU: the shapes the generators promise, that a seed pins the bytes, and for every instance that the
oracle finds it feasible and bounded, reaches HiGHS' objective (HIGHS_RTOL) and the exact integer optimum, with an integral
(half-integral: two_matching) x; the issue's eight instances by the dual simplex alone, `matching` and `unit_packing` by the primal."""
import math

import numpy as np
import pytest

from minilp_amd import lpgen
from tests import degenerate_lp as D


def _cols(lp):
    return np.bincount(lp["indices"], minlength=lp["n"])


def test_assignment_shape():
    lp = D.assignment(7, 3)
    assert (lp["m"], lp["n"]) == (14, 49) and (lp["ops"] == lpgen.EQ).all() and (lp["rhs"] == 1.0).all() and (lp["data"] == 1.0).all()
    assert (np.diff(lp["indptr"]) == 7).all() and (_cols(lp) == 2).all()
    assert set(lp["obj"]) <= set(range(1, 10)) and (lp["lo"] == 0).all() and np.isinf(lp["hi"]).all() and lp["direction"] == lpgen.MINIMIZE
    for i in range(7):                                       # column i * n + j sits in row i and in row n + j
        for j in range(7):
            rows = [r for r in range(14) if i * 7 + j in lp["indices"][lp["indptr"][r]:lp["indptr"][r + 1]]]
            assert rows == [i, 7 + j]


def test_unit_transport_shape():
    S, Dn, deg = 60, 80, 3
    lp = D.unit_transport(S, Dn, deg, 3)
    assert (lp["m"], lp["n"]) == (S + Dn, Dn * deg) and (lp["data"] == 1.0).all() and (_cols(lp) == 2).all()
    assert (lp["ops"][:S] == lpgen.LE).all() and (lp["ops"][S:] == lpgen.GE).all()
    d = lp["rhs"][S:]
    assert set(d) <= {1.0, 2.0, 3.0} and (lp["rhs"][:S] == math.ceil(2.0 * d.sum() / S)).all()
    assert set(lp["obj"]) <= set(range(1, 6)) and (np.diff(lp["indptr"])[S:] == deg).all() and (np.diff(lp["indptr"])[:S] >= 1).all()
    for j in range(Dn):                                      # the arcs of a demand node go to distinct supply nodes
        arcs = lp["indices"][lp["indptr"][S + j]:lp["indptr"][S + j + 1]]
        assert list(arcs) == list(range(j * deg, (j + 1) * deg))


def test_unit_cover_shape():
    lp = D.unit_cover(70, 90, 5, 5)
    assert (lp["m"], lp["n"]) == (70, 90) and (lp["ops"] == lpgen.GE).all() and (lp["rhs"] == 1.0).all() and (lp["obj"] == 1.0).all()
    assert (lp["lo"] == 0).all() and (lp["hi"] == 1).all() and (lp["data"] == 1.0).all()
    for i in range(70):
        row = lp["indices"][lp["indptr"][i]:lp["indptr"][i + 1]]
        assert len(row) == 5 and (np.diff(row) > 0).all()


def test_two_matching_shape():
    lp = D.two_matching(D.grid_points(6, 6))
    assert (lp["m"], lp["n"]) == (36, 630) and (lp["ops"] == lpgen.EQ).all() and (lp["rhs"] == 2.0).all() and (_cols(lp) == 2).all()
    assert (lp["obj"] == np.round(lp["obj"])).all() and lp["obj"].min() == 1.0 and lp["obj"].max() == round(math.hypot(5, 5))
    thin = D.two_matching(D.grid_points(9, 9), nearest=12)
    assert thin["m"] == 81 and 81 * 6 <= thin["n"] <= 81 * 12 and (np.diff(thin["indptr"]) >= 12).all() and (_cols(thin) == 2).all()


@pytest.mark.parametrize("case", list(D.CASES))
def test_a_seed_pins_the_instance(case):
    a, b = D.CASES[case](), D.CASES[case]()
    assert a["name"] == b["name"] and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes()
                                          for k in ("obj", "lo", "hi", "indptr", "indices", "data", "ops", "rhs"))
    assert (np.diff(a["indptr"]) > 0).all()


@pytest.mark.parametrize("case", list(D.CASES) + list(D.PRIMAL_CASES))
def test_oracle_side_preconditions(case):
    ref = D.reference(case)                                     # (asserts them; see its docstring)
    assert ref["pivots"] >= 40
    if ref["family"] not in ("unit_cover", "unit_packing"):
        assert ref["exact"] is not None and ref["objective"] == ref["exact"]
    # the eight instances of the issue are dual-only, their primal counterparts primal-only: tests/test_degenerate.py builds on both
    assert (ref["primal_iters"] > 0) == (case in D.PRIMAL_CASES)


def test_primal_counterparts_shape():
    lp = D.matching(6, 1)
    assert lp["direction"] == lpgen.MAXIMIZE and (lp["ops"] == lpgen.LE).all() and (lp["rhs"] == 1.0).all() and (_cols(lp) == 2).all()
    assert np.array_equal(lp["indices"], D.assignment(6, 1)["indices"]) and set(lp["obj"]) <= set(range(1, 10))
    lp = D.unit_packing(30, 20, 4, 2)
    assert lp["direction"] == lpgen.MAXIMIZE and (lp["ops"] == lpgen.LE).all() and (lp["obj"] == 1.0).all() and np.isinf(lp["hi"]).all()
    assert (np.diff(lp["indptr"]) == 4).all()
