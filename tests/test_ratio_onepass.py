"""GPU: the list form of the primal Harris test — both passes in ONE grid pass of k_ratio_primal_fused (tests/test_ratio_list_model.py
states the rule and checks it against the two passes on the CPU).

MLP_STR_K=0, MLP_RATIO_ONE=0 and MLP_HYPER=0 throughout: the grid form of the test and the dense chain of the medium nucleus then run
at sizes of a few thousand rows (2 and 4 ratio blocks).  Every solve must take the oracle's pivots (solver.rs:782-853 decides the same
leaving row whatever the form); the counters of the control block show that the list form decided (`ratio_list_decisions`) and
whether its final block had to re-scan (`ratio_list_overflows`: never with the default cap on continuous data, always with a cap of
0).  On the degenerate instances every ratio ties: the form must take the pivots of the publish-wait form of the same build."""
import numpy as np
import pytest

import minilp_amd as M
from minilp_amd import lpgen
from oracle import minilp_oracle as O
from tests import degenerate_lp as D
from tests.common import obj_close

pytestmark = pytest.mark.gpu

INSTANCES = {"two blocks": ((1500, 1200, 10, 3), None), "four blocks": ((4000, 3500, 12, 4), 300)}
_cache = {}


def _grid(monkeypatch):
    for k, val in (("MLP_STR_K", "0"), ("MLP_RATIO_ONE", "0"), ("MLP_HYPER", "0")):
        monkeypatch.setenv(k, val)


def _instance(name, hi=None):
    """The model and the oracle's solve of it, computed once."""
    key = (name, hi)
    if key not in _cache:
        args, budget = INSTANCES[name]
        lp = lpgen.gen_sparse_lp(*args)
        if hi is not None:
            lp["hi"] = np.full(lp["n"], np.inf)
            lp["hi"][::2] = hi
        kw = dict(trace=True) if budget is None else dict(trace=True, budget=budget)
        so = lpgen.build_problem(O.Problem, lp).solve(**kw)
        _cache[key] = (lp, kw, [t[:5] for t in so.trace()], so.objective())
    return _cache[key]


def _solve(lp, kw):
    s = lpgen.build_problem(M.Problem, lp).solve(**kw)
    return s, s.stats()


@pytest.mark.parametrize("name", list(INSTANCES))
def test_list_form_takes_the_oracles_pivots(monkeypatch, name):
    _grid(monkeypatch)
    lp, kw, trace, obj = _instance(name)
    s, st = _solve(lp, kw)
    blocks = (lp["m"] + 1023) // 1024
    print(f"{name}: {st['iterations']} pivots, ratio blocks {blocks}, form {s.state('ratio_primal_form')}, list {s.state('ratio_list')}")
    assert int(s.state("ratio_primal_form")[0]) == 1 and int(s.state("ratio_list")[0]) == 1
    assert [t[:5] for t in s.trace()] == trace
    assert obj_close(s.objective(), obj)
    assert s.reinvert() < 1e-8
    assert st["ratio_list_decisions"] > 0 and st["ratio_list_overflows"] == 0, (st["ratio_list_decisions"], st["ratio_list_overflows"])


def test_knob_restores_the_publish_wait_form(monkeypatch):
    _grid(monkeypatch)
    monkeypatch.setenv("MLP_RATIO_LIST", "0")
    lp, kw, trace, obj = _instance("two blocks")
    s, st = _solve(lp, kw)
    assert int(s.state("ratio_list")[0]) == 0 and st["ratio_list_decisions"] == 0
    assert [t[:5] for t in s.trace()] == trace


def test_a_list_that_does_not_fit_is_rescanned_by_the_final_block(monkeypatch):
    _grid(monkeypatch)
    monkeypatch.setenv("MLP_RATIO_LIST_CAP", "0")
    lp, kw, trace, obj = _instance("two blocks")
    s, st = _solve(lp, kw)
    assert [t[:5] for t in s.trace()] == trace
    assert obj_close(s.objective(), obj)
    assert s.reinvert() < 1e-8
    assert st["ratio_list_decisions"] > 0 and st["ratio_list_overflows"] > 0, (st["ratio_list_decisions"], st["ratio_list_overflows"])


def test_bound_flips(monkeypatch):
    """No candidate within the entering variable's own range: a bound flip.  An upper bound of 5 on EVERY variable (what
    tools/regime_curve.py sets) does not get there: with every variable boxed the start is dual feasible and the whole solve is the dual
    simplex — 5 276 pivots, no primal ratio test, no flip, in the oracle as well.  An upper bound of 0.2 on every second variable keeps
    the solve primal (1 641 pivots in the oracle, 31 of them flips)."""
    _grid(monkeypatch)
    lp, kw, trace, obj = _instance("two blocks", hi=0.2)
    s, st = _solve(lp, kw)
    print(f"bounded: {st['iterations']} pivots, {st['bound_flips']} flips, list decisions {st['ratio_list_decisions']}")
    assert [t[:5] for t in s.trace()] == trace
    assert obj_close(s.objective(), obj)
    assert st["bound_flips"] > 0 and st["ratio_list_decisions"] > 0


@pytest.mark.parametrize("case", [c for c in D.PRIMAL_CASES if D.family(c) in ("matching", "unit_packing")])
def test_ties_take_the_pivots_of_the_publish_wait_form(monkeypatch, case):
    _grid(monkeypatch)
    lp = D.PRIMAL_CASES[case]()
    so = lpgen.build_problem(O.Problem, lp).solve()
    runs = []
    for on in ("1", "0"):
        monkeypatch.setenv("MLP_RATIO_LIST", on)
        s = lpgen.build_problem(M.Problem, lp).solve(trace=True)
        runs.append((s.trace(), s.objective(), s.stats(), s.values().tobytes()))
    st = runs[0][2]
    print(f"{case}: {st['iterations']} pivots ({st['primal_iters']} primal), list decisions {st['ratio_list_decisions']}")
    assert abs(runs[0][1] - so.objective()) <= 1e-9 * max(1.0, abs(so.objective()))
    assert runs[0][0] == runs[1][0] and runs[0][3] == runs[1][3]   # the same pivots, and x bit for bit
    assert st["primal_iters"] > 0
    assert st["ratio_list_decisions"] > 0 and runs[1][2]["ratio_list_decisions"] == 0


@pytest.mark.parametrize("name", list(INSTANCES))
def test_medium_nucleus_without_a_btran_launch(monkeypatch, name):
    """t_K rides in the ratio launch and its final block forms rho_K (the sums of k_btran, in its order): the pivots are the oracle's with
    and without the BTRAN launch, and x agrees bit for bit.  state("btran_ride")[1] counts the iterations whose rho_K the ratio launch
    formed — the predicate that empties the BTRAN stage is the one that asks the ratio launch for it."""
    _grid(monkeypatch)
    lp, kw, trace, obj = _instance(name)
    runs = []
    for on in ("1", "0"):
        monkeypatch.setenv("MLP_BTRAN_RIDE", on)
        s, st = _solve(lp, kw)
        runs.append(([t[:5] for t in s.trace()], s.values().tobytes(), s.state("btran_ride").tolist(), st, s.reinvert()))
    print(f"{name}: btran_ride on {runs[0][2]}, off {runs[1][2]}; primal pivots {runs[0][3]['primal_iters']}, nucleus {runs[0][3]['nucleus_size']}")
    assert runs[0][0] == trace and runs[1][0] == trace
    assert runs[0][1] == runs[1][1]
    assert runs[0][2][1] > 0 and runs[1][2][1] == 0, (runs[0][2], runs[1][2])
    assert runs[0][4] < 1e-8
