"""GPU: every form of k_update_pivot<PHASE, DSE, PSE, COMB, PULL> — one instance per form of the iteration, the trip's loads issued as one
group ahead of its stores — takes the oracle's pivots.

Each case runs a solve whose settings force one form, and checks the oracle's pivot trace and objective, reinvert() < 1e-8,
max_pivot_err < 1e-7 (the engine's own refresh threshold) and a stats / state field that shows the intended path ran.  On the sizes with
pulled F products (no float atomics) two solves must also agree bit for bit in x, the reduced costs and the basis — a case whose solve
is beyond the 2^21 non-zeros up to which the products are pulled fails rather than compares.

The engine-level stepped solve (mlp_engine_open / mlp_engine_stage) keeps k_band_combine and the COMB = 0 form of the update kernel: it
sums the same band partials independently, so on the banded cases the stepped and the whole solve must agree bit for bit — they do on
the parent of the change that made the forms (STEPPED lists the cases; checked there)."""
import numpy as np
import pytest

import minilp_amd as M
from minilp_amd import lpgen
from oracle import minilp_oracle as O
from tests import bounded_lp as B
from tests.common import obj_close

pytestmark = pytest.mark.gpu

REFRESH_TOL = 1e-7
HEAD = dict(MLP_HYPER="0", MLP_DETERMINISTIC="0")  # pushed F products: the head has all its slots (tests/test_primal_head.py)
MEDIUM = {k: "0" for k in ("MLP_STR_K", "MLP_RATIO_ONE", "MLP_HYPER", "MLP_PRIMAL_HEAD", "MLP_SMALL_BASIS")}  # tests/test_v_ride.py::_medium
BAND_ROWS = 8192  # rows per band of the banded sweep: 16 bands end at 131 072 rows


def _bounded_every_second(lp, hi):
    lp["hi"] = np.full(lp["n"], np.inf)
    lp["hi"][::2] = hi
    return lp


# name: (instance, pivot budget, settings, two solves bit for bit, what shows the path)
CASES = {
    "banded COMB, one short band": (lambda: lpgen.gen_sparse_lp(4000, 3500, 12, 4), 300, dict(MEDIUM, MLP_BANDED="1"), True,
                                    lambda st, s: st["banded_sweep"] == 1 and st["primal_iters"] > 0 and s.state("v_ride")[1] > 0),
    "banded COMB, three bands, last one short": (lambda: lpgen.gen_sparse_lp(20000, 6000, 6, 5), 200, dict(MEDIUM, MLP_BANDED="1"), True,
                                                 lambda st, s: st["banded_sweep"] == 1 and st["primal_iters"] > 0),
    "banded COMB, seventeen bands: a second round of partials": (lambda: lpgen.gen_sparse_lp(16 * BAND_ROWS + 7, 3000, 3, 6), 150,
                                                                 dict(MEDIUM, MLP_BANDED="1"), True,
                                                                 lambda st, s: st["banded_sweep"] == 1 and st["num_constraints"] > 16 * BAND_ROWS),
    "banded COMB in the locality order": (lambda: lpgen.gen_sparse_lp(4000, 3500, 12, 4), 300,
                                          dict(MEDIUM, MLP_BANDED="1", MLP_ORDER_FROM="0", MLP_ORDER_EVERY="5"), True,
                                          lambda st, s: st["banded_sweep"] == 1 and st["primal_iters"] > 0),
    "bound flips": (lambda: _bounded_every_second(lpgen.gen_sparse_lp(1500, 1200, 10, 3), 0.2), None, MEDIUM, True,
                    lambda st, s: st["bound_flips"] > 0),
    "primal, materialised tableau row": (lambda: lpgen.gen_sparse_lp(1500, 1200, 10, 3), None, MEDIUM, True,
                                         lambda st, s: st["banded_sweep"] == 0 and st["primal_iters"] > 0 and st["beta_rebuilds"] == 0),
    "eager DSE": (lambda: lpgen.gen_sparse_lp(1500, 1200, 10, 3), None, dict(MEDIUM, MLP_LAZY_DSE="0"), True,
                  # (the norms are read and no rebuild is counted: the recurrence kept them through the primal pivots)
                  lambda st, s: st["primal_iters"] > 0 and s.state("flags")[3] == 1 and np.isfinite(s.state("dual_edge_sq_norms")).all()
                  and s.stats()["beta_rebuilds"] == 0),
    "eager DSE, banded": (lambda: lpgen.gen_sparse_lp(20000, 6000, 6, 5), 200, dict(MEDIUM, MLP_BANDED="1", MLP_LAZY_DSE="0"), True,
                          lambda st, s: st["banded_sweep"] == 1 and st["primal_iters"] > 0),
    # (PULL = 2 against PULL = 1 is the setting alone: no counter tells the two apart; test_the_two_pulling_forms_agree holds them together)
    "primal head, update pulls and the head applies": (lambda: B.primal_start(400, 300, 12, 7), None, HEAD, False,
                                                       lambda st, s: s.state("primal_head_launches")[0] > 0),
    "primal head, update pulls and applies": (lambda: B.primal_start(400, 300, 12, 7), None, dict(HEAD, MLP_HEAD_APPLY="0"), False,
                                              lambda st, s: s.state("primal_head_launches")[0] > 0),
    # (a covering LP of the size of tests/degenerate_lp.py's unit_cover-400x500x6, with continuous data: on the 0/1 instance itself every
    # ratio ties, and the tie-break differs from the reference's by design, so no pivot sequence can be compared there — DESIGN §8)
    "dual without PSE over the listed row": (lambda: lpgen.gen_cover_lp(400, 500, 6, 5), None, dict(MLP_HYPER="0", MLP_STR_K="0", MLP_RATIO_ONE="0"), False,
                                             lambda st, s: st["dual_iters"] > 0 and s.state("flags")[2] == 0 and s.state("dual_list_tests")[0] > 0),
    "dual with PSE": (lambda: B.gen_bounded_lp(*B.SMALL), None, dict(MLP_HYPER="0"), False,
                      # (x = 0 is not dual feasible, so PSE is on from the start and the dual pivots of phase 1 run the PSE form; the flag itself
                      # is cleared again at the optimum — solver.rs:482 — so after the solve the two pivot counts are what can be read)
                      lambda st, s: st["dual_iters"] > 0 and st["primal_iters"] > 0),
}
STEPPED = ["banded COMB, one short band", "banded COMB, three bands, last one short", "banded COMB, seventeen bands: a second round of partials",
           "banded COMB in the locality order", "eager DSE, banded"]
_ref = {}


def _reference(name):
    """The instance and the oracle's solve of it, computed once."""
    if name not in _ref:
        gen, budget = CASES[name][:2]
        lp = gen()
        kw = dict(trace=True) if budget is None else dict(trace=True, budget=budget)
        so = lpgen.build_problem(O.Problem, lp).solve(**kw)
        _ref[name] = (lp, kw, [t[:5] for t in so.trace()], so.objective())
    return _ref[name]


@pytest.mark.parametrize("name", list(CASES))
def test_form_takes_the_oracles_pivots(monkeypatch, name):
    _, _, env, twice, ran = CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    lp, kw, trace, obj = _reference(name)
    s = lpgen.build_problem(M.Problem, lp).solve(**kw)
    st = s.stats()
    print(f"{name}: {st['iterations']} pivots ({st['primal_iters']} primal, {st['dual_iters']} dual, {st['bound_flips']} flips), nucleus "
          f"{st['nucleus_size']}, banded {st['banded_sweep']}, max_pivot_err {st['max_pivot_err']:.2e}")
    assert [t[:5] for t in s.trace()] == trace
    assert obj_close(s.objective(), obj)
    assert ran(st, s), st
    assert st["max_pivot_err"] < REFRESH_TOL, st["max_pivot_err"]
    if twice:  # pulled F products: nothing in the solve depends on the order of arrival
        assert st["nnz"] < 2 ** 21, st["nnz"]  # (the F products are pulled — deterministic — up to 2^21 non-zeros, pushed beyond)
        t = lpgen.build_problem(M.Problem, lp).solve(**kw)
        assert s.values().tobytes() == t.values().tobytes()
        for what in ("nb_var_obj_coeffs", "basic_vars"):
            assert s.state(what).tobytes() == t.state(what).tobytes(), what
    r = s.reinvert()
    assert r < 1e-8, r


def test_the_two_pulling_forms_agree(monkeypatch):
    """PULL = 2 (the head applies the basic side) and PULL = 1 (the update does) take the same pivots and end in the same basis."""
    lp, kw, trace, obj = _reference("primal head, update pulls and the head applies")
    for k, v in HEAD.items():
        monkeypatch.setenv(k, v)
    runs = []
    for apply in ("1", "0"):
        monkeypatch.setenv("MLP_HEAD_APPLY", apply)
        s = lpgen.build_problem(M.Problem, lp).solve(**kw)
        runs.append(([t[:5] for t in s.trace()], s.state("basic_vars").tobytes(), int(s.state("primal_head_launches")[0])))
    assert runs[0][0] == runs[1][0] == trace and runs[0][1] == runs[1][1]
    assert runs[0][2] > 0 and runs[1][2] > 0


def _stepped(lp, pivots):
    """`pivots` iterations through the engine-level stepping API, from the slack basis."""
    A = M.api
    s = lpgen.build_problem(M.Problem, lp).solve(budget=0, trace=True)
    it = 0
    while it < pivots:
        st, info = s.engine_open()
        if st in (A.ITER_OPTIMAL, A.ITER_INFEASIBLE, A.ITER_UNBOUNDED):
            break
        if st == A.ITER_FEASIBLE:
            continue
        while st in (A.ITER_PIVOT, A.ITER_FLIP) and it < pivots:
            while True:
                stage = info["next_stage"]
                st, info = s.engine_stage(stage)
                if stage == A.STAGE_APPLY or st not in (A.ITER_PIVOT, A.ITER_FLIP):
                    break
            if stage != A.STAGE_APPLY:
                break
            it += 1
    return s, it


@pytest.mark.parametrize("name", STEPPED)
def test_stepped_solve_agrees_bit_for_bit_with_the_whole_solve(monkeypatch, name):
    _, budget, env, _, _ = CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    lp, kw, trace, _ = _reference(name)
    whole = lpgen.build_problem(M.Problem, lp).solve(**kw)
    stepped, n = _stepped(lp, budget)
    assert n == budget and whole.stats()["banded_sweep"] == 1
    assert [t[:5] for t in stepped.trace()] == trace
    assert whole.values().tobytes() == stepped.values().tobytes()
    for what in ("nb_var_obj_coeffs", "primal_edge_sq_norms", "basic_vars"):
        assert whole.state(what).tobytes() == stepped.state(what).tobytes(), what
