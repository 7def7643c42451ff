"""GPU: the medium nucleus with the v partials riding in the ratio launch — v = B^-T alpha_q needs neither the leaving row nor rho, so the
rider blocks behind the ratio blocks of k_ratio_primal_fused form t_K AND the per-stripe partials of W^T t_K (v_ride_body), and the BASIS
stage is one launch: the v tail beside the eta-only pass over W (k_fused_w, VT).  MLP_V_RIDE=0 restores k_fused_w<8> with the v partials
+ k_post_fused.

MLP_STR_K=0, MLP_RATIO_ONE=0, MLP_HYPER=0, MLP_PRIMAL_HEAD=0 and MLP_SMALL_BASIS=0 make the medium chain run from the first pivot of a
model of a few thousand rows (as in tests/test_medium_chain.py).  The same sums run in the same order in both forms, and the pulled F
product is the default at these sizes, so on and off must agree bit for bit — and take the oracle's pivots."""
import numpy as np
import pytest

import minilp_amd as M
from minilp_amd import lpgen
from oracle import minilp_oracle as O
from tests import degenerate_lp as D
from tests.common import obj_close

pytestmark = pytest.mark.gpu

REFRESH_TOL = 1e-7  # the engine re-inverts W when the two-way pivot check (alpha_q[r] against alpha_r[q]) disagrees by more

# name: (gen_sparse_lp arguments, pivot budget, lanes per slot of the riders, smallest nucleus at the end)
INSTANCES = {
    "two blocks": ((1500, 1200, 10, 3), None, 16, 0),
    "four blocks": ((4000, 3500, 12, 4), 300, 16, 0),
    # two column chunks per stripe, the capacity growing 256 -> 2 048 with re-captured graphs, k not a multiple of 8 on the way
    "nucleus past 1024": ((4000, 3500, 12, 4), 1700, 16, 1025),
    "64 lanes": ((2000, 1000, 30, 7), None, 64, 0),  # two t_K rounds per rider
    "4 lanes": ((1500, 1020, 4, 4), None, 4, 0),
}
_cache = {}


def _medium(monkeypatch):
    for key in ("MLP_STR_K", "MLP_RATIO_ONE", "MLP_HYPER", "MLP_PRIMAL_HEAD", "MLP_SMALL_BASIS"):
        monkeypatch.setenv(key, "0")


def _lanes(lp):
    avg = len(lp["data"]) / lp["n"]
    return 64 if avg >= 40.0 else (16 if avg >= 6.0 else 4)


def _instance(name, hi=None):
    """The model and the oracle's solve of it, computed once."""
    key = (name, hi)
    if key not in _cache:
        args, budget, _, _ = INSTANCES[name]
        lp = lpgen.gen_sparse_lp(*args)
        if hi is not None:
            lp["hi"] = np.full(lp["n"], np.inf)
            lp["hi"][::2] = hi
        kw = dict(trace=True) if budget is None else dict(trace=True, budget=budget)
        so = lpgen.build_problem(O.Problem, lp).solve(**kw)
        _cache[key] = (lp, kw, [t[:5] for t in so.trace()], so.objective())
    return _cache[key]


def _on_off(monkeypatch, lp, kw):
    """The solve with MLP_V_RIDE = 1 and = 0: (pivots, x as bytes, state("v_ride"), stats, reinvert(), objective) of each."""
    runs = []
    for on in ("1", "0"):
        monkeypatch.setenv("MLP_V_RIDE", on)
        s = lpgen.build_problem(M.Problem, lp).solve(**kw)
        st = s.stats()
        runs.append(([t[:5] for t in s.trace()], s.values().tobytes(), s.state("v_ride").tolist(), st, s.reinvert(), s.objective()))
    return runs


@pytest.mark.parametrize("name", list(INSTANCES))
def test_on_and_off_agree_bit_for_bit_on_the_oracles_pivots(monkeypatch, name):
    _medium(monkeypatch)
    lp, kw, trace, obj = _instance(name)
    _, _, lanes, k_min = INSTANCES[name]
    assert _lanes(lp) == lanes
    on, off = _on_off(monkeypatch, lp, kw)
    print(f"{name}: v_ride on {on[2]}, off {off[2]}; {on[3]['iterations']} pivots ({on[3]['primal_iters']} primal), nucleus {on[3]['nucleus_size']}, "
          f"max_pivot_err {on[3]['max_pivot_err']:.2e} / {off[3]['max_pivot_err']:.2e}, reinvert {on[4]:.2e} / {off[4]:.2e}")
    assert on[0] == trace and off[0] == trace
    assert on[1] == off[1]
    assert obj_close(on[5], obj)
    for r in (on, off):
        assert r[4] < 1e-8, r[4]
        assert r[3]["max_pivot_err"] < REFRESH_TOL, r[3]["max_pivot_err"]
    assert on[3]["nucleus_size"] >= k_min, on[3]["nucleus_size"]
    assert on[2][1] > 0 and off[2][1] == 0, (on[2], off[2])


@pytest.mark.parametrize("name", ["nucleus past 1024", "64 lanes"])
def test_pushed_products(monkeypatch, name):
    """MLP_DETERMINISTIC=0 keeps the F product on the push: float atomics, so not bitwise — the oracle's pivots and objective all the same."""
    _medium(monkeypatch)
    monkeypatch.setenv("MLP_DETERMINISTIC", "0")
    lp, kw, trace, obj = _instance(name)
    s = lpgen.build_problem(M.Problem, lp).solve(**kw)
    st = s.stats()
    print(f"{name}, pushed: v_ride {s.state('v_ride').tolist()}, {st['iterations']} pivots, nucleus {st['nucleus_size']}, max_pivot_err {st['max_pivot_err']:.2e}")
    assert [t[:5] for t in s.trace()] == trace
    assert obj_close(s.objective(), obj)
    assert st["max_pivot_err"] < REFRESH_TOL, st["max_pivot_err"]
    assert s.state("v_ride")[1] > 0


def test_bound_flips(monkeypatch):
    """An upper bound of 0.2 on every second variable (tests/test_ratio_onepass.py): some iterations end in a bound flip — their riders have
    run and left only scratch behind."""
    _medium(monkeypatch)
    lp, kw, trace, obj = _instance("two blocks", hi=0.2)
    on, off = _on_off(monkeypatch, lp, kw)
    print(f"bounded: {on[3]['iterations']} pivots, {on[3]['bound_flips']} flips, v_ride on {on[2]}, off {off[2]}")
    assert on[0] == trace and off[0] == trace
    assert obj_close(on[5], obj)
    assert on[3]["bound_flips"] > 0
    assert on[1] == off[1]
    assert on[2][1] > 0 and off[2][1] == 0, (on[2], off[2])


def test_without_the_btran_ride_there_is_no_v_ride(monkeypatch):
    _medium(monkeypatch)
    monkeypatch.setenv("MLP_BTRAN_RIDE", "0")
    lp, kw, trace, obj = _instance("two blocks")
    s = lpgen.build_problem(M.Problem, lp).solve(**kw)
    assert s.state("v_ride").tolist() == [0, 0]
    assert [t[:5] for t in s.trace()] == trace


def test_publish_wait_form(monkeypatch):
    """MLP_RATIO_LIST=0: the ratio blocks wait inside the launch for their last-arriving block; the riders come behind them in dispatch
    order, so no wait times out."""
    _medium(monkeypatch)
    monkeypatch.setenv("MLP_RATIO_LIST", "0")
    lp, kw, trace, obj = _instance("two blocks")
    on, off = _on_off(monkeypatch, lp, kw)
    assert on[0] == trace and off[0] == trace
    assert on[3]["ratio_stalls"] == 0 and off[3]["ratio_stalls"] == 0
    assert on[1] == off[1]
    assert on[2][1] > 0 and off[2][1] == 0, (on[2], off[2])


_DEGENERATE = [next(c for c in D.PRIMAL_CASES if D.family(c) == fam) for fam in ("matching", "unit_packing")]


@pytest.mark.parametrize("case", _DEGENERATE)
def test_degenerate_data(monkeypatch, case):
    """Every ratio ties: on and off take the same pivots and give the same x bit for bit."""
    _medium(monkeypatch)
    lp = D.PRIMAL_CASES[case]()
    on, off = _on_off(monkeypatch, lp, dict(trace=True))
    print(f"{case}: {on[3]['iterations']} pivots ({on[3]['primal_iters']} primal), v_ride on {on[2]}, off {off[2]}")
    assert on[0] == off[0] and on[1] == off[1]
    assert on[3]["primal_iters"] > 0
    assert off[2][1] == 0
