"""Engine::run_loop against the commit before BatchPlan (csrc/batch.h): the cases of tools/record_batches.py — graphs of
several iterations, the graph split, eager iterations, a pivot budget, the sampled iterations of profile mode, the hypersparse kernel and
its back-off, the primal head's slot room, k_small_basis, pending rank-1 terms, the compact factor and the switch to it — replayed on
the tree and compared with tests/golden/batch_plan_parent.json, which that commit wrote on the MI355X.  Every recorded field must be
equal after every call: SHA-1 of the trace, the bytes of the objective, SHA-1 of the values and of the mode-2 basis blob,
budget_exhausted, every integer counter of stats(), the bytes of its *_bytes doubles and six state() keys.  No tolerance.  The file was
merged from two recordings of that commit in two processes; a field listed under its "unstable" key is one the two disagreed on, and
only an objective / values / basis hash of a case run with MLP_DETERMINISTIC=0 (float atomics) may be listed there."""
import importlib.util
import json
import os

import pytest

from tests.common import ROOT


def _recorder():
    spec = importlib.util.spec_from_file_location("record_batches", os.path.join(ROOT, "tools", "record_batches.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


NAMES = ["graphs", "graph split", "eager", "budget", "sampled", "sampled each", "hypersparse", "back-off", "head outgrown", "head room",
         "small basis", "pending terms", "factor", "factor switch"]
FIELDS = ["basis", "budget_exhausted", "bytes", "call", "objective", "state", "stats", "trace", "values"]


def test_the_golden_file_holds_every_case():
    rec = _recorder()
    gold = json.load(open(rec.GOLDEN))
    cases, unstable = gold["cases"], [tuple(u) for u in gold["unstable"]]
    assert sorted(cases) == sorted(rec.CASES) == sorted(NAMES)
    for name, i, field in unstable:                                                      # only what float atomics may move
        assert field in ("objective", "values", "basis") and rec.CASES[name][1].get("MLP_DETERMINISTIC") == "0", (name, i, field)
    for name, calls in cases.items():
        assert len(calls) == sum(1 for what, _ in rec.CASES[name][2] if what != "sampling"), name
        for i, c in enumerate(calls):
            left_out = sorted(f for n, j, f in unstable if n == name and j == i)
            assert sorted(list(c) + left_out) == FIELDS, (name, i)
            assert len(c["trace"]) == 40 and sorted(c["state"]) == sorted(rec.STATE), (name, i)
            st = c["stats"]
            for k in ("iterations", "hyper_iters", "hyper_bails", "ratio_stalls", "factor_refactors", "factor_switches", "reinversions",
                      "final_refreshes", "beta_rebuilds", "nucleus_size", "nucleus_capacity", "iter_samples", "sweep_launches", "str_launches",
                      "fused_launches", "fold_launches", "update_launches", "ftran_launches"):
                assert isinstance(st[k], int), (name, i, k)
            assert st["ratio_stalls"] == 0, (name, i)                                    # (no case provokes a stall)
            assert {"sweep_bytes", "fused_bytes", "ftran_bytes", "fold_bytes"} <= set(c["bytes"]) and all(len(h) == 16 for h in c["bytes"].values())
    last = {name: calls[-1] for name, calls in cases.items()}
    stats = {name: c["stats"] for name, c in last.items()}
    state = {name: c["state"] for name, c in last.items()}

    g = stats["graphs"]
    assert g["iterations"] > 64 and g["iter_samples"] == 0 and not last["graphs"]["budget_exhausted"]   # (a cold solve of several full rings)
    assert last["graph split"]["trace"] == last["graphs"]["trace"] and last["eager"]["trace"] == last["graphs"]["trace"]

    b = cases["budget"]
    assert [c["stats"]["iterations"] for c in b[:3]] == [7, 47, 48] and all(c["budget_exhausted"] for c in b[:3])
    assert not b[3]["budget_exhausted"]
    for f in ("trace", "objective", "values", "basis"):
        assert b[3][f] == last["graphs"][f], f
    assert b[3]["stats"]["iterations"] == g["iterations"] and b[3]["stats"]["nucleus_size"] == g["nucleus_size"]

    sp = stats["sampled"]
    assert sp["iter_samples"] >= 2 and sp["update_launches"] == sp["iter_samples"] and sp["sweep_launches"] + sp["str_launches"] >= 1
    assert last["sampled"]["trace"] == last["graphs"]["trace"]
    e = cases["sampled each"]
    assert e[0]["stats"]["iterations"] == 0 and e[0]["budget_exhausted"]
    assert e[1]["stats"]["iter_samples"] == 25 and e[1]["stats"]["iterations"] == 25

    assert stats["hypersparse"]["hyper_iters"] > 0
    bo = stats["back-off"]
    assert bo["hyper_bails"] >= 3 and 0 < bo["hyper_iters"] < bo["iterations"]
    assert sum(state["back-off"]["hyper_bail_reasons"]) == bo["hyper_bails"]

    ho = stats["head outgrown"]
    assert 0 < state["head outgrown"]["primal_head_launches"][0] < ho["iterations"] and ho["nucleus_size"] > 62
    assert 0 < state["head room"]["primal_head_launches"][0] < stats["head room"]["primal_iters"]
    assert state["small basis"]["small_basis_launches"][0] > 0
    assert cases["pending terms"][0]["state"]["lowrank_pending"][0] > 0 and cases["pending terms"][0]["budget_exhausted"]
    assert stats["factor"]["factor_active"] == 1 and stats["factor"]["factor_refactors"] >= 2
    assert stats["factor switch"]["factor_switches"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_every_recorded_field_is_equal(name):
    rec = _recorder()
    gold = json.load(open(rec.GOLDEN))
    want = gold["cases"][name]
    got = rec.record_case(name)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        for field in sorted(w):                                                          # (a field left out as unstable is not compared)
            if isinstance(w[field], dict):
                assert sorted(g[field]) == sorted(w[field]), (name, i, field)
                for k in sorted(w[field]):
                    assert g[field][k] == w[field][k], (name, i, field, k, g[field][k], w[field][k])
            else:
                assert g[field] == w[field], (name, i, field, g[field], w[field])
        assert sorted(set(g) - set(w)) == sorted(f for n, j, f in gold["unstable"] if n == name and j == i), (name, i)
