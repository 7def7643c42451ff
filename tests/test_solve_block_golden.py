"""The calls that run dense right-hand sides through the tableau solve against the commit before Engine::SolveBlock and
Engine::warm_resolve: set_rhs, rhs_scenarios, basis_solve, the dense and sparse tableau reads, both rangings,
branch_penalties, dual_values, add_constraints and fix_var replayed by tools/record_solve_block.py on the three representations of
B^-1 — default inverse, pending rank-1 terms, compact factor — at 1, 16 and 17 entries, and compared with
tests/golden/solve_block_parent.json, which that commit wrote on the MI355X (two runs of it agreed in every field, so none is left
out).  Every recorded field must be equal: the bytes of the objective, SHA-1 of the values, of the mode-2 basis blob and of every
array a read returns, the integer counters and the `bytes` of the info struct.  No tolerance: the claim is bit identity."""
import importlib.util
import json
import os

import pytest

from tests.common import ROOT


def _recorder():
    spec = importlib.util.spec_from_file_location("record_solve_block", os.path.join(ROOT, "tools", "record_solve_block.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_golden_file_holds_every_case_and_call():
    rec = _recorder()
    gold = json.load(open(rec.GOLDEN))
    assert sorted(gold) == sorted(rec.CASES) == ["compact-factor", "mixed", "pending-terms"] and rec.LENGTHS == (1, 16, 17)
    for name, case in gold.items():
        assert sorted(case) == sorted(rec.MUTATORS + rec.READS), name
        for call in rec.MUTATORS:                                                        # no call ended Infeasible: every state is recorded
            r = case[call]
            assert sorted(set(r) - {"kind", "var"}) == ["basis", "info", "objective", "values"] and len(r["objective"]) == 16 and r["info"], (name, call)
            assert call.startswith("fix_var") or len(r["info"]["bytes"]) == 16, (name, call)
        for call in rec.READS:
            r = case[call]
            assert sorted(r) == ["info", "out"] and r["out"] and all(len(h) == 40 for h in r["out"].values()), (name, call)
            assert call == "basis_head" or ("bytes" in r["info"] and len(r["info"]) >= 4), (name, call)
        for k in rec.LENGTHS:
            batches = (k + 15) // 16
            inside, again, current = (case["set_rhs %s %d" % (w, k)]["info"] for w in ("inside", "re-solve", "current"))
            assert inside["changed"] == k and inside["solves"] == 1 and inside["pivots"] == 0, (name, k)
            assert again["changed"] == k and again["solves"] == 1 and again["pivots"] >= 1, (name, k)
            assert current["requests"] == k and current["changed"] == current["solves"] == current["pivots"] == 0, (name, k)
            sc = case["rhs_scenarios %d" % k]["info"]
            assert sc["scenarios"] == sc["solves"] == k and sc["batches"] == batches, (name, k)
            for call in ("basis_solve", "basis_solve transposed", "binv_rows", "binv_cols", "tableau_cols", "tableau_rows", "rhs_ranging", "cost_ranging"):
                info = case["%s %d" % (call, k)]["info"]
                assert info["solves"] == k and info["batches"] == batches, (name, call, k)   # the 17th request opens a second batch
            assert case["branch_penalties %d" % k]["info"]["requests"] == k, (name, k)
        assert case["branch_penalties 17"]["info"]["solves"] >= 16, name
        assert case["add_constraints of two general rows"]["info"]["rows"] == 2 and case["add_constraints of two general rows"]["info"]["pivots"] >= 1, name
        assert case["fix_var basic"]["info"]["dual_iters"] >= 1, name
        assert case["dual_values"]["info"]["max_row_violation_at"] >= 0, name              # a row -> constraint look-up did run


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed", "pending-terms", "compact-factor"])
def test_every_recorded_field_is_equal(name):
    rec = _recorder()
    assert name in rec.CASES
    gold = json.load(open(rec.GOLDEN))[name]
    got = rec.record_case(name)
    assert sorted(got) == sorted(gold)
    for call in sorted(gold):
        assert got[call] == gold[call], (name, call, got[call], gold[call])
