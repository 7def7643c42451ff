"""The bound and fixing mutators against the commit before their kernels were merged: fix_vars, set_var_bounds,
unfix_vars and unfix_var replayed by tools/record_bound_moves.py on small instances of the bit-reproducible pull path — default inverse,
pending rank-1 terms, compact factor — and compared with tests/golden/bound_moves_parent.json, which that commit wrote on the MI355X
(two runs of it agreed in every case, so none is left out).  Every recorded field must be equal: the bytes of the objective, SHA-1 of
the values and of the mode-2 basis blob, the integer counters of the info struct.  No tolerance: the claim is bit identity."""
import importlib.util
import json
import os

import pytest

from tests.common import ROOT


def _recorder():
    spec = importlib.util.spec_from_file_location("record_bound_moves", os.path.join(ROOT, "tools", "record_bound_moves.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_golden_file_holds_every_case_and_call():
    rec = _recorder()
    gold = json.load(open(rec.GOLDEN))
    assert sorted(gold) == sorted(rec.CASES)
    calls = (["fix_vars %s %d" % (kd, k) for kd in rec.FIX_KINDS for k in rec.LENGTHS] + ["set_var_bounds mixed %d" % k for k in rec.LENGTHS] +
             ["unfix_vars of the 16 shifted", "unfix_var"])
    for name, case in gold.items():
        assert sorted(case) == sorted(calls), name
        for call, r in case.items():
            assert r == dict(infeasible=True) or (sorted(r) == ["basis", "info", "objective", "values"] and len(r["objective"]) == 16 and r["info"]), (name, call)
        assert not case["fix_vars shift 16"].get("infeasible") and case["unfix_vars of the 16 shifted"]["info"]["unfixed"] == 16, name
        assert case["fix_vars shift 17"]["info"]["shifted"] == 17 and case["fix_vars value 16"]["info"]["shifted"] == 0, name
    assert sum(1 for case in gold.values() for r in case.values() if r.get("infeasible")) <= 4      # (the long mixed lists under pending terms)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cover", "sparse-maximize", "mixed", "bounded", "pending-terms", "compact-factor"])
def test_every_recorded_field_is_equal(name):
    rec = _recorder()
    assert name in rec.CASES
    gold = json.load(open(rec.GOLDEN))[name]
    got = rec.record_case(name)
    assert sorted(got) == sorted(gold)
    for call in sorted(gold):
        assert got[call] == gold[call], (name, call, got[call], gold[call])
