"""The C boundary against the commit before it was consolidated: every mlp_solution_* entry point of §7.1 - §7.9 replayed by
tools/record_boundary.py — valid, n == 0 and one fault at a time, on a solved model, a model that is not solved and a one-rank pump, of
a Minimize and a Maximize instance — and compared with tests/golden/boundary_parent.json, which that commit wrote on the MI355X (two
runs of it agreed in every field, so none is left out).  Every recorded field must be equal: status, error text, whether the handle was
consumed, the integer outputs, the integer fields and `bytes` of the eight reports, the bits of the objective.  No tolerance."""
import importlib.util
import json
import os

import pytest

from tests.common import ROOT


def _recorder():
    spec = importlib.util.spec_from_file_location("record_boundary", os.path.join(ROOT, "tools", "record_boundary.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_golden_file_holds_every_case_and_call():
    rec = _recorder()
    gold = json.load(open(rec.GOLDEN))
    assert sorted(gold) == sorted(rec.CASES) and len(rec.CASES) == 6
    calls = rec.call_names()
    assert len(calls) == len(set(calls)) >= 200
    for name, case in gold.items():
        assert sorted(case) == sorted(calls), name
        for call, r in case.items():
            assert ("error" in r) == (r["status"] < 0), (name, call)
            assert ("objective" in r) == ("reports" in r) and len(r.get("objective", "0" * 16)) == 16, (name, call)
            if call.endswith(rec.NULL_HANDLE):
                assert r["status"] == -1 and r["error"].startswith("NULL solution") and not r.get("reports"), (name, call)   # (the live handle's reports stay)
            elif "consumed" in r:                                                        # a mutator: any failure frees the solution
                assert r["consumed"] == (r["status"] != 0) == ("reports" not in r), (name, call)
            else:                                                                        # a read frees nothing
                assert "reports" in r, (name, call)
        # n == 0 is a successful no-op, also on a model that is not solved (on the pump the reads refuse the handle before they look at n)
        empty = {call: r for call, r in case.items() if call.endswith(": n == 0") and ("consumed" in r or not name.endswith("/pump"))}
        assert len(empty) >= 6 and all(r["status"] == 0 for r in empty.values()), name
    assert gold["cover/not-solved"]["set_var_bounds: valid"]["error"] == "set_var_bounds: model not solved"
    assert gold["sparse-maximize/solved"]["cutoff_bounds: valid, pruned"]["outputs"]["flag"] == 1
    assert gold["cover/pump"]["cutoff_bounds: valid"]["error"] == "cutoff_bounds is not available on a sharded solution"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cover/solved", "cover/not-solved", "cover/pump", "sparse-maximize/solved", "sparse-maximize/not-solved",
                                  "sparse-maximize/pump"])
def test_every_recorded_field_is_equal(name):
    rec = _recorder()
    assert name in rec.CASES
    gold = json.load(open(rec.GOLDEN))[name]
    got = json.loads(json.dumps(rec.record_case(name)))
    assert sorted(got) == sorted(gold)
    for call in sorted(gold):
        assert got[call] == gold[call], (name, call, got[call], gold[call])
