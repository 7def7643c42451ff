"""GPU: a Solution reads the MLP_* environment once, when it is created, and keeps those settings for life; a clone has exactly its
parent's (csrc/settings.h).  Shown on MLP_SMALL_BASIS, whose form leaves a count behind
(state("small_basis_launches")): a solve interrupted after 20 pivots, the variable switched, then continued on the parent and on a
clone of it — neither changes form, and both end on the trace of the uninterrupted solve."""
import pytest

import minilp_amd as M
from minilp_amd import lpgen

pytestmark = pytest.mark.gpu

_FULL = {}


def _problem():
    return lpgen.build_problem(M.Problem, lpgen.gen_sparse_lp(700, 600, 12, 6))


def _count(s):
    return int(s.state("small_basis_launches")[0])


def _uninterrupted(monkeypatch, small_basis):
    """Trace and count of the whole solve under MLP_SMALL_BASIS=small_basis (solved once per value)."""
    if small_basis not in _FULL:
        monkeypatch.setenv("MLP_SMALL_BASIS", small_basis)
        s = _problem().solve(trace=True)
        _FULL[small_basis] = (s.trace(), _count(s))
    return _FULL[small_basis]


@pytest.mark.parametrize("first,then", [("0", "1"), ("1", "0")], ids=["off then on", "on then off"])
def test_a_solution_and_its_clone_keep_the_settings_of_its_creation(monkeypatch, first, then):
    monkeypatch.setenv("MLP_HYPER", "0")
    full, full_count = _uninterrupted(monkeypatch, first)
    assert len(full) > 40 and (full_count > 0) == (first == "1"), (len(full), full_count)
    monkeypatch.setenv("MLP_SMALL_BASIS", first)
    s = _problem().solve(budget=20, trace=True)
    head, at_20 = s.trace(), _count(s)
    assert len(head) == 20 and s.budget_exhausted
    monkeypatch.setenv("MLP_SMALL_BASIS", then)
    c = s.clone()
    s.continue_solve(-1)
    c.continue_solve(-1)
    print(f"MLP_SMALL_BASIS={first} then {then}: {len(full)} pivots; count at 20 pivots {at_20}, parent {_count(s)}, clone {_count(c)}, uninterrupted {full_count}")
    if first == "0":
        assert at_20 == 0 and _count(s) == 0 and _count(c) == 0
    else:
        assert at_20 > 0 and _count(s) > at_20 and _count(c) > at_20
    assert s.trace() == full
    assert head + c.trace() == full


def test_two_solutions_of_one_process_each_follow_the_environment_of_their_creation(monkeypatch):
    monkeypatch.setenv("MLP_HYPER", "0")
    counts = []
    for on in ("1", "0"):
        monkeypatch.setenv("MLP_SMALL_BASIS", on)
        counts.append(_count(_problem().solve(budget=40)))
    assert counts[0] > 0 and counts[1] == 0, counts
