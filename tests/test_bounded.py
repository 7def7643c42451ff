"""GPU: bounded-variable LPs with continuous data (tests/bounded_lp.py), pivot for pivot, on every forced pivot path.

The bounded ratio rule of the reference has three parts: a basic variable leaves at its lower or at its upper bound, an entering column
whose own range is shorter than every ratio flips instead of pivoting (solver.rs:782-853, 842-851), and a non-basic column may sit at an
upper bound or have no lower bound at all.  The engine restates the primal Harris pass in every iteration form (single block, grid, two
launches, the sparse list of the pushed F product, k_primal_head, the hypersparse kernel), takes the flip decision in two places and has
a flip branch in the update kernel.  Every other family the suite compares pivot for pivot has x >= 0 and no upper bound; gen_mixed_lp has
bounds but integer data and is dual-only.  `gen_bounded_lp` has narrow and wide boxes, upper-only, lower-only (of either sign) and fixed
columns on continuous data, and is solved by the dual loop on the artificial objective followed by the primal loop with steepest edge:
136 ... 1 619 pivots and 4 ... 13 bound flips per instance, 64 ... 751 of the iterations primal.  tests/test_bounded_generators.py shows
on the CPU that no decision of those sequences lies within rounding of a tie (the relabelled twin takes the same sequence), so a
diverging sequence here is a finding about a kernel.

Every (instance, path) of bounded_lp.CASES x test_degenerate.PATHS (all fourteen sets; random bases have cycles, so the two bump-only
sets run on every instance) is solved once and held to:

  1. [t[:5] for t in trace] equal to the oracle's over the whole solve, flips (row == -1) included;
  2. stats(): bound_flips and basis_changes equal to the oracle's bound_flips and pivots, primal_iters > 0 (and dual_iters > 0);
  3. the oracle's objective (obj_close), |x - x_oracle|inf <= X_ATOL, check_feasible;
  4. the host KKT check of test_degenerate.py (numpy.longdouble, from values(), dual_values(), reduced_costs() and basis_status()
     alone): every term <= 1e-7, certificate() agreeing with it to 1e-9;
  5. every non-basic column with lo < hi has x EXACTLY equal to the bound its status names (hi for MLP_AT_UPPER, upper-only columns
     included; lo for MLP_AT_LOWER); no column is MLP_NB_FREE; the statuses are those of the oracle's final basis;
  6. reinvert() < 1e-8 where the explicit inverse is kept (read last);
  7. max_pivot_err < 1e-9.

Per path set, test_the_forced_path_took_primal_and_dual_pivots asserts from stats() / state() that the forced form ran on at least one
instance (test_degenerate.ENGAGED), and for the six sets that force a primal form that it took primal pivots (PRIMAL_ENGAGED).  Two
predicates cannot hold on a two-phase solve, for reasons that lie in the host's dispatch and not in a kernel:

  * `hypersparse`: the kernel takes the dual loop WITHOUT primal steepest edge only (Engine::hyper_capable: `enable_pse` declines it), and
    a solve that starts dual infeasible keeps the primal weights up to date through its dual loop.  hyper_iters is 0 on every instance.
  * `pushed-F-head5`: k_primal_head needs the nucleus inside its slots (56, here 5); the dual loop has grown it to 60 ... 335 columns before
    the first primal iteration.  primal_head_launches is 0 with five slots; with all 56 (`pushed-F`) the head still serves the 120 x 160
    instance, which shows that the knob is read.

Both forms are therefore held to bounded columns on the one-loop variants of the family (bounded_lp.primal_start: primal from the
slack basis, nucleus growing from zero; bounded_lp.dual_start: dual feasible start, dual loop on the real objective), with the same
seven assertions: test_primal_start_* on the six primal sets — PRIMAL_ENGAGED must hold on every pair there, the head-5 hand-over
included — and test_dual_start_* on default, hypersparse (hyper_iters > 0) and hypersparse with MLP_HYPER_HEAVY=2 (the kernel hands
iterations back: hyper_bails >= 3).  The relabelling check covers those four instances too.

Warm starts at an optimum with columns at upper bounds (300 x 260; default, grid-forms, large-nucleus-J3, factor, and hypersparse, whose
re-solves are dual loops without primal steepest edge: hyper_iters > 0 there): fix_var of a basic boxed column at the midpoint of its
range, unfix_var, add_constraint of a '<=' row over two columns non-basic at upper and two basic ones; objective and x against the
oracle after every step."""
import numpy as np
import pytest

import minilp_amd as M
from minilp_amd import lpgen
from oracle import minilp_oracle as O
from tests import bounded_lp as B
from tests.common import X_ATOL, check_feasible, obj_close
from tests.test_degenerate import ATOL, CERT, ENGAGED, KKT_TOL, PATHS, PRIMAL_ENGAGED, PRIMAL_PATHS, TERMS, _setenv, host_kkt

pytestmark = pytest.mark.gpu

CASES = {B.case_id(c): c for c in B.CASES}
PRIMAL_START = {B.case_id(c): c for c in B.PRIMAL_START_CASES}
DUAL_START = {B.case_id(c): c for c in B.DUAL_START_CASES}
EVERY_CASE = {**CASES, **PRIMAL_START, **DUAL_START}
# the sets of the dual-start variant: the hypersparse kernel, and the kernel handing every iteration back whose eta update touches more
# than two entries (tests/test_hyper.py)
DUAL_PATHS = {"default": PATHS["default"], "hypersparse": PATHS["hypersparse"], "hypersparse-hand-over": dict(MLP_HYPER="1", MLP_HYPER_HEAVY="2")}
EVERY_PATH = {**PATHS, **DUAL_PATHS}
STATE = ("dual_list_tests", "lowrank_pending", "fpull", "factor_sb", "primal_head_launches", "small_basis_launches")
COUNTERS = ("hyper_iters", "hyper_bails", "str_launches", "banded_sweep", "nucleus_size", "factor_active", "factor_refactors", "factor_bump_max")

# ------------------------------------------------------------------------------------------------ one solve per pair, everything read once
_RUNS = {}


def collect(lp, budget):
    """Solve with the environment as it is and read everything the assertions need (the Solution is dropped)."""
    s = lpgen.build_problem(M.Problem, lp).solve(budget=budget, trace=True)
    st = s.stats()
    x = s.values()
    vstat, cstat = s.basis_status()
    rec = dict(objective=s.objective(), x=x, exhausted=s.budget_exhausted, stats=st, trace=s.trace(), vstat=vstat,
               kkt=host_kkt(lp, x, s.dual_values(), s.reduced_costs(), vstat, cstat), cert=s.certificate(),
               state={k: s.state(k).tolist() for k in STATE})
    rec["reinvert"] = s.reinvert() if st["factor_active"] == 0 else None     # (last: it replaces the inverse)
    return rec


def run(monkeypatch, case, path):
    if (case, path) not in _RUNS:
        ref = B.reference(EVERY_CASE[case])
        with monkeypatch.context() as mp:
            mp.delenv("MLP_HYPER_HEAVY", raising=False)
            _setenv(mp, EVERY_PATH[path])
            _RUNS[case, path] = collect(ref["lp"], 4 * len(ref["trace"]))     # (the budget only ends a stall; the sequence is compared)
    return _RUNS[case, path]


def _head(rec):
    return int(rec["state"]["primal_head_launches"][0])


def check(case, path, rec):
    """The seven assertions of the module docstring on the record of one finished solve."""
    ref = B.reference(EVERY_CASE[case])
    lp, so = ref["lp"], ref["stats"]
    st, x, k, vstat = rec["stats"], rec["x"], rec["kkt"], rec["vstat"]
    dx = float(np.abs(x - ref["x"]).max())
    print(f"{case} [{path}]: pivots {st['basis_changes']} (oracle {so['pivots']}), flips {st['bound_flips']} (oracle {so['bound_flips']}), "
          f"primal / dual {st['primal_iters']} / {st['dual_iters']} (oracle {so['primal_iters']} / {so['dual_iters']}); objective "
          f"{rec['objective']!r} (oracle {ref['objective']!r}), |dx| {dx:.2e}; KKT " + ", ".join(f"{t} {float(k[t]):.2e}" for t in TERMS) +
          f"; reinvert {rec['reinvert']}, max_pivot_err {st['max_pivot_err']:.2e}; " + ", ".join(f"{c} {st[c]}" for c in COUNTERS) + "; " +
          ", ".join(f"{s} {rec['state'][s]}" for s in STATE))
    assert not rec["exhausted"], (st["iterations"], len(ref["trace"]))
    # 1. the oracle's sequence, flips included
    a, b = [t[:5] for t in rec["trace"]], [t[:5] for t in ref["trace"]]
    i = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
    assert a == b, (i, len(a), len(b), rec["trace"][i:i + 1], ref["trace"][i:i + 1])
    # 2. the counters
    assert st["bound_flips"] == so["bound_flips"] and st["basis_changes"] == so["pivots"], (st["bound_flips"], st["basis_changes"])
    assert (st["primal_iters"] > 0) == (so["primal_iters"] > 0) and (st["dual_iters"] > 0) == (so["dual_iters"] > 0)
    # 3. objective, x, feasibility
    assert obj_close(rec["objective"], ref["objective"]), (rec["objective"], ref["objective"])
    assert dx <= X_ATOL, dx
    check_feasible(lp, x)
    # 4. host KKT, and the device certificate against it
    for t in TERMS:
        assert float(k[t]) <= KKT_TOL, (t, float(k[t]))
    for name, t in CERT:
        assert abs(rec["cert"][name] - float(k[t])) <= ATOL, (name, rec["cert"][name], float(k[t]))
    # 5. a non-basic column is exactly at the bound its status names
    ranged = lp["lo"] < lp["hi"]
    at_lo, at_up = ranged & (vstat == M.MLP_AT_LOWER), ranged & (vstat == M.MLP_AT_UPPER)
    assert not (vstat == M.MLP_NB_FREE).any() and not (ranged & (vstat == M.MLP_NB_FIXED)).any()
    assert np.isfinite(lp["lo"][at_lo]).all() and np.isfinite(lp["hi"][at_up]).all()
    assert (x[at_lo] == lp["lo"][at_lo]).all(), np.flatnonzero(at_lo)[x[at_lo] != lp["lo"][at_lo]][:5]
    assert (x[at_up] == lp["hi"][at_up]).all(), np.flatnonzero(at_up)[x[at_up] != lp["hi"][at_up]][:5]
    assert np.array_equal(at_up, ref["nb_upper"] & ranged) and np.array_equal(at_lo, ref["nb_lower"] & ranged)   # (the oracle's final basis)
    assert (at_up & (ref["kinds"] == B.UPPER_ONLY)).any() and (at_lo & (lp["lo"] < 0)).any()
    # 6. the incremental inverse against a fresh one
    if "MLP_FACTOR" not in EVERY_PATH[path]:
        assert st["factor_active"] == 0
    if st["factor_active"] == 0:
        assert rec["reinvert"] < 1e-8, rec["reinvert"]
    # 7. every pivot element against its recomputation
    assert st["max_pivot_err"] < 1e-9, st["max_pivot_err"]


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("case", list(CASES))
def test_bounded_instance_on_a_forced_path(monkeypatch, case, path):
    rec = run(monkeypatch, case, path)
    check(case, path, rec)
    assert rec["stats"]["primal_iters"] > 0 and rec["stats"]["dual_iters"] > 0 and rec["stats"]["bound_flips"] >= 4


@pytest.mark.parametrize("path", list(PATHS))
def test_the_forced_path_took_primal_and_dual_pivots(monkeypatch, path):
    """A knob that no longer engages would otherwise go unnoticed: on at least one instance the counters of the forced form must move,
    in a solve that took dual pivots, primal pivots and bound flips; for the sets that force a primal form, the primal counters too."""
    recs = {case: run(monkeypatch, case, path) for case in CASES}
    mixed = [c for c, r in recs.items() if r["stats"]["primal_iters"] > 0 and r["stats"]["dual_iters"] > 0 and r["stats"]["bound_flips"] > 0]
    assert len(mixed) == len(CASES)
    if path == "hypersparse":
        # the kernel is the dual loop without primal steepest edge; these solves start dual infeasible, so their dual loop keeps the primal
        # weights (Engine::hyper_capable declines on enable_pse) and ENGAGED cannot hold: hyper_iters stays 0 and the solve is the default
        # one.  The kernel itself runs on bounded columns in test_dual_start_* and in the warm starts below (hyper_iters > 0 there).
        assert all(r["stats"]["hyper_iters"] == 0 and r["stats"]["hyper_bails"] == 0 for r in recs.values())
        return
    hit = [c for c in mixed if ENGAGED[path](recs[c])]
    print(path, "engaged on", hit)
    assert hit, path
    if path == "pushed-F-head5":
        # k_primal_head needs the nucleus inside its slots for a whole batch (Engine::run_loop), and the dual loop of a two-phase solve
        # has grown it past five before the first primal iteration: PRIMAL_ENGAGED (0 < launches < iterations) cannot hold.  What shows
        # that the five slots were in force: primal_head_launches is 0 on every instance, while `pushed-F` (56 slots) still serves the
        # smallest one through the head.  The hand-over itself is held to bounded columns in test_primal_start_*.
        assert all(_head(r) == 0 and r["stats"]["primal_iters"] > 0 for r in recs.values())
        assert any(_head(run(monkeypatch, c, "pushed-F")) > 0 for c in CASES)
        return
    if path in PRIMAL_PATHS:
        primal = [c for c in mixed if PRIMAL_ENGAGED[path](recs[c]["stats"], _head(recs[c]), recs[c]["state"]["fpull"])]
        print(path, "primal form engaged on", primal)
        assert primal, path


# ------------------------------------------------------------------------------------------------ the one-loop variants
@pytest.mark.parametrize("path", PRIMAL_PATHS)
@pytest.mark.parametrize("case", list(PRIMAL_START))
def test_primal_start_on_a_primal_path(monkeypatch, case, path):
    """Primal loop from the slack basis: the nucleus grows from zero, so k_primal_head serves the first pivots of the pushed-F sets and
    hands over when its slots (56; five with MLP_PRIMAL_HEAD_K=5) run out — with boxed, upper-only and fixed columns and bound flips."""
    rec = run(monkeypatch, case, path)
    check(case, path, rec)
    st = rec["stats"]
    assert st["dual_iters"] == 0 and st["primal_iters"] > 0 and st["bound_flips"] >= 4
    assert PRIMAL_ENGAGED[path](st, _head(rec), rec["state"]["fpull"]), (path, _head(rec), rec["state"]["fpull"], st["iterations"], st["banded_sweep"])


@pytest.mark.parametrize("path", list(DUAL_PATHS))
@pytest.mark.parametrize("case", list(DUAL_START))
def test_dual_start_on_the_hypersparse_kernel(monkeypatch, case, path):
    """Dual loop on the real objective without primal steepest edge: the loop the hypersparse kernel takes, over columns at upper bounds,
    with negative lower bounds and without a lower bound; with MLP_HYPER_HEAVY=2 the kernel hands iterations back and takes over again."""
    rec = run(monkeypatch, case, path)
    check(case, path, rec)
    st = rec["stats"]
    assert st["primal_iters"] == 0 and st["dual_iters"] > 0
    if path == "hypersparse":
        assert st["hyper_iters"] > 0, (st["hyper_iters"], st["hyper_bails"], st["iterations"])
    if path == "hypersparse-hand-over":
        assert st["hyper_bails"] >= 3 and 0 < st["hyper_iters"] < st["iterations"], (st["hyper_iters"], st["hyper_bails"], st["iterations"])


# ------------------------------------------------------------------------------------------------ warm starts at an optimum with columns at upper
WARM_CASE = (300, 260, 8, 6)
WARM = ("default", "grid-forms", "large-nucleus-J3", "factor", "hypersparse")


def _same(sg, so, what):
    xg, xo = sg.values(), so.values()
    assert np.isfinite(xo).all() and np.isfinite(so.objective())
    assert obj_close(sg.objective(), so.objective()), (what, sg.objective(), so.objective())
    assert np.abs(xg - xo).max() <= X_ATOL, (what, float(np.abs(xg - xo).max()))
    return xo


@pytest.mark.parametrize("path", WARM)
def test_warm_starts_at_an_optimum_with_columns_at_upper(monkeypatch, path):
    ref = B.reference(WARM_CASE)
    lp, kinds = ref["lp"], ref["kinds"]
    lo, hi = lp["lo"], lp["hi"]
    _setenv(monkeypatch, PATHS[path])
    sg = lpgen.build_problem(M.Problem, lp).solve()
    so = lpgen.build_problem(O.Problem, lp).solve()
    x = _same(sg, so, "root")
    root = so.objective()
    vstat, _ = sg.basis_status()
    assert np.array_equal(vstat == M.MLP_AT_UPPER, ref["nb_upper"] & (lo < hi))
    hyper0 = sg.stats()["hyper_iters"]
    # a basic boxed column to the midpoint of its range, and back
    j = int(np.flatnonzero((vstat == M.MLP_BASIC) & (kinds == B.WIDE))[0])
    mid = 0.5 * (lo[j] + hi[j])
    assert lo[j] < x[j] < hi[j] and abs(x[j] - mid) > 1e-3
    sg, so = sg.fix_var(j, mid), so.fix_var(j, mid)
    xf = _same(sg, so, "fix_var")
    assert abs(xf[j] - mid) <= X_ATOL and so.objective() > root
    (sg, wg), (so, wo) = sg.unfix_var(j), so.unfix_var(j)
    assert wg and wo
    x = _same(sg, so, "unfix_var")
    assert obj_close(sg.objective(), root)
    # a '<=' row over two columns non-basic at upper and two basic ones that cuts the optimum off
    up = [int(v) for v in np.flatnonzero(ref["nb_upper"] & np.isin(kinds, (B.WIDE, B.UPPER_ONLY)))[:2]]
    bas = [int(v) for v in np.flatnonzero((vstat == M.MLP_BASIC) & (kinds == B.NONNEG))[:2]]
    cols, coef = up + bas, [1.0, 2.0, 3.0, 1.0]
    assert len(cols) == 4 and (x[up] == hi[up]).all()
    val = float(np.dot(coef, x[cols]))
    rhs = 0.9 * val + 0.01
    assert rhs < val - 1e-3                                   # (precondition: the row is violated at the optimum)
    expr = list(zip(cols, coef))
    sg, so = sg.add_constraint(expr, M.LE, rhs), so.add_constraint(expr, O.LE, rhs)
    x = _same(sg, so, "add_constraint")
    check_feasible(lp, sg.values())
    assert float(np.dot(coef, sg.values()[cols])) <= rhs + 1e-7 and so.objective() > root
    st = sg.stats()
    print(f"[{path}] root {root!r}; x[{j}] fixed at {mid:.6g} and released; row over {cols} <= {rhs:.6g}: objective {sg.objective()!r} "
          f"(oracle {so.objective()!r}); pivots {st['basis_changes']}, flips {st['bound_flips']}, primal / dual {st['primal_iters']} / {st['dual_iters']}, "
          f"hypersparse {st['hyper_iters']}")
    if path == "factor":
        assert st["factor_active"] == 1
    if path == "large-nucleus-J3":
        assert int(sg.state("lowrank_pending")[1]) == 3 and st["banded_sweep"] == 1
    if path == "hypersparse":
        assert hyper0 == 0 and st["hyper_iters"] > 0          # (the cold solve declines the kernel, the dual re-solves run on it)
