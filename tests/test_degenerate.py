"""GPU: degenerate integer-data LPs (tests/degenerate_lp.py) on every forced pivot path.

Every family the suite compares pivot for pivot has continuous random data: no ratio test ties, no step has length zero, no entry cancels
to exactly 0.  The instances here are nothing but ties (0/1 matrices, small integer costs and right-hand sides): assignment, transport
with unit gains, covering with unit costs, the degree LP of a TSP.  The Harris pass-2 tie-break differs from the reference's by design
(DESIGN.md §8), so no pivot sequence is compared; what every (instance, path) is held to instead:

  1. status and objective against the oracle (1e-9 relative); on the totally unimodular families the exact integer as well
     (linear_sum_assignment / round(HiGHS), 1e-9 absolute);
  2. scipy's HiGHS, live, to HIGHS_RTOL;
  3. integrality of x (assignment, unit_transport: |x - round x| <= 1e-9; two_matching: |2x - round 2x| <= 1e-9; expected exactly 0);
  4. a host KKT check in numpy.longdouble against the generator's own CSR that uses values(), dual_values(), reduced_costs() and
     basis_status() and nothing else of the engine: every term <= 1e-7, and certificate() agrees with the host's numbers to 1e-9;
  5. termination inside a pivot budget B (below);
  6. reinvert() < 1e-8 on the paths that keep an explicit inverse.

Forced paths (PATHS): the sets tools/fuzz_medium.py rotates and tests/test_factor.py, test_hyper.py, test_primal_head.py use.  For every
set test_the_forced_path_took_pivots asserts from stats() / state() that the path really ran on at least one instance.

These eight instances are solved by the dual simplex alone (x = 0 is dual feasible; the oracle takes 0 primal iterations on each): the
primal forms a set forces (the primal head, the pulled / pushed F product of the primal FTRAN) take none of their pivots.  Those forms
are held to degenerate data by test_primal_pivots_on_degenerate_data on the primal-start instances (matching, unit_packing), with
primal_iters, primal_head_launches and state("fpull") asserted.

Pivot budget: B = max(3, 4 x RATIO[family]) x the oracle's pivot count of the instance, RATIO the largest engine / oracle pivot ratio
over all paths.  It guards against a stall or a cycle, it is no performance claim.  RATIO stands at 1.0 for every family, so B is
4 x the oracle's count (assignment 62 / 273 pivots, unit_transport 89 / 642, unit_cover 87 / 832, two_matching 44 / 109): every
(instance, path) terminates inside it on the MI355X, i.e. no ratio exceeds 4.  Every test prints its pivot count, ratio, integrality and
KKT maxima.  A path that needs more than 10 x the oracle's pivots is a finding to explain, not a reason to raise B.

At these sizes (n <= 16 384) the Harris tests run in their single-block form unless MLP_RATIO_ONE=0 says otherwise, so what
MLP_RATIO_TWO_KERNELS=1 alone changes here is that k_small_basis is declined; the two-launch form itself runs in the sets with
MLP_RATIO_ONE=0 only when the grid is not co-resident.
"""
import math

import numpy as np
import pytest

import minilp_amd as M
from minilp_amd import lpgen
from oracle import minilp_oracle as O
from tests import degenerate_lp as D
from tests.common import HIGHS_RTOL, check_feasible, obj_close

pytestmark = pytest.mark.gpu

ATOL = 1e-9
KKT_TOL = 1e-7
LD = np.longdouble

_BIG = dict(MLP_BIGTILE="1", MLP_STR_K="0", MLP_RATIO_ONE="0", MLP_HYPER="0")
PATHS = {
    "default": {},
    "hypersparse": dict(MLP_HYPER="1"),
    "grid-forms": dict(MLP_HYPER="0", MLP_STR_K="0", MLP_RATIO_ONE="0"),
    "ratio-two-kernels": dict(MLP_RATIO_TWO_KERNELS="1"),
    "ratio-two-kernels-grid": dict(MLP_RATIO_TWO_KERNELS="1", MLP_RATIO_ONE="0", MLP_HYPER="0"),   # the two-launch Harris tests themselves
    "pushed-F": dict(MLP_DETERMINISTIC="0", MLP_HYPER="0"),
    "pushed-F-head5": dict(MLP_DETERMINISTIC="0", MLP_HYPER="0", MLP_PRIMAL_HEAD_K="5"),
    "large-nucleus-J3": dict(_BIG, MLP_LOWRANK="3", MLP_LDPAD="16", MLP_BANDED="1"),
    "large-nucleus-J3-push": dict(_BIG, MLP_LOWRANK="3", MLP_LDPAD="16", MLP_BANDED="1", MLP_FPULL="0"),
    "large-nucleus-J16-eager": dict(_BIG, MLP_LOWRANK="16", MLP_NO_GRAPH="1"),
    "banded-order": dict(MLP_BANDED="1", MLP_ORDER_FROM="0", MLP_ORDER_EVERY="5"),
    "factor": dict(MLP_FACTOR="1"),
    "factor-sparse-bump": dict(MLP_FACTOR="1", MLP_FACTOR_SB_FROM="2"),
    "factor-dense-bump": dict(MLP_FACTOR="1", MLP_FACTOR_SB="0"),
}
BUMP_ONLY = ("factor-sparse-bump", "factor-dense-bump")       # on the families whose bases have cycles: cover and two_matching
KNOBS = sorted({k for env in PATHS.values() for k in env})
# (MLP_FACTOR_FUSE, MLP_FACTOR_RHO_PART and MLP_PB_DET are read once per Solution like every knob; they are not varied here)

# largest measured engine / oracle pivot ratio per family (module docstring)
RATIO = {"assignment": 1.0, "unit_transport": 1.0, "unit_cover": 1.0, "two_matching": 1.0}


def _pairs():
    return [(c, p) for c in D.CASES for p in PATHS if p not in BUMP_ONLY or D.family(c) in ("unit_cover", "two_matching")]


def _setenv(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


reference = D.reference      # instance, oracle optimum and pivot count, HiGHS, exact integer: computed once, preconditions asserted


def budget(case):
    ref = reference(case)
    return int(math.ceil(max(3.0, 4.0 * RATIO[ref["family"]]) * ref["pivots"]))


# ------------------------------------------------------------------------------------------------ host KKT check (nothing of the engine)
def host_kkt(lp, x, pi, r, vstat, cstat):
    """Every KKT term of (x, pi, r, statuses) for a Minimize instance in numpy.longdouble, from the instance's CSR alone."""
    assert lp["direction"] == lpgen.MINIMIZE
    m, n = lp["m"], lp["n"]
    ip, ix, ops = lp["indptr"], lp["indices"], lp["ops"]
    a, c, b, lo, hi = (np.asarray(lp[k]).astype(LD) for k in ("data", "obj", "rhs", "lo", "hi"))
    x, pi, r = np.asarray(x).astype(LD), np.asarray(pi).astype(LD), np.asarray(r).astype(LD)
    rowof = np.repeat(np.arange(m), np.diff(ip))
    act = np.zeros(m, dtype=LD)
    np.add.at(act, rowof, a * x[ix])
    s = b - act                                                # slack: '<=' in [0, inf), '>=' in (-inf, 0], '=' fixed at 0
    le, ge, eq = ops == lpgen.LE, ops == lpgen.GE, ops == lpgen.EQ
    zero = LD(0)
    row_viol = np.where(le, -s, np.where(ge, s, np.abs(s))).max(initial=zero)
    bound_viol = np.maximum(lo - x, x - hi).max(initial=zero)
    aty = np.zeros(n, dtype=LD)
    np.add.at(aty, ix, a * pi[rowof])
    r_host = c - aty
    vb, cb = vstat == M.MLP_BASIC, cstat == M.MLP_BASIC
    # reduced costs: a basic variable reports exactly 0 and c - A^T pi vanishes there; a non-basic one reports c - A^T pi
    rc_err = max(np.abs(r_host[vb]).max(initial=zero), np.abs(r[~vb] - r_host[~vb]).max(initial=zero), np.abs(r[vb]).max(initial=zero),
                 np.abs(pi[cb]).max(initial=zero))
    # status: a non-basic variable sits at the bound its status names; a non-basic slack has the status of its operator
    at_lo, at_up, fx, fr = (vstat == k for k in (M.MLP_AT_LOWER, M.MLP_AT_UPPER, M.MLP_NB_FIXED, M.MLP_NB_FREE))
    assert (vb | at_lo | at_up | fx | fr).all()
    with np.errstate(invalid="ignore"):
        status_err = max(np.abs(x - lo)[at_lo | fx].max(initial=zero), np.abs(x - hi)[at_up | fx].max(initial=zero))
    want = np.where(le, M.MLP_AT_LOWER, np.where(ge, M.MLP_AT_UPPER, M.MLP_NB_FIXED))
    assert (cb | (cstat == want)).all(), np.flatnonzero(~(cb | (cstat == want)))[:5]
    # signs by status (minimisation): at lower r >= 0, at upper r <= 0, free r = 0; '<=' rows pi <= 0, '>=' rows pi >= 0
    sign_viol = max((-r)[at_lo].max(initial=zero), r[at_up].max(initial=zero), np.abs(r)[fr].max(initial=zero),
                    pi[le].max(initial=zero), (-pi)[ge].max(initial=zero))
    # complementary slackness
    with np.errstate(invalid="ignore"):
        gap_lo = np.where(np.isfinite(lo), x - lo, zero)
        gap_hi = np.where(np.isfinite(hi), hi - x, zero)
    cs = max((np.maximum(r, zero) * gap_lo).max(initial=zero), (np.maximum(-r, zero) * gap_hi).max(initial=zero), (np.abs(pi) * np.abs(s)).max(initial=zero))

    def lagrangian(rc, l_lo, l_hi, val):
        """sum rc_j l_j with l_j the bound that minimises rc_j x_j; an infinite one takes the current value and |rc_j| counts as dual
        infeasibility (the definition of include/minilp_hip.h)."""
        ell = np.where(rc > 0, l_lo, np.where(rc < 0, l_hi, zero))
        inf = np.isinf(ell)
        ell = np.where(inf, val, ell)
        return (rc * ell)[rc != 0].sum(), np.abs(rc)[inf & (rc != 0)].max(initial=zero)

    INF = LD(np.inf)
    t1, i1 = lagrangian(r, lo, hi, x)
    t2, i2 = lagrangian(-pi, np.where(ge, -INF, zero), np.where(le, INF, zero), s)
    primal = (c * x).sum()
    dual = (b * pi).sum() + t1 + t2
    gap = abs(primal - dual) / max(LD(1), abs(primal))
    return dict(row_viol=max(row_viol, zero), bound_viol=max(bound_viol, zero), rc_err=rc_err, status_err=status_err, sign_viol=max(sign_viol, zero),
                comp_slack=cs, gap=gap, primal=primal, dual=dual, dual_inf=max(i1, i2))


TERMS = ("row_viol", "bound_viol", "rc_err", "status_err", "sign_viol", "comp_slack", "gap", "dual_inf")
CERT = (("primal_objective", "primal"), ("dual_objective", "dual"), ("relative_gap", "gap"), ("max_row_violation", "row_viol"),
        ("max_bound_violation", "bound_viol"), ("max_dual_infeasibility", "dual_inf"))


# ------------------------------------------------------------------------------------------------ one solve, everything read once
_RUNS = {}


def collect(lp, pivots):
    """Solve with the environment as it is and read everything the assertions need (the Solution is dropped)."""
    s = lpgen.build_problem(M.Problem, lp).solve(budget=pivots, trace=True)
    st = s.stats()
    x = s.values()
    vstat, cstat = s.basis_status()
    rec = dict(objective=s.objective(), x=x, exhausted=s.budget_exhausted, stats=st, trace=s.trace(),
               kkt=host_kkt(lp, x, s.dual_values(), s.reduced_costs(), vstat, cstat), cert=s.certificate(),
               state={k: s.state(k).tolist() for k in ("dual_list_tests", "lowrank_pending", "fpull", "factor_sb", "primal_head_launches",
                                                      "small_basis_launches")})
    rec["reinvert"] = s.reinvert() if st["factor_active"] == 0 else None     # (last: it replaces the inverse)
    return rec


def run(monkeypatch, case, path):
    if (case, path) not in _RUNS:
        ref = reference(case)
        with monkeypatch.context() as mp:
            _setenv(mp, PATHS[path])
            _RUNS[case, path] = collect(ref["lp"], budget(case))
    return _RUNS[case, path]


# ------------------------------------------------------------------------------------------------ per-solve assertions
@pytest.mark.parametrize("case,path", _pairs(), ids=lambda v: v)
def test_degenerate_instance_on_a_forced_path(monkeypatch, case, path):
    ref = reference(case)
    lp, fam = ref["lp"], ref["family"]
    rec = run(monkeypatch, case, path)
    st, x, k = rec["stats"], rec["x"], rec["kkt"]
    frac = float(np.abs(x - np.round(x)).max())
    half = float(np.abs(2 * x - np.round(2 * x)).max())
    print(f"{case} [{path}]: objective {rec['objective']!r} (oracle {ref['objective']!r}, HiGHS {ref['highs']!r}); pivots {st['iterations']} "
          f"(oracle {ref['pivots']}, ratio {st['iterations'] / ref['pivots']:.3f}, budget {budget(case)}); hypersparse {st['hyper_iters']}; "
          f"max|x - round x| {frac:.3g}, max|2x - round 2x| {half:.3g}; KKT " + ", ".join(f"{t} {float(k[t]):.2e}" for t in TERMS) +
          f"; reinvert {rec['reinvert']}; fpull {rec['state']['fpull']}, dual_list_tests {rec['state']['dual_list_tests']}, factor_sb {rec['state']['factor_sb']}")
    # 5. termination
    assert not rec["exhausted"], (st["iterations"], ref["pivots"], budget(case))
    # 1. the oracle's objective, and the exact integer
    assert obj_close(rec["objective"], ref["objective"]), (rec["objective"], ref["objective"])
    if ref["exact"] is not None:
        assert abs(rec["objective"] - ref["exact"]) <= ATOL, (rec["objective"], ref["exact"])
    # 2. HiGHS
    assert abs(rec["objective"] - ref["highs"]) <= HIGHS_RTOL * max(1.0, abs(ref["highs"]))
    # 3. integrality
    if fam in ("assignment", "unit_transport"):
        assert frac <= ATOL, frac
    if fam == "two_matching":
        assert half <= ATOL, half
    # 4. host KKT, and the device certificate against it
    check_feasible(lp, x)
    for t in TERMS:
        assert float(k[t]) <= KKT_TOL, (t, float(k[t]))
    assert abs(float(k["primal"]) - rec["objective"]) <= KKT_TOL * max(1.0, abs(rec["objective"]))
    for name, t in CERT:
        assert abs(rec["cert"][name] - float(k[t])) <= ATOL, (name, rec["cert"][name], float(k[t]))
    # 6. the incremental inverse against a fresh one
    if "MLP_FACTOR" not in PATHS[path]:
        assert st["factor_active"] == 0
    if st["factor_active"] == 0:                              # (a factor path whose bump outgrew its carriers is back on the explicit inverse)
        assert rec["reinvert"] < 1e-8, rec["reinvert"]


# what shows, per forced set, that the path it forces took pivots (evaluated on the record of a finished solve)
def _sb(rec):
    return dict(zip(("in_use", "factorisations", "fallbacks", "rounds", "tail", "skipped", "failed_bump"), (int(v) for v in rec["state"]["factor_sb"])))


ENGAGED = {
    "default": lambda r: r["stats"]["iterations"] > 0,
    "hypersparse": lambda r: r["stats"]["hyper_iters"] > 0,
    "grid-forms": lambda r: r["stats"]["hyper_iters"] == 0 and r["stats"]["str_launches"] == 0 and int(r["state"]["dual_list_tests"][0]) > 0,
    "ratio-two-kernels": lambda r: r["stats"]["iterations"] > 0 and int(r["state"]["small_basis_launches"][0]) == 0,
    "ratio-two-kernels-grid": lambda r: r["stats"]["hyper_iters"] == 0 and r["stats"]["iterations"] > 0 and int(r["state"]["small_basis_launches"][0]) == 0,
    # (the primal head and the pulled / pushed F product serve the primal iteration: what these four sets force is asserted on the
    #  primal-start instances, test_primal_pivots_on_degenerate_data; here only their share in a dual-only solve)
    "pushed-F": lambda r: r["stats"]["hyper_iters"] == 0 and r["stats"]["iterations"] > 0,
    "pushed-F-head5": lambda r: r["stats"]["hyper_iters"] == 0 and r["stats"]["iterations"] > 0,
    "large-nucleus-J3": lambda r: int(r["state"]["lowrank_pending"][1]) == 3 and r["stats"]["banded_sweep"] == 1 and r["stats"]["nucleus_size"] > 3,
    "large-nucleus-J3-push": lambda r: int(r["state"]["lowrank_pending"][1]) == 3 and r["stats"]["banded_sweep"] == 1 and r["stats"]["nucleus_size"] > 3
    and int(r["state"]["fpull"][0]) == 0,
    "large-nucleus-J16-eager": lambda r: int(r["state"]["lowrank_pending"][1]) == 16 and r["stats"]["nucleus_size"] > 16,
    "banded-order": lambda r: r["stats"]["banded_sweep"] == 1 and r["stats"]["iterations"] > 0,
    "factor": lambda r: r["stats"]["factor_active"] == 1 and r["stats"]["factor_refactors"] >= 1,
    "factor-sparse-bump": lambda r: r["stats"]["factor_active"] == 1 and r["stats"]["factor_bump_max"] >= 2 and _sb(r)["factorisations"] >= 1,
    "factor-dense-bump": lambda r: r["stats"]["factor_active"] == 1 and r["stats"]["factor_bump_max"] >= 2 and _sb(r)["factorisations"] == 0,
}


@pytest.mark.parametrize("path", list(PATHS))
def test_the_forced_path_took_pivots(monkeypatch, path):
    """A knob that no longer engages would otherwise go unnoticed: on at least one instance the counters of the forced form must move."""
    hit = [case for case, p in _pairs() if p == path and ENGAGED[path](run(monkeypatch, case, path))]
    print(path, "engaged on", hit)
    assert hit, path


# ------------------------------------------------------------------------------------------------ primal pivots on degenerate data
PRIMAL_PATHS = ("default", "grid-forms", "pushed-F", "pushed-F-head5", "large-nucleus-J3", "large-nucleus-J3-push")
# what shows that the PRIMAL form a set forces took pivots: (stats, primal_head_launches, state("fpull"))
PRIMAL_ENGAGED = {
    "default": lambda st, head, fp: True,
    "grid-forms": lambda st, head, fp: st["str_launches"] == 0 and head == 0,
    "pushed-F": lambda st, head, fp: head > 0,                                   # k_primal_head serves the pushed F products only
    "pushed-F-head5": lambda st, head, fp: 0 < head < st["iterations"],          # five slots: it hands over once the nucleus outgrows them
    "large-nucleus-J3": lambda st, head, fp: head == 0 and int(fp[0]) == 1 and int(fp[1]) >= 1 and st["banded_sweep"] == 1,
    "large-nucleus-J3-push": lambda st, head, fp: head == 0 and int(fp[0]) == 0 and st["banded_sweep"] == 1,
}


@pytest.mark.parametrize("path", PRIMAL_PATHS)
@pytest.mark.parametrize("case", list(D.PRIMAL_CASES))
def test_primal_pivots_on_degenerate_data(monkeypatch, case, path):
    """The instances above are solved by the dual simplex alone, so the primal forms (k_primal_head, the pulled / pushed F product, the
    primal Harris tests, pricing over equal scores) take none of their pivots.  `matching` and `unit_packing` start primal feasible: the
    whole solve is the primal loop with steepest edge, every score and every ratio a tie at the start.  Asserted: primal pivots were
    taken, and by the form the set forces (primal_head_launches, state("fpull")); the oracle's objective (1e-9), the exact integer
    (matching), HiGHS; integrality (matching); feasibility and the device certificate (1e-7, the bound of tests/test_cut_rounds.py);
    reinvert() < 1e-8; termination inside 10 x the oracle's pivots — the ratio at which the tie-break's detours would be a finding:
    no engine / oracle ratio has been measured for these instances."""
    ref = reference(case)
    lp = ref["lp"]
    assert ref["primal_iters"] > 0                            # (precondition: the oracle's solve is a primal one)
    _setenv(monkeypatch, PATHS[path])
    s = lpgen.build_problem(M.Problem, lp).solve(budget=10 * ref["pivots"])
    st, x = s.stats(), s.values()
    head, fp = int(s.state("primal_head_launches")[0]), s.state("fpull").tolist()
    frac = float(np.abs(x - np.round(x)).max())
    cert = s.certificate()
    print(f"{case} [{path}]: objective {s.objective()!r} (oracle {ref['objective']!r}); pivots {st['iterations']} (primal {st['primal_iters']}, "
          f"oracle {ref['pivots']}, ratio {st['iterations'] / ref['pivots']:.3f}); through k_primal_head {head}; fpull {fp}; "
          f"max|x - round x| {frac:.3g}; certificate gap {cert['relative_gap']:.2e}, rows {cert['max_row_violation']:.2e}, "
          f"dual {cert['max_dual_infeasibility']:.2e}")
    assert not s.budget_exhausted, (st["iterations"], ref["pivots"])
    assert st["primal_iters"] > 0
    assert PRIMAL_ENGAGED[path](st, head, fp), (path, head, fp, st["iterations"], st["banded_sweep"], st["str_launches"])
    assert obj_close(s.objective(), ref["objective"]), (s.objective(), ref["objective"])
    assert abs(s.objective() - ref["highs"]) <= HIGHS_RTOL * max(1.0, abs(ref["highs"]))
    if ref["exact"] is not None:
        assert abs(s.objective() - ref["exact"]) <= ATOL and frac <= ATOL, (s.objective(), ref["exact"], frac)
    check_feasible(lp, x)
    assert max(abs(cert["relative_gap"]), cert["max_row_violation"], cert["max_bound_violation"], cert["max_dual_infeasibility"]) <= KKT_TOL, cert
    assert st["factor_active"] == 0 and s.reinvert() < 1e-8


# ------------------------------------------------------------------------------------------------ warm starts on a degenerate optimum
WARM = ("default", "factor", "large-nucleus-J3")


def _status(f):
    try:
        return f(), "ok"
    except (M.Infeasible, O.Infeasible):
        return None, "infeasible"


@pytest.mark.parametrize("path", WARM)
def test_branch_and_bound_dive_on_the_unit_cover(monkeypatch, path):
    """Six levels: clone, fix the most fractional variable to 0 on one clone and to 1 on the other, compare status and objective with the
    oracle doing the same, continue with the smaller objective; then unfix all six in reverse order: the root's objective again."""
    _setenv(monkeypatch, PATHS[path])
    ref = reference("unit_cover-70x90x5")
    lp = ref["lp"]
    sg = lpgen.build_problem(M.Problem, lp).solve()
    so = lpgen.build_problem(O.Problem, lp).solve()
    assert obj_close(sg.objective(), so.objective())
    root = so.objective()
    fixed = []
    for level in range(6):
        x = sg.values()
        score = np.abs(x - np.round(x))
        score[fixed] = -1.0
        j = int(np.argmax(score))
        kids = []
        for v in (0.0, 1.0):
            cg, stg = _status(lambda: sg.clone().fix_var(j, v))
            co, sto = _status(lambda: so.clone().fix_var(j, v))
            assert stg == sto, (level, j, v, stg, sto)
            if cg is not None:
                assert obj_close(cg.objective(), co.objective()), (level, j, v, cg.objective(), co.objective())
                assert cg.objective() >= sg.objective() - 1e-9 * max(1.0, abs(sg.objective()))
                kids.append((co.objective(), v, cg, co))
        assert kids, level                                  # (x_j = 1 keeps a covering LP feasible)
        obj, v, sg, so = min(kids, key=lambda t: (t[0], t[1]))
        fixed.append(j)
        print(f"[{path}] level {level}: x[{j}] = {x[j]:.6g} -> {v:g}, objective {obj!r}, pivots so far {sg.stats()['iterations']}")
    for j in reversed(fixed):
        (sg, wg), (so, wo) = sg.unfix_var(j), so.unfix_var(j)
        assert wg == wo
        assert obj_close(sg.objective(), so.objective()), (j, sg.objective(), so.objective())
    assert obj_close(sg.objective(), root) and obj_close(so.objective(), root), (sg.objective(), so.objective(), root)
    check_feasible(lp, sg.values())
    st = sg.stats()
    print(f"[{path}] back at the root: {sg.objective()!r}; primal iterations {st['primal_iters']}, dual {st['dual_iters']}")
    if path == "factor":
        assert st["factor_active"] == 1
    if path == "large-nucleus-J3":
        assert int(sg.state("lowrank_pending")[1]) == 3 and st["banded_sweep"] == 1


@pytest.mark.parametrize("path", WARM)
def test_forbidden_arcs_on_the_assignment_one_by_one_and_in_one_call(monkeypatch, path):
    """x_ij <= 0 on the optimal arc of three rows: by add_constraint three times, and by one add_constraints on a clone.  Both reach the
    oracle's objective (and the exact optimum of the assignment problem without those arcs), and x stays integral."""
    from scipy.optimize import linear_sum_assignment
    _setenv(monkeypatch, PATHS[path])
    lp = reference("assignment-24")["lp"]
    n = 24
    sg = lpgen.build_problem(M.Problem, lp).solve()
    so = lpgen.build_problem(O.Problem, lp).solve()
    x = sg.values()
    arcs = [i * n + int(np.argmax(x[i * n:(i + 1) * n])) for i in range(3)]
    assert all(abs(x[a] - 1.0) <= ATOL for a in arcs)
    C = lp["obj"].reshape(n, n).copy()
    C.reshape(-1)[arcs] = 1e6
    r, c = linear_sum_assignment(C)
    exact = float(C[r, c].sum())
    assert exact < 1e6
    batch = sg.clone().add_constraints([([(a, 1.0)], M.LE, 0.0) for a in arcs])
    for a in arcs:
        sg, so = sg.add_constraint([(a, 1.0)], M.LE, 0.0), so.add_constraint([(a, 1.0)], O.LE, 0.0)
    print(f"[{path}] objective one by one {sg.objective()!r}, in one call {batch.objective()!r}, oracle {so.objective()!r}, exact {exact!r}")
    assert abs(so.objective() - exact) <= ATOL              # (precondition: the oracle finds the exact optimum)
    for s in (sg, batch):
        assert obj_close(s.objective(), so.objective()) and abs(s.objective() - exact) <= ATOL
        xs = s.values()
        assert np.abs(xs - np.round(xs)).max() <= ATOL and np.abs(xs[arcs]).max() <= ATOL
        check_feasible(lp, xs)
    assert obj_close(sg.objective(), batch.objective())
    if path == "factor":
        assert sg.stats()["factor_active"] == 1 and batch.stats()["factor_active"] == 1


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("path", ["default", "large-nucleus-J3"])
@pytest.mark.parametrize("case", list(D.CASES))
def test_two_solves_are_identical(monkeypatch, case, path):
    """Where the repository claims reproducibility (small models, the hypersparse path, the pulled F product): the same trace, pivot
    element and objective after every pivot included, and the same bytes of values().  Arithmetic is exact on the unimodular families, so
    a difference there is a race in a tie-break."""
    a = run(monkeypatch, case, path)
    _setenv(monkeypatch, PATHS[path])
    b = collect(reference(case)["lp"], budget(case))
    assert a["trace"] == b["trace"]
    assert a["x"].tobytes() == b["x"].tobytes() and a["objective"] == b["objective"]
