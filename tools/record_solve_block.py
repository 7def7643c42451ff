"""Records what the calls that run dense right-hand sides through the tableau solve leave behind or return, bit for bit (DESIGN.md §7.4,
§7.10), on the three representations of B^-1 that tools/record_bound_moves.py builds (same generators, arguments and environment):
set_rhs, rhs_scenarios, basis_solve, binv_rows / binv_cols / tableau_cols / tableau_rows / basis_head, rhs_ranging / cost_ranging,
branch_penalties, dual_values, add_constraints of two general rows, fix_var of a basic and of a non-basic variable; lists of 1, 16 and
17 entries (below, at and across the batch of 16).

    python tools/record_solve_block.py [OUT.json]        (default: tests/golden/solve_block_parent.json)

A mutator records the bytes of objective(), SHA-1 of values() and of save_basis(2), the integer fields and `bytes` of its info struct; a
read records SHA-1 of every array it returns, the integer fields and `bytes` of its info struct.  The committed file is the output of
the commit BEFORE Engine::SolveBlock and Engine::warm_resolve; tests/test_solve_block_golden.py replays `record_case` on the current
tree and asserts equality of every field."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import minilp_amd as M                                                                   # noqa: E402


def _bound_moves():
    """tools/record_bound_moves.py: the cases are built by its own _case."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("record_bound_moves", os.path.join(ROOT, "tools", "record_bound_moves.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_case, _env, _ints = (getattr(_bound_moves(), n) for n in ("_case", "_env", "_ints"))

GOLDEN = os.path.join(ROOT, "tests", "golden", "solve_block_parent.json")
LENGTHS = (1, 16, 17)
CASES = ("mixed", "pending-terms", "compact-factor")
RESOLVE_KINDS = ("loose-beyond", "tighten", "eq+", "eq-", "mixed")                       # tests/test_rhs.py::rhs_list, tried in this order
MUTATORS = (["set_rhs %s %d" % (w, k) for w in ("inside", "re-solve", "current") for k in LENGTHS] +
            ["add_constraints of two general rows", "fix_var basic", "fix_var non-basic"])
READS = (["%s %d" % (c, k) for c in ("rhs_scenarios", "basis_solve", "basis_solve transposed", "binv_rows", "binv_cols", "tableau_cols",
                                      "tableau_rows", "rhs_ranging", "cost_ranging", "branch_penalties") for k in LENGTHS] +
         ["basis_head", "dual_values"])
STATS = ("iterations", "basis_changes", "bound_flips", "primal_iters", "dual_iters", "reinversions")   # fix_var has no info struct of its own


def _info(info):
    out = _ints(info)
    if "bytes" in info:
        out["bytes"] = np.float64(info["bytes"]).tobytes().hex()
    return out


def _sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def _state(s, info):
    return dict(objective=np.float64(s.objective()).tobytes().hex(), values=_sha(s.values()), basis=hashlib.sha1(bytes(s.save_basis(2))).hexdigest(),
                info=_info(info))


def _mutate(f, info_of):
    """The recorded state after f() (the solution it returns), or the verdict when the call says Infeasible."""
    try:
        t = f()
    except M.Infeasible:
        return dict(infeasible=True)
    return _state(t, info_of(t))


def _read(arrays, info):
    return dict(out={k: _sha(a) for k, a in arrays.items()}, info=_info(info))


def _spread(pool, k):
    """k entries of pool, evenly spread (all of it when it has fewer)."""
    pool = list(pool)
    if len(pool) <= k:
        return pool
    return [pool[(t * len(pool)) // k] for t in range(k)]


def _two_rows(x):
    """Two rows over the largest values of x, both violated at x: a <= row and a >= row with unlike coefficients."""
    top = [int(j) for j in np.argsort(x)[::-1][:8]]
    a, b = top[:5], top[3:]
    wa, wb = [1.0, 0.5, 2.0, 1.5, 0.75], [-1.25, 0.5, -2.0, -1.0, 3.0]
    ra, rb = float(np.dot(wa, x[a])), float(np.dot(wb, x[b]))
    return [(list(zip(a, wa)), M.LE, ra - 0.1 * abs(ra) - 1e-3), (list(zip(b, wb)), M.GE, rb + 0.1 * abs(rb) + 1e-3)]


def _record_mutators(lp, fresh, out):
    from tests.test_fixing import _request_lists
    from tests.test_rhs import rhs_list
    s = fresh()
    vs, cst = s.basis_status()
    x, b = s.values(), s.constraint_rhs()
    rhs_info = lambda t: t.rhs_info()
    for k in LENGTHS:
        cs, vals = rhs_list(lp, x, cst, "loose-in", k)                                   # basic slacks moved inside their bounds: no pivot
        out["set_rhs inside %d" % k] = _mutate(lambda: fresh().set_rhs(cs, vals), rhs_info)
        rec = None
        for kind in RESOLVE_KINDS:                                                       # the first kind whose list pivots and stays feasible
            cs, vals = rhs_list(lp, x, cst, kind, k)
            if not cs:
                continue
            rec = dict(_mutate(lambda: fresh().set_rhs(cs, vals), rhs_info), kind=kind)
            if not rec.get("infeasible") and rec["info"]["pivots"] >= 1:
                break
        out["set_rhs re-solve %d" % k] = rec
        cs = list(range(0, lp["m"], 3))[:k]                                              # rows with basic and with non-basic slacks
        out["set_rhs current %d" % k] = _mutate(lambda: fresh().set_rhs(cs, b[cs]), rhs_info)
    rows = _two_rows(x)
    out["add_constraints of two general rows"] = _mutate(lambda: fresh().add_constraints(rows), lambda t: t.cut_info())
    stats = lambda t: {n: t.stats()[n] for n in STATS}
    for name, kind in (("basic", "basic"), ("non-basic", "shift")):
        for j, val in zip(*_request_lists(lp, vs, x, kind, 8)):                          # the first variable that stays feasible
            rec = dict(_mutate(lambda: fresh().fix_var(j, val), stats), var=int(j))
            if not rec.get("infeasible"):
                break
        out["fix_var %s" % name] = rec


def _record_reads(lp, s, out):
    from tests.test_rhs import _scenarios
    n, nc, nr = s.num_vars, s.num_constraints, s.num_rows
    vs, cst = s.basis_status()
    head = s.basis_head()
    out["basis_head"] = dict(out=dict(head=_sha(head)), info={})
    out["dual_values"] = dict(out=dict(pi=_sha(s.dual_values())), info=_info(s.certificate()))  # (where the largest row violation sits)
    rng = np.random.default_rng(7)
    tab, rng_info = s.tableau_info, s.ranging_info
    for k in LENGTHS:
        cs, rhs = _scenarios(lp, s, k)
        out["rhs_scenarios %d" % k] = _read(s.rhs_scenarios(cs, rhs), s.rhs_info())
        out["basis_solve %d" % k] = _read(dict(x=s.basis_solve(rng.standard_normal((k, nc)))), tab())
        out["basis_solve transposed %d" % k] = _read(dict(x=s.basis_solve(rng.standard_normal((k, nr)), transpose=True)), tab())
        basic = _spread(head, k)
        out["binv_rows %d" % k] = _read(dict(rows=s.binv_rows(basic)), tab())
        out["binv_cols %d" % k] = _read(dict(cols=s.binv_cols(_spread(range(nc), k))), tab())
        nonbasic = sorted(set(range(n + nc)) - set(int(v) for v in head))
        out["tableau_cols %d" % k] = _read(dict(cols=s.tableau_cols(_spread(nonbasic, k) + basic[:1])), tab())   # k solves and a unit vector
        ip, ix, dv = s.tableau_rows(basic)
        out["tableau_rows %d" % k] = _read(dict(indptr=ip, indices=ix, data=dv), tab())
        lo, hi = s.rhs_ranging(_spread(np.flatnonzero(cst != 0), k))                     # a non-basic slack: a column of B^-1 each
        out["rhs_ranging %d" % k] = _read(dict(lo=lo, hi=hi), rng_info())
        ba = _spread(np.flatnonzero(vs == 0), k)
        lo, hi = s.cost_ranging(ba)                                                      # a basic variable: a row of B^-1 each
        out["cost_ranging %d" % k] = _read(dict(lo=lo, hi=hi), rng_info())
        out["branch_penalties %d" % k] = _read(s.branch_penalties(ba), s.branch_info())


def record_case(name):
    lp, fresh, env = _case(name)
    out = {}
    with _env(**env):
        _record_reads(lp, fresh(), out)                                                  # on the solution itself: a clone has no pending terms
        _record_mutators(lp, fresh, out)
    return out


def record():
    return {name: record_case(name) for name in CASES}


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    rec = record()
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases, %d calls -> %s" % (len(rec), sum(len(c) for c in rec.values()), path))
