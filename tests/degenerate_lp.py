"""Degenerate integer-data LP generators (tests/test_degenerate.py, tests/test_degenerate_generators.py, tools/fuzz_medium.py).

Every family of minilp_amd/lpgen.py that the suite compares pivot for pivot has continuous random data: ratio tests never tie, no step
has length zero.  The four families here are nothing but ties: 0/1 matrices, small integer costs and right-hand sides.  Three of them
(assignment, unit_transport, and two_matching up to a factor 2) have integral vertices, so on them every basis inverse, tableau entry and
basic value is a small integer (half-integer) and floating-point arithmetic is exact in any summation order.

Those four start dual feasible and are solved by the dual simplex alone.  `matching` and `unit_packing` are their primal counterparts
(Maximize, '<=' rows, x = 0 feasible): the primal simplex from the slack basis, every pricing score and every ratio a tie at the start.

Seeded with numpy.random.default_rng; instances are `lpgen`-style dicts (lpgen.build_problem, tests.common.check_feasible work on them).
No row is empty (check_feasible's reduceat needs that)."""
import math

import numpy as np

from minilp_amd import lpgen


def _lp(name, obj, lo, hi, rows, ops, rhs, direction=lpgen.MINIMIZE):
    """rows: list of sorted int arrays of column indices; every coefficient is 1."""
    indptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int64)
    assert (np.diff(indptr) > 0).all(), "empty row"
    indices = np.concatenate(rows).astype(np.int64)
    return dict(name=name, direction=direction, m=len(rows), n=len(obj), obj=np.asarray(obj, dtype=np.float64),
                lo=np.asarray(lo, dtype=np.float64), hi=np.asarray(hi, dtype=np.float64), indptr=indptr, indices=indices,
                data=np.ones(len(indices)), ops=np.asarray(ops, dtype=np.int32), rhs=np.asarray(rhs, dtype=np.float64))


def assignment(n, seed):
    """n x n assignment problem: column i * n + j is x_ij, integer costs 1..9, bounds [0, inf); n '=' rows sum_j x_ij = 1 then n '=' rows
    sum_i x_ij = 1.  The 2n rows have rank 2n - 1: the redundant row is intended (a basis always keeps one fixed slack)."""
    rng = np.random.default_rng(seed)
    cost = rng.integers(1, 10, size=n * n)
    rows = [np.arange(i * n, (i + 1) * n) for i in range(n)] + [np.arange(j, n * n, n) for j in range(n)]
    return _lp(f"assignment_{n}_s{seed}", cost, np.zeros(n * n), np.full(n * n, np.inf), rows, np.full(2 * n, lpgen.EQ), np.ones(2 * n))


def unit_transport(S, D, deg, seed):
    """Transportation with unit gains: every demand node is linked to `deg` distinct random supply nodes (arc j * deg + t), gain 1 on both
    rows, integer costs 1..5; S supply rows '<=' the common capacity ceil(2 sum(demand) / S), then D demand rows '>=' integer demands
    1..3.  x = 0 is dual feasible; every basis is a forest.  The arcs are redrawn (same generator) until every supply node has one."""
    rng = np.random.default_rng(seed)
    for _ in range(64):
        sup = np.stack([np.sort(rng.choice(S, size=deg, replace=False)) for _ in range(D)])
        if len(np.unique(sup)) == S:
            break
    else:
        raise AssertionError("a supply node without an arc in 64 draws")
    n = D * deg
    arc_sup = sup.reshape(-1)
    cost = rng.integers(1, 6, size=n)
    demand = rng.integers(1, 4, size=D)
    cap = math.ceil(2.0 * float(demand.sum()) / S)
    rows = [np.flatnonzero(arc_sup == i) for i in range(S)] + [np.arange(j * deg, (j + 1) * deg) for j in range(D)]
    ops = np.concatenate((np.full(S, lpgen.LE), np.full(D, lpgen.GE)))
    rhs = np.concatenate((np.full(S, float(cap)), demand.astype(np.float64)))
    return _lp(f"unit_transport_{S}x{D}_deg{deg}_s{seed}", cost, np.zeros(n), np.full(n, np.inf), rows, ops, rhs)


def unit_cover(m, n, k, seed):
    """Set covering relaxation: m '>=' rows of k ones (distinct random columns), rhs 1, all costs 1, bounds [0, 1].  Not totally
    unimodular (x is fractional); every dual ratio is a tie at the start."""
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(n, size=k, replace=False)) for _ in range(m)]
    return _lp(f"unit_cover_{m}x{n}_k{k}_s{seed}", np.ones(n), np.zeros(n), np.ones(n), rows, np.full(m, lpgen.GE), np.ones(m))


def matching(n, seed):
    """Maximum-weight bipartite matching on K_nn: the columns and rows of `assignment` with '<=' rows and Maximize (weights 1..9).  Totally
    unimodular; x = 0 is primal feasible, so the solve is the primal simplex from the slack basis."""
    rng = np.random.default_rng(seed)
    w = rng.integers(1, 10, size=n * n)
    rows = [np.arange(i * n, (i + 1) * n) for i in range(n)] + [np.arange(j, n * n, n) for j in range(n)]
    return _lp(f"matching_{n}_s{seed}", w, np.zeros(n * n), np.full(n * n, np.inf), rows, np.full(2 * n, lpgen.LE), np.ones(2 * n), lpgen.MAXIMIZE)


def unit_packing(m, n, k, seed):
    """Set packing relaxation: Maximize sum x over m '<=' rows of k ones, rhs 1, x >= 0 (the rows of `unit_cover`).  Fractional; all
    pricing scores and all primal ratios tie at the start."""
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(n, size=k, replace=False)) for _ in range(m)]
    return _lp(f"unit_packing_{m}x{n}_k{k}_s{seed}", np.ones(n), np.zeros(n), np.full(n, np.inf), rows, np.full(m, lpgen.LE), np.ones(m), lpgen.MAXIMIZE)


def grid_points(w, h):
    """The w x h integer grid, row by row."""
    return np.array([(x, y) for y in range(h) for x in range(w)], dtype=np.int64)


def two_matching(points, nearest=None):
    """Degree LP of a TSP: one column per edge i < j with bounds [0, 1] and the integer-rounded Euclidean distance as its cost, one '='
    row per city with rhs 2.  nearest = K keeps an edge only if one end is among the K nearest neighbours of the other (ties by index).
    Vertices are half-integral."""
    pts = np.asarray(points, dtype=np.int64)
    c = len(pts)
    d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(axis=2)
    keep = np.ones((c, c), dtype=bool)
    if nearest is not None:
        keep[:] = False
        for i in range(c):
            order = np.argsort(np.where(np.arange(c) == i, np.iinfo(np.int64).max, d2[i]), kind="stable")[:nearest]
            keep[i, order] = True
        keep |= keep.T
    ii, jj = np.nonzero(np.triu(keep, 1))
    cost = np.rint(np.sqrt(d2[ii, jj].astype(np.float64)))
    e = len(ii)
    rows = [np.flatnonzero((ii == v) | (jj == v)) for v in range(c)]
    return _lp(f"two_matching_{c}_e{e}", cost, np.zeros(e), np.ones(e), rows, np.full(c, lpgen.EQ), np.full(c, 2.0))


# the instances: the smallest at which each path still splits work over several waves or blocks
CASES = {
    "assignment-24": lambda: assignment(24, 1),
    "assignment-70": lambda: assignment(70, 2),
    "unit_transport-60x80x3": lambda: unit_transport(60, 80, 3, 3),
    "unit_transport-400x600x4": lambda: unit_transport(400, 600, 4, 4),
    "unit_cover-70x90x5": lambda: unit_cover(70, 90, 5, 5),
    "unit_cover-400x500x6": lambda: unit_cover(400, 500, 6, 6),
    "two_matching-6x6": lambda: two_matching(grid_points(6, 6)),
    "two_matching-9x9-nn12": lambda: two_matching(grid_points(9, 9), nearest=12),
}


# primal counterparts (the primal simplex from the slack basis)
PRIMAL_CASES = {
    "matching-24": lambda: matching(24, 7),
    "unit_packing-120x90x5": lambda: unit_packing(120, 90, 5, 8),
    "unit_packing-500x400x6": lambda: unit_packing(500, 400, 6, 9),
}


def family(case):
    return case.split("-")[0]


def highs(lp):
    """scipy's HiGHS on an instance: (objective, x), or (None, None) when it does not report an optimum."""
    import scipy.sparse as sp
    from scipy.optimize import linprog
    A = sp.csr_matrix((lp["data"], lp["indices"], lp["indptr"]), shape=(lp["m"], lp["n"]))
    ops = lp["ops"]
    le, ge, eq = ops == lpgen.LE, ops == lpgen.GE, ops == lpgen.EQ
    sg = -1.0 if lp["direction"] == lpgen.MAXIMIZE else 1.0
    r = linprog(sg * lp["obj"], A_ub=sp.vstack([A[le], -A[ge]]) if (le | ge).any() else None,
                b_ub=np.concatenate([lp["rhs"][le], -lp["rhs"][ge]]) if (le | ge).any() else None,
                A_eq=A[eq] if eq.any() else None, b_eq=lp["rhs"][eq] if eq.any() else None, bounds=list(zip(lp["lo"], lp["hi"])),
                method="highs", options={"primal_feasibility_tolerance": 1e-10, "dual_feasibility_tolerance": 1e-10})
    return (sg * float(r.fun), np.asarray(r.x)) if r.status == 0 else (None, None)


# ------------------------------------------------------------------------------------------------ references (computed once, never changed)
ATOL = 1e-9
_REF = {}


def reference(case):
    """The instance, the oracle's optimum and pivot count, HiGHS' objective, the exact integer where there is one.  The oracle-side
    preconditions are asserted here: feasible and bounded, HiGHS' objective to HIGHS_RTOL, the exact
    integer optimum and an integral (two_matching: half-integral) x on the families with integral vertices."""
    if case in _REF:
        return _REF[case]
    from oracle import minilp_oracle as O
    from tests.common import HIGHS_RTOL, check_feasible
    lp = (CASES[case] if case in CASES else PRIMAL_CASES[case])()
    fam = family(case)
    so = lpgen.build_problem(O.Problem, lp).solve()          # raises Infeasible / Unbounded: the instance must be neither
    xo = so.values()
    check_feasible(lp, xo)
    st = so.stats()
    h, _ = highs(lp)
    assert h is not None and abs(so.objective() - h) <= HIGHS_RTOL * max(1.0, abs(h)), (case, so.objective(), h)
    exact = None
    if fam == "assignment":
        from scipy.optimize import linear_sum_assignment
        n = math.isqrt(lp["n"])
        C = lp["obj"].reshape(n, n)
        r, c = linear_sum_assignment(C)
        exact = float(C[r, c].sum())
    elif fam == "matching":
        from scipy.optimize import linear_sum_assignment
        n = math.isqrt(lp["n"])
        C = lp["obj"].reshape(n, n)                           # (positive weights on K_nn: a maximum matching is perfect)
        r, c = linear_sum_assignment(C, maximize=True)
        exact = float(C[r, c].sum())
    elif fam in ("unit_transport", "two_matching"):          # integer costs, (half-)integral vertices
        exact = float(round(h))
        assert abs(h - exact) <= HIGHS_RTOL * max(1.0, abs(h))
    if fam in ("assignment", "unit_transport", "matching"):
        assert np.abs(xo - np.round(xo)).max() <= ATOL
    if fam == "two_matching":
        assert np.abs(2 * xo - np.round(2 * xo)).max() <= ATOL
    if exact is not None:
        assert abs(so.objective() - exact) <= ATOL
    _REF[case] = dict(lp=lp, family=fam, objective=so.objective(), pivots=int(st["pivots"] + st["bound_flips"]),
                      primal_iters=int(st["primal_iters"]), highs=h, exact=exact)
    return _REF[case]
