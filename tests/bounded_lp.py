"""Bounded-variable LPs with continuous data (tests/test_bounded.py, tests/test_bounded_generators.py, tests/test_sparse_row.py).

Every family of minilp_amd/lpgen.py whose pivot sequence the suite compares has x >= 0 and no upper bound; gen_mixed_lp has boxed, fixed and
free columns but integer data (sequences comparable up to the first tie only) and is solved by the dual loop alone.  `gen_bounded_lp`
is the family in between: gen_sparse_lp's pattern, continuous data of either sign, Minimize, every bound kind of the bounded ratio rule
(solver.rs:782-853) at once:

  kinds 0-2  [0, inf)                     kind 6  (-inf, u]        upper bound only: non-basic it sits AT its upper bound
  kinds 3, 9 [0, ~0.02]  narrow boxes: an entering column whose own range is shorter than every ratio flips (solver.rs:842-851)
  kinds 4, 5 [l, l + w]  wide boxes, l of either sign             kind 7  [l, inf), l of either sign             kind 8  fixed at l

The rows ('=' one in eight, '<=' and '>=' otherwise) are built around a strictly feasible x0, the cost is c = A^T y + r for a
dual-feasible (y, r), so the LP is feasible and bounded.  The start point (every column at the bound its cost prefers, boxes with a
negative cost at their upper bound) is neither primal nor dual feasible: the solve is the dual loop on the artificial objective, then
the primal loop with steepest edge, which takes the bound flips.  `primal_start` and `dual_start` are the variants with one loop only.

Free columns are left out on purpose.  With a tenth of the columns free the oracle (a restatement of the reference) reports Unbounded on
(120, 160, 6, 11), which HiGHS solves, and returns a non-finite x and a NaN objective on (300, 260, 8, 6): the quirk of the reference
that tests/test_ranging.py::_highs_obj describes.  It belongs to the reference, not to the bounded ratio rule under test here.

That no decision of a sequence lies within rounding of a tie is checked on the CPU (test_bounded_generators.py): the instance with its
rows and columns in reverse order, where every row sum rounds differently, must give the same sequence of (phase, entering, leaving)."""
import numpy as np

from minilp_amd.lpgen import EQ, GE, LE, MINIMIZE, _stream, build_problem, gen_sparse_lp, splitmix64, uniform01

NONNEG, NARROW, WIDE, UPPER_ONLY, LOWER_ONLY, FIXED = range(6)
KIND_NAMES = ("nonneg", "narrow", "wide", "upper_only", "lower_only", "fixed")
_KIND_OF = np.array([NONNEG, NONNEG, NONNEG, NARROW, WIDE, WIDE, UPPER_ONLY, LOWER_ONLY, FIXED, NARROW])


def column_kinds(n, seed):
    """The bound kind (NONNEG ... FIXED) gen_bounded_lp gives each of n columns."""
    return _KIND_OF[(splitmix64(_stream(seed, 61), n) % np.uint64(10)).astype(np.int64)]


def gen_bounded_lp(m, n, k, seed=12, narrow=0.02):
    base = gen_sparse_lp(m, n, k, seed)
    u = lambda tag, cnt: uniform01(_stream(seed, tag), cnt)
    kind = (splitmix64(_stream(seed, 61), n) % np.uint64(10)).astype(np.int64)
    l0 = -1.0 + 1.5 * u(62, n); w = 0.3 + 1.2 * u(63, n); t = 0.15 + 0.7 * u(64, n)
    lo = np.zeros(n); hi = np.full(n, np.inf); x0 = t.copy()               # kinds 0-2: [0, inf)
    nb = (kind == 3) | (kind == 9); hi[nb] = narrow * w[nb]                # narrow boxes [0, ~0.02]: the flips
    wb = (kind == 4) | (kind == 5); lo[wb] = l0[wb]; hi[wb] = l0[wb] + w[wb]   # wide boxes, lower bound of either sign
    up = kind == 6; lo[up] = -np.inf; hi[up] = l0[up] + w[up]              # upper bound only
    ng = kind == 7; lo[ng] = l0[ng]                                        # lower bound only, of either sign
    fx = kind == 8; lo[fx] = l0[fx]; hi[fx] = l0[fx]                       # fixed
    box = nb | wb
    x0[box] = lo[box] + t[box] * (hi[box] - lo[box]); x0[up] = hi[up] - t[up]; x0[ng] = lo[ng] + t[ng]; x0[fx] = lo[fx]
    sgn = np.where(u(65, m * k) < 0.3, -1.0, 1.0)
    data = (0.1 + 0.9 * base["data"]) * sgn
    lhs = np.add.reduceat(data * x0[base["indices"]], base["indptr"][:-1])
    opk = (splitmix64(_stream(seed, 66), m) % np.uint64(8)).astype(np.int64)
    ops = np.where(opk == 0, EQ, np.where(opk < 5, LE, GE)).astype(np.int32)
    slack = 0.05 + 0.5 * u(67, m)
    rhs = np.where(ops == EQ, lhs, np.where(ops == LE, lhs + slack, lhs - slack))   # x0 is strictly feasible
    # a dual-feasible point (y by row kind, r by bound kind) makes the LP bounded: c = A^T y + r
    y = u(68, m) * np.where(ops == LE, -1.0, np.where(ops == GE, 1.0, 2.0 * u(69, m) - 1.0)) * (u(70, m) < 0.6)
    r = u(71, n); sr = np.where(u(72, n) < 0.5, -1.0, 1.0)
    r = np.where(up, -r, np.where(box | fx, sr * r, r))
    c = np.bincount(base["indices"], weights=data * y[np.repeat(np.arange(m), k)], minlength=n) + r
    return dict(base, name=f"bounded_{m}x{n}_k{k}_s{seed}", direction=MINIMIZE, obj=c, lo=lo, hi=hi, data=data, ops=ops, rhs=rhs)


def _start_point(lp):
    """Where a solve starts (solver.rs:133-187): every column non-basic at the bound its cost prefers — a finite upper bound if the
    cost is negative, else the lower bound — and at the other one where that bound is infinite."""
    lo, hi = lp["lo"], lp["hi"]
    return np.where(lp["obj"] < 0, np.where(np.isfinite(hi), hi, lo), np.where(np.isfinite(lo), lo, hi))


def primal_start(m, n, k, seed):
    """gen_bounded_lp with the rows moved so that the start point is strictly feasible (every slack basic and off its bound, so no
    ratio ties at zero): the whole solve is the primal loop with steepest edge FROM THE SLACK BASIS, the nucleus growing from zero —
    what k_primal_head and its hand-over at MLP_PRIMAL_HEAD_K slots need (in a two-phase solve the dual loop has outgrown them before
    the first primal iteration).  A '=' row becomes '<=' or '>=' by the sign of its multiplier in the generator's dual-feasible point,
    which therefore stays dual feasible: the LP is bounded."""
    lp = gen_bounded_lp(m, n, k, seed)
    u = lambda tag, cnt: uniform01(_stream(seed, tag), cnt)
    ops = lp["ops"]
    ysign = np.where(ops == EQ, 2.0 * u(69, m) - 1.0, 0.0)                              # (the sign y has on a '=' row of gen_bounded_lp)
    ops = np.where(ops == EQ, np.where(ysign > 0, GE, LE), ops).astype(np.int32)
    lhs = np.add.reduceat(lp["data"] * _start_point(lp)[lp["indices"]], lp["indptr"][:-1])
    slack = 0.05 + 0.5 * u(67, m)
    return dict(lp, name=f"bounded_primal_{m}x{n}_k{k}_s{seed}", ops=ops, rhs=np.where(ops == LE, lhs + slack, lhs - slack))


def dual_start(m, n, k, seed):
    """gen_bounded_lp with the cost c = r alone (y = 0 in the generator's dual-feasible point): positive on the columns without an upper
    bound, negative on those without a lower one, of either sign on boxes, which then start at the bound their cost prefers.  The start
    point is dual feasible and primal infeasible: the whole solve is the dual loop on the real objective without primal steepest edge —
    the one loop the hypersparse kernel takes (Engine::hyper_capable) — over boxed, upper-only, lower-only and fixed columns."""
    lp = gen_bounded_lp(m, n, k, seed)
    u = lambda tag, cnt: uniform01(_stream(seed, tag), cnt)
    lo, hi = lp["lo"], lp["hi"]
    r = u(71, n); sr = np.where(u(72, n) < 0.5, -1.0, 1.0)
    return dict(lp, name=f"bounded_dual_{m}x{n}_k{k}_s{seed}", obj=np.where(np.isinf(lo), -r, np.where(np.isfinite(hi), sr * r, r)))


def relabelled(lp):
    """The same LP with its rows and its columns in reverse order (column j becomes n - 1 - j, row i becomes m - 1 - i; every row stays
    sorted by column).  Row sums, dot products and reductions over it add the same numbers in another order."""
    m, n = lp["m"], lp["n"]
    ip = lp["indptr"]
    order = np.arange(len(lp["indices"]))[::-1]                  # rows reversed, and the entries of each row reversed
    indptr = np.concatenate(([0], np.cumsum(np.diff(ip)[::-1]))).astype(np.int64)
    return dict(lp, name=lp["name"] + "_relabelled", obj=lp["obj"][::-1].copy(), lo=lp["lo"][::-1].copy(), hi=lp["hi"][::-1].copy(),
                indptr=indptr, indices=(n - 1 - lp["indices"][order]).astype(np.int64), data=lp["data"][order].copy(),
                ops=lp["ops"][::-1].copy(), rhs=lp["rhs"][::-1].copy())


def relabel_var(v, m, n):
    """A variable id of the relabelled instance as an id of the original one (columns 0 .. n-1, then the slack of row i at n + i)."""
    return v if v < 0 else (n - 1 - v if v < n else n + (m - 1 - (v - n)))


# the instances: (m, n, k, seed).  SMALL joins the CPU test only.
SMALL = (40, 30, 6, 9)
CASES = [(120, 160, 6, 11), (300, 400, 6, 3), (300, 260, 8, 6), (400, 300, 12, 7), (700, 600, 12, 6)]


# the variants with one loop only: ("primal" | "dual", m, n, k, seed)
PRIMAL_START_CASES = [("primal", 400, 300, 12, 7), ("primal", 700, 600, 12, 6)]
DUAL_START_CASES = [("dual", 300, 400, 6, 3), ("dual", 700, 600, 12, 6)]
_VARIANT = {"primal": primal_start, "dual": dual_start}


def instance(case):
    return _VARIANT[case[0]](*case[1:]) if isinstance(case[0], str) else gen_bounded_lp(*case)


def case_id(case):
    return ("bounded-%s-%dx%d-k%d-s%d" if isinstance(case[0], str) else "bounded-%dx%d-k%d-s%d") % tuple(case)


# ------------------------------------------------------------------------------------------------ references (computed once, never changed)
_REF = {}


def reference(case):
    """The instance, the oracle's trace, stats, objective and x, which columns it leaves non-basic at their upper / lower bound, and the
    live HiGHS objective.  Asserted here: the oracle terminates Optimal (solve() raises otherwise) with a feasible x and HiGHS' objective
    to HIGHS_RTOL."""
    case = tuple(case)
    if case in _REF:
        return _REF[case]
    from oracle import minilp_oracle as O
    from tests.common import HIGHS_RTOL, check_feasible
    from tests.degenerate_lp import highs
    lp = instance(case)
    so = build_problem(O.Problem, lp).solve(trace=True)
    x = so.values()
    assert np.isfinite(x).all() and np.isfinite(so.objective())
    check_feasible(lp, x)
    h, _ = highs(lp)
    assert h is not None and abs(so.objective() - h) <= HIGHS_RTOL * max(1.0, abs(h)), (case, so.objective(), h)
    nbv = so.state("nb_vars").astype(np.int64)
    at_max, at_min = so.state("nb_at_max") != 0, so.state("nb_at_min") != 0
    n = lp["n"]
    nb_upper = np.zeros(n, dtype=bool)
    nb_lower = np.zeros(n, dtype=bool)
    nb_upper[nbv[at_max & (nbv < n)]] = True
    nb_lower[nbv[at_min & ~at_max & (nbv < n)]] = True
    _REF[case] = dict(lp=lp, case=case, kinds=column_kinds(n, case[-1]), trace=so.trace(), stats=so.stats(), objective=so.objective(), x=x,
                      nb_upper=nb_upper, nb_lower=nb_lower, highs=h)
    return _REF[case]
