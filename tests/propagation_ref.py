"""Bound propagation from row activities, restated in numpy from the rules in include/minilp_hip.h (mlp_solution_propagate_bounds).
The yardstick of tests/test_propagation.py; it knows nothing of the kernels.

The model is the engine's internal form: columns j of [A | I] (j < n structural, n + r the slack of row r), every row the equality
sum_j a_rj x_j = rhs_r over all its entries, the slack included.  A constraint without terms has no row."""
import math

import numpy as np

from minilp_amd import lpgen

INF = math.inf
ACCEPT_RTOL = 1e-7   # a finite bound must improve by more than this (relative to max(1, |bound|)) to be accepted
CROSS_RTOL = 1e-9    # an accepted bound may cross the opposite one by this much and is clamped; more is Infeasible
INT_EPS = 1e-9       # floor(u' + INT_EPS), ceil(l' - INT_EPS) on a marked variable


def internal_form(lp):
    """(indptr, indices, data, rhs, lo, hi) of an lpgen-style instance in the internal form: the slack of row r is column n + r with
    coefficient 1 at the end of the row, bounds [0, inf) for '<=', (-inf, 0] for '>=', [0, 0] for '='."""
    n = lp["n"]
    ip = np.asarray(lp["indptr"], dtype=np.int64)
    keep = np.flatnonzero(np.diff(ip) > 0)
    indptr, indices, data = [0], [], []
    for r, c in enumerate(keep):
        b, e = int(ip[c]), int(ip[c + 1])
        indices.extend(int(j) for j in lp["indices"][b:e])
        data.extend(float(a) for a in lp["data"][b:e])
        indices.append(n + r)
        data.append(1.0)
        indptr.append(len(indices))
    ops = np.asarray(lp["ops"])[keep]
    slo = np.where(ops == lpgen.GE, -INF, 0.0)
    shi = np.where(ops == lpgen.LE, INF, 0.0)
    lo = np.concatenate((np.asarray(lp["lo"], dtype=np.float64), slo))
    hi = np.concatenate((np.asarray(lp["hi"], dtype=np.float64), shi))
    return (np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64), np.asarray(data, dtype=np.float64),
            np.asarray(lp["rhs"], dtype=np.float64)[keep], lo, hi)


def propagate(form, num_vars, fixed=None, is_int=None, max_rounds=10):
    """form: internal_form(...); fixed: {column: value} of the columns flagged by fix_var(s); is_int: num_vars marks or None.
    Returns a dict: vars / lo / hi (the list), infeasible, rounds, accepted (all bound changes), accepted_struct (per round, structural
    variables only), lo_all / hi_all (the working bounds of every column at the end), ratios (improvement / threshold of every
    candidate that improved a finite bound, whether accepted or not: the test of the yardstick looks for values near 1)."""
    indptr, col, a, rhs, lo, hi = form
    m, N, n = len(rhs), len(lo), num_vars
    row = np.repeat(np.arange(m), np.diff(indptr))
    lo, hi = lo.copy(), hi.copy()
    is_fixed = np.zeros(N, dtype=bool)
    for j, x in (fixed or {}).items():
        lo[j] = hi[j] = x
        is_fixed[j] = True
    lo0, hi0 = lo.copy(), hi.copy()
    marked = np.zeros(N, dtype=bool)
    if is_int is not None:
        marked[:n] = np.asarray(is_int, dtype=bool)
    nz, pos = a != 0.0, a > 0.0
    out = dict(vars=np.zeros(0, dtype=np.uint32), lo=np.zeros(0), hi=np.zeros(0), infeasible=False, rounds=0, accepted=0,
               accepted_struct=[], ratios=[])
    with np.errstate(invalid="ignore", divide="ignore"):
        for rnd in range(1, max_rounds + 1):
            out["rounds"] = rnd
            cmin = np.where(nz, np.where(pos, a * lo[col], a * hi[col]), 0.0)
            cmax = np.where(nz, np.where(pos, a * hi[col], a * lo[col]), 0.0)
            imin, imax = np.isinf(cmin), np.isinf(cmax)
            minfin = np.bincount(row, np.where(imin, 0.0, cmin), m)
            maxfin = np.bincount(row, np.where(imax, 0.0, cmax), m)
            mininf = np.bincount(row, imin, m).astype(np.int64)
            maxinf = np.bincount(row, imax, m).astype(np.int64)
            rest_min = np.where(~imin & (mininf[row] == 0), minfin[row] - cmin, np.where(imin & (mininf[row] == 1), minfin[row], -INF))
            rest_max = np.where(~imax & (maxinf[row] == 0), maxfin[row] - cmax, np.where(imax & (maxinf[row] == 1), maxfin[row], INF))
            t_min, t_max = (rhs[row] - rest_min) / a, (rhs[row] - rest_max) / a
            up_c = np.where(nz, np.where(pos, t_min, t_max), INF)
            lo_c = np.where(nz, np.where(pos, t_max, t_min), -INF)
            un, ln = np.full(N, INF), np.full(N, -INF)
            np.minimum.at(un, col, up_c)
            np.maximum.at(ln, col, lo_c)
            un = np.where(marked, np.floor(un + INT_EPS), un)
            ln = np.where(marked, np.ceil(ln - INT_EPS), ln)
            thr_u, thr_l = ACCEPT_RTOL * np.maximum(1.0, np.abs(hi)), ACCEPT_RTOL * np.maximum(1.0, np.abs(lo))
            acc_u = (np.isinf(hi) & np.isfinite(un)) | (un < hi - thr_u)
            acc_l = (np.isinf(lo) & np.isfinite(ln)) | (ln > lo + thr_l)
            su, sl = np.isfinite(hi) & (un < hi), np.isfinite(lo) & (ln > lo)
            out["ratios"].extend(((hi - un)[su] / thr_u[su]).tolist())
            out["ratios"].extend(((ln - lo)[sl] / thr_l[sl]).tolist())
            over_l, over_u = ln - hi, lo - un           # against the bounds at the start of the round
            tol_l, tol_u = CROSS_RTOL * np.maximum(1.0, np.abs(hi)), CROSS_RTOL * np.maximum(1.0, np.abs(lo))
            if (acc_l & (over_l > tol_l)).any() or (acc_u & (over_u > tol_u)).any():
                out["infeasible"] = True
                return out
            ln = np.where(acc_l & (over_l > 0.0), hi, ln)
            un = np.where(acc_u & (over_u > 0.0), lo, un)
            nacc = int(acc_u.sum() + acc_l.sum())
            out["accepted"] += nacc
            out["accepted_struct"].append(int(acc_u[:n].sum() + acc_l[:n].sum()))
            lo, hi = np.where(acc_l, ln, lo), np.where(acc_u, un, hi)
            if nacc == 0:
                break
    listed = np.flatnonzero(((lo[:n] != lo0[:n]) | (hi[:n] != hi0[:n])) & ~is_fixed[:n])
    out.update(vars=listed.astype(np.uint32), lo=lo[listed], hi=hi[listed], lo_all=lo, hi_all=hi)
    return out
