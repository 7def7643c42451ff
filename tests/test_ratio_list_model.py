"""CPU: the rule of the list form of the primal Harris test (k_ratio_primal_fused, rl_cap >= 0), as a numpy model.

The plain rule (solver.rs:782-853) is two passes over the positions p with |alpha_p| >= EPS:
  pass 1   max_step = min(bound, min_p (step_p + EPS) / |alpha_p|)
  pass 2   the winner is the position with the largest |alpha_p| among those with step_p / |alpha_p| <= max_step, the lowest
           position on ties (cand_better); none: a bound flip or an unbounded ray.
The list form makes ONE pass over the grid: block b (256 threads x 4 positions, position = b * 256 + t + u * nblocks * 256) knows its
own minimum m_b, keeps S_b = its positions with q = step / |alpha| <= min(m_b, bound), takes top_b = the best of S_b, drops every other
member with q >= q_top (whenever such a member is eligible, so is top_b, which beats it) and hands what is left — at most `cap`
entries, the count as it is when there are more — to the block that arrives last.  That block folds the minima into max_step, keeps the
listed entries with q <= max_step and takes the best; when a count exceeds the cap it re-scans every position instead.

Winner and max_step must be IDENTICAL to the plain rule's in every case: continuous data, all-zero steps, equal |alpha| at different
positions, entries below EPS, a bound below every ratio, for caps 0, 1 and 8 and m from 1 to 5 000."""
import numpy as np
import pytest

EPS = 1e-8   # solver.rs:12
BLK, PT = 256, 4
NONE = -1


def better(ka, ia, kb, ib):
    """cand_better: a beats b (b may be none)."""
    return ib == NONE or ka > kb or (ka == kb and ia < ib)


def two_pass(alpha, step, bound):
    ca = np.abs(alpha)
    live = ca >= EPS
    mn = np.inf
    if live.any():
        mn = float(np.min((step[live] + EPS) / ca[live]))
    max_step = min(bound, mn) if mn < bound else bound
    best_k, best_i = 0.0, NONE
    for p in np.flatnonzero(live):
        if step[p] / ca[p] <= max_step and better(ca[p], p, best_k, best_i):
            best_k, best_i = ca[p], int(p)
    return max_step, best_i


def list_form(alpha, step, bound, cap):
    m = len(alpha)
    nb = max(1, -(-m // (BLK * PT)))
    ca = np.abs(alpha)
    part_min, cnts, lists = [], [], []
    for b in range(nb):
        pos = (b * BLK + np.arange(BLK)[:, None] + np.arange(PT)[None, :] * nb * BLK).reshape(-1)
        pos = pos[pos < m]
        pos = pos[ca[pos] >= EPS]
        mb = float(np.min((step[pos] + EPS) / ca[pos])) if len(pos) else np.inf
        part_min.append(mb)
        lim = mb if mb < bound else bound
        q = step[pos] / ca[pos]
        mem = q <= lim
        sp, sq = pos[mem], q[mem]
        top_k, top_i, top_q = 0.0, NONE, 0.0
        for p, qq in zip(sp, sq):
            if better(ca[p], p, top_k, top_i):
                top_k, top_i, top_q = ca[p], int(p), qq
        ent = []
        if top_i != NONE:
            ent.append((top_k, top_q, top_i))
            ent += [(ca[p], qq, int(p)) for p, qq in zip(sp, sq) if p != top_i and qq < top_q]
        cnts.append(len(ent))      # above the cap: stored as it is
        lists.append(ent[:cap])    # (which entries of an overflowing list are kept does not matter: nobody reads them)
    mn = min(part_min)
    max_step = mn if mn < bound else bound
    overflow = any(c > cap for c in cnts)
    best_k, best_i = 0.0, NONE
    if overflow:   # the final block re-runs pass 2 over every position
        for p in range(m):
            if ca[p] >= EPS and step[p] / ca[p] <= max_step and better(ca[p], p, best_k, best_i):
                best_k, best_i = ca[p], p
    else:
        for ent in lists:
            for k, qq, p in ent:
                if qq <= max_step and better(k, p, best_k, best_i):
                    best_k, best_i = k, p
    return max_step, best_i, overflow, max(cnts)


def _data(kind, m, rng):
    alpha = rng.standard_normal(m) * np.where(rng.random(m) < 0.3, 0.0, 1.0)  # supp(alpha_q) is sparse
    step = rng.random(m) * 10.0
    bound = np.inf
    if kind == "continuous":
        pass
    elif kind == "zero steps":
        step[:] = 0.0
    elif kind == "half zero steps":
        step[rng.random(m) < 0.5] = 0.0
    elif kind == "equal alpha":
        alpha = np.where(alpha != 0.0, np.sign(alpha) * 0.5, 0.0)
        step = np.round(step)            # many equal ratios as well
    elif kind == "equal alpha zero steps":
        alpha = np.where(alpha != 0.0, np.sign(alpha) * 2.0, 0.0)
        step[:] = 0.0
    elif kind == "below EPS":
        tiny = rng.random(m) < 0.5
        alpha = np.where(tiny, alpha * 1e-9, alpha)   # |alpha| < EPS: not a candidate, whatever its ratio
        step = np.where(tiny, 0.0, step)
    elif kind == "near ties":
        step = np.abs(alpha) * (1.0 + rng.integers(0, 3, m) * 1e-9)   # ratios within EPS / |alpha| of each other: long lists
    elif kind == "small bound":
        step = step + 1.0
        bound = 1e-3                      # below every ratio: no candidate (a bound flip)
    elif kind == "finite bound":
        bound = float(np.median(step))
    elif kind == "infinite steps":
        step = np.where(rng.random(m) < 0.5, np.inf, step)
    else:
        raise AssertionError(kind)
    return alpha, step, bound


KINDS = ["continuous", "zero steps", "half zero steps", "equal alpha", "equal alpha zero steps", "below EPS", "near ties", "small bound",
         "finite bound", "infinite steps"]
SIZES = [1, 2, 255, 256, 257, 1023, 1024, 1025, 2048, 2049, 3000, 4097, 5000]


@pytest.mark.parametrize("cap", [0, 1, 8])
@pytest.mark.parametrize("kind", KINDS)
def test_list_form_takes_the_winner_and_the_step_bound_of_the_two_passes(kind, cap):
    rng = np.random.default_rng(1000 * KINDS.index(kind) + cap)
    seen_list = seen_ovf = seen_none = 0
    for m in SIZES:
        for rep in range(3):
            alpha, step, bound = _data(kind, m, rng)
            ms0, w0 = two_pass(alpha, step, bound)
            ms1, w1, ovf, longest = list_form(alpha, step, bound, cap)
            assert ms1 == ms0 or (np.isinf(ms0) and np.isinf(ms1)), (kind, m, ms0, ms1)
            assert w1 == w0, (kind, m, cap, w0, w1, ovf)
            seen_ovf += ovf
            seen_list += not ovf
            seen_none += w0 == NONE
            if kind in ("zero steps", "equal alpha zero steps"):
                assert longest <= 1, longest          # every ratio zero: top_b alone survives
    if cap == 0:
        assert seen_ovf > 0 or kind == "small bound"  # cap 0: any block with a candidate overflows
    if cap == 8:
        assert seen_list > 0
    if kind == "small bound":
        assert seen_none == len(SIZES) * 3 and seen_ovf == 0


def test_continuous_data_lists_one_or_two_entries_per_block():
    rng = np.random.default_rng(7)
    longest = 0
    for m in (1000, 5000):
        for rep in range(20):
            alpha, step, bound = _data("continuous", m, rng)
            longest = max(longest, list_form(alpha, step, bound, 8)[3])
    assert 1 <= longest <= 2, longest


def test_a_block_without_candidates_lists_nothing():
    alpha = np.zeros(3000)
    step = np.ones(3000)
    alpha[5] = 1.0            # block 0 of 3 holds the only live position
    ms, w, ovf, longest = list_form(alpha, step, np.inf, 8)
    assert (ms, w, ovf, longest) == ((1.0 + EPS) / 1.0, 5, False, 1)
    assert two_pass(alpha, step, np.inf) == (ms, w)
