"""GPU: the dense chain of the medium nucleus with the pushed F product — k_ftran_fused<G> (head, W gather, atomic push of -F alpha_K into
the singleton positions) -> ratio test -> k_fused_w<8> (v partials + eager eta update of W) -> k_post_fused — against the oracle.

MLP_STR_K=0, MLP_RATIO_ONE=0, MLP_HYPER=0, MLP_PRIMAL_HEAD=0 and MLP_SMALL_BASIS=0 make that chain run from the first pivot of a model
of a few thousand rows (as in tests/test_ratio_onepass.py); MLP_DETERMINISTIC=0 keeps the F product on the push.  The instances cover
every lane count of the FTRAN (the engine picks 64 / 16 / 4 lanes per slot from the average column length: >= 40, >= 6, below), columns
that fit the two entries per lane a slot holds ahead of its multiplier and columns that do not, and a nucleus that grows past 512 and
1 024 slots (the column chunk FW_TC of the W pass).  The pushed sums go through float atomics, so the solve is not bitwise repeatable;
the pivots are the oracle's all the same."""
import numpy as np
import pytest

import minilp_amd as M
from minilp_amd import lpgen
from oracle import minilp_oracle as O
from tests.common import obj_close

pytestmark = pytest.mark.gpu

REFRESH_TOL = 1e-7  # the engine re-inverts W when the two-way pivot check (alpha_q[r] against alpha_r[q]) disagrees by more

# name: (gen_sparse_lp arguments, pivot budget, lanes per slot, smallest nucleus at the end)
INSTANCES = {
    "64 lanes, columns within the prefetch": ((2000, 1000, 30, 7), None, 64, 0),
    "64 lanes, columns beyond the prefetch": ((1500, 300, 40, 5), None, 64, 0),
    "16 lanes": ((1500, 1200, 10, 3), None, 16, 0),
    "16 lanes, nucleus past 1024": ((4000, 3500, 12, 4), 1700, 16, 1025),  # (1 400 pivots leave the nucleus at 965 slots)
    "4 lanes": ((1500, 1020, 4, 4), None, 4, 0),  # (5.9 entries per column on average, 14 at most; no column is empty with this seed)
}
_cache = {}


def _lanes(lp):
    avg = len(lp["data"]) / lp["n"]
    return 64 if avg >= 40.0 else (16 if avg >= 6.0 else 4)


def _instance(name):
    """The model and the oracle's solve of it, computed once."""
    if name not in _cache:
        args, budget, _, _ = INSTANCES[name]
        lp = lpgen.gen_sparse_lp(*args)
        kw = dict(trace=True) if budget is None else dict(trace=True, budget=budget)
        so = lpgen.build_problem(O.Problem, lp).solve(**kw)
        _cache[name] = (lp, kw, [t[:5] for t in so.trace()], so.objective())
    return _cache[name]


@pytest.mark.parametrize("name", list(INSTANCES))
def test_medium_chain_takes_the_oracles_pivots(monkeypatch, name):
    for key in ("MLP_STR_K", "MLP_RATIO_ONE", "MLP_HYPER", "MLP_PRIMAL_HEAD", "MLP_SMALL_BASIS", "MLP_DETERMINISTIC"):
        monkeypatch.setenv(key, "0")
    lp, kw, trace, obj = _instance(name)
    _, _, lanes, k_min = INSTANCES[name]
    assert _lanes(lp) == lanes
    counts = np.bincount(lp["indices"], minlength=lp["n"])
    s = lpgen.build_problem(M.Problem, lp).solve(**kw)
    st = s.stats()
    print(f"{name}: {st['iterations']} pivots ({st['primal_iters']} primal), nucleus {st['nucleus_size']}, longest column {counts.max()}, "
          f"max_pivot_err {st['max_pivot_err']:.2e}, reinversions {st['reinversions']}")
    assert [t[:5] for t in s.trace()] == trace
    assert obj_close(s.objective(), obj)
    assert st["max_pivot_err"] < REFRESH_TOL, st["max_pivot_err"]
    assert st["primal_iters"] > 0 and st["nucleus_size"] >= k_min, (st["primal_iters"], st["nucleus_size"])
    assert s.reinvert() < 1e-8
