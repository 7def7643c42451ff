"""Per-call wall time of the calls around Engine::SolveBlock / Engine::warm_resolve, one process, one JSON line:

set_rhs / rhs_scenarios  the harness and instance of profiles/rhs.json (tests/test_rhs.py): gen_mixed_lp(6000, 10000, 4, 3), the tighten
                         list of 64 rows on a clone, 64 scenarios of 16 constraints; 5 timed calls after one warm-up, ms per call
fix_vars / fix_info      as profiles/boundary_refactor.json measured them: gen_cover_lp(70, 90, 5, 5) after its solve, through ctypes with
                         prebuilt arrays; fix_vars of one non-basic variable at its current value, 5 x 500 calls after 200 untimed;
                         fix_info, 5 x 20000 calls after 2000 untimed; us per call

    python tools/solve_block_timing.py

profiles/solve_block_refactor.json holds the lines of two builds of the library alternating on one MI355X, 5 processes each."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import minilp_amd as M                                                                   # noqa: E402
from minilp_amd import api, lpgen                                                        # noqa: E402


def rhs_calls():
    from tests.test_rhs import TIGHTEN_K, _scenarios, rhs_list
    lp = lpgen.gen_mixed_lp(6000, 10000, 4, 3)
    s = lpgen.build_problem(M.Problem, lp).solve()
    _, cst = s.basis_status()
    cs, vals = rhs_list(lp, s.values(), cst, "tighten", TIGHTEN_K)
    sc, rhs = _scenarios(lp, s, 64)
    assert len(cs) == TIGHTEN_K and len(sc) == 16
    warm, dev = [], []
    for rep in range(6):
        a = s.clone()
        t0 = time.perf_counter()
        a = a.set_rhs(cs, vals)
        t1 = time.perf_counter()
        s.rhs_scenarios(sc, rhs)
        t2 = time.perf_counter()
        if rep:
            warm.append((t1 - t0) * 1e3)
            dev.append((t2 - t1) * 1e3)
    return dict(set_rhs_ms=warm, rhs_scenarios_ms=dev, set_rhs_pivots=a.rhs_info()["pivots"])


def fix_calls():
    L = M.lib()
    s = lpgen.build_problem(M.Problem, lpgen.gen_cover_lp(70, 90, 5, 5)).solve()
    vs, _ = s.basis_status()
    j = int(np.flatnonzero((vs == 1) | (vs == 2))[0])
    v, x = np.array([j], dtype=np.uint32), np.array([s.values()[j]])
    pv, px = v.ctypes.data_as(C.POINTER(C.c_uint32)), x.ctypes.data_as(C.POINTER(C.c_double))
    h, info = C.byref(s._h), api.MlpFixInfo()

    def per_call(f, n, untimed):
        for _ in range(untimed):
            f()
        out = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(n):
                f()
            out.append((time.perf_counter() - t0) / n * 1e6)
        return out

    fix = per_call(lambda: L.mlp_solution_fix_vars(h, pv, px, 1), 500, 200)
    read = per_call(lambda: L.mlp_solution_fix_info(s._h, C.byref(info)), 20000, 2000)
    assert info.requests == 1 and info.shifted == 0 and info.solves == 0 and info.pivots == 0
    return dict(fix_vars_us=fix, fix_info_us=read)


if __name__ == "__main__":
    print("TIMING " + json.dumps(dict(rhs_calls(), **fix_calls())))
