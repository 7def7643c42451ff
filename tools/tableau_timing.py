#!/usr/bin/env python3
"""Device time of the tableau reads (csrc/tableau.inc) at config 4's late basis (tests/golden/cfg4_basis_p240000.bin.gz,
nucleus 20 493): per operation one batch of 16 requests, median of `--reps` calls after one warm-up, HIP-event time and GB/s against
the algorithmic bytes of mlp_tableau_info; for comparison the same state's certificate()["device_ms"] (one W0 stream plus two passes
over A).  Recorded, not asserted.

    python tools/tableau_timing.py [--reps 5] [--out profiles/tableau.json]"""
import argparse
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tableau.json"))
    a = ap.parse_args()
    import minilp_amd as M
    from minilp_amd import lpgen
    lp = lpgen.gen_sparse_lp(100000, 100000, 100, 4)
    prob = lpgen.build_problem(M.Problem, lp)
    with gzip.open(os.path.join(ROOT, "tests", "golden", "cfg4_basis_p240000.bin.gz"), "rb") as f:
        s = prob.solve_from_basis(f.read(), budget=0)
    rng = np.random.default_rng(1)
    head = s.basis_head()
    n, ncons, m = s.num_vars, s.num_constraints, s.num_rows
    bas = rng.choice(head[head < n], size=16, replace=False)
    nonbasic = np.setdiff1d(np.arange(n + ncons), head)
    nb = rng.choice(nonbasic[nonbasic < n], size=16, replace=False)
    _, cs = s.basis_status()
    rows = rng.choice(np.flatnonzero(cs != M.MLP_BASIC), size=16, replace=False)
    ops = {"binv_rows": lambda: s.binv_rows(bas), "tableau_rows": lambda: s.tableau_rows(bas), "binv_cols": lambda: s.binv_cols(rows),
           "tableau_cols": lambda: s.tableau_cols(nb), "ftran": lambda: s.basis_solve(rng.standard_normal((16, ncons))),
           "btran": lambda: s.basis_solve(rng.standard_normal((16, m)), transpose=True)}
    cert = sorted(s.certificate()["device_ms"] for _ in range(a.reps + 1))[a.reps // 2]
    out = {"instance": "gen_sparse_lp(100000, 100000, 100, 4), basis after 240 000 pivots", "nucleus": int(s.stats()["nucleus_size"]),
           "reps": a.reps, "certificate_device_ms": cert, "ops": {}}
    for name, fn in ops.items():
        fn()
        ms, info = [], None
        for _ in range(a.reps):
            fn()
            info = s.tableau_info()
            ms.append(info["device_ms"])
        med = float(np.median(ms))
        out["ops"][name] = {"device_ms_per_batch": med, "bytes": info["bytes"], "GBps": info["bytes"] / med / 1e6, "nnz": info["nnz"],
                            "ratio_to_certificate": med / cert}
        print(name, out["ops"][name], flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
