"""Records what Engine::run_loop ("Where the batch is decided") leaves behind after every call of a solve, on small
instances that between them take every branch of the batch policy: graphs of several iterations, the split of a batch into long and
short graphs, eager iterations, a pivot budget, the sampled (event-bracketed) iterations of profile mode, the hypersparse kernel and its
back-off, the primal head's slot room, k_small_basis, pending rank-1 terms, the compact factor's room and the switch to it.

    python tools/record_batches.py [OUT.json]        (default: tests/golden/batch_plan_parent.json; two recordings, merged)
    python tools/record_batches.py --raw RAW.json | --merge RAW1.json RAW2.json [OUT.json]      (the two recordings as two processes)

After each call: SHA-1 of [t[:5] for t in trace()], the bytes of objective(), SHA-1 of values() and of save_basis(2), budget_exhausted,
every integer field of stats(), the bytes of its *_bytes doubles (functions of shapes, not of time) and the state() keys of STATE.  Times
are not recorded.  The committed file is the output of the commit BEFORE BatchPlan (csrc/batch.h); tests/test_batch_golden.py replays
`record_case` on the current tree and asserts equality of every field the file holds."""
import contextlib
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import minilp_amd as M                                                                   # noqa: E402
from minilp_amd import lpgen                                                             # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "batch_plan_parent.json")
STATE = ("small_basis_launches", "primal_head_launches", "dual_list_tests", "fpull", "hyper_bail_reasons", "lowrank_pending")

_SPARSE = (lpgen.gen_sparse_lp, (700, 600, 12, 6), {})
_COVER = (lpgen.gen_cover_lp, (700, 900, 12, 5), {})
_FREE = dict(MLP_HYPER="0", MLP_DETERMINISTIC="0")                                       # (the pushed F product: the primal head's regime)
_SOLVE = (("solve", {}),)
# name -> (generator, its arguments, its keywords), environment, calls: ("solve", keywords) first, then ("continue", budget) / ("sampling", flag)
CASES = {
    "graphs": (_SPARSE, dict(MLP_HYPER="0"), _SOLVE),
    "graph split": (_SPARSE, dict(MLP_HYPER="0", MLP_BATCH="5", MLP_GRAPH_ITERS="3"), _SOLVE),
    "eager": (_SPARSE, dict(MLP_HYPER="0", MLP_NO_GRAPH="1"), _SOLVE),
    "budget": (_SPARSE, dict(MLP_HYPER="0"), (("solve", dict(budget=7)), ("continue", 40), ("continue", 1), ("continue", -1))),
    "sampled": (_SPARSE, dict(MLP_HYPER="0"), (("solve", dict(profile=True)),)),
    "sampled each": (_SPARSE, dict(MLP_HYPER="0"), (("solve", dict(budget=0, profile=True)), ("sampling", True), ("continue", 25))),
    "hypersparse": (_COVER, dict(MLP_HYPER="1"), _SOLVE),
    "back-off": (_COVER, dict(MLP_HYPER="1", MLP_HYPER_HEAVY="2"), _SOLVE),
    "head outgrown": ((lpgen.gen_sparse_lp, (2500, 2000, 10, 4), {}), _FREE, _SOLVE),
    "head room": (_SPARSE, dict(_FREE, MLP_PRIMAL_HEAD_K="6"), _SOLVE),
    "small basis": ((lpgen.gen_sparse_lp, (3000, 2600, 12, 9), {}), dict(MLP_HYPER="0"), _SOLVE),
    "pending terms": ((lpgen.gen_sparse_lp, (200, 150, 8, 3), {}), dict(MLP_LOWRANK="3"), (("solve", dict(budget=40)), ("continue", -1))),
    "factor": ((lpgen.gen_transport_lp, (600, 700, 4, 5), dict(tight=0.45)), dict(MLP_FACTOR="1"), _SOLVE),
    "factor switch": ((lpgen.gen_transport_lp, (1500, 1500, 4, 21), dict(tight=0.45)), dict(MLP_FACTOR_FROM="256", MLP_HYPER="0"), _SOLVE),
}
# the only fields two runs of one build may disagree on, and so the only ones a golden file may leave out (its "unstable" key)
MAY_BE_UNSTABLE = ("objective", "values", "basis")


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _sha(b):
    return hashlib.sha1(b).hexdigest()


def _snapshot(s):
    state = {k: [int(v) for v in s.state(k)] for k in STATE}                             # first: reading the basis blob folds the pending terms
    st = s.stats()
    ints = {k: int(v) for k, v in st.items() if isinstance(v, (int, np.integer)) and not isinstance(v, bool)}
    ints["kase"] = [int(v) for v in st["kase"]]
    return dict(trace=_sha(repr([tuple(int(v) for v in t[:5]) for t in s.trace()]).encode()),
                objective=np.float64(s.objective()).tobytes().hex(), values=_sha(np.ascontiguousarray(s.values()).tobytes()),
                basis=_sha(bytes(s.save_basis(2))), budget_exhausted=bool(s.budget_exhausted), stats=ints,
                bytes={k: np.float64(v).tobytes().hex() for k, v in st.items() if k.endswith("_bytes")},
                state=state)


def record_case(name):
    """The snapshots after each call of the case, in order."""
    (gen, args, kw), env, calls = CASES[name]
    lp = gen(*args, **kw)
    out = []
    with _env(**env):
        s = None
        for what, arg in calls:
            if what == "solve":
                s = lpgen.build_problem(M.Problem, lp).solve(trace=True, **arg)
            elif what == "continue":
                s.continue_solve(arg)
            else:
                s.set_sampling(arg)
                continue                                                                 # (a switch, not a run: the next call shows it)
            out.append(dict(_snapshot(s), call="%s %r" % (what, arg)))
    return out


def record():
    return {name: record_case(name) for name in CASES}


def merge(a, b):
    """One golden file from two recordings of one build: the fields of MAY_BE_UNSTABLE the two disagree on are left out and listed under
    "unstable" (only in a case run with MLP_DETERMINISTIC=0: float atomics); any other disagreement is an error."""
    unstable = []
    for name in CASES:
        assert len(a[name]) == len(b[name]), name
        for i, (x, y) in enumerate(zip(a[name], b[name])):
            for k in sorted(x):
                if x[k] == y[k]:
                    continue
                if k not in MAY_BE_UNSTABLE or CASES[name][1].get("MLP_DETERMINISTIC") != "0":
                    raise AssertionError("two runs of one build disagree on %s[%d].%s: %r against %r" % (name, i, k, x[k], y[k]))
                unstable.append([name, i, k])
                del x[k]
    return dict(cases=a, unstable=unstable)


def _dump(rec, path):
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--raw"]:                                                       # one recording, unmerged: for two processes
        _dump(record(), sys.argv[2])
        sys.exit(0)
    if sys.argv[1:2] == ["--merge"]:                                                     # --merge RAW1 RAW2 [OUT.json]
        rec = merge(json.load(open(sys.argv[2])), json.load(open(sys.argv[3])))
        path = sys.argv[4] if len(sys.argv) > 4 else GOLDEN
    else:
        rec = merge(record(), record())
        path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    _dump(rec, path)
    print("%d cases, %d calls, unstable: %s -> %s" % (len(rec["cases"]), sum(len(c) for c in rec["cases"].values()), rec["unstable"], path))
