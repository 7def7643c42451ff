"""Records what the bound and fixing mutators (fix_vars, set_var_bounds, unfix_vars, unfix_var) leave behind, bit
for bit, on small instances of the bit-reproducible pull path: the bytes of objective(), SHA-1 of values() and of save_basis(2), and the
integer fields of the call's info struct.

    python tools/record_bound_moves.py [OUT.json]        (default: tests/golden/bound_moves_parent.json)

The committed file is the output of the commit BEFORE the kernels of fixing.inc / bounds.inc were merged;
tests/test_bound_moves_golden.py replays `record()` on the current tree and asserts equality of every field."""
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "bound_moves_parent.json")
LENGTHS = (1, 16, 17)
FIX_KINDS = ("shift", "value", "mixed")                                                  # tests/test_fixing.py::_request_lists
CASES = ("cover", "sparse-maximize", "mixed", "bounded", "pending-terms", "compact-factor")


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


def _case(name):
    """(lp, fresh, env): fresh() returns a new solution in the case's solved state."""
    from tests.test_bounds import BOUND_INSTANCES
    if name in BOUND_INSTANCES:
        gen, args = BOUND_INSTANCES[name]
        lp = gen(*args)
        s = lpgen.build_problem(M.Problem, lp).solve()
        return lp, s.clone, {}
    if name == "pending-terms":                                                          # a clone would fold the pending terms: solve anew
        from tests.test_gmi_cuts import _pending, _solved_with_pending_terms
        env = dict(MLP_LOWRANK="3")

        def fresh():
            s, lp, _ = _solved_with_pending_terms(lpgen.gen_sparse_lp(200, 150, 8, 3), True)
            assert _pending(s) > 0
            return s

        with _env(**env):
            _, lp, _ = _solved_with_pending_terms(lpgen.gen_sparse_lp(200, 150, 8, 3), True)
        return lp, fresh, env
    assert name == "compact-factor"
    env = dict(MLP_FACTOR="1")
    lp = lpgen.gen_transport_lp(600, 700, 4, 5, tight=0.45)
    with _env(**env):
        s = lpgen.build_problem(M.Problem, lp).solve()
    assert s.stats()["factor_active"] == 1
    return lp, s.clone, env


def _ints(info):
    return {k: int(v) for k, v in info.items() if isinstance(v, (int, np.integer)) and not isinstance(v, bool)}


def _state(s, info):
    return dict(objective=np.float64(s.objective()).tobytes().hex(), values=hashlib.sha1(s.values().tobytes()).hexdigest(),
                basis=hashlib.sha1(bytes(s.save_basis(2))).hexdigest(), info=_ints(info))


def _call(f, info_of):
    """The recorded state after f() (the solution it returns), or the verdict when the call says Infeasible."""
    try:
        t = f()
    except M.Infeasible:
        return None, dict(infeasible=True)
    return t, _state(t, info_of(t))


def record_case(name):
    from tests.test_bounds import bound_list
    from tests.test_fixing import _request_lists
    lp, fresh, env = _case(name)
    out = {}
    with _env(**env):
        s = fresh()
        vs, _ = s.basis_status()
        x = s.values()
        fixed16 = None
        for kind in FIX_KINDS:
            for k in LENGTHS:
                js, vals = _request_lists(lp, vs, x, kind, k)
                t, out["fix_vars %s %d" % (kind, k)] = _call(lambda: fresh().fix_vars(js, vals), lambda t: t.fix_info())
                if kind == "shift" and k == 16:
                    fixed16 = (t, js)
        for k in LENGTHS:
            js, los, his = bound_list(lp, x, vs, "mixed", k)
            _, out["set_var_bounds mixed %d" % k] = _call(lambda: fresh().set_var_bounds(js, los, his), lambda t: t.bounds_info())
        if fixed16[0] is not None:
            t, js = fixed16
            _, out["unfix_vars of the 16 shifted"] = _call(lambda: t.unfix_vars(js)[0], lambda t: t.fix_info())
        js, vals = _request_lists(lp, vs, x, "value", 1)                                 # one variable fixed at the bound it sits at
        t = fresh().fix_vars(js, vals)
        _, out["unfix_var"] = _call(lambda: t.unfix_var(js[0])[0], lambda t: t.fix_info())      # (the single form reports nothing: fix_vars' info stays)
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
