"""GPU: parity with the oracle on models with more than 524 288 rows or columns.

Every grid-wide kernel launched through grid_for() (csrc/kernels.hip) gets at most 512 workgroups of 256 threads with 4 elements per
thread: 524 288 elements.  Below that size a kernel's stride loop makes one trip per thread, the fused one-launch forms of the Harris
tests are chosen and the kernels that hold PT = 4 positions per thread in registers see all of their input.  Above it other code runs:
the later trips of every stride loop, the two-launch Harris test (k_ratio_primal_p1 / _p2), the size guards themselves, dozens of bands
in the banded sweep, reductions over hundreds of thousands of per-block partials.  The rest of the suite stops at 160 000; here five
instances of the committed generators with 560 000 .. 900 000 rows / columns are solved for a fixed budget beside the oracle:

  tall       gen_sparse_lp(700000, 60000, 4, 51)                      primal loop only
  wide       gen_cover_lp(60000, 700000, 12, 52)                      dual loop only
  cover4     gen_cover_lp(560000, 600000, 4, 55)                      dual loop only, 4 non-zeros per row
  twophase   gen_twophase_lp(600000, 560000, 20, 53, ge_every=2000)   1.2e7 non-zeros: dual loop on the artificial objective, primal loop
  transport  gen_transport_lp(300000, 300000, 3, 54, tight=0.5)       584 999 x 900 000, two entries per column

The contract is the suite's own: identical t[:5] traces, OBJ_RTOL = 1e-9, X_ATOL = 1e-7 (tests/common.py), stage RTOL = 1e-11
(tests/test_stage_parity.py), the KKT terms of tests/test_duals.py::check_kkt.  Each case also asserts the FORM that ran (banded sweep,
hypersparse iteration, compact factor, the two-launch Harris test), so that a change which routes these sizes back to a small-model
kernel fails here instead of passing.  The LPs, the oracle's runs and the engine's runs are built once per module."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import minilp_amd as M
from minilp_amd import lpgen
from oracle import minilp_oracle as O
from tests.common import ROOT, X_ATOL, obj_close
from tests.test_duals import _extend, check_kkt
from tests.test_stage_parity import _step_and_compare

pytestmark = pytest.mark.gpu

CAP = 4 * 256 * 512   # elements one trip of a grid_for() grid covers (kernels.hip: grid_for, BLK = 256, 4 per thread, 512 blocks)
B = 3000              # pivots per case of the parity runs (the oracle takes 1.4 .. 21 s for them, single thread)
INSTANCES = {
    "tall": lambda: lpgen.gen_sparse_lp(700000, 60000, 4, 51),
    "wide": lambda: lpgen.gen_cover_lp(60000, 700000, 12, 52),
    "cover4": lambda: lpgen.gen_cover_lp(560000, 600000, 4, 55),
    "twophase": lambda: lpgen.gen_twophase_lp(600000, 560000, 20, 53, ge_every=2000),
    "transport": lambda: lpgen.gen_transport_lp(300000, 300000, 3, 54, tight=0.5),
}
# the large-nucleus machinery as tests/test_lowrank.py and test_stage_parity.py force it on small instances
BIG = dict(MLP_LOWRANK="3", MLP_BIGTILE="1", MLP_LDPAD="16", MLP_BANDED="1", MLP_STR_K="0")
# what the engine's parity run of a case is forced to (section 1); everything else is the default at that size
FORCED = {"tall": {}, "wide": {"MLP_BANDED": "1"}, "cover4": {}, "twophase": {}, "transport": {"MLP_FACTOR": "1"}}


class _Runs:
    """The instances, the oracle's problems / budget-B solutions and the engine's budget-B solutions, each built on first use."""

    def __init__(self):
        self.lp, self.oprob, self.osol, self.gsol = {}, {}, {}, {}

    def instance(self, name):
        if name not in self.lp:
            self.lp[name] = INSTANCES[name]()
        return self.lp[name]

    def oracle_problem(self, name):
        if name not in self.oprob:
            self.oprob[name] = lpgen.build_problem(O.Problem, self.instance(name))
        return self.oprob[name]

    def oracle(self, name):
        if name not in self.osol:
            t = time.perf_counter()
            self.osol[name] = self.oracle_problem(name).solve(budget=B, trace=True)
            print(f"[{name}] oracle: {B} pivots in {time.perf_counter() - t:.1f} s")
        return self.osol[name]

    def engine(self, name):
        if name not in self.gsol:
            with pytest.MonkeyPatch.context() as mp:
                for k, v in FORCED[name].items():
                    mp.setenv(k, v)
                self.gsol[name] = _engine_run(self.instance(name), B, name)
        return self.gsol[name]


def _engine_run(lp, budget, tag):
    t = time.perf_counter()
    prob = lpgen.build_problem(M.Problem, lp)
    t1 = time.perf_counter()
    s = prob.solve(budget=budget, trace=True)
    print(f"[{tag}] engine: build {t1 - t:.1f} s, {budget} pivots in {time.perf_counter() - t1:.1f} s")
    return s


@pytest.fixture(scope="module")
def runs():
    r = _Runs()
    yield r
    r.gsol.clear()
    r.osol.clear()
    r.oprob.clear()


def _same_run(sg, so, n=None):
    """The suite's contract between an engine run and an oracle run of the same budget."""
    tg, to = [t[:5] for t in sg.trace()], [t[:5] for t in so.trace()]
    diff = next((i for i, (a, b) in enumerate(zip(tg, to)) if a != b), None)
    assert diff is None, (diff, tg[diff], to[diff])
    assert len(tg) == len(to) and (n is None or len(tg) >= n), (len(tg), len(to), n)
    assert obj_close(sg.objective(), so.objective()), (sg.objective(), so.objective())
    dx = float(np.abs(sg.values() - so.values()).max())
    assert dx <= X_ATOL, dx


# ------------------------------------------------------------------------------------------------ 1. pivot for pivot past the cap
@pytest.mark.parametrize("name", list(INSTANCES))
def test_pivot_for_pivot_past_the_grid_cap(runs, name):
    """B = 3 000 pivots of each family with a dimension above 524 288: the oracle's sequence, objective and point — and the proof that
    the run left the small-model code (see the module docstring)."""
    lp = runs.instance(name)
    assert max(lp["m"], lp["n"]) > CAP
    so, sg = runs.oracle(name), runs.engine(name)
    _same_run(sg, so, n=B - 1)
    st = sg.stats()
    assert st["bound_flips"] == 0 and sg.budget_exhausted
    form = {}
    if name == "tall":
        assert lp["m"] > CAP and st["dual_iters"] == 0 and st["primal_iters"] >= B - 1
        # the Harris test over the m basic positions: neither the one-block form nor the fused grid (PT = 4 positions per thread of at
        # most 512 blocks) can hold 700 000 positions — launch_ratio_primal takes pass 1 and pass 2 as two launches with stride loops
        form["ratio_primal_form"] = int(sg.state("ratio_primal_form")[0])
        assert form["ratio_primal_form"] == 2
        form["primal_head_launches"] = int(sg.state("primal_head_launches")[0])
        form["small_basis_launches"] = int(sg.state("small_basis_launches")[0])
    if name == "wide":
        assert lp["n"] > CAP and st["primal_iters"] == 0 and st["dual_iters"] >= B - 1
        assert st["banded_sweep"] == 1 and st["hyper_iters"] == 0     # (forced: the banded sweep under the multi-kernel dual iteration)
    if name == "cover4":
        assert min(lp["m"], lp["n"]) > CAP and st["primal_iters"] == 0
        assert st["hyper_iters"] > 0                                   # the hypersparse iteration takes it by default
        form["hyper_bails"] = st["hyper_bails"]
    if name == "twophase":
        assert min(lp["m"], lp["n"]) > CAP and st["dual_iters"] > 100 and st["primal_iters"] > 1000
        assert st["banded_sweep"] == 1                                 # the auto rule: m >= 32 768 and nnz >= 2^22
    if name == "transport":
        assert min(lp["m"], lp["n"]) > CAP
        assert st["factor_active"] == 1
        form["factor_refactors"] = st["factor_refactors"]
    print(name, {k: st[k] for k in ("primal_iters", "dual_iters", "nucleus_size", "banded_sweep", "hyper_iters", "factor_active")}, form)


def test_multi_kernel_dual_iteration_at_600000_columns(runs, monkeypatch):
    """The 4-per-row cover instance again with the hypersparse iteration switched off: k_price_dual, the dual Harris test (grid or list
    form) and k_sweep walk n = 600 000 columns and m = 560 000 rows."""
    monkeypatch.setenv("MLP_HYPER", "0")
    sg = _engine_run(runs.instance("cover4"), B, "cover4, MLP_HYPER=0")
    _same_run(sg, runs.oracle("cover4"), n=B - 1)
    st = sg.stats()
    assert st["hyper_iters"] == 0 and st["dual_iters"] >= B - 1
    print("dual Harris tests over the listed non-zeros / pauses of the listing:", sg.state("dual_list_tests").tolist())


# ------------------------------------------------------------------------------------------------ 2. every stage at that size
@pytest.mark.parametrize("name,start", [("tall", 0), ("cover4", 0), ("twophase", 320)])
def test_every_stage_matches_the_oracle_past_the_grid_cap(runs, name, start):
    """40 stepped iterations with alpha_q, rho, alpha_r, tau, v, x_B, d, x_N, beta, gamma compared element by element (RTOL = 1e-11): a
    vector whose tail beyond element 524 288 was never written cannot pass, whatever the pivot sequence does.  The two-phase instance is
    stepped from pivot 320, behind its phase switch (pivot 306), so that the primal stages run."""
    n, worst, phases = _step_and_compare(runs.instance(name), 40, start=start)
    assert n == 40, n
    assert phases == ({1} if name == "cover4" else {0}), phases
    print(name, n, "iterations; worst relative differences:", {k: f"{v:.1e}" for k, v in worst.items()})


# ------------------------------------------------------------------------------------------------ 3. the forms that replace the fused ones
@pytest.mark.parametrize("two_kernels", [False, True], ids=["default ratio form", "MLP_RATIO_TWO_KERNELS=1"])
@pytest.mark.parametrize("fpull", ["1", "0"], ids=["MLP_FPULL=1", "MLP_FPULL=0"])
def test_large_nucleus_machinery_with_700000_rows(runs, monkeypatch, fpull, two_kernels):
    """The delayed-update mode, the 16-row tiles, the padded pitch, the blocked F push and the banded sweep forced on the tall instance:
    600 pivots, the oracle's sequence.  The pulled F product holds PT = 4 positions per thread of at most 512 blocks in its second
    launch: with m = 700 000 the engine must DECLINE it (state("fpull")[3] == 0) and run the pushed product with the two-launch Harris
    test, whether MLP_FPULL asks for the pull or not."""
    for k, v in dict(BIG, MLP_FPULL=fpull).items():
        monkeypatch.setenv(k, v)
    if two_kernels:
        monkeypatch.setenv("MLP_RATIO_TWO_KERNELS", "1")
    so = runs.oracle_problem("tall").solve(budget=600, trace=True)
    sg = _engine_run(runs.instance("tall"), 600, f"tall, large-nucleus machinery, MLP_FPULL={fpull}")
    fp = sg.state("fpull").tolist()
    print("pulled F product [packed copy kept, builds, built at pivot, pull supported]:", fp,
          "-> the engine declined the pull, the pushed product ran" if not fp[3] else "-> the pull ran")
    _same_run(sg, so, n=600)
    st = sg.stats()
    assert st["banded_sweep"] == 1 and st["primal_iters"] == 600
    assert fp[3] == 0.0 and int(sg.state("ratio_primal_form")[0]) == 2
    assert int(sg.state("primal_head_launches")[0]) == 0 and int(sg.state("small_basis_launches")[0]) == 0
    if fpull == "0":
        assert fp[0] == 0.0


# ------------------------------------------------------------------------------------------------ 4. sharded, m > 524 288
def test_sharded_large_nucleus_machinery_with_700000_rows():
    """Two ranks on one device (tools/shard_test.py, sharded from the first pivot), a 700 000 x 60 000 instance, the machinery of the
    test above forced, so that shard_world > 1 && lrJ > 0 && pb_on && !det_pull && rowinfo holds: the arm of Engine::launch_stage that
    took the pulled F product WITHOUT asking whether pass 2 of its Harris test (k_fpull_p2: 4 positions per thread, 512 blocks, no
    stride loop) covers every basic position.  200 pivots: both ranks take the unsharded engine's pivots, and the ranks report that
    the pull is declined at this size (fpull_supported: grid_for(m) * BLK * 4 >= m)."""
    env = dict(os.environ, **BIG)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "shard_test.py"), "2", "700000", "60000", "4", "200"],
                       capture_output=True, text=True, timeout=900, env=env)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "traces identical: True" in r.stdout
    assert "sharding live after the probe / at the end: None / 1" in r.stdout
    assert "pulled F product supported on the sharded ranks: [0, 0]" in r.stdout, r.stdout[-1500:]


# ------------------------------------------------------------------------------------------------ 5. reads and warm starts
def test_certificate_on_the_two_phase_run_and_no_warm_start_from_an_unsolved_model(runs):
    """On the two-phase run after B pivots (primal loop, not optimal): the device certificate against the host formula with
    m = 600 000 and n = 560 000 (k_du_*).  A warm start from this state is refused by the reference (solver.rs:555-556 asserts a
    solved model) — by the oracle and by the engine alike; the warm starts at this size are in the next test, from an optimum."""
    lp = runs.instance("twophase")
    sg = runs.engine("twophase")
    scale = max(1.0, float(np.abs(lp["obj"]).max()))
    cert = check_kkt(lp, sg, optimal=False)
    assert cert["btran_residual"] <= 1e-9 * scale, cert
    print("two-phase certificate:", {k: cert[k] for k in ("primal_objective", "dual_objective", "btran_residual", "device_ms")})
    with pytest.raises(O.OraclePanic, match="not solved"):
        runs.oracle("twophase").clone().add_constraint([(0, 1.0), (1, 1.0)], O.LE, 1.0)
    with pytest.raises(M.InternalError, match="not solved"):
        sg.clone().add_constraint([(0, 1.0), (1, 1.0)], M.LE, 1.0)


def test_warm_starts_with_700000_columns(runs, monkeypatch):
    """The wide instance (60 000 x 700 000, banded sweep forced) continued to its optimum on both sides (60 013 pivots, 57 s of the
    oracle): the optimality certificate, then one <= row over four variables appended on both sides (row append, rebuild of the
    band-major copy with n > 524 288) as tests/test_sweep_order.py does it, then clone() + fix_var."""
    for k, v in FORCED["wide"].items():
        monkeypatch.setenv(k, v)
    lp = runs.instance("wide")
    so, sg = runs.oracle("wide").clone(), runs.engine("wide").clone()
    t = time.perf_counter()
    so.continue_solve(-1)
    t1 = time.perf_counter()
    sg.continue_solve(-1)
    print(f"[wide] to the optimum: oracle {t1 - t:.1f} s, engine {time.perf_counter() - t1:.1f} s, {sg.stats()['iterations']} iterations")
    assert not so.budget_exhausted and not sg.budget_exhausted and sg.stats()["banded_sweep"] == 1
    assert obj_close(sg.objective(), so.objective()), (sg.objective(), so.objective())
    assert float(np.abs(sg.values() - so.values()).max()) <= X_ATOL
    check_kkt(lp, sg)
    opt = sg.objective()
    x = so.values()
    vars_ = sorted(int(j) for j in np.argsort(-x, kind="stable")[:4])
    lhs = float(sum(x[v] for v in vars_))
    assert lhs > 0.1
    expr, rhs = [(v, 1.0) for v in vars_], 0.9 * lhs + 0.01
    so, sg = so.add_constraint(expr, O.LE, rhs), sg.add_constraint(expr, M.LE, rhs)
    assert obj_close(sg.objective(), so.objective()), (sg.objective(), so.objective())
    assert float(np.abs(sg.values() - so.values()).max()) <= X_ATOL
    assert sg.num_constraints == lp["m"] + 1 and sg.stats()["banded_sweep"] == 1
    check_kkt(_extend(lp, vars_, [1.0] * 4, lpgen.LE, rhs), sg)
    fx = int(np.argmax(so.values()))
    co, cg = so.fix_var(fx, 0.0), sg.clone().fix_var(fx, 0.0)
    assert obj_close(cg.objective(), co.objective()), (cg.objective(), co.objective())
    assert float(np.abs(cg.values() - co.values()).max()) <= X_ATOL
    print("objective at the optimum / with the row / with the variable fixed:", opt, sg.objective(), cg.objective())


def test_certificate_on_the_compact_factor_of_the_transport_run(runs):
    """The transport run after B pivots on the compact factor (584 999 x 900 000): the device certificate against the host formula."""
    lp, sg = runs.instance("transport"), runs.engine("transport")
    assert sg.stats()["factor_active"] == 1
    cert = check_kkt(lp, sg, optimal=False)
    print("transport certificate:", {k: cert[k] for k in ("primal_objective", "dual_objective", "btran_residual", "device_ms")})
