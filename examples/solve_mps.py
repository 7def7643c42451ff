#!/usr/bin/env python3
"""solve_mps — counterpart of the reference's examples/solve_mps.rs (19-43): read a free-format MPS file,
minimise, print the objective and the non-zero variables.

    python examples/solve_mps.py model.mps [--max] [--all] [--ranging] [--tableau VAR] [--gomory-rounds K]
                                 [--gmi-rounds K [--continuous NAME,...]] [--branch-penalties [--continuous NAME,...]]
                                 [--cutoff VALUE [--tighten] [--continuous NAME,...]] [--rhs-sweep ROW:FROM:TO:STEPS]

--ranging adds a sensitivity table: per variable its value, basis status, reduced cost and cost range; per row its dual value and
rhs range (rows in file order).  --tableau VAR prints the tableau row of the basic variable VAR (by name): its non-zero coefficients on the
non-basic variables and on the slacks of the rows, the raw material of a mixed-integer cut.  --gomory-rounds K adds K rounds of Gomory cuts, each over all basic structural variables with a
fractional value (|x - round x| > 1e-6) in one add_gomory_cuts call, and prints the bound and the call's counters after each round.
That cut is valid only for a pure integer model with integer slacks whose non-basic columns sit at a zero lower bound.  --gmi-rounds K adds
K rounds of Gomory mixed-integer cuts instead (one add_gmi_cuts call per round over the basic integer variables with a fractional value):
every structural variable is integer unless listed in --continuous, the slacks are continuous; it prints the bound, the cuts emitted and
skipped and the counters after each round.  --branch-penalties prints, for every basic structural variable with a fractional value at the
LP optimum, the one-pivot bounds of its down and up branch (plain, and with Tomlin's strengthening: every structural variable is integer
unless listed in --continuous, the slacks are continuous), the child bounds they give and the columns that would enter.  --cutoff VALUE
prints the bounds that the reduced costs imply once an incumbent of objective VALUE is known (Solution.cutoff_bounds; every structural
variable is integer unless listed in --continuous): per tightened variable its bounds and whether it can be fixed.  --tighten then applies
all of them to the solution on the device (Solution.tighten_by_reduced_cost) and prints the count and the objective, which does not move.
--rhs-sweep ROW:FROM:TO:STEPS moves the right-hand side of row ROW (its number in file order) from FROM to TO in STEPS equal steps: first
ONE Solution.rhs_scenarios call prints, per step, the value of the current dual solution there and whether the current basis stays
feasible; then a chain of Solution.set_rhs calls, each from the basis of the step before, prints the optimum and the pivots of every step.

Runs on the MI355X engine (libminilp_hip.so); there is no CPU back end.  `run(B, ...)` takes the module that
provides the reference's API so that the tests can drive the same code with their checker."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(B, path, maximize=False, show_all=False, ranging=False, gomory_rounds=0, tableau=None, gmi_rounds=0, continuous=(), branch_penalties=False, cutoff=None, tighten=False,
        propagate=False, rhs_sweep=None):
    text = open(path).read()
    t0 = time.time()
    f = B.MpsFile(text, B.MAXIMIZE if maximize else B.MINIMIZE)  # MpsFile::parse (mps.rs:39)
    t1 = time.time()
    try:
        sol = f.problem.solve()
    except B.Infeasible:
        print("problem %s: infeasible" % f.problem_name)
        return 1
    except B.Unbounded:
        print("problem %s: unbounded" % f.problem_name)
        return 1
    t2 = time.time()
    print("problem %s: %d variables, parsed in %.3fs, solved in %.3fs" % (f.problem_name, len(f.variables), t1 - t0, t2 - t1))
    print("objective: %.12g" % sol.objective())
    x = sol.values()
    for name, var in sorted(f.variables.items(), key=lambda kv: kv[1]):
        if show_all or x[var] != 0.0:
            print("%s = %.12g" % (name, x[var]))
    if ranging:
        tag = ["basic", "lower", "upper", "free", "fixed"]
        vs, cs = sol.basis_status()
        r, (clo, chi) = sol.reduced_costs(), sol.cost_ranging()
        pi, (rlo, rhi) = sol.dual_values(), sol.rhs_ranging()
        print("%-12s %14s %-6s %14s   %s" % ("variable", "value", "status", "reduced cost", "cost range"))
        for name, var in sorted(f.variables.items(), key=lambda kv: kv[1]):
            print("%-12s %14.8g %-6s %14.8g   [%.8g, %.8g]" % (name, x[var], tag[vs[var]], r[var], clo[var], chi[var]))
        print("%-12s %-6s %14s   %s" % ("row", "status", "dual value", "rhs range"))
        for c in range(sol.num_constraints):
            print("%-12d %-6s %14.8g   [%.8g, %.8g]" % (c, tag[cs[c]], pi[c], rlo[c], rhi[c]))
    if tableau is not None:
        if tableau not in f.variables:
            print("tableau: no variable named %s" % tableau)
            return 1
        var = f.variables[tableau]
        if var not in sol.basis_head():
            print("tableau: %s is not basic (value %.12g)" % (tableau, x[var]))
            return 1
        names = {v: n for n, v in f.variables.items()}
        ip, ix, dv = sol.tableau_rows([var])
        print("tableau row of %s (= %.12g):" % (tableau, x[var]))
        for col, a in zip(ix, dv):
            print("  %-12s %.12g" % (names[col] if col < len(x) else "slack(row %d)" % (col - len(x)), a))
    if branch_penalties:
        unknown = [nm for nm in continuous if nm not in f.variables]
        if unknown:
            print("branch penalties: no variable named %s" % ", ".join(unknown))
            return 1
        marks = [True] * len(f.variables)
        for nm in continuous:
            marks[f.variables[nm]] = False
        names = {v: n for n, v in f.variables.items()}
        col = lambda c: "-" if c < 0 else (names[c] if c < len(x) else "slack(row %d)" % (c - len(x)))
        plain, strong = sol.branch_penalties(range(len(x))), sol.branch_penalties(range(len(x)), marks)
        sg = -1.0 if maximize else 1.0
        obj = sol.objective()
        rows = [v for v in range(len(x)) if plain["status"][v] == 0]
        print("branch penalties of %d fractional basic variables (objective %.12g), %s" % (len(rows), obj, sol.branch_info()))
        print("%-12s %12s %14s %14s %14s %14s %14s %14s   %s" % ("variable", "fraction", "down", "up", "down (int)", "up (int)",
                                                                  "bound down", "bound up", "entering (down, up)"))
        for v in rows:
            print("%-12s %12.8g %14.8g %14.8g %14.8g %14.8g %14.8g %14.8g   %s, %s" %
                  (names[v], plain["frac"][v], plain["down"][v], plain["up"][v], strong["down"][v], strong["up"][v],
                   obj + sg * plain["down"][v], obj + sg * plain["up"][v], col(plain["down_col"][v]), col(plain["up_col"][v])))
    if cutoff is not None:
        unknown = [nm for nm in continuous if nm not in f.variables]
        if unknown:
            print("cutoff: no variable named %s" % ", ".join(unknown))
            return 1
        marks = [True] * len(f.variables)
        for nm in continuous:
            marks[f.variables[nm]] = False
        names = {v: n for n, v in f.variables.items()}
        cv, clo, chi, pruned = sol.cutoff_bounds(cutoff, marks)
        if pruned:
            print("cutoff %.12g: the LP bound %.12g is already worse, nothing to tighten" % (cutoff, sol.objective()))
        else:
            print("cutoff %.12g: %d variables tightened, %d of them fixed, %s" % (cutoff, len(cv), int((clo == chi).sum()), sol.fix_info()))
            if tighten:
                sol, count, _ = sol.tighten_by_reduced_cost(cutoff, marks)
                print("tightened: %d bounds applied on the device, objective %.12g unchanged, %s" % (count, sol.objective(), sol.bounds_info()))
            print("%-12s %14s %14s   %s" % ("variable", "lower", "upper", ""))
            for v, a, b in zip(cv, clo, chi):
                print("%-12s %14.8g %14.8g   %s" % (names[int(v)], a, b, "fixed" if a == b else ""))
    if propagate:  # the bounds that the rows imply (no variable is taken as integer), applied to the solution
        try:
            sol, count, infeasible = sol.tighten_by_propagation()
        except B.Infeasible:
            print("propagation: the tightened model is infeasible")
            return 1
        if infeasible:
            print("propagation: the rows prove the model infeasible, %s" % sol.propagate_info())
            return 1
        print("propagation: %d variables tightened, objective %.12g, %s %s" % (count, sol.objective(), sol.propagate_info(), sol.bounds_info()))
    if rhs_sweep is not None:
        try:
            row, lo, hi, steps = rhs_sweep.split(":")
            row, lo, hi, steps = int(row), float(lo), float(hi), int(steps)
            if not (0 <= row < sol.num_constraints and steps >= 1):
                raise ValueError(rhs_sweep)
        except ValueError:
            print("rhs sweep: expected ROW:FROM:TO:STEPS with a row below %d" % sol.num_constraints)
            return 1
        grid = [lo + (hi - lo) * t / max(1, steps - 1) for t in range(steps)]
        if steps > 1:
            grid[-1] = hi
        res = sol.rhs_scenarios([row], [[v] for v in grid])
        print("rhs sweep of row %d (now %.12g), %s" % (row, sol.constraint_rhs([row])[0], sol.rhs_info()))
        for v, bound, ok in zip(grid, res["bound"], res["feasible"]):
            print("what-if  row %d = %r: bound %.12g %s" % (row, v, bound, "feasible" if ok else "pivots needed"))
        for v in grid:
            try:
                sol = sol.set_rhs([row], [v])
            except B.Infeasible:
                print("set_rhs  row %d = %r: infeasible" % (row, v))
                return 0
            print("set_rhs  row %d = %r: optimum %.12g, %d pivots" % (row, v, sol.objective(), sol.rhs_info()["pivots"]))
    for k in range(gomory_rounds):
        x = sol.values()
        vs, _ = sol.basis_status()
        frac = [v for v in range(len(x)) if vs[v] == 0 and abs(x[v] - round(x[v])) > 1e-6]
        if not frac:
            print("gomory round %d: no fractional basic variable" % (k + 1))
            break
        try:
            sol = sol.add_gomory_cuts(frac)
        except B.Infeasible:
            print("gomory round %d: infeasible" % (k + 1))
            return 1
        print("gomory round %d: %d cuts, bound %.12g, %s" % (k + 1, len(frac), sol.objective(), sol.cut_info()))
    if gmi_rounds:
        unknown = [nm for nm in continuous if nm not in f.variables]
        if unknown:
            print("gmi: no variable named %s" % ", ".join(unknown))
            return 1
        is_int = [True] * len(f.variables)
        for nm in continuous:
            is_int[f.variables[nm]] = False
    for k in range(gmi_rounds):
        x = sol.values()
        vs, _ = sol.basis_status()
        frac = [v for v in range(len(x)) if is_int[v] and vs[v] == 0 and abs(x[v] - round(x[v])) > 1e-6]
        if not frac:
            print("gmi round %d: no fractional basic integer variable" % (k + 1))
            break
        try:
            sol, status = sol.add_gmi_cuts(frac, is_int)
        except B.Infeasible:
            print("gmi round %d: infeasible" % (k + 1))
            return 1
        status = list(status)
        print("gmi round %d: %d cuts emitted, %d skipped (fraction) + %d skipped (free column), bound %.12g, %s %s" %
              (k + 1, status.count(0), status.count(1), status.count(2), sol.objective(), sol.gmi_info(), sol.cut_info()))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("file")
    ap.add_argument("--max", action="store_true", help="maximise instead of minimise (solve_mps.rs:32 minimises)")
    ap.add_argument("--all", action="store_true", help="print zero-valued variables too")
    ap.add_argument("--ranging", action="store_true", help="print the sensitivity table (status, reduced costs, duals, cost and rhs ranges)")
    ap.add_argument("--gomory-rounds", type=int, default=0, metavar="K",
                    help="K rounds of Gomory cuts over the fractional basic variables (one add_gomory_cuts call per round)")
    ap.add_argument("--tableau", metavar="VAR", help="print the tableau row of the basic variable VAR (by name)")
    ap.add_argument("--gmi-rounds", type=int, default=0, metavar="K",
                    help="K rounds of Gomory mixed-integer cuts over the fractional basic integer variables (one add_gmi_cuts call per round)")
    ap.add_argument("--continuous", default="", metavar="NAME,...",
                    help="with --gmi-rounds / --branch-penalties / --cutoff: the variables that are NOT integer (all others are; slacks are continuous)")
    ap.add_argument("--branch-penalties", action="store_true",
                    help="print the one-pivot branching bounds of the fractional basic variables (Solution.branch_penalties)")
    ap.add_argument("--cutoff", type=float, default=None, metavar="VALUE",
                    help="print the bounds the reduced costs imply for an incumbent of objective VALUE (Solution.cutoff_bounds)")
    ap.add_argument("--tighten", action="store_true",
                    help="with --cutoff: apply the listed bounds to the solution (Solution.tighten_by_reduced_cost)")
    ap.add_argument("--propagate", action="store_true",
                    help="tighten the bounds by propagation over the rows (Solution.tighten_by_propagation) and print the count and the counters")
    ap.add_argument("--rhs-sweep", default=None, metavar="ROW:FROM:TO:STEPS",
                    help="move the right-hand side of row ROW from FROM to TO: one Solution.rhs_scenarios call, then a chain of Solution.set_rhs calls")
    a = ap.parse_args()
    import minilp_amd as B
    return run(B, a.file, a.max, a.all, a.ranging, a.gomory_rounds, a.tableau, a.gmi_rounds, [nm for nm in a.continuous.split(",") if nm],
               a.branch_penalties, a.cutoff, a.tighten, a.propagate, a.rhs_sweep)


if __name__ == "__main__":
    sys.exit(main())
