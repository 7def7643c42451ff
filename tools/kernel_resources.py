#!/usr/bin/env python3
"""Compiler report of the kernels' resources, without a GPU: compiles minilp_amd/csrc/kernels.hip device-only for gfx950 with the flags of
minilp_amd/build.py plus -Rpass-analysis=kernel-resource-usage and prints, per kernel, VGPRs, SGPR spills, VGPR spills, ScratchSize,
LDS and occupancy.  Nothing but these numeric remarks is read.

    python tools/kernel_resources.py --match k_update_pivot                    # table of the matching kernels
    python tools/kernel_resources.py --match k_update_pivot --json parent.json # ... and the figures as JSON (run on the parent's tree)
    python tools/kernel_resources.py --match k_update_pivot --parent parent.json --json profiles/update_forms_resources.json --check

--source names another kernels.hip (a checkout of the parent commit).  --check applies the requirements of the update kernel's forms:
every instance without scratch and without VGPR spill; the primal + PSE + lazy + banded instance within 104 VGPRs and 112 bytes of LDS.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from minilp_amd import build as mbuild  # noqa: E402

FIELDS = {"VGPRs": "vgprs", "AGPRs": "agprs", "TotalSGPRs": "sgprs", "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill",
          "ScratchSize [bytes/lane]": "scratch", "LDS Size [bytes/block]": "lds", "Occupancy [waves/SIMD]": "occupancy"}
NAME = re.compile(r"remark: Function Name: (\S+)")
FIELD = re.compile(r"remark:\s+([A-Za-z \[\]/]+): (\d+) \[-Rpass-analysis=kernel-resource-usage\]")
COMB_FORM = "k_update_pivot<0, 0, 1, 1, 0>"  # primal, lazy (no DSE), PSE, band partials summed inside, no pull


def short(name):
    """_ZN3mlp14k_update_pivotILi0ELi0ELi1ELi1ELi0EEEvNS_7DevViewEi -> k_update_pivot<0, 0, 1, 1, 0>: the kernels live in one namespace and
    take integers as template arguments, so the two rules of the mangling that this needs are applied here."""
    m = re.match(r"_ZN3mlp(\d+)", name)
    if not m:
        return name
    n = int(m.group(1))
    base, rest = name[m.end():m.end() + n], name[m.end() + n:]
    t = re.match(r"I((?:L[a-z]n?\d+E)+)E", rest)
    if not t:
        return base
    args = [a.replace("n", "-") for a in re.findall(r"L[a-z](n?\d+)E", t.group(1))]
    return base + "<" + ", ".join(args) + ">"


def report(source):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [mbuild.hipcc()] + mbuild.FLAGS + ["-x", "hip", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                                                   "-c", source, "-o", os.path.join(tmp, "kernels.o")]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            raise SystemExit("compilation failed")
    rows, cur = {}, None
    for line in p.stderr.split("\n"):
        m = NAME.search(line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        m = FIELD.search(line)
        if m and cur is not None and m.group(1).strip() in FIELDS:
            cur[FIELDS[m.group(1).strip()]] = int(m.group(2))
    return {short(n): r for n, r in rows.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--source", default=os.path.join(mbuild.CSRC, "kernels.hip"))
    ap.add_argument("--match", default="", help="only kernels whose name contains this")
    ap.add_argument("--json", help="write the figures here")
    ap.add_argument("--parent", help="figures of the parent commit (a file written with --json): stored beside the new ones")
    ap.add_argument("--check", action="store_true", help="apply the requirements of the k_update_pivot forms")
    a = ap.parse_args()
    rows = {k: v for k, v in sorted(report(a.source).items()) if a.match in k}
    print(f"{'kernel':58s} {'VGPRs':>5s} {'SGPR spill':>10s} {'VGPR spill':>10s} {'scratch':>7s} {'LDS':>6s} {'occ':>3s}")
    for k, r in rows.items():
        print(f"{k:58s} {r['vgprs']:5d} {r['sgpr_spill']:10d} {r['vgpr_spill']:10d} {r['scratch']:7d} {r['lds']:6d} {r['occupancy']:3d}")
    out = {"flags": mbuild.FLAGS, "kernels": rows}
    if a.parent:
        with open(a.parent) as f:
            out["parent"] = json.load(f)["kernels"]
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    if a.check:
        bad = [f"{k}: scratch {r['scratch']}, VGPR spill {r['vgpr_spill']}" for k, r in rows.items()
               if k.startswith("k_update_pivot") and (r["scratch"] or r["vgpr_spill"])]
        c = rows.get(COMB_FORM)
        if c is None:
            bad.append(f"{COMB_FORM}: no such instance")
        elif c["vgprs"] > 104 or c["lds"] > 112:
            bad.append(f"{COMB_FORM}: {c['vgprs']} VGPRs (at most 104), {c['lds']} bytes of LDS (at most 112)")
        if bad:
            raise SystemExit("requirements missed:\n  " + "\n  ".join(bad))
        print("requirements met")


if __name__ == "__main__":
    main()
