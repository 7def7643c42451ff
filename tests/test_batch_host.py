"""The batch policy of Engine::run_loop (minilp_amd/csrc/batch.h) against the expressions the loop held before the header existed: host
code only, no GPU.  tests/host/batch_check.cpp holds those expressions (transcribed by hand from the parent commit, with its line
numbers), walks the cross products of small value sets and has its own main; it is compiled with the host compiler — with the address
and undefined-behaviour sanitizers where the compiler has them — and run."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minilp_amd", "csrc")


def _compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return c
    return None


def test_every_decision_of_a_batch_is_what_run_loop_computed(tmp_path):
    cxx = _compiler()
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "batch_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "host", "batch_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # (the sanitizer runtimes linked statically where the compiler has them so: the program then starts whatever else a machine preloads)
    errors = ""
    for name, extra in (("sanitized, static runtimes", san + ["-static-libasan", "-static-libubsan"]), ("sanitized", san), ("plain", [])):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            print("batch_check build:", name)
            break
        errors += f"[{name}]\n{r.stderr}\n"
    else:
        raise AssertionError(errors)
    r = subprocess.run([exe], capture_output=True, text=True, stdin=subprocess.DEVNULL)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) cases, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 100000, r.stdout


def test_the_batch_policy_is_host_code_only():
    """batch.h includes nothing of HIP and names nothing of the engine: only standard headers, no `hip`, no `Engine`, no kernels.h."""
    text = open(os.path.join(CSRC, "batch.h")).read()
    includes = re.findall(r"^\s*#\s*include\s*[<\"]([^>\"]+)[>\"]", text, re.M)
    assert includes and all(i in ("algorithm", "cstdint") for i in includes), includes
    code = re.sub(r"//[^\n]*", "", text)                                                 # (the comments may name the engine)
    assert not re.search(r"\bhip|\bEngine\b|__global__|__device__|DevView|Geom\b", code), "batch.h must stay free of HIP and of the engine"
    assert '#include "batch.h"' in open(os.path.join(CSRC, "engine.h")).read()
