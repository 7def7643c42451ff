"""Settings::from_env (minilp_amd/csrc/settings.cpp) against the parse rules the knobs had where each was read before: host code only,
no GPU.  tests/host/settings_check.cpp holds the table (transcribed by hand from the parent commit, with its line numbers) and its own
main; it is compiled with the host compiler together with settings.cpp — with the address and undefined-behaviour sanitizers where the
compiler has them — and run."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minilp_amd", "csrc")


def _compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return c
    return None


def test_every_knob_parses_as_it_did_where_it_was_read(tmp_path):
    cxx = _compiler()
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "settings_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "host", "settings_check.cpp"),
            os.path.join(CSRC, "settings.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # (the sanitizer runtimes linked statically where the compiler has them so: the program then starts whatever else a machine preloads)
    errors = ""
    for name, extra in (("sanitized, static runtimes", san + ["-static-libasan", "-static-libubsan"]), ("sanitized", san), ("plain", [])):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            print("settings_check build:", name)
            break
        errors += f"[{name}]\n{r.stderr}\n"
    else:
        raise AssertionError(errors)
    env = {k: v for k, v in os.environ.items() if not k.startswith("MLP_")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout


def test_the_engine_reads_the_environment_in_one_place_only():
    """getenv appears in csrc/ only in settings.cpp and at the pool's MLP_POOL_POISON, so no function-local static can cache a knob: a
    `static const` on a line that names an MLP_* variable is the pool's alone."""
    hits = []
    for name in sorted(os.listdir(CSRC)):
        if name == "settings.cpp" or not name.endswith((".hip", ".inc", ".h", ".cpp")):
            continue
        with open(os.path.join(CSRC, name)) as f:
            for i, line in enumerate(f, 1):
                if ("getenv" in line or ("static const" in line and "MLP_" in line)) and "MLP_POOL_POISON" not in line:
                    hits.append(f"{name}:{i}: {line.strip()}")
    assert not hits, hits
