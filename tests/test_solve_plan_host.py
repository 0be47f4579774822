"""The witness solver's plan (cap_amd/csrc/solve_plan.hpp) is host code without HIP and its row rule (solve29.hpp) builds
for the host like gatecheck29.hpp: this CPU test compiles tests/cpp/solve_plan_check.cpp - a stand-alone program - which
meets every refusal of the rule with its lowest row named, checks levels and order on a hand-made circuit, solves random
circuits (OUT rows with and without q_ecc, fifth roots on each of wires 0 .. 3) and puts every defining row through
wc29::Check::gate, with field29.hpp's bound assertions on - plain and under ASan + UBSan.  (`-m "not gpu"`)"""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _run(tmp_path, cxx, flags):
    exe = str(tmp_path / "solve_plan_check")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-x", "c++"] + flags +
                          [os.path.join(HERE, "cpp", "solve_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "bad=0" in out.stdout, out.stdout[-800:] + out.stderr[-800:]
    m = re.search(r"refusals=(\d+) gates=(\d+) roots=(\d+) zero_dens=(\d+)", out.stdout)
    # every refusal of the rule (7 shapes + 4 broken conditions x 4 wires), hundreds of solved rows, fifth roots among them,
    # and both degenerate runs
    assert m and int(m.group(1)) >= 23 and int(m.group(2)) >= 500 and int(m.group(3)) >= 100 and int(m.group(4)) == 2


def test_solve_plan_on_the_host(tmp_path):
    cxx = next((c for c in ("g++", CLANG, "clang++") if shutil.which(c) or os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    _run(tmp_path, cxx, [])


def test_solve_plan_on_the_host_under_asan_and_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ for the sanitizer build")
    _run(tmp_path, CLANG, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
