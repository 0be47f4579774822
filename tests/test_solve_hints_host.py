"""The solver's hints on the host: the hint table, the firing step and the refusals of cap_amd/csrc/solve_plan.hpp are host
code without HIP, and the three hint rules of solve29.hpp build for the host like the row rule.  This CPU test compiles
tests/cpp/solve_hints_check.cpp - a stand-alone program - which meets every hint refusal with its hint index named, checks
firing order, levels and chains on a hand-made circuit, compares plans without hints with the rule as it was before hints,
solves random circuits that lay unpack / is_zero / is_equal on given and computed values (bits against from_mont, inverses,
flags, wc29::Check::gate at EVERY row) and emulates packed workgroups over the hint items at W = 1, 4 and 16 - with
field29.hpp's bound assertions on, plain and under ASan + UBSan.  (`-m "not gpu"`)"""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _run(tmp_path, cxx, flags):
    exe = str(tmp_path / "solve_hints_check")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-x", "c++"] + flags +
                          [os.path.join(HERE, "cpp", "solve_hints_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "bad=0" in out.stdout, out.stdout[-800:] + out.stderr[-800:]
    m = re.search(r"refusals=(\d+) plans=(\d+) bits=(\d+) invs=(\d+) flags=(\d+) zero_sources=(\d+) gates=(\d+) packed=(\d+)",
                  out.stdout)
    assert m, out.stdout[-400:]
    refusals, plans, bits, invs, flags, zero_sources, gates, packed = (int(x) for x in m.groups())
    # every hint refusal (some in two forms) and the two row-rule ones that must still come first; three unhinted plans;
    # thousands of bits, every inverse and flag of 38 witnesses, zero sources among them; every row of every witness;
    # W in {1, 4, 16} x ragged counts
    assert refusals >= 16 and plans == 3 and bits >= 20000 and invs == flags == 5 * 38 and zero_sources >= 38
    assert gates == 2048 * 38 and packed == 16


def test_solve_hints_on_the_host(tmp_path):
    cxx = next((c for c in ("g++", CLANG, "clang++") if shutil.which(c) or os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    _run(tmp_path, cxx, [])


def test_solve_hints_on_the_host_under_asan_and_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ for the sanitizer build")
    _run(tmp_path, CLANG, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
