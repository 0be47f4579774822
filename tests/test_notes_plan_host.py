"""cap_amd/csrc/notes_plan.hpp - the plan of capgpu_plonk_prove_notes* (groups of one domain size and SRS, their run order,
the constant-stride test of the device form) and the index functions of k_move_rows_at - is host code without HIP: this
CPU test compiles tests/cpp/notes_plan_check.cpp, which runs every assignment of 1 .. 8 notes to four (n, SRS) classes and
random ones of 256 through it, and the index functions over source offsets past 2^33 elements - plain and under
ASan + UBSan.  (`-m "not gpu"`)"""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _run(tmp_path, cxx, flags):
    exe = str(tmp_path / "notes_plan_check")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-x", "c++"] + flags +
                          [os.path.join(HERE, "cpp", "notes_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "bad=0" in out.stdout, out.stdout[-800:] + out.stderr[-800:]
    m = re.search(r"assignments=(\d+) random=(\d+) direct=(\d+) gathered=(\d+) moves=(\d+)", out.stdout)
    # every assignment of 1 .. 8 notes to 4 classes; both answers of the stride test were met; the moves ran
    assert m and int(m.group(1)) == sum(4 ** k for k in range(1, 9)) and int(m.group(2)) >= 32
    assert int(m.group(3)) > 0 and int(m.group(4)) > 0 and int(m.group(5)) > 0


def test_notes_plan_on_the_host(tmp_path):
    cxx = next((c for c in ("g++", CLANG, "clang++") if shutil.which(c) or os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    _run(tmp_path, cxx, [])


def test_notes_plan_on_the_host_under_asan_and_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ for the sanitizer build")
    _run(tmp_path, CLANG, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
