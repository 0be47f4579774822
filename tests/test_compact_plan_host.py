"""cap_amd/csrc/compact.hpp - the plan of batch compaction (capgpu_plonk_set_compaction) - is host code without HIP: this CPU
test compiles tests/cpp/compact_plan_check.cpp, which runs every refusal mask of 1 .. 12 proofs and random masks of 256
through compact_plan and checks the survivors' order, the moves' ranges and distinctness, their number and their effect on
an array of row tags - plain and under ASan + UBSan.  (`-m "not gpu"`)"""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _run(tmp_path, cxx, flags):
    exe = str(tmp_path / "compact_plan_check")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-x", "c++"] + flags +
                          [os.path.join(HERE, "cpp", "compact_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "bad=0" in out.stdout, out.stdout[-800:] + out.stderr[-800:]
    m = re.search(r"masks=(\d+) zero_moves=(\d+) max_moves=(\d+)", out.stdout)
    # every mask of 1 .. 12 proofs, and both extremes were met
    assert m and int(m.group(1)) >= sum(1 << p for p in range(1, 13)) and int(m.group(2)) > 0 and int(m.group(3)) > 0


def test_compact_plan_on_the_host(tmp_path):
    cxx = next((c for c in ("g++", CLANG, "clang++") if shutil.which(c) or os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    _run(tmp_path, cxx, [])


def test_compact_plan_on_the_host_under_asan_and_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ for the sanitizer build")
    _run(tmp_path, CLANG, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
