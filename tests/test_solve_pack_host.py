"""The packed witness solver's shared logic (cap_amd/csrc/solve_pack.hpp: the item decode of k_solve_vars_packed<W> and the
choice of W) is host + device code without HIP in its host part: this CPU test compiles tests/cpp/solve_pack_check.cpp - a
stand-alone program - which emulates packed workgroups with the kernel's own decode and requires every witness to come out
word for word as its lone row-by-row solve, for W in {1, 2, 4, 8, 16}, counts around W, with and without a witness list,
with foreign row strides, on a circuit with a 301-row level and one-row levels, with a zero denominator in slot 1 between
two good witnesses; and the automatic rule on hand-made width profiles.  Plain and under ASan + UBSan.  (`-m "not gpu"`)"""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _run(tmp_path, cxx, flags):
    exe = str(tmp_path / "solve_pack_check")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-x", "c++"] + flags +
                          [os.path.join(HERE, "cpp", "solve_pack_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "bad=0" in out.stdout, out.stdout[-800:] + out.stderr[-800:]
    m = re.search(r"cases=(\d+) items=(\d+) zero_dens=(\d+)", out.stdout)
    # 5 values of W x 5 counts (W = 1 has no W - 1) x {no list, list}; 350 witnesses of 325 rows; the degenerate witness
    assert m and int(m.group(1)) == 48 and int(m.group(2)) == 350 * 325 and int(m.group(3)) == 1


def test_solve_pack_on_the_host(tmp_path):
    cxx = next((c for c in ("g++", CLANG, "clang++") if shutil.which(c) or os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    _run(tmp_path, cxx, [])


def test_solve_pack_on_the_host_under_asan_and_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ for the sanitizer build")
    _run(tmp_path, CLANG, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
