"""cap_amd/csrc/given_gather.hpp - the packing rule of a gathered part of capgpu_plonk_prove_given_one / _io_one requests:
who is set aside and why, the slots in arrival order, the rows zero-filled to the part's largest lengths, the scatter, the
normalised outcome - is host code without HIP: this CPU test compiles tests/cpp/given_gather_check.cpp, which runs every
assignment of 1 .. 8 requests to three keys with 0 .. 2 of them set aside through it - plain and under ASan + UBSan.
(`-m "not gpu"`)"""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _run(tmp_path, cxx, flags):
    exe = str(tmp_path / "given_gather_check")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-x", "c++"] + flags +
                          [os.path.join(HERE, "cpp", "given_gather_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "bad=0" in out.stdout, out.stdout[-800:] + out.stderr[-800:]
    m = re.search(r"assignments=(\d+) plans=(\d+) runs=(\d+) key_gone=(\d+) no_solver=(\d+) lengths=(\d+) zero_filled=(\d+)",
                  out.stdout)
    # every assignment of 1 .. 8 requests to 3 keys, each with nobody, every one and every two of them set aside
    assert m and int(m.group(1)) == sum(3 ** k for k in range(1, 9))
    assert int(m.group(2)) == sum(3 ** k * (1 + k + k * (k - 1) // 2) for k in range(1, 9))
    # every reason was met, and short rows were filled
    assert all(int(m.group(i)) > 0 for i in range(3, 8))


def test_given_gather_on_the_host(tmp_path):
    cxx = next((c for c in ("g++", CLANG, "clang++") if shutil.which(c) or os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    _run(tmp_path, cxx, [])


def test_given_gather_on_the_host_under_asan_and_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ for the sanitizer build")
    _run(tmp_path, CLANG, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
