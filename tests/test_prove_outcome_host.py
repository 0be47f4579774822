"""cap_amd/csrc/outcome.hpp is host+device: this CPU test compiles the rule of capgpu_plonk_prove_each* for the host
(tests/cpp/prove_outcome_check.cpp) - the status for every (degree flags, fault kind), blanking of exactly one record between
guard bytes, the three wordings against literal strings at cap 0 / 1 / exact - plain and under ASan + UBSan.
(`-m "not gpu"`)"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _run(tmp_path, cxx, flags):
    exe = str(tmp_path / "prove_outcome_check")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-x", "c++"] + flags +
                          [os.path.join(HERE, "cpp", "prove_outcome_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "bad=0" in out.stdout, out.stdout[-800:] + out.stderr[-800:]


def test_outcome_rule_on_the_host(tmp_path):
    cxx = next((c for c in ("g++", CLANG, "clang++") if shutil.which(c) or os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    _run(tmp_path, cxx, [])


def test_outcome_rule_on_the_host_under_asan_and_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ for the sanitizer build")
    _run(tmp_path, CLANG, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
