"""cap_amd/csrc/verify_front.hpp is host+device: this CPU test compiles its CAP_HD parts for the host together with
verify.hip's host verifier (tests/cpp/verify_front_check.cpp) and runs them - the device front end's transcript byte layout,
its seven challenges and its 34 scalars against verifier_terms for proofs of two keys (0 and 4 public inputs) and ext_msg
lengths 0, 1, 135, 136, 137 and 300 (around the sponge's 136-byte rate), then the weight rule: r_0 = 1, every other
r_i < 2^128, pairwise distinct, and every r_i (i >= 1) changes when any single u_j changes.  (`-m "not gpu"`)"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _run(tmp_path, cxx, flags):
    exe = str(tmp_path / "verify_front_check")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-x", "c++", "-pthread"] + flags +
                          [os.path.join(HERE, "cpp", "verify_front_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "bad=0" in out.stdout, out.stdout[-800:] + out.stderr[-800:]


def test_front_end_against_the_host_verifier(tmp_path):
    cxx = next((c for c in ("g++", CLANG, "clang++") if shutil.which(c) or os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    _run(tmp_path, cxx, [])


def test_front_end_against_the_host_verifier_under_ubsan_and_asan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ for the sanitizer build")
    _run(tmp_path, CLANG, ["-fsanitize=undefined,address", "-fno-sanitize-recover=all"])
