"""cap_amd/csrc/srs_check.hpp is host+device: this CPU test compiles its CAP_HD point predicate - what k_srs_points runs one
lane per resident base - for the host (tests/cpp/srs_check_host.cpp, a stand-alone program) and runs it against the
saturated field of field.hpp / curve.hpp on the generator, random curve points, (x, -y), (x, y + 1), (0, 0), coordinates
next to zero, every image x + k p below 2^256 and the bounds of the memory format, with the lazy field's bounds asserted
(CAP_FL_CHECK).  Plain, and under the address and undefined-behaviour sanitizers.  (`-m "not gpu"`)"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _run(tmp_path, cxx, flags):
    exe = str(tmp_path / "srs_check_host")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-x", "c++"] + flags +
                          [os.path.join(HERE, "cpp", "srs_check_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "bad=0" in out.stdout, out.stdout[-800:] + out.stderr[-800:]


def test_point_predicate_against_the_saturated_field(tmp_path):
    cxx = next((c for c in ("g++", CLANG, "clang++") if shutil.which(c) or os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    _run(tmp_path, cxx, [])


def test_point_predicate_under_ubsan_and_asan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ for the sanitizer build")
    _run(tmp_path, CLANG, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
