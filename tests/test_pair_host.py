"""G1L::add_affine_pair - the first addition of a bucket-accumulation item, two affine table points - compiled for the
host (tests/cpp/pair_check.cpp): against add_mixed from infinity for all four sign combinations, the refusal on equal and
opposite points, and the accumulator invariants of what comes out; once with the bound assertions (CAP_FL_CHECK) and once
under clang's unsigned-integer-overflow sanitizer, as tests/test_field29_host.py builds madd_check.  (`-m "not gpu"`)"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _cxx():
    for c in ("g++", CLANG, "clang++"):
        if shutil.which(c) or os.path.exists(c):
            return c
    pytest.skip("no host C++ compiler")


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "bad=0" in out.stdout, out.stdout[-500:] + out.stderr[-800:]


def test_pair_addition_against_add_mixed(tmp_path):
    exe = str(tmp_path / "pair_check")
    subprocess.check_call([_cxx(), "-O1", "-std=c++17", os.path.join(CPP, "pair_check.cpp"), "-o", exe])
    _run(exe)


def test_pair_addition_has_no_integer_wraps(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ for the sanitizer build")
    ign = tmp_path / "ignore.txt"
    ign.write_text("src:*/field.hpp\nsrc:*/curve.hpp\n")
    exe = str(tmp_path / "pair_check_san")
    subprocess.check_call([CLANG, "-O1", "-std=c++17", "-fsanitize=unsigned-integer-overflow",
                           f"-fsanitize-ignorelist={ign}", "-fno-sanitize-recover=all",
                           os.path.join(CPP, "pair_check.cpp"), "-o", exe])
    _run(exe)
