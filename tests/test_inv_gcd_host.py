"""Fr inversion by a constant-time GCD (cap_amd/csrc/invgcd29.hpp) is host + device code without HIP on the host: this CPU
test compiles tests/cpp/inv_gcd_check.cpp - a stand-alone program with its own main - with field29.hpp's and the header's
bound assertions on, plain and under ASan + UBSan.  For every vector (the edge values, 2^k, 2^k - 1 and r - 2^k for every k,
their lazy representatives, 100 000 SplitMix64 values) the program compares canonical(inv_gcd(a)) limb for limb with
canonical(a^(r - 2)), checks a * inv = 1, and reads the loop's end state: g = 0 and f = +-1 (f = r for 0).  Then it solves
random circuits row by row through the solver's row rule in both inverse forms: the same words, the same zero_den flags.
(`-m "not gpu"`)"""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _run(tmp_path, cxx, flags):
    exe = str(tmp_path / "inv_gcd_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-x", "c++"] + flags +
                          [os.path.join(HERE, "cpp", "inv_gcd_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "bad=0" in out.stdout, out.stdout[-800:] + out.stderr[-800:]
    m = re.search(r"edge=(\d+) vectors=(\d+) zeros=(\d+) neg_f=(\d+) rows=(\d+) inv_rows=(\d+) root_rows=(\d+) flagged=(\d+) "
                  r"jumps=(\d+)", out.stdout)
    assert m, out.stdout[-400:]
    edge, vectors, zeros, neg_f, rows, inv_rows, root_rows, flagged, jumps = map(int, m.groups())
    # (7 + 3 * 254) values, each as a field element, as the GCD's own start value and as that value + r and + 7r
    assert edge == 4 * (7 + 3 * 254) and vectors >= edge + 100000
    # 0 and 2^0 - 1 in four representations each; both signs of the final f occur; the proven count in whole jumps
    assert zeros == 8 and neg_f > 1000 and vectors - neg_f > 1000 and jumps * 29 >= 735
    # mixed circuits: inverted rows, fifth roots and zero denominators all went through both forms
    assert rows >= 500 and inv_rows >= 100 and root_rows >= 100 and flagged >= 2


def test_inv_gcd_on_the_host(tmp_path):
    cxx = next((c for c in ("g++", CLANG, "clang++") if shutil.which(c) or os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    _run(tmp_path, cxx, [])


def test_inv_gcd_on_the_host_under_asan_and_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ for the sanitizer build")
    _run(tmp_path, CLANG, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
