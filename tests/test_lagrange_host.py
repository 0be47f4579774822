"""The Lagrange key builder's per-lane code (cap_amd/csrc/lagrange_elem29.hpp: what lag_load, lag_stage and lag_finish
execute) compiled for the host with the bound assertions of field29.hpp on (CAP_FL_CHECK), both multiplication schedules,
against Python integers (tests/lagrange_model.py): scalar_mul singly, and the whole build at the degenerate SRS families
a random tau never produces - doublings and cancellations in every butterfly, infinity on either side.  (`-m "not gpu"`)"""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from oracle import capref as cr
from tests import lagrange_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
R = M.R
SIZES = (0, 1, 2, 3, 6)            # n = 1, 2, 4, 8, 64


def _cxx():
    for c in ("g++", "/opt/rocm/lib/llvm/bin/clang++", "clang++"):
        if shutil.which(c) or os.path.exists(c):
            return c
    pytest.skip("no host C++ compiler")


@pytest.fixture(scope="module", params=["rowwise", "colwise"])
def twin(tmp_path_factory, request):
    exe = str(tmp_path_factory.mktemp("lag" + request.param) / "lagrange_check")
    flags = ["-DCAP_FL_COLWISE"] if request.param == "colwise" else ["-DCAP_FL_ROWWISE"]
    subprocess.check_call([_cxx(), "-O1", "-std=c++17"] + flags + [os.path.join(HERE, "cpp", "lagrange_check.cpp"), "-o", exe])
    return exe


def _hex_points(pts):
    out = []
    for row in cr.array_to_ints(np.asarray(pts, np.uint64).reshape(-1, 4)):
        out.append(f"{row:x}")
    return [out[i] + " " + out[i + 1] for i in range(0, len(out), 2)]


def _run(exe, mode, lines):
    out = subprocess.run([exe, mode], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-600:])       # -6: a bound assertion fired
    return out.stdout.split("\n")[:-1]


def scalar_cases():
    """(k, why) - the digits of scalar_mul are taken two bits at a time from `top | 1` down"""
    ks = [(k, "small") for k in range(6)]
    for j in (6, 7, 31, 32, 33, 64, 127, 200, 253):              # top bit of 2^j at an even / an odd position, and of
        ks += [(1 << j, f"2^{j}"), ((1 << j) - 1, f"2^{j}-1")]   # 2^j - 1 at the other parity; word boundaries
    ks += [(R - 1, "r-1"), ((R + 1) // 2, "(r+1)/2")]
    rng = random.Random(11)
    ks += [(rng.randrange(R), "random") for _ in range(24)]
    return ks


def test_scalar_mul_against_python(twin):
    rng = random.Random(12)
    ks = scalar_cases()
    assert {w for _, w in ks} >= {"small", "2^6", "2^7", "2^253-1", "r-1", "(r+1)/2", "random"}
    recs = []                                                     # (s, form, k)
    for k, _ in ks:
        recs.append((rng.randrange(1, R), 0, k))                  # B generic, z = 1
        recs.append((rng.randrange(1, R), 1, k))                  # B generic, zz != 1
        recs.append((0, 0, k))                                    # B at infinity, from the (0, 0) encoding
    recs += [(rng.randrange(1, R), 2, k) for k in (0, 1, 6, R - 1)]   # B at infinity with stale x, y
    recs += [(1, 0, R - 1), (1, 1, (R + 1) // 2), (R - 1, 0, R - 1)]    # [r-1]G = -G, [(r+1)/2](2G) = G, [r-1](-G) = G
    src = _hex_points(M.points([s for s, _, _ in recs]))
    got = _run(twin, "scalar", [f"{p} {form:x} {k:x}" for p, (_, form, k) in zip(src, recs)])
    want = _hex_points(M.points([0 if form == 2 else s * (2 if form == 1 else 1) * k % R for s, form, k in recs]))
    assert len(got) == len(want) == len(recs)
    for g, w, rec in zip(got, want, recs):
        assert [int(x, 16) for x in g.split()] == [int(x, 16) for x in w.split()], rec


@pytest.mark.parametrize("log_n", SIZES)
def test_whole_build_at_every_family(twin, log_n):
    n = 1 << log_n
    w_inv = pow(M.omega(log_n), R - 2, R)
    tail = [f"{pow(w_inv, k, R):x}" for k in range(max(n // 2, 1))] + [f"{pow(n, R - 2, R):x}"]
    lines, want, ran = [], [], []
    for label in M.FAMILIES:
        s = M.family_logs(label, log_n)
        lines += [f"{log_n:x}"] + _hex_points(M.points(s)) + tail
        want.append(_hex_points(M.points(M.expected_logs(s, log_n))))
        ran.append(label)
    got = _run(twin, "transform", lines)
    assert len(got) == len(M.FAMILIES) * (n + 3)
    for f, label in enumerate(ran):
        for j in range(n + 3):
            g, w = got[f * (n + 3) + j], want[f][j]
            assert [int(x, 16) for x in g.split()] == [int(x, 16) for x in w.split()], (label, j)
    assert tuple(ran) == M.FAMILIES and len(ran) == 12


def test_sizes_are_the_roster():
    assert [1 << k for k in SIZES] == [1, 2, 4, 8, 64]
