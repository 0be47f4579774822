"""cap_amd/csrc/pairing29.hpp - the tower Fq2/Fq6/Fq12, the prepared-line Miller loop and the final exponentiation of the
device pairing check - compiled for the host with field29.hpp's bound assertions on (CAP_FL_CHECK), both multiplication
schedules, against oracle/pairing.py.  (`-m "not gpu"`)"""
import os
import random
import subprocess

import pytest

from oracle import pairing as op
from oracle.bn254 import G1_GEN, P, R, g1_mul
from tests.helpers import from_tower, to_tower
from tests.test_field29_host import _cxx

HERE = os.path.dirname(os.path.abspath(__file__))
X = 4965661367192848881
M = 2 * X * (6 * X * X + 3 * X + 1)      # the hard part raises to M (p^4 - p^2 + 1)/r (pairing29.hpp)


@pytest.fixture(scope="module", params=["rowwise", "colwise"])
def exe(tmp_path_factory, request):
    out = tmp_path_factory.mktemp("p29" + request.param)
    path = str(out / "pairing29_check")
    flag = "-DCAP_FL_COLWISE" if request.param == "colwise" else "-DCAP_FL_ROWWISE"
    subprocess.check_call([_cxx(), "-O1", "-std=c++17", flag, os.path.join(HERE, "cpp", "pairing29_check.cpp"),
                           "-o", path])
    return path


def h(v):
    return f"{v:x}"


def f12_arg(f):
    return " ".join(h(v) for v in to_tower(f))


def g1_arg(p):
    return "0 0" if p is None else f"{h(p[0])} {h(p[1])}"


def g2_arg(q):
    return " ".join(h(v) for v in (q[0][0], q[0][1], q[1][0], q[1][1]))


def run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-800:]
    return out.stdout.strip().split("\n")


def parse_f12(line):
    return from_tower([int(v, 16) for v in line.split()])


def rand_f12(rng):
    return [rng.randrange(P) for _ in range(12)]


def easy_part(f):
    conj = [(-c) % P if i % 2 else c for i, c in enumerate(f)]
    r = op.f12_mul(conj, op.f12_pow(f, P ** 12 - 2))
    return op.f12_mul(op.f12_pow(r, P * P), r)


def test_tower_operations_match_the_flat_oracle(exe):
    rng = random.Random(11)
    lines, exp = [], []
    for _ in range(6):
        a, b = rand_f12(rng), rand_f12(rng)
        lines.append(f"M {f12_arg(a)} {f12_arg(b)}")
        exp.append(op.f12_mul(a, b))
        lines.append(f"S {f12_arg(a)}")
        exp.append(op.f12_mul(a, a))
        lines.append(f"I {f12_arg(a)}")
        exp.append(op.f12_pow(a, P ** 12 - 2))
        for j in (1, 2, 3):
            lines.append(f"F {j} {f12_arg(a)}")
            exp.append(op.f12_pow(a, P ** j))
    # edge values: one, a base-field element, p - 1 in every coefficient
    for a in ([1] + [0] * 11, [5] + [0] * 11, [P - 1] * 12):
        lines.append(f"M {f12_arg(a)} {f12_arg(a)}")
        exp.append(op.f12_mul(a, a))
    for line, got, want in zip(lines, run(exe, lines), exp):
        assert parse_f12(got) == want, line[:40]


def test_cyclotomic_squaring(exe):
    rng = random.Random(12)
    cyc = [easy_part(rand_f12(rng)) for _ in range(4)]
    got = run(exe, [f"C {f12_arg(c)}" for c in cyc])
    for c, g in zip(cyc, got):
        assert parse_f12(g) == op.f12_mul(c, c)


def test_final_exponentiation_of_random_elements(exe):
    rng = random.Random(13)
    fs = [rand_f12(rng) for _ in range(3)] + [[1] + [0] * 11]
    got = run(exe, [f"E {f12_arg(f)}" for f in fs])
    for f, g in zip(fs, got):
        assert parse_f12(g) == op.f12_pow(op.final_exponentiation(f), M)


def rand_points(rng, n):
    out = []
    for _ in range(n):
        a, b = rng.randrange(1, R), rng.randrange(1, R)
        out.append((a, b, g1_mul(G1_GEN, a), op.g2_mul(op.G2_GEN, b)))
    return out


def test_prepared_line_miller_loop_and_pairing_value(exe):
    rng = random.Random(14)
    pts = rand_points(rng, 2)
    lines, exp = [], []
    for _, _, p, q in pts:
        lines.append(f"L {g1_arg(p)} {g2_arg(q)}")
        exp.append(op.miller_loop(q, p))
        lines.append(f"P {g1_arg(p)} {g2_arg(q)}")
        exp.append(op.f12_pow(op.pairing(q, p), M))
    lines.append(f"P {g1_arg(None)} {g2_arg(pts[0][3])}")       # infinity in G1: e = 1
    exp.append([1] + [0] * 11)
    for line, got, want in zip(lines, run(exe, lines), exp):
        assert parse_f12(got) == want, line[:20]


def test_bilinearity_and_the_two_pair_check(exe):
    rng = random.Random(15)
    a, b = rng.randrange(1, R), rng.randrange(1, R)
    G2 = op.G2_GEN
    aP, abP = g1_mul(G1_GEN, a), g1_mul(G1_GEN, a * b % R)
    bQ = op.g2_mul(G2, b)
    out = run(exe, [f"P {g1_arg(aP)} {g2_arg(bQ)}", f"P {g1_arg(abP)} {g2_arg(G2)}"])
    assert parse_f12(out[0]) == parse_f12(out[1])
    neg = lambda p: (p[0], (-p[1]) % P)  # noqa: E731
    checks = [
        (aP, bQ, neg(abP), G2, 1),                                   # e(aP, bQ) e(-abP, Q) = 1
        (aP, bQ, neg(g1_mul(G1_GEN, (a * b + 1) % R)), G2, 0),        # off by one
        (None, bQ, None, G2, 1),                                     # both infinity
        (None, bQ, neg(abP), G2, 0),                                 # one infinity: e(-abP, Q) != 1
        (aP, bQ, None, G2, 0),
    ]
    got = run(exe, [f"K {g1_arg(p1)} {g2_arg(q1)} {g1_arg(p2)} {g2_arg(q2)}" for p1, q1, p2, q2, _ in checks])
    assert [int(g) for g in got] == [c[-1] for c in checks]
