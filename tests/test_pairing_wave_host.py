"""cap_amd/csrc/pairing_wave.hpp - one Fq12 spread over a group of six lanes, the six-lane form of the device pairing check -
on six emulated lanes (tests/hip/pairing_wave_host.cpp), with field29.hpp's bound assertions (CAP_FL_CHECK) and clang's
unsigned-overflow sanitizer on.  Every result must equal what the one-lane Tower<> of pairing29.hpp gives on the same
inputs, limb for limb after canonicalisation, and the values must be the oracle's.  (`-m "not gpu"`)"""
import os
import random
import subprocess

import pytest

from oracle import pairing as op
from oracle.bn254 import G1_GEN, P, R, g1_mul
from tests.helpers import from_tower, to_tower
from tests.test_field29_host import CLANG, _cxx

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hip", "pairing_wave_host.cpp")
X = 4965661367192848881
M = 2 * X * (6 * X * X + 3 * X + 1)      # the hard part raises to M (p^4 - p^2 + 1)/r (pairing29.hpp)
RINV = pow(1 << 261, -1, P)              # a raw internal value v stands for v / 2^261


@pytest.fixture(scope="module", params=["rowwise", "colwise"])
def exe(tmp_path_factory, request):
    out = tmp_path_factory.mktemp("pw" + request.param)
    path = str(out / "pairing_wave_host")
    flag = "-DCAP_FL_COLWISE" if request.param == "colwise" else "-DCAP_FL_ROWWISE"
    if os.path.exists(CLANG):
        ign = out / "ignore.txt"
        ign.write_text("src:*/field.hpp\nsrc:*/curve.hpp\nsrc:*/pairing.hpp\n")
        cmd = [CLANG, "-O1", "-std=c++17", flag, "-fsanitize=unsigned-integer-overflow", f"-fsanitize-ignorelist={ign}",
               "-fno-sanitize-recover=all", SRC, "-o", path]
    else:
        cmd = [_cxx(), "-O1", "-std=c++17", flag, SRC, "-o", path]
    subprocess.check_call(cmd)
    return path


def h(v):
    return f"{v:x}"


def f12_arg(f):
    return " ".join(h(v) for v in to_tower(f))


def raw_arg(t):
    return " ".join(h(v) for v in t)


def g1_arg(p):
    return "0 0" if p is None else f"{h(p[0])} {h(p[1])}"


def g2_arg(q):
    return " ".join(h(v) for v in (q[0][0], q[0][1], q[1][0], q[1][1]))


def run(exe, lines):
    """two output lines per operation: the group form's, then Tower<>'s; they must be the same text"""
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-800:]
    res = [r.strip() for r in out.stdout.strip().split("\n")]
    assert len(res) == 2 * len(lines)
    for line, wave, tower in zip(lines, res[0::2], res[1::2]):
        assert wave == tower, f"group form and Tower<> differ for: {line[:60]}"
    return res[0::2]


def parse_f12(line):
    return from_tower([int(v, 16) for v in line.split()])


def parse_raw(line):
    """raw internal values -> the flat Fq12 they stand for"""
    return from_tower([int(v, 16) * RINV % P for v in line.split()])


def rand_f12(rng):
    return [rng.randrange(P) for _ in range(12)]


def easy_part(f):
    conj = [(-c) % P if i % 2 else c for i, c in enumerate(f)]
    r = op.f12_mul(conj, op.f12_pow(f, P ** 12 - 2))
    return op.f12_mul(op.f12_pow(r, P * P), r)


def line_f12(s, b0, b1):
    """s + b0 w + b1 w^3 (s in Fq, b0, b1 in Fq2 as (x, y)) in the flat basis"""
    return from_tower([s, 0, b0[0], b0[1], 0, 0, b1[0], b1[1], 0, 0, 0, 0])


def test_group_operations_match_tower_and_the_flat_oracle(exe):
    rng = random.Random(21)
    lines, exp = [], []
    for _ in range(4):
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
        s, b0, b1 = rng.randrange(P), (rng.randrange(P), rng.randrange(P)), (rng.randrange(P), rng.randrange(P))
        lines.append(f"N {f12_arg(a)} {h(s)} {h(b0[0])} {h(b0[1])} {h(b1[0])} {h(b1[1])}")
        exp.append(op.f12_mul(a, line_f12(s, b0, b1)))
    for a in ([1] + [0] * 11, [5] + [0] * 11, [P - 1] * 12, [0] * 12):
        lines.append(f"M {f12_arg(a)} {f12_arg(a)}")
        exp.append(op.f12_mul(a, a))
        lines.append(f"S {f12_arg(a)}")
        exp.append(op.f12_mul(a, a))
    for line, got, want in zip(lines, run(exe, lines), exp):
        assert parse_f12(got) == want, line[:40]


# the representatives an f12 may hold (pairing29.hpp: every Fq normalized and < 2p): the ends of that range and of the
# canonical one, as field29's own tests take them
EXTREME = [0, 1, P - 1, P, P + 1, 2 * P - 1]


def raw_vectors(rng):
    vs = [[e] * 12 for e in EXTREME]
    vs += [[rng.choice(EXTREME) for _ in range(12)] for _ in range(3)]
    vs += [[rng.randrange(2 * P) for _ in range(12)] for _ in range(3)]
    return vs


def test_raw_limb_vectors_at_the_bounds(exe):
    """product, squaring, line product and Frobenius over raw internal representatives up to 2p - 1 in every coefficient:
    no bound assertion fires, no column sum wraps, the group form equals Tower<>, and the value is the oracle's"""
    rng = random.Random(22)
    vs = raw_vectors(rng)
    plain = lambda t: from_tower([v * RINV % P for v in t])  # noqa: E731
    lines, exp = [], []
    for i, a in enumerate(vs):
        b = vs[(i * 5 + 3) % len(vs)]
        lines.append(f"R M {raw_arg(a)} {raw_arg(b)}")
        exp.append(op.f12_mul(plain(a), plain(b)))
        lines.append(f"R S {raw_arg(a)}")
        exp.append(op.f12_mul(plain(a), plain(a)))
        s, b0, b1 = b[0], (b[1], b[2]), (b[3], b[4])
        lines.append(f"R N {raw_arg(a)} {h(s)} {h(b0[0])} {h(b0[1])} {h(b1[0])} {h(b1[1])}")
        exp.append(op.f12_mul(plain(a), line_f12(s * RINV % P, [v * RINV % P for v in b0], [v * RINV % P for v in b1])))
        lines.append(f"R F {1 + i % 3} {raw_arg(a)}")
        exp.append(op.f12_pow(plain(a), P ** (1 + i % 3)))
    for line, got, want in zip(lines, run(exe, lines), exp):
        assert parse_raw(got) == want, line[:40]
    # the cyclotomic squaring and the whole final exponentiation on the same raw vectors: equality with Tower<> (run()
    # asserts it) on inputs outside the cyclotomic subgroup too - both sides evaluate the same formulas
    run(exe, [f"R C {raw_arg(a)}" for a in vs])
    run(exe, [f"R E {raw_arg(a)}" for a in (vs[5], vs[-1])])


def test_cyclotomic_squaring(exe):
    rng = random.Random(23)
    cyc = [easy_part(rand_f12(rng)) for _ in range(3)]
    got = run(exe, [f"C {f12_arg(c)}" for c in cyc])
    for c, g in zip(cyc, got):
        assert parse_f12(g) == op.f12_mul(c, c)


def test_final_exponentiation(exe):
    rng = random.Random(24)
    fs = [rand_f12(rng) for _ in range(2)] + [[1] + [0] * 11, [0] * 12]
    got = run(exe, [f"E {f12_arg(f)}" for f in fs])
    for f, g in zip(fs[:3], got):
        assert parse_f12(g) == op.f12_pow(op.final_exponentiation(f), M)
    assert parse_f12(got[3]) == [0] * 12                   # 0 stays 0


def test_miller_loop_and_the_full_check_agree_with_the_oracle(exe):
    rng = random.Random(25)
    a, b = rng.randrange(1, R), rng.randrange(1, R)
    G2 = op.G2_GEN
    aG, abG = g1_mul(G1_GEN, a), g1_mul(G1_GEN, a * b % R)
    bH = op.g2_mul(G2, b)
    got = run(exe, [f"L {g1_arg(aG)} {g2_arg(bH)}"])
    assert parse_f12(got[0]) == op.miller_loop(bH, aG)
    neg = lambda p: (p[0], (-p[1]) % P)  # noqa: E731
    # e(aG, bH) e(-abG, H) == 1 by the oracle itself
    prod = op.f12_mul(op.miller_loop(bH, aG), op.miller_loop(G2, neg(abG)))
    assert op.final_exponentiation(prod) == [1] + [0] * 11
    checks = [
        (aG, bH, neg(abG), G2, 1),
        (aG, bH, neg(g1_mul(G1_GEN, (a * b + 1) % R)), G2, 0),
        (None, bH, None, G2, 1),                                     # both at infinity
        (None, bH, neg(abG), G2, 0),
        (aG, bH, None, G2, 0),
    ]
    got = run(exe, [f"K {g1_arg(p1)} {g2_arg(q1)} {g1_arg(p2)} {g2_arg(q2)}" for p1, q1, p2, q2, _ in checks])
    assert [int(g) for g in got] == [c[-1] for c in checks]
