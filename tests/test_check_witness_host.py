"""cap_amd/csrc/gatecheck29.hpp - the gate constraint and the permutation's index form of the device witness check -
compiled for the host with field29.hpp's bound assertions on (CAP_FL_CHECK), both multiplication schedules, against
oracle/plonk.py.  (`-m "not gpu"`)"""
import os
import random
import subprocess

import pytest

from oracle import bn254 as bn
from oracle import plonk as pl
from oracle.bn254 import R
from tests.test_field29_host import _cxx

HERE = os.path.dirname(os.path.abspath(__file__))
NO_INDEX = 0xFFFFFFFF


@pytest.fixture(scope="module", params=["rowwise", "colwise"])
def exe(tmp_path_factory, request):
    out = tmp_path_factory.mktemp("gate" + request.param)
    path = str(out / "gate_check")
    flag = "-DCAP_FL_COLWISE" if request.param == "colwise" else "-DCAP_FL_ROWWISE"
    subprocess.check_call([_cxx(), "-O1", "-std=c++17", flag, os.path.join(HERE, "cpp", "gate_check.cpp"), "-o", path])
    return path


def run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-800:]
    return out.stdout.strip().split("\n")


def hx(vals):
    return " ".join(f"{v:x}" for v in vals)


def satisfied_row(rng, q, w):
    """w[4] solved so that the gate holds (q_o must not cancel against the q_ecc term)"""
    rest = pl.gate_eval(q, w[:4] + [0], 0)
    d = (q[pl.Q_O] - q[pl.Q_ECC] * w[0] * w[1] * w[2] * w[3]) % R
    assert d
    return w[:4] + [rest * pow(d, R - 2, R) % R]


def gate_rows():
    rng = random.Random(21)
    rows = []
    for _ in range(40):                                         # random rows: the gate does not hold
        rows.append(([rng.randrange(R) for _ in range(13)], [rng.randrange(R) for _ in range(5)], rng.randrange(R)))
    for _ in range(20):                                         # random rows whose output wire makes it hold
        q = [rng.randrange(R) for _ in range(13)]
        rows.append((q, satisfied_row(rng, q, [rng.randrange(R) for _ in range(5)]), 0))
    edge = [0, 1, R - 1]
    rows.append(([0] * 13, [rng.randrange(R) for _ in range(5)], 0))          # all selectors 0: holds whatever the wires
    rows.append(([0] * 13, [rng.randrange(R) for _ in range(5)], 5))          # ... but not with a public input
    for a in edge:                                              # operands 0 / 1 / r - 1 everywhere
        for b in edge:
            rows.append(([a] * 13, [b] * 5, a))
            rows.append(([b] * 13, [a, b, a, b, a], b))
    for s in range(13):                                         # each selector alone, once failing and once holding
        q = [0] * 13
        q[s] = rng.randrange(1, R)
        w = [rng.randrange(1, R) for _ in range(5)]
        rows.append((q, w, 0))
        rows.append((q, w, (-pl.gate_eval(q, w, 0)) % R))       # the public input that cancels the term
    rows.append(([0] * 10 + [1, 0, 0], [3, 4, 5, 6, 0], 0))     # q_o alone with a zero output: holds
    return rows


def test_gate_value_matches_the_oracle(exe):
    rows = gate_rows()
    lines = [f"{op} {hx(q)} {hx(w)} {pi:x}" for q, w, pi in rows for op in ("G", "H")]
    got = run(exe, lines)
    assert len(got) == 2 * len(rows)
    holds = 0
    for k, (q, w, pi) in enumerate(rows):
        want = pl.gate_eval(q, w, pi)
        for line in got[2 * k:2 * k + 2]:                       # canonical operands, then operands + r
            val, ok = line.split()
            assert int(val, 16) == want, f"row {k}"
            assert int(ok) == (1 if want == 0 else 0), f"row {k}"
        holds += want == 0
    assert 30 <= holds <= len(rows) - 60                        # both verdicts are well represented


def test_values_are_compared_mod_r(exe):
    rng = random.Random(22)
    a, b = rng.randrange(R), rng.randrange(R)
    top = (1 << 256) - 1
    cases = [(a, a, 1), (a, b, 0), (a, a + R, 1), (a + R, a + 2 * R, 1), (a, b + R, 0), (0, R, 1), (0, 5 * R, 1),
             (1, R, 0), (top, top % R, 1), (top, (top - 1) % R, 0)]
    got = run(exe, [f"E {x:x} {y:x}" for x, y, _ in cases])
    assert [int(g) for g in got] == [c[2] for c in cases]


@pytest.mark.parametrize("log_n", range(4, 11))
def test_permutation_index_matches_the_oracles_position_table(exe, log_n):
    """every cell of the extended domain: k_i omega^j -> i n + j, exactly the `pos` table of
    oracle.plonk.check_circuit_satisfiability; values outside the five cosets are refused, not mis-indexed"""
    n = 1 << log_n
    omega = bn.root_of_unity(log_n)
    kinv = [pow(k, R - 2, R) for k in pl.K]
    winv = [pow(omega, R - 1 - (1 << b), R) for b in range(log_n)]
    pos, vals = {}, []
    x = 1
    for j in range(n):
        for i in range(pl.NUM_WIRES):
            pos[pl.K[i] * x % R] = (i, j)
        x = x * omega % R
    vals = list(pos)
    rng = random.Random(log_n)
    rng.shuffle(vals)
    outside = [0, rng.randrange(R), bn.root_of_unity(log_n + 1), pl.K[2] * bn.root_of_unity(log_n + 1) % R,
               bn.FR_GENERATOR, (pl.K[1] + 1) % R]
    assert not any(v in pos for v in outside)
    allv = vals + outside
    got = run(exe, [f"I {log_n} {hx(kinv)} {hx(winv)} {len(allv)} {hx(allv)}"])[0].split()
    assert len(got) == len(allv)
    for v, g in zip(vals, got):
        i, j = pos[v]
        assert int(g, 16) == i * n + j
    assert [int(g, 16) for g in got[len(vals):]] == [NO_INDEX] * len(outside)
