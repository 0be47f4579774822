"""The pairing tower (cap_amd/csrc/pairing29.hpp: Tower) on the bound-tracking field of tests/cpp/bound29.hpp: every
function with every coefficient at the top of class E (normalized, < 2p), prepared lines canonical, the G1 point as
k_pairing_check2 hands it over; miller2 and final_exp as they run, and the Miller step and the exponentiation step to
the fixed point of the class.  Every field operation asserts its precondition for ALL inputs of the class; the bounds
are the "tower" section of tests/golden/lazy_envelope.json (python -m tests.test_ntt_elem_host rewrites the file).
With class E widened to 17p the check must fail and name the operation.
(`-m "not gpu"`)"""
import json
import os
import subprocess

import pytest

from tests.lazy_bound_classes import L29, U
from tests.test_field29_host import CLANG, CPP, _cxx

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "lazy_envelope.json")
SRC = os.path.join(CPP, "tower_envelope_check.cpp")
CLASS_E = 2 * U                                                      # "normalized and < 2p"


def _build(out, sanitize=False):
    exe = str(out / "tower_envelope_check")
    if sanitize:
        ign = out / "ignore.txt"
        ign.write_text("src:*/field.hpp\nsrc:*/curve.hpp\nsrc:*/pairing.hpp\n")
        cmd = [CLANG, "-O1", "-std=c++17", "-fsanitize=unsigned-integer-overflow,undefined",
               f"-fsanitize-ignorelist={ign}", "-fno-sanitize-recover=all", SRC, "-o", exe]
    else:
        cmd = [_cxx(), "-O1", "-std=c++17", SRC, "-o", exe]
    subprocess.check_call(cmd)
    return exe


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("towerenv"))


def tower_envelope(exe=None):
    """the "tower" section of the golden table; fails if a precondition does"""
    if exe is None:
        import pathlib
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            return tower_envelope(_build(pathlib.Path(d)))
    out = subprocess.run([exe, "envelope"], capture_output=True, text=True)
    assert out.returncode == 0, "a precondition fails for some input of class E, or a result leaves it:\n" + \
        out.stderr[-3000:]
    return json.loads(out.stdout)["tower"]


def test_envelope_equals_the_committed_table_and_stays_inside_class_e(plain):
    with open(GOLDEN) as f:
        want = json.load(f)["tower"]
    env = tower_envelope(plain)
    assert env == want, "the tower section differs from tests/golden/lazy_envelope.json"
    assert env["class_E"] == CLASS_E
    assert len(env["ops"]) >= 40 and len(env["chains"]) >= 5
    for sec in ("ops", "chains"):
        for name, (lim, mag) in env[sec].items():
            assert lim <= L29 and mag <= CLASS_E, (sec, name)


def test_a_wider_class_fails_the_envelope(plain):
    out = subprocess.run([plain, "envelope", "e17"], capture_output=True, text=True)
    first = out.stderr.split("\n")[0]
    assert out.returncode == 2 and first.startswith("bound violated in sub "), (out.returncode, out.stderr[-500:])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ for the sanitizer build")
    return _build(tmp_path_factory.mktemp("towerenv_san"), True)


@pytest.fixture(params=["plain", "sanitized"])
def exe(request):
    """each build on its own: without clang++ the sanitized half skips and the plain half still runs"""
    return request.getfixturevalue(request.param)


_WORDS = {}


def test_top_of_class_elements_through_the_real_tower(exe):
    """every function the device check knows (f2 .. f12 products, squarings, inverses, Frobenius maps, the sparse line
    product, cyclotomic squaring, the exponentiation by x, final_exp) on the records of tests/devcheck_vectors.py that sit
    at the top of class E - every coefficient within 2^64 of 2p - 1, all 2p - 1, all + p representatives - through
    the real Tower<0> and Tower<1>, plain and under clang's integer sanitizers: oracle/pairing.py's value and the class
    (devcheck_vectors.check_tower), and a true magnitude at most the golden table's figure.  miller2 and check2 need
    prepared line tables and run on concrete values in tests/test_devcheck_host.py only."""
    from tests import devcheck_vectors as dv
    with open(GOLDEN) as f:
        table = json.load(f)["tower"]["ops"]
    recs = [r for r in dv.generate()[0]["tower"] if r.kind in ("edge:top", "edge:2p-1", "edge:lazy")]
    assert {r.op for r in recs} == set(dv.OPS["tower"]) and {r.sched for r in recs} == {0, 1}
    text = "\n".join(f"{dv.OPS['tower'][r.op]:x} {r.sched:x} {r.aux:x} " + " ".join(f"{w:x}" for w in r.words)
                     for r in recs) + "\n"
    out = subprocess.run([exe, "run"], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-1500:]
    assert _WORDS.setdefault("tower", out.stdout) == out.stdout, "the plain and the sanitized build differ in their words"
    res = out.stdout.strip().split("\n")
    assert len(res) == len(recs)
    for r, line in zip(recs, res):
        w = [int(x, 16) for x in line.split()]
        assert len(w) == 108
        msg = dv.check_tower(r, w + [0, 0])
        assert msg is None, f"{r.describe()}: {msg}"
        key = f"f12_frob {r.aux}" if r.op == "f12_frob" else r.op
        for c in range(12):
            v = dv.val(w[9 * c:9 * c + 9])
            assert v * U <= table[key][1] * dv.P, f"{r.describe()}: coefficient {c} is {v / dv.P:.4f} p, the table says " \
                                                 f"{table[key][1] / U:.4f} p"
