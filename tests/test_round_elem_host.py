"""The arithmetic of the prover's four lazy-field round kernels (cap_amd/csrc/round_elem29.hpp: the bodies of
k_perm_numden, k_kx_columns, k_quotient<true / false> and k_lincomb, with ColAcc) on the host, where the bound assertions
of field29.hpp (CAP_FL_CHECK) are compiled in - on the GPU they are not.

  * rows and points drawn as tests/round_model.py draws its cases (the index rule, saturated limb images, edge
    challenges, beta = 0, the contracts' bounds) for n = 8 and 64 rows and m = 96 and 192 points, through the bodies,
    against that module's models: every result's residue and representation; both multiplication schedules, plain and
    under clang's integer sanitizers (a stand-alone program);
  * the envelope: the same templates on tests/cpp/bound29.hpp with EVERY operand an arbitrary 32-byte image - the largest
    class any contract admits - so each precondition is checked for all inputs; the bounds of what leaves are the
    "rounds" section of tests/golden/lazy_envelope.json (python -m tests.test_ntt_elem_host rewrites the file);
  * ColAcc: six products of saturated images through the real accumulator stay within the bound table's figure, and a
    seventh product before the reduction makes the envelope fail.
(`-m "not gpu"`)"""
import json
import os
import random
import subprocess

import pytest

from tests import round_model as rm
from tests.test_field29_host import CLANG, CPP, _cxx

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "lazy_envelope.json")
R = rm.R
U = 1 << 20
I261_INV = pow(1 << 261, -1, R)
M256 = (1 << 256) - 1
SRC = os.path.join(CPP, "round_elem_check.cpp")


def _build(out, sanitize):
    exe = str(out / "round_elem_check")
    if sanitize:
        ign = out / "ignore.txt"
        ign.write_text("src:*/field.hpp\nsrc:*/curve.hpp\n")
        cmd = [CLANG, "-O1", "-std=c++17", "-fsanitize=unsigned-integer-overflow,undefined",
               f"-fsanitize-ignorelist={ign}", "-fno-sanitize-recover=all", SRC, "-o", exe]
    else:
        cmd = [_cxx(), "-O1", "-std=c++17", SRC, "-o", exe]
    subprocess.check_call(cmd)
    return exe


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("roundelem"), False)


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ for the sanitizer build")
    return _build(tmp_path_factory.mktemp("roundelem_san"), True)


def round_envelope(exe=None):
    """the "rounds" section of the golden table; fails if a precondition does"""
    if exe is None:
        import pathlib
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            return round_envelope(_build(pathlib.Path(d), False))
    out = subprocess.run([exe, "envelope"], capture_output=True, text=True)
    assert out.returncode == 0, "a precondition fails for some input:\n" + out.stderr[-3000:]
    return json.loads(out.stdout)["rounds"]


def test_envelope_every_operand_at_its_maximum_equals_the_committed_table(plain):
    with open(GOLDEN) as f:
        want = json.load(f)["rounds"]
    env = round_envelope(plain)
    assert env == want, "the rounds section differs from tests/golden/lazy_envelope.json"
    canonical = [env["k_perm_numden"]["num"], env["k_perm_numden"]["den"], env["k_kx_columns"]["out"],
                 env["k_lincomb"]["out_29_terms"], env["k_lincomb"]["out_30_terms"]]
    assert all(m <= U for m in canonical)                                               # packed canonical: < r
    assert env["k_quotient_fold"]["out"] <= 2 * U and env["k_quotient_direct"]["out"] <= 2 * U   # stored: < 2r


def test_a_seventh_product_before_the_reduction_fails_the_envelope(plain):
    out = subprocess.run([plain, "envelope", "1"], capture_output=True, text=True)
    assert out.returncode == 2 and "ColAcc::reduce" in out.stderr, (out.returncode, out.stderr[-500:])


# ---- rows as tests/round_model.py draws them -------------------------------------------------------------------------
def _hex(imgs):
    return " ".join(f"{v:x}" for v in imgs)


def perm_rows(rng):
    """-> [(line, check)]: the three proofs of rm.perm_case - beta = 0; gamma = 0 with wires 0 or r - 1; edge challenges"""
    rows = []
    for n in (8, 64):
        tw = rm.fill(rng, n, phase=1)
        ks = [1] + [rm.internal_value(rm.draw_edge(rng, rm.CANON, "internal")) for _ in range(4)]
        for p in range(3):
            wires = rm.fill(rng, 5 * n, phase=p) if p != 1 else [rng.choice([0, R - 1]) for _ in range(5 * n)]
            sig = rm.fill(rng, 5 * n, phase=2 + p)
            beta = [0, rng.randrange(1, R), rm.ark_value(rm.draw_edge(rng, rm.CANON, "ark"))][p]
            gamma = [rng.randrange(R), 0, rm.ark_value(rm.draw_edge(rng, rm.CANON, "ark"))][p]
            w = [[rm.ark_value(v) for v in wires[i * n:(i + 1) * n]] for i in range(5)]
            s = [[rm.ark_value(v) for v in sig[i * n:(i + 1) * n]] for i in range(5)]
            num, den, _, _ = rm.grand_product(w, s, [rm.ark_value(v) for v in tw], ks, beta, gamma)
            for j in range(n):
                imgs = [rm.ark(beta), rm.ark(gamma), tw[j]] + [rm.internal(k) for k in ks] + \
                    [wires[i * n + j] for i in range(5)] + [sig[i * n + j] for i in range(5)]
                rows.append(("P " + _hex(imgs), ("exact", [rm.ark(num[j]), rm.ark(den[j])])))
    return rows


def kx_rows(rng):
    rows = []
    for x in rm.fill(rng, 96, form="internal"):
        k = rm.draw_edge(rng, rm.CANON, "internal") if rng.random() < 0.7 else rm.saturated(rm.CANON)
        rows.append((f"K {k:x} {x:x}", ("exact", [rm.internal(rm.internal_value(k) * rm.internal_value(x) % R)])))
    return rows


def quotient_rows(rng):
    """the points of rm.quot_case: key columns and coset evaluations below 2r by the index rule, tables canonical,
    proof 0 with gamma and alpha at the saturated image, proof 1 with beta = 0 (direct form only)"""
    val, rows = rm.internal_value, []
    top = val(rm.saturated(rm.CANON))
    for m in (96, 192):
        xs, inx = rm.fill(rng, m, form="internal"), rm.fill(rng, m, form="internal")
        ks = [1] + [val(rm.draw_edge(rng, rm.CANON, "internal")) for _ in range(4)]
        zh = rm.fill(rng, 8, form="internal")
        cols = [rm.fill(rng, m, rm.WEAK, "internal") for _ in range(18)]
        cols += [[rm.internal(ks[j + 1] * val(x) % R) for x in xs] for j in range(4)]
        chs = [(val(rm.draw_edge(rng, rm.CANON, "internal")) or 1, top, top),
               (0, val(rm.draw_edge(rng, rm.CANON, "internal")), rng.randrange(R)),
               (rng.randrange(1, R), rng.randrange(R), rng.randrange(R))]
        for p, (b, g, a) in enumerate(chs):
            cos = [rm.fill(rng, m, rm.WEAK, "internal") for _ in range(6)]
            ch = (b, g, a, a * a % R, rm.inv(b) if b else 0, a * pow(b, 5, R) % R)
            for i in range(m):
                for five in (0, 1):
                    if five and i >= m - m // 6:
                        continue
                    it, inext, zi = rm.quotient_indices(m, five, i)
                    want = rm.quotient_point(True, [val(cols[s][it]) for s in range(18)], [val(cos[j][i]) for j in range(5)],
                                             val(cos[5][i]), val(cos[5][inext]), val(xs[it]),
                                             [val(cols[18 + j][it]) for j in range(4)], val(inx[it]), val(zh[zi]), ch, ks) \
                        if b else None
                    direct = rm.quotient_point(False, [val(cols[s][it]) for s in range(18)],
                                               [val(cos[j][i]) for j in range(5)], val(cos[5][i]), val(cos[5][inext]),
                                               val(xs[it]), [val(cols[18 + j][it]) for j in range(4)], val(inx[it]),
                                               val(zh[zi]), ch, ks)
                    assert want is None or want == direct            # the two forms: the same field element
                    imgs = [cols[s][it] for s in range(22)] + [cos[j][i] for j in range(6)] + \
                        [cos[5][inext], xs[it], inx[it]] + [rm.internal(v) for v in ch] + [rm.internal(k) for k in ks] + zh
                    for fold in ((1, 0) if b else (0,)):
                        if (i + fold + five) % 2 and five:           # both indexings, half of the second's points
                            continue
                        rows.append((f"Q {fold} {zi} " + _hex(imgs), ("weak", [rm.internal(direct)])))
    return rows


def lincomb_rows(rng):
    rows = []
    for n, nterms in ((8, 1), (8, 6), (8, 7), (64, 29), (8, 29)):
        for k in range(n):
            terms = []
            for t in range(nterms):
                s = rm.draw_edge(rng, rm.CANON, "internal") if t % 4 != 3 else rng.randrange(R)
                if t % 7 == 0 or k % 2:                              # odd rows: every scalar and value saturated
                    s = rm.saturated(rm.CANON)
                v = rm.saturated(rm.CANON) if k % 2 else rm.fill(rng, 1, phase=t)[0]
                terms.append((int(rng.random() < 0.85 or k % 2), s, v))
            want = sum(s * v for on, s, v in terms if on) * I261_INV % R
            rows.append((f"L {nterms} " + " ".join(f"{on} {s:x} {v:x}" for on, s, v in terms), ("exact", [want])))
    return rows


@pytest.fixture(scope="module")
def rows():
    rng = random.Random(0x20D)
    return {"grand product": perm_rows(rng), "kx columns": kx_rows(rng), "quotient": quotient_rows(rng),
            "lincomb": lincomb_rows(rng)}


def run_rows(exe, sched, lines):
    out = subprocess.run([exe, "run", str(sched)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, f"schedule {sched}: exit {out.returncode}\n" + out.stderr[-1500:]
    return out.stdout.strip().split("\n")


def check_rows(exe, sched, group):
    res = run_rows(exe, sched, [ln for ln, _ in group])
    assert len(res) == len(group)
    for (line, (how, want)), got in zip(group, res):
        got = [int(x, 16) for x in got.split()]
        assert len(got) == len(want)
        for o, w in zip(got, want):
            if how == "exact":
                assert o == w, line[:120]                            # packed canonical
            else:
                assert o % R == w and o < 2 * R and o < 1 << 256, line[:120]     # stored: below 2r


@pytest.mark.parametrize("group", ["grand product", "kx columns", "quotient", "lincomb"])
@pytest.mark.parametrize("sched", [0, 1])
def test_bodies_against_the_round_models(plain, rows, group, sched):
    assert len(rows[group]) >= 72
    check_rows(plain, sched, rows[group])


@pytest.mark.parametrize("group", ["grand product", "kx columns", "quotient", "lincomb"])
def test_no_integer_wraps_under_the_sanitizers(sanitized, rows, group):
    for sched in (0, 1):
        check_rows(sanitized, sched, rows[group])


def test_six_products_stay_within_the_bound_tables_figure(plain, sanitized):
    """ColAcc with six products of images at the class's edge - every limb saturated, 2^256 - 1, r - 1, random - through
    the real accumulator and reduce_cols (its column assertion on, nothing wraps under the sanitizer): the reduced sum's
    true magnitude is at most what the bound accumulator returns for six products of arbitrary images"""
    with open(GOLDEN) as f:
        bound = json.load(f)["rounds"]["ColAcc"]
    assert bound["products"] == 6
    rng = random.Random(6)
    sat = sum(((1 << 29) - 1) << (29 * i) for i in range(8)) | (((1 << 24) - 1) << 232)
    assert sat == M256
    lines, want = [], []
    for it in range(60):
        n = 6 if it < 40 else rng.randrange(1, 7)
        ops = [(M256, M256) if it % 4 == 0 else
               tuple(rng.choice([M256, R - 1, rm.saturated(rm.WEAK), rng.getrandbits(256)]) for _ in range(2))
               for _ in range(n)]
        lines.append(f"S {n} " + " ".join(f"{a:x} {b:x}" for a, b in ops))
        want.append(sum(a * b for a, b in ops) * I261_INV % R)
    for exe in (plain, sanitized):
        for sched in (0, 1):
            for line, got, w in zip(lines, run_rows(exe, sched, lines), want):
                x = [int(a, 16) for a in got.split()]
                v = sum(a << (29 * i) for i, a in enumerate(x))
                assert v % R == w and max(x) < 1 << 29, line[:100]
                assert v * U <= bound["reduced"] * R, f"{v / R:.3f} p above the table's {bound['reduced'] / U:.3f} p"
