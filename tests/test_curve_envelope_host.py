"""The G1 group law (cap_amd/csrc/curve29.hpp: G1Law), its quad-lane form (quad29.hpp) and the Lagrange key builder
(lagrange_elem29.hpp) on the bound-tracking field of tests/cpp/bound29.hpp, where every field operation asserts its
precondition for ALL inputs of a class - and what ties that table to the real code.

  * the envelope (tests/cpp/curve_envelope_check.cpp): every operation of the law on every path, with operands at the
    maximum of the class its comment names (T table point, R register point, A accumulator of the lean forms, M bucket
    memory up to any 32-byte image), and the chains the kernels build from them, each run to the fixed point of its class;
    the bounds are the "curve", "quad" and "lagrange" sections of tests/golden/lazy_envelope.json
    (python -m tests.test_ntt_elem_host rewrites the file);
  * negative controls: class A widened to y < 17p, and the accumulate chain restated without the weak reduction of x3,
    must fail and name the operation; zz and zzz as arbitrary images violate nothing - a positive row of the table;
  * the operations bound29.hpp gained for the law (is_zero, eq, inv, the lazy forms of mul and mul_add_mul) against the
    real ones on the base field at the precondition's edge; is_zero on every multiple of p below 2^261 and its neighbours;
  * concrete operands at the top of each class - a curve point scaled by lambda, x as its + p and y as its + 2p
    representative, lambda drawn by rejection so that zz + p and zzz + p stay inside the class, bucket images just below
    2^256 - through the real G1LT<0> and G1LT<1>, plain and under clang's integer sanitizers: the oracle's point, the
    class, and a true magnitude no larger than the table's figure.
(`-m "not gpu"`)"""
import json
import os
import random
import subprocess

import pytest

from oracle import bn254 as bn
from tests.lazy_bound_classes import C256, C261, L29, L30, L31, NORM, U, limbs_of, operand
from tests.test_field29_host import CLANG, CPP, _cxx

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "lazy_envelope.json")
SRC = os.path.join(CPP, "curve_envelope_check.cpp")
SECTIONS = ("curve", "quad", "lagrange")
P = bn.P
R261 = (1 << 261) % P
INV261 = pow(1 << 261, -1, P)
# the classes, from the headers' words (curve29.hpp's header comment, madd_acc's "Invariants of acc", quad29.hpp)
CLASS_T = [U, U]
CLASS_R = [2 * U, 2 * U, U * 11 // 10, U * 11 // 10]
CLASS_A = [2 * U, 3 * U, U * 12 // 10, U * 12 // 10]
CLASS_Q = [2 * U, 2 * U, U * 12 // 10, U * 12 // 10]
CLASS_M = C256 + 1                                                   # any 32 bytes, rounded up


def _build(out, sanitize):
    exe = str(out / "curve_envelope_check")
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
    return _build(tmp_path_factory.mktemp("curveenv"), False)


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ for the sanitizer build")
    return _build(tmp_path_factory.mktemp("curveenv_san"), True)


@pytest.fixture(params=["plain", "sanitized"])
def exe(request):
    """each build on its own: without clang++ the sanitized half skips and the plain half still runs"""
    return request.getfixturevalue(request.param)


_WORDS = {}


def same_words_in_both_builds(key, text):
    """the two builds print the same words (whichever runs second compares)"""
    assert _WORDS.setdefault(key, text) == text, f"{key}: the plain and the sanitized build differ in their words"


def curve_envelope(exe=None):
    """the "curve", "quad" and "lagrange" sections of the golden table; fails if a precondition does"""
    if exe is None:
        import pathlib
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            return curve_envelope(_build(pathlib.Path(d), False))
    out = subprocess.run([exe, "envelope"], capture_output=True, text=True)
    assert out.returncode == 0, "a precondition fails for some input of a class, or a result leaves its class:\n" + \
        out.stderr[-3000:]
    return json.loads(out.stdout)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _within(entry, cls):
    for name, top in zip(("x", "y", "zz", "zzz"), cls):
        lim, mag = entry[name]
        assert lim <= L29 and mag <= top, (entry, cls)


def test_envelope_equals_the_committed_table_and_stays_inside_the_stated_classes(plain, golden):
    env = curve_envelope(plain)
    assert sorted(env) == sorted(SECTIONS)
    for key in SECTIONS:
        assert env[key] == golden[key], f"the {key} section differs from tests/golden/lazy_envelope.json"
    cv = env["curve"]
    assert cv["classes"] == {"T": CLASS_T, "R": CLASS_R, "A": CLASS_A, "M": CLASS_M}
    lean = ("madd_acc(", "add_affine_pair(", "add_acc(")
    general = ("dbl(", "dbl_affine(", "add_mixed(A, T", "add_mixed(A, -T", "add_mixed(R,", "add_mixed(inf", "add(A, A)",
               "add(R, R)", "add(M any image, M any image)", "term_mul", "from_affine(")
    seen = 0
    for name, e in cv["ops"].items():
        if name.startswith(lean):
            _within(e, CLASS_A)
            seen += 1
        elif name.startswith(general):
            _within(e, CLASS_R)
            seen += 1
        elif name.startswith(("to_jac_ext", "store_affine")):
            assert all(m <= U for m in e.values()), name                        # canonical
        elif name.startswith("store("):
            assert all(m <= C256 for m in e.values()), name                     # below 2^256
    assert seen >= 40
    ch = cv["chains"]
    for name in ("msm_accumulate: acc", "msm_reduce_segments(item sums): S", "msm_reduce_segments(item sums): T",
                 "folds(segment sums): point"):
        _within(ch[name], CLASS_A)
    for name in ("g1_sum_kernel: acc", "k_verify_terms: acc"):
        _within(ch[name], CLASS_R)
    for name in ("msm_reduce_segments(any image): S", "folds(any image): point"):
        _within(ch[name], [CLASS_M] * 4)
    for name, e in ch.items():
        if name.endswith("to_jac_ext") or name == "k_verify_terms: out":
            assert all(m <= U for m in e.values()), name
        if name.endswith("stored") and "any image" not in name:
            assert all(m <= C256 for m in e.values()), name
    for name, e in env["quad"]["ops"].items():
        _within(e, CLASS_Q)
    _within(env["quad"]["chains"]["add / dbl from Q"], CLASS_Q)
    lg = env["lagrange"]["chains"]
    assert all(m <= C256 for m in lg["lag_stage: stored"].values()) and lg["lag_finish: out"]["x, y"] <= U
    # the stated classes close, and the table says how much further "y < k p" would: madd_acc's 4p - y needs y < 3.9p,
    # the g1_xyzz image needs y < 2^256 (5.29p)
    k = cv["largest_k_of_y"]
    assert k["madd_acc"] >= 3 and k["add_acc"] >= 3 and k["madd_acc then store"] >= 3 and k["store, load, add_acc"] >= 3
    assert k == {"madd_acc": 3, "add_acc": 126, "madd_acc then store": 3, "store, load, add_acc": 5}


@pytest.mark.parametrize("control,names", [
    ("y17", ("[madd_acc]",)),                                           # 16p + s2 - y: y must stay below 15.9p
    ("noweak", ("sub2p_lazy", "[msm_accumulate]")),                     # qq - x3 + 2p takes a weakly reduced x3
])
def test_the_envelope_fails_when_it_should(plain, control, names):
    out = subprocess.run([plain, "envelope", control], capture_output=True, text=True)
    assert out.returncode == 2, (control, out.returncode, out.stderr[-500:])
    first = out.stderr.split("\n")[0]
    assert first.startswith("bound violated in ") and all(n in first for n in names), first


# ---- the operations the bound field gained, against the real ones ----------------------------------------------------
def _line(op, sched, ops):
    return f"{op} {sched} {len(ops)} " + " ".join(
        "L " + " ".join(f"{a:x}" for a in x) + f" {cls[0]:x} {cls[1]:x} {cls[2]:x} 0" for x, cls in ops)


def test_new_bound_operations_against_the_real_ones_at_the_preconditions_edge(exe):
    rng = random.Random(0x15E)
    lines, checks = [], []
    norm_top = NORM(C261)
    # is_zero: every multiple of p below 2^261 (k = 0 .. 168) and its neighbours
    for k in range(169):
        for d in (-1, 0, 1):
            v = k * P + d
            if v < 0:
                continue
            x = limbs_of(v, L29, L29, rng, 0)
            for sched in (0, 1):
                lines.append(_line("is_zero", sched, [(x, norm_top)]))
                checks.append(("B", int(d == 0)))
    # eq: a - weak_reduce(b) + 16p with a at the top of sub's minuend class (limbs < 2^30) and b any normalized value
    a_cls = (L30, 1 << 28, C261 - 17 * U)
    for it in range(40):
        b, bx = operand(norm_top, rng, ["edge", "sat", "random", "small"][it % 4])
        if it % 2 == 0:                                                 # equal modulo p, another representative
            a, cls = b % P + rng.randrange(81) * P, NORM(82 * U)
            ax = limbs(a)
        else:
            cls = a_cls
            a, ax = operand(cls, rng, "edge" if it % 3 else "random")
        for sched in (0, 1):
            lines.append(_line("eq", sched, [(ax, cls), (bx, norm_top)]))
            checks.append(("B", int((a - b) % P == 0)))
    # inv (the field's windows and the law's square-and-multiply): limbs < 2^30, any magnitude a product can take
    for it in range(12):
        for op in ("inv", "g1_inv"):
            cls = (L30, L30, 168 * U) if op == "inv" else NORM(C256 + 1)
            v, x = operand(cls, rng, ["edge", "sat", "random"][it % 3])
            for sched in (0, 1):
                lines.append(_line(op, sched, [(x, cls)]))
                checks.append(("L", pow(v, -1, P) * R261 * R261 % P if v % P else 0))
    # the lazy forms: one un-carried operand below 2^31 against a normalized one (mul); b < 1.5 * 2^30 and c < 2^30
    # next to normalized a and d (mul_add_mul, as madd_acc calls it)
    lazy_b = (3 << 29, 3 << 29, 4 * U)
    for it in range(24):
        how = ["sat", "edge", "edge_spread", "random"][it % 4]
        a, ax = operand((L31, L31, 16 * U), rng, how)
        b, bx = operand(NORM(C261 // 2), rng, how)
        for sched in (0, 1):
            lines.append(_line("mul", sched, [(ax, (L31, L31, 16 * U)), (bx, NORM(C261 // 2))]))
            checks.append(("L", a * b * INV261 % P))
        ops = [operand(NORM(18 * U), rng, how), operand(lazy_b, rng, how), operand((L30, L30, 4 * U), rng, how),
               operand(NORM(2 * U), rng, how)]
        cl = [NORM(18 * U), lazy_b, (L30, L30, 4 * U), NORM(2 * U)]
        for sched in (0, 1):
            lines.append(_line("mul_add_mul", sched, [(o[1], c) for o, c in zip(ops, cl)]))
            checks.append(("L", (ops[0][0] * ops[1][0] + ops[2][0] * ops[3][0]) * INV261 % P))
    out = subprocess.run([exe, "ops"], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-1500:]
    res = out.stdout.strip().split("\n")
    assert len(res) == len(checks)
    for line, got, (kind, want) in zip(lines, res, checks):
        t = got.split()
        assert t[0] == kind, line
        if kind == "B":
            assert int(t[1]) == want, line
            continue
        x = [int(a, 16) for a in t[1:10]]
        lo, hi, mag = (int(a, 16) for a in t[10:13])
        v = sum(a << (29 * i) for i, a in enumerate(x))
        assert v % P == want, line
        assert max(x[:8]) <= lo and x[8] <= hi, f"{line}\n-> {got}: a limb above the bound table's"
        assert v * U <= mag * P, f"{line}\n-> {got}: {v / P:.4f} p, above the bound table's {mag / U:.4f} p"


# ---- top-of-class concrete operands through the real law ------------------------------------------------------------
def mont(v):
    return v * R261 % P


def limbs(v):
    assert v < 1 << 261
    return [(v >> (29 * i)) & L29 for i in range(8)] + [v >> 232]


def _hex(vals):
    return " ".join(" ".join(f"{a:x}" for a in limbs(v)) for v in vals)


class Pt:
    """an XYZZ register point: the affine point it stands for and the four representatives it is held as"""

    def __init__(self, aff, coords):
        self.aff, self.coords = aff, coords


def curve_point(rng):
    return bn.g1_mul(bn.G1_GEN, rng.randrange(1, bn.R))


def top_of_class(rng, aff, kx, ky, kz, zmax):
    """aff scaled by lambda: x + kx p, y + ky p, zz + kz p, zzz + kz p, lambda drawn until zz, zzz + kz p < zmax p / 2^20"""
    X, Y = aff
    while True:
        lam = rng.randrange(1, P)
        zz, zzz = mont(lam * lam % P), mont(pow(lam, 3, P))
        if (zz + kz * P) * U < zmax * P and (zzz + kz * P) * U < zmax * P:
            break
    return Pt(aff, [mont(X * lam * lam % P) + kx * P, mont(Y * pow(lam, 3, P) % P) + ky * P, zz + kz * P, zzz + kz * P])


def bucket_image(rng, aff):
    """the same point as a 32-byte image just below 2^256: every coordinate its largest representative"""
    pt = top_of_class(rng, aff, 0, 0, 0, 2 * U)
    pt.coords = [v + ((1 << 256) - 1 - v) // P * P for v in pt.coords]
    return pt


def table_point(aff):
    return [mont(aff[0]), mont(aff[1])]


def decode(vals):
    x, y, zz, zzz = (v * INV261 % P for v in vals)
    if zz == 0:
        return bn.INF
    assert pow(zz, 3, P) == zzz * zzz % P
    return (x * pow(zz, -1, P) % P, y * pow(zzz, -1, P) % P)


def concrete_cases(rng):
    """-> [(line, expected affine point, golden entry, class)]"""
    cases = []
    neg = bn.g1_neg
    for it in range(6):
        a, b, c = curve_point(rng), curve_point(rng), curve_point(rng)
        A1, A2, A3 = (top_of_class(rng, p, 1, 2, 1, CLASS_A[2]) for p in (a, b, c))
        R1, R2 = (top_of_class(rng, p, 1, 1, 1, CLASS_R[2]) for p in (a, b))
        M1, M2 = bucket_image(rng, a), bucket_image(rng, b)
        tb, tc = table_point(b), table_point(c)
        for n in (0, 1):
            sign = "-T" if n else "T"
            cases.append((f"madd {_hex(A1.coords)} {_hex(tb)} {n}", bn.g1_add(a, neg(b) if n else b),
                          ("ops", f"madd_acc(A, {sign})"), CLASS_A))
            cases.append((f"addmixed {_hex(A1.coords)} {_hex(tb)} {n}", bn.g1_add(a, neg(b) if n else b),
                          ("ops", f"add_mixed(A, {sign})"), CLASS_R))
            for n1 in (0, 1):
                cases.append((f"pair {_hex(tb)} {n} {_hex(tc)} {n1}",
                              bn.g1_add(neg(b) if n else b, neg(c) if n1 else c),
                              ("ops", f"add_affine_pair({'-T' if n else 'T'}, {'-T' if n1 else 'T'})"), CLASS_A))
        cases.append((f"addacc {_hex(A1.coords)} {_hex(A2.coords)}", bn.g1_add(a, b), ("ops", "add_acc(A, A)"), CLASS_A))
        cases.append((f"add {_hex(A1.coords)} {_hex(A2.coords)}", bn.g1_add(a, b), ("ops", "add(A, A)"), CLASS_R))
        cases.append((f"add {_hex(R1.coords)} {_hex(R2.coords)}", bn.g1_add(a, b), ("ops", "add(R, R)"), CLASS_R))
        cases.append((f"dbl {_hex(A1.coords)}", bn.g1_add(a, a), ("ops", "dbl(A)"), CLASS_R))
        cases.append((f"dbl {_hex(R1.coords)}", bn.g1_add(a, a), ("ops", "dbl(R)"), CLASS_R))
        cases.append((f"dblaffine {_hex(tb)}", bn.g1_add(b, b), ("ops", "dbl_affine(T)"), CLASS_R))
        cases.append((f"addacc {_hex(M1.coords)} {_hex(M2.coords)}", bn.g1_add(a, b),
                      ("ops", "add_acc(M any image, M any image)"), CLASS_A))
        cases.append((f"add {_hex(M1.coords)} {_hex(M2.coords)}", bn.g1_add(a, b),
                      ("ops", "add(M any image, M any image)"), CLASS_R))
        cases.append((f"dbl {_hex(M1.coords)}", bn.g1_add(a, a), ("ops", "dbl(M any image)"), CLASS_R))
        # the item chain and the fold chain
        pts = [curve_point(rng) for _ in range(8)]
        signs = [(it >> 0) & 1, (it >> 1) & 1] + [(it + j) & 1 for j in range(6)]
        want = bn.INF
        for p, s in zip(pts, signs):
            want = bn.g1_add(want, neg(p) if s else p)
        cases.append(("item " + " ".join(f"{_hex(table_point(p))} {s}" for p, s in zip(pts, signs)), want,
                      ("chains", "msm_accumulate: acc"), CLASS_A))
        s3 = bn.g1_add(bn.g1_add(a, b), c)
        cases.append((f"fold {_hex(A1.coords)} {_hex(A2.coords)} {_hex(A3.coords)}", bn.g1_add(s3, s3),
                      ("ops", "dbl(A)"), CLASS_R))
    return cases


@pytest.mark.parametrize("sched", [0, 1])
def test_top_of_class_operands_through_the_real_law(exe, golden, sched):
    cases = concrete_cases(random.Random(0xC1A55))
    text = "\n".join(c[0] for c in cases) + "\n"
    out = subprocess.run([exe, "run", str(sched)], input=text, capture_output=True, text=True)
    assert out.returncode == 0, f"schedule {sched}: exit {out.returncode}\n" + out.stderr[-1500:]
    same_words_in_both_builds(("top", sched), out.stdout)
    res = out.stdout.strip().split("\n")
    pos = 0
    for line, want, (sec, entry), cls in cases:
        t = res[pos].split()
        pos += 1
        assert t[0] == "1", line[:60]                                   # the lean form took its common path
        x = [int(a, 16) for a in t[1:]]
        assert len(x) == 36 and max(x) <= L29, line[:60]                 # normalized limbs
        vals = [sum(a << (29 * i) for i, a in enumerate(x[9 * c:9 * c + 9])) for c in range(4)]
        assert decode(vals) == want, line[:60]
        bound = golden["curve"][sec][entry]
        for v, name, top in zip(vals, ("x", "y", "zz", "zzz"), cls):
            assert v * U <= top * P, (line[:60], name, v / P)            # the class its comment names
            assert v * U <= bound[name][1] * P, f"{line[:60]} {name}: {v / P:.4f} p above the table's " \
                                                f"{bound[name][1] / U:.4f} p"
        if line.startswith("fold"):
            xj, yj, zj = (int(w, 16) for w in res[pos].split())
            pos += 1
            assert max(xj, yj, zj) < P                                   # the C ABI: canonical
            inv256 = pow(1 << 256, -1, P)
            xj, yj, zj = (w * inv256 % P for w in (xj, yj, zj))
            zi = pow(zj, -1, P)
            assert (xj * zi * zi % P, yj * pow(zi, 3, P) % P) == want
    assert pos == len(res)


# ---- the remaining operations and chains through the real law ---------------------------------------------------------
def _words8(k):
    return " ".join(f"{(k >> (32 * i)) & 0xffffffff:x}" for i in range(8))


def _pt_of(tokens):
    x = [int(a, 16) for a in tokens]
    assert len(x) == 36 and max(x) <= L29
    return [sum(a << (29 * i) for i, a in enumerate(x[9 * c:9 * c + 9])) for c in range(4)]


def _check_point(t, want, cls, bound, what):
    """one printed point: the oracle's point, the class, and a magnitude at most the table's figure"""
    assert t[0] == "1", what
    vals = _pt_of(t[1:])
    assert decode(vals) == want, what
    for v, name, top in zip(vals, ("x", "y", "zz", "zzz"), cls):
        assert v * U <= top * P, (what, name, v / P)
        b = bound[name][1] if isinstance(bound[name], list) else bound[name]
        assert v * U <= b * P, f"{what} {name}: {v / P:.4f} p above the table's {b / U:.4f} p"


def _mul(pt, k):
    return bn.g1_mul(pt, k % bn.R) if pt is not None and k % bn.R else bn.INF


@pytest.mark.parametrize("sched", [0, 1])
def test_remaining_operations_and_chains_through_the_real_law(exe, golden, sched):
    """term_mul, to_affine with store_affine, to_jac_ext of a bucket image, both inversions, the S / T walk of
    msm_reduce_segments with an empty bucket, a copy and the equal-operand fallback, mul_small, the window Horner, the
    body of g1_sum_kernel on Jacobian triples just below 2^256, the quad form, the butterfly of lag_stage, lag_finish in both ranges of j and the sum of k_verify_terms - operands at the top of their classes, plain and under the
    sanitizers: the oracle's value, the class, a magnitude at most the golden table's"""
    rng = random.Random(0x70B + sched)
    cv, top = golden["curve"], (1 << 256) - 1
    lines, checks = [], []                                              # checks: functions over the output lines
    neg, add = bn.g1_neg, bn.g1_add
    inv256 = pow(1 << 256, -1, P)

    def ext(w):
        v = int(w, 16)
        assert v < P
        return v * inv256 % P
    for it in range(3):
        a, b = curve_point(rng), curve_point(rng)
        A, B = top_of_class(rng, a, 1, 2, 1, CLASS_A[2]), top_of_class(rng, b, 1, 2, 1, CLASS_A[2])
        M = bucket_image(rng, a)
        lazy_q = [mont(b[0]) + P, mont(b[1]) + P]                       # the ABI point's class: products, < 2p
        for k in (top, top - 1 - it, rng.getrandbits(256), 3):
            lines.append(f"termmul {_hex(lazy_q)} {_words8(k)}")
            checks.append((1, lambda o, k=k, b=b: _check_point(o[0], _mul(b, k), CLASS_R,
                                                               cv["ops"]["term_mul: closure over all digit orders"], "term_mul")))
        for pt, src, key in ((A, a, "to_affine(A)"), (M, a, "to_affine(M any image)")):
            lines.append(f"toaffine {_hex(pt.coords)}")

            def chk(o, src=src, key=key):
                vals = _pt_of(o[0][1:])
                assert (vals[0] * INV261 % P, vals[1] * INV261 % P) == src
                for v, name in zip(vals[:2], ("x", "y")):
                    assert v < 2 * P and v * U <= cv["ops"][key][name][1] * P, key
                assert [int(w, 16) for w in o[1]] == [mont(src[0]), mont(src[1])]      # store_affine: canonical
            checks.append((2, chk))
        lines.append(f"jac {_hex(M.coords)}")

        def chk_jac(o, a=a):
            xj, yj, zj = (ext(w) for w in o[0])
            zi = pow(zj, -1, P)
            assert (xj * zi * zi % P, yj * pow(zi, 3, P) % P) == a
        checks.append((1, chk_jac))
        for v in (M.coords[3], A.coords[3], top):
            lines.append(f"inv {_hex([v])}")

            def chk_inv(o, v=v):
                vals = _pt_of(o[0][1:])
                want = pow(v, -1, P) * R261 * R261 % P
                assert vals[1] % P == want and vals[2] % P == want
                assert vals[1] * U <= cv["ops"]["inv(any image)"]["out"][1] * P
                assert vals[2] * U <= cv["ops"]["F::inv(any image)"]["out"][1] * P
            checks.append((1, chk_inv))
        # the walks: an empty bucket right after the top one (T == S: add_acc refuses, add doubles) and one in the middle
        # (a skip); then the top bucket empty (S and T start at infinity: copies)
        pts = [curve_point(rng) for _ in range(5)]
        for bks in ([pts[0], None, pts[1], pts[2], None, pts[3]], [pts[0], pts[1], None, pts[2], pts[3], None]):
            lines.append("segwalk 6 " + " ".join(_hex(top_of_class(rng, p, 1, 2, 1, CLASS_A[2]).coords) if p else
                                                 _hex([0] * 4) for p in bks))

            def chk_walk(o, bks=bks):
                S = T = bks[-1]
                for cur in reversed(bks[:-1]):
                    S = add(S, cur)
                    T = add(T, S)
                for t, want in zip(o, (S, T)):
                    _check_point(t, want, CLASS_A, {n: CLASS_M for n in ("x", "y", "zz", "zzz")}, "msm_reduce_segments")
            checks.append((2, chk_walk))
        for k in (1, 2, 0xffffffff, 0x80000001):
            lines.append(f"mulsmall {_hex(A.coords)} {k}")
            checks.append((1, lambda o, k=k, a=a: _check_point(o[0], _mul(a, k), CLASS_A, cv["chains"]["folds(any image): point"],
                                                               "mul_small")))
        sums = [curve_point(rng), None, curve_point(rng), curve_point(rng)]
        lines.append("horner 5 4 " + " ".join(_hex(top_of_class(rng, p, 1, 2, 1, CLASS_A[2]).coords) if p else _hex([0] * 4)
                                              for p in sums))

        def chk_horner(o, sums=sums):
            want = bn.INF
            for p in sums:
                want = add(_mul(want, 32), p)
            _check_point(o[0], want, CLASS_A, cv["chains"]["folds(any image): point"], "msm_var_horner")
        checks.append((1, chk_horner))
        # Jacobian triples of the C ABI as a caller may write them: every word its largest representative below 2^256
        jac = []
        for p in (a, b, None, pts[4]):
            if p is None:
                jac.append((p, [top, top, 0]))
                continue
            z = rng.randrange(1, P)
            w = [p[0] * z * z % P, p[1] * pow(z, 3, P) % P, z]
            jac.append((p, [(v << 256) % P + (top - (v << 256) % P) // P * P for v in w]))
        lines.append("g1sum 4 " + " ".join(_words8(v) for _, w in jac for v in w))

        def chk_sum(o, jac=jac):
            want = bn.INF
            for p, _ in jac:
                want = add(want, p)
            want = add(want, want)
            _check_point(o[0], want, CLASS_R, cv["chains"]["g1_sum_kernel: acc"], "g1_sum_kernel")
            xj, yj, zj = (ext(w) for w in o[1])
            zi = pow(zj, -1, P)
            assert (xj * zi * zi % P, yj * pow(zi, 3, P) % P) == want
        checks.append((2, chk_sum))
        QA, QB = top_of_class(rng, a, 1, 1, 1, CLASS_Q[2]), top_of_class(rng, b, 1, 1, 1, CLASS_Q[2])
        lines.append(f"quad {_hex(QA.coords)} {_hex(QB.coords)}")

        def chk_quad(o, a=a, b=b):
            s = add(a, b)
            for t, want, key in zip(o, (s, add(s, s), add(add(s, s), b)), ("add(Q, Q)", "dbl(Q)", "add(Q, Q)")):
                _check_point(t, want, CLASS_Q, golden["quad"]["ops"][key], "quad " + key)
        checks.append((3, chk_quad))
        for k, has in ((rng.getrandbits(254), 1), (bn.R - 1, 1), (1, 0)):
            lines.append(f"lagstage {_hex(A.coords)} {_hex(B.coords)} {_words8(k)} {has}")

            def chk_lag(o, a=a, b=b, k=k):
                kb = _mul(b, k)
                for t, want in zip(o, (add(a, kb), add(a, neg(kb)))):
                    _check_point(t, want, CLASS_R, golden["lagrange"]["chains"]["lag_stage: stored"], "lag_stage")
            checks.append((2, chk_lag))
        # lag_finish, n = 2: the array as store() wrote a top-of-class point and a bucket image, canonical SRS rows; both
        # ranges of j - [n_inv] a[j], and the blinding points srs[j] - srs[j - n] (equal rows: the point at infinity)
        rows = [curve_point(rng), curve_point(rng), curve_point(rng), None]
        rows[3] = rows[1]
        n_inv = (top, rng.getrandbits(254), pow(2, -1, bn.R))[it]
        for j in range(4):
            lines.append(f"lagfinish {j} {_words8(n_inv)} {_hex(A.coords)} {_hex(bucket_image(rng, b).coords)} " +
                         " ".join(_hex(table_point(q)) for q in rows))

            def chk_fin(o, j=j, n_inv=n_inv, a=a, b=b, rows=rows):
                want = _mul((a, b)[j], n_inv) if j < 2 else add(rows[j], neg(rows[j - 2]))
                words = [int(w, 16) for w in o[0]]
                assert max(words) * U <= golden["lagrange"]["chains"]["lag_finish: out"]["x, y"] * P     # canonical
                assert (ext(o[0][0]), ext(o[0][1])) == (want if want is not None else (0, 0))
            checks.append((1, chk_fin))
        terms = [(curve_point(rng), k) for k in (top, rng.getrandbits(256), 1, 2)]
        lines.append("terms 4 " + " ".join(f"{_hex([mont(q[0]) + P, mont(q[1]) + P])} {_words8(k)}" for q, k in terms))

        def chk_terms(o, terms=terms):
            want = bn.INF
            for q, k in terms:
                want = add(want, _mul(q, k))
            assert (ext(o[0][0]), ext(o[0][1])) == neg(want)
        checks.append((1, chk_terms))
    text = "\n".join(lines) + "\n"
    out = subprocess.run([exe, "run", str(sched)], input=text, capture_output=True, text=True)
    assert out.returncode == 0, f"schedule {sched}: exit {out.returncode}\n" + out.stderr[-1500:]
    same_words_in_both_builds(("remaining", sched), out.stdout)
    res = [ln.split() for ln in out.stdout.strip().split("\n")]
    pos = 0
    for n, chk in checks:
        chk(res[pos:pos + n])
        pos += n
    assert pos == len(res)
