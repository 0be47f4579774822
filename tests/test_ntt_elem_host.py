"""The arithmetic of the NTT kernels (cap_amd/csrc/ntt_elem29.hpp: the stages of lds_ntt, the element steps of the column
and row passes, the bodies of ntt3_combine / ntt3_combine5) on the host, where the bound assertions of field29.hpp
(CAP_FL_CHECK) are compiled in - on the GPU they are not - and a second time on a field whose values are bounds.

  * whole tile transforms through the shared stage functions, threads emulated between the barriers, for log_len 1 .. 11
    and tile widths 1, 4, 16, followed by every input / output form of the plans, against Python-integer DFTs: residue
    and representation of every output word; both multiplication schedules, both twiddle forms, plain and under clang's
    integer sanitizers (a stand-alone program);
  * the envelope: the same templates on tests/cpp/bound29.hpp, where every operation asserts its precondition for ALL
    values of the operands' class - regenerated and compared with tests/golden/lazy_envelope.json, so a change that
    moves a bound shows up in review (python -m tests.test_ntt_elem_host rewrites the file);
  * what ties the envelope to the real code: each operation's postcondition against the real operation on operands at
    the precondition's edge, and each stage's bound against the largest value the concrete runs hold there.
(`-m "not gpu"`)"""
import json
import os
import random
import struct
import subprocess
import sys

import pytest

from oracle import bn254 as bn
from tests.test_field29_host import CLANG, CPP, _cxx
from tools.ntt_conformance import INPUTS

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "lazy_envelope.json")
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
INV261 = pow(1 << 261, -1, R)
M256 = (1 << 256) - 1
# inputs built to sit near the envelope: every limb saturated inside the class, and zeros on every subtracted operand
# with the largest admitted value on the minuend chain (row 0 is the minuend of every butterfly it meets)
TIGHT = ["max_all", "max_impulse_0", "max_padded_half"]
OUT_FORMS = ["col_tw", "col_tw_scaled", "row_canonical", "row_post_scale", "row_post_scalar", "row_post_scale_lazy_out",
             "row_lazy_out"]
IN_CLASS = ["raw_256", "pre_scaled", "pre_scaled_fold"]
VARIANTS = [(0, 1), (1, 1), (0, 0), (1, 0)]                         # (schedule, Shoup twiddles)


def _bits(rng, n):
    return rng.getrandbits(n)


def _field(rng):
    return _bits(rng, 300) % R


def make_column(name, n, rng):
    """the input families of tools/ntt_conformance.py (same names, same shapes) as Python integers, plus TIGHT"""
    rnd = lambda: [_field(rng) for _ in range(n)]
    if name in ("random", "random_b"):
        return rnd()
    if name == "zero":
        return [0] * n
    if name == "all_rm1":
        return [R - 1] * n
    if name == "alt_rm1_one":
        return [1 if i & 1 else R - 1 for i in range(n)]
    if name in ("zeros90", "rm1_90"):
        fill = 0 if name == "zeros90" else R - 1
        return [fill if _bits(rng, 16) < 58982 else _field(rng) for _ in range(n)]
    if name.startswith("impulse_"):
        pos = {"impulse_0": 0, "impulse_1": 1 % n, "impulse_half_m1": max(n // 2 - 1, 0), "impulse_half": n // 2,
               "impulse_last": n - 1, "impulse_seeded": _bits(rng, 32) % n}[name]
        x = [0] * n
        x[pos] = _field(rng)
        return x
    if name == "padded_half_plus_2":
        return [v if i < min(n, n // 2 + 2) else 0 for i, v in enumerate(rnd())]
    if name == "odd_only":
        return [v if i & 1 else 0 for i, v in enumerate(rnd())]
    if name == "three_mod_four_only":
        return [v if i % 4 == 3 else 0 for i, v in enumerate(rnd())]
    if name == "x_plus_r":
        return [v + R for v in rnd()]
    if name == "max_all":
        return [M256] * n
    if name == "max_impulse_0":
        return [M256] + [0] * (n - 1)
    if name == "max_padded_half":
        return [M256 if i < max(n // 2, 1) else 0 for i in range(n)]
    raise ValueError(name)


def _factor(rng):
    """a 32-byte table entry or scalar: any image, the edges now and then"""
    k = _bits(rng, 4)
    return [0, 1, R - 1, R, M256, R + 1][k] if k < 6 else _bits(rng, 256)


def dft(v, w):
    """X[k] = sum_j v[j] w^(jk) mod r, w of order len(v): decimation in time on Python integers"""
    n = len(v)
    if n == 1:
        return list(v)
    ev, od = dft(v[0::2], w * w % R), dft(v[1::2], w * w % R)
    out, t = [0] * n, 1
    for k in range(n // 2):
        x = t * od[k] % R
        out[k], out[k + n // 2] = (ev[k] + x) % R, (ev[k] - x) % R
        t = t * w % R
    return out


def _words(vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)


class Case:
    pass


def build_cases():
    rng = random.Random(0x1A2B)
    names = INPUTS + TIGHT
    cases = []
    for log_len in range(1, 12):
        n = 1 << log_len
        w = bn.root_of_unity(log_len)
        tiles = []                                              # (log_c, in_form, column names)
        for log_c in (0, 2, 4):
            if log_len + log_c > 11:
                continue
            C = 1 << log_c
            nt = -(-len(names) // C)
            tiles += [(log_c, t % 3, [names[(t * C + c) % len(names)] for c in range(C)], False) for t in range(nt)]
        tiles += [(0, 0, [name], True) for name in TIGHT]        # the tightness figures: raw images, no pre-scale
        for log_c, in_form, cols, tight in tiles:
            c = Case()
            c.log_len, c.log_c, c.in_form, c.cols, c.index, c.tight = log_len, log_c, in_form, cols, len(cases), tight
            C = 1 << log_c
            c.raw = [make_column(name, n, rng) for name in cols]
            c.pre = [[_factor(rng) for _ in range(n)] for _ in range(C)] if in_form >= 1 else None
            c.fraw = [[_factor(rng) for _ in range(n)] for _ in range(C)] if in_form == 2 else None
            c.fpre = [[_factor(rng) for _ in range(n)] for _ in range(C)] if in_form == 2 else None
            # inter-pass twiddles come from the domain's own tables, canonical; post-scale factors are any image
            c.outf = [[_factor(rng) % (R if (k + ci + c.index) % 7 < 2 else 1 << 256) for ci in range(C)] for k in range(n)]
            c.tw = [pow(w, i, R) for i in range(n // 2)]
            c.X = []
            for ci in range(C):
                v = list(c.raw[ci])
                if in_form >= 1:
                    v = [x * f % R * INV261 % R if x else 0 for x, f in zip(v, c.pre[ci])]
                if in_form == 2:
                    v = [(x + a * b % R * INV261) % R for x, a, b in zip(v, c.fraw[ci], c.fpre[ci])]
                c.X.append(dft([x % R for x in v], w))
            cases.append(c)
    blob = [struct.pack("<I", len(cases))]
    for c in cases:
        blob.append(struct.pack("<4I", c.log_len, c.log_c, c.in_form, c.index))
        blob.append(_words(c.tw))
        for arr in (c.raw, c.pre, c.fraw, c.fpre):
            if arr is not None:
                blob += [_words(col) for col in arr]
        blob += [_words(row) for row in c.outf]
    return cases, b"".join(blob)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    cs, blob = build_cases()
    path = tmp_path_factory.mktemp("nttelem_in") / "cases.bin"
    path.write_bytes(blob)
    return cs, str(path)


def _build(out, sanitize):
    exe = str(out / "ntt_elem_check")
    src = os.path.join(CPP, "ntt_elem_check.cpp")
    if sanitize:
        ign = out / "ignore.txt"
        ign.write_text("src:*/field.hpp\nsrc:*/curve.hpp\n")
        cmd = [CLANG, "-O1", "-std=c++17", "-fsanitize=unsigned-integer-overflow,undefined",
               f"-fsanitize-ignorelist={ign}", "-fno-sanitize-recover=all", src, "-o", exe]
    else:
        cmd = [_cxx(), "-O1", "-std=c++17", src, "-o", exe]
    subprocess.check_call(cmd)
    return exe


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("nttelem"), False)


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ for the sanitizer build")
    return _build(tmp_path_factory.mktemp("nttelem_san"), True)


def envelope_of(exe):
    out = subprocess.run([exe, "envelope"], capture_output=True, text=True)
    assert out.returncode == 0, "a precondition fails for some input of a class:\n" + out.stderr[-3000:]
    return json.loads(out.stdout)


def run_variant(exe, path, sched, shoup, tmp):
    res = os.path.join(str(tmp), f"out_{sched}_{shoup}.bin")
    out = subprocess.run([exe, "run", str(sched), str(shoup), path, res], capture_output=True, text=True)
    assert out.returncode == 0, f"schedule {sched} shoup {shoup}: exit {out.returncode}\n" + out.stderr[-1500:]
    with open(res, "rb") as f:
        return f.read()


def check_outputs(cs, data, env, what):
    """every output word against the Python DFT (residue and representation), and every stage maximum against the
    envelope; -> {log_len: {tight input: share of the envelope at the last stage}}"""
    form_env = env["ntt"]["shoup" if what[1] else "montgomery"]
    U = env["unit_per_p"]
    pos, tight = 0, {}
    for c in cs:
        n, C = 1 << c.log_len, 1 << c.log_c
        (nrec,) = struct.unpack_from("<I", data, pos)
        pos += 4
        bound = form_env[str(c.log_len)][IN_CLASS[c.in_form]]["lds"]
        assert nrec == len(bound), (what, c.log_len, nrec)
        for r in range(nrec):
            limbs = struct.unpack_from("<9I", data, pos)
            pos += 36
            v = sum(x << (29 * i) for i, x in enumerate(limbs))
            assert v * U <= bound[r] * R, f"{what} log_len {c.log_len} {c.cols}: the tile holds {v / R:.2f} r behind " \
                                          f"stage {r}, above the envelope's {bound[r] / U:.2f} r"
        if c.tight:
            tight.setdefault(str(c.log_len), {})[c.cols[0]] = (v * U * 10000 // (bound[-1] * R)) / 10000
        for k in range(n):
            for ci in range(C):
                o = int.from_bytes(data[pos:pos + 32], "little")
                pos += 32
                form, f, x = (k + ci + c.index) % 7, c.outf[k][ci], c.X[ci][k]
                scaled = x * f % R * INV261 % R
                where = f"{what} case {c.index} log_len {c.log_len} log_c {c.log_c} in_form {c.in_form} " \
                        f"{c.cols[ci % len(c.cols)]} k {k} {OUT_FORMS[form]}"
                if form == 0:
                    assert o % R == (x if k == 0 else scaled) and o < 2 * R, where     # packed weak
                elif form == 1:
                    assert o % R == scaled and o < 2 * R, where
                elif form == 2:
                    assert o == x, where                                              # packed canonical
                elif form in (3, 4):
                    assert o == scaled, where
                elif form == 5:
                    assert o % R == scaled and o < 2 * R and o < 1 << 256, where      # stored
                else:
                    assert o % R == x and o < 2 * R and o < 1 << 256, where
    assert pos == len(data)
    return tight


@pytest.fixture(scope="module")
def envelope(plain):
    return envelope_of(plain)


@pytest.mark.parametrize("sched,shoup", VARIANTS)
def test_tiles_and_element_steps_against_python_dfts(plain, cases, envelope, tmp_path, sched, shoup):
    cs, path = cases
    check_outputs(cs, run_variant(plain, path, sched, shoup, tmp_path), envelope, (sched, shoup))


@pytest.mark.parametrize("sched,shoup", VARIANTS)
def test_no_integer_wraps_under_the_sanitizers(sanitized, cases, envelope, tmp_path, sched, shoup):
    cs, path = cases
    check_outputs(cs, run_variant(sanitized, path, sched, shoup, tmp_path), envelope, (sched, shoup))
    assert envelope_of(sanitized) == envelope


def test_bound_constants(envelope):
    k = envelope["constants"]
    assert envelope["unit_per_p"] == 1 << 20
    assert k == {"C256": (1 << 276) // R, "C261": (1 << 281) // R, "C262": (1 << 282) // R,
                 "RT": -(-R >> 212), "RQ": -(-R >> 197)}
    P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47                # the base field: the same
    assert k == {"C256": (1 << 276) // P, "C261": (1 << 281) // P, "C262": (1 << 282) // P,
                 "RT": -(-P >> 212), "RQ": -(-P >> 197)}


def full_envelope(exe, cs, path, tmp):
    env = envelope_of(exe)
    env["ntt_tightness"] = {}
    for shoup in (1, 0):
        env["ntt_tightness"]["shoup" if shoup else "montgomery"] = check_outputs(
            cs, run_variant(exe, path, 0, shoup, tmp), env, (0, shoup))
    return env


def test_envelope_equals_the_committed_table(plain, cases, tmp_path):
    """No precondition fails for any input of a class, and the table of bounds is the committed one.  The share of the
    envelope that the tightness inputs reach is part of the table (a figure for the reader, no threshold)."""
    cs, path = cases
    env = full_envelope(plain, cs, path, tmp_path)
    with open(GOLDEN) as f:
        want = json.load(f)
    # tests/test_round_elem_host.py, test_curve_envelope_host.py and test_tower_envelope_host.py own these sections
    want = {k: v for k, v in want.items() if k not in ("rounds", "curve", "quad", "lagrange", "tower")}
    assert sorted(env) == sorted(want)
    for key in env:
        assert env[key] == want[key], f"{key} differs from tests/golden/lazy_envelope.json"
    for form in ("shoup", "montgomery"):
        for ll in range(1, 12):
            for cl, t in env["ntt"][form][str(ll)].items():
                assert max(t["lds"]) <= env["constants"]["C261"]                     # LDS holds normalized values
                for name, mag in t["mem"].items():                                  # packed canonical: < r, weak: < 2r
                    assert mag <= (1 if name in OUT_FORMS[2:5] else 2) << 20, (form, ll, cl, name)


# ---- every operation of the bound table against the real operation ---------------------------------------------------
from tests.lazy_bound_classes import (C256, C261, C262, L29, L30, L31, NORM, SUB2, SUB4, SUB8, SUB16, TOP, U,  # noqa: E402,F401
                                      limbs_of, operand)
OPS = {  # op: (operand classes at the edge of the precondition, expected residue)
    "normalize": ([((1 << 32) - 9, (1 << 29) - 9, C261)], lambda a: a),
    "weak_reduce": ([NORM(C261)], lambda a: a),
    "canonical": ([NORM(C261)], lambda a: a),
    "add": ([(L31, L31, C262), (L31, L31, C262)], lambda a, b: a + b),
    "add_norm": ([(L30, 1 << 27, C261 // 2), (L30, 1 << 27, C261 // 2)], lambda a, b: a + b),
    "sub": ([(L30, 1 << 28, C261 - 17 * U), (L30, SUB16, U * 159 // 10)], lambda a, b: a - b),
    "sub_from_lazy": ([(L31, 1 << 28, C261 - 17 * U), (L30, SUB16, U * 159 // 10)], lambda a, b: a - b),
    "sub2p": ([(L31, 1 << 28, C261 - 3 * U), NORM(U * 19 // 10)], lambda a, b: a - b),
    "sub2p_lazy": ([(L30, 1 << 28, C261), NORM(U * 19 // 10)], lambda a, b: a - b),
    "sub8p": ([(L31, 1 << 28, C261 - 9 * U), NORM(U * 799 // 100)], lambda a, b: a - b),
    "sub8p_lazy": ([(L30, 1 << 28, C261), NORM(U * 799 // 100)], lambda a, b: a - b),
    "neg": ([(L30, SUB16, U * 159 // 10)], lambda b: -b),
    "neg_lazy": ([NORM(U * 159 // 10)], lambda b: -b),
    "neg2p_lazy": ([NORM(U * 19 // 10)], lambda b: -b),
    "neg4p_lazy": ([NORM(U * 39 // 10)], lambda b: -b),
    "mul": ([(L30, L30, 168 * U), (L30, L30, 168 * U)], lambda a, b: a * b * INV261),
    "sqr": ([(L30, L30, 168 * U)], lambda a: a * a * INV261),
    "mul_shoup": ([(L30, L30, C262), NORM(U) + (True,)], lambda a, w: a * w),
    "mul_add_mul": ([NORM(91 * U)] * 4, lambda a, b, c, d: (a * b + c * d) * INV261),
    "pack": ([(L29, (1 << 24) - 1, C256)], lambda a: a),
    "store": ([NORM(C261)], lambda a: a),
    "to_ext": ([(L30, L30, 168 * U)], lambda a: a * INV261 << 256),
}
OPS_LAZY_WEAK = ([(L30, L30, C261)], lambda a: a)                                  # one lazy sum of two, as k_perm_numden
OPS_LAZY_MUL = ([(L31, L31, 16 * U), NORM(C261 // 2)], lambda a, b: a * b * INV261)   # neg_lazy's result as a multiplicand
OPS_SHOUP_4P = ([(L30, L29, C261), NORM(U) + (True,)], lambda a, w: a * w)             # a < 2^261: below 4p
IMAGE_OPS = {"load": lambda a: a, "from_ext": lambda a: a * 32}


def test_every_postcondition_of_the_bound_table_holds_for_the_real_operation(plain):
    """Operands at the precondition's edge (largest magnitude, saturated limbs, carries pushed down) and random ones
    through the real operation with its assertions on; the result's limbs and true magnitude stay within what the bound
    operation returns for the operands' class.  A precondition the class violates ends the program (exit 2)."""
    rng = random.Random(77)
    lines, checks = [], []
    table = [(op, cl, fn) for op, (cl, fn) in OPS.items()] + [("mul",) + OPS_LAZY_MUL, ("mul_shoup",) + OPS_SHOUP_4P,
                                                              ("weak_reduce",) + OPS_LAZY_WEAK]
    for op, classes, fn in table:
        for sched in (0, 1):
            for how in ["sat", "edge", "edge_spread", "small"] + ["random"] * 12 + ["edge"] * 6:
                vals, txt = [], []
                for cls in classes:
                    v, x = operand(cls, rng, how)
                    vals.append(v)
                    txt.append("L " + " ".join(f"{a:x}" for a in x) + f" {cls[0]:x} {cls[1]:x} {cls[2]:x} 0")
                lines.append(f"{op} {sched} {len(classes)} " + " ".join(txt))
                checks.append((op, fn(*vals) % (1 << 256 if op == "pack" else R)))     # pack: the same integer
    for op, fn in IMAGE_OPS.items():
        for sched in (0, 1):
            for v in [0, 1, R - 1, R, M256] + [rng.getrandbits(256) for _ in range(12)]:
                lines.append(f"{op} {sched} 1 E " + " ".join(f"{(v >> (32 * i)) & 0xffffffff:x}" for i in range(8)) +
                             f" {C256 + 1:x} 0")
                checks.append((op, fn(v) % R))
    out = subprocess.run([plain, "ops"], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-1500:]
    res = out.stdout.strip().split("\n")
    assert len(res) == len(checks)
    for line, got, (op, want) in zip(lines, res, checks):
        t = got.split()
        if t[0] == "E":
            v, mag = sum(int(a, 16) << (32 * i) for i, a in enumerate(t[1:9])), int(t[9], 16)
            assert v < 1 << 256 and (v == want if op in ("pack", "to_ext") else v % R == want), line
        else:
            x = [int(a, 16) for a in t[1:10]]
            lo, hi, mag = (int(a, 16) for a in t[10:13])
            v = sum(a << (29 * i) for i, a in enumerate(x))
            assert max(x[:8]) <= lo and x[8] <= hi, f"{line}\n-> {got}: a limb above the bound table's"
            assert v % R == want, line
            if op == "canonical":
                assert v < R, line
        assert v * U <= mag * R, f"{line}\n-> {got}: {v / R:.4f} p, above the bound table's {mag / U:.4f} p"


def test_single_call_records_pass_the_assertions_and_do_not_depend_on_the_schedule(plain, sanitized, tmp_path):
    """the records tests/test_gpu_elemcheck.py gives the device (single butterflies, element steps, combine bodies)
    through the host twin: no assertion fires, nothing wraps, and both multiplication schedules and both compilers give
    the same words"""
    from tests import elemcheck_vectors as ev
    recs = ev.generate()
    inp = str(tmp_path / "records.bin")
    ev.write_records(inp, recs)
    results = []
    for exe, tag in ((plain, "plain"), (sanitized, "san")):
        for sched in (0, 1):
            res = str(tmp_path / f"{tag}{sched}.bin")
            out = subprocess.run([exe, "elem", str(sched), inp, res], capture_output=True, text=True)
            assert out.returncode == 0, f"{tag} schedule {sched}: {out.stderr[-1200:]}"
            results.append(ev.read_results(res, len(recs)))
    for r in results[1:]:
        assert (r == results[0]).all()
    for op in range(len(ev.OPS)):
        assert results[0][[i for i, r in enumerate(recs) if r.op == op]].any(axis=1).mean() > 0.5, ev.OPS[op]       # (a zero in gives a zero out)


if __name__ == "__main__":          # rewrite the golden table: python -m tests.test_ntt_elem_host
    import pathlib
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        dd = pathlib.Path(d)
        exe = _build(dd, False)
        cs, blob = build_cases()
        (dd / "cases.bin").write_bytes(blob)
        env = full_envelope(exe, cs, str(dd / "cases.bin"), d)
    from tests.test_round_elem_host import round_envelope
    env["rounds"] = round_envelope()                                # the whole file anew: nothing stale survives
    from tests.test_curve_envelope_host import curve_envelope
    from tests.test_tower_envelope_host import tower_envelope
    env.update(curve_envelope())                                    # "curve", "quad", "lagrange"
    env["tower"] = tower_envelope()
    with open(GOLDEN, "w") as f:
        json.dump(env, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN, file=sys.stderr)
