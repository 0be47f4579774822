"""The device conformance check on the CPU (`-m "not gpu"`): tests/devcheck_vectors.py generates the vectors, the HOST
driver (tests/hip/devcheck_host.cpp: the op table of tests/hip/devcheck_ops.hpp with field29.hpp's bound assertions on)
runs every group for both multiplication schedules, and the Python checker compares every record with Python integers and
the oracle.  This validates vectors, expectations and checker without a GPU; tests/test_gpu_devcheck.py then runs the
same vectors through the gfx950 driver.

Also here: the checker is shown to see defects (a corrupted result file; host builds with a deliberately wrong variant
swapped into the op table, -DDEVCHECK_MUTANT=n), and the un-reduced representatives are shown to be determined by the
source: g++ -O1 against clang++ -O2 with the unsigned-overflow sanitizer and -DCAP_HOST_MUL32, and schedule 0 against
schedule 1, limb for limb - which is what lets the GPU test demand the device's limbs to equal the host's."""
import os
import subprocess

import pytest

from tests import devcheck_vectors as dv
from tests.devcheck_vectors import CLANG, run_driver

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = "/opt/rocm/bin/hipcc"


def build_host(out, flags=(), cxx=None):
    if not (cxx or dv.host_cxx()):
        pytest.skip("no host C++ compiler")
    return dv.build_host(out, flags, cxx)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("devcheck")
    recs, g2 = dv.generate()
    vec = str(d / "vectors.bin")
    dv.write_vectors(vec, recs, g2)
    exe = build_host(str(d / "devcheck_host"), ["-O1"])
    return {"dir": d, "recs": recs, "vec": vec, "res": run_driver(exe, vec, str(d / "host.bin"))}


def test_op_codes_of_the_header_are_distinct_and_dense():
    for g, ops in dv.OPS.items():
        assert sorted(ops.values()) == list(range(len(ops))), g
    assert set(dv.FIELD_RULES) == set(dv.OPS["field"])


@pytest.mark.parametrize("group", dv.GROUPS)
def test_host_driver_matches_python_and_meets_the_floors(work, group):
    fails, counts = dv.check_group(group, work["recs"][group], work["res"][group])
    assert not fails, f"{group}:\n" + dv.format_fails(fails)
    floors = dv.check_floors(group, work["recs"][group], counts)
    assert not floors, "\n".join(floors)


def test_quad_waves_are_mixed_by_construction(work):
    """what the GPU run relies on: waves of 16 quads with exactly one odd quad, with all quads different, and a partial
    last wave"""
    recs = work["recs"]["quad"]
    waves = [recs[i:i + 16] for i in range(0, len(recs), 16)]
    assert len(waves[-1]) == 7
    odd = {}
    for w in waves[:-1]:
        kinds = [r.kind for r in w]
        special = [k for k in kinds if k != "random"]
        if len(special) == 1:
            odd[special[0]] = True
    assert set(odd) >= {"edge:" + c for c in dv.QUAD_CASES[1:]}
    assert any(len({(r.kind, r.op) for r in w}) == 16 for w in waves[:-1])
    assert any(len({r.sched for r in w}) == 2 for w in waves[:-1])


def test_both_schedules_give_the_same_limbs(work):
    """field29.hpp: "same arithmetic, same results, same bounds" - the Montgomery quotient digits are determined by the
    operands, so the un-reduced representative is too, whatever the schedule"""
    n, per_group = 0, {}
    for g in ("field", "curve", "quad", "tower", "pair"):      # (field.hpp's 32-bit-limb group has no schedules)
        seen = {}
        for r, out in zip(work["recs"][g], work["res"][g]):
            k = (r.op, r.field, r.aux, tuple(r.words))
            if k in seen and seen[k][0] != r.sched:
                assert seen[k][1] == out, f"{r.describe()}: schedule 0 and 1 differ in their limbs"
                n += 1
                per_group[g] = per_group.get(g, 0) + 1
            seen.setdefault(k, (r.sched, out))
    assert n > 20000 and per_group["quad"] >= 6 * 16, per_group   # the six constructed waves


def test_representatives_do_not_depend_on_compiler_flags_or_limb_width(work):
    """clang++ -O2 with the unsigned-integer-overflow and undefined-behaviour sanitizers (every 64-bit column sum and
    32-bit limb sum traps on wrap-around, as in tests/test_field29_host.py; the records include the edge:top operands, the
    two chains, miller2 and check2) and field.hpp's 32-bit-limb forms (-DCAP_HOST_MUL32, what the device
    runs) against g++ -O1 with the 64-bit-limb forms: the result files are equal limb for limb"""
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ for the sanitizer build")
    d = work["dir"]
    ign = d / "ignore.txt"
    ign.write_text("src:*/field.hpp\nsrc:*/curve.hpp\nsrc:*/pairing.hpp\n")
    exe = build_host(str(d / "devcheck_host_san"), ["-O2", "-DCAP_HOST_MUL32", "-fsanitize=unsigned-integer-overflow,undefined",
                                                     f"-fsanitize-ignorelist={ign}", "-fno-sanitize-recover=all"], CLANG)
    other = run_driver(exe, work["vec"], str(d / "san.bin"))
    diff = dv.compare_files(work["res"], other)
    assert not diff, f"{len(diff)} records differ, first {diff[:5]}"


def test_chain_records_equal_the_envelope_programs_words(work):
    """the two chains of the curve group (an item of msm_accumulate, a fold of the reductions) word for word against
    tests/cpp/curve_envelope_check.cpp, which runs the same operands through the real law for
    tests/test_curve_envelope_host.py - the device is then held to these words by tests/test_gpu_devcheck.py"""
    from tests.test_curve_envelope_host import _build
    exe = _build(work["dir"], False)
    hexw = lambda w: " ".join(f"{x:x}" for x in w)                   # noqa: E731
    n = 0
    for sched in (0, 1):
        lines, want = [], []
        for r, out in zip(work["recs"]["curve"], work["res"]["curve"]):
            if r.sched != sched or r.op not in dv.CHAIN_OPS:
                continue
            if r.op == "item_chain":
                t = [r.words[18 * i:18 * i + 18] for i in range(4)]
                lines.append("item " + " ".join(f"{hexw(t[i & 3])} {(r.aux >> i) & 1}" for i in range(8)))
                want.append([f"{out[36]} " + hexw(out[:36])])
            else:
                A, B = r.words[:36], r.words[36:72]
                lines.append(f"fold {hexw(A)} {hexw(B)} {hexw(A)}")
                want.append([None, " ".join("".join(f"{x:08x}" for x in reversed(out[9 * c:9 * c + 8])) for c in range(3))])
        res = subprocess.run([exe, "run", str(sched)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-800:]
        got = res.stdout.strip().split("\n")
        pos = 0
        for line, w in zip(lines, want):
            for expect in w:
                if expect is not None:
                    assert got[pos].strip() == expect, line[:40]
                    n += 1
                pos += 1
        assert pos == len(got)
    assert n == 2 * sum(dv.CHAIN_OPS.values())


def test_results_stay_within_the_envelopes_figures(work):
    """tests/golden/lazy_envelope.json bounds every result for ALL inputs of a class; the concrete results of the curve
    and tower groups - random operands, the + p representatives, the edge:top records at the top of the classes - must
    have a true magnitude no larger than the table's figure for their operation (common path: two ordinary, different
    points; the special cases return copies and literal zeros)"""
    import json
    with open(os.path.join(HERE, "golden", "lazy_envelope.json")) as f:
        env = json.load(f)
    U, P = env["unit_per_p"], dv.P
    ops = env["curve"]["ops"]
    names = {"add": ["add(A, A)", "add(M any image, M any image)"],
             "add_acc": ["add_acc(A, A)", "add_acc(M any image, M any image)"],
             "dbl": ["dbl(A)", "dbl(M any image)"], "dbl_affine": ["dbl_affine(x, y < 2p)"],
             "madd_acc": ["madd_acc(A, T)", "madd_acc(A, -T)"], "add_mixed": ["add_mixed(A, T)", "add_mixed(A, -T)"],
             "item_chain": None}
    n = 0
    for r, out in zip(work["recs"]["curve"], work["res"]["curve"]):
        if r.op not in names or not (r.kind in ("random", "edge:top")):
            continue
        if r.op == "item_chain":
            bound = [env["curve"]["chains"]["msm_accumulate: acc"][c][1] for c in ("x", "y", "zz", "zzz")]
        else:
            bound = [max(ops[k][c][1] for k in names[r.op]) for c in ("x", "y", "zz", "zzz")]
        for c in range(4):
            v = dv.val(out[9 * c:9 * c + 9])
            assert v * U <= bound[c] * P, f"{r.describe()}: coordinate {c} is {v / P:.4f} p, the table says {bound[c] / U:.4f} p"
        n += 1
    assert n > 1000
    tw, n = env["tower"]["ops"], 0
    for r, out in zip(work["recs"]["tower"], work["res"]["tower"]):
        key = f"f12_frob {r.aux}" if r.op == "f12_frob" else r.op
        for c in range(12):
            v = dv.val(out[9 * c:9 * c + 9])
            assert v * U <= tw[key][1] * P, f"{r.describe()}: coefficient {c} is {v / P:.4f} p, the table says {tw[key][1] / U:.4f} p"
        n += 1
    assert n > 2000


# ---- the checker sees defects ---------------------------------------------------------------------------------------
def test_checker_names_a_flipped_bit_and_swapped_outputs(work):
    import copy
    for group, idx in (("field", 1234), ("curve", 77), ("quad", 40), ("tower", 300), ("pair", 9), ("field32", 500)):
        res = copy.deepcopy(work["res"][group])
        res[idx][3] ^= 1 << 7                                     # one bit of one limb
        fails, _ = dv.check_group(group, work["recs"][group], res)
        assert [f[0] for f in fails] == [idx], (group, [f[0] for f in fails][:5])
    res = copy.deepcopy(work["res"]["field"])
    i = next(k for k, r in enumerate(work["recs"]["field"]) if r.op == "mul" and r.kind == "random")
    j = next(k for k, r in enumerate(work["recs"]["field"]) if k > i + 1 and r.op == "mul" and r.kind == "random")
    res[i], res[j] = res[j], res[i]
    fails, _ = dv.check_group("field", work["recs"]["field"], res)
    assert [f[0] for f in fails] == [i, j]
    res = copy.deepcopy(work["res"]["tower"])
    res[5] = [dv.POISON] * len(res[5])                            # a record the driver never wrote
    fails, counts = dv.check_group("tower", work["recs"]["tower"], res)
    assert [f[0] for f in fails] == [5] and "0xFF" in fails[0][2]
    assert dv.check_floors("tower", work["recs"]["tower"], counts)     # ... and it is missing from the counts
    fails, _ = dv.check_group("pair", work["recs"]["pair"], work["res"]["pair"][:-1])
    assert fails and "result records" in fails[0][2]


# mutant -> the (group, op) it must be flagged in, and in no record outside it
MUTANTS = {1: ("tower", {"f2_mul"}), 2: ("curve", {"add_mixed"}), 3: ("curve", {"term_mul"}), 4: ("pair", {"miller2", "check2", "pairing2"}),
           5: ("tower", {"f12_frob"})}


@pytest.mark.parametrize("n", sorted(MUTANTS))
def test_mutant_of_the_op_table_is_flagged_in_its_own_group_only(work, n):
    """1 a product without its final weak reduction, 2 a mixed addition that skips the equal-operand path, 3 term_mul
    dropping the top digit when `top` is even, 4 a Miller loop without its last Frobenius line, 5 a Frobenius map with
    the wrong constant row.  Host builds only (devcheck_ops.hpp refuses them under hipcc)."""
    d = work["dir"]
    exe = build_host(str(d / f"mutant{n}"), ["-O1", f"-DDEVCHECK_MUTANT={n}"])
    res = run_driver(exe, work["vec"], str(d / f"mutant{n}.bin"))
    group, ops = MUTANTS[n]
    for g in dv.GROUPS:
        fails, _ = dv.check_group(g, work["recs"][g], res[g])
        if g != group:
            assert not fails, f"mutant {n} flagged in {g}:\n" + dv.format_fails(fails)
        else:
            assert fails, f"mutant {n} was not noticed"
            assert {f[1].op for f in fails} <= ops, {f[1].op for f in fails}
            assert {f[1].sched for f in fails} == {0, 1}


def test_hip_driver_cross_compiles_for_gfx950():
    """compile only, and only when the built binary is missing (build() makes it: cap_amd/csrc/Makefile)"""
    exe = os.path.join(HERE, "hip", "devcheck")
    if os.path.exists(exe):
        return
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    subprocess.check_call(["make", "-C", os.path.join(dv.ROOT, "cap_amd", "csrc"), "../../tests/hip/devcheck"])
    assert os.path.exists(exe)
