"""The NTT's addressing forms (NttIo: zero extension past src_len, both grouping levels, decimated input, a caller's
pre-scale table with pre_inner, lazy_out) and the 3 * 2^k transforms (ntt3_forward, ntt3_inverse, ntt3_combine) on the
MI355X.  None of them can be reached from the C ABI, so tests/hip/nttcheck - a program that links libcapgpu.so and calls
cap::ntt_run / cap::ntt3_forward / cap::ntt3_inverse in the code the product ships - runs the cases of
tests/ntt_io_model.py; the expected values come from the oracle after the Python model of the addressing
(tests/test_ntt_expectations.py checks that model without a GPU).  Checked per case: every element of every destination
array, the representation the headers promise (lazy_out results below 2 r, all others canonical), and that every byte
outside the destination arrays still holds its sentinel.

The binary (built by build()) runs ONCE, as one fresh child process under its own time limit; the tests only parse its
result file.  The limit is five times the wall time measured on the MI355X, not below 60 s; MEASURED_S is that time (0.73 s for the 141 cases;
the module takes 7 s with the Python side's expectations)."""
import os
import subprocess
import time

import pytest

from oracle import bn254 as bn
from oracle import capref as cr
from tests import ntt_io_model as io
from tests.test_quotient_domain import root_6n

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "hip", "nttcheck")
MEASURED_S = 0.73                                  # 141 cases
TIME_LIMIT_S = max(60.0, 5 * MEASURED_S)
GROUPS = {"nttio": io.ntt_io_cases, "prover": io.prover_cases, "ntt3": io.ntt3_cases}


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    assert os.path.exists(EXE), "tests/hip/nttcheck is missing: build() makes it (make -C cap_amd/csrc)"
    d = tmp_path_factory.mktemp("nttcheck")
    groups = {g: make() for g, make in GROUPS.items()}
    cases = [c for g in GROUPS for c in groups[g]]
    inp, res = str(d / "cases.bin"), str(d / "results.bin")
    io.write_cases(inp, cases)
    t0 = time.time()
    try:
        out = subprocess.run([EXE, inp, res], capture_output=True, text=True, timeout=TIME_LIMIT_S)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"nttcheck did not finish within {TIME_LIMIT_S} s: {(e.stderr or b'')[-800:]}")
    print(f"nttcheck: {len(cases)} cases, wall time {time.time() - t0:.2f} s")
    assert out.returncode == 0, f"nttcheck ended with {out.returncode}: {out.stderr[-1200:]}"
    results = dict(zip((id(c) for c in cases), io.read_results(res, cases)))
    return {g: [(c,) + results[id(c)] for c in groups[g]] for g in GROUPS}


@pytest.mark.parametrize("group", list(GROUPS))
def test_device_results_match_the_oracle_through_the_addressing_model(run, group):
    bad = [line for c, rc, dst in run[group] for line in io.check_case(c, rc, dst)]
    assert not bad, f"{len(bad)} complaints, first:\n" + "\n".join(bad[:12])


def test_small_forward_results_point_by_point(run):
    """M = 2, 4 and 32: every device result of ntt3_forward against the oracle's Horner evaluation of the case's
    polynomial at the point its index stands for, s_a omega_M^k with s_a = 5 omega_N^a - no transform and none of the
    model's block arithmetic on the expected side"""
    inv32 = pow(32, io.R - 2, io.R)
    seen = set()
    for c, rc, dst in run["ntt3"]:
        if c.kind != io.NTT3_FORWARD or c.log_n > 5:
            continue
        assert rc == 0, c.name
        M = 1 << c.log_n
        w_n, m = root_6n(c.log_n - 1)
        w_m = bn.root_of_unity(c.log_n)
        assert m == M and pow(w_n, 3, io.R) == w_m and pow(w_n, M, io.R) != 1 and pow(w_n, 3 * M // 2, io.R) != 1
        for q in range(c.count):
            poly = c.src[q * c.src_outer:q * c.src_outer + c.src_len]
            base = c.dst_offset + q * c.dst_outer
            got = io.to_ints(dst[base:base + 3 * M])
            for a in range(3):
                s_a = bn.FR_GENERATOR * pow(w_n, a, io.R) % io.R
                want = [32 * cr.poly_eval_fr(poly, bn.to_mont(s_a * pow(w_m, k, io.R) % io.R, io.R)) % io.R
                        for k in range(M)]
                assert all(v < 2 * io.R for v in got[a * M:(a + 1) * M]), (c.name, q, a)
                assert [v % io.R for v in got[a * M:(a + 1) * M]] == want, (c.name, q, a)
        seen.add((c.log_n, c.count, c.src_len))
    assert seen == {(m, k, sl) for m in (1, 2, 5) for k in (1, 4, 18) for sl in {1, min(1 << m, (1 << m) // 2 + 2), 1 << m}}


def forms_of(c):
    """the addressing forms of the issue's list that an ntt_run case exercises"""
    n = 1 << c.log_n
    out = {f"src_len {'0 1 n/2+2 n-1 n'.split()[(0, 1, n // 2 + 2, n - 1, n).index(c.src_len)]}"
           } if c.src_len in (0, 1, n // 2 + 2, n - 1, n) else set()
    out |= {f"src_group {c.src_group}", f"dst_group {c.dst_group}", f"lazy_out {c.lazy_out}"}
    if c.src_group > 1 and c.src_elem_stride == 1:
        assert c.src_inner and c.src_outer != c.src_inner, c.name                    # distinct outer and inner strides
    if c.dst_group > 1:
        assert c.dst_inner and c.dst_outer != c.dst_inner, c.name
    if c.src_group2 == 2 and c.dst_group2 == 2 and c.src_inner2 and c.dst_inner2:
        out.add("second grouping level")
    if c.src_elem_stride == 3 and c.src_inner:
        out.add("decimated with a group offset" + (", with a table" if len(c.pre) and c.pre_inner else ""))
    elif len(c.pre) and c.pre_inner:
        out.add(f"pre-scale table with pre_inner, dir {c.dir}")
    return out


FORMS = ({f"src_len {s}" for s in "0 1 n/2+2 n-1 n".split()} | {f"{side}_group {g}" for side in ("src", "dst") for g in (1, 3, 5)}
         | {"lazy_out 0", "lazy_out 1", "second grouping level", "decimated with a group offset",
            "decimated with a group offset, with a table", "pre-scale table with pre_inner, dir 0",
            "pre-scale table with pre_inner, dir 1"})


def test_every_form_runs_at_every_size_and_tile(run, cg):
    """each form of the list at 2^6, 2^10 and 2^12, and at 2^12 with the 256-element AND with the 1024-element tile (the
    only size here whose tiles are 16 columns wide, log_c = 4, as in the 256-proof batch)"""
    by = {}
    for c, _, _ in run["nttio"]:
        plan = cg.ntt_plan(c.log_n, c.count)
        by.setdefault((c.log_n, plan["tile_log"]), set()).update(forms_of(c))
        if plan["tile_log"] == 10:
            assert plan["log_c"] == [4, 4], plan
    assert set(by) == {(6, 8), (10, 8), (12, 8), (12, 10)}
    for key, forms in by.items():
        assert FORMS <= forms, (key, sorted(FORMS - forms))


def test_every_ntt3_form_runs_at_every_size_and_count(run):
    got = {}
    for c, _, _ in run["ntt3"]:
        what = {io.NTT3_FORWARD: ("forward", c.src_len), io.NTT3_INVERSE: ("inverse", getattr(c, "degree", None)),
                io.NTT3_ROUND_TRIP: ("round trip", None)}[c.kind]
        got.setdefault((c.log_n, c.count), set()).add(what)
    assert set(got) == {(m, k) for m in (1, 2, 5, 6, 11, 12) for k in (1, 4, 18)}
    for (log_m, count), forms in got.items():
        M = 1 << log_m
        # M / 2 + 2 coefficients and degree 5 n + 7 (n = M / 2) where M and 3 M points hold them: from M = 8 on
        want = {("forward", 1), ("forward", min(M, M // 2 + 2)), ("forward", M), ("inverse", 3 * M - 1),
                ("inverse", min(5 * (M // 2) + 7, 3 * M - 1)), ("round trip", None)}
        assert forms == want, (log_m, count)
