"""What the GPU NTT tests expect, checked on a machine without a GPU (`-m "not gpu"`): the closed forms of
tools/ntt_conformance.py against the C restatement and, at small sizes, against Python integers (oracle/bn254.py); the
Python model of the NttIo addressing (tests/ntt_io_model.py) against a direct evaluation at log_n = 3; the block order of
the 3 * 2^k transforms against a direct evaluation at log_m = 3.  A wrong expectation is caught here, not on the device."""
import numpy as np
import pytest

from oracle import bn254 as bn
from oracle import capref as cr
from tests import ntt_io_model as io
from tools import ntt_conformance as nc

R = bn.R


@pytest.mark.parametrize("log_n", [1, 2, 3, 4, 7, 10])
def test_closed_forms_equal_the_oracle_and_python_integers(log_n):
    seen = 0
    for inverse, coset in nc.MODES:
        py = {(False, False): bn.ntt, (False, True): bn.coset_ntt, (True, False): bn.intt, (True, True): bn.coset_intt}
        for k, name in enumerate(nc.INPUTS):
            cf = nc.closed_form(log_n, name, inverse, coset, seed=3)
            if cf is None:
                continue
            seen += 1
            raw, ref = nc.make_input(log_n, k, 3)
            assert cf == cr.array_to_ints(cr.ntt_fr(ref, log_n, inverse, coset)), (name, inverse, coset)
            if log_n <= 4:
                assert cf == py[(inverse, coset)](cr.array_to_ints(raw), log_n), (name, inverse, coset)
    assert seen == 4 * 6 + 3 * 2                 # six impulses in every mode; the two constants wherever they are sparse


def test_inputs_are_what_their_names_say():
    log_n, n = 6, 64
    ints = {name: cr.array_to_ints(nc.make_input(log_n, k, 5)[0]) for k, name in enumerate(nc.INPUTS)}
    assert all(v < R for name, vals in ints.items() if name != "x_plus_r" for v in vals)
    assert set(ints["all_rm1"]) == {R - 1} and ints["alt_rm1_one"][:4] == [R - 1, 1, R - 1, 1]
    assert 40 <= ints["zeros90"].count(0) < n and 40 <= ints["rm1_90"].count(R - 1) < n
    for name, k in nc.impulse_positions(log_n, 5).items():
        assert [i for i, v in enumerate(ints[name]) if v] == [k]
    assert {0, 1, n // 2 - 1, n // 2, n - 1} <= set(nc.impulse_positions(log_n, 5).values())
    assert all(ints["padded_half_plus_2"][:n // 2 + 2]) and not any(ints["padded_half_plus_2"][n // 2 + 2:])
    assert all(ints["odd_only"][1::2]) and not any(ints["odd_only"][0::2])
    assert all(ints["three_mod_four_only"][3::4]) and not any(v for i, v in enumerate(ints["three_mod_four_only"]) if i % 4 != 3)
    raw, ref = nc.make_input(log_n, nc.INPUTS.index("x_plus_r"), 5)
    assert [a - b for a, b in zip(cr.array_to_ints(raw), cr.array_to_ints(ref))] == [R] * n
    assert len(nc.INPUTS) % 2 == 1


def test_nttio_model_reproduces_a_direct_evaluation():
    """decimated, grouped, zero-extended and pre-scaled input at log_n = 3: array (q2, a) is the transform of the
    elements 3 g + a of polynomial q2 that lie below src_len, each times its table entry"""
    log_n, n, count = 3, 8, 6
    rng = bn.SplitMix64(9)
    table = [rng.field(R) for _ in range(3 * n + 14)]
    c = io.ntt_run_case("direct", 77, io.internal_table(table), log_n=log_n, count=count, src_elem_stride=3, src_group=3,
                        src_inner=1, src_outer=3 * n + 2, src_len=3 * n - 4, dst_outer=n + 1, pre_inner=7)
    src = io.to_ints(c.src)
    w = bn.root_of_unity(log_n)
    assert len(c.regions) == count
    for q, (start, exp, lazy) in enumerate(c.regions):
        q2, a = divmod(q, 3)
        poly = src[q2 * (3 * n + 2):][:3 * n - 4]                        # the polynomial, cut at src_len
        # the table holds t 2^261 and the kernel's product removes 2^261: the factor is t itself
        phase = [v * table[3 * g + a + 7 * a] % R for g, v in enumerate(poly[a::3])]
        assert len(phase) <= n
        assert io.to_ints(exp) == [bn.poly_eval(phase, pow(w, j, R)) for j in range(n)], q
        assert start == q * (n + 1) and not lazy
    # grouping on both sides and the coset table of the domain, against Python's coset transform
    c = io.ntt_run_case("groups", 78, log_n=log_n, count=7, coset=1, src_len=n - 1, src_group=3, src_inner=n + 1,
                        src_group2=2, src_inner2=3 * (n + 1) + 1, src_outer=6 * (n + 1) + 5, dst_group=3, dst_inner=n + 2,
                        dst_group2=2, dst_inner2=3 * (n + 2) + 2, dst_outer=6 * (n + 2) + 7)
    src = io.to_ints(c.src)
    for q, (start, exp, _) in enumerate(c.regions):
        base = (q // 6) * (6 * (n + 1) + 5) + (q // 3 % 2) * (3 * (n + 1) + 1) + (q % 3) * (n + 1)
        assert io.to_ints(exp) == bn.coset_ntt(src[base:base + n - 1] + [0], log_n), q
        assert start == (q // 6) * (6 * (n + 2) + 7) + (q // 3 % 2) * (3 * (n + 2) + 2) + (q % 3) * (n + 2)


def test_ntt3_block_order_matches_a_direct_evaluation():
    """index a M + k <-> the point s_a omega_M^k, s_a = 5 omega_N^a, for a polynomial of 3 M coefficients"""
    log_m, M = 3, 8
    sa, wm = io.shifts(log_m)
    coeffs = io.random_raw(21, 3 * M)
    ci = io.to_ints(coeffs)
    blocks = io.eval_blocks(coeffs, log_m)
    for a in range(3):
        assert blocks[a] == [bn.poly_eval(ci, sa[a] * pow(wm, k, R) % R) for k in range(M)], a
    # the three cosets together are the coset 5 <omega_N>, and block 0 is the oracle's own coset transform
    wn = sa[1] * pow(5, R - 2, R) % R
    assert {s * pow(wm, k, R) % R for s in sa for k in range(M)} == {5 * pow(wn, i, R) % R for i in range(3 * M)}
    short = coeffs[:M // 2 + 2]
    padded = np.zeros((M, 4), dtype=np.uint64)
    padded[:len(short)] = short
    assert io.eval_blocks(short, log_m)[0] == io.to_ints(cr.ntt_fr(padded, log_m, False, True))
    # forward expectation: internal form = 32 x the arkworks image, block a of polynomial q at q * dst_outer + a M;
    # the oracle's Horner evaluation agrees point by point (Montgomery in, Montgomery out)
    c = io.expect_ntt3_forward(io.Case("fwd", io.random_raw(22, 2 * (M + 1)), kind=io.NTT3_FORWARD, log_n=log_m, count=2,
                                       dst_elems=2 * (3 * M + 2) + 3, dst_offset=1, src_outer=M + 1, src_len=M // 2 + 2,
                                       dst_outer=3 * M + 2))
    assert [r[0] for r in c.regions] == [1 + q * (3 * M + 2) + a * M for q in range(2) for a in range(3)]
    inv32 = pow(32, R - 2, R)
    for i, (start, exp, lazy) in enumerate(c.regions):
        q, a = divmod(i, 3)
        poly = c.src[q * (M + 1):q * (M + 1) + M // 2 + 2]
        want = [cr.poly_eval_fr(poly, bn.to_mont(sa[a] * pow(wm, k, R) % R, R)) for k in range(M)]
        assert [v * inv32 % R for v in io.to_ints(exp)] == want and lazy


def test_case_lists_stay_inside_their_buffers_and_cover_the_forms():
    cases = io.ntt_io_cases(sizes=((6, 3),)) + io.prover_cases() + io.ntt3_cases(log_ms=(1, 2, 5), counts=(1, 4))
    assert any(c.src_group2 == 2 and c.dst_group2 == 2 for c in cases)
    assert any(c.src_elem_stride == 3 and c.pre_inner for c in cases) and any(c.pre_inner == 64 for c in cases)
    assert {c.lazy_out for c in cases if c.kind == io.NTT_RUN} == {0, 1}
    assert {c.kind for c in cases} == {0, 1, 2, 3}
    for c in cases:
        covered = np.zeros(c.dst_elems, dtype=bool)
        for start, exp, _ in c.regions:
            assert start >= 0 and start + len(exp) <= c.dst_elems and not covered[start:start + len(exp)].any(), c.name
            covered[start:start + len(exp)] = True
        # a perfect device result passes check_case; one wrong element, or a written gap, does not
        dst = np.full((c.dst_elems, 4), io.SENTINEL, dtype=np.uint64)
        for start, exp, _ in c.regions:
            dst[start:start + len(exp)] = exp
        assert io.check_case(c, 0, dst) == [], c.name
        start, exp, _ = c.regions[-1]
        dst[start + len(exp) - 1, 0] ^= np.uint64(1)
        assert io.check_case(c, 0, dst), c.name
        if not covered.all():
            dst[start + len(exp) - 1, 0] ^= np.uint64(1)
            dst[np.nonzero(~covered)[0][0], 3] = 0
            assert io.check_case(c, 0, dst), c.name
