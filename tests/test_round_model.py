"""tests/round_model.py without a GPU: the models behind tests/test_gpu_rounds.py against the oracle, the case list
against its buffers, the edge generator against each contract, and the checker against a perfect and a spoilt result."""
import functools
import random
import struct

import numpy as np
import pytest

from oracle import bn254 as bn
from oracle import plonk as pl
from tests import ntt_io_model as io
from tests import round_model as rm
from tests import test_quot5_identity as q5
from tests import test_quotient_fold_identity as qf
from tests.test_quotient_domain import root_6n

R = bn.R
prod = lambda xs: functools.reduce(lambda a, b: a * b % R, xs, 1)


@pytest.fixture(scope="module")
def cases():
    """every group but the scans, whose lists are long (they are built once more, alone, below)"""
    return {g: make() for g, make in rm.GROUPS.items() if g != "scans"}


def test_forms_and_saturated_images():
    assert rm.ark(1) == (1 << 256) % R and rm.internal(1) == 32 * rm.ark(1) % R
    assert io.to_ints(io.internal_table([7]))[0] == rm.internal(7)
    for v in (0, 1, R - 1, 12345):
        assert rm.ark_value(rm.ark(v)) == v and rm.internal_value(rm.internal(v)) == v
        assert rm.internal_value(rm.internal(v) + R) == v            # any representative
    for bound in (rm.CANON, rm.WEAK):
        s = rm.saturated(bound)
        assert s < bound and rm.limbs29(s)[:8] == [rm.LIMB] * 8
        assert s + (1 << 232) >= bound                               # the largest such image


def test_edge_generator_respects_each_contract():
    rng = random.Random(1)
    for bound in (rm.CANON, rm.WEAK):
        for form in ("ark", "internal"):
            fixed = rm.edge_images(bound, form)
            assert {0, 1, R - 1, rm.saturated(bound)} <= set(fixed) and all(v < bound for v in fixed)
            assert (bound == rm.WEAK) == ({R, R + 1, 2 * R - 1} <= set(fixed))
            drawn = [rm.draw_edge(rng, bound, form) for _ in range(2000)] + rm.fill(rng, 2000, bound, form)
            assert all(0 <= v < bound for v in drawn)
            part = [rm.partly_saturated(rng, bound) for _ in range(500)]
            assert all(v < bound and set(rm.limbs29(v)[:8]) <= {0, rm.LIMB} for v in part)
            assert len({tuple(rm.limbs29(v)[:8]) for v in part}) > 100
    f = rm.fill(rng, 64, rm.WEAK, "internal")
    assert all(f[i] == rm.saturated(rm.WEAK) for i in range(0, 64, 4))
    assert any(v >= R for v in f) and len(set(f[3::4])) == 16


def test_contracts_of_the_quotient_and_perm_cases(cases):
    """canonical inputs below r, weak inputs below 2 r, the k_j x columns canonical, beta = 0 present with beta_inv = 0"""
    for c in cases["quotient"]:
        m, P, per_key = c.params[0], c.params[1], c.params[5]
        pkc, cos, xs, inv_nx1, chal, qc = (io.to_ints(x) for x in c.inputs)
        assert all(v < 2 * R for v in pkc + cos) and any(v >= R for v in pkc) and any(v >= R for v in cos)
        assert all(v < R for v in xs + inv_nx1 + chal + qc)
        for q in range(P if per_key else 1):
            assert all(v < R for v in pkc[(q * 22 + 18) * m:(q + 1) * 22 * m])
        assert chal[6] == 0 and chal[6 + 4] == 0 and chal[4] != 0 and chal[12 + 4] != 0
        sat = rm.saturated(rm.WEAK)
        assert all(pkc[s * m] == sat for s in range(18)) and all(cos[j * m] == sat for j in range(6))
        assert xs[0] == inv_nx1[0] == chal[1] == chal[2] == rm.saturated(rm.CANON)
    for c in cases["grand product"]:
        n, P = c.params[0], c.params[1]
        wires, sig, tw, chal = (io.to_ints(x) for x in c.inputs[:4])
        assert all(v < R for v in wires + sig + tw + chal)
        assert chal[0] == 0 and chal[6 + 1] == 0 and set(wires[5 * n:10 * n]) == {0, R - 1}


def test_every_case_stays_inside_its_buffers(cases):
    for g, cs in cases.items():
        for c in cs:
            assert rm.stays_inside(c), c.name
            assert max([len(x) for x in c.inputs] + [c.dst_elems]) * 32 < 20e6, c.name


def test_scan_cases_cover_the_list_and_stay_inside():
    cs = rm.scan_cases()
    assert all(rm.stays_inside(c) for c in cs)
    seen = {(c.params[0], c.params[1], c.params[2]) for c in cs}
    assert seen == {(op, rev, n) for op in (0, 1) for rev in (0, 1) for n in rm.SCAN_LENS}
    for what, values in (("batch", lambda c: c.params[4]), ("gap", lambda c: c.params[3] - c.params[2]),
                         ("data", lambda c: c.name.split()[-1])):
        for key in ("op=0 rev=0", "op=0 rev=1", "op=1 rev=0", "op=1 rev=1"):
            got = {values(c) for c in cs if key in c.name}
            want = {"batch": {1, 3}, "gap": {0, 8}, "data": {"random", "ones", "r-1"}}[what]
            assert want <= got, (what, key, got)
    assert {"zero@0", "zero@mid", "zero@last"} <= {c.name.split()[-1] for c in cs if "op=0" in c.name}
    # the prover's own shapes at 2^16: the product scan of exactly 64 blocks and the suffix sum of 65, batched
    assert any(c.params == [0, 0, 65536, c.params[3], 3] for c in cs) and any(c.params == [1, 1, 65539, c.params[3], 3] for c in cs)
    # the model: a plain prefix product / suffix sum on values
    rng = random.Random(3)
    v = [rng.randrange(R) for _ in range(9)]
    assert [rm.ark_value(x) for x in rm.scan_model([rm.ark(x) for x in v], 0, 0)] == [prod(v[:j]) for j in range(9)]
    assert [rm.ark_value(x) for x in rm.scan_model([rm.ark(x) for x in v], 1, 1)] == [sum(v[j + 1:]) % R for j in range(9)]


def test_grand_product_model_gives_the_oracles_permutation_polynomial():
    n, pk, tr = q5.instance(4)
    omega = bn.root_of_unity(4)
    tw = [pow(omega, j, R) for j in range(n)]
    ev = lambda poly: [bn.poly_eval(list(poly), x) for x in tw]
    wires = [ev(p) for p in tr["wire_polys"]]                     # (the blinders vanish on the domain)
    sig = [ev(p) for p in pk.sigma_polys]
    num, den, z, total = rm.grand_product(wires, sig, tw, pl.K, tr["beta"], tr["gamma"])
    assert total != 0 and z[0] == 1 and z == ev(tr["z_poly"])
    assert num != den and prod(num) == prod(den)                                 # the product closes: a valid permutation


@pytest.mark.parametrize("five", [0, 1])
def test_quotient_model_gives_quotient_values_without_pi(five):
    """the oracle's proof at n = 16 laid out as k_quotient reads it - m = 6 n points in three blocks of M = 2 n, index
    a M + k <-> 5 omega_N^a omega_M^k - through quotient_model with the true tables, both forms"""
    log_n = 4
    n, pk, tr = q5.instance(log_n)
    m, M = 6 * n, 2 * n
    wN, _ = root_6n(log_n)
    pts = [bn.FR_GENERATOR * pow(wN, a + 3 * k, R) % R for a in range(3) for k in range(M)]
    ev = lambda poly: [bn.poly_eval(list(poly), x) for x in pts]
    pkc = [ev(p) for p in pk.selector_polys] + [ev(p) for p in pk.sigma_polys] + [[pl.K[j] * x % R for x in pts] for j in range(1, 5)]
    cos = [ev(p) for p in tr["wire_polys"]] + [ev(tr["z_poly"])]
    if five:                                                      # blocks 0, 1 and the even elements of block 2, compact
        cos = [col[:2 * M] + col[2 * M::2] + [0] * (M // 2) for col in cos]
    _, _, c, _ = q5.constants(log_n)
    zh_inv = [rm.inv(c[k] - 1) for k in range(6)]
    inv_nx1 = [rm.inv(n * (x - 1)) for x in pts]
    b, g, a = tr["beta"], tr["gamma"], tr["alpha"]
    ch = (b, g, a, a * a % R, rm.inv(b), a * pow(b, 5, R) % R)
    want = [q5.quotient_values_without_pi(log_n, k) for k in range(6)]
    for fold in (False, True):
        got = rm.quotient_model(m, five, pkc, cos, pts, inv_nx1, zh_inv, ch, pl.K, fold)
        assert len(got) == (5 * n if five else m)
        for i, v in enumerate(got):
            it, _, zi = rm.quotient_indices(m, five, i)
            a_, k = divmod(it, M)
            coset, j = (a_ + 3 * k) % 6, (a_ + 3 * k) // 6
            assert zi == coset and v == want[coset][j], (fold, i)
    if five:
        assert {rm.quotient_indices(m, 1, i)[2] for i in range(5 * n)} == {0, 1, 2, 3, 4}


def test_quotient_point_forms_agree_with_the_fold_identity():
    rng = random.Random(5)
    for _ in range(50):
        v = qf.draw(rng, edge=False)
        beta = rng.randrange(1, R)
        sel = [rng.randrange(R) for _ in range(13)] + v["sig"]
        kx = [pl.K[j] * v["x"] % R for j in range(1, 5)]
        ch = (beta, v["gamma"], v["alpha"], v["alpha"] ** 2 % R, rm.inv(beta), v["alpha"] * pow(beta, 5, R) % R)
        args = (sel, v["w"], v["z"], v["zw"], v["x"], kx, 3, 7, ch, pl.K)
        d, f = rm.quotient_point(False, *args), rm.quotient_point(True, *args)
        assert d == f == ((pl.gate_eval(sel[:13], v["w"], 0) + qf.direct(v["alpha"], beta, v["gamma"], v["w"], v["sig"], v["x"],
                                                                        v["z"], v["zw"])) * 7 + ch[3] * (v["z"] - 1) * 3) % R


@pytest.mark.parametrize("log_n", [4, 5])
def test_top_model_gives_top_coefficients(log_n):
    assert rm.top_model(**rm.top_inputs_of_instance(log_n)) == q5.top_coefficients(log_n)


def test_division_model_gives_the_polynomial_back():
    rng = random.Random(9)
    for a in (1, R - 1, rng.randrange(R)):
        f = [rng.randrange(R) for _ in range(19)]
        q, r = rm.synthetic_division(f, a)
        back = [((q[k - 1] if k else 0) - a * (q[k] if k < len(q) else 0)) % R for k in range(len(f))]
        back[0] = (back[0] + r) % R
        assert back == f and r == rm.horner(f, a) and q == pl.divide_by_linear(f, a)


def test_models_of_the_small_kernels(cases):
    """the expected values of powers, evaluations and lincomb cases restated independently at a few positions"""
    c = cases["powers"][1]
    pw, exp = io.to_ints(c.inputs[0]), io.to_ints(c.regions[0][1])
    ps = c.params[0]
    for q in range(c.params[1]):
        base = rm.ark_value(pw[q * 24])
        assert all(rm.ark_value(exp[q * ps + e]) == pow(base, e, R) for e in (0, 1, 2, 255, 256, 257, ps - 1))
    c = cases["lincomb"][3]
    P, nterms, stride, out_len = c.params[:4]
    pool, recs, exp = io.to_ints(c.inputs[0]), c.inputs[1], io.to_ints(c.regions[1][1])
    for k in (0, 1, 17, 18, 19, out_len - 1):
        acc = 0
        for t in range(nterms, 2 * nterms):
            s = io.to_ints(recs[2 * t:2 * t + 1])[0]
            off, len_ = int(recs[2 * t + 1][0]), int(recs[2 * t + 1][1])
            if k < len_:
                acc += rm.internal_value(s) * rm.ark_value(pool[off + k])
        assert rm.ark_value(exp[k]) == acc % R
    assert {int(r[1]) for r in recs[1::2]} == {16, 18, 19} and out_len > 19


def test_the_checker_passes_a_perfect_result_and_no_other(cases):
    rng = random.Random(11)
    for g, cs in cases.items():
        for c in cs:
            if max(len(x) for x in c.inputs) > 100000:
                continue
            dst = rm.perfect_result(c)
            assert rm.check_case(c, 0, dst) == [], c.name
            assert rm.check_case(c, rm.REFUSED, dst), c.name
            start, exp, weak = c.regions[rng.randrange(len(c.regions))]
            if len(exp):
                spoilt = dst.copy()
                spoilt[start + rng.randrange(len(exp)), rng.randrange(4)] ^= np.uint64(1 << rng.randrange(32))
                assert rm.check_case(c, 0, spoilt), c.name
            covered = np.zeros(c.dst_elems, dtype=bool)
            for s, e, _ in c.regions:
                covered[s:s + len(e)] = True
            gaps = np.nonzero(~covered)[0]
            assert len(gaps), f"{c.name}: no gap to watch"
            spoilt = dst.copy()
            spoilt[gaps[rng.randrange(len(gaps))], 0] ^= np.uint64(1)
            assert rm.check_case(c, 0, spoilt), c.name
            if weak:                                              # the other representative below 2 r passes, 2 r more does not
                other = dst.copy()
                other[start:start + len(exp)] = rm.add_r(exp)
                assert rm.check_case(c, 0, other) == [], c.name


def test_case_file_round_trip(tmp_path, cases):
    cs = cases["degree check"] + cases["lincomb"][:1] + cases["copies and blinders"][:3]
    path = str(tmp_path / "cases.bin")
    rm.write_cases(path, cs)
    raw = open(path, "rb").read()
    assert len(raw) == 16 + sum(8 * (4 + rm.NPARAMS) + sum(8 + 32 * len(x) for x in c.inputs) for c in cs)
    # a result file of perfect results reads back and passes
    res = str(tmp_path / "results.bin")
    with open(res, "wb") as f:
        f.write(struct.pack("<QQ", rm.MAGIC_OUT, len(cs)))
        for c in cs:
            f.write(struct.pack("<QQ", 0, c.dst_elems))
            f.write(rm.perfect_result(c).tobytes())
    for c, (rc, dst) in zip(cs, rm.read_results(res, cs)):
        assert rm.check_case(c, rc, dst) == []
