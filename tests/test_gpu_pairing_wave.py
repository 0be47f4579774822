"""The wave form of the device pairing check (k_pairing_check2_wave: one check per group of six lanes, ten per wavefront)
behind capgpu_pairing_set_form, and capgpu_plonk_verify_dev, the one-proof verifier that always uses it: verdicts equal
the lane form's and the host's, and capgpu_pairing_stats shows which kernel decided."""
import copy
import random

import numpy as np
import pytest

from cap_amd import bench_utils as bu
from oracle import bn254 as bn
from tests.test_gpu_verify_each import g1_neg, g1_words, host_verdict, pubs_arr, scalar_ladder

pytestmark = pytest.mark.gpu

L = 6                     # lanes per check (pairing_wave.hpp: kGroup)
PER_WAVE = 64 // L        # 10


@pytest.fixture
def forms(cg):
    """run(form, fn): fn() under that pairing form -> (result, growth of the lane counter, growth of the wave counter);
    the process-wide setting is LANE again afterwards, whatever happens"""
    def run(form, fn):
        cg.pairing_set_form(form)
        before = cg.pairing_stats()
        try:
            out = fn()
        finally:
            cg.pairing_set_form(cg.PAIRING_LANE)
        after = cg.pairing_stats()
        return out, after["lane_checks"] - before["lane_checks"], after["wave_checks"] - before["wave_checks"]
    yield run
    cg.pairing_set_form(cg.PAIRING_LANE)


def test_form_api(cg):
    assert cg.pairing_get_form() == cg.PAIRING_LANE            # the default; every test here restores it
    for bad in (-1, 2, 7):
        assert cg.load().capgpu_pairing_set_form(bad) == -1    # CAPGPU_ERR_INVALID_ARG
        assert cg.pairing_get_form() == cg.PAIRING_LANE
    try:
        cg.pairing_set_form(cg.PAIRING_WAVE)
        assert cg.pairing_get_form() == cg.PAIRING_WAVE
    finally:
        cg.pairing_set_form(cg.PAIRING_LANE)
    assert cg.pairing_get_form() == cg.PAIRING_LANE
    assert cg.load().capgpu_pairing_get_form(None) == -1


@pytest.fixture(scope="module")
def ladder():
    """70 distinct (a_i, [a_i]G, [a_i b]G) from random 254-bit scalars, and b: shared by the tests below, never changed"""
    rng = random.Random(0x9A7E)
    b = rng.randrange(1 << 253, bn.R)
    return b, scalar_ladder(rng, 70, b)


def mixed_checks(lad, count):
    """check i of a call: accepted e([a]G, [b]H) e(-[ab]G, H), rejected with R's y coordinate changed to its negative
    (every word of the coordinate differs; a single changed word would leave the curve, which the entry point refuses
    as an argument error, not a verdict) or with [ab + 1]G, and the cases at infinity - several kinds inside every
    wavefront and every group position -> (p words, r words, expected)"""
    p, r, want = [], [], []
    for i in range(count):
        _, P, S = lad[i % len(lad)]
        kind = (i * 5 + i // 7) % 7
        if kind in (0, 1, 2):
            p.append(P), r.append(g1_neg(S)), want.append(True)
        elif kind == 3:
            p.append(P), r.append(S), want.append(False)                           # y -> -y
        elif kind == 4:
            p.append(P), r.append(g1_neg(bn.g1_add(S, bn.G1_GEN))), want.append(False)
        elif kind == 5:
            p.append(None), r.append(g1_neg(S)), want.append(False)                # P at infinity
        else:
            p.append(P if i % 2 else None), r.append(None), want.append(i % 2 == 0)  # R at infinity / both
    return np.stack([g1_words(x) for x in p]), np.stack([g1_words(x) for x in r]), want


@pytest.mark.parametrize("count", [1, 3, PER_WAVE - 1, PER_WAVE, PER_WAVE + 1, 65])
def test_pairing_checks_agree_between_the_forms_and_with_the_host(cg, forms, ladder, count):
    """the tails of a group, of a wavefront (10 checks) and of the grid"""
    b, lad = ladder
    h2 = cg.g2_generator()
    bh = cg.g2_mul(h2, b)
    p, r, want = mixed_checks(lad, count if count > 3 else 7)
    if count <= 3:                                  # an accepted, a rejected and an infinity case even in the shortest call
        pick = [0, 3, 5][:count]
        p, r, want = p[pick], r[pick], [want[k] for k in pick]
    lane, dl, dw = forms(cg.PAIRING_LANE, lambda: cg.pairing_check_pairs_dev(p, r, bh, h2))
    assert (dl, dw) == (count, 0)
    wave, dl, dw = forms(cg.PAIRING_WAVE, lambda: cg.pairing_check_pairs_dev(p, r, bh, h2))
    assert (dl, dw) == (0, count)
    assert [bool(x) for x in wave] == want
    assert [bool(x) for x in lane] == want
    host = {}
    for i in range(count):
        key = p[i].tobytes() + r[i].tobytes()
        if key not in host:
            host[key] = host_verdict(cg, p[i], r[i], bh, h2)
        assert bool(wave[i]) == host[key], i


def test_a_g2_point_at_infinity_is_a_null_line_table_in_both_forms(cg, forms, ladder):
    """Q1, Q2 or both at infinity, with P or R at infinity mixed in, for a wavefront and a bit of checks.  A factor whose
    G2 point is at infinity is 1, so check i holds iff the other factor is 1 too, that is iff its G1 point is at
    infinity (the points of the ladder have prime order, e([a]G, Q) != 1): both device forms and the host
    pairing_check give exactly these verdicts, and none of them an argument error"""
    b, lad = ladder
    h2 = cg.g2_generator()
    bh = cg.g2_mul(h2, b)
    zero2 = np.zeros(16, np.uint64)
    p, r, _ = mixed_checks(lad, PER_WAVE + 3)
    n = len(p)
    p_inf, r_inf = [not p[i].any() for i in range(n)], [not r[i].any() for i in range(n)]
    assert any(p_inf) and any(r_inf) and not all(p_inf) and not all(r_inf)
    for q1, q2, want in ((zero2, h2, r_inf), (bh, zero2, p_inf), (zero2, zero2, [True] * n)):
        lane, dl, dw = forms(cg.PAIRING_LANE, lambda: cg.pairing_check_pairs_dev(p, r, q1, q2))
        assert (dl, dw) == (n, 0)
        wave, dl, dw = forms(cg.PAIRING_WAVE, lambda: cg.pairing_check_pairs_dev(p, r, q1, q2))
        assert (dl, dw) == (0, n)
        assert [bool(x) for x in wave] == want
        assert [bool(x) for x in lane] == want
        assert [host_verdict(cg, p[i], r[i], q1, q2) for i in range(n)] == want


@pytest.fixture(scope="module")
def proved(cg, tau):
    """the small synthetic circuits of the verify tests (n = 2^4 and 2^6), a proof with and one without ext_msg for each"""
    srs = cg.srs_generate(tau, (1 << 6) + 3)
    h2 = cg.g2_generator()
    bh = cg.g2_mul(h2, tau)
    out = []
    for log_n, nin, seed in ((4, 2, 91), (6, 3, 92)):
        sc = bu.synthetic_circuit(log_n, nin, seed=seed)
        pkh, vk = cg.plonk_preprocess(srs, sc.n, sc.num_inputs, sc.selectors_mont(), sc.sigma_mont())
        for k, msg in enumerate((None, b"memo")):
            w, pubs = sc.witness(700 + 10 * log_n + k)
            pr = cg.plonk_prove(pkh, sc.wires_mont(w), pubs_arr(pubs), bu.to_mont_array(bu.blinders(40 + k)), msg)
            out.append({"vk": vk, "pubs": pubs_arr(pubs), "proof": pr, "msg": msg})
        cg.plonk_free_key(pkh)
    yield {"h2": h2, "bh": bh, "proofs": out}
    cg.srs_free(srs)


def both(cg, env, vk, pubs, proof, msg):
    """(verdict or error code) of plonk_verify and of plonk_verify_dev: they must be the same"""
    def call(fn):
        try:
            return fn(vk, env["h2"], env["bh"], pubs, proof, msg)
        except cg.CapGpuError as e:
            return ("error", e.code if hasattr(e, "code") else str(e))
    host, dev = call(cg.plonk_verify), call(cg.plonk_verify_dev)
    assert host == dev, (host, dev)
    return dev


def test_plonk_verify_dev_accepts_what_the_prover_makes_and_uses_the_wave_kernel(cg, proved):
    assert cg.pairing_get_form() == cg.PAIRING_LANE
    for x in proved["proofs"]:
        before = cg.pairing_stats()
        assert both(cg, proved, x["vk"], x["pubs"], x["proof"], x["msg"]) is True
        after = cg.pairing_stats()
        assert after["wave_checks"] == before["wave_checks"] + 1 and after["lane_checks"] == before["lane_checks"]


def other_point(k):
    return g1_words(bn.g1_mul(bn.G1_GEN, 1000 + k))


def test_plonk_verify_dev_rejects_every_altered_commitment_evaluation_input_and_message(cg, proved):
    for x in (proved["proofs"][1], proved["proofs"][2]):           # n = 2^4 with a message, n = 2^6 without
        base = x["proof"]
        comms = [lambda pr, i=i: pr.wires_poly_comms[i] for i in range(5)]
        comms += [lambda pr: pr.prod_perm_poly_comm]
        comms += [lambda pr, i=i: pr.split_quot_poly_comms[i] for i in range(5)]
        comms += [lambda pr: pr.opening_proof, lambda pr: pr.shifted_opening_proof]
        evals = [lambda pr, i=i: pr.wires_evals[i] for i in range(5)]
        evals += [lambda pr, i=i: pr.wire_sigma_evals[i] for i in range(4)]
        evals += [lambda pr: pr.perm_next_eval]
        assert len(comms) == 13 and len(evals) == 10
        for k, get in enumerate(comms):                             # another point of the curve in its place
            pr = copy.deepcopy(base)
            for j, wd in enumerate(other_point(k)):
                get(pr)[j] = int(wd)
            assert both(cg, proved, x["vk"], x["pubs"], pr, x["msg"]) is False, ("commitment", k)
        for k, get in enumerate(evals):                             # another canonical field element
            pr = copy.deepcopy(base)
            get(pr)[0] ^= 1
            assert both(cg, proved, x["vk"], x["pubs"], pr, x["msg"]) is False, ("evaluation", k)
        pubs = x["pubs"].copy()
        pubs[0, 0] ^= 1
        assert both(cg, proved, x["vk"], pubs, base, x["msg"]) is False
        assert both(cg, proved, x["vk"], x["pubs"], base, (x["msg"] or b"") + b"!") is False
        # a field word of at least the modulus: whatever plonk_verify answers, verdict or error, the same here
        pr = copy.deepcopy(base)
        pr.wires_evals[2][:] = [0xFFFFFFFFFFFFFFFF] * 4
        both(cg, proved, x["vk"], x["pubs"], pr, x["msg"])
        pubs = x["pubs"].copy()
        pubs[1, :] = 0xFFFFFFFFFFFFFFFF
        both(cg, proved, x["vk"], pubs, base, x["msg"])
        pr = copy.deepcopy(base)
        pr.opening_proof[0:4] = [0xFFFFFFFFFFFFFFFF] * 4
        both(cg, proved, x["vk"], x["pubs"], pr, x["msg"])
        # a public-input count the key does not expect is an error in both
        assert both(cg, proved, x["vk"], x["pubs"][:1], base, x["msg"])[0] == "error"


def test_verify_each_and_batch_verify_under_the_wave_form(cg, forms, proved):
    """5 proofs over two keys, proof 3 corrupted: the same verdicts as under LANE; the batch is rejected, and accepted
    once proof 3 is repaired - its final pairing product then decided by one wave-form check on the device"""
    xs = [proved["proofs"][k] for k in (0, 2, 1, 3, 0)]
    vks, pubs, msgs = [x["vk"] for x in xs], [x["pubs"] for x in xs], [x["msg"] for x in xs]
    good = [x["proof"] for x in xs]
    bad = list(good)
    bad[3] = copy.deepcopy(good[3])
    bad[3].wires_evals[1][0] ^= 1
    h2, bh = proved["h2"], proved["bh"]
    lane, dl, dw = forms(cg.PAIRING_LANE, lambda: cg.plonk_verify_each(vks, h2, bh, pubs, bad, msgs))
    assert (dl, dw) == (5, 0)
    wave, dl, dw = forms(cg.PAIRING_WAVE, lambda: cg.plonk_verify_each(vks, h2, bh, pubs, bad, msgs))
    assert (dl, dw) == (0, 5)
    assert list(wave) == list(lane) == [True, True, True, False, True]

    def batch(proofs):
        return cg.plonk_batch_verify(vks, h2, bh, pubs, proofs, msgs, on_device=True)
    assert forms(cg.PAIRING_LANE, lambda: batch(bad)) == (False, 0, 0)          # the product on the host, as before
    assert forms(cg.PAIRING_WAVE, lambda: batch(bad)) == (False, 0, 1)
    assert forms(cg.PAIRING_LANE, lambda: batch(good)) == (True, 0, 0)
    assert forms(cg.PAIRING_WAVE, lambda: batch(good)) == (True, 0, 1)
