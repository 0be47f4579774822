"""The public-input polynomial reaches the quotient as COEFFICIENTS: k_quotient leaves PI(x) out of the numerator and the
inverse 6n transform adds kappa * PI_i, kappa = 1 / (5^(6n) - 1), to each of the six blocks of n coefficients
(cap_amd/csrc/ntt.hpp: Ntt3Domain::kappa; prove_run.hpp: pi_fold; the identity itself: tests/test_pi_fold_identity.py).
The quotient is the same polynomial, so every proof must stay what it was, byte for byte: the C oracle's."""
from contextlib import contextmanager

import numpy as np
import pytest

from cap_amd import bench_utils as bu
from oracle import capref as cr
from tests import helpers as H

pytestmark = pytest.mark.gpu


def pubs_arr(pubs):
    return bu.to_mont_array(pubs) if pubs else np.zeros((0, 4), np.uint64)


def make_case(cg, tau, log_n, nin, P, seed):
    """(srs, key, C-oracle key, wires [P], public inputs [P], blinders [P]) of a synthetic circuit"""
    sc = bu.synthetic_circuit(log_n, nin, seed=seed)
    h = cg.srs_generate(tau, sc.n + 3)
    pkh, _vk = cg.plonk_preprocess(h, sc.n, nin, sc.selectors_mont(), sc.sigma_mont())
    key = cr.PlonkKey(cg.srs_download(h, 0, sc.n + 3), sc.n, nin, sc.selectors_mont(), sc.sigma_mont())
    ws, ps, bls = [], [], []
    for p in range(P):
        w, pubs = sc.witness(300 + p)
        ws.append(sc.wires_mont(w)); ps.append(pubs_arr(pubs)); bls.append(bu.to_mont_array(bu.blinders(400 + p)))
    return sc, h, pkh, key, np.stack(ws), np.stack(ps), np.stack(bls)


def oracle_points(key, ws, ps, bls, msg):
    out = []
    for p in range(len(ws)):
        rc, comms, evals = key.prove(ws[p], ps[p], bls[p], msg)
        assert rc == 0
        out.append(H.cref_proof_points(comms, evals))
    return out


@contextmanager
def transcript(cg, mode):
    old = cg.plonk_get_transcript()
    cg.plonk_set_transcript(mode)
    try:
        yield
    finally:
        cg.plonk_set_transcript(old)


# (4, 1, 1) the smallest domain; (5, 0, 2) no public inputs: the null addend; (6, 27, 3) the transfer note's count;
# (11, 5, 2) M = 2^12: the first size whose transforms take two passes
@pytest.mark.parametrize("log_n,nin,P", [(4, 1, 1), (5, 0, 2), (6, 27, 3), (11, 5, 2)])
def test_proofs_equal_the_c_oracles(cg, tau, log_n, nin, P):
    sc, h, pkh, key, ws, ps, bls = make_case(cg, tau, log_n, nin, P, seed=70 + log_n)
    msg = b"pi-fold"
    proofs = cg.plonk_prove_batch(pkh, ws, ps, bls, msg, P)
    want = oracle_points(key, ws, ps, bls, msg)
    for p in range(P):
        assert H.proof_points(proofs[p]) == want[p], f"proof {p}"
    cg.plonk_free_key(pkh)
    cg.srs_free(h)


def test_coefficient_form_input(cg, tau):
    log_n, nin, P = 6, 4, 2
    sc, h, pkh, key, ws, ps, bls = make_case(cg, tau, log_n, nin, P, seed=81)
    wc = np.stack([cr.ntt_fr(c, log_n, True, False).reshape(-1, 4) for c in ws.reshape(-1, sc.n, 4)]).reshape(ws.shape)
    proofs = cg.plonk_prove_batch(pkh, wc, ps, bls, b"memo", P, input_form="coeffs")
    want = oracle_points(key, ws, ps, bls, b"memo")
    for p in range(P):
        assert H.proof_points(proofs[p]) == want[p], f"proof {p}"
    cg.plonk_free_key(pkh)
    cg.srs_free(h)


def test_device_transcript(cg, tau):
    log_n, nin, P = 6, 3, 2
    sc, h, pkh, key, ws, ps, bls = make_case(cg, tau, log_n, nin, P, seed=82)
    with transcript(cg, "device"):
        proofs = cg.plonk_prove_batch(pkh, ws, ps, bls, b"memo", P)
    want = oracle_points(key, ws, ps, bls, b"memo")
    for p in range(P):
        assert H.proof_points(proofs[p]) == want[p], f"proof {p}"
    cg.plonk_free_key(pkh)
    cg.srs_free(h)


def test_two_keys_with_different_public_input_counts(cg, tau):
    """One batch, one domain, keys of 5 and of 0 public inputs (rows padded to 5, garbage in the padding): the addend of
    a proof is its own key's polynomial - zero for the key without inputs.  Each proof equals its single-key call's."""
    log_n = 6
    n = 1 << log_n
    srs = cg.srs_generate(tau, n + 3)
    circuits = [bu.synthetic_circuit(log_n, ni, seed=seed) for ni, seed in ((5, 91), (0, 92))]
    keys = [cg.plonk_preprocess(srs, n, sc.num_inputs, sc.selectors_mont(), sc.sigma_mont())[0] for sc in circuits]
    order = [1, 0, 0, 1]
    wires, rows, blinds, msgs, alone = [], [], [], [], []
    for i, k in enumerate(order):
        sc = circuits[k]
        w, pubs = sc.witness(700 + i)
        bl = bu.to_mont_array(bu.blinders(800 + i))
        row = np.full((5, 4), 0xFFFF, np.uint64)
        if pubs:
            row[:len(pubs)] = bu.to_mont_array(pubs)
        wires.append(sc.wires_mont(w)); rows.append(row); blinds.append(bl); msgs.append(b"note-%d" % i)
        alone.append(cg.plonk_prove_batch(keys[k], sc.wires_mont(w)[None], pubs_arr(pubs)[None], bl[None], msgs[i], 1)[0])
    got = cg.plonk_prove_multi([keys[k] for k in order], np.stack(wires), np.stack(rows), np.stack(blinds), msgs)
    for i in range(len(order)):
        assert bytes(got[i]) == bytes(alone[i]), i
    for pkh in keys:
        cg.plonk_free_key(pkh)
    cg.srs_free(srs)


def test_public_inputs_that_differ_from_the_witness_are_refused(cg, tau):
    """The addend is built from the CALLER's public inputs.  Where they are not the witness's public values the numerator
    is not divisible by Z_H, the quotient's top coefficients do not cancel, and the degree check - which runs after the
    addend - refuses the proof with CAPGPU_ERR_PROOF (-7), as it did when PI went through the evaluation domain.  The
    other proof of the batch is not affected by a later good call."""
    log_n, nin, P = 5, 2, 2
    sc, h, pkh, key, ws, ps, bls = make_case(cg, tau, log_n, nin, P, seed=83)
    bad = ps.copy()
    bad[1, 0, 0] ^= 1
    with pytest.raises(cg.CapGpuError) as e:
        cg.plonk_prove_batch(pkh, ws, bad, bls, None, P)
    assert e.value.code == -7
    proofs = cg.plonk_prove_batch(pkh, ws, ps, bls, None, P)
    want = oracle_points(key, ws, ps, bls, None)
    for p in range(P):
        assert H.proof_points(proofs[p]) == want[p], f"proof {p}"
    cg.plonk_free_key(pkh)
    cg.srs_free(h)
