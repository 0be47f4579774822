"""CPU companion of tests/test_gpu_verify_forged.py: the forged pair and triple rebuilt from one oracle proof at n = 16.

With tau known, a proof's error is e = tau A - B over oracle.plonk.verifier_pairing_inputs (the proof holds iff e is the
point at infinity).  Moving opening_proof by D changes nothing zeta or v depend on, and moves e by (tau - zeta) D.  So
for W + D and W - D on two copies of a proof, and for W + D, W + D, W - 2D on three, every error is a point other than
infinity and the errors sum to infinity: a batch verifier whose weights are all equal accepts these blocks.  The host's
capgpu_plonk_batch_verify must reject them and accept the clean control.  (The same edit on shifted_opening_proof would
not cancel: its term carries u, which the edit changes.)"""
import copy

import pytest

from cap_amd import bench_utils as bu
from cap_amd import lib as cg
from oracle import bn254 as bn
from oracle import plonk as pl
from tests import helpers as H
from tests.test_verify import make_proof, make_vk

D = bn.g1_mul(bn.G1_GEN, 777)


@pytest.fixture(scope="module")
def made(tau):
    """one oracle proof (n = 16, 2 public inputs), reused by every test"""
    sc = bu.synthetic_circuit(4, 2, seed=11)
    w, pubs = sc.witness(11)
    pk = pl.preprocess(pl.Circuit(n=sc.n, num_inputs=2, selectors=sc.selectors, sigma=sc.sigma), tau)
    op = pl.prove(pk, w, pubs, bu.blinders(11), ext_msg=b"forge")
    return sc, pk, pubs, op


def with_opening(op, delta):
    out = copy.copy(op)
    out.opening_proof = bn.g1_add(op.opening_proof, delta)
    return out


_errors = {}


def error(made, op, tau):
    """tau A - B, once per distinct opening (the pair and the triple share W + D)"""
    sc, pk, pubs, _ = made
    if op.opening_proof not in _errors:
        a, b = pl.verifier_pairing_inputs(sc.n, 2, pk.selector_comms, pk.sigma_comms, pubs, op, b"forge")
        _errors[op.opening_proof] = bn.g1_add(bn.g1_mul(a, tau), bn.g1_neg(b))
    return _errors[op.opening_proof]


def forged_sets(op):
    return {"pair": [with_opening(op, D), with_opening(op, bn.g1_neg(D))],
            "triple": [with_opening(op, D), with_opening(op, D), with_opening(op, bn.g1_neg(bn.g1_mul(D, 2)))]}


def test_the_errors_of_each_forged_set_cancel_under_equal_weights(made, tau):
    op = made[3]
    assert error(made, op, tau) == bn.INF
    for name, forged in forged_sets(op).items():
        errs = [error(made, f, tau) for f in forged]
        assert all(e != bn.INF for e in errs), name
        total = bn.INF
        for e in errs:
            total = bn.g1_add(total, e)
        assert total == bn.INF, name


def test_the_host_batch_verifier_rejects_them_and_accepts_the_control(made, tau):
    sc, pk, pubs, op = made
    h2 = cg.g2_generator()
    bh = cg.g2_mul(h2, tau)
    vk = make_vk(sc.n, 2, pk.selector_comms, pk.sigma_comms)
    pub_arr = bu.to_mont_array(pubs)
    clean = make_proof(*H.oracle_proof_points(op))
    assert cg.plonk_verify(vk, h2, bh, pub_arr, clean, b"forge")
    for name, forged in forged_sets(op).items():
        k = len(forged)
        proofs = [make_proof(*H.oracle_proof_points(f)) for f in forged]
        assert [cg.plonk_verify(vk, h2, bh, pub_arr, p, b"forge") for p in proofs] == [False] * k, name
        for lead in (0, 1):                      # the forged set at the head of the block, and behind a clean proof
            block = [clean] * lead + proofs
            n = len(block)
            assert cg.plonk_batch_verify([vk] * n, h2, bh, [pub_arr] * n, [clean] * n, [b"forge"] * n) is True, name
            assert cg.plonk_batch_verify([vk] * n, h2, bh, [pub_arr] * n, block, [b"forge"] * n) is False, name
