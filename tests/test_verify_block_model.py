"""tests/verify_block_model.py against the oracle, without a GPU: for one proof the model's 34 scalars on their points must
give oracle.plonk.verifier_pairing_inputs' A (the a-terms) and B (all the others); a folded block of valid proofs must
satisfy tau A == B, and stop doing so when one opening is moved; the input checks must refuse what the host verifier's
non-canonical matrix (tests/test_verify.py) refuses."""
import copy

import pytest

from cap_amd import bench_utils as bu
from oracle import bn254 as bn
from oracle import capref as cr
from oracle import plonk as pl
from tests import helpers as H
from tests import verify_block_model as vm


@pytest.fixture(scope="module")
def made(tau):
    """two oracle proofs under two keys (n = 16 with 2 inputs, n = 32 with 3)"""
    out = []
    for log_n, nin, seed, msg in ((4, 2, 11, b"note-11"), (5, 3, 12, None)):
        sc = bu.synthetic_circuit(log_n, nin, seed=seed)
        w, pubs = sc.witness(seed)
        pk = pl.preprocess(pl.Circuit(n=sc.n, num_inputs=nin, selectors=sc.selectors, sigma=sc.sigma), tau)
        op = pl.prove(pk, w, pubs, bu.blinders(seed), ext_msg=msg)
        key = vm.Key(sc.n, nin, list(pk.selector_comms), list(pk.sigma_comms))
        out.append((key, pubs, op, msg))
    return out


def sum_terms(key, fr, terms):
    acc = bn.INF
    for t in terms:
        acc = bn.g1_add(acc, bn.g1_mul(vm.term_point(key, fr, t), fr.scalars[t]))
    return acc


def test_one_proof_gives_the_oracles_pairing_inputs(made):
    for key, pubs, op, msg in made:
        pts, ev = H.oracle_proof_points(op)
        fr = vm.front(key, [vm.mont(p) for p in pubs], vm.Proof.from_values(pts, ev), msg)
        a, b = pl.verifier_pairing_inputs(key.n, key.num_inputs, key.sel, key.sig, pubs, op, msg)
        assert sum_terms(key, fr, range(vm.A_TERMS)) == a
        assert sum_terms(key, fr, range(vm.A_TERMS, vm.TERMS)) == b
        assert all(0 <= s < bn.R for s in fr.scalars) and len(fr.scalars) == vm.TERMS


def test_a_folded_block_pairs_up_and_a_moved_opening_does_not(made, tau):
    keys = [m[0] for m in made]
    order = [0, 1, 0]
    pubs_raw = [[vm.mont(p) for p in made[k][1]] for k in order]
    proofs = [vm.Proof.from_values(*H.oracle_proof_points(made[k][2])) for k in order]
    msgs = [made[k][3] for k in order]
    blk = vm.block(keys, order, pubs_raw, proofs, msgs)
    assert blk.valid == [1, 1, 1] and blk.weights[0] == 1 and all(1 < w < 1 << 128 for w in blk.weights[1:])
    assert blk.S == bn.keccak256(b"".join(bn.fr_to_bytes_le(f.chal["u"]) for f in blk.fronts))
    a, nb = cr.affine_to_ints(blk.A), cr.affine_to_ints(blk.negB)
    assert bn.g1_mul(a, tau) == bn.g1_neg(nb)
    # the same sums by hand: A = sum r_i (W_i + u_i W'_i)
    acc = bn.INF
    for i, f in enumerate(blk.fronts):
        acc = bn.g1_add(acc, bn.g1_mul(sum_terms(keys[order[i]], f, range(vm.A_TERMS)), blk.weights[i]))
    assert acc == a
    moved = copy.deepcopy(proofs)
    w = bn.g1_add(H.oracle_proof_points(made[0][2])[0][11], bn.g1_mul(bn.G1_GEN, 777))
    moved[2].pts[11] = (vm.mont(w[0], bn.P), vm.mont(w[1], bn.P))
    bad = vm.block(keys, order, pubs_raw, moved, msgs)
    assert bad.valid == [1, 1, 1] and bad.S != blk.S            # u_2 is drawn after the openings: the seed moves with it
    assert bn.g1_mul(cr.affine_to_ints(bad.A), tau) != bn.g1_neg(cr.affine_to_ints(bad.negB))


def test_input_checks_refuse_every_second_encoding(made):
    key, pubs, op, msg = made[0]
    pubs_raw = [vm.mont(p) for p in pubs]
    good = vm.Proof.from_values(*H.oracle_proof_points(op))
    assert vm.front(key, pubs_raw, good, msg) is not None
    for i in range(13):
        for c in range(2):
            pr = copy.deepcopy(good)
            xy = list(pr.pts[i]); xy[c] += bn.P; pr.pts[i] = tuple(xy)
            assert vm.front(key, pubs_raw, pr, msg) is None
        pr = copy.deepcopy(good)
        pr.pts[i] = (pr.pts[i][0] ^ 1, pr.pts[i][1])
        assert vm.front(key, pubs_raw, pr, msg) is None
    for i in range(10):
        pr = copy.deepcopy(good)
        pr.ev[i] += bn.R
        assert vm.front(key, pubs_raw, pr, msg) is None
    for i in range(len(pubs_raw)):
        pb = list(pubs_raw); pb[i] += bn.R
        assert vm.front(key, pb, good, msg) is None
    inf = copy.deepcopy(good)
    inf.pts[3] = (0, 0)
    assert vm.front(key, pubs_raw, inf, msg) is not None         # infinity is a point of the group
    blk = vm.block([key], [0, 0], [pubs_raw, pubs_raw], [good, pr], [msg, msg])
    assert blk.valid == [1, 0] and blk.ubytes[1] == bytes(32) and blk.scalars[1] == [0] * vm.TERMS
    assert not blk.pts[2:4].any() and not blk.pts[4 + 13:4 + 26].any() and blk.sc[2:4] == [0, 0]
    assert vm.Proof.from_bytes(good.struct_bytes()).struct_bytes() == good.struct_bytes()
