"""The block verifier where its job is to say no (capgpu_plonk_verify_block_dev, _resident, _bytes, _bytes_resident).

Forged blocks.  block_ok comes from the fold - seed, weights, gather, fold, two MSMs, one pairing check - and each_ok from
the unweighted terms, one check per proof; every other rejecting case of the suite holds a single bad proof, which a fold
with equal weights (r_i = 1 throughout, or a seed that never reaches k_verify_weights) rejects as well.  Here the bad
proofs come in sets whose errors cancel under equal weights: opening_proof moved by +D and -D on two copies of a proof
(nothing zeta or v depend on changes, each copy is off by +-(tau - zeta) D); by +D, +D, -2D on three; and by [a] G and
-[a (tau - zeta_i) / (tau - zeta_j)] G on two different proofs under two keys (tests/test_verify_forged_host.py shows on
the CPU that these errors do sum to the point at infinity).  Every forged block goes through every entry point next to a
clean control of the same layout, which must be accepted.

Every field.  k_verify_front re-implements the host's input checks on lanes 0..12 (points) and 13..22 (evaluations):
each of the 23 fields is tried in its second encoding (+p, +r) and each point off the curve, public inputs + r in every
lane round, and each field moved to another valid value (+1, +G); a block without one valid proof, where both sums are
the point at infinity and only the `every` flag of k_verify_verdicts keeps block_ok from 1.

The reference for every verdict is the host verifier (capgpu_plonk_verify, capgpu_plonk_batch_verify); no tolerance.
Environment: test_gpu_verify_block.py's (n = 2^8 with 4 inputs, n = 2^7 with none, a 2^8 + 3 SRS)."""
import copy
import ctypes

import numpy as np
import pytest

from cap_amd import bench_utils as bu
from oracle import bn254 as bn
from oracle import capref as cr
from tests import verify_block_model as vm
from tests.test_gpu_verify_block import Env, pubs_arr, rows
from tests.test_verify import _add_to_words

pytestmark = pytest.mark.gpu

POINT_FIELDS = [("wires_poly_comms", i) for i in range(5)] + [("prod_perm_poly_comm", None)] + \
    [("split_quot_poly_comms", i) for i in range(5)] + [("opening_proof", None), ("shifted_opening_proof", None)]
EVAL_FIELDS = [("wires_evals", i) for i in range(5)] + [("wire_sigma_evals", i) for i in range(4)] + \
    [("perm_next_eval", None)]
D777 = bn.g1_mul(bn.G1_GEN, 777)


@pytest.fixture(scope="module")
def env(cg, tau):
    e = Env(cg, tau)
    e.host_seen = {}
    yield e
    for h in e.vkh:
        cg.plonk_vk_release(h)
    for pkh, _ in e.keys:
        cg.plonk_free_key(pkh)
    cg.srs_free(e.srs)


@pytest.fixture(scope="module")
def pool(env):
    """eight clean proofs of key 0 with their public inputs; never modified"""
    return [env.prove(0, 1700 + i, b"forge") for i in range(8)]


def field_of(pr, name, i):
    return getattr(pr, name) if i is None else getattr(pr, name)[i]


def get_point(words):
    return cr.affine_to_ints(np.array(list(words), np.uint64))


def put_point(words, pt):
    for k, v in enumerate(cr.points_to_array([pt])[0]):
        words[k] = int(v)


def moved(pr, name, i, delta):
    """a copy of pr with one point moved by `delta` (a point of the curve)"""
    out = copy.deepcopy(pr)
    tgt = field_of(out, name, i)
    put_point(tgt, bn.g1_add(get_point(tgt), delta))
    return out


def host_each(env, vk, pubs, pr, msg):
    """capgpu_plonk_verify, once per distinct (key, inputs, proof, message)"""
    key = (bytes(vk), pubs.tobytes(), bytes(pr), msg)
    if key not in env.host_seen:
        env.host_seen[key] = env.cg.plonk_verify(vk, env.h2, env.bh, pubs, pr, msg)
    return env.host_seen[key]


def through_every_entry_point(env, handles, vks, pubs_l, proofs, msgs, bad, width=4):
    """block_ok is `not bad`, each_ok is False exactly at `bad`, block_ok == all(each_ok), and the host agrees - through
    plonk_verify_block (host arrays and resident, each on and off), plonk_verify_block_bytes (host and resident; the
    records decode: status 0), plonk_batch_verify on the device and on the host, and proof.txn_batch_verify"""
    from cap_amd import proof as papi
    cg = env.cg
    count = len(proofs)
    want_each = [i not in bad for i in range(count)]
    want = not bad
    assert [host_each(env, vks[i], pubs_l[i], proofs[i], msgs[i]) for i in range(count)] == want_each
    assert cg.plonk_batch_verify(vks, env.h2, env.bh, pubs_l, proofs, msgs) == want
    assert cg.plonk_batch_verify(vks, env.h2, env.bh, pubs_l, proofs, msgs, on_device=True) == want
    for resident in (False, True):
        ok, each = env.block(handles, pubs_l, proofs, msgs, width=width, each=True, resident=resident)
        assert (ok, list(each)) == (want, want_each) and ok == all(each), f"resident={resident}"
        assert env.block(handles, pubs_l, proofs, msgs, width=width, each=False, resident=resident) == want
    pr = rows(pubs_l, width)
    blob = b"".join(cg.proof_serialize(p) for p in proofs)
    ok, each, st = cg.plonk_verify_block_bytes(handles, env.h2, env.bh, pr, blob, msgs, each=True, num_inputs=width,
                                               status=True)
    assert list(st) == [0] * count and (ok, list(each)) == (want, want_each)
    assert cg.plonk_verify_block_bytes(handles, env.h2, env.bh, pr, blob, msgs, num_inputs=width) == want
    d_b = cg.DevBuf.from_numpy(np.frombuffer(blob, dtype=np.uint8))
    d_p = cg.DevBuf.from_numpy(pr if pr.size else np.zeros(4, np.uint64))
    try:
        ok, each, st = cg.plonk_verify_block_bytes(handles, env.h2, env.bh, d_p, d_b, msgs, each=True, num_inputs=width,
                                                   status=True)
        assert list(st) == [0] * count and (ok, list(each)) == (want, want_each)
        assert cg.plonk_verify_block_bytes(handles, env.h2, env.bh, d_p, d_b, msgs, num_inputs=width) == want
    finally:
        d_b.free()
        d_p.free()
    if want:
        papi.txn_batch_verify(handles, env.h2, env.bh, pr, proofs, msgs, num_inputs=width)
        papi.txn_batch_verify(handles, env.h2, env.bh, pr, blob, msgs, num_inputs=width)
    else:
        for form in (proofs, blob):
            with pytest.raises(papi.TxnApiError):
                papi.txn_batch_verify(handles, env.h2, env.bh, pr, form, msgs, num_inputs=width)


def padded(pool, count, at):
    """`count` clean proofs from the pool, with the proofs of `at` (index -> (proof, inputs)) in their places"""
    proofs = [pool[i % 8][0] for i in range(count)]
    pubs_l = [pool[i % 8][1] for i in range(count)]
    for i, (pr, pubs) in at.items():
        proofs[i], pubs_l[i] = pr, pubs
    return proofs, pubs_l


@pytest.mark.parametrize("i,j", [(0, 1), (1, 2), (0, 64), (63, 64), (64, 65)])
def test_a_pair_whose_errors_cancel_under_equal_weights(env, pool, i, j):
    """W + D and W - D on two copies of one proof, in a block of 66: index 0 has r_0 = 1, indices 64 and 65 cross the
    wavefront boundary of the weight, gather and fold kernels"""
    base, pubs = pool[3]
    plus = moved(base, "opening_proof", None, D777)
    minus = moved(base, "opening_proof", None, bn.g1_neg(D777))
    handles, vks, msgs = [env.vkh[0]] * 66, [env.keys[0][1]] * 66, [b"forge"] * 66
    proofs, pubs_l = padded(pool, 66, {i: (base, pubs), j: (base, pubs)})
    through_every_entry_point(env, handles, vks, pubs_l, proofs, msgs, [])              # the clean control
    proofs, pubs_l = padded(pool, 66, {i: (plus, pubs), j: (minus, pubs)})
    through_every_entry_point(env, handles, vks, pubs_l, proofs, msgs, [i, j])


def test_a_triple_whose_errors_cancel_under_equal_weights(env, pool):
    """W + D, W + D and W - 2D"""
    base, pubs = pool[5]
    plus = moved(base, "opening_proof", None, D777)
    minus2 = moved(base, "opening_proof", None, bn.g1_neg(bn.g1_mul(D777, 2)))
    handles, vks, msgs = [env.vkh[0]] * 7, [env.keys[0][1]] * 7, [b"forge"] * 7
    proofs, pubs_l = padded(pool, 7, {1: (base, pubs), 3: (base, pubs), 6: (base, pubs)})
    through_every_entry_point(env, handles, vks, pubs_l, proofs, msgs, [])
    proofs, pubs_l = padded(pool, 7, {1: (plus, pubs), 3: (plus, pubs), 6: (minus2, pubs)})
    through_every_entry_point(env, handles, vks, pubs_l, proofs, msgs, [1, 3, 6])


def test_two_different_proofs_under_two_keys_whose_errors_cancel(env, pool, tau):
    """proof i (key 0) gets W_i + [a] G, proof j (key 1) gets W_j - [a (tau - zeta_i) / (tau - zeta_j)] G; the zetas come
    from tests/verify_block_model.py (they do not depend on the openings)"""
    pi, pubs_i = pool[2]
    pj, pubs_j = env.prove(1, 1750, b"other")
    keys = [vm.Key.from_ctypes(k[1]) for k in env.keys]
    zi = vm.front(keys[0], cr.array_to_ints(pubs_i), vm.Proof.from_bytes(bytes(pi)), b"forge").chal["zeta"]
    zj = vm.front(keys[1], [], vm.Proof.from_bytes(bytes(pj)), b"other").chal["zeta"]
    a = 0xA11CE
    b = a * (tau - zi) % bn.R * pow((tau - zj) % bn.R, -1, bn.R) % bn.R
    fi = moved(pi, "opening_proof", None, bn.g1_mul(bn.G1_GEN, a))
    fj = moved(pj, "opening_proof", None, bn.g1_neg(bn.g1_mul(bn.G1_GEN, b)))
    ks = [0, 0, 0, 1, 0]
    handles, vks = [env.vkh[k] for k in ks], [env.keys[k][1] for k in ks]
    msgs = [b"forge"] * 3 + [b"other", b"forge"]
    proofs, pubs_l = padded(pool, 5, {1: (pi, pubs_i), 3: (pj, pubs_j)})
    through_every_entry_point(env, handles, vks, pubs_l, proofs, msgs, [])
    proofs, pubs_l = padded(pool, 5, {1: (fi, pubs_i), 3: (fj, pubs_j)})
    through_every_entry_point(env, handles, vks, pubs_l, proofs, msgs, [1, 3])


# ---- every field, on the device front end ---------------------------------------------------------------------------------
def both_ways(env, handles, vks, pubs_l, proofs, msgs, width=4):
    """(block_ok, each_ok) with each=True, block_ok again with each=False, against the host verifiers row by row"""
    count = len(proofs)
    host = [host_each(env, vks[i], pubs_l[i], proofs[i], msgs[i]) for i in range(count)]
    ok, each = env.block(handles, pubs_l, proofs, msgs, width=width, each=True)
    assert list(each) == host, [i for i in range(count) if bool(each[i]) != host[i]]
    assert ok == all(each) and env.block(handles, pubs_l, proofs, msgs, width=width, each=False) == ok
    return ok, list(each)


def test_checks_matrix_every_field_in_its_second_encoding_and_off_the_curve(env, pool):
    """one clean proof, then one proof per row: + p on x and on y of each of the 13 points, + r on each of the 10
    evaluations, x ^ 1 (off the curve) for each of the 13 points.  Exactly the clean proof is accepted."""
    base, pubs = pool[0]
    proofs, names = [base], ["clean"]
    for name, i in POINT_FIELDS:
        for off in (0, 4):
            pr = copy.deepcopy(base)
            _add_to_words((ctypes.c_uint64 * 4).from_buffer(field_of(pr, name, i), 8 * off), bn.P)
            proofs.append(pr); names.append(f"{name}[{i}] coordinate {off // 4} + p")
    for name, i in EVAL_FIELDS:
        pr = copy.deepcopy(base)
        _add_to_words(field_of(pr, name, i), bn.R)
        proofs.append(pr); names.append(f"{name}[{i}] + r")
    for name, i in POINT_FIELDS:
        pr = copy.deepcopy(base)
        field_of(pr, name, i)[0] ^= 1
        proofs.append(pr); names.append(f"{name}[{i}] x ^ 1")
    count = len(proofs)
    assert count == 1 + 26 + 10 + 13
    ok, each = both_ways(env, [env.vkh[0]] * count, [env.keys[0][1]] * count, [pubs] * count, proofs, [b"forge"] * count)
    assert not ok and [names[i] for i in range(count) if each[i]] == ["clean"]


def test_public_inputs_plus_r_in_every_lane_round(env):
    """the 254-input key of test_many_public_inputs_wrap_the_lane_stride: + r at input 0, 63, 64, 200 and 253, one at a
    time; each is rejected, as the host verifier rejects it"""
    cg = env.cg
    sc = bu.synthetic_circuit(8, 254, seed=64)
    pkh, vk = cg.plonk_preprocess(env.srs, sc.n, sc.num_inputs, sc.selectors_mont(), sc.sigma_mont())
    vkh = cg.plonk_vk_upload(vk)
    try:
        w, pubs = sc.witness(11)
        big = cg.plonk_prove(pkh, sc.wires_mont(w), pubs_arr(pubs), bu.to_mont_array(bu.blinders(12)), b"wide")
        small, no_pubs = env.prove(1, 13, b"none")
        handles, proofs, msgs = [vkh, env.vkh[1], vkh], [big, small, big], [b"wide", b"none", b"wide"]
        vks = [vk, env.keys[1][1], vk]
        clean = [pubs_arr(pubs), no_pubs, pubs_arr(pubs)]
        assert both_ways(env, handles, vks, clean, proofs, msgs, width=254) == (True, [True] * 3)
        for j in (0, 63, 64, 200, 253):
            pb = [p.copy() for p in clean]
            v = cr.array_to_ints(pb[2][j])[0] + bn.R
            assert v < 1 << 256
            pb[2][j] = cr.int_to_limbs(v)
            assert both_ways(env, handles, vks, pb, proofs, msgs, width=254) == (False, [True, True, False]), j
            assert cg.plonk_batch_verify(vks, env.h2, env.bh, pb, proofs, msgs) is False
    finally:
        cg.plonk_vk_release(vkh)
        cg.plonk_free_key(pkh)


def test_binding_matrix_every_field_moved_to_another_valid_value(env, pool):
    """23 tampered copies and one clean copy; every edit keeps its field valid: each evaluation + 1 mod r, each point + G.
    Only the clean copy is accepted."""
    base, pubs = pool[1]
    proofs, names = [], []
    for name, i in EVAL_FIELDS:
        pr = copy.deepcopy(base)
        tgt = field_of(pr, name, i)
        v = (bn.from_mont(cr.array_to_ints(np.array(list(tgt), np.uint64))[0], bn.R) + 1) % bn.R
        for k, word in enumerate(cr.int_to_limbs(bn.to_mont(v, bn.R))):
            tgt[k] = int(word)
        proofs.append(pr); names.append(f"{name}[{i}] + 1")
    for name, i in POINT_FIELDS:
        proofs.append(moved(base, name, i, bn.G1_GEN)); names.append(f"{name}[{i}] + G")
    proofs.insert(11, base); names.insert(11, "clean")
    count = len(proofs)
    assert count == 24
    ok, each = both_ways(env, [env.vkh[0]] * count, [env.keys[0][1]] * count, [pubs] * count, proofs, [b"forge"] * count)
    assert not ok and [names[i] for i in range(count) if each[i]] == ["clean"]


@pytest.mark.parametrize("count", [1, 2, 65])
def test_a_block_without_a_valid_proof_is_rejected(env, pool, count):
    """every proof fails its input checks (off-curve and non-canonical ones mixed): both sums are the point at infinity,
    on which the pairing check accepts - the `every` flag of k_verify_verdicts is what rejects the block"""
    cg = env.cg
    proofs, pubs_l = [], []
    for i in range(count):
        pr = copy.deepcopy(pool[i % 8][0])
        if i % 2:
            name, k = EVAL_FIELDS[i % 10]
            _add_to_words(field_of(pr, name, k), bn.R)
        else:
            name, k = POINT_FIELDS[i % 13]
            field_of(pr, name, k)[4] ^= 1
        proofs.append(pr); pubs_l.append(pool[i % 8][1])
    handles, vks, msgs = [env.vkh[0]] * count, [env.keys[0][1]] * count, [b"forge"] * count
    assert cg.plonk_batch_verify(vks, env.h2, env.bh, pubs_l, proofs, msgs) is False
    for resident in (False, True):
        ok, each = env.block(handles, pubs_l, proofs, msgs, each=True, resident=resident)
        assert ok is False and list(each) == [False] * count
        assert env.block(handles, pubs_l, proofs, msgs, each=False, resident=resident) is False
    assert [host_each(env, vks[i], pubs_l[i], proofs[i], msgs[i]) for i in range(min(count, 4))] == [False] * min(count, 4)


def test_degenerate_proofs_in_one_block_equal_the_host(env, pool):
    """the variants of test_plonk_verify_each_on_degenerate_proofs_equals_plonk_verify in one block: both openings at
    infinity, all commitments at infinity, all evaluations 0, all evaluations r - 1"""
    cg = env.cg
    base, pubs = pool[4]
    rm1 = [int(x) for x in bu.to_mont_array([bn.R - 1]).reshape(-1)]

    def put(dst, src):
        for k in range(len(src)):
            dst[k] = src[k]

    def variant(edit):
        pr = copy.deepcopy(base)
        edit(pr)
        return pr

    def all_evals(pr, words):
        for name, i in EVAL_FIELDS:
            put(field_of(pr, name, i), words)
    variants = {
        "untouched": base,
        "both opening proofs at infinity": variant(lambda pr: (put(pr.opening_proof, [0] * 8),
                                                                put(pr.shifted_opening_proof, [0] * 8))),
        "all commitments at infinity": variant(lambda pr: [put(field_of(pr, n, i), [0] * 8) for n, i in POINT_FIELDS]),
        "all evaluations zero": variant(lambda pr: all_evals(pr, [0] * 4)),
        "all evaluations r - 1": variant(lambda pr: all_evals(pr, rm1)),
    }
    names = list(variants)
    proofs = [variants[n] for n in names]
    count = len(proofs)
    handles, vks, pubs_l, msgs = [env.vkh[0]] * count, [env.keys[0][1]] * count, [pubs] * count, [b"forge"] * count
    ok, each = both_ways(env, handles, vks, pubs_l, proofs, msgs)
    assert each[0], "the untouched proof"
    assert ok == cg.plonk_batch_verify(vks, env.h2, env.bh, pubs_l, proofs, msgs)
    # and each degenerate proof alone, where no other proof's terms hide its sums
    for i in range(1, count):
        ok1, each1 = both_ways(env, handles[:1], vks[:1], pubs_l[:1], [proofs[i]], msgs[:1])
        assert ok1 == cg.plonk_batch_verify(vks[:1], env.h2, env.bh, pubs_l[:1], [proofs[i]], msgs[:1]), names[i]
