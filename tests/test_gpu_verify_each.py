"""Per-proof verification on the device (capgpu_plonk_verify_each_dev, capgpu_pairing_check_pairs_dev): one verdict per
proof / pairing check, each equal to the host verifier's (capgpu_plonk_verify / capgpu_pairing_check)."""
import copy

import numpy as np
import pytest

from cap_amd import bench_utils as bu
from oracle import bn254 as bn

pytestmark = pytest.mark.gpu


def pubs_arr(pubs):
    return bu.to_mont_array(pubs) if pubs else np.zeros((0, 4), np.uint64)


def g1_words(pt):
    """affine oracle point -> 8 Montgomery words (infinity = zeros)"""
    if pt is None:
        return np.zeros(8, np.uint64)
    return np.array(bn.limbs_le(bn.to_mont(pt[0], bn.P)) + bn.limbs_le(bn.to_mont(pt[1], bn.P)), np.uint64)


def g1_neg(pt):
    return None if pt is None else (pt[0], (-pt[1]) % bn.P)


def test_pairing_check_pairs_on_the_device_matches_the_host(cg):
    h2 = cg.g2_generator()
    rng = np.random.default_rng(7)
    a, b = 1234567, 7654321
    bh = cg.g2_mul(h2, b)
    aG, abG, ab1G = bn.g1_mul(bn.G1_GEN, a), bn.g1_mul(bn.G1_GEN, a * b), bn.g1_mul(bn.G1_GEN, a * b + 1)
    # e([a]G, [b]H) e(-[ab]G, H) = 1;  with ab + 1: != 1;  infinity entries are factors of 1
    p = np.stack([g1_words(aG), g1_words(aG), g1_words(None), g1_words(None), g1_words(aG)])
    r = np.stack([g1_words(g1_neg(abG)), g1_words(g1_neg(ab1G)), g1_words(None), g1_words(g1_neg(abG)), g1_words(None)])
    assert list(cg.pairing_check_pairs_dev(p, r, bh, h2)) == [True, False, True, False, False]
    # counts around the wave size: a mix of accepted and rejected checks, each against the host pairing check
    pool = [bn.g1_mul(bn.G1_GEN, k) for k in (3, 5, 15, 7)]
    for cnt in (0, 1, 63, 64, 65, 1000):
        kinds = rng.integers(0, 4, size=cnt)
        ps, rs = [], []
        for k in kinds:
            if k == 0:    # accepted: e([3]G, [b]H) e(-[3b]G, H)
                ps.append(g1_words(pool[0])); rs.append(g1_words(g1_neg(bn.g1_mul(bn.G1_GEN, 3 * b))))
            elif k == 1:  # rejected
                ps.append(g1_words(pool[1])); rs.append(g1_words(g1_neg(pool[2])))
            elif k == 2:  # both at infinity
                ps.append(g1_words(None)); rs.append(g1_words(None))
            else:         # one at infinity
                ps.append(g1_words(None)); rs.append(g1_words(pool[3]))
        p = np.array(ps, np.uint64).reshape(-1, 8)
        r = np.array(rs, np.uint64).reshape(-1, 8)
        got = cg.pairing_check_pairs_dev(p, r, bh, h2)
        assert got.shape == (cnt,)
        host = {}
        for i in range(cnt):
            key = int(kinds[i])
            if key not in host:
                host[key] = cg.pairing_check(np.stack([p[i], r[i]]), np.stack([bh, h2]))
            assert bool(got[i]) == host[key], (cnt, i)
    # off-curve input names the index
    bad = np.stack([g1_words(aG)] * 3)
    bad[2, 4] ^= np.uint64(1)
    with pytest.raises(cg.CapGpuError):
        cg.pairing_check_pairs_dev(np.stack([g1_words(aG)] * 3), bad, bh, h2)
    assert b"input 2" in cg.load().capgpu_last_error()
    off_twist = bh.copy()
    off_twist[0] ^= np.uint64(1)
    with pytest.raises(cg.CapGpuError):
        cg.pairing_check_pairs_dev(p[:1], r[:1], off_twist, h2)


def test_plonk_verify_each_flags_exactly_the_bad_proofs(cg, tau):
    """The 9 proofs under two keys of test_gpu_plonk's device batch-verifier test, with its corruptions (wrong public
    input, another curve point in a commitment, wrong key, swapped messages) plus a non-canonical evaluation and an
    off-curve point: each verdict equals plonk_verify's, and exactly the corrupted proofs are rejected."""
    srs = cg.srs_generate(tau, (1 << 8) + 3)
    h2 = cg.g2_generator()
    bh = cg.g2_mul(h2, tau)
    circuits = [bu.synthetic_circuit(8, 4, seed=61), bu.synthetic_circuit(7, 0, seed=62)]
    keys = [cg.plonk_preprocess(srs, sc.n, sc.num_inputs, sc.selectors_mont(), sc.sigma_mont()) for sc in circuits]
    vks, pubs_l, proofs, msgs = [], [], [], []
    for i in range(9):
        k = i % 2
        w, pubs = circuits[k].witness(300 + i)
        msg = b"n%d" % i if i % 3 else None
        pr = cg.plonk_prove(keys[k][0], circuits[k].wires_mont(w), pubs_arr(pubs), bu.to_mont_array(bu.blinders(400 + i)),
                            msg)
        vks.append(keys[k][1]); pubs_l.append(pubs_arr(pubs)); proofs.append(pr); msgs.append(msg)

    def each(v, p, pr, m):
        got = cg.plonk_verify_each(v, h2, bh, p, pr, m)
        host = [cg.plonk_verify(v[i], h2, bh, p[i], pr[i], m[i]) for i in range(len(pr))]
        assert list(got) == host
        return [i for i, ok in enumerate(got) if not ok]

    assert each(vks, pubs_l, proofs, msgs) == []
    assert each(vks[:1], pubs_l[:1], proofs[:1], msgs[:1]) == []
    assert len(cg.plonk_verify_each([], h2, bh, [], [], [])) == 0
    pubs_b, proofs_b, msgs_b, vks_b = [p.copy() for p in pubs_l], [copy.deepcopy(p) for p in proofs], list(msgs), list(vks)
    pubs_b[4][1, 0] ^= 1                                                    # wrong public input
    for k in range(8):
        proofs_b[3].wires_poly_comms[0][k] = proofs[5].wires_poly_comms[1][k]   # another point of the curve
    msgs_b[1], msgs_b[7] = msgs[7], msgs[1]                                 # swapped messages
    proofs_b[8].wires_evals[2][:] = [0xFFFFFFFFFFFFFFFF] * 4  # non-canonical evaluation (>= r)
    proofs_b[0].opening_proof[4] ^= 1                                       # off the curve
    bad = each(vks_b, pubs_b, proofs_b, msgs_b)
    assert bad == [0, 1, 3, 4, 7, 8]
    # a proof under the wrong key: a third key of key 0's shape (4 public inputs)
    twin = bu.synthetic_circuit(8, 4, seed=63)
    twin_key = cg.plonk_preprocess(srs, twin.n, twin.num_inputs, twin.selectors_mont(), twin.sigma_mont())
    keys.append(twin_key)
    assert each([vks[0], twin_key[1], vks[0]], [pubs_l[0], pubs_l[2], pubs_l[4]], [proofs[0], proofs[2], proofs[4]],
                [msgs[0], msgs[2], msgs[4]]) == [1]
    # malformed arguments are errors, as in the batch verifier: a public-input count the key does not expect
    with pytest.raises(cg.CapGpuError):
        cg.plonk_verify_each([vks[0]], h2, bh, [pubs_l[1]], [proofs[0]], [msgs[0]])
    for pkh, _ in keys:
        cg.plonk_free_key(pkh)
    cg.srs_free(srs)


def test_verify_each_finds_three_bad_transfer_notes_in_64(cg, tau):
    """64 full-size transfer-note proofs (n = 2^15, 27 public inputs), 3 corrupted at known indices: exactly those are
    flagged, and the batch verifier on the device accepts the remaining 61."""
    sc = bu.note_circuit("transfer_2x2", seed=2)
    assert sc.n == 1 << 15 and sc.num_inputs == 27
    srs = cg.srs_generate(tau, sc.n + 3)
    pkh, vk = cg.plonk_preprocess(srs, sc.n, sc.num_inputs, sc.selectors_mont(), sc.sigma_mont())
    h2 = cg.g2_generator()
    bh = cg.g2_mul(h2, tau)
    count = 64
    ws, ps, bs = [], [], []
    for i in range(4):
        w, pubs = sc.witness(50 + i)
        ws.append(sc.wires_mont(w)); ps.append(pubs_arr(pubs)); bs.append(bu.to_mont_array(bu.blinders(50 + i)))
    wires = np.stack([ws[i % 4] for i in range(count)])
    pubs_all = np.stack([ps[i % 4] for i in range(count)])
    blind = np.stack([bu.to_mont_array(bu.blinders(900 + i)) for i in range(count)])
    proofs = cg.plonk_prove_batch(pkh, wires, pubs_all, blind, b"memo", count)
    pubs_l = [pubs_all[i].copy() for i in range(count)]
    msgs = [b"memo"] * count
    bad_idx = [5, 33, 62]
    pubs_l[5][26, 0] ^= 1
    proofs[33] = copy.deepcopy(proofs[33])
    for k in range(8):
        proofs[33].opening_proof[k] = proofs[34].opening_proof[k]
    msgs[62] = b"memO"
    got = cg.plonk_verify_each([vk] * count, h2, bh, pubs_l, proofs, msgs)
    assert [i for i in range(count) if not got[i]] == bad_idx
    good = [i for i in range(count) if i not in bad_idx]
    assert cg.plonk_batch_verify([vk] * len(good), h2, bh, [pubs_l[i] for i in good], [proofs[i] for i in good],
                                 [msgs[i] for i in good], on_device=True)
    for i in (0, 5, 33, 62):
        assert bool(got[i]) == cg.plonk_verify(vk, h2, bh, pubs_l[i], proofs[i], msgs[i])
    cg.plonk_free_key(pkh)
    cg.srs_free(srs)
