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


# ---- through the public entry points: data that differs from lane to lane, boundary relations, degenerate proofs ------
def g2_words(q):
    """oracle twist point -> 16 Montgomery words (x.c0, x.c1, y.c0, y.c1); None = sixteen zero words"""
    if q is None:
        return np.zeros(16, np.uint64)
    return np.array([w for c in (q[0][0], q[0][1], q[1][0], q[1][1]) for w in bn.limbs_le(bn.to_mont(c, bn.P))], np.uint64)


def plus_p(words, k):
    """the same residue written as value + p in the 4-word coordinate k (fits in 256 bits: non-canonical)"""
    out = np.array(words, np.uint64).copy()
    v = bn.from_limbs_le([int(x) for x in out[4 * k:4 * k + 4]]) + bn.P
    assert v < 1 << 256
    out[4 * k:4 * k + 4] = bn.limbs_le(v)
    return out


def host_verdict(cg, p, r, q1, q2):
    """what the host pairing_check does with one check: its verdict, or "error" """
    try:
        return cg.pairing_check(np.stack([p, r]), np.stack([q1, q2]))
    except cg.CapGpuError:
        return "error"


def dev_verdict(cg, p, r, q1, q2):
    try:
        return bool(cg.pairing_check_pairs_dev(p[None], r[None], q1, q2)[0])
    except cg.CapGpuError:
        return "error"


def scalar_ladder(rng, count, b_over_c):
    """count distinct checks from random 254-bit scalars: P_i = [a_i]G and S_i = [a_i b / c]G with a_i = a_0 + i d
    (one point addition per step instead of a scalar multiplication) -> [(a_i, P_i, S_i)]"""
    a, d = rng.randrange(1 << 253, bn.R), rng.randrange(1 << 253, bn.R)
    P, S = bn.g1_mul(bn.G1_GEN, a), bn.g1_mul(bn.G1_GEN, a * b_over_c % bn.R)
    dP, dS = bn.g1_mul(bn.G1_GEN, d), bn.g1_mul(bn.G1_GEN, d * b_over_c % bn.R)
    out = []
    for _ in range(count):
        out.append((a, P, S))
        a, P, S = (a + d) % bn.R, bn.g1_add(P, dP), bn.g1_add(S, dS)
    return out


def test_pairing_check_pairs_on_random_scalars_with_different_data_in_every_lane(cg):
    """1000 checks in one call, at least 64 distinct accepting and 64 distinct rejecting ones among them, built from
    random 254-bit scalars: e([a]G, [b]H) e(-[ab]G, H) and, off by one, e([a]G, [b]H) e(-[ab + 1]G, H); every verdict
    against the construction, against the host pairing_check, and a sample against oracle/pairing.py."""
    import random

    from oracle import pairing as op
    rng = random.Random(0x3E11)
    h2 = cg.g2_generator()
    assert np.array_equal(h2, g2_words(op.G2_GEN))
    b, c = rng.randrange(1 << 253, bn.R), rng.randrange(1 << 253, bn.R)
    bh, ch = cg.g2_mul(h2, b), cg.g2_mul(h2, c)
    bh_py, ch_py = op.g2_mul(op.G2_GEN, b), op.g2_mul(op.G2_GEN, c)
    assert np.array_equal(bh, g2_words(bh_py)) and np.array_equal(ch, g2_words(ch_py))
    for q2, q2_py, ratio in ((h2, op.G2_GEN, b), (ch, ch_py, b * pow(c, -1, bn.R) % bn.R)):
        lad = scalar_ladder(rng, 160, ratio)
        checks = []                                               # (P, R, expected)
        for i, (a, P, S) in enumerate(lad):
            if i % 2 == 0:
                checks.append((P, g1_neg(S), True))
            else:
                checks.append((P, g1_neg(bn.g1_add(S, bn.G1_GEN)), False))    # -[ab/c + 1]G
        one = bn.g1_mul(bn.G1_GEN, ratio)
        checks += [(bn.G1_GEN, g1_neg(one), True), (bn.G1_GEN, one, False), (lad[0][1], lad[0][1], False),
                   (None, None, True), (None, g1_neg(lad[1][2]), False), (lad[2][1], None, False)]
        order = [rng.randrange(len(checks)) for _ in range(1000 - len(checks))] + list(range(len(checks)))
        rng.shuffle(order)
        p = np.stack([g1_words(checks[k][0]) for k in order])
        r = np.stack([g1_words(checks[k][1]) for k in order])
        acc = {p[i].tobytes() + r[i].tobytes() for i, k in enumerate(order) if checks[k][2]}
        rej = {p[i].tobytes() + r[i].tobytes() for i, k in enumerate(order) if not checks[k][2]}
        assert len(acc) >= 64 and len(rej) >= 64 and len(order) == 1000
        got = cg.pairing_check_pairs_dev(p, r, bh, q2)
        assert [bool(g) for g in got] == [checks[k][2] for k in order]
        host = {}
        for i, k in enumerate(order):
            if k not in host:
                host[k] = cg.pairing_check(np.stack([p[i], r[i]]), np.stack([bh, q2]))
            assert bool(got[i]) == host[k], (k, i)
        for k in (0, 1, len(lad), len(lad) + 2):                  # accepting, rejecting, (1, 2), P == R
            P, Rr, want = checks[k]
            assert op.pairing_product_is_one([(P, bh_py), (Rr, q2_py)]) == want, k


def test_pairing_check_pairs_on_boundary_relations_does_what_the_host_does(cg):
    """Q1 == Q2 with R = -P; Q2 = -Q1 with R = P; P == R; P = (1, 2); a G2 point at infinity (sixteen zero words: the null
    line table of k_pairing_check2) on either side and both; non-canonical G1 and G2 coordinates (x + p fits in 256
    bits).  The host pairing_check decides whether each is a verdict or an error, and the device entry point must do
    the same."""
    import random

    from oracle import pairing as op
    rng = random.Random(0x3E12)
    h2 = cg.g2_generator()
    b = rng.randrange(1 << 253, bn.R)
    bh = cg.g2_mul(h2, b)
    neg_bh = cg.g2_mul(bh, bn.R - 1)
    a = rng.randrange(1 << 253, bn.R)
    P = bn.g1_mul(bn.G1_GEN, a)
    abP = bn.g1_mul(bn.G1_GEN, a * b % bn.R)
    zero2 = np.zeros(16, np.uint64)
    w = g1_words
    cases = {
        "Q1 == Q2, R = -P": (w(P), w(g1_neg(P)), bh, bh, True),
        "Q1 == Q2, R = P": (w(P), w(P), bh, bh, False),
        "Q2 = -Q1, R = P": (w(P), w(P), bh, neg_bh, True),
        "Q2 = -Q1, R = -P": (w(P), w(g1_neg(P)), bh, neg_bh, False),
        "P == R": (w(P), w(P), bh, h2, False),
        "P = (1, 2)": (w(bn.G1_GEN), w(g1_neg(bn.g1_mul(bn.G1_GEN, b))), bh, h2, True),
        "P = R = (1, 2)": (w(bn.G1_GEN), w(bn.G1_GEN), bh, h2, False),
        "Q1 at infinity": (w(P), w(g1_neg(abP)), zero2, h2, None),
        "Q1 at infinity, R at infinity": (w(P), w(None), zero2, h2, None),
        "Q2 at infinity": (w(P), w(g1_neg(abP)), bh, zero2, None),
        "Q2 at infinity, P at infinity": (w(None), w(g1_neg(abP)), bh, zero2, None),
        "both Q at infinity": (w(P), w(g1_neg(abP)), zero2, zero2, None),
        "P.x + p": (plus_p(w(P), 0), w(g1_neg(abP)), bh, h2, None),
        "R.y + p": (w(P), plus_p(w(g1_neg(abP)), 1), bh, h2, None),
        "Q1.x.c0 + p": (w(P), w(g1_neg(abP)), plus_p(bh, 0), h2, None),
        "Q2.y.c1 + p": (w(P), w(g1_neg(abP)), bh, plus_p(h2, 3), None),
    }
    seen = {}
    for name, (p, r, q1, q2, want) in cases.items():
        host, dev = host_verdict(cg, p, r, q1, q2), dev_verdict(cg, p, r, q1, q2)
        seen[name] = (host, dev)
        if want is not None:
            assert host == want, (name, host)
    print("host / device:", seen)
    assert all(h == d for h, d in seen.values()), {k: v for k, v in seen.items() if v[0] != v[1]}
    # where the host gives a verdict for a point at infinity, a whole wave of such checks gives it in every lane
    for q1, q2 in ((zero2, h2), (bh, zero2), (zero2, zero2)):
        if host_verdict(cg, w(P), w(g1_neg(abP)), q1, q2) == "error":
            continue
        lad = scalar_ladder(rng, 70, b)
        p = np.stack([w(x[1]) for x in lad] + [w(None)])
        r = np.stack([w(g1_neg(x[2])) for x in lad] + [w(None)])
        got = cg.pairing_check_pairs_dev(p, r, q1, q2)
        assert [bool(g) for g in got] == [host_verdict(cg, p[i], r[i], q1, q2) for i in range(len(p))]
    assert op.pairing_product_is_one([(P, op.g2_mul(op.G2_GEN, b)), (g1_neg(abP), op.G2_GEN)])


def test_plonk_verify_each_on_degenerate_proofs_equals_plonk_verify(cg, tau):
    """Well-formed but degenerate proofs - a commitment at infinity, opening_proof == shifted_opening_proof, two wire
    commitments equal, all evaluations zero, evaluations r - 1 - drive k_verify_terms through infinity terms, equal
    partial sums in its LDS tree and zero sums; each verdict equals plonk_verify's.  A proof made for an all-zero
    public-input vector must be accepted."""
    srs = cg.srs_generate(tau, (1 << 7) + 3)
    h2 = cg.g2_generator()
    bh = cg.g2_mul(h2, tau)
    sc = bu.synthetic_circuit(7, 3, seed=71)
    # public inputs drawn as bits (free_class), so that some seed gives the all-zero vector
    sc.free_class = [bu.VAR_BOOL if k < sc.num_inputs else bu.VAR_UNIFORM for k in range(len(sc.free_vars))]
    pkh, vk = cg.plonk_preprocess(srs, sc.n, sc.num_inputs, sc.selectors_mont(), sc.sigma_mont())
    zero_w = None
    for seed in range(500, 700):
        try:
            wz, pz = sc.witness(seed)
        except RuntimeError:
            continue
        if not any(pz):
            zero_w = (wz, pz)
            break
    assert zero_w is not None
    w1, p1 = sc.witness(499)

    def prove(w, pubs, k):
        return cg.plonk_prove(pkh, sc.wires_mont(w), pubs_arr(pubs), bu.to_mont_array(bu.blinders(800 + k)), b"deg")
    base, zero_pr = prove(w1, p1, 0), prove(*zero_w, 1)
    rm1 = [int(x) for x in bu.to_mont_array([bn.R - 1]).reshape(-1)]

    def variant(edit):
        pr = copy.deepcopy(base)
        edit(pr)
        return pr

    def put(dst, src):
        for k in range(len(src)):
            dst[k] = src[k]

    def all_evals(pr, words):
        for i in range(5):
            put(pr.wires_evals[i], words)
        for i in range(4):
            put(pr.wire_sigma_evals[i], words)
        put(pr.perm_next_eval, words)
    variants = {
        "untouched": base,
        "zero public inputs": zero_pr,
        "wire commitment at infinity": variant(lambda pr: put(pr.wires_poly_comms[1], [0] * 8)),
        "permutation commitment at infinity": variant(lambda pr: put(pr.prod_perm_poly_comm, [0] * 8)),
        "opening proof at infinity": variant(lambda pr: put(pr.opening_proof, [0] * 8)),
        "both opening proofs at infinity": variant(lambda pr: (put(pr.opening_proof, [0] * 8),
                                                                put(pr.shifted_opening_proof, [0] * 8))),
        "opening == shifted opening": variant(lambda pr: put(pr.shifted_opening_proof, list(pr.opening_proof))),
        "two wire commitments equal": variant(lambda pr: put(pr.wires_poly_comms[3], list(pr.wires_poly_comms[2]))),
        "all evaluations zero": variant(lambda pr: all_evals(pr, [0] * 4)),
        "all evaluations r - 1": variant(lambda pr: all_evals(pr, rm1)),
        "all commitments at infinity": variant(lambda pr: [put(c, [0] * 8) for c in
                                                           list(pr.wires_poly_comms) + list(pr.split_quot_poly_comms) +
                                                           [pr.prod_perm_poly_comm, pr.opening_proof,
                                                            pr.shifted_opening_proof]]),
    }
    names = list(variants)
    proofs = [variants[n] for n in names]
    pubs = [pubs_arr(zero_w[1]) if n == "zero public inputs" else pubs_arr(p1) for n in names]
    got = cg.plonk_verify_each([vk] * len(names), h2, bh, pubs, proofs, [b"deg"] * len(names))
    host = [cg.plonk_verify(vk, h2, bh, pubs[i], proofs[i], b"deg") for i in range(len(names))]
    assert dict(zip(names, map(bool, got))) == dict(zip(names, host))
    assert got[names.index("untouched")] and got[names.index("zero public inputs")]
    # the zero-input proof is a proof for the zero vector only
    assert not cg.plonk_verify_each([vk], h2, bh, [pubs_arr(p1)], [zero_pr], [b"deg"])[0] or p1 == zero_w[1]
    cg.plonk_free_key(pkh)
    cg.srs_free(srs)
