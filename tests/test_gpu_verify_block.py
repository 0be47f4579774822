"""The block verifier (capgpu_plonk_verify_block_dev / _resident over capgpu_plonk_vk_upload keys): transcripts, scalars,
weights, the fold, two one-shot MSMs and the pairing check on the device with one host wait.  block_ok is
capgpu_plonk_batch_verify's predicate, each_ok[i] capgpu_plonk_verify's verdict, and block_ok == all(each_ok).
n = 2^8 and 2^7 synthetic circuits under a 2^8 + 3 SRS, as test_gpu_verify_each.py uses."""
import copy
import ctypes

import numpy as np
import pytest

from cap_amd import bench_utils as bu

pytestmark = pytest.mark.gpu

MSG_LENS = (0, 1, 135, 136, 137, 300)   # the padded message around the sponge's 136-byte rate


def pubs_arr(pubs):
    return bu.to_mont_array(pubs) if pubs else np.zeros((0, 4), np.uint64)


def rows(pubs_l, width):
    """plonk_prove_multi's layout: one row of `width` per proof, a shorter vector in the first of its row"""
    out = np.zeros((len(pubs_l), max(width, 1), 4), np.uint64)
    for i, p in enumerate(pubs_l):
        out[i, :p.shape[0]] = p
    return out[:, :width]


class Env:
    """session-wide: SRS, two circuits (n = 2^8 with 4 inputs, n = 2^7 with none), their keys and uploaded handles"""

    def __init__(self, cg, tau):
        self.cg = cg
        self.srs = cg.srs_generate(tau, (1 << 8) + 3)
        self.h2 = cg.g2_generator()
        self.bh = cg.g2_mul(self.h2, tau)
        self.circuits = [bu.synthetic_circuit(8, 4, seed=61), bu.synthetic_circuit(7, 0, seed=62)]
        self.keys = [cg.plonk_preprocess(self.srs, sc.n, sc.num_inputs, sc.selectors_mont(), sc.sigma_mont())
                     for sc in self.circuits]
        self.vkh = [cg.plonk_vk_upload(k[1]) for k in self.keys]

    def prove(self, k, seed, msg):
        sc = self.circuits[k]
        w, pubs = sc.witness(seed)
        pr = self.cg.plonk_prove(self.keys[k][0], sc.wires_mont(w), pubs_arr(pubs), bu.to_mont_array(bu.blinders(seed + 100)),
                                 msg)
        return pr, pubs_arr(pubs)

    def host(self, ks, pubs_l, proofs, msgs, vks=None):
        """(capgpu_plonk_batch_verify, [capgpu_plonk_verify]) on the host"""
        cg = self.cg
        vks = vks or [self.keys[k][1] for k in ks]
        each = [cg.plonk_verify(vks[i], self.h2, self.bh, pubs_l[i], proofs[i], msgs[i]) for i in range(len(proofs))]
        return cg.plonk_batch_verify(vks, self.h2, self.bh, pubs_l, proofs, msgs), each

    def block(self, handles, pubs_l, proofs, msgs, width=4, each=True, resident=False):
        cg = self.cg
        pr = rows(pubs_l, width)
        if not resident:
            return cg.plonk_verify_block(handles, self.h2, self.bh, pr, proofs, msgs, each=each, num_inputs=width)
        arr = (cg.Proof * len(proofs))()
        for i, p in enumerate(proofs):
            ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(p), ctypes.sizeof(cg.Proof))
        d_pr = cg.DevBuf(ctypes.sizeof(arr))
        cg.check(cg.load().capgpu_memcpy_h2d(d_pr.ptr, ctypes.byref(arr), ctypes.c_size_t(ctypes.sizeof(arr))))
        d_pub = cg.DevBuf.from_numpy(pr if pr.size else np.zeros(4, np.uint64))
        try:
            return cg.plonk_verify_block(handles, self.h2, self.bh, d_pub, d_pr, msgs, each=each, num_inputs=width)
        finally:
            d_pr.free()
            d_pub.free()


@pytest.fixture(scope="module")
def env(cg, tau):
    e = Env(cg, tau)
    yield e
    for h in e.vkh:
        cg.plonk_vk_release(h)
    for pkh, _ in e.keys:
        cg.plonk_free_key(pkh)
    cg.srs_free(e.srs)


@pytest.fixture(scope="module")
def pool(env):
    """eight proofs of key 0 with their public inputs, shared (never modified) by the count tests"""
    return [env.prove(0, 700 + i, b"blk") for i in range(8)]


@pytest.mark.parametrize("resident", [False, True])
def test_mixed_block_flags_exactly_the_bad_proofs(env, resident):
    """The nine proofs under two keys of test_plonk_verify_each_flags_exactly_the_bad_proofs with its corruptions: a wrong
    public input, another curve point in a commitment, swapped messages, a non-canonical evaluation, an off-curve opening,
    and a wrong key of the same shape."""
    cg = env.cg
    ks, pubs_l, proofs, msgs = [], [], [], []
    for i in range(9):
        k = i % 2
        msg = b"n%d" % i if i % 3 else None
        pr, pubs = env.prove(k, 300 + i, msg)
        ks.append(k); pubs_l.append(pubs); proofs.append(pr); msgs.append(msg)
    handles = [env.vkh[k] for k in ks]

    def check(handles, ks, pubs_l, proofs, msgs, vks=None):
        want_block, want_each = env.host(ks, pubs_l, proofs, msgs, vks)
        got_block, got_each = env.block(handles, pubs_l, proofs, msgs, resident=resident)
        assert list(got_each) == want_each
        assert got_block == want_block and got_block == all(got_each)
        assert env.block(handles, pubs_l, proofs, msgs, each=False, resident=resident) == want_block
        return [i for i, ok in enumerate(got_each) if not ok]

    assert check(handles, ks, pubs_l, proofs, msgs) == []
    pubs_b, proofs_b, msgs_b = [p.copy() for p in pubs_l], [copy.deepcopy(p) for p in proofs], list(msgs)
    pubs_b[4][1, 0] ^= 1                                                    # wrong public input
    for k in range(8):
        proofs_b[3].wires_poly_comms[0][k] = proofs[5].wires_poly_comms[1][k]   # another point of the curve
    msgs_b[1], msgs_b[7] = msgs[7], msgs[1]                                 # swapped messages
    proofs_b[8].wires_evals[2][:] = [0xFFFFFFFFFFFFFFFF] * 4                # non-canonical evaluation (>= r)
    proofs_b[0].opening_proof[4] ^= 1                                       # off the curve
    assert check(handles, ks, pubs_b, proofs_b, msgs_b) == [0, 1, 3, 4, 7, 8]
    # a proof under the wrong key: a third key of key 0's shape
    twin = bu.synthetic_circuit(8, 4, seed=63)
    tw_pk, tw_vk = cg.plonk_preprocess(env.srs, twin.n, twin.num_inputs, twin.selectors_mont(), twin.sigma_mont())
    tw_h = cg.plonk_vk_upload(tw_vk)
    vk0 = env.keys[0][1]
    assert check([env.vkh[0], tw_h, env.vkh[0]], None, [pubs_l[0], pubs_l[2], pubs_l[4]], [proofs[0], proofs[2], proofs[4]],
                 [msgs[0], msgs[2], msgs[4]], vks=[vk0, tw_vk, vk0]) == [1]
    cg.plonk_vk_release(tw_h)
    cg.plonk_free_key(tw_pk)


@pytest.mark.parametrize("count", [1, 2, 64, 65])
def test_counts_around_the_wave_boundary(env, pool, count):
    """clean blocks accept; one proof corrupted at the first, a middle and the last position rejects with exactly that
    index flagged (64 and 65: the wave boundary of the weight and fold kernels)"""
    proofs = [pool[i % 8][0] for i in range(count)]
    pubs_l = [pool[i % 8][1] for i in range(count)]
    handles = [env.vkh[0]] * count
    msgs = [b"blk"] * count
    ok, each = env.block(handles, pubs_l, proofs, msgs)
    assert ok and all(each) and len(each) == count
    for pos in sorted({0, count // 2, count - 1}):
        bad = list(proofs)
        bad[pos] = copy.deepcopy(proofs[pos])
        bad[pos].perm_next_eval[0] ^= 1
        ok, each = env.block(handles, pubs_l, bad, msgs)
        assert not ok and [i for i in range(count) if not each[i]] == [pos]
        assert not env.block(handles, pubs_l, bad, msgs, each=False)


def test_many_public_inputs_wrap_the_lane_stride(env):
    """254 public inputs at n = 2^8 - the largest count bench_utils.synthetic_circuit accepts there (it wants
    n > num_inputs + 1) - so that the lanes of PI(zeta) take up to four inputs each; a key without inputs in the same block"""
    cg = env.cg
    sc = bu.synthetic_circuit(8, 254, seed=64)
    pkh, vk = cg.plonk_preprocess(env.srs, sc.n, sc.num_inputs, sc.selectors_mont(), sc.sigma_mont())
    vkh = cg.plonk_vk_upload(vk)
    w, pubs = sc.witness(11)
    big = cg.plonk_prove(pkh, sc.wires_mont(w), pubs_arr(pubs), bu.to_mont_array(bu.blinders(12)), b"wide")
    small, no_pubs = env.prove(1, 13, b"none")
    handles, pubs_l, proofs, msgs = [vkh, env.vkh[1], vkh], [pubs_arr(pubs), no_pubs, pubs_arr(pubs)], [big, small, big], \
        [b"wide", b"none", b"wide"]
    vks = [vk, env.keys[1][1], vk]
    assert env.host(None, pubs_l, proofs, msgs, vks) == (True, [True] * 3)
    assert env.block(handles, pubs_l, proofs, msgs, width=254)[0]
    for j in (0, 63, 64, 200, 253):                     # one input wrong, in every lane round
        pb = [p.copy() for p in pubs_l]
        pb[2][j, 0] ^= 1
        want = env.host(None, pb, proofs, msgs, vks)
        ok, each = env.block(handles, pb, proofs, msgs, width=254)
        assert (ok, list(each)) == want == (False, [True, True, False])
    cg.plonk_vk_release(vkh)
    cg.plonk_free_key(pkh)


def test_boundary_messages_and_an_infinity_commitment(env):
    """one proof per ext_msg length 0, 1, 135, 136, 137, 300 in one block; then a proof whose commitment is the all-zero
    point: the verdict is the host's, whatever that is"""
    ks, pubs_l, proofs, msgs = [], [], [], []
    for i, ln in enumerate(MSG_LENS):
        msg = bytes((7 * j + i) & 0xFF for j in range(ln))
        pr, pubs = env.prove(i % 2, 500 + i, msg or None)
        ks.append(i % 2); pubs_l.append(pubs); proofs.append(pr); msgs.append(msg or None)
    handles = [env.vkh[k] for k in ks]
    assert env.host(ks, pubs_l, proofs, msgs) == (True, [True] * 6)
    ok, each = env.block(handles, pubs_l, proofs, msgs)
    assert ok and all(each)
    shifted = msgs[1:] + msgs[:1]                       # every proof under another length's message
    want = env.host(ks, pubs_l, proofs, shifted)
    ok, each = env.block(handles, pubs_l, proofs, shifted)
    assert (ok, list(each)) == want and not ok
    inf = [copy.deepcopy(p) for p in proofs[:2]]
    for k in range(8):
        inf[0].wires_poly_comms[1][k] = 0
        inf[1].prod_perm_poly_comm[k] = 0
    want = env.host(ks[:2], pubs_l[:2], inf, msgs[:2])
    ok, each = env.block(handles[:2], pubs_l[:2], inf, msgs[:2])
    assert (ok, list(each)) == want and ok == all(each)


def test_argument_and_lifetime_rules(env, pool):
    cg = env.cg
    pr, pubs = pool[0]
    # a malformed key at upload names the field
    for edit, name in ((lambda v: v.selector_comms[3].__setitem__(4, v.selector_comms[3][4] ^ 1), b"selector_comms[3]"),
                       (lambda v: v.sigma_comms[2].__setitem__(0, v.sigma_comms[2][0] ^ 1), b"sigma_comms[2]"),
                       (lambda v: [v.k[1].__setitem__(j, 0xFFFFFFFFFFFFFFFF) for j in range(4)], b"k[1]"),
                       (lambda v: setattr(v, "domain_size", 200), b"domain_size")):
        vk = copy.deepcopy(env.keys[0][1])
        edit(vk)
        with pytest.raises(cg.CapGpuError):
            cg.plonk_vk_upload(vk)
        assert name in cg.load().capgpu_last_error()
    # unknown and released handles
    h = cg.plonk_vk_upload(env.keys[0][1])
    assert env.block([h], [pubs], [pr], [b"blk"]) == (True, [True])
    cg.plonk_vk_release(h)
    blk = ctypes.c_int(7)
    p = rows([pubs], 4).reshape(-1)
    for bad in (h, 0xDEADBEEF):
        rc = cg.load().capgpu_plonk_verify_block_dev((ctypes.c_uint64 * 1)(bad), cg._p(env.h2), cg._p(env.bh), cg._p(p),
                                                     ctypes.c_size_t(4), ctypes.byref(pr), None, None, ctypes.c_size_t(1),
                                                     ctypes.byref(blk), None)
        assert rc == -1 and blk.value == 0
    assert cg.load().capgpu_plonk_vk_release(ctypes.c_uint64(h)) == -1
    # release followed by a fresh upload works
    h2 = cg.plonk_vk_upload(env.keys[0][1])
    assert h2 != h and env.block([h2], [pubs], [pr], [b"blk"]) == (True, [True])
    cg.plonk_vk_release(h2)
    # an empty block behaves as the host batch verifier; G2 off the twist is an error in both
    assert cg.plonk_batch_verify([], env.h2, env.bh, [], [], []) is True
    assert cg.plonk_verify_block([], env.h2, env.bh, np.zeros((0, 4), np.uint64), [], None, num_inputs=0) is True
    off = env.bh.copy()
    off[0] ^= np.uint64(1)
    with pytest.raises(cg.CapGpuError):
        cg.plonk_verify_block([env.vkh[0]], env.h2, off, rows([pubs], 4), [pr], [b"blk"])
    # rows narrower than a key's public inputs
    with pytest.raises(cg.CapGpuError):
        cg.plonk_verify_block([env.vkh[0]], env.h2, env.bh, rows([pubs], 4)[:, :3], [pr], [b"blk"], num_inputs=3)


def test_one_wait_per_call_and_no_scratch_growth_on_a_repeat(env, pool):
    cg = env.cg
    proofs, pubs_l = [p[0] for p in pool], [p[1] for p in pool]
    handles, msgs = [env.vkh[0]] * 8, [b"blk"] * 8
    for each in (False, True):
        for resident in (False, True):
            env.block(handles, pubs_l, proofs, msgs, each=each, resident=resident)          # sizes the scratch
            s0, g0 = cg.verify_sync_stats(), cg.scratch_stats()
            got = env.block(handles, pubs_l, proofs, msgs, each=each, resident=resident)
            s1, g1 = cg.verify_sync_stats(), cg.scratch_stats()
            assert (got[0] if each else got) is True
            assert (s1["block_calls"] - s0["block_calls"], s1["stream_waits"] - s0["stream_waits"]) == (1, 1)
            assert g1 == g0
