"""Proofs as the 769 note bytes a validator holds, on the device: capgpu_proof_decode_batch[_dev] against a loop of
capgpu_proof_deserialize word for word, capgpu_proof_encode_batch[_dev] against capgpu_proof_serialize byte for byte, the
corruption table of include/capgpu.h (status = 1 + the offset of the first malformed field, the struct all-ones words, the
neighbours untouched), and capgpu_plonk_verify_block_bytes / _bytes_resident against the host verifiers.  The environment
is test_gpu_verify_block.py's: n = 2^8 with 4 inputs and n = 2^7 with none, under a 2^8 + 3 SRS."""
import ctypes

import numpy as np
import pytest

from oracle import bn254 as bn
from tests.test_gpu_verify_block import Env, rows

pytestmark = pytest.mark.gpu

NB = 769
COUNTS = (1, 2, 4, 5, 20)      # 13 lanes per proof: proof 4 straddles a wavefront, proof 19 a 256-lane block
HEADS = ((0, 5), (200, 5), (432, 5), (600, 4))
POINTS = [8 + 32 * k for k in range(5)] + [168] + [208 + 32 * k for k in range(5)] + [368, 400]
SCALARS = [440 + 32 * k for k in range(5)] + [608 + 32 * k for k in range(4)] + [736]
TAG = 768


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
    """eight proofs of key 0: (Proof, public inputs, the proof's 769 bytes from capgpu_proof_serialize); never modified"""
    out = []
    for i in range(8):
        pr, pubs = env.prove(0, 900 + i, b"note")
        out.append((pr, pubs, env.cg.proof_serialize(pr)))
    assert all(len(p[2]) == NB for p in out)
    return out


def words(pr):
    return bytes(pr)


def place(recs, stride, lead=0, fill=0xA5):
    """the records `stride` apart behind `lead` bytes, in a buffer of exactly the bytes they span"""
    buf = bytearray([fill]) * (lead + (len(recs) - 1) * stride + NB)
    for i, r in enumerate(recs):
        buf[lead + i * stride:lead + i * stride + NB] = r
    return bytes(buf)


def patch(rec, off, data):
    return rec[:off] + bytes(data) + rec[off + len(data):]


def le32(v):
    return int(v).to_bytes(32, "little")


@pytest.mark.parametrize("stride", [769, 800])
@pytest.mark.parametrize("count", COUNTS)
def test_decode_equals_the_host_reader(cg, pool, count, stride):
    recs = [pool[i % 8][2] for i in range(count)]
    proofs, status = cg.proof_decode_batch(place(recs, stride), count=count, stride=stride)
    assert list(status) == [0] * count
    for i in range(count):
        want, used = cg.proof_deserialize(recs[i])
        assert used == NB and words(proofs[i]) == words(want), f"proof {i} differs from capgpu_proof_deserialize's"
        assert words(want) == words(pool[i % 8][0])


@pytest.mark.parametrize("shift", [1, 3])
def test_decode_dev_at_odd_addresses(cg, pool, shift):
    """device buffers, d_bytes advanced by 1 and by 3 bytes, both strides, the count that fills more than one block"""
    count = 20
    recs = [pool[i % 8][2] for i in range(count)]
    for stride in (769, 800):
        host = place(recs, stride, lead=shift)
        d_all = cg.DevBuf.from_numpy(np.frombuffer(host, dtype=np.uint8))
        d_pr, d_st = cg.proof_decode_batch(d_all.view(shift, len(host) - shift), count=count, stride=stride)
        status = d_st.to_numpy(np.int32, count)
        got = d_pr.to_numpy(np.uint8).tobytes()
        assert list(status) == [0] * count
        for i in range(count):
            assert got[1152 * i:1152 * (i + 1)] == words(pool[i % 8][0]), f"proof {i} (stride {stride})"
        assert d_all.to_numpy(np.uint8).tobytes() == host, "the records are never written"
        for b in (d_all, d_pr, d_st):
            b.free()


@pytest.mark.parametrize("count", COUNTS)
def test_encode_equals_proof_serialize(cg, pool, count):
    proofs = [pool[i % 8][0] for i in range(count)]
    want = [pool[i % 8][2] for i in range(count)]
    assert cg.proof_encode_batch(proofs) == b"".join(want)
    # a wider stride through the C ABI: the bytes between the caller's records stay what they were
    arr = (cg.Proof * count)()
    for i, p in enumerate(proofs):
        ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(p), ctypes.sizeof(cg.Proof))
    out = np.full((count - 1) * 800 + NB, 0xA5, np.uint8)
    cg.check(cg.load().capgpu_proof_encode_batch(arr, ctypes.c_size_t(count), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                                 ctypes.c_size_t(800)))
    assert out.tobytes() == place(want, 800)
    # device buffers, the records at an odd address
    d_pr = cg.DevBuf.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8))
    d_out = cg.DevBuf.from_numpy(np.full(3 + (count - 1) * 800 + NB, 0xA5, np.uint8))
    cg.check(cg.load().capgpu_proof_encode_batch_dev(d_pr.ptr, ctypes.c_size_t(count), ctypes.c_void_p(d_out.ptr.value + 3),
                                                     ctypes.c_size_t(800)))
    assert d_out.to_numpy(np.uint8).tobytes() == place(want, 800, lead=3)
    d_pr.free()
    d_out.free()


def test_device_only_round_trip_accepts(env, pool):
    """proof structs in device memory -> k_proof_encode -> capgpu_plonk_verify_block_bytes_resident: the bytes never visit
    the host, and the block they make is accepted"""
    cg = env.cg
    count = 5
    arr = (cg.Proof * count)()
    for i in range(count):
        ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(pool[i][0]), ctypes.sizeof(cg.Proof))
    d_pr = cg.DevBuf.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8))
    d_bytes = cg.proof_encode_batch(d_pr, count=count, stride=777)
    d_pub = cg.DevBuf.from_numpy(rows([pool[i][1] for i in range(count)], 4))
    ok, each, st = cg.plonk_verify_block_bytes([env.vkh[0]] * count, env.h2, env.bh, d_pub, d_bytes, [b"note"] * count,
                                               each=True, num_inputs=4, stride=777, status=True)
    assert ok and all(each) and list(st) == [0] * count
    for b in (d_pr, d_bytes, d_pub):
        b.free()


def corruption_table(good):
    """(name, corrupted record, byte offset the status must name) for one good record"""
    p_le, r_le = le32(bn.P), le32(bn.R)
    rows_ = []
    for off, n in HEADS:
        rows_.append((f"length prefix at {off}", patch(good, off, (4 if n == 5 else 5).to_bytes(8, "little")), off))
    rows_.append(("tag 1", patch(good, TAG, b"\x01"), TAG))
    rows_.append(("tag 2", patch(good, TAG, b"\x02"), TAG))
    for off in POINTS:
        x = good[off:off + 32]
        rows_.append((f"both flags at {off}", patch(good, off + 31, [x[31] | 0xC0]), off))
        rows_.append((f"infinity flag with x != 0 at {off}", patch(good, off + 31, [(x[31] & 0x3F) | 0x40]), off))
        rows_.append((f"x = p at {off}", patch(good, off, p_le), off))
        rows_.append((f"x = 4 at {off}", patch(good, off, le32(4)), off))
    for off in SCALARS:
        rows_.append((f"scalar r at {off}", patch(good, off, r_le), off))
    two = patch(patch(good, SCALARS[7], r_le), POINTS[9] + 31, [good[POINTS[9] + 31] | 0xC0])
    rows_.append(("two corruptions: the lower offset", two, POINTS[9]))
    rows_.append(("three corruptions: the lower offset", patch(two, 200, (4).to_bytes(8, "little")), 200))
    return rows_


def test_corruption_table(cg, pool):
    """one record corrupted at a time inside a block of five: its status names the field, its struct is all-ones words, the
    host reader refuses it too, and the four neighbours decode as before"""
    recs = [pool[i][2] for i in range(5)]
    tables = [corruption_table(r) for r in recs]
    assert len(tables[0]) == 4 + 2 + 13 * 4 + 10 + 2
    wrong = []
    for case in range(len(tables[0])):
        at = case % 5                                    # the corrupted record moves through the block
        name, rec, off = tables[at][case]
        with pytest.raises(cg.CapGpuError) as e:
            cg.proof_deserialize(rec)
        assert e.value.code == cg.CAPGPU_ERR_SERIALIZATION, name
        block = list(recs)
        block[at] = rec
        proofs, status = cg.proof_decode_batch(b"".join(block))
        if list(status) != [1 + off if i == at else 0 for i in range(5)]:
            wrong.append((name, at, list(status)))
        if words(proofs[at]) != b"\xff" * 1152:
            wrong.append((name, at, "not all-ones"))
        if any(words(proofs[i]) != words(pool[i][0]) for i in range(5) if i != at):
            wrong.append((name, at, "a neighbour changed"))
    assert wrong == []


def test_records_that_decode_but_must_not_verify(env, pool):
    """a flipped sign flag, an evaluation of r - 1 and the infinity encoding all decode (status 0): the verdict on each is
    capgpu_plonk_verify's on the host-deserialised proof"""
    cg = env.cg
    good = pool[0][2]
    recs = [good,
            patch(good, POINTS[1] + 31, [good[POINTS[1] + 31] ^ 0x80]),
            patch(good, SCALARS[2], le32(bn.R - 1)),
            patch(good, POINTS[6], b"\0" * 31 + b"\x40")]
    count = len(recs)
    pubs_l = [pool[0][1]] * count
    want = []
    for r in recs:
        pr, _ = cg.proof_deserialize(r)
        want.append(cg.plonk_verify(env.keys[0][1], env.h2, env.bh, pool[0][1], pr, b"note"))
    assert want[0] is True
    ok, each, st = cg.plonk_verify_block_bytes([env.vkh[0]] * count, env.h2, env.bh, rows(pubs_l, 4), b"".join(recs),
                                               [b"note"] * count, each=True, status=True)
    assert list(st) == [0] * count
    assert list(each) == want and ok == all(want)


@pytest.mark.parametrize("resident", [False, True])
def test_mixed_block_from_bytes(env, resident):
    """The nine proofs under two keys of test_mixed_block_flags_exactly_the_bad_proofs as note bytes, its corruptions
    re-expressed in bytes - an off-curve opening and a non-canonical evaluation cannot be written in a decodable record, so
    those two are undecodable - then two more undecodable records.  block_ok, each_ok and the statuses against the host's
    capgpu_plonk_batch_verify / capgpu_plonk_verify over the decodable proofs, 0 for the others."""
    cg = env.cg
    ks, pubs_l, recs, msgs = [], [], [], []
    for i in range(9):
        k = i % 2
        msg = b"n%d" % i if i % 3 else None
        pr, pubs = env.prove(k, 300 + i, msg)
        ks.append(k); pubs_l.append(pubs); recs.append(cg.proof_serialize(pr)); msgs.append(msg)
    handles = [env.vkh[k] for k in ks]

    def run(pubs_l, recs, msgs, each=True, stride=NB):
        pr = rows(pubs_l, 4)
        blob = place(recs, stride, fill=0)
        if not resident:
            return cg.plonk_verify_block_bytes(handles, env.h2, env.bh, pr, blob, msgs, each=each, num_inputs=4,
                                               stride=stride, status=each)
        d_b = cg.DevBuf.from_numpy(np.frombuffer(blob, dtype=np.uint8))
        d_p = cg.DevBuf.from_numpy(pr)
        try:
            return cg.plonk_verify_block_bytes(handles, env.h2, env.bh, d_p, d_b, msgs, each=each, num_inputs=4,
                                               stride=stride, status=each)
        finally:
            d_b.free()
            d_p.free()

    def check(pubs_l, recs, msgs, want_status, stride=NB):
        decoded = {}
        for i, r in enumerate(recs):
            try:
                decoded[i] = cg.proof_deserialize(r)[0]
            except cg.CapGpuError:
                assert want_status[i] != 0
        assert sorted(decoded) == [i for i in range(9) if want_status[i] == 0]
        idx = sorted(decoded)
        want_each = [i in decoded and cg.plonk_verify(env.keys[ks[i]][1], env.h2, env.bh, pubs_l[i], decoded[i], msgs[i])
                     for i in range(9)]
        want_block = len(idx) == 9 and cg.plonk_batch_verify([env.keys[ks[i]][1] for i in idx], env.h2, env.bh,
                                                             [pubs_l[i] for i in idx], [decoded[i] for i in idx],
                                                             [msgs[i] for i in idx])
        ok, each, st = run(pubs_l, recs, msgs, stride=stride)
        assert list(st) == want_status
        assert list(each) == want_each
        assert ok == want_block and ok == all(each)
        assert run(pubs_l, recs, msgs, each=False, stride=stride) == want_block      # each_ok_out = NULL
        return [i for i in range(9) if not each[i]]

    assert check(pubs_l, recs, msgs, [0] * 9) == []
    pubs_b, recs_b, msgs_b = [p.copy() for p in pubs_l], list(recs), list(msgs)
    pubs_b[4][1, 0] ^= 1                                                          # wrong public input
    recs_b[3] = patch(recs[3], POINTS[0], recs[5][POINTS[1]:POINTS[1] + 32])        # another point of the curve
    msgs_b[1], msgs_b[7] = msgs[7], msgs[1]                                       # swapped messages
    recs_b[8] = patch(recs[8], SCALARS[2], b"\xff" * 32)                            # non-canonical evaluation: no such record
    recs_b[0] = patch(recs[0], POINTS[11], le32(4))                                 # opening off the curve: no such record
    status = [1 + POINTS[11], 0, 0, 0, 0, 0, 0, 0, 1 + SCALARS[2]]
    assert check(pubs_b, recs_b, msgs_b, status, stride=800) == [0, 1, 3, 4, 7, 8]
    recs_b[2] = patch(recs[2], POINTS[7] + 31, [recs[2][POINTS[7] + 31] | 0xC0])     # both flags on a quotient part
    recs_b[6] = patch(recs[6], TAG, b"\x01")                                        # a plookup proof
    status[2], status[6] = 1 + POINTS[7], 1 + TAG
    assert check(pubs_b, recs_b, msgs_b, status) == [0, 1, 2, 3, 4, 6, 7, 8]
    # the reference's entry point over the same bytes
    from cap_amd import proof as papi
    if not resident:
        papi.txn_batch_verify(handles, env.h2, env.bh, rows(pubs_l, 4), recs, msgs, num_inputs=4)
        with pytest.raises(papi.TxnApiError):
            papi.txn_batch_verify(handles, env.h2, env.bh, rows(pubs_l, 4), recs_b, msgs, num_inputs=4)


def test_accounting_and_argument_errors(env, pool):
    cg = env.cg
    L = cg.load()
    count = 8
    blob = b"".join(p[2] for p in pool)
    pr = rows([p[1] for p in pool], 4)
    handles, msgs = [env.vkh[0]] * count, [b"note"] * count
    d_b, d_p = cg.DevBuf.from_numpy(np.frombuffer(blob, dtype=np.uint8)), cg.DevBuf.from_numpy(pr)
    for each in (False, True):
        for resident in (False, True):
            args = (d_p, d_b) if resident else (pr, blob)
            cg.plonk_verify_block_bytes(handles, env.h2, env.bh, *args, msgs, each=each, num_inputs=4)   # sizes the scratch
            s0, g0 = cg.verify_sync_stats(), cg.scratch_stats()
            got = cg.plonk_verify_block_bytes(handles, env.h2, env.bh, *args, msgs, each=each, num_inputs=4)
            s1, g1 = cg.verify_sync_stats(), cg.scratch_stats()
            assert (got[0] if each else got) is True
            assert (s1["block_calls"] - s0["block_calls"], s1["stream_waits"] - s0["stream_waits"]) == (1, 1)
            assert g1 == g0
    # an empty block
    assert cg.plonk_verify_block_bytes([], env.h2, env.bh, np.zeros((0, 4), np.uint64), b"", None, num_inputs=0) is True
    assert cg.proof_decode_batch(b"")[1].size == 0 and cg.proof_encode_batch([]) == b""
    # stride 768 and null pointers: CAPGPU_ERR_INVALID_ARG
    blk = ctypes.c_int(7)
    u8 = np.frombuffer(blob, dtype=np.uint8)
    u8p = u8.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    hs = (ctypes.c_uint64 * count)(*handles)
    h2, bh, pp, n, four = cg._p(env.h2), cg._p(env.bh), cg._p(pr.reshape(-1)), ctypes.c_size_t(count), ctypes.c_size_t(4)
    for stride, recs, out in ((768, u8p, ctypes.byref(blk)), (769, None, ctypes.byref(blk)), (769, u8p, None)):
        assert L.capgpu_plonk_verify_block_bytes(hs, h2, bh, pp, four, recs, ctypes.c_size_t(stride), None, None, n, out,
                                                 None, None) == -1
        assert L.capgpu_plonk_verify_block_bytes_resident(hs, h2, bh, d_p.ptr, four, d_b.ptr if recs else None,
                                                          ctypes.c_size_t(stride), None, None, n, out, None, None) == -1
    arr, st = (cg.Proof * count)(), (ctypes.c_int * count)()
    out = (ctypes.c_uint8 * (count * NB))()
    for bad in (lambda: L.capgpu_proof_decode_batch(u8p, ctypes.c_size_t(768), n, arr, st),
                lambda: L.capgpu_proof_decode_batch(None, ctypes.c_size_t(769), n, arr, st),
                lambda: L.capgpu_proof_decode_batch(u8p, ctypes.c_size_t(769), n, None, st),
                lambda: L.capgpu_proof_decode_batch(u8p, ctypes.c_size_t(769), n, arr, None),
                lambda: L.capgpu_proof_decode_batch_dev(d_b.ptr, ctypes.c_size_t(768), n, d_p.ptr, d_p.ptr),
                lambda: L.capgpu_proof_decode_batch_dev(None, ctypes.c_size_t(769), n, d_p.ptr, d_p.ptr),
                lambda: L.capgpu_proof_encode_batch(arr, n, out, ctypes.c_size_t(768)),
                lambda: L.capgpu_proof_encode_batch(None, n, out, ctypes.c_size_t(769)),
                lambda: L.capgpu_proof_encode_batch(arr, n, None, ctypes.c_size_t(769)),
                lambda: L.capgpu_proof_encode_batch_dev(d_p.ptr, n, d_b.ptr, ctypes.c_size_t(768)),
                lambda: L.capgpu_proof_encode_batch_dev(None, n, d_b.ptr, ctypes.c_size_t(769))):
        assert bad() == -1
        assert b"bad argument" in L.capgpu_last_error()
    d_b.free()
    d_p.free()
