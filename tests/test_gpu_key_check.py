"""capgpu_plonk_key_check on the device: does a resident proving key commit to a verifying key?  The n = 16 and n = 64
synthetic circuits of the PLONK tests: a fresh key against its own verifying key (passed, and as NULL), the same key after
a serialize -> deserialize round trip (the case the call exists for: the blob's verifying key is taken on faith), verifying
keys with one commitment replaced, the verifying key of a circuit that differs in one selector cell, altered shapes."""
import numpy as np
import pytest

from cap_amd import bench_utils as bu
from cap_amd import parameters as prm
from cap_amd import proof as capproof
from oracle import capref as cr

pytestmark = pytest.mark.gpu


def report(rep):
    return (rep.verdict, rep.column, rep.columns_differing)


def clone(vk):
    return type(vk).from_buffer_copy(bytes(vk))


@pytest.fixture(scope="module", params=[4, 6], ids=["n16", "n64"])
def made(cg, tau, request):
    log_n = request.param
    sc = bu.synthetic_circuit(log_n, 3, seed=70 + log_n)
    h = cg.srs_generate(tau, sc.n + 3)
    pk, vk = cg.plonk_preprocess(h, sc.n, 3, sc.selectors_mont(), sc.sigma_mont())
    yield sc, h, pk, vk
    cg.plonk_free_key(pk)
    cg.srs_free(h)


def test_fresh_key_commits_to_its_own_verifying_key(cg, made):
    sc, h, pk, vk = made
    assert report(cg.plonk_key_check(pk, vk)) == (0, 0, 0)
    assert report(cg.plonk_key_check(pk)) == (0, 0, 0)
    assert report(cg.plonk_key_check(pk, clone(vk))) == (0, 0, 0)
    with pytest.raises(cg.CapGpuError) as e:
        cg.plonk_key_check(0xDEAD0000)
    assert e.value.code == -4


def test_key_after_a_blob_round_trip(cg, tau, made):
    sc, h, pk, vk = made
    g2 = cg.g2_generator()
    blob = cg.plonk_key_serialize(pk, g2, cg.g2_mul(g2, tau))
    srs2, pk2, vk2, _h, _bh, used = cg.plonk_key_deserialize(blob)
    try:
        assert used == len(blob) and bytes(vk2) == bytes(vk)
        assert report(cg.plonk_key_check(pk2)) == (0, 0, 0)
        assert report(cg.plonk_key_check(pk2, vk)) == (0, 0, 0)
    finally:
        cg.plonk_free_key(pk2)
        cg.srs_free(srs2)
    key, used = prm.deserialize_proving_key(blob, check=True)      # the host mirror's optional argument
    cg.plonk_free_key(key.handle)
    cg.srs_free(key.srs.handle)


def test_blob_whose_polynomials_do_not_match_its_commitments(cg, tau, made):
    """One byte of a selector polynomial's first coefficient changed in the blob: the key loads - its verifying key is the
    blob's - and the check names the column; the host mirror raises."""
    sc, h, pk, vk = made
    g2 = cg.g2_generator()
    blob = bytearray(cg.plonk_key_serialize(pk, g2, cg.g2_mul(g2, tau)))
    # ProvingKey blob: sigma polynomials (u64 count, then per polynomial u64 length + coefficients), then the selectors
    at = 8
    for _ in range(5):
        at += 8 + 32 * int.from_bytes(blob[at:at + 8], "little")
    assert int.from_bytes(blob[at:at + 8], "little") == 13, "selector count where the layout puts it"
    assert int.from_bytes(blob[at + 8:at + 16], "little") > 0, "the first selector is not the zero polynomial"
    at += 8 + 8                                                    # the count, the first selector's length
    blob[at] ^= 1
    srs2, pk2, vk2, *_ = cg.plonk_key_deserialize(bytes(blob))
    try:
        assert bytes(vk2) == bytes(vk)
        assert report(cg.plonk_key_check(pk2)) == (2, 0, 1)
    finally:
        cg.plonk_free_key(pk2)
        cg.srs_free(srs2)
    with pytest.raises(capproof.TxnApiError) as e:
        prm.deserialize_proving_key(bytes(blob), check=True)
    assert "selector 0" in str(e.value)
    key, _ = prm.deserialize_proving_key(bytes(blob))                # the default checks nothing, as before
    cg.plonk_free_key(key.handle)
    cg.srs_free(key.srs.handle)


def test_one_commitment_replaced(cg, made):
    sc, h, pk, vk = made
    other = cr.g1_fixed_base_batch(cr.ints_to_array([0xBEEF]))[0]
    for col in (0, 7, 12):
        bad = clone(vk)
        for w in range(8):
            bad.selector_comms[col][w] = int(other[w])
        assert report(cg.plonk_key_check(pk, bad)) == (2, col, 1)
    for col in (0, 4):
        bad = clone(vk)
        for w in range(8):
            bad.sigma_comms[col][w] = int(other[w])
        assert report(cg.plonk_key_check(pk, bad)) == (2, 13 + col, 1)
    bad = clone(vk)
    for w in range(8):
        bad.selector_comms[5][w] = int(other[w])
        bad.sigma_comms[2][w] = int(other[w])
    assert report(cg.plonk_key_check(pk, bad)) == (2, 5, 2)


def test_verifying_key_of_a_circuit_that_differs_in_one_selector_cell(cg, made):
    sc, h, pk, vk = made
    for col, row in ((3, 5), (11, sc.n - 1)):
        sel = sc.selectors_mont().copy()
        sel[col, row, 0] ^= np.uint64(1)
        pk2, vk2 = cg.plonk_preprocess(h, sc.n, 3, sel, sc.sigma_mont())
        try:
            assert report(cg.plonk_key_check(pk, vk2)) == (2, col, 1)
            assert report(cg.plonk_key_check(pk2, vk)) == (2, col, 1)
            assert report(cg.plonk_key_check(pk2, vk2)) == (0, 0, 0)
        finally:
            cg.plonk_free_key(pk2)


def test_altered_shape(cg, made):
    sc, h, pk, vk = made
    for field, value in (("num_inputs", 4), ("num_inputs", 0), ("domain_size", 2 * sc.n), ("domain_size", sc.n // 2)):
        bad = clone(vk)
        setattr(bad, field, value)
        assert report(cg.plonk_key_check(pk, bad)) == (1, 0, 0), field
    bad = clone(vk)
    bad.k[2][0] ^= 1
    assert report(cg.plonk_key_check(pk, bad)) == (1, 0, 0)
