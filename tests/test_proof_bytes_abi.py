"""The entry points that take proofs as note bytes exist in the library and in its Python layer, check their arguments
before they look for a device (stride < 769 or a null pointer: CAPGPU_ERR_INVALID_ARG), and refuse without a GPU - there
is no host fallback behind them.  (`-m "not gpu"`)"""
import ctypes
import os
import re

import numpy as np

from cap_amd import lib as cg
from cap_amd import proof as papi
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("capgpu_proof_decode_batch", "capgpu_proof_decode_batch_dev", "capgpu_proof_encode_batch",
       "capgpu_proof_encode_batch_dev", "capgpu_plonk_verify_block_bytes", "capgpu_plonk_verify_block_bytes_resident")


def test_entry_points_are_exported_and_wrapped():
    L = cg.load()
    for name in NEW:
        assert hasattr(L, name)
    assert callable(cg.proof_decode_batch) and callable(cg.proof_encode_batch) and callable(cg.plonk_verify_block_bytes)
    hdr = open(os.path.join(ROOT, "include", "capgpu.h")).read()
    assert re.search(r"#define CAPGPU_PROOF_BYTES 769\b", hdr) and cg.PROOF_BYTES == 769
    assert ctypes.sizeof(cg.Proof) == 1152
    cpp = open(os.path.join(ROOT, "include", "capgpu_proof.hpp")).read()
    for name in ("capgpu_proof_decode_batch", "capgpu_proof_encode_batch", "capgpu_plonk_verify_block_bytes"):
        assert name in cpp


def test_arguments_are_checked_before_a_device_is_looked_for():
    L = cg.load()
    sz = ctypes.c_size_t
    recs = np.zeros(2 * 769, np.uint8)
    u8p = recs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    arr, st, blk = (cg.Proof * 2)(), (ctypes.c_int * 2)(), ctypes.c_int(7)
    h2 = cg.g2_generator()
    bh = cg.g2_mul(h2, 12345)
    hs = (ctypes.c_uint64 * 2)(1, 1)
    dev = ctypes.c_void_p(0x1000)       # never dereferenced: every call below is refused first
    refused = (
        lambda: L.capgpu_proof_decode_batch(u8p, sz(768), sz(2), arr, st),
        lambda: L.capgpu_proof_decode_batch(None, sz(769), sz(2), arr, st),
        lambda: L.capgpu_proof_decode_batch(u8p, sz(769), sz(2), None, st),
        lambda: L.capgpu_proof_decode_batch(u8p, sz(769), sz(2), arr, None),
        lambda: L.capgpu_proof_decode_batch_dev(dev, sz(768), sz(2), dev, dev),
        lambda: L.capgpu_proof_decode_batch_dev(None, sz(769), sz(2), dev, dev),
        lambda: L.capgpu_proof_encode_batch(arr, sz(2), u8p, sz(768)),
        lambda: L.capgpu_proof_encode_batch(None, sz(2), u8p, sz(769)),
        lambda: L.capgpu_proof_encode_batch_dev(dev, sz(2), dev, sz(768)),
        lambda: L.capgpu_proof_encode_batch_dev(dev, sz(2), None, sz(769)),
        lambda: L.capgpu_plonk_verify_block_bytes(hs, cg._p(h2), cg._p(bh), None, sz(0), u8p, sz(768), None, None, sz(2),
                                                  ctypes.byref(blk), None, None),
        lambda: L.capgpu_plonk_verify_block_bytes(hs, cg._p(h2), cg._p(bh), None, sz(0), None, sz(769), None, None, sz(2),
                                                  ctypes.byref(blk), None, None),
        lambda: L.capgpu_plonk_verify_block_bytes_resident(hs, cg._p(h2), cg._p(bh), None, sz(0), dev, sz(768), None, None,
                                                           sz(2), ctypes.byref(blk), None, None),
    )
    for call in refused:
        assert call() == -1
    if H.gpu_present():
        return      # a test of this process may have initialised the library: the refusals below are the CPU runner's
    assert L.capgpu_proof_decode_batch(u8p, sz(769), sz(2), arr, st) == -6
    assert L.capgpu_proof_decode_batch(None, sz(769), sz(0), None, None) == -6
    assert L.capgpu_proof_encode_batch(arr, sz(2), u8p, sz(769)) == -6
    assert L.capgpu_plonk_verify_block_bytes(None, cg._p(h2), cg._p(bh), None, sz(0), None, sz(769), None, None, sz(0),
                                             ctypes.byref(blk), None, None) == -6
    assert b"not initialised" in L.capgpu_last_error()
    for call in (lambda: cg.proof_decode_batch(recs.tobytes()), lambda: cg.proof_encode_batch([cg.Proof()]),
                 lambda: cg.plonk_verify_block_bytes([], h2, bh, np.zeros((0, 4), np.uint64), b"", num_inputs=0)):
        try:
            call()
        except cg.CapGpuError as e:
            assert e.code == -6
        else:
            raise AssertionError("no refusal without a device")
    try:
        papi.txn_batch_verify([], h2, bh, np.zeros((0, 4), np.uint64), b"", num_inputs=0)
    except papi.TxnApiError as e:
        assert "not initialised" in str(e)
    else:
        raise AssertionError("txn_batch_verify over bytes did not reach the library")


def test_python_layer_refuses_short_buffers():
    for call in (lambda: cg.proof_decode_batch(b"\0" * 769, count=2), lambda: cg.proof_decode_batch(b"\0" * 769, stride=768),
                 lambda: cg.proof_encode_batch([cg.Proof()], stride=10),
                 lambda: papi._as_records([b"\0" * 768])):
        try:
            call()
        except ValueError:
            continue
        raise AssertionError("accepted")
    assert papi._as_records([b"\1" * 769, b"\2" * 769]) == b"\1" * 769 + b"\2" * 769
    assert papi._as_records([cg.Proof()]) is None and papi._as_records(b"ab") == b"ab"
