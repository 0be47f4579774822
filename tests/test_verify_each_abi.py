"""The per-proof device verifier's entry points exist in the library and the Rust bindings, and refuse without a GPU
(no host fallback).  (`-m "not gpu"`)"""
import ctypes

import numpy as np
import pytest

from cap_amd import lib as cg
from tests import helpers as H

NEW = ("capgpu_pairing_check_pairs_dev", "capgpu_plonk_verify_each_dev")


def test_entry_points_are_exported():
    L = cg.load()
    for name in NEW:
        assert hasattr(L, name)
    assert callable(cg.pairing_check_pairs_dev) and callable(cg.plonk_verify_each)


def test_no_host_fallback_without_a_device():
    if H.gpu_present():
        pytest.skip("GPU present: the refusal path is covered on the CPU-only runner")
    L = cg.load()
    h2 = cg.g2_generator()
    bh = cg.g2_mul(h2, 12345)
    p = np.zeros((2, 8), np.uint64)
    ok = np.zeros(2, np.int32)
    intp = ctypes.POINTER(ctypes.c_int)
    rc = L.capgpu_pairing_check_pairs_dev(p.ctypes.data_as(cg.u64p), p.ctypes.data_as(cg.u64p), ctypes.c_size_t(2),
                                          bh.ctypes.data_as(cg.u64p), h2.ctypes.data_as(cg.u64p),
                                          ok.ctypes.data_as(intp))
    assert rc == -6
    rc = L.capgpu_plonk_verify_each_dev(None, h2.ctypes.data_as(cg.u64p), bh.ctypes.data_as(cg.u64p), None, None, None,
                                        None, None, ctypes.c_size_t(0), ok.ctypes.data_as(intp))
    assert rc == -6
    with pytest.raises(cg.CapGpuError):
        cg.pairing_check_pairs_dev(p, p, bh, h2)
    with pytest.raises(cg.CapGpuError):
        cg.plonk_verify_each([], h2, bh, [], [], [])
