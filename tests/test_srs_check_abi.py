"""The parameter-audit entry points of include/capgpu.h (capgpu_srs_check, capgpu_plonk_key_check): struct layouts,
argument checks that need no device, and - like every compute entry point - a loud refusal without one.
(`-m "not gpu"`)"""
import ctypes

import numpy as np

from cap_amd import lib as cg


def _p(a):
    return a.ctypes.data_as(cg.u64p)


def test_report_layouts_match_the_header():
    S = cg.SrsReport
    assert ctypes.sizeof(S) == 176
    assert {name: getattr(S, name).offset for name, _ in S._fields_} == {
        "verdict": 0, "point_fault": 4, "first_bad_point": 8, "first_bad_link": 16, "points_checked": 24,
        "links_checked": 32, "pairing_checks": 40, "reserved": 44, "fold_a": 48, "fold_b": 112}
    K = cg.KeyReport
    assert ctypes.sizeof(K) == 16
    assert {name: getattr(K, name).offset for name, _ in K._fields_} == {
        "verdict": 0, "column": 4, "columns_differing": 8, "reserved": 12}
    assert cg.SRS_CHECK_LOCATE == 1


def test_report_text_names_the_fault():
    assert str(cg.SrsReport()) == "" and str(cg.KeyReport()) == ""
    assert str(cg.SrsReport(verdict=1, point_fault=2, first_bad_point=64)) == "SRS point 64 is not on the curve"
    assert str(cg.SrsReport(verdict=1, point_fault=1, first_bad_point=0)) == "SRS point 0 is the point at infinity"
    assert "first bad link: point 8 is not tau times point 7" in str(cg.SrsReport(verdict=2, first_bad_link=7))
    assert "first bad link" not in str(cg.SrsReport(verdict=2, first_bad_link=2**64 - 1))
    assert "first: sigma 1" in str(cg.KeyReport(verdict=2, column=14, columns_differing=2))
    assert "first: selector 12" in str(cg.KeyReport(verdict=2, column=12, columns_differing=1))


def test_malformed_arguments_are_refused_before_a_device_is_looked_for():
    """out == NULL, a NULL open key, flag bits other than LOCATE and a G2 input off the twist are CAPGPU_ERR_INVALID_ARG
    (-1) whether or not the library is initialised."""
    L = cg.load()
    h = cg.g2_generator()
    rep = cg.SrsReport()
    handle = ctypes.c_uint64(1)
    assert L.capgpu_srs_check(handle, _p(h), _p(h), None, ctypes.c_uint32(0), None) == -1
    assert b"capgpu_srs_check" in L.capgpu_last_error()
    assert L.capgpu_srs_check(handle, None, _p(h), None, ctypes.c_uint32(0), ctypes.byref(rep)) == -1
    assert L.capgpu_srs_check(handle, _p(h), None, None, ctypes.c_uint32(0), ctypes.byref(rep)) == -1
    for flags in (2, 3, 1 << 31):
        assert L.capgpu_srs_check(handle, _p(h), _p(h), None, ctypes.c_uint32(flags), ctypes.byref(rep)) == -1
        assert b"flag" in L.capgpu_last_error()
    off = h.copy()
    off[0] ^= np.uint64(1)
    assert L.capgpu_srs_check(handle, _p(off), _p(h), None, ctypes.c_uint32(0), ctypes.byref(rep)) == -1
    assert L.capgpu_srs_check(handle, _p(h), _p(off), None, ctypes.c_uint32(1), ctypes.byref(rep)) == -1
    assert L.capgpu_plonk_key_check(handle, None, None) == -1
    assert b"capgpu_plonk_key_check" in L.capgpu_last_error()


def test_both_calls_refuse_without_a_device():
    from tests import helpers as H
    L = cg.load()
    if H.gpu_present():
        return  # the refusal path belongs to the CPU-only runner; the GPU suite exercises the calls themselves
    h = cg.g2_generator()
    srs_rep, key_rep, vk = cg.SrsReport(), cg.KeyReport(), cg.VerifyingKey()
    seed = (ctypes.c_uint8 * 32)()
    for flags in (0, 1):
        for s in (None, seed):
            assert L.capgpu_srs_check(ctypes.c_uint64(1), _p(h), _p(h), s, ctypes.c_uint32(flags),
                                      ctypes.byref(srs_rep)) == -6
            assert b"not initialised" in L.capgpu_last_error()
    for v in (None, ctypes.byref(vk)):
        assert L.capgpu_plonk_key_check(ctypes.c_uint64(1), v, ctypes.byref(key_rep)) == -6
        assert b"not initialised" in L.capgpu_last_error()
    for call in (lambda: cg.srs_check(1, h, h), lambda: cg.plonk_key_check(1)):
        try:
            call()
        except cg.CapGpuError as e:
            assert e.code == -6
        else:
            raise AssertionError("the wrapper returned without a device")
