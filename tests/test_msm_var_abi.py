"""The one-shot MSM entry points (capgpu_msm_g1_var*, capgpu_msm_var_plan) at the C boundary, on a machine without a GPU:
they are exported, check their arguments before they look for a device, refuse to compute without one, and the plan is
plain host arithmetic.  (`-m "not gpu"`)"""
import ctypes

import numpy as np
import pytest

from cap_amd import lib as cg
from tests import helpers as H

SYMBOLS = ("capgpu_msm_g1_var", "capgpu_msm_g1_var_batch", "capgpu_msm_g1_var_dev", "capgpu_msm_var_plan")
INVALID_ARG, NOT_INITIALISED = -1, -6


def test_symbols_are_exported():
    L = cg.load()
    for name in SYMBOLS:
        assert hasattr(L, name), name


def _args(n=4):
    bases = np.zeros((n, 8), np.uint64)
    scalars = np.zeros((n, 4), np.uint64)
    out = np.zeros(12, np.uint64)
    return bases, scalars, out


def test_bad_arguments_are_refused_before_the_device_is_looked_for():
    L = cg.load()
    bases, scalars, out = _args()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)            # noqa: E731
    n = ctypes.c_size_t(4)
    # capgpu_msm_g1_var: null pointers, a stride that is neither 64 nor 72
    assert L.capgpu_msm_g1_var(None, ctypes.c_size_t(64), 1, cg._p(scalars), n, cg._p(out)) == INVALID_ARG
    assert L.capgpu_msm_g1_var(vp(bases), ctypes.c_size_t(64), 1, None, n, cg._p(out)) == INVALID_ARG
    assert L.capgpu_msm_g1_var(vp(bases), ctypes.c_size_t(64), 1, cg._p(scalars), n, None) == INVALID_ARG
    assert L.capgpu_msm_g1_var(vp(bases), ctypes.c_size_t(96), 1, cg._p(scalars), n, cg._p(out)) == INVALID_ARG
    assert b"stride" in L.capgpu_last_error()
    # _batch: null arrays, a negative count, a null entry for an MSM that has points
    ns = (ctypes.c_size_t * 1)(4)
    bp = (cg.u64p * 1)(cg._p(bases))
    sp = (cg.u64p * 1)(cg._p(scalars))
    nullp = (cg.u64p * 1)()
    assert L.capgpu_msm_g1_var_batch(None, sp, ns, 1, cg._p(out)) == INVALID_ARG
    assert L.capgpu_msm_g1_var_batch(bp, sp, ns, -1, cg._p(out)) == INVALID_ARG
    assert L.capgpu_msm_g1_var_batch(bp, sp, ns, 1, None) == INVALID_ARG
    assert L.capgpu_msm_g1_var_batch(nullp, sp, ns, 1, cg._p(out)) == INVALID_ARG
    # _dev: the pointers are never dereferenced on the host, so host addresses serve as stand-ins
    assert L.capgpu_msm_g1_var_dev(None, vp(scalars), n, n, 1, 0, vp(out)) == INVALID_ARG
    assert L.capgpu_msm_g1_var_dev(vp(bases), None, n, n, 1, 0, vp(out)) == INVALID_ARG
    assert L.capgpu_msm_g1_var_dev(vp(bases), vp(scalars), n, n, 1, 0, None) == INVALID_ARG
    assert L.capgpu_msm_g1_var_dev(vp(bases), vp(scalars), n, n, -1, 0, vp(out)) == INVALID_ARG
    assert L.capgpu_msm_g1_var_dev(vp(bases), vp(scalars), ctypes.c_size_t(3), n, 2, 0, vp(out)) == INVALID_ARG
    # the plan
    buf = ctypes.create_string_buffer(256)
    assert L.capgpu_msm_var_plan(ctypes.c_size_t(100), 1, None, ctypes.c_size_t(256)) == INVALID_ARG
    assert L.capgpu_msm_var_plan(ctypes.c_size_t(100), -1, buf, ctypes.c_size_t(256)) == INVALID_ARG
    assert L.capgpu_msm_var_plan(ctypes.c_size_t(1 << 31), 1, buf, ctypes.c_size_t(256)) == INVALID_ARG


def test_valid_calls_refuse_without_a_device():
    if H.gpu_present():
        pytest.skip("GPU present: the refusal path is covered on the CPU-only runner")
    L = cg.load()
    bases, scalars, out = _args()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)            # noqa: E731
    n = ctypes.c_size_t(4)
    assert L.capgpu_msm_g1_var(vp(bases), ctypes.c_size_t(64), 1, cg._p(scalars), n, cg._p(out)) == NOT_INITIALISED
    ns = (ctypes.c_size_t * 1)(4)
    bp = (cg.u64p * 1)(cg._p(bases))
    sp = (cg.u64p * 1)(cg._p(scalars))
    assert L.capgpu_msm_g1_var_batch(bp, sp, ns, 1, cg._p(out)) == NOT_INITIALISED
    assert L.capgpu_msm_g1_var_dev(vp(bases), vp(scalars), n, n, 1, 0, vp(out)) == NOT_INITIALISED
    with pytest.raises(cg.CapGpuError) as e:
        cg.msm_g1_var(bases, scalars)
    assert e.value.code == NOT_INITIALISED


def test_plan_needs_no_device_and_reports_its_workspace():
    pl = cg.msm_var_plan(1 << 16)
    assert pl["path"] == "bucket" and pl["windows"] == (256 + pl["c"] - 1) // pl["c"] + (256 % pl["c"] == 0)
    assert pl["parts"] == 1 and pl["ranges"] == 1 and pl["tail"] == "horner-quad"
    assert pl["workspace_bytes"] > 64 * (1 << 16)              # at least the converted points
    # no window table: below the smallest one capgpu_srs_upload would build for these points (c = 13: 20 windows)
    assert pl["workspace_bytes"] < 20 * 64 * (1 << 16)
    assert cg.msm_var_plan(0)["path"] == "empty"
    big = cg.msm_var_plan(1 << 24)
    assert big["parts"] == 256 and big["ranges"] > 1            # long inputs run range after range
    assert cg.msm_var_plan(1000, 3)["workspace_bytes"] > cg.msm_var_plan(1000, 1)["workspace_bytes"]
