"""The witness solver's entry points (capgpu_plonk_key_set_given, capgpu_plonk_key_solver_info, capgpu_plonk_solve_vars[_dev])
at the C boundary, on a machine without a GPU: they are exported, the two structs have the header's layout, pointer errors
come before the device is looked for and CAPGPU_ERR_NOT_INITIALISED after them, and the mirrors name the calls.
(`-m "not gpu"`)"""
import ctypes
import os

import numpy as np
import pytest

from cap_amd import lib as cg
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("capgpu_plonk_key_set_given", "capgpu_plonk_key_solver_info", "capgpu_plonk_solve_vars",
           "capgpu_plonk_solve_vars_dev")
INVALID_ARG, NOT_INITIALISED = -1, -6
u32p = ctypes.POINTER(ctypes.c_uint32)


def test_symbols_are_exported():
    L = cg.load()
    for name in SYMBOLS:
        assert hasattr(L, name), name


def test_struct_layouts_match_the_header():
    assert ctypes.sizeof(cg.SolverInfo) == 48 and ctypes.sizeof(cg.SolveStatus) == 16
    assert [f[0] for f in cg.SolverInfo._fields_] == ["num_given", "num_defined", "levels", "widest_level", "inv_rows", "root_rows"]
    assert cg.SolveStatus.kind.offset == 0 and cg.SolveStatus.reserved.offset == 4 and cg.SolveStatus.row.offset == 8
    hdr = open(os.path.join(ROOT, "include", "capgpu.h")).read()
    assert "} capgpu_solver_info; /* 48 bytes */" in hdr and "} capgpu_solve_status; /* 16 bytes */" in hdr


def _solve_args():
    return dict(g=np.zeros(8, np.uint64), v=np.zeros(64, np.uint64), st=(cg.SolveStatus * 2)())


def _solve(L, name, a, count=2, **null):
    ptr = (lambda k: a[k].ctypes.data_as(ctypes.c_void_p)) if name.endswith("_dev") else (lambda k: cg._p(a[k]))
    return getattr(L, name)(ctypes.c_uint64(1), count, None if null.get("g") else ptr("g"), None if null.get("v") else ptr("v"),
                            None if null.get("st") else a["st"])


@pytest.mark.parametrize("name", SYMBOLS[2:])
def test_bad_solve_arguments_are_refused_before_the_device_is_looked_for(name):
    L = cg.load()
    a = _solve_args()
    for missing in ("g", "v", "st"):
        assert _solve(L, name, a, **{missing: True}) == INVALID_ARG, missing
        assert b"capgpu_plonk_solve_vars: bad argument" in L.capgpu_last_error()
    assert _solve(L, name, a, count=-1) == INVALID_ARG


def test_bad_set_up_arguments_are_refused_before_the_device_is_looked_for():
    L = cg.load()
    info = cg.SolverInfo()
    assert L.capgpu_plonk_key_set_given(ctypes.c_uint64(1), None, ctypes.c_size_t(3), ctypes.byref(info)) == INVALID_ARG
    assert b"capgpu_plonk_key_set_given: bad argument" in L.capgpu_last_error()
    assert L.capgpu_plonk_key_solver_info(ctypes.c_uint64(1), None) == INVALID_ARG
    assert b"capgpu_plonk_key_solver_info: bad argument" in L.capgpu_last_error()


def test_valid_calls_refuse_without_a_device():
    if H.gpu_present():
        pytest.skip("GPU present: the refusal path is covered on the CPU-only runner")
    L = cg.load()
    a = _solve_args()
    ids = np.arange(3, dtype=np.uint32)
    info = cg.SolverInfo()
    calls = [lambda: _solve(L, "capgpu_plonk_solve_vars", a), lambda: _solve(L, "capgpu_plonk_solve_vars_dev", a),
             lambda: _solve(L, "capgpu_plonk_solve_vars", a, count=0, g=True, v=True, st=True),
             lambda: L.capgpu_plonk_key_set_given(ctypes.c_uint64(1), ids.ctypes.data_as(u32p), ctypes.c_size_t(3), None),
             lambda: L.capgpu_plonk_key_solver_info(ctypes.c_uint64(1), ctypes.byref(info))]
    for call in calls:
        L.capgpu_msm_var_plan(ctypes.c_size_t(1), -1, None, ctypes.c_size_t(0))      # leaves another message behind
        assert call() == NOT_INITIALISED
        assert b"not initialised" in L.capgpu_last_error()
    for fn, args in ((cg.plonk_key_set_given, (1, [0, 1])), (cg.plonk_key_solver_info, (1,)),
                     (cg.plonk_solve_vars, (1, np.zeros((1, 2, 4), np.uint64)))):
        with pytest.raises(cg.CapGpuError) as e:
            fn(*args)
        assert e.value.code == NOT_INITIALISED


def test_the_mirrors_name_the_calls():
    for fn in ("plonk_key_set_given", "plonk_key_solver_info", "plonk_solve_vars"):
        assert callable(getattr(cg, fn)), fn
    rs = open(os.path.join(ROOT, "bindings", "capgpu-sys", "src", "lib.rs")).read()
    for name in SYMBOLS:
        assert f"pub fn {name}(" in rs, name
    for text in ("pub struct capgpu_solver_info", "pub struct capgpu_solve_status", "pub fn set_given(", "pub fn solve("):
        assert text in rs, text
