"""The solver hints' entry points (capgpu_plonk_key_set_given_hints, capgpu_plonk_key_hint_info) at the C boundary, on a
machine without a GPU: they are exported, the two structs have the header's layout, pointer errors come before the device
is looked for and CAPGPU_ERR_NOT_INITIALISED after them, and the mirrors name the calls.  (`-m "not gpu"`)"""
import ctypes
import os
import re

import numpy as np
import pytest

from cap_amd import lib as cg
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("capgpu_plonk_key_set_given_hints", "capgpu_plonk_key_hint_info")
INVALID_ARG, NOT_INITIALISED = -1, -6
u32p = ctypes.POINTER(ctypes.c_uint32)


def test_symbols_are_exported():
    L = cg.load()
    for name in SYMBOLS:
        assert hasattr(L, name), name


def test_struct_layouts_and_kinds_match_the_header():
    assert ctypes.sizeof(cg.Hint) == 16 and ctypes.sizeof(cg.HintInfo) == 48 and ctypes.sizeof(cg.SolverInfo) == 48
    assert [(f[0], getattr(cg.Hint, f[0]).offset) for f in cg.Hint._fields_] == [("kind", 0), ("src", 4), ("first", 8), ("count", 12)]
    assert [f[0] for f in cg.HintInfo._fields_] == ["num_hints", "num_hinted", "bits_hints", "inv_hints", "iszero_hints",
                                                    "hint_items"]
    hdr = open(os.path.join(ROOT, "include", "capgpu.h")).read()
    assert "} capgpu_hint; /* 16 bytes */" in hdr and "} capgpu_hint_info; /* 48 bytes */" in hdr
    kinds = dict(re.findall(r"#define CAPGPU_HINT_([A-Z0-9]+) (\d+)", hdr))
    assert kinds == {"BITS": str(cg.HINT_BITS), "INV0": str(cg.HINT_INV0), "ISZERO": str(cg.HINT_ISZERO)}
    # the fields of capgpu_hint_info in the header's order
    body = re.search(r"typedef struct capgpu_hint_info \{(.*?)\} capgpu_hint_info;", hdr, flags=re.S).group(1)
    assert re.findall(r"uint64_t (\w+);", body) == [f[0] for f in cg.HintInfo._fields_]
    body = re.search(r"typedef struct capgpu_hint \{(.*?)\} capgpu_hint;", hdr, flags=re.S).group(1)
    assert re.findall(r"uint32_t (\w+);", body) == [f[0] for f in cg.Hint._fields_]


def _set_up(L, given=True, hints=True, targets=True, num_hints=1, num_targets=1):
    ids = np.arange(3, dtype=np.uint32)
    tab = (cg.Hint * 1)(cg.Hint(cg.HINT_INV0, 0, 0, 1))
    tg = np.array([2], np.uint32)
    return L.capgpu_plonk_key_set_given_hints(ctypes.c_uint64(1), ids.ctypes.data_as(u32p) if given else None, ctypes.c_size_t(3),
                                              tab if hints else None, ctypes.c_size_t(num_hints),
                                              tg.ctypes.data_as(u32p) if targets else None, ctypes.c_size_t(num_targets), None, None)


def test_bad_arguments_are_refused_before_the_device_is_looked_for():
    L = cg.load()
    assert _set_up(L, given=False) == INVALID_ARG
    assert b"capgpu_plonk_key_set_given_hints: bad argument (given_vars is NULL)" in L.capgpu_last_error()
    assert _set_up(L, hints=False) == INVALID_ARG
    assert b"capgpu_plonk_key_set_given_hints: bad argument (hints is NULL)" in L.capgpu_last_error()
    assert _set_up(L, targets=False) == INVALID_ARG
    assert b"capgpu_plonk_key_set_given_hints: bad argument (targets is NULL)" in L.capgpu_last_error()
    assert _set_up(L, num_hints=1 << 32) == INVALID_ARG and b"below 2^32" in L.capgpu_last_error()
    assert _set_up(L, num_targets=1 << 32) == INVALID_ARG and b"below 2^32" in L.capgpu_last_error()
    assert L.capgpu_plonk_key_hint_info(ctypes.c_uint64(1), None) == INVALID_ARG
    assert b"capgpu_plonk_key_hint_info: bad argument" in L.capgpu_last_error()
    # the Python mirror refuses ids that do not fit the ABI's 32 bits before it calls
    with pytest.raises(cg.CapGpuError) as e:
        cg.plonk_key_set_given_hints(1, [0, 1], [(cg.HINT_INV0, 1 << 32, [2])])
    assert e.value.code == INVALID_ARG and "hint 0" in str(e.value)
    if not H.gpu_present():
        # valid calls - NULL hints with num_hints == 0 among them - reach the device look-up
        info = cg.HintInfo()
        for call in (lambda: _set_up(L), lambda: _set_up(L, hints=False, targets=False, num_hints=0, num_targets=0),
                     lambda: L.capgpu_plonk_key_hint_info(ctypes.c_uint64(1), ctypes.byref(info))):
            L.capgpu_msm_var_plan(ctypes.c_size_t(1), -1, None, ctypes.c_size_t(0))      # leaves another message behind
            assert call() == NOT_INITIALISED
            assert b"not initialised" in L.capgpu_last_error()
        for fn, args in ((cg.plonk_key_set_given_hints, (1, [0, 1], [(cg.HINT_ISZERO, 0, [2])])), (cg.plonk_key_hint_info, (1,))):
            with pytest.raises(cg.CapGpuError) as e:
                fn(*args)
            assert e.value.code == NOT_INITIALISED


def test_the_mirrors_name_the_calls():
    for fn in ("plonk_key_set_given_hints", "plonk_key_hint_info"):
        assert callable(getattr(cg, fn)), fn
    rs = open(os.path.join(ROOT, "bindings", "capgpu-sys", "src", "lib.rs")).read()
    for name in SYMBOLS:
        assert f"pub fn {name}(" in rs, name
    for text in ("pub struct capgpu_hint {", "pub struct capgpu_hint_info {", "pub fn set_given_hints(", "pub fn hint_info(",
                 "pub const CAPGPU_HINT_BITS: u32 = 0;", "pub const CAPGPU_HINT_INV0: u32 = 1;",
                 "pub const CAPGPU_HINT_ISZERO: u32 = 2;"):
        assert text in rs, text
