"""The given-value proving entry points (capgpu_plonk_prove_given*, capgpu_plonk_reserve_given) and the solver's packing
knobs (capgpu_plonk_set/get_solve_pack, capgpu_plonk_solve_stats) at the C boundary, on a machine without a GPU: they are
exported, the two records they fill keep the header's sizes, argument errors come before the device is looked for and
CAPGPU_ERR_NOT_INITIALISED after them, and the packing setting needs no capgpu_init.  (`-m "not gpu"`)"""
import ctypes
import os

import numpy as np
import pytest

from cap_amd import lib as cg
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROVE = ("capgpu_plonk_prove_given", "capgpu_plonk_prove_given_dev", "capgpu_plonk_prove_given_async")
SYMBOLS = PROVE + ("capgpu_plonk_reserve_given", "capgpu_plonk_set_solve_pack", "capgpu_plonk_get_solve_pack",
                   "capgpu_plonk_solve_stats")
INVALID_ARG, NOT_INITIALISED = -1, -6


def test_symbols_are_exported():
    L = cg.load()
    for name in SYMBOLS:
        assert hasattr(L, name), name
    hdr = open(os.path.join(ROOT, "include", "capgpu.h")).read()
    for name in SYMBOLS:
        assert f"int {name}(" in hdr, name


def test_record_layouts_are_unchanged():
    assert ctypes.sizeof(cg.SolveStatus) == 16
    assert ctypes.sizeof(cg.ProveOutcome) == 56
    hdr = open(os.path.join(ROOT, "include", "capgpu.h")).read()
    assert "} capgpu_solve_status; /* 16 bytes */" in hdr
    assert "} capgpu_prove_outcome;" in hdr and "/* 56 bytes */" in hdr


def _args(count=2, num_given=3, nin=1):
    return dict(h=(ctypes.c_uint64 * count)(*([1] * count)), g=np.zeros(count * num_given * 4, np.uint64),
                p=np.zeros(count * nin * 4, np.uint64), b=np.zeros(count * 13 * 4, np.uint64), pr=(cg.Proof * count)(),
                oc=(cg.ProveOutcome * count)(), sv=(cg.SolveStatus * count)(), t=ctypes.c_uint64(7))


def _call(L, name, a, count=2, nin=1, msgs=None, lens=None, **null):
    g = lambda k: None if null.get(k) else a[k]                  # noqa: E731
    ptr = lambda k: None if null.get(k) else cg._p(a[k])         # noqa: E731
    given = ptr("g")
    if name.endswith("_dev") and given is not None:             # never dereferenced on the host: a host address stands in
        given = a["g"].ctypes.data_as(ctypes.c_void_p)
    args = [g("h"), count, given, ptr("p"), ctypes.c_size_t(nin), msgs, lens, ptr("b"), g("pr"), g("oc"), g("sv")]
    if name.endswith("_async"):
        args.append(None if null.get("t") else ctypes.byref(a["t"]))
    return getattr(L, name)(*args)


@pytest.mark.parametrize("name", PROVE)
def test_bad_arguments_are_refused_before_the_device_is_looked_for(name):
    L = cg.load()
    a = _args()
    for missing in ("h", "g", "p", "b", "pr", "oc"):
        assert _call(L, name, a, **{missing: True}) == INVALID_ARG, missing
        assert L.capgpu_last_error() == b"capgpu_plonk_prove_given: bad argument", missing
    assert _call(L, name, a, count=-1) == INVALID_ARG
    assert L.capgpu_last_error() == b"capgpu_plonk_prove_given: bad argument"
    msgs = (ctypes.c_char_p * 2)(b"a", b"b")                     # messages without their lengths
    assert _call(L, name, a, msgs=msgs) == INVALID_ARG
    if name.endswith("_async"):
        assert _call(L, name, a, t=True) == INVALID_ARG
    # solved_out is optional: without it the call gets as far as the device
    if not H.gpu_present():
        assert _call(L, name, a, sv=True) == NOT_INITIALISED


@pytest.mark.parametrize("name", PROVE)
def test_valid_calls_refuse_without_a_device(name):
    if H.gpu_present():
        pytest.skip("GPU present: the refusal path is covered on the CPU-only runner")
    L = cg.load()
    a = _args()
    assert _call(L, name, a) == NOT_INITIALISED
    assert b"not initialised" in L.capgpu_last_error()
    # count == 0 writes nothing; (without a device it still has nothing to run on)
    assert _call(L, name, a, count=0) == NOT_INITIALISED
    assert a["t"].value == 7
    assert L.capgpu_plonk_reserve_given(ctypes.c_uint64(1), 2, -1) == NOT_INITIALISED
    assert L.capgpu_plonk_solve_stats(None, None, None) == NOT_INITIALISED
    with pytest.raises(cg.CapGpuError) as e:
        cg.plonk_prove_given([1, 1], a["g"], a["p"], a["b"])
    assert e.value.code == NOT_INITIALISED


def test_count_zero_with_null_pointers_passes_the_argument_check():
    """count == 0 asks for no pointer at all: the call is refused, if at all, for the missing device."""
    L = cg.load()
    for name in PROVE:
        tail = [ctypes.byref(ctypes.c_uint64(0))] if name.endswith("_async") else []
        rc = getattr(L, name)(None, 0, None, None, ctypes.c_size_t(0), None, None, None, None, None, None, *tail)
        assert rc == (0 if H.gpu_present() and _initialised(L) else NOT_INITIALISED), name


def _initialised(L):
    return L.capgpu_plonk_solve_stats(None, None, None) == 0


def test_solve_pack_setting_needs_no_init():
    L = cg.load()
    w = ctypes.c_int(-5)
    before = cg.plonk_get_solve_pack()
    try:
        for good in (1, 2, 4, 8, 16, 0):
            assert L.capgpu_plonk_set_solve_pack(good) == 0
            assert L.capgpu_plonk_get_solve_pack(ctypes.byref(w)) == 0 and w.value == good
            assert cg.plonk_get_solve_pack() == good
        for bad in (3, -1, 5, 32, 17):
            assert L.capgpu_plonk_set_solve_pack(bad) == INVALID_ARG, bad
            assert f"capgpu_plonk_set_solve_pack: {bad} is none of".encode() in L.capgpu_last_error()
            assert cg.plonk_get_solve_pack() == 0                # the refused value changed nothing
        with pytest.raises(cg.CapGpuError):
            cg.plonk_set_solve_pack(3)
        assert L.capgpu_plonk_get_solve_pack(None) == INVALID_ARG
    finally:
        cg.plonk_set_solve_pack(before)


def test_the_mirrors_name_the_calls():
    for fn in ("plonk_prove_given", "plonk_prove_given_async", "plonk_reserve_given", "plonk_set_solve_pack",
               "plonk_get_solve_pack", "plonk_solve_stats"):
        assert callable(getattr(cg, fn)), fn
    hpp = open(os.path.join(ROOT, "include", "capgpu_proof.hpp")).read()
    assert "capgpu_plonk_prove_given(" in hpp and "prove_given(" in hpp
    rs = open(os.path.join(ROOT, "bindings", "capgpu-sys", "src", "lib.rs")).read()
    for name in SYMBOLS:
        assert f"pub fn {name}(" in rs, name
