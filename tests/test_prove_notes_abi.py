"""The notes entry points (capgpu_plonk_prove_notes / _dev / _async, _notes_plan, _reserve_notes, _notes_stats) at the C
boundary, on a machine without a GPU: they are exported, the two structs have the header's layout, the pointer refusals -
in the header's order - come before the device is looked for and CAPGPU_ERR_NOT_INITIALISED after them, and the mirrors
name the calls.  (`-m "not gpu"`)"""
import ctypes
import os

import numpy as np
import pytest

from cap_amd import lib as cg
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROVING = ("capgpu_plonk_prove_notes", "capgpu_plonk_prove_notes_dev", "capgpu_plonk_prove_notes_async")
SYMBOLS = PROVING + ("capgpu_plonk_notes_plan", "capgpu_plonk_reserve_notes", "capgpu_plonk_notes_stats")
INVALID_ARG, NOT_INITIALISED = -1, -6


def test_symbols_are_exported():
    L = cg.load()
    for name in SYMBOLS:
        assert hasattr(L, name), name


def test_struct_layouts_match_the_header():
    assert ctypes.sizeof(cg.NotesGroup) == 32 and ctypes.sizeof(cg.NotesStats) == 56
    assert [(f, getattr(cg.NotesGroup, f).offset) for f, _ in cg.NotesGroup._fields_] == [
        ("srs_handle", 0), ("domain_size", 8), ("count", 16), ("first", 20), ("max_inputs", 24), ("run_order", 28)]
    assert [getattr(cg.NotesStats, f).offset for f, _ in cg.NotesStats._fields_] == list(range(0, 56, 8))
    hdr = open(os.path.join(ROOT, "include", "capgpu.h")).read()
    assert "} capgpu_notes_group;  /* 32 bytes */" in hdr and "} capgpu_notes_stats;           /* 56 bytes */" in hdr


def _args(count=2, n=16, nin=1):
    rows = [np.zeros(5 * n * 4, np.uint64) for _ in range(count)]
    return dict(h=(ctypes.c_uint64 * count)(*([1] * count)), rows=rows,
                w=(ctypes.c_void_p * count)(*[r.ctypes.data for r in rows]), x=(ctypes.c_uint64 * count)(*range(count)),
                p=np.zeros(count * nin * 4, np.uint64), b=np.zeros(count * 13 * 4, np.uint64), pr=(cg.Proof * count)(),
                oc=(cg.ProveOutcome * count)(), t=ctypes.c_uint64(7), m=(ctypes.c_char_p * count)(*([b"m"] * count)),
                l=(ctypes.c_size_t * count)(*([1] * count)))


def _call(L, name, a, count=2, nin=1, form=0, misalign=0, **null):
    g = lambda k: None if null.get(k) else a[k]                  # noqa: E731
    ptr = lambda k: None if null.get(k) else cg._p(a[k])         # noqa: E731
    if name.endswith("_dev"):                                   # never dereferenced on the host: a host address stands in
        wires = [None if null.get("w") else ctypes.c_void_p(a["rows"][0].ctypes.data + misalign), g("x")]
    else:
        wires = [g("w")]
    args = [g("h"), count, *wires, ptr("p"), ctypes.c_size_t(nin), g("m"), g("l"), ptr("b"), form, g("pr"), g("oc")]
    if name.endswith("_async"):
        args.append(None if null.get("t") else ctypes.byref(a["t"]))
    return getattr(L, name)(*args)


@pytest.mark.parametrize("name", PROVING)
def test_bad_arguments_are_refused_before_the_device_is_looked_for(name):
    L = cg.load()
    a = _args()
    missing = ["h", "w", "p", "b", "pr", "oc", "l"] + (["x"] if name.endswith("_dev") else []) + \
        (["t"] if name.endswith("_async") else [])
    for k in missing:
        assert _call(L, name, a, **{k: True}) == INVALID_ARG, k
        assert L.capgpu_last_error() == b"capgpu_plonk_prove_notes: bad argument", k
    assert _call(L, name, a, count=-1) == INVALID_ARG
    # the order: the form before the pointers, the pointers before the rows / the alignment
    assert _call(L, name, a, form=7, b=True) == INVALID_ARG and b"input_form 7" in L.capgpu_last_error()
    if name.endswith("_dev"):
        assert _call(L, name, a, misalign=8) == INVALID_ARG and b"not 16-byte aligned" in L.capgpu_last_error()
        assert _call(L, name, a, misalign=8, oc=True) == INVALID_ARG and b"bad argument" in L.capgpu_last_error()
    else:
        a["w"][1] = None
        assert _call(L, name, a) == INVALID_ARG and L.capgpu_last_error() == b"capgpu_plonk_prove_notes: wires[1] is NULL"
        assert _call(L, name, a, oc=True) == INVALID_ARG and b"bad argument" in L.capgpu_last_error()


def test_plan_reserve_and_stats_pointer_checks():
    L = cg.load()
    h = (ctypes.c_uint64 * 2)(1, 1)
    groups, num = (cg.NotesGroup * 2)(), ctypes.c_size_t(9)
    assert L.capgpu_plonk_notes_plan(None, 2, groups, ctypes.c_size_t(2), ctypes.byref(num), None) == INVALID_ARG
    assert L.capgpu_plonk_notes_plan(h, 2, None, ctypes.c_size_t(2), ctypes.byref(num), None) == INVALID_ARG
    assert L.capgpu_plonk_notes_plan(h, 2, groups, ctypes.c_size_t(2), None, None) == INVALID_ARG
    assert L.capgpu_plonk_notes_plan(h, -1, groups, ctypes.c_size_t(2), ctypes.byref(num), None) == INVALID_ARG
    assert b"capgpu_plonk_notes_plan: bad argument" in L.capgpu_last_error()
    assert L.capgpu_plonk_reserve_notes(None, 2, 0, -1) == INVALID_ARG
    assert L.capgpu_plonk_reserve_notes(h, 2, 7, -1) == INVALID_ARG and b"input_form 7" in L.capgpu_last_error()
    assert L.capgpu_plonk_notes_stats(None) == INVALID_ARG
    s = cg.plonk_notes_stats()                                  # process-wide counters: readable without a device
    assert set(s) == {f for f, _ in cg.NotesStats._fields_}


@pytest.mark.parametrize("name", PROVING)
def test_valid_calls_refuse_without_a_device(name):
    if H.gpu_present():
        pytest.skip("GPU present: the refusal path is covered on the CPU-only runner")
    L = cg.load()
    a = _args()
    assert _call(L, name, a) == NOT_INITIALISED
    assert b"not initialised" in L.capgpu_last_error()
    assert _call(L, name, a, count=0) == NOT_INITIALISED        # count == 0 is answered after the device is looked for
    if name == "capgpu_plonk_prove_notes":
        with pytest.raises(cg.CapGpuError) as e:
            cg.plonk_prove_notes([1, 1], a["rows"], a["p"], a["b"])
        assert e.value.code == NOT_INITIALISED
        h = (ctypes.c_uint64 * 2)(1, 1)
        groups, num = (cg.NotesGroup * 2)(), ctypes.c_size_t(9)
        assert L.capgpu_plonk_notes_plan(h, 2, groups, ctypes.c_size_t(2), ctypes.byref(num), None) == NOT_INITIALISED
        assert L.capgpu_plonk_reserve_notes(h, 2, 0, -1) == NOT_INITIALISED


def test_the_mirrors_name_the_calls():
    from cap_amd import proof
    for fn in ("plonk_prove_notes", "plonk_prove_notes_dev", "plonk_prove_notes_async", "plonk_notes_plan",
               "plonk_reserve_notes", "plonk_notes_stats"):
        assert callable(getattr(cg, fn)), fn
    assert callable(proof.prove_notes)
    hpp = open(os.path.join(ROOT, "include", "capgpu_proof.hpp")).read()
    assert "capgpu_plonk_prove_notes(" in hpp and "prove_notes(" in hpp
    rs = open(os.path.join(ROOT, "bindings", "capgpu-sys", "src", "lib.rs")).read()
    for name in SYMBOLS:
        assert f"pub fn {name}(" in rs, name
    assert "pub fn prove_notes(" in rs and "pub struct capgpu_notes_group" in rs and "pub struct capgpu_notes_stats" in rs
