"""The per-proof outcome entry points (capgpu_plonk_prove_each*, capgpu_prove_outcome_text) at the C boundary, on a machine
without a GPU: they are exported, capgpu_prove_outcome has the header's layout, argument errors come before the device is
looked for and CAPGPU_ERR_NOT_INITIALISED after them, the text needs no device, and the mirrors name the calls.
(`-m "not gpu"`)"""
import ctypes
import os

import numpy as np
import pytest

from cap_amd import lib as cg
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("capgpu_plonk_prove_each", "capgpu_plonk_prove_each_dev", "capgpu_plonk_prove_each_async",
           "capgpu_prove_outcome_text")
INVALID_ARG, NOT_INITIALISED = -1, -6


def test_symbols_are_exported():
    L = cg.load()
    for name in SYMBOLS:
        assert hasattr(L, name), name


def test_outcome_layout_matches_the_header():
    assert ctypes.sizeof(cg.WitnessFault) == 48
    assert ctypes.sizeof(cg.ProveOutcome) == 56
    assert cg.ProveOutcome.status.offset == 0 and cg.ProveOutcome.status.size == 4
    assert cg.ProveOutcome.degree_flags.offset == 4 and cg.ProveOutcome.degree_flags.size == 4
    assert cg.ProveOutcome.fault.offset == 8 and cg.ProveOutcome.fault.size == 48
    hdr = open(os.path.join(ROOT, "include", "capgpu.h")).read()
    assert "} capgpu_prove_outcome;" in hdr and "/* 56 bytes */" in hdr


def _args(count=2, n=16, nin=1):
    return dict(h=(ctypes.c_uint64 * count)(*([1] * count)), w=np.zeros(count * 5 * n * 4, np.uint64),
                p=np.zeros(count * nin * 4, np.uint64), b=np.zeros(count * 13 * 4, np.uint64), pr=(cg.Proof * count)(),
                oc=(cg.ProveOutcome * count)(), t=ctypes.c_uint64(7))


def _call(L, name, a, count=2, nin=1, form=0, **null):
    g = lambda k: None if null.get(k) else a[k]                  # noqa: E731
    ptr = lambda k: None if null.get(k) else cg._p(a[k])         # noqa: E731
    wires = ptr("w")
    if name.endswith("_dev") and wires is not None:             # never dereferenced on the host: a host address stands in
        wires = a["w"].ctypes.data_as(ctypes.c_void_p)
    args = [g("h"), count, wires, ptr("p"), ctypes.c_size_t(nin), None, None, ptr("b"), form, g("pr"), g("oc")]
    if name.endswith("_async"):
        args.append(None if null.get("t") else ctypes.byref(a["t"]))
    return getattr(L, name)(*args)


@pytest.mark.parametrize("name", SYMBOLS[:3])
def test_bad_arguments_are_refused_before_the_device_is_looked_for(name):
    L = cg.load()
    a = _args()
    for missing in ("h", "w", "p", "b", "pr", "oc"):
        assert _call(L, name, a, **{missing: True}) == INVALID_ARG, missing
        assert b"bad argument" in L.capgpu_last_error()
    assert _call(L, name, a, count=-1) == INVALID_ARG
    assert _call(L, name, a, form=7) == INVALID_ARG and b"input_form 7" in L.capgpu_last_error()
    # messages without their lengths
    msgs = (ctypes.c_char_p * 2)(b"a", b"b")
    wires = a["w"].ctypes.data_as(ctypes.c_void_p) if name.endswith("_dev") else cg._p(a["w"])
    tail = [ctypes.byref(a["t"])] if name.endswith("_async") else []
    assert getattr(L, name)(a["h"], 2, wires, cg._p(a["p"]), ctypes.c_size_t(1), msgs, None, cg._p(a["b"]), 0, a["pr"],
                            a["oc"], *tail) == INVALID_ARG
    if name.endswith("_async"):
        assert _call(L, name, a, t=True) == INVALID_ARG


@pytest.mark.parametrize("name", SYMBOLS[:3])
def test_valid_calls_refuse_without_a_device(name):
    if H.gpu_present():
        pytest.skip("GPU present: the refusal path is covered on the CPU-only runner")
    L = cg.load()
    a = _args()
    assert _call(L, name, a) == NOT_INITIALISED
    assert b"not initialised" in L.capgpu_last_error()
    if name == "capgpu_plonk_prove_each":
        with pytest.raises(cg.CapGpuError) as e:
            cg.plonk_prove_each([1, 1], a["w"], a["p"], a["b"])
        assert e.value.code == NOT_INITIALISED


def test_outcome_text_needs_no_device():
    L = cg.load()
    o = cg.ProveOutcome()
    assert cg.prove_outcome_text(o) == "" and str(o) == ""
    o.status, o.degree_flags = -7, 2
    assert cg.prove_outcome_text(o) == ("capgpu_plonk_prove: proof 0: quotient polynomial has the wrong degree (flags 2): "
                                        "the circuit is not satisfied by this witness")
    o.fault.kind, o.fault.row = 1, 17
    assert cg.prove_outcome_text(o) == ("capgpu_plonk_prove: 1 of 1 witnesses do not satisfy their circuit; first: proof 0: "
                                        "gate 17 not satisfied")
    o.fault.kind, o.fault.wire, o.fault.row, o.fault.wire2, o.fault.row2 = 2, 3, 5, 1, 9
    assert cg.prove_outcome_text(o).endswith("first: proof 0: copy constraint (3,5) -> (1,9) violated")
    buf = ctypes.create_string_buffer(b"xxxxxxxx", 8)
    assert L.capgpu_prove_outcome_text(ctypes.byref(o), buf, ctypes.c_size_t(8)) == 0 and buf.raw == b"capgpu_\0"
    assert L.capgpu_prove_outcome_text(ctypes.byref(o), buf, ctypes.c_size_t(0)) == 0 and buf.raw == b"capgpu_\0"
    assert L.capgpu_prove_outcome_text(ctypes.byref(o), None, ctypes.c_size_t(0)) == 0
    assert L.capgpu_prove_outcome_text(None, buf, ctypes.c_size_t(8)) == INVALID_ARG
    assert L.capgpu_prove_outcome_text(ctypes.byref(o), None, ctypes.c_size_t(8)) == INVALID_ARG


def test_the_mirrors_name_the_calls():
    from cap_amd import proof
    for fn in ("plonk_prove_each", "plonk_prove_each_dev", "plonk_prove_each_async", "prove_outcome_text"):
        assert callable(getattr(cg, fn)), fn
    assert callable(proof.prove_each)
    hpp = open(os.path.join(ROOT, "include", "capgpu_proof.hpp")).read()
    assert "capgpu_plonk_prove_each(" in hpp and "capgpu_prove_outcome_text(" in hpp and "prove_each(" in hpp
    rs = open(os.path.join(ROOT, "bindings", "capgpu-sys", "src", "lib.rs")).read()
    for name in SYMBOLS:
        assert f"pub fn {name}(" in rs, name
    assert "pub fn prove_each(" in rs and "pub struct capgpu_prove_outcome" in rs
