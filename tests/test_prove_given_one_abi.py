"""capgpu_plonk_prove_given_one / _io_one at the C boundary, on a machine without a GPU: both are exported with the declared
signatures, every NULL-pointer refusal is CAPGPU_ERR_INVALID_ARG before the device is looked for, well-formed arguments
before capgpu_init give CAPGPU_ERR_NOT_INITIALISED, and the C++ shim, the Rust binding and lib.py name both calls.
(`-m "not gpu"`)"""
import ctypes
import os
import re

import numpy as np
import pytest

from cap_amd import lib as cg
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE, IO_ONE = "capgpu_plonk_prove_given_one", "capgpu_plonk_prove_given_io_one"
INVALID_ARG, NOT_INITIALISED = -1, -6

# the parameter lists include/capgpu.h declares (types only, in order)
SIGNATURES = {
    ONE: ["uint64_t", "const uint64_t*", "size_t", "const uint64_t*", "size_t", "const uint8_t*", "size_t", "const uint64_t*",
          "capgpu_proof*", "capgpu_prove_outcome*", "capgpu_solve_status*"],
    IO_ONE: ["uint64_t", "const uint64_t*", "size_t", "size_t", "const uint8_t*", "size_t", "const uint64_t*", "uint64_t*",
             "capgpu_proof*", "capgpu_prove_outcome*", "capgpu_solve_status*"],
}


def _declared(name):
    hdr = open(os.path.join(ROOT, "include", "capgpu.h")).read()
    m = re.search(rf"\bint {name}\((.*?)\);", hdr, flags=re.S)
    assert m, f"{name} is not declared in include/capgpu.h"
    params = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    return [re.sub(r"\s*\w+\s*$", "", p.strip()).replace(" *", "*") for p in params]


def test_symbols_are_exported_with_the_declared_signatures():
    L = cg.load()
    for name, want in SIGNATURES.items():
        assert hasattr(L, name), name
        assert _declared(name) == want, name


def _args(num_given=3, nin=1):
    return dict(g=np.zeros(num_given * 4, np.uint64), p=np.zeros(max(nin, 1) * 4, np.uint64), b=np.zeros(13 * 4, np.uint64),
                pr=cg.Proof(), oc=cg.ProveOutcome(), sv=cg.SolveStatus(), m=b"msg")


def _call(L, name, a, num_given=3, nin=1, **null):
    arr = lambda k: None if null.get(k) else cg._p(a[k])           # noqa: E731
    ref = lambda k: None if null.get(k) else ctypes.byref(a[k])    # noqa: E731
    msg = None if null.get("m") else a["m"]
    mlen = ctypes.c_size_t(0 if msg is None else len(msg))
    head = [ctypes.c_uint64(1), arr("g"), ctypes.c_size_t(num_given)]
    if name == ONE:
        args = head + [arr("p"), ctypes.c_size_t(nin), msg, mlen, arr("b"), ref("pr"), ref("oc"), ref("sv")]
    else:
        args = head + [ctypes.c_size_t(nin), msg, mlen, arr("b"), arr("p"), ref("pr"), ref("oc"), ref("sv")]
    return getattr(L, name)(*args)


@pytest.mark.parametrize("name", [ONE, IO_ONE])
def test_null_pointers_are_refused_before_the_device_is_looked_for(name):
    L = cg.load()
    a = _args()
    for missing in ("g", "p", "b", "pr", "oc"):
        assert _call(L, name, a, **{missing: True}) == INVALID_ARG, missing
        assert L.capgpu_last_error() == b"capgpu_plonk_prove_given_one: bad argument", missing
    if H.gpu_present():
        return                                                      # (another test of this process may have initialised the library)
    # optional pointers: without them the call gets as far as the device
    assert _call(L, name, a, sv=True) == NOT_INITIALISED
    assert _call(L, name, a, m=True) == NOT_INITIALISED
    assert _call(L, name, a, nin=0, p=True) == NOT_INITIALISED       # no public inputs: no row to point at


@pytest.mark.parametrize("name", [ONE, IO_ONE])
def test_well_formed_calls_refuse_without_a_device(name):
    if H.gpu_present():
        pytest.skip("GPU present: the refusal path is covered on the CPU-only runner")
    L = cg.load()
    a = _args()
    assert _call(L, name, a) == NOT_INITIALISED
    assert b"not initialised" in L.capgpu_last_error()
    assert bytes(a["pr"]) == bytes(ctypes.sizeof(cg.Proof))          # nothing was written
    g, b = np.zeros((3, 4), np.uint64), np.zeros((13, 4), np.uint64)
    with pytest.raises(cg.CapGpuError) as e:
        cg.plonk_prove_given_one(1, g, np.zeros((1, 4), np.uint64), b, b"msg")
    assert e.value.code == NOT_INITIALISED
    with pytest.raises(cg.CapGpuError) as e:
        cg.plonk_prove_given_io_one(1, g, b, b"msg", num_inputs=1)
    assert e.value.code == NOT_INITIALISED


def test_the_mirrors_name_both_calls():
    for fn in ("plonk_prove_given_one", "plonk_prove_given_io_one"):
        assert callable(getattr(cg, fn)), fn
    hpp = open(os.path.join(ROOT, "include", "capgpu_proof.hpp")).read()
    rs = open(os.path.join(ROOT, "bindings", "capgpu-sys", "src", "lib.rs")).read()
    for name in (ONE, IO_ONE):
        assert f"{name}(" in hpp, name
        assert f"pub fn {name}(" in rs, name
    assert "prove_given_one(" in hpp and "prove_given_io_one(" in hpp
    assert re.search(r"pub fn prove_given_one\(.*?-> std::result::Result<capgpu_proof, ProveError>", rs, flags=re.S)
    # the header no longer lists the gathered form as left out, and states the one normalisation
    hdr = open(os.path.join(ROOT, "include", "capgpu.h")).read()
    assert "LEFT OUT: coalesced single-proof calls" not in hdr
    assert "degree_flags = 0 for every outcome whose fault.kind != 0" in hdr
