"""The inverse-form setting and the batch inverse (capgpu_fr_set_inverse_form, capgpu_fr_get_inverse_form,
capgpu_fr_inverse_batch[_dev], capgpu_fr_inverse_stats) at the C boundary, with no device work: the five symbols are exported
and mirrored, the set call refuses everything but the two forms and says so, NULL pointers are refused before the device is
looked for and a valid call before capgpu_init returns CAPGPU_ERR_NOT_INITIALISED, and CAPGPU_FR_INVERSE sets the process
default.  The not-initialised and environment cases run in a child process that never calls capgpu_init, so they hold with
and without a GPU.  (`-m "not gpu"`)"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from cap_amd import lib as cg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("capgpu_fr_set_inverse_form", "capgpu_fr_get_inverse_form", "capgpu_fr_inverse_batch",
           "capgpu_fr_inverse_batch_dev", "capgpu_fr_inverse_stats")
INVALID_ARG, NOT_INITIALISED = -1, -6


def test_symbols_are_exported_declared_and_mirrored():
    L = cg.load()
    hdr = open(os.path.join(ROOT, "include", "capgpu.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "capgpu-sys", "src", "lib.rs")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(rf"\bint {name}\(", hdr), name
        assert f"pub fn {name}(" in rs, name
    assert re.search(r"#define CAPGPU_INVERSE_FERMAT 0\b", hdr) and re.search(r"#define CAPGPU_INVERSE_GCD 1\b", hdr)
    assert "pub const CAPGPU_INVERSE_FERMAT: c_int = 0;" in rs and "pub const CAPGPU_INVERSE_GCD: c_int = 1;" in rs
    assert (cg.INVERSE_FERMAT, cg.INVERSE_GCD) == (0, 1)
    for fn in ("fr_set_inverse_form", "fr_get_inverse_form", "fr_inverse_batch", "fr_inverse_stats"):
        assert callable(getattr(cg, fn)), fn


def test_set_refuses_everything_but_the_two_forms():
    L = cg.load()
    before = cg.fr_get_inverse_form()
    try:
        for bad in (2, -1, 7):
            L.capgpu_msm_var_plan(ctypes.c_size_t(1), -1, None, ctypes.c_size_t(0))      # leaves another message behind
            assert L.capgpu_fr_set_inverse_form(bad) == INVALID_ARG
            msg = L.capgpu_last_error()
            assert b"capgpu_fr_set_inverse_form" in msg and str(bad).encode() in msg and b"CAPGPU_INVERSE_GCD" in msg
            assert cg.fr_get_inverse_form() == before, "a refused form leaves the setting alone"
        with pytest.raises(cg.CapGpuError) as e:
            cg.fr_set_inverse_form(2)
        assert e.value.code == INVALID_ARG
        for form, want in ((1, 1), (0, 0), ("gcd", 1), ("fermat", 0)):
            cg.fr_set_inverse_form(form)
            assert cg.fr_get_inverse_form() == want
    finally:
        cg.fr_set_inverse_form(before)


def test_get_refuses_null():
    L = cg.load()
    assert L.capgpu_fr_get_inverse_form(None) == INVALID_ARG
    assert b"capgpu_fr_get_inverse_form" in L.capgpu_last_error() and b"NULL" in L.capgpu_last_error()


@pytest.mark.parametrize("name", SYMBOLS[2:4])
def test_batch_refuses_null_arrays_before_the_device_is_looked_for(name):
    L = cg.load()
    a = np.zeros(8, np.uint64)
    p = a.ctypes.data_as(ctypes.c_void_p)
    for args in ((None, p), (p, None), (None, None)):
        assert getattr(L, name)(args[0], args[1], ctypes.c_size_t(2)) == INVALID_ARG
        assert name.encode() + b": bad argument" in L.capgpu_last_error()


def test_stats_take_null_pointers():
    L = cg.load()
    assert L.capgpu_fr_inverse_stats(None, None) == 0
    s = cg.fr_inverse_stats()
    assert set(s) == {"fermat_launches", "gcd_launches"}


CHILD = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from cap_amd import lib as cg
L = cg.load()
print("default", cg.fr_get_inverse_form())
a = np.zeros(8, np.uint64)
p = a.ctypes.data_as(ctypes.c_void_p)
for name in ("capgpu_fr_inverse_batch", "capgpu_fr_inverse_batch_dev"):
    for count in (2, 0):
        L.capgpu_msm_var_plan(ctypes.c_size_t(1), -1, None, ctypes.c_size_t(0))
        rc = getattr(L, name)(p, p, ctypes.c_size_t(count))
        print(name, count, rc, b"not initialised" in L.capgpu_last_error())
try:
    cg.fr_inverse_batch(np.zeros((2, 4), np.uint64))
    print("wrapper no error")
except cg.CapGpuError as e:
    print("wrapper", e.code)
print("stats", cg.fr_inverse_stats())
"""


def _child(env_value):
    env = dict(os.environ)
    env.pop("CAPGPU_FR_INVERSE", None)
    if env_value is not None:
        env["CAPGPU_FR_INVERSE"] = env_value
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout[-800:] + out.stderr[-800:]
    return out.stdout.splitlines()


def test_valid_batch_calls_before_init_are_not_initialised():
    lines = _child(None)
    assert "default 0" in lines
    for name in SYMBOLS[2:4]:
        for count in (2, 0):
            assert f"{name} {count} {NOT_INITIALISED} True" in lines, lines
    assert f"wrapper {NOT_INITIALISED}" in lines
    assert "stats {'fermat_launches': 0, 'gcd_launches': 0}" in lines, "a refused call launches nothing"


@pytest.mark.parametrize("value,want", [("gcd", 1), ("fermat", 0), ("GCD", 0), ("1", 0), ("euclid", 0), ("", 0)])
def test_environment_sets_the_process_default(value, want):
    assert f"default {want}" in _child(value)
