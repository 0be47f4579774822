"""The entry points of the solver's DEFERRED form (capgpu_plonk_key_set_solve_form, capgpu_plonk_key_solve_form_info) at the C
boundary, on a machine without a GPU: they are exported and declared, the info struct has the header's 64 bytes and field
order, argument errors come before the device is looked for and CAPGPU_ERR_NOT_INITIALISED after them, and the mirrors name
the calls.  (`-m "not gpu"`)"""
import ctypes
import os
import re

from cap_amd import lib as cg
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("capgpu_plonk_key_set_solve_form", "capgpu_plonk_key_solve_form_info")
INVALID_ARG, NOT_INITIALISED = -1, -6
FIELDS = ["form", "deferred_vars", "frac_rows", "flush_levels", "flush_items", "levels", "inv_levels_direct",
          "inv_levels_deferred"]


def test_symbols_are_exported_and_declared():
    L = cg.load()
    hdr = open(os.path.join(ROOT, "include", "capgpu.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert f"int {name}(" in hdr, name


def test_struct_layout_and_forms_match_the_header():
    assert ctypes.sizeof(cg.SolveFormInfo) == 64
    hdr = open(os.path.join(ROOT, "include", "capgpu.h")).read()
    assert "} capgpu_solve_form_info; /* 64 bytes */" in hdr
    body = re.search(r"typedef struct capgpu_solve_form_info \{(.*?)\} capgpu_solve_form_info;", hdr, flags=re.S).group(1)
    assert re.findall(r"uint64_t (\w+);", body) == [f[0] for f in cg.SolveFormInfo._fields_] == FIELDS
    assert [getattr(cg.SolveFormInfo, f).offset for f in FIELDS] == list(range(0, 64, 8))
    forms = dict(re.findall(r"#define CAPGPU_SOLVE_FORM_([A-Z]+) (\d+)\n", hdr))
    assert forms == {"DIRECT": str(cg.SOLVE_FORM_DIRECT), "DEFERRED": str(cg.SOLVE_FORM_DEFERRED)} == {"DIRECT": "0", "DEFERRED": "1"}
    # the form is a call of its own: the solver's flags are the two they were
    assert set(re.findall(r"#define CAPGPU_SOLVER_([A-Z_]+) ", hdr)) == {"LINEAR", "DERIVE_PUBLIC"}


def test_bad_arguments_are_refused_before_the_device_is_looked_for():
    L = cg.load()
    info = cg.SolveFormInfo()
    for form in (2, -1, 7):
        assert L.capgpu_plonk_key_set_solve_form(ctypes.c_uint64(1), ctypes.c_int(form), ctypes.byref(info)) == INVALID_ARG, form
        err = L.capgpu_last_error()
        assert b"capgpu_plonk_key_set_solve_form: bad argument (form" in err and b"the key is unchanged" in err, err
        assert b"CAPGPU_SOLVE_FORM_DIRECT (0)" in err and b"CAPGPU_SOLVE_FORM_DEFERRED (1)" in err, err
    for form in (0, 1):
        assert L.capgpu_plonk_key_set_solve_form(ctypes.c_uint64(0), ctypes.c_int(form), ctypes.byref(info)) == INVALID_ARG
        assert b"capgpu_plonk_key_set_solve_form: bad argument (pk_handle is 0)" in L.capgpu_last_error()
    assert L.capgpu_plonk_key_solve_form_info(ctypes.c_uint64(1), None) == INVALID_ARG
    assert b"capgpu_plonk_key_solve_form_info: bad argument (info_out is NULL)" in L.capgpu_last_error()
    assert L.capgpu_plonk_key_solve_form_info(ctypes.c_uint64(0), ctypes.byref(info)) == INVALID_ARG
    assert b"capgpu_plonk_key_solve_form_info: bad argument (pk_handle is 0)" in L.capgpu_last_error()
    if not H.gpu_present():
        for call in (lambda: L.capgpu_plonk_key_set_solve_form(ctypes.c_uint64(1), ctypes.c_int(1), ctypes.byref(info)),
                     lambda: L.capgpu_plonk_key_set_solve_form(ctypes.c_uint64(1), ctypes.c_int(0), None),   # info_out is optional
                     lambda: L.capgpu_plonk_key_solve_form_info(ctypes.c_uint64(1), ctypes.byref(info))):
            assert call() == NOT_INITIALISED
            assert b"not initialised" in L.capgpu_last_error()


def test_the_mirrors_name_the_calls():
    for fn in ("plonk_key_set_solve_form", "plonk_key_solve_form_info"):
        assert callable(getattr(cg, fn)), fn
    rs = open(os.path.join(ROOT, "bindings", "capgpu-sys", "src", "lib.rs")).read()
    for name in SYMBOLS:
        assert f"pub fn {name}(" in rs, name
    for text in ("pub struct capgpu_solve_form_info {", "pub const CAPGPU_SOLVE_FORM_DIRECT: c_int = 0;",
                 "pub const CAPGPU_SOLVE_FORM_DEFERRED: c_int = 1;", "pub fn set_solve_form(", "pub fn solve_form_info("):
        assert text in rs, text
    body = re.search(r"pub struct capgpu_solve_form_info \{(.*?)\}", rs, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): u64,", body) == FIELDS
    hpp = open(os.path.join(ROOT, "include", "capgpu_proof.hpp")).read()
    for name in SYMBOLS:
        assert name + "(" in hpp, name
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert name in doc, name
