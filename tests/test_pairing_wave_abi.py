"""The pairing-form switch and the one-proof device verifier at the ABI, without a GPU (`-m "not gpu"`): the symbols are
exported and wrapped, the form is process-wide state that needs no capgpu_init and starts from CAPGPU_PAIRING, and
capgpu_plonk_verify_dev refuses to run without a device (no host path behind it)."""
import ctypes
import os
import subprocess
import sys

import numpy as np

from cap_amd import lib as cg
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("capgpu_pairing_set_form", "capgpu_pairing_get_form", "capgpu_pairing_stats", "capgpu_plonk_verify_dev")


def test_symbols_are_exported_and_wrapped():
    L = cg.load()
    for name in NEW:
        assert hasattr(L, name), name
    for name in ("pairing_set_form", "pairing_get_form", "pairing_stats", "plonk_verify_dev"):
        assert callable(getattr(cg, name)), name
    assert (cg.PAIRING_LANE, cg.PAIRING_WAVE) == (0, 1)
    hdr = open(os.path.join(ROOT, "include", "capgpu.h")).read()
    assert "#define CAPGPU_PAIRING_LANE 0" in hdr and "#define CAPGPU_PAIRING_WAVE 1" in hdr


def form_in_child(env_value):
    """the initial form of a fresh process (no capgpu_init), and what an unknown value and a set / get do there"""
    env = dict(os.environ)
    env.pop("CAPGPU_PAIRING", None)
    if env_value is not None:
        env["CAPGPU_PAIRING"] = env_value
    code = ("from cap_amd import lib as cg; L = cg.load(); a = cg.pairing_get_form(); "
            "bad = L.capgpu_pairing_set_form(2); b = cg.pairing_get_form(); cg.pairing_set_form(1 - a); "
            "print(a, bad, b, cg.pairing_get_form(), cg.pairing_stats())")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-500:]
    return out.stdout.strip()


def test_form_is_process_state_that_starts_from_the_environment():
    zero = "{'lane_checks': 0, 'wave_checks': 0}"
    assert form_in_child(None) == f"0 -1 0 1 {zero}"            # the default is LANE; an unknown form changes nothing
    assert form_in_child("lane") == f"0 -1 0 1 {zero}"
    assert form_in_child("wave") == f"1 -1 1 0 {zero}"


def test_verify_dev_needs_a_device_and_checks_its_arguments_first():
    L = cg.load()
    ok = ctypes.c_int(7)
    assert L.capgpu_plonk_verify_dev(None, None, None, None, ctypes.c_size_t(0), None, ctypes.c_size_t(0), None,
                                     ctypes.byref(ok)) == -1    # CAPGPU_ERR_INVALID_ARG
    if H.gpu_present():
        return                                                  # the refusal below is for a process without a device
    vk, pr = cg.VerifyingKey(), cg.Proof()
    h2 = cg.g2_generator()
    rc = L.capgpu_plonk_verify_dev(ctypes.byref(vk), h2.ctypes.data_as(cg.u64p), h2.ctypes.data_as(cg.u64p), None,
                                   ctypes.c_size_t(0), None, ctypes.c_size_t(0), ctypes.byref(pr), ctypes.byref(ok))
    assert rc == -6 and ok.value == 0                           # CAPGPU_ERR_NOT_INITIALISED
    a, b = ctypes.c_uint64(9), ctypes.c_uint64(9)
    assert L.capgpu_pairing_stats(ctypes.byref(a), ctypes.byref(b)) == 0 and (a.value, b.value) == (0, 0)
    assert L.capgpu_pairing_stats(None, None) == 0
