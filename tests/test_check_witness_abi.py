"""The witness-check entry points of include/capgpu.h: struct layout, and - like every compute entry point - a loud
refusal without a device.  (`-m "not gpu"`)"""
import ctypes

import numpy as np

from cap_amd import lib as cg


def test_witness_fault_layout_matches_the_header():
    F = cg.WitnessFault
    assert ctypes.sizeof(F) == 48
    offsets = {name: getattr(F, name).offset for name, _ in F._fields_}
    assert offsets == {"kind": 0, "wire": 4, "wire2": 8, "reserved": 12, "row": 16, "row2": 24, "gates_failed": 32,
                       "copies_failed": 40}


def test_fault_text_is_the_oracles_wording():
    f = cg.WitnessFault(kind=1, row=1234)
    assert str(f) == "gate 1234 not satisfied"
    f = cg.WitnessFault(kind=2, wire=2, row=40, wire2=0, row2=7)
    assert str(f) == "copy constraint (2,40) -> (0,7) violated"
    assert str(cg.WitnessFault()) == ""


def test_check_entry_points_refuse_without_a_device():
    from tests import helpers as H
    L = cg.load()
    assert L.capgpu_plonk_set_precheck(1) == 0 and L.capgpu_plonk_set_precheck(0) == 0
    if H.gpu_present():
        return  # the refusal path belongs to the CPU-only runner; the GPU suite exercises the calls themselves
    data = np.zeros(5 * 16 * 4, dtype=np.uint64)
    faults = (cg.WitnessFault * 1)()
    handle = ctypes.c_uint64(1)
    handles = (ctypes.c_uint64 * 1)(1)
    zero = ctypes.c_size_t(0)
    p = data.ctypes.data_as(cg.u64p)
    assert L.capgpu_plonk_check_witness(handle, p, None, zero, 0, faults) == -6
    assert b"not initialised" in L.capgpu_last_error()
    assert L.capgpu_plonk_check_witness_batch(handle, 1, p, None, zero, 0, faults) == -6
    assert L.capgpu_plonk_check_witness_batch_dev(handle, 1, ctypes.c_void_p(16), None, zero, 0, faults) == -6
    assert L.capgpu_plonk_check_witness_multi(handles, 1, p, None, zero, 0, faults) == -6
