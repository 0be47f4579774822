"""The solver's DEFERRED form on the host (capgpu_plonk_key_set_solve_form): the rule of cap_amd/csrc/solve_defer.hpp is host
code without HIP, and the fraction rows and the flush group of solve_defer29.hpp build for the host like the row rule.  This
CPU test compiles tests/cpp/solve_defer_check.cpp - a stand-alone program - which solves 300 random circuits, with hints and
under the four flag values, item by item through the direct plan and through the deferred schedule and compares every
variable's image and the reported row limb for limb; meets every case a pending variable can be met in; and checks that the
direct plan's bytes are left alone - with field29.hpp's bound assertions on, plain and under ASan + UBSan.  The Python
restatement of the rule (tests/solve_defer_model.py) is checked here against hand-made circuits whose schedule is known.
(`-m "not gpu"`)"""
import os
import re
import shutil
import subprocess
import types

import pytest

from tests import solve_defer_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _run(tmp_path, cxx, flags):
    exe = str(tmp_path / "solve_defer_check")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-x", "c++"] + flags +
                          [os.path.join(HERE, "cpp", "solve_defer_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "bad=0" in out.stdout, out.stdout[-800:] + out.stderr[-800:]
    m = re.search(r"circuits=(\d+) flags=(\d+)/(\d+)/(\d+)/(\d+) values=(\d+) frac_rows=(\d+) flush_items=(\d+) zero_dens=(\d+) "
                  r"cases: hash=(\d+) hint=(\d+) root_lin=(\d+) two_cells=(\d+) behind_zero=(\d+)", out.stdout)
    assert m, out.stdout[-400:]
    f = [int(x) for x in m.groups()]
    assert f[0] == 300 and f[1:5] == [75] * 4 and f[5] == 300 * 1200
    assert all(x > 0 for x in f[6:]), f                                    # every case was met


def test_deferred_form_on_the_host(tmp_path):
    cxx = next((c for c in ("g++", CLANG, "clang++") if shutil.which(c) or os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    _run(tmp_path, cxx, [])


def test_deferred_form_on_the_host_under_asan_and_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ for the sanitizer build")
    _run(tmp_path, CLANG, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _circuit(rows, num_vars, num_inputs=0):
    """rows: (wires[5], {selector: value}) from row num_inputs on"""
    n = 16
    sc = types.SimpleNamespace(n=n, num_vars=num_vars, num_inputs=num_inputs, selectors=[[0] * n for _ in range(13)],
                               wire_vars=[[0] * n for _ in range(5)])
    for j, (w, sel) in enumerate(rows, start=num_inputs):
        for i in range(5):
            sc.wire_vars[i][j] = w[i]
        for s, x in sel.items():
            sc.selectors[s][j] = x
    return sc


def test_the_model_of_the_rule_on_circuits_with_a_known_schedule():
    ecc, mul, root = {M.Q_ECC: 1, M.Q_O: 1}, {M.Q_O: 1, M.Q_LC: 1}, {M.Q_HASH: 1, M.Q_O: 1}
    # a chain of three additions' rows 10 -> 11 -> 12, a select on a pending input (13), then a fifth root that reads 13
    # (flush), a second chain 15 -> 16 behind it and the final flush.  Given: 0 .. 4.
    sc = _circuit([([1, 2, 3, 4, 10], ecc), ([10, 10, 3, 4, 11], ecc), ([11, 2, 3, 4, 12], ecc), ([12, 1, 0, 0, 13], mul),
                   ([14, 1, 2, 3, 13], root), ([14, 2, 3, 4, 15], ecc), ([15, 15, 15, 4, 16], ecc), ([1, 2, 0, 0, 17], mul)], 20)
    m = M.defer_model(sc, [0, 1, 2, 3, 4], [], 0)
    assert m["deferred"] == [10, 11, 12, 13, 15, 16] and m["flush_before"] == [4, 7] and m["flush_sizes"] == [4, 2]
    assert m["masks"] == {0: 0, 1: 0b0011, 2: 0b0001, 3: 0b0001, 5: 0, 6: 0b0111} and m["slots"] == 4
    assert m["info_deferred"] == dict(form=1, deferred_vars=6, frac_rows=6, flush_levels=2, flush_items=2, levels=9,
                                      inv_levels_direct=5, inv_levels_deferred=2)
    assert m["info_direct"] == dict(form=0, deferred_vars=0, frac_rows=0, flush_levels=0, flush_items=0, levels=7,
                                    inv_levels_direct=5, inv_levels_deferred=2)
    # a pending variable on a hash cell of an OUT row flushes; the same variable on a cell without q_hash does not
    hashed = dict(mul)
    hashed[M.Q_HASH + 1] = 1
    sc = _circuit([([1, 2, 3, 4, 10], ecc), ([10, 1, 0, 0, 11], hashed), ([11, 10, 0, 0, 12], hashed)], 20)
    m = M.defer_model(sc, [0, 1, 2, 3, 4], [], 0)
    assert m["deferred"] == [10, 11] and m["flush_before"] == [2] and m["masks"] == {0: 0, 1: 0b0001}
    # hints: a pending source flushes, an INV0 level counts on both sides
    rows = [([1, 2, 3, 4, 10 + k], ecc) for k in range(10)]
    sc = _circuit(rows, 300)
    m = M.defer_model(sc, [0, 1, 2, 3, 4], [(M.HINT_INV0, 12, [40]), (M.HINT_BITS, 1, list(range(50, 90)))], 0)
    assert m["flush_before"] == [1] and m["flush_sizes"] == [10] and m["info_deferred"]["flush_items"] == 1
    assert m["info_deferred"]["inv_levels_direct"] == 2 and m["info_deferred"]["inv_levels_deferred"] == 2
    assert m["info_deferred"]["levels"] == 3
    assert M.GROUP == 32                                                   # sd::kGroup: pairs per flush item
