"""capgpu_msm_tail_plan at the C boundary, on a machine without a GPU: the call reports what msm.hip's tail_form decides -
the one function run_tail and msm_run_slice launch from - so these tests pin, as literals, the form of the launches the
product makes, and keep the reduction's writes into `partial` within what ws_layout reserves for every form the
conformance configurations force (tools/msm_conformance.py: CONFIGS), each queried in a fresh child because the switches
are read once per process.  (`-m "not gpu"`)"""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from cap_amd import lib as cg
from tools import msm_conformance as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1
SWITCH_PREFIXES = ("CAPGPU_MSM_", "CAPGPU_ACC_")


def clean_env(add=None):
    """the environment without any of the switches (the suite may itself run with some of them set), plus `add`"""
    env = {k: v for k, v in os.environ.items() if not k.startswith(SWITCH_PREFIXES)}
    env.update(add or {})
    return env


# the default-environment queries of the tests below, answered by ONE child with a clean environment
DEFAULT_SHAPES = ([(13, 4099, 1), (13, 4099, 2), (13, 4099, 5), (15, 32770, 1280), (15, 4096, 40), (15, 65536, 4, True),
                   (13, 3000, 23), (13, 3000, 24), (13, 3000, 63), (13, 3000, 64), (9, 1000, 255), (9, 1000, 256),
                   (15, 4096, 130), (15, 4096, 131), (15, 4096, 256), (15, 4096, 513), (13, 8192, 1), (13, 8193, 1),
                   (13, 2000, 49), (13, 2000, 50)] + [(c, 2048, 1) for c in range(9, 17)])
_default = {}


def default_plan(c, n_sub, sub_msms, has_parts=False):
    if not _default:
        code = ("import json, sys; from cap_amd import lib as cg; "
                "print(json.dumps([cg.msm_tail_plan(*s) for s in json.loads(sys.argv[1])]))")
        out = subprocess.run([sys.executable, "-c", code, json.dumps(DEFAULT_SHAPES)], cwd=ROOT, env=clean_env(),
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-800:]
        for shape, plan in zip(DEFAULT_SHAPES, json.loads(out.stdout.splitlines()[-1])):
            _default[tuple(shape) + (False,) * (4 - len(shape))] = plan
    return _default[(c, n_sub, sub_msms, has_parts)]


def test_symbol_is_exported_and_declared():
    assert hasattr(cg.load(), "capgpu_msm_tail_plan")
    with open(os.path.join(ROOT, "include", "capgpu.h")) as f:
        assert "int capgpu_msm_tail_plan(int c, size_t n_sub, int sub_msms, int has_parts, char* buf, size_t cap);" in f.read()
    with open(os.path.join(ROOT, "bindings", "capgpu-sys", "src", "lib.rs")) as f:
        assert "pub fn capgpu_msm_tail_plan(" in f.read()


def test_bad_arguments_are_refused():
    L = cg.load()
    buf = ctypes.create_string_buffer(1024)
    n, cap = ctypes.c_size_t(4096), ctypes.c_size_t(1024)
    assert L.capgpu_msm_tail_plan(13, n, 1, 0, None, cap) == INVALID_ARG
    assert L.capgpu_msm_tail_plan(13, n, 1, 0, buf, ctypes.c_size_t(0)) == INVALID_ARG
    assert L.capgpu_msm_tail_plan(13, ctypes.c_size_t(0), 1, 0, buf, cap) == INVALID_ARG
    assert L.capgpu_msm_tail_plan(13, n, 0, 0, buf, cap) == INVALID_ARG
    assert L.capgpu_msm_tail_plan(13, n, -3, 0, buf, cap) == INVALID_ARG
    # windows the batched plans cannot run: more than 31 of them (c <= 8), bucket sets beyond 2^15 (c >= 17: the deep plan's)
    for c in (-1, 0, 2, 8, 17, 22, 64):
        assert L.capgpu_msm_tail_plan(c, n, 1, 0, buf, cap) == INVALID_ARG, c
    assert b"9..16" in L.capgpu_last_error()
    for c in range(9, 17):
        assert L.capgpu_msm_tail_plan(c, n, 1, 0, buf, cap) == 0, c
    # a launch beyond what one slice holds (batch_slice: 3 * 2^30 entries), a table of 2^31 entries, a short buffer
    assert L.capgpu_msm_tail_plan(15, ctypes.c_size_t(1 << 16), 4000, 0, buf, cap) == INVALID_ARG
    assert L.capgpu_msm_tail_plan(13, ctypes.c_size_t(1 << 27), 1, 0, buf, cap) == INVALID_ARG
    assert L.capgpu_msm_tail_plan(13, n, 1, 0, buf, ctypes.c_size_t(40)) == INVALID_ARG
    with pytest.raises(cg.CapGpuError):
        cg.msm_tail_plan(8, 4096)


def subset(plan, **want):
    return {k: plan.get(k) for k in want} == want, (plan, want)


def test_default_form_of_a_single_proofs_launches():
    """1, 2 and 5 MSMs of 4096 buckets (n = 2^12 + 3 points): the quad tails from the items to the 64-term finish"""
    for sb, item_len, grid in ((1, 8, 57), (2, 8, 113), (5, 32, 131)):
        p = default_plan(13, 4099, sb)
        ok, why = subset(p, c=13, windows=20, buckets=4096, sub_msms=sb, bin_buckets=0, items="chained", scan="one-block",
                         digits=13, acc="one-shot", acc_threads=256, acc_grid=grid, acc_lds=0, item_len=item_len,
                         combine="quad", combine_lanes=2, heavy=0, reduce="grid-quad", grid_sums=128, slices=16,
                         finish="quad-64", partial_points=131 * sb - (sb - 1), sums_parts=0)
        assert ok, why


def test_default_form_of_the_wire_launch_at_2p15():
    """1280 MSMs of 2^15 + 2 points on the wide table: persistent accumulation from the counter, one thread per bucket with
    the heavy list, running sums over 256 segments of 64 buckets with the quad finish"""
    p = default_plan(15, 32770, 1280)
    ok, why = subset(p, c=15, windows=18, buckets=16384, bin_buckets=128, items="chained", scan="one-block", digits=15,
                     acc="persistent-counter", acc_threads=256, acc_grid=1032, item_len=256, combine="bucket",
                     combine_lanes=1, heavy=1, reduce="segments", seg_len=64, segments=256, seg_divides=1, finish="quad",
                     partial_points=2 * 256 * 1280, partial_reserved=2 * 512 * 1280)
    assert ok, why


def test_default_form_of_a_40_msm_wide_launch_and_of_a_2p16_point_part():
    p = default_plan(15, 4096, 40)
    ok, why = subset(p, digits=15, bin_buckets=128, acc="persistent-counter", acc_grid=1032, item_len=32, combine="bucket",
                     heavy=1, reduce="grid-quad", grid_sums=256, slices=16, finish="quad-128",
                     partial_points=40 * 256 + 2 * 40 + 2, partial_reserved=40 * 259)
    assert ok, why
    p = default_plan(15, 65536, 4, True)
    ok, why = subset(p, digits=15, bin_buckets=64, scan="one-block", scan_rows=16384, acc="one-shot", acc_grid=832,
                     item_len=32, combine="quad", combine_lanes=2, reduce="grid-quad", slices=16, finish="quad-128",
                     sums_parts=1, partial_points=4 * 256 + 8 + 1, partial_reserved=4 * 259)
    assert ok, why


def test_default_thresholds_between_the_forms():
    """where the default rules change form, one launch size either side"""
    one = default_plan
    assert one(13, 3000, 23)["reduce"] == "grid-quad" and one(13, 3000, 24)["reduce"] == "grid"
    assert one(13, 3000, 63)["reduce"] == "grid" and one(13, 3000, 64)["reduce"] == "segments"
    assert one(9, 1000, 255)["reduce"] == "grid" and one(9, 1000, 256)["reduce"] == "segments"
    assert one(15, 4096, 130)["reduce"] == "grid-quad" and one(15, 4096, 131)["reduce"] == "segments"
    # (the tuned segment length is for launches of up to 512 MSMs: 256 of them fill the chip once with segments of 32)
    assert one(15, 4096, 256)["seg_len"] == 32 and one(15, 4096, 513)["seg_len"] == 64
    assert one(13, 8192, 1)["scan"] == "one-block" and one(13, 8193, 1)["scan"] == "chained"
    assert [one(c, 2048, 1)["digits"] for c in range(9, 17)] == ["generic", "generic", 11, "generic", 13, "generic", 15,
                                                                 "generic"]
    # msm_accumulate goes persistent above 256 * 4 + 8 workgroups of 256 items
    assert one(13, 2000, 49)["acc"] == "one-shot" and one(13, 2000, 50)["acc"] == "persistent-counter"


# ---- every form the conformance configurations reach, forced ones in a fresh child each --------------------------------
_forms = {}


def forms_of(name):
    if name not in _forms:
        env = clean_env(None if name == "default" else mc.CONFIGS[name][0])
        out = subprocess.run([sys.executable, "-m", "tools.msm_conformance", "--forms", name], cwd=ROOT, env=env,
                             capture_output=True, text=True, timeout=120)
        assert out.returncode in (0, 1), out.stderr[-800:]
        _forms[name] = json.loads(out.stdout.splitlines()[-1])["cases"]
    return _forms[name]


@pytest.mark.parametrize("name", ["default"] + list(mc.CONFIGS))
def test_reduction_writes_no_more_than_ws_layout_reserves(name):
    """... and the shape of every conformance case has the form the case names (the GPU test asserts the same through the
    SRS handle's plan; here a change of a threshold shows up without a device)"""
    cases = forms_of(name)
    assert set(cases) == set(mc.DEFAULT_CASES if name == "default" else mc.CONFIGS[name][1])
    for case, res in cases.items():
        assert not res["mismatches"], (name, case, res["mismatches"])
        tail = res["tail"]
        assert 0 < tail["partial_points"] <= tail["partial_reserved"], (name, case, tail)


def test_the_configurations_reach_every_reduction_combine_and_accumulate_form():
    seen = {"reduce": set(), "combine": set(), "acc": set(), "scan": set(), "items": set(), "digits": set()}
    for name in ["default"] + list(mc.CONFIGS):
        for res in forms_of(name).values():
            t = res["tail"]
            seen["reduce"].add((t["reduce"], t.get("slices"), t.get("finish")))
            seen["combine"].add((t["combine"], t["combine_lanes"], t["heavy"]))
            seen["acc"].add((t["acc"], t["acc_threads"]))
            for k in ("scan", "items", "digits"):
                seen[k].add(t[k])
    assert seen["reduce"] >= {("segments", None, "quad"), ("segments", None, "one-lane"), ("bits", None, None),
                              ("grid-quad", 8, "quad-64"), ("grid-quad", 16, "quad-64"), ("grid-quad", 16, "quad-128"),
                              ("grid", 8, "final_small"), ("grid", 16, "final_small"), ("grid", 32, "final_small"),
                              ("grid", 64, "final_small"), ("grid", 8, "final")}, seen["reduce"]
    assert seen["combine"] >= {("bucket", 1, 1), ("bucket", 1, 0), ("quad", 2, 0), ("quad", 4, 0), ("quad", 8, 0),
                               ("wave", 8, 0), ("wave", 16, 0), ("wave", 32, 0), ("wave", 64, 0)}, seen["combine"]
    assert seen["acc"] >= {("one-shot", 256), ("persistent-counter", 256), ("persistent-stride", 256),
                           ("persistent-counter", 64), ("one-shot", 64), ("one-shot", 128)}, seen["acc"]
    assert seen["scan"] == {"one-block", "chained", "seg-tot-add"} and seen["items"] == {"chained", "separate"}
    assert seen["digits"] == {"generic", 11, 13, 15}
