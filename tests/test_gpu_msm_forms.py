"""The fixed-base MSM at every form its launch switches select: every MSM of every launch exactly against the known-tau
identity, one per case bit for bit against the C restatement's Pippenger, after asserting through cg.msm_plan and
cg.msm_tail_plan that the shape reached the form the case was written for and through cg.profile_stats() that the kernels
this form implies - and no others - were launched (tools/msm_conformance.py holds the cases, the inputs and the checks).

What the earlier MSM tests leave out: they run in the default environment only, where run_tail never picks the bit
planes, the one-lane msm_reduce_final and msm_reduce_grid_final, msm_reduce_grid<16 | 32 | 64>, the wave combines, the
separate item and scan kernels, msm_combine walking a many-item bucket itself, a segment length that does not divide the
bucket count, the fixed-stride and the 64- and 128-thread msm_accumulate, the run-time window size of msm_digits_local
(windows of 10, 12, 14 and 16 bits; c = 16 with its 17th window and 32768 buckets) or the small-launch table.
No default-environment case reaches msm_combine_wave<G>: the default launches of 24 - 63 narrow MSMs have 98304 and more
buckets of about one item each and take the one-thread-per-bucket combine, so the wave combines run in the forced
children only (one_lane, item_*, bit_planes, c*, small_c9).

The default environment runs in this process.  The switches are read once per process, so each forced environment is ONE
fresh child (python -m tools.msm_conformance NAME), one at a time, each under its own time limit; after a child that ended
by a signal, at its limit, with an exception (a HIP error among them) or in any way but a clean 0 or 1, no further child
is started and the remaining cases fail with that reason.  Nothing is tried twice.

Time limits: five times the child's wall time measured on the MI355X, not below 60 s.  MEASURED_S below holds the measured
wall times per configuration (seconds, on the MI355X: start-up, the tables and the oracle's share included)."""
import json
import os
import subprocess
import sys
import time

import pytest

from tools import msm_conformance as mc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH_PREFIXES = ("CAPGPU_MSM_", "CAPGPU_ACC_")

# every kernel of msm.hip from the scans on (the deep sort and the one-shot variable-base MSM, which have tests of their
# own, aside), template instantiations told apart, and a case that launches it: (configuration, case).  Which
# instantiation a case launched is inferred from its tail plan (mc.kernels_of) - run_tail dispatches on the same fields -
# and not measured: the profile shares one name among the instantiations; what is measured is that this name was launched.
COVERED_BY = {
    "msm_digits_local<0>": ("default", "grid_quad8_c9"),
    "msm_digits_local<11>": ("small_c11", "1msm"),
    "msm_digits_local<13>": ("default", "quad2_1msm"),
    "msm_digits_local<15>": ("default", "wide_grid_quad"),
    "msm_scatter_runs": ("default", "grid_quad8_c9"),
    "msm_sort_level2": ("default", "wide_grid_quad"),
    "msm_scan<0>": ("default", "grid_quad8_c9"),
    "msm_scan<1>": ("unchained", "long_scan"),
    "msm_scan_seg": ("unchained", "long_scan"),
    "msm_scan_tot": ("unchained", "long_scan"),
    "msm_scan_add": ("unchained", "long_scan"),
    "msm_scan_chained": ("default", "quad4_chained_scan"),
    "msm_item_bases": ("unchained", "long_scan"),
    "msm_sort_items": ("unchained", "long_scan"),
    "msm_items": ("default", "grid_quad8_c9"),
    "msm_accumulate": ("default", "grid_quad8_c9"),
    "msm_combine": ("default", "one_lane_grid_narrow"),
    "msm_combine_heavy": ("default", "one_lane_grid_narrow"),
    "msm_combine_quad<2>": ("default", "quad2_1msm"),
    "msm_combine_quad<4>": ("default", "quad4_chained_scan"),
    "msm_combine_quad<8>": ("default", "grid_quad8_c9"),
    "msm_combine_wave<8>": ("one_lane", "wave8"),
    "msm_combine_wave<16>": ("one_lane", "wave16"),
    "msm_combine_wave<32>": ("one_lane", "wave32"),
    "msm_combine_wave<64>": ("one_lane", "wave64"),
    "msm_reduce_segments": ("default", "segments_narrow"),
    "msm_reduce_final_quad": ("default", "segments_narrow"),
    "msm_reduce_final": ("final_one_lane", "narrow"),
    "msm_reduce_grid_quad<8>": ("default", "grid_quad8_c9"),
    "msm_reduce_grid_quad<16>": ("default", "quad2_1msm"),
    "msm_reduce_grid_final_quad<64>": ("default", "grid_quad8_c9"),
    "msm_reduce_grid_final_quad<128>": ("default", "wide_grid_quad"),
    "msm_reduce_grid<8>": ("default", "one_lane_grid_narrow"),
    "msm_reduce_grid<16>": ("grid_slices", "slices16"),
    "msm_reduce_grid<32>": ("grid_slices", "slices32"),
    "msm_reduce_grid<64>": ("grid_slices", "slices64"),
    "msm_reduce_grid_final_small": ("default", "one_lane_grid_narrow"),
    "msm_reduce_grid_final": ("one_lane", "16384_buckets"),
    "msm_reduce_bits": ("bit_planes", "8_chunks"),
    "msm_reduce_bits_final": ("bit_planes", "8_chunks"),
    "msm_sum_parts": ("default", "parts_default"),
    "msm_fill_inf": ("default", "empty"),
}

_handles = {}
_default = {}          # case -> result of the default environment, run once


def switches_set():
    return sorted(k for k in os.environ if k.startswith(SWITCH_PREFIXES))


def default_case(cg, name):
    """in this process - or, when the suite itself runs with one of the switches set, in a child without them"""
    if name not in _default and switches_set():
        _default.update(run_config("default"))
    if name not in _default:
        cs = mc.DEFAULT_CASES[name]
        if cs["srs"] not in _handles:
            _handles[cs["srs"]] = cg.srs_generate(mc.TAU, mc.SRS_POINTS[cs["srs"]])
        _default[name] = mc.run_case(cg, _handles[cs["srs"]], cs["n"], cs["batch"], cs["offset"], mc.INPUTS,
                                     expect=cs["expect"], launch=cs["launch"], montgomery=cs["montgomery"],
                                     seed=1 + list(mc.DEFAULT_CASES).index(name))
    return _default[name]


@pytest.fixture(scope="module", autouse=True)
def free_tables():
    yield
    if _handles:
        from cap_amd import lib
        for h in _handles.values():
            lib.srs_free(h)
        _handles.clear()


@pytest.mark.parametrize("name", list(mc.DEFAULT_CASES))
def test_default_environment_forms(cg, name):
    """the smallest shapes that reach each form the default rules select"""
    res = default_case(cg, name)
    cs = mc.DEFAULT_CASES[name]
    assert not res["mismatches"], "\n".join(res["mismatches"])
    calls = -(-len(mc.INPUTS) // cs["batch"]) + (1 if cs["montgomery"] else 0)
    assert res["msms"] == calls * cs["batch"] and res["launches"]


def test_no_points_is_infinity(cg):
    if "A" not in _handles:
        _handles["A"] = cg.srs_generate(mc.TAU, mc.SRS_POINTS["A"])
    _default["empty"] = mc.run_empty(cg, _handles["A"])
    assert not _default["empty"]["mismatches"], _default["empty"]["mismatches"]


@pytest.mark.parametrize("c", [2, 5, 8])
def test_windows_the_tile_format_cannot_hold_are_refused(cg, tau, c):
    """CAPGPU_MSM_C below 9 means more than 31 windows, one more than a tile entry's 5-bit window field counts: the table is
    refused with a clean error - the SRS's and the Lagrange-form commit key's alike -, nothing is left behind, and the next
    call without the switch works"""
    from oracle import capref as cr
    old = os.environ.get("CAPGPU_MSM_C")
    os.environ["CAPGPU_MSM_C"] = str(c)
    try:
        with pytest.raises(cg.CapGpuError) as e:
            cg.srs_generate(tau, 2048)
        assert e.value.code == -1 and "CAPGPU_MSM_C" in str(e.value) and "9..16" in str(e.value)
    finally:
        if old is None:
            del os.environ["CAPGPU_MSM_C"]
        else:
            os.environ["CAPGPU_MSM_C"] = old
    if old is not None:
        return
    h = cg.srs_generate(tau, 2048)
    try:
        assert cg.msm_plan(h, 2048, 1)["c"] == 13
        import numpy as np
        sc = cr.random_field(40 + c, 1, 2048, False)
        want = cr.g1_to_affine(cr.msm_g1(cg.srs_download(h, 0, 2048), sc))
        assert np.array_equal(cr.g1_to_affine(cg.msm_g1(h, sc)), want)
        # the Lagrange-form key of the 2^10 domain is a table of its own, built at its first use: refused under the switch
        # (and not remembered as failed), built without it - the constant polynomial 1 commits to the generator
        from cap_amd import bench_utils as bu
        from oracle import bn254 as bn
        ones = np.tile(bu.to_mont_array([1])[0], (1024, 1))
        os.environ["CAPGPU_MSM_C"] = str(c)
        try:
            with pytest.raises(cg.CapGpuError) as e:
                cg.lagrange_commit(h, 10, ones)
            assert e.value.code == -1 and "CAPGPU_MSM_C" in str(e.value) and "9..16" in str(e.value)
        finally:
            del os.environ["CAPGPU_MSM_C"]
        assert cr.affine_to_ints(cr.g1_to_affine(cg.lagrange_commit(h, 10, ones))) == bn.G1_GEN
    finally:
        cg.srs_free(h)


# ---- forced environments: one fresh child each -------------------------------------------------------------------
MEASURED_S = {"default": 3.7, "one_lane": 1.5, "grid_slices": 0.7, "bit_planes": 0.7, "final_one_lane": 0.7, "seg_tune0": 0.6,
              "seg_tune1": 0.7, "heavy_off": 0.6, "unchained": 0.9, "acc_one_shot": 0.6, "acc_counter": 0.7,
              "acc_stride": 0.6, "acc_threads64": 0.6, "acc_threads128": 0.6, "item_max8": 1.2, "item_min4": 1.2,
              "item_waves4": 0.9, "item_small_buckets0": 1.0, "c9": 0.7, "c10": 0.7, "c12": 0.8, "c14": 0.8, "c16": 0.8,
              "wide_off": 0.5, "wide_c14": 0.7, "wide_c16": 0.8, "wide_min1": 0.6, "sub_bits5": 2.2, "sub_bits6": 2.2,
              "sub_bits7": 2.3, "small_c9": 0.6, "small_c10": 0.9, "small_c11": 0.7, "small_c12": 0.7, "split16": 2.1,
              "acc_lds": 0.5}
_stopped = []          # the reason no further child is started, once there is one
_results = {}


def time_limit(name):
    return max(60.0, 5 * MEASURED_S[name])


def run_config(name):
    if name in _results:
        return _results[name]
    if _stopped:
        pytest.fail(f"not started: {_stopped[0]}")
    env = {k: v for k, v in os.environ.items() if not k.startswith(SWITCH_PREFIXES)}
    env.update({} if name == "default" else mc.CONFIGS[name][0])
    t0 = time.time()
    try:
        out = subprocess.run([sys.executable, "-m", "tools.msm_conformance", name], cwd=ROOT, env=env,
                             capture_output=True, text=True, timeout=time_limit(name))
        code, stdout, stderr = out.returncode, out.stdout, out.stderr
    except subprocess.TimeoutExpired as e:
        code, stdout, stderr = 124, "", str(e.stderr or b"")[-800:]
    print(f"msm_conformance {name}: wall time {time.time() - t0:.1f} s, exit code {code}")
    if code not in (0, 1):             # a signal (134, 139, -6, -11), the limit (124, 137), an exception (3), anything else
        _stopped.append(f"the child of configuration {name} ended with {code}: {stderr[-800:]}")
        pytest.fail(_stopped[0])
    lines = [json.loads(ln) for ln in stdout.splitlines() if ln.startswith("{")]
    assert lines and lines[-1]["config"] == name, stdout[-400:]
    _results[name] = lines[-1]["cases"]
    return _results[name]


def test_the_configurations_are_all_measured():
    assert set(MEASURED_S) == set(mc.CONFIGS) | {"default"}


def test_every_configuration_has_a_montgomery_form_case():
    """Montgomery-form scalars (msm_g1_dev(..., montgomery=True)) in at least one case of every configuration"""
    for name, (_env, cases) in list(mc.CONFIGS.items()) + [("default", ({}, mc.DEFAULT_CASES))]:
        assert any(cs["montgomery"] for cs in cases.values()), name


@pytest.mark.parametrize("name,case", [(n, c) for n, (_, cases) in mc.CONFIGS.items() for c in cases])
def test_forced_forms(name, case):
    res = run_config(name)
    assert case in res, f"{name}: the child reported nothing for {case}"
    cs = mc.CONFIGS[name][1][case]
    assert not res[case]["mismatches"], "\n".join(res[case]["mismatches"])
    for key, want in cs["expect"].items():                 # (the child asserted it; once more on what it reported)
        assert res[case]["tail"][key] == want, (key, res[case]["tail"])
    calls = -(-len(mc.INPUTS) // cs["batch"]) + (1 if cs["montgomery"] else 0)
    assert res[case]["msms"] == calls * cs["batch"]


def test_heavy_list_off_runs_the_same_launch_as_the_default_with_it(cg):
    """the same shape and inputs with and without msm_combine_heavy (the all-equal input puts 47 items into one bucket
    of every window): both exact, and only the list differs"""
    on, off = default_case(cg, "segments_narrow"), run_config("heavy_off")["narrow"]
    assert on["tail"]["heavy"] == 1 and off["tail"]["heavy"] == 0
    assert on["launches"].get("msm_combine_heavy") == 1 and "msm_combine_heavy" not in off["launches"]
    assert {k: v for k, v in on["launches"].items() if k != "msm_combine_heavy"} == off["launches"]
    assert not on["mismatches"] and not off["mismatches"]


def test_every_kernel_of_the_tail_is_launched_by_a_case(cg):
    """COVERED_BY names a case for every kernel; the case must have launched it - the instantiation is inferred from the
    case's tail plan, the launch of the kernel's profile name is observed - and the union over all cases must be the whole
    list"""
    seen = set()
    for kernel, (config, case) in COVERED_BY.items():
        if config == "default":
            res = _default["empty"] if case == "empty" and "empty" in _default else \
                (mc.run_empty(cg, _handles.setdefault("A", cg.srs_generate(mc.TAU, mc.SRS_POINTS["A"])))
                 if case == "empty" else default_case(cg, case))
        else:
            res = run_config(config)[case]
        assert not res["mismatches"], (kernel, config, case, res["mismatches"])
        assert kernel in res["kernels"], (kernel, config, case, res["kernels"])
        profile_name = {"msm_scan<0>": "msm_scan", "msm_scan<1>": "msm_scan_items", "msm_scatter_runs": "msm_scatter",
                        "msm_reduce_final_quad": "msm_reduce_final", "msm_reduce_grid_final_small": "msm_reduce_grid_final"
                        }.get(kernel, kernel.split("<")[0].replace("_quad", "").replace("_wave", ""))
        assert res["launches"].get(profile_name, 0) >= 1, (kernel, profile_name, res["launches"])
        seen.add(kernel)
    for name in mc.CONFIGS:
        for res in run_config(name).values():
            seen.update(res["kernels"])
    for res in _default.values():
        seen.update(res["kernels"])
    assert seen == set(COVERED_BY), (seen ^ set(COVERED_BY))
