"""Conformance of the fixed-base MSM at a given form of its tail: every MSM of a launch exactly against the known-tau
identity  MSM(tau-powers[off : off + n], f) = [tau^off f(tau)] G  (f(tau) from the C restatement's poly_eval_fr, or in
closed form with Python integers where all scalars of an MSM are equal), one MSM per case also bit for bit against the C
restatement's Pippenger on the downloaded points.  Before a case compares anything it asserts through cg.msm_plan and
cg.msm_tail_plan that the launch has the form the case was written for (table, parts, item kernels, scan form, digits
kernel, accumulation mode and grid, item length, combine and reduction kernels), and through cg.profile_stats() that the
kernel names this form implies were launched, as often as it implies, and no others of the MSM.

The inputs (INPUTS) reach what uniformly random scalars never do: one crowded bucket per window (all scalars equal: many
work items, the list of heavy buckets), every digit in the TOP bucket (the last element of the last segment, row and
column), a negative digit with a carry in every window up to the top one, every digit in bucket 0, empty upper windows.

Most switches that steer the form are read once per process (msm.hip keeps them in function-local statics), so a forced
configuration is ONE fresh process of this module:

    python -m tools.msm_conformance one_lane          # runs CONFIGS["one_lane"] with its environment, prints one JSON line
    python -m tools.msm_conformance --forms one_lane  # the forms and the sizing of `partial` only: no device needed

Exit code 0: all equal, 1: a mismatch (a form that is not the one the case names counts as one), 3: an exception (a HIP
error among them: nothing more is started on the device after one).  tests/test_gpu_msm_forms.py runs the default
environment in-process and every configuration through this command line; tests/test_msm_tail_plan_abi.py runs --forms."""
import json
import os
import sys
import traceback

import numpy as np

from oracle import bn254 as bn
from oracle import capref as cr

TAU = bn.SplitMix64(0xCA9).field(bn.R)
INPUTS = ["random", "equal", "top_bucket", "top_plus_one", "ones", "half_small"]
CANONICAL = ["random", "equal", "ones", "half_small"]        # inputs below r whatever the window: the Montgomery-form run
EQUAL_K = 0x1F2E3D4C5B6A79880123456789ABCDEF0FEDCBA9876543210011223344556677 % bn.R

SRS_POINTS = {"A": 1024, "B": 50_000, "P": (1 << 18) + 1024}   # c = 9; c = 13 with the wide table; wide only, parts

# every kernel name the fixed-base launch can record in the profile (msm.hip: launch("...")), deep plan aside
ALL_NAMES = ["msm_digits_local", "msm_scan", "msm_scan_chained", "msm_scan_seg", "msm_scan_tot", "msm_scan_add",
             "msm_scatter", "msm_sort_level2", "msm_items", "msm_scan_items", "msm_item_bases", "msm_sort_items",
             "msm_accumulate", "msm_combine", "msm_combine_heavy", "msm_reduce_segments", "msm_reduce_final",
             "msm_reduce_grid", "msm_reduce_grid_final", "msm_reduce_bits", "msm_reduce_bits_final", "msm_sum_parts",
             "msm_fill_inf", "msm_deep_sort_mid", "msm_deep_sort_low"]


def pattern_scalar(c: int, chunk: int) -> int:
    """`chunk` in every c-bit window that lies wholly inside 256 bits (any 256-bit integer is a valid input: the result
    is that of the integer mod r)"""
    return sum(chunk << (c * w) for w in range(256 // c))


def make_scalars(kind: str, c: int, n: int, seed: int):
    """-> ((n, 4) uint64, the common value k when all n scalars are equal, else None)"""
    if kind == "random":
        sc = cr.random_field(seed, 1, n, False)
        for i, v in enumerate((0, 1, bn.R - 1)):
            if i < n:
                sc[i] = cr.int_to_limbs(v)
        return sc, None
    if kind == "half_small":
        sc = cr.random_field(seed ^ 0x5A5A, 1, n, False)
        sc[::2, 1:] = 0
        sc[::2, 0] &= np.uint64(0xFFFF)
        return sc, None
    k = {"equal": EQUAL_K, "top_bucket": pattern_scalar(c, 1 << (c - 1)),
         "top_plus_one": pattern_scalar(c, (1 << (c - 1)) + 1),
         "ones": sum(1 << (c * w) for w in range(253 // c))}[kind]
    assert k < 1 << 256
    limbs = np.frombuffer(k.to_bytes(32, "little"), dtype=np.uint64)
    return np.tile(limbs, (n, 1)), k


def expected_scalar(sc, k, n: int, offset: int) -> int:
    """e with MSM(tau-powers[offset : offset + n], sc) = [e] G"""
    t_off = pow(TAU, offset, bn.R)
    if k is not None:                                      # k (tau^off + ... + tau^(off + n - 1)), Python integers only
        geo = (pow(TAU, n, bn.R) - 1) * pow(TAU - 1, bn.R - 2, bn.R) % bn.R
        return k % bn.R * geo % bn.R * t_off % bn.R
    f_tau = bn.from_mont(cr.poly_eval_fr(cr.vec_to_mont(1, sc), bn.to_mont(TAU, bn.R)), bn.R)
    return f_tau * t_off % bn.R


def expected_launches(plan: dict, tail: dict) -> dict:
    """profile name -> launches of ONE call (a single slice), as the plan and the tail's form imply"""
    e = {"msm_digits_local": 1, "msm_accumulate": 1, "msm_combine": 1}
    if tail["scan"] == "one-block":
        e["msm_scan"] = 1
    elif tail["scan"] == "chained":
        e["msm_scan_chained"] = 1
    else:
        e.update(msm_scan_seg=1, msm_scan_tot=1, msm_scan_add=1)
    e["msm_sort_level2" if plan["sort"] == "two-level" else "msm_scatter"] = 1
    if tail["items"] == "chained":
        e["msm_items"] = 1
    else:
        e.update(msm_scan_items=1, msm_item_bases=1, msm_sort_items=1)
    if tail["combine"] == "bucket" and tail["heavy"]:
        e["msm_combine_heavy"] = 1
    if tail["reduce"] == "segments":
        e.update(msm_reduce_segments=1, msm_reduce_final=1)
    elif tail["reduce"] in ("grid", "grid-quad"):
        e.update(msm_reduce_grid=1, msm_reduce_grid_final=1)
    else:
        e.update(msm_reduce_bits=1, msm_reduce_bits_final=1)
    if plan["parts"] > 1:
        e["msm_sum_parts"] = 1
    return e


def kernels_of(plan: dict, tail: dict) -> list:
    """the kernels (template instantiations told apart) one call of this form launches, in msm.hip's spelling - INFERRED
    from the form (run_tail launches from the same TailForm fields), not observed: the profile has one name for all
    instantiations of a kernel, and that name's launch count is what run_case observes"""
    k = [f"msm_digits_local<{0 if tail['digits'] == 'generic' else tail['digits']}>", "msm_accumulate"]
    k += {"one-block": ["msm_scan<0>"], "chained": ["msm_scan_chained"],
          "seg-tot-add": ["msm_scan_seg", "msm_scan_tot", "msm_scan_add"]}[tail["scan"]]
    k.append("msm_sort_level2" if plan["sort"] == "two-level" else "msm_scatter_runs")
    k += ["msm_items"] if tail["items"] == "chained" else ["msm_scan<1>", "msm_item_bases", "msm_sort_items"]
    if tail["combine"] == "bucket":
        k += ["msm_combine"] + (["msm_combine_heavy"] if tail["heavy"] else [])
    else:
        k.append(f"msm_combine_{tail['combine']}<{tail['combine_lanes']}>")
    if tail["reduce"] == "segments":
        k += ["msm_reduce_segments", "msm_reduce_final_quad" if tail["finish"] == "quad" else "msm_reduce_final"]
    elif tail["reduce"] == "grid-quad":
        k += [f"msm_reduce_grid_quad<{tail['slices']}>", f"msm_reduce_grid_final_quad<{tail['finish'].split('-')[1]}>"]
    elif tail["reduce"] == "grid":
        k += [f"msm_reduce_grid<{tail['slices']}>", "msm_reduce_grid_" + tail["finish"]]
    else:
        k += ["msm_reduce_bits", "msm_reduce_bits_final"]
    if plan["parts"] > 1:
        k.append("msm_sum_parts")
    return k


def form_errors(tail: dict, expect: dict) -> list:
    bad = [f"form: {key}={tail.get(key)!r}, the case was written for {want!r}" for key, want in expect.items()
           if tail.get(key) != want]
    if tail["partial_points"] > tail["partial_reserved"]:
        bad.append(f"form: the reduction writes {tail['partial_points']} points into the {tail['partial_reserved']} reserved")
    return bad


def run_case(cg, handle, n, batch, offset, inputs, expect=None, launch=None, montgomery=False, seed=1):
    """Runs `batch` MSMs of n points at `offset` per call through cg.msm_g1_dev, MSM b of call j holding input
    (j * batch + b) mod len(inputs), in as many calls as it takes to use every input.  expect: the items of
    cg.msm_tail_plan the case was written for; launch: the (c, n_sub, sub_msms, has_parts) it was written for (checked
    against cg.msm_plan).  montgomery: one more call with the canonical inputs in Montgomery form.
    -> {"plan", "tail", "launches": {name: count}, "kernels", "msms", "mismatches": [text, ...]}"""
    plan = cg.msm_plan(handle, n, batch)
    bad = []
    if plan.get("sort") == "deep" or plan["slice"] < batch:
        return {"plan": plan, "tail": {}, "launches": {}, "kernels": [], "msms": 0,
                "mismatches": [f"form: not one batched launch: {plan}"]}
    shape = (plan["c"], plan["n_sub"], batch * plan["parts"], plan["parts"] > 1)
    tail = cg.msm_tail_plan(*shape)
    if launch is not None and tuple(launch) != shape:
        bad.append(f"form: the launch is (c, n_sub, sub_msms, parts) = {shape}, the case was written for {tuple(launch)}")
    if tail.get("bin_buckets", 0) != plan.get("bin_buckets", 0):
        bad.append(f"form: bin_buckets {tail.get('bin_buckets')} in the tail plan, {plan.get('bin_buckets')} in the plan")
    bad += form_errors(tail, expect or {})
    res = {"plan": plan, "tail": tail, "launches": {}, "kernels": kernels_of(plan, tail), "msms": 0, "mismatches": bad}
    if bad:
        return res                                          # not the launch the case is about: nothing is run
    c = plan["c"]
    K = len(inputs)
    calls = (K + batch - 1) // batch
    srs = None
    for j in range(calls + (1 if montgomery else 0)):
        mont = j == calls
        kinds = [k for k in inputs if k in CANONICAL] if mont else inputs
        made, host, want = {}, np.empty((batch, n, 4), dtype=np.uint64), []
        for b in range(batch):
            kind = kinds[(j * batch + b) % len(kinds)]
            key = (kind, b) if kind in ("random", "half_small") else kind        # the random inputs differ per MSM
            if key not in made:
                sc, k = make_scalars(kind, c, n, seed * 100_003 + 97 * j + b)
                made[key] = (sc, expected_scalar(sc, k, n, offset))
            host[b] = made[key][0]
            want.append(made[key][1])
        d = cg.DevBuf.from_numpy(cr.vec_to_mont(1, host.reshape(-1, 4)) if mont else host)
        if j == 0:
            cg.profile_enable(True)
            cg.profile_reset()
        try:
            out = cg.msm_g1_dev(handle, d, n, count=batch, montgomery=mont, offset=offset)
            got = out.to_numpy().reshape(batch, 12)
        finally:
            if j == 0:
                stats = cg.profile_stats()
                cg.profile_enable(False)
        out.free()
        d.free()
        if j == 0:
            res["launches"] = {name: cnt for name, (_ms, cnt) in stats.items() if name.startswith("msm_")}
            exp = expected_launches(plan, tail)
            for name in sorted(set(ALL_NAMES) | set(res["launches"])):
                if res["launches"].get(name, 0) != exp.get(name, 0):
                    bad.append(f"launches: {name} ran {res['launches'].get(name, 0)} times, the form implies {exp.get(name, 0)}")
        want_aff = cr.g1_fixed_base_batch(np.stack([cr.int_to_limbs(e) for e in want]))
        for b in range(batch):
            aff = cr.g1_to_affine(got[b])
            if not np.array_equal(aff, want_aff[b]):
                bad.append(f"call {j}{' (Montgomery)' if mont else ''} MSM {b} ({kinds[(j * batch + b) % len(kinds)]}): "
                           f"differs from [tau^off f(tau)] G")
        res["msms"] += batch
        if j == 0:
            # MSM 0: the expected point once more in Python integers, and the C restatement's Pippenger bit for bit
            if cr.affine_to_ints(cr.g1_to_affine(got[0])) != bn.g1_mul(bn.G1_GEN, want[0]):
                bad.append("call 0 MSM 0: differs from the known-tau point computed in Python integers")
            srs = cg.srs_download(handle, offset, n)
            if not np.array_equal(cr.g1_to_affine(got[0]), cr.g1_to_affine(cr.msm_g1(srs, host[0]))):
                bad.append("call 0 MSM 0: differs from the C restatement's Pippenger on the downloaded points")
    del bad[12:]
    return res


def run_empty(cg, handle, batch=3):
    """MSMs over no points: msm_fill_inf"""
    d = cg.DevBuf.from_numpy(np.zeros((1, 4), np.uint64))
    cg.profile_enable(True)
    cg.profile_reset()
    try:
        out = cg.msm_g1_dev(handle, d, 0, count=batch, stride=0)
        got = out.to_numpy().reshape(batch, 12)
    finally:
        stats = cg.profile_stats()
        cg.profile_enable(False)
    out.free()
    d.free()
    launches = {name: cnt for name, (_ms, cnt) in stats.items() if name.startswith("msm_")}
    bad = [f"MSM {b} over no points is not infinity" for b in range(batch)
           if cr.affine_to_ints(cr.g1_to_affine(got[b])) is not None]
    if launches != {"msm_fill_inf": 1}:
        bad.append(f"launches: {launches}")
    return {"launches": launches, "kernels": ["msm_fill_inf"], "mismatches": bad}


def case(srs, n, batch, offset, launch, montgomery=False, **expect):
    return {"srs": srs, "n": n, "batch": batch, "offset": offset, "launch": launch, "montgomery": montgomery,
            "expect": expect}


P_N = SRS_POINTS["P"]
# ---- the default environment: the smallest shapes that reach each form the default rules select -------------------------
DEFAULT_CASES = {
    # one MSM on 256 buckets: grid-quad 8 with the 64-term finish, eight quads per bucket
    "grid_quad8_c9": case("A", 1000, 1, 24, (9, 1000, 1, False), True, digits="generic", items="chained", scan="one-block",
                          acc="one-shot", item_len=8, combine="quad", combine_lanes=8, reduce="grid-quad", slices=8,
                          finish="quad-64", grid_sums=32),
    # a single proof's launches - 1, 2 and 5 MSMs of 4096 buckets: grid-quad 16, two quads per bucket
    "quad2_1msm": case("B", 2500, 1, 7, (13, 2500, 1, False), True, digits=13, acc="one-shot", acc_grid=41, item_len=8,
                       combine="quad", combine_lanes=2, reduce="grid-quad", slices=16, finish="quad-64", grid_sums=128),
    "quad2_2msm": case("B", 3001, 2, 0, (13, 3001, 2, False), item_len=8, combine="quad", combine_lanes=2,
                       reduce="grid-quad", slices=16, finish="quad-64"),
    "quad2_5msm": case("B", 2999, 5, 1, (13, 2999, 5, False), item_len=32, combine="quad", combine_lanes=2,
                       reduce="grid-quad", slices=16, finish="quad-64"),
    # longer single MSMs: four and eight quads per bucket; the bin table of more than 32768 rows is scanned chained
    "quad4_chained_scan": case("B", 20_000, 1, 30_000, (13, 20_000, 1, False), scan="chained", scan_segments=10, item_len=9,
                               combine="quad", combine_lanes=4, reduce="grid-quad", finish="quad-64"),
    "quad8_chained_scan": case("B", 30_000, 1, 20_000, (13, 30_000, 1, False), scan="chained", scan_segments=15, item_len=13,
                               combine="quad", combine_lanes=8, reduce="grid-quad", finish="quad-64"),
    "chained_scan_10000": case("B", 10_000, 1, 3, (13, 10_000, 1, False), scan="chained", scan_segments=5,
                               items="chained", combine="quad", combine_lanes=4),
    # 24 - 63 MSMs of fewer than 4096 points have no wide table: the one-lane grid with final_small (one thread per bucket:
    # 98304 and more buckets of one item each)
    "one_lane_grid_narrow": case("B", 3000, 40, 5, (13, 3000, 40, False), True, acc="one-shot", acc_grid=933, item_len=32,
                                 combine="bucket", heavy=1, reduce="grid", slices=8, finish="final_small", grid_sums=128),
    # running sums on the narrow tables: from 64 MSMs of 4096 buckets (segments of 16), from 256 of 256 buckets (of 4)
    "segments_narrow": case("B", 1500, 64, 11, (13, 1500, 64, False), True, acc="persistent-counter", acc_grid=1032,
                            combine="bucket", heavy=1, reduce="segments", seg_len=16, segments=256, finish="quad"),
    "segments_c9": case("A", 1000, 256, 0, (9, 1000, 256, False), acc="persistent-counter", acc_grid=1032,
                        combine="bucket", heavy=1, reduce="segments", seg_len=4, segments=64, finish="quad"),
    # the wide table from 24 MSMs of 4096 points: grid-quad 16 with the 128-term finish, one thread per bucket
    "wide_grid_quad": case("B", 4096, 24, 100, (15, 4096, 24, False), True, digits=15, acc="persistent-counter",
                           combine="bucket", heavy=1, reduce="grid-quad", slices=16, finish="quad-128", grid_sums=256),
    # ... and running sums beyond 130 MSMs, with the segment length tuned to the launch (32, not the 64 of large launches)
    "wide_segments_tuned": case("B", 4096, 131, 0, (15, 4096, 131, False), digits=15, combine="bucket", heavy=1,
                                reduce="segments", seg_len=32, segments=512, seg_divides=1, finish="quad"),
    # a table just above 2^18 points holds the wide windows only: 33 parts of 8192 points, the last one of 1024
    "parts_default": case("P", P_N, 1, 0, (15, 8192, 33, True), digits=15, combine="bucket", reduce="grid-quad",
                          finish="quad-128", sums_parts=1),
}

QUAD_OFF = {"CAPGPU_MSM_QUAD_MAX": "0", "CAPGPU_MSM_QUAD_MAX_WIDE": "0"}


def window_cases(c, one, many, lots, count=200):
    """a table of 50 000 points with c-bit windows (CAPGPU_MSM_C): 1, 24 and `count` MSMs"""
    return {"1msm": case("B", 2500, 1, 9, (c, 2500, 1, False), True, digits="generic", **one),
            "24msm": case("B", 2500, 24, 0, (c, 2500, 24, False), digits="generic", **many),
            "many": case("B", 1200, count, 1, (c, 1200, count, False), digits="generic", **lots)}


def small_cases(c, digits, lanes1, kind8, lanes8, len8):
    return {"1msm": case("B", 2500, 1, 0, (c, 2500, 1, False), True, digits=digits, item_len=8, combine=lanes1[0],
                         combine_lanes=lanes1[1], reduce="grid-quad", finish="quad-64"),
            "8msm": case("B", 2500, 8, 77, (c, 2500, 8, False), digits=digits, item_len=len8, combine=kind8,
                         combine_lanes=lanes8, reduce="grid-quad", finish="quad-64")}


def sub_bits_cases(bits):
    return {"24msm": case("B", 4096, 24, 0, (15, 4096, 24, False), True, bin_buckets=1 << bits, reduce="grid-quad"),
            "parts": case("P", P_N, 1, 0, (15, 8192, 33, True), bin_buckets=1 << bits, sums_parts=1)}


ACC_SHAPE = ("B", 2000, 20, 13, (13, 2000, 20, False))   # 106 920 items at most: more than (256 * 1 + 8) workgroups of 256
# ---- forced environments: name -> (environment, cases) ---------------------------------------------------------------
CONFIGS = {
    "one_lane": ({**QUAD_OFF, "CAPGPU_MSM_ITEM_MAX": "8"}, {
        "256_buckets": case("A", 1000, 1, 0, (9, 1000, 1, False), combine="wave", combine_lanes=32, reduce="grid", slices=8,
                            finish="final_small", grid_sums=32),
        "wave8": case("B", 2500, 1, 0, (13, 2500, 1, False), True, item_len=8, combine="wave", combine_lanes=8,
                      reduce="grid", slices=8, finish="final_small", grid_sums=128),
        "wave16": case("B", 12_000, 1, 1, (13, 12_000, 1, False), item_len=8, combine="wave", combine_lanes=16,
                       reduce="grid", finish="final_small"),
        "wave32": case("B", 20_000, 1, 2, (13, 20_000, 1, False), item_len=8, combine="wave", combine_lanes=32,
                       reduce="grid", finish="final_small"),
        "wave64": case("B", 50_000, 1, 0, (13, 50_000, 1, False), item_len=8, combine="wave", combine_lanes=64,
                       reduce="grid", finish="final_small"),
        "16384_buckets": case("B", 4096, 24, 3, (15, 4096, 24, False), item_len=8, combine="bucket", heavy=1,
                              reduce="grid", slices=8, finish="final", grid_sums=256)}),
    "grid_slices": ({**QUAD_OFF, "CAPGPU_MSM_GRID_SLICES": "64"}, {
        "slices16_c9": case("A", 1000, 1, 0, (9, 1000, 1, False), reduce="grid", slices=16, finish="final_small"),
        "slices16": case("B", 2500, 20, 0, (13, 2500, 20, False), reduce="grid", slices=16, finish="final_small"),
        "slices32": case("B", 2500, 12, 0, (13, 2500, 12, False), reduce="grid", slices=32, finish="final_small"),
        "slices64": case("B", 2500, 1, 0, (13, 2500, 1, False), True, reduce="grid", slices=64, finish="final_small")}),
    "bit_planes": ({"CAPGPU_MSM_GRID_REDUCE": "0"}, {
        "8_chunks": case("B", 2500, 1, 0, (13, 2500, 1, False), True, combine="wave", combine_lanes=8, reduce="bits",
                         planes=13, chunks=8),
        "1_chunk_wide": case("B", 4096, 24, 0, (15, 4096, 24, False), combine="bucket", reduce="bits", planes=15, chunks=1),
        "1_chunk_c9": case("A", 1000, 1, 5, (9, 1000, 1, False), reduce="bits", planes=9, chunks=1)}),
    "final_one_lane": ({"CAPGPU_MSM_QUAD_FINAL": "0"}, {
        "narrow": case("B", 1500, 64, 0, (13, 1500, 64, False), True, reduce="segments", seg_len=16, finish="one-lane"),
        "wide": case("B", 4096, 131, 0, (15, 4096, 131, False), reduce="segments", seg_len=32, finish="one-lane")}),
    "seg_tune0": ({"CAPGPU_MSM_SEG_TUNE": "0"}, {
        "wide": case("B", 4096, 131, 0, (15, 4096, 131, False), True, reduce="segments", seg_len=64, segments=256,
                     seg_divides=1)}),
    # 300 MSMs of 1024 points on a table of 15-bit windows: 432 segments of 38 buckets, the last one of 6
    "seg_tune1": ({"CAPGPU_MSM_SEG_TUNE": "1", "CAPGPU_MSM_C": "15"}, {
        "wide": case("B", 1024, 300, 0, (15, 1024, 300, False), True, reduce="segments", seg_len=38, segments=432,
                     seg_divides=0, finish="quad")}),
    "heavy_off": ({"CAPGPU_MSM_HEAVY_COMBINE": "0"}, {
        "narrow": case("B", 1500, 64, 11, (13, 1500, 64, False), True, combine="bucket", heavy=0, reduce="segments")}),
    "unchained": ({"CAPGPU_MSM_CHAINED": "0"}, {
        "long_scan": case("B", 10_000, 1, 3, (13, 10_000, 1, False), True, items="separate", scan="seg-tot-add",
                          scan_segments=5),
        "wide": case("B", 4096, 24, 0, (15, 4096, 24, False), items="separate", scan="one-block")}),
    "acc_one_shot": ({"CAPGPU_ACC_PERSISTENT": "0"}, {
        "narrow": case("B", 1500, 64, 0, (13, 1500, 64, False), True, acc="one-shot", acc_grid=1259, acc_threads=256)}),
    "acc_counter": ({"CAPGPU_ACC_PERSISTENT": "1"}, {
        "k1": case(*ACC_SHAPE, True, acc="persistent-counter", acc_grid=264, acc_threads=256)}),
    "acc_stride": ({"CAPGPU_ACC_PERSISTENT": "1", "CAPGPU_ACC_DYNAMIC": "0"}, {
        "k1": case(*ACC_SHAPE, True, acc="persistent-stride", acc_grid=264, acc_threads=256)}),
    "acc_threads64": ({"CAPGPU_ACC_THREADS": "64"}, {
        "counter": case(*ACC_SHAPE, True, acc="persistent-counter", acc_grid=1032, acc_threads=64),
        "one_shot": case("B", 2500, 1, 0, (13, 2500, 1, False), acc="one-shot", acc_grid=162, acc_threads=64)}),
    "acc_threads128": ({"CAPGPU_ACC_THREADS": "128"}, {
        "one_shot": case(*ACC_SHAPE, True, acc="one-shot", acc_grid=836, acc_threads=128)}),
    "item_max8": ({"CAPGPU_MSM_ITEM_MAX": "8"}, {
        "long": case("B", 50_000, 1, 0, (13, 50_000, 1, False), True, item_len=8, combine="wave", combine_lanes=64,
                     reduce="grid-quad"),
        "5msm": case("B", 2500, 5, 0, (13, 2500, 5, False), item_len=8, combine="quad", combine_lanes=2)}),
    "item_min4": ({"CAPGPU_MSM_ITEM_MIN": "4", "CAPGPU_MSM_ITEM_SMALL": "0"}, {
        "short": case("B", 2500, 1, 0, (13, 2500, 1, False), True, item_len=4, combine="quad", combine_lanes=2),
        "long": case("B", 50_000, 1, 0, (13, 50_000, 1, False), item_len=4, combine="wave", combine_lanes=64)}),
    "item_waves4": ({"CAPGPU_MSM_ITEM_WAVES": "4"}, {
        "long": case("B", 50_000, 1, 0, (13, 50_000, 1, False), True, item_len=8, combine="wave", combine_lanes=64)}),
    "item_small_buckets0": ({"CAPGPU_MSM_ITEM_SMALL_BUCKETS": "0"}, {
        "short": case("B", 2500, 1, 0, (13, 2500, 1, False), True, item_len=32, combine="quad", combine_lanes=2),
        "long": case("B", 50_000, 1, 0, (13, 50_000, 1, False), item_len=32, combine="quad", combine_lanes=4)}),
    "c9": ({"CAPGPU_MSM_C": "9"}, window_cases(
        9, dict(combine="wave", combine_lanes=64, reduce="grid-quad", slices=8, finish="quad-64"),
        dict(item_len=36, combine="wave", combine_lanes=16, reduce="grid", finish="final_small"),
        dict(combine="wave", combine_lanes=8, reduce="grid", finish="final_small"))),
    "c10": ({"CAPGPU_MSM_C": "10"}, window_cases(
        10, dict(combine="quad", combine_lanes=8, reduce="grid-quad", slices=8, finish="quad-64", grid_sums=48),
        dict(combine="wave", combine_lanes=8, reduce="grid", finish="final_small", grid_sums=48),
        dict(combine="wave", combine_lanes=8, reduce="grid", finish="final_small"))),
    "c12": ({"CAPGPU_MSM_C": "12"}, window_cases(
        12, dict(combine="quad", combine_lanes=2, reduce="grid-quad", slices=16, finish="quad-64", grid_sums=96),
        dict(combine="wave", combine_lanes=8, reduce="grid", finish="final_small", grid_sums=96),
        dict(combine="bucket", heavy=1, reduce="segments", seg_len=16, segments=128))),
    "c14": ({"CAPGPU_MSM_C": "14"}, window_cases(
        14, dict(combine="quad", combine_lanes=2, reduce="grid-quad", slices=16, finish="quad-128", grid_sums=192),
        dict(combine="bucket", heavy=1, reduce="grid-quad", slices=16, finish="quad-128", grid_sums=192),
        dict(combine="bucket", heavy=1, reduce="segments", seg_len=16, segments=512), count=131)),
    # 17 windows (the 17th takes the carry) and 32768 buckets, which no grid form takes
    "c16": ({"CAPGPU_MSM_C": "16"}, window_cases(
        16, dict(windows=17, combine="wave", combine_lanes=8, reduce="bits", planes=16, chunks=16),
        dict(windows=17, combine="bucket", heavy=1, reduce="bits", planes=16, chunks=1),
        dict(windows=17, combine="bucket", heavy=1, reduce="segments", seg_len=38, segments=863, seg_divides=0),
        count=150)),
    "wide_off": ({"CAPGPU_MSM_WIDE": "0"}, {
        "40msm": case("B", 4096, 40, 0, (13, 4096, 40, False), True, digits=13, combine="bucket", heavy=1, reduce="grid",
                      slices=8, finish="final_small")}),
    "wide_c14": ({"CAPGPU_MSM_WIDE_C": "14"}, {
        "24msm": case("B", 4096, 24, 0, (14, 4096, 24, False), True, digits="generic", reduce="grid-quad", slices=16,
                      finish="quad-128", grid_sums=192),
        "131msm": case("B", 4096, 131, 0, (14, 4096, 131, False), reduce="segments", seg_len=16, segments=512)}),
    "wide_c16": ({"CAPGPU_MSM_WIDE_C": "16"}, {
        "24msm": case("B", 4096, 24, 0, (16, 4096, 24, False), True, digits="generic", windows=17, reduce="bits", planes=16,
                      chunks=1),
        "70msm": case("B", 4096, 70, 0, (16, 4096, 70, False), windows=17, reduce="segments", seg_len=32, segments=1024)}),
    "wide_min1": ({"CAPGPU_MSM_WIDE_MIN": "1"}, {
        "lone": case("B", 4096, 1, 17, (15, 4096, 1, False), True, digits=15, combine="quad", combine_lanes=2,
                     reduce="grid-quad", slices=16, finish="quad-128")}),
    "sub_bits5": ({"CAPGPU_MSM_SUB_BITS": "5"}, sub_bits_cases(5)),
    "sub_bits6": ({"CAPGPU_MSM_SUB_BITS": "6"}, sub_bits_cases(6)),
    "sub_bits7": ({"CAPGPU_MSM_SUB_BITS": "7"}, sub_bits_cases(7)),
    "small_c9": ({"CAPGPU_MSM_SMALL_C": "9", "CAPGPU_MSM_SMALL_MAX": "8"},
                 small_cases(9, "generic", ("wave", 64), "wave", 64, 11)),
    "small_c10": ({"CAPGPU_MSM_SMALL_C": "10", "CAPGPU_MSM_SMALL_MAX": "8"},
                  small_cases(10, "generic", ("quad", 8), "quad", 8, 11)),
    "small_c11": ({"CAPGPU_MSM_SMALL_C": "11", "CAPGPU_MSM_SMALL_MAX": "8"},
                  small_cases(11, 11, ("quad", 4), "quad", 2, 12)),
    "small_c12": ({"CAPGPU_MSM_SMALL_C": "12", "CAPGPU_MSM_SMALL_MAX": "8"},
                  small_cases(12, "generic", ("quad", 2), "quad", 2, 32)),
    # 16 parts of 17408 points, the last one of 2048
    "split16": ({"CAPGPU_MSM_SPLIT": "16"}, {
        "parts": case("P", P_N, 1, 0, (15, 17_408, 16, True), True, sums_parts=1, reduce="grid-quad", finish="quad-128")}),
    "acc_lds": ({"CAPGPU_ACC_LDS": "65536"}, {
        "one_shot": case(*ACC_SHAPE, True, acc="one-shot", acc_grid=418, acc_lds=65536)}),
}


def run_named(cg, cases, handles):
    """runs the cases of one configuration; handles: {srs name: handle}, filled as tables are needed"""
    out = {}
    for name, cs in cases.items():
        if cs["srs"] not in handles:
            handles[cs["srs"]] = cg.srs_generate(TAU, SRS_POINTS[cs["srs"]])
        out[name] = run_case(cg, handles[cs["srs"]], cs["n"], cs["batch"], cs["offset"], INPUTS, expect=cs["expect"],
                             launch=cs["launch"], montgomery=cs["montgomery"], seed=len(out) + 1)
    return out


def forms_only(cg, cases):
    """the forms and the sizing of `partial` from the tail plan alone (host arithmetic: no device, no table)"""
    out = {}
    for name, cs in cases.items():
        tail = cg.msm_tail_plan(*cs["launch"])
        out[name] = {"tail": tail, "mismatches": form_errors(tail, cs["expect"])}
    return out


def main(argv):
    try:
        from cap_amd import lib as cg
        forms = argv[:1] == ["--forms"]
        name = argv[-1]
        env, cases = ({}, DEFAULT_CASES) if name == "default" else CONFIGS[name]
        missing = {k: v for k, v in env.items() if os.environ.get(k) != v}
        if missing:
            raise RuntimeError(f"configuration {name} needs {missing} in the environment of a fresh process")
        if forms:
            res = forms_only(cg, cases)
        else:
            cg.init(0)
            handles = {}
            res = run_named(cg, cases, handles)
            for h in handles.values():
                cg.srs_free(h)
        print(json.dumps({"config": name, "cases": res}), flush=True)
        return 1 if any(r["mismatches"] for r in res.values()) else 0
    except Exception:
        traceback.print_exc()
        return 3


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
