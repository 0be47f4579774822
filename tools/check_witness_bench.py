"""What the device witness check costs next to a proof, on transfer-note witnesses (n = 2^15, 27 public inputs,
bench_utils' note shape), one process, one device.  Writes one JSON:
    check_dev_ms               capgpu_plonk_check_witness_batch_dev on --count resident witnesses: host clock around the
                               call (it ends in a stream synchronise), profiler OFF, best of --reps
    split_ms                   k_check_gates / k_check_copies / k_check_targets from a SEPARATE call with the library's
                               HIP-event profiler on (that call's wall time is reported beside them, not used elsewhere)
    first_check_ms             the first check of the key: derives the selector values and the permutation's index table
    prove_step_ms              capgpu_plonk_prove_batch_dev per call with precheck off / on, interleaved A/B, --steps
                               calls each (medians), and their ratio - the figure to judge
    check_over_step            check_dev_ms / the precheck-off step (both with the profiler off)
    hbm_floor_ms               the bytes the check must read once (wires; the key's tables stay in cache) at --hbm-tbs
    parent_bench_ms_per_step   bench.py's ms_per_step of the parent commit, for reference: passed in with
                               --parent-ms-per-step (this tool cannot run another commit), recorded as given
    resource_usage             VGPRs / scratch / occupancy of the kernels (hipcc -Rpass-analysis=kernel-resource-usage
                               with the Makefile's flags), with --resource-usage
    python tools/check_witness_bench.py --count 256 --out profiles/check_witness_r08.json [--resource-usage]"""
import argparse
import json
import os
import re
import shlex
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("k_check_gates", "k_check_copies", "k_check_targets", "k_perm_index")


def makefile_flags():
    """CXXFLAGS of cap_amd/csrc/Makefile with $(ARCH) filled in: the kernels are reported as the product builds them"""
    mk = open(os.path.join(ROOT, "cap_amd", "csrc", "Makefile")).read()
    arch = re.search(r"^ARCH \?= (\S+)", mk, flags=re.M).group(1)
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, flags=re.M).group(1)
    return shlex.split(flags.replace("$(ARCH)", arch))


def resource_usage():
    src = os.path.join(ROOT, "cap_amd", "csrc", "plonk.hip")
    out = subprocess.run(["/opt/rocm/bin/hipcc"] + makefile_flags() +
                         ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                         capture_output=True, text=True, cwd=os.path.dirname(src))
    res, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            hit = [k for k in KERNELS if k in m.group(1)]
            cur = hit[0] if hit else None
            if cur:
                res[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if cur and m:
            res[cur][m.group(1)] = int(m.group(2))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    # 6.3 TB/s: what a plain float4 copy kernel reaches on an MI355X, 79 % of HBM3E's 8.0 TB/s specification - the rate a
    # kernel that streams its input once can hope for
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="HBM read rate the floor is priced at, TB/s")
    ap.add_argument("--parent-ms-per-step", type=float, default=None,
                    help="bench.py ms_per_step of the parent commit (recorded for reference)")
    ap.add_argument("--out", default="")
    ap.add_argument("--resource-usage", action="store_true")
    a = ap.parse_args()
    from cap_amd import bench_utils as bu
    from cap_amd import lib as cg
    cg.init(0)
    cg.set_device(0)  # one context: the check, the steps and the profiler's split all on the same stream
    tau = bu.SplitMix64(0xCA9).field()
    sc = bu.note_circuit("transfer_2x2", seed=2)
    srs = cg.srs_generate(tau, sc.n + 3)
    pkh, _vk = cg.plonk_preprocess(srs, sc.n, sc.num_inputs, sc.selectors_mont(), sc.sigma_mont())
    cnt = a.count
    wires, pubs = sc.witnesses_mont(np.arange(3, 3 + cnt, dtype=np.uint64))
    bl = np.stack([bu.to_mont_array(bu.blinders(7000 + i)) for i in range(cnt)])
    d = cg.DevBuf.from_numpy(wires)

    def check_ms():
        t0 = time.perf_counter()
        faults = cg.plonk_check_witness_batch(pkh, d, pubs, cnt)
        ms = (time.perf_counter() - t0) * 1e3
        assert all(f.kind == 0 for f in faults)
        return ms

    first_ms = check_ms()
    best = min(check_ms() for _ in range(a.reps))
    cg.profile_enable(True)
    cg.profile_reset()
    profiled_ms = check_ms()
    st = cg.profile_stats()
    cg.profile_enable(False)
    split = {k: round(st[k][0], 3) for k in KERNELS if k in st}

    def step(on):
        cg.plonk_set_precheck(on)
        t0 = time.perf_counter()
        cg.plonk_prove_batch_dev(pkh, d, pubs, bl, b"memo", cnt)
        return (time.perf_counter() - t0) * 1e3

    step(False), step(True)  # warm-up: scratch, tables
    off, on = [], []
    for _ in range(a.steps):
        off.append(step(False))
        on.append(step(True))
    cg.plonk_set_precheck(False)
    off_ms, on_ms = statistics.median(off), statistics.median(on)
    wire_bytes = cnt * 5 * sc.n * 32
    res = {
        "witnesses": cnt, "shape": "transfer_2x2 (n = 2^15, 27 public inputs)",
        "check_dev_ms": round(best, 3),
        "split_ms": dict(split, profiled_call_wall_ms=round(profiled_ms, 3)),
        "first_check_ms": round(first_ms, 3),
        "prove_step_ms": {"precheck_off": round(off_ms, 3), "precheck_on": round(on_ms, 3),
                          "on_over_off": round(on_ms / off_ms, 4), "steps_each": a.steps,
                          "off_all": [round(x, 2) for x in off], "on_all": [round(x, 2) for x in on]},
        "check_over_step": round(best / off_ms, 4),
        "wire_bytes": wire_bytes,
        "hbm_tbs": a.hbm_tbs,
        "hbm_floor_ms": round(wire_bytes / (a.hbm_tbs * 1e12) * 1e3, 3),
        "parent_bench_ms_per_step": a.parent_ms_per_step,
        "note": "one context, one stream; check and prove steps timed with the profiler off, kernel split from a separate "
                "profiled call; the prove steps prove the whole batch on one context (bench.py cuts it over two)",
    }
    if a.resource_usage:
        res["resource_usage"] = resource_usage()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    d.free()
    cg.plonk_free_key(pkh)
    cg.srs_free(srs)


if __name__ == "__main__":
    main()
