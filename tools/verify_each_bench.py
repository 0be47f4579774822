"""Per-proof verification on the device against the host verifier, on transfer-note proofs (n = 2^15, 27 public inputs,
bench_utils' note shape).  Writes one JSON:
    host_verify_ms_per_proof   capgpu_plonk_verify, one thread (measured on --host-sample proofs)
    host_loop_ms_projected     that x count: what checking every proof one by one costs on one core
    batch_verify_dev_ms        capgpu_plonk_batch_verify_dev on all proofs (one verdict)
    verify_each_dev_ms         capgpu_plonk_verify_each_dev on all proofs (one verdict each), best of --reps
    split                      k_verify_terms / k_pairing_check2 (library HIP-event profiler) and the rest (host
                               transcripts and terms, copies)
    resource_usage             VGPRs / scratch of both kernels (hipcc -Rpass-analysis=kernel-resource-usage), with
                               --resource-usage
    python tools/verify_each_bench.py --count 256 --out profiles/verify_each_r07.json [--resource-usage]"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def resource_usage():
    src = os.path.join(ROOT, "cap_amd", "csrc", "verify_dev.hip")
    out = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                          "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                         capture_output=True, text=True, cwd=os.path.dirname(src))
    res, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: \S*(k_verify_terms|k_pairing_check2)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if cur and m:
            res[cur][m.group(1)] = int(m.group(2))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--host-sample", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--resource-usage", action="store_true")
    a = ap.parse_args()
    from cap_amd import bench_utils as bu
    from cap_amd import lib as cg
    cg.init(0)
    tau = bu.SplitMix64(0xCA9).field()
    sc = bu.note_circuit("transfer_2x2", seed=2)
    srs = cg.srs_generate(tau, sc.n + 3)
    pkh, vk = cg.plonk_preprocess(srs, sc.n, sc.num_inputs, sc.selectors_mont(), sc.sigma_mont())
    h2 = cg.g2_generator()
    bh = cg.g2_mul(h2, tau)
    cnt = a.count
    wit = [sc.witness(3 + i) for i in range(4)]
    wires = np.stack([sc.wires_mont(wit[i % 4][0]) for i in range(cnt)])
    pubs = np.stack([bu.to_mont_array(wit[i % 4][1]) for i in range(cnt)])
    bl = np.stack([bu.to_mont_array(bu.blinders(7000 + i)) for i in range(cnt)])
    proofs = cg.plonk_prove_batch(pkh, wires, pubs, bl, b"memo", cnt)
    vks, pl, msgs = [vk] * cnt, [pubs[i] for i in range(cnt)], [b"memo"] * cnt

    t0 = time.perf_counter()
    host = [cg.plonk_verify(vk, h2, bh, pl[i], proofs[i], b"memo") for i in range(a.host_sample)]
    host_ms = (time.perf_counter() - t0) * 1e3 / a.host_sample
    assert all(host)

    ok_b = cg.plonk_batch_verify(vks, h2, bh, pl, proofs, msgs, on_device=True)  # warm-up (window tables, kernels)
    t0 = time.perf_counter()
    ok_b = cg.plonk_batch_verify(vks, h2, bh, pl, proofs, msgs, on_device=True)
    batch_ms = (time.perf_counter() - t0) * 1e3

    ok = cg.plonk_verify_each(vks, h2, bh, pl, proofs, msgs)  # warm-up
    best, split = None, None
    for _ in range(a.reps):
        cg.profile_enable(True)
        cg.profile_reset()
        t0 = time.perf_counter()
        ok = cg.plonk_verify_each(vks, h2, bh, pl, proofs, msgs)
        ms = (time.perf_counter() - t0) * 1e3
        st = cg.profile_stats()
        cg.profile_enable(False)
        kt = {k: round(st[k][0], 3) for k in ("k_verify_terms", "k_pairing_check2") if k in st}
        if best is None or ms < best:
            best, split = ms, kt
    res = {
        "proofs": cnt, "shape": "transfer_2x2 (n = 2^15, 27 public inputs)",
        "all_verdicts_correct": bool(ok.all()) and bool(ok_b),
        "host_verify_ms_per_proof": round(host_ms, 3), "host_sample": a.host_sample,
        "host_loop_ms_projected": round(host_ms * cnt, 1),
        "batch_verify_dev_ms": round(batch_ms, 3),
        "verify_each_dev_ms": round(best, 3),
        "split_ms": dict(split, host_terms_and_copies=round(best - sum(split.values()), 3)),
        "ratio_to_host_loop": round(best / (host_ms * cnt), 4),
        "ratio_to_batch_verify_dev": round(best / batch_ms, 3),
        "note": "verify_each_dev timed with the library's HIP-event profiler on (kernel split); profile run separate",
    }
    if a.resource_usage:
        res["resource_usage"] = resource_usage()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    cg.plonk_free_key(pkh)
    cg.srs_free(srs)


if __name__ == "__main__":
    main()
