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
    python tools/verify_each_bench.py --count 256 --out profiles/verify_each_r07.json [--resource-usage]
With --form-ab: the lane form of the pairing check against the wave form (capgpu_pairing_set_form) in ONE process and one
session - verify_each_dev at counts 1, 2, 64, 256, 4096 in both forms, capgpu_plonk_verify_dev and the host
capgpu_plonk_verify at count 1, batch_verify_dev in both forms at 64 and 256; arms interleaved, 3 warm-up and 10 timed
calls per arm (wall clock, profiler off), three repetitions; medians, the spread of the repetitions' medians and the
kernel split (HIP-event profiler, in calls of their own) as a text table:
    python tools/verify_each_bench.py --form-ab --out profiles/pairing_wave_ab.txt"""
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
        m = re.search(r"Function Name: \S*?(k_verify_terms|k_pairing_check2_wave|k_pairing_check2)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if cur and m:
            res[cur][m.group(1)] = int(m.group(2))
    return res


def form_ab(a, cg, vk, h2, bh, pl, proofs):
    """the --form-ab table (see the top of the file); pl / proofs hold max(a.counts) entries"""
    import statistics
    KERNELS = ("k_verify_terms", "k_pairing_check2", "k_pairing_check2_wave")

    def each(n, form):
        def run():
            cg.pairing_set_form(form)
            try:
                return bool(cg.plonk_verify_each([vk] * n, h2, bh, pl[:n], proofs[:n], [b"memo"] * n).all())
            finally:
                cg.pairing_set_form(cg.PAIRING_LANE)
        return run

    def batch(n, form):
        def run():
            cg.pairing_set_form(form)
            try:
                return cg.plonk_batch_verify([vk] * n, h2, bh, pl[:n], proofs[:n], [b"memo"] * n, on_device=True)
            finally:
                cg.pairing_set_form(cg.PAIRING_LANE)
        return run
    groups = []                                    # (title, [(arm name, callable)]): the arms of a group are interleaved
    for n in a.counts:
        arms = [("verify_each_dev lane", each(n, cg.PAIRING_LANE)), ("verify_each_dev wave", each(n, cg.PAIRING_WAVE))]
        if n == 1:
            arms += [("plonk_verify_dev", lambda: cg.plonk_verify_dev(vk, h2, bh, pl[0], proofs[0], b"memo")),
                     ("plonk_verify (host)", lambda: cg.plonk_verify(vk, h2, bh, pl[0], proofs[0], b"memo"))]
        if n in (64, 256):
            arms += [("batch_verify_dev lane", batch(n, cg.PAIRING_LANE)), ("batch_verify_dev wave", batch(n, cg.PAIRING_WAVE))]
        groups.append((n, arms))
    lines = ["pairing form A/B: transfer_2x2 (n = 2^15, 27 public inputs), one process, arms interleaved,",
             f"{a.warmup} warm-up + {a.timed} timed calls per arm and repetition, {a.ab_reps} repetitions; ms per call (wall",
             "clock, profiler off); spread = max - min of the repetitions' medians; kernel split from separate calls",
             "", f"{'count':>6}  {'arm':<24}{'median':>10}{'spread':>10}   kernels (ms per call, HIP events)"]
    verdict, outcome = [], []
    for n, arms in groups:
        meds = {name: [] for name, _ in arms}
        kern = {name: {} for name, _ in arms}
        for _ in range(a.ab_reps):
            times = {name: [] for name, _ in arms}
            for it in range(a.warmup + a.timed):       # wall clock with the profiler off: what a caller sees
                for name, fn in arms:
                    t0 = time.perf_counter()
                    ok = fn()
                    ms = (time.perf_counter() - t0) * 1e3
                    assert ok, (n, name)
                    if it >= a.warmup:
                        times[name].append(ms)
            for name in times:
                meds[name].append(statistics.median(times[name]))
            for _ in range(a.split_calls):             # the kernel split in calls of their own, not timed
                for name, fn in arms:
                    cg.profile_enable(True)
                    cg.profile_reset()
                    ok = fn()
                    st = cg.profile_stats()
                    cg.profile_enable(False)
                    assert ok, (n, name)
                    for k in KERNELS:
                        if k in st:
                            kern[name].setdefault(k, []).append(st[k][0])
        row = {}
        for name, _ in arms:
            med, spread = statistics.median(meds[name]), max(meds[name]) - min(meds[name])
            row[name] = (med, spread)
            ks = "  ".join(f"{k} {statistics.median(v):.3f}" for k, v in kern[name].items())
            lines.append(f"{n:>6}  {name:<24}{med:>10.3f}{spread:>10.3f}   {ks}")
        (lm, ls), (wm, ws) = row["verify_each_dev lane"], row["verify_each_dev wave"]
        won = "wave" if lm - wm > max(ls, ws) else ("lane" if wm - lm > max(ls, ws) else "no difference")
        outcome.append((n, won))
        verdict.append(f"count {n}: wave {wm:.3f} ms, lane {lm:.3f} ms, margin {lm - wm:+.3f} ms, larger spread "
                       f"{max(ls, ws):.3f} ms -> {won}")
    not_wave = [n for n, won in outcome if won != "wave"]
    lane_from = next((n for k, (n, won) in enumerate(outcome) if all(w == "lane" for _, w in outcome[k:])), None)
    verdict.append("wave form below lane form by more than the larger spread at every count measured" if not not_wave else
                   "wave form NOT below lane form by more than the larger spread at count(s) " + ", ".join(map(str, not_wave)))
    verdict.append(f"lane form wins from count {lane_from} on" if lane_from is not None else
                   f"lane form does not win at any count up to {outcome[-1][0]}: its crossover lies beyond this table")
    lines += [""] + verdict
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form-ab", action="store_true")
    ap.add_argument("--counts", type=lambda v: [int(x) for x in v.split(",")], default=[1, 2, 64, 256, 4096])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timed", type=int, default=10)
    ap.add_argument("--ab-reps", type=int, default=3)
    ap.add_argument("--split-calls", type=int, default=3)
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
    if a.form_ab:
        # 64 distinct proofs, repeated up to the largest count (the verifier does the same work for each entry)
        base = min(64, max(a.counts))
        wires = np.stack([sc.wires_mont(wit[i % 4][0]) for i in range(base)])
        pubs = np.stack([bu.to_mont_array(wit[i % 4][1]) for i in range(base)])
        bl = np.stack([bu.to_mont_array(bu.blinders(7000 + i)) for i in range(base)])
        made = cg.plonk_prove_batch(pkh, wires, pubs, bl, b"memo", base)
        top = max(a.counts)
        form_ab(a, cg, vk, h2, bh, [pubs[i % base] for i in range(top)], [made[i % base] for i in range(top)])
        cg.plonk_free_key(pkh)
        cg.srs_free(srs)
        return
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
