#!/usr/bin/env python3
"""Same-session A/B of the per-proof outcome calls (capgpu_plonk_prove_each*) at the transfer shape (n = 2^15, 27 public
inputs), 256 device-resident witnesses per call, in both transcript modes:
  (i)   all good:      plonk_prove_multi (capgpu_plonk_prove_multi_dev_ex) against plonk_prove_each_dev;
  (ii)  one bad of 256: plonk_prove_each_dev against what a caller does today - plonk_check_witness_batch on the device
        buffer, then plonk_prove_multi of the 255 good ones (from a second, already compacted device buffer: the caller's
        own filtering of 5.24 MB witnesses is NOT charged to that arm);
  (iii) --coalesced:   64 threads call plonk_prove under plonk_set_coalescing, one of them with a bad witness, precheck
        off - run once per library build (CAPGPU_LIBRARY names the other one): ms per round of 64 calls.
Each arm runs 3 warm-up + 10 timed calls; the arms are interleaved and the round is repeated 3 times.  One process, the
library loaded first (no torch).  One JSON line per arm and repetition, then the medians and the spread of the
repetitions' medians; everything is also appended to --out (default profiles/prove_each_ab.txt).
  python tools/gpu_prove_each_ab.py [--steps 10] [--coalesced] [--out FILE]"""
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from cap_amd import bench_utils as bu  # noqa: E402
from cap_amd import lib as cg  # noqa: E402

P, WARM, CALLERS = 256, 3, 64


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    steps = int(arg("--steps", 10))
    out_path = arg("--out", os.path.join(ROOT, "profiles", "prove_each_ab.txt"))
    out = open(out_path, "a")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    cg.init(0)
    log_n, ni = 15, 27
    n = 1 << log_n
    tau = bu.SplitMix64(0xCA9).field()
    srs = cg.srs_generate(tau, n + 3)
    sc = bu.synthetic_circuit(log_n, ni, seed=2 + log_n + ni)
    pk, _ = cg.plonk_preprocess(srs, n, ni, sc.selectors_mont(), sc.sigma_mont())
    wit = [sc.witness(3 + i) for i in range(4)]
    base = [sc.wires_mont(w) for w, _ in wit]
    pubs4 = [bu.to_mont_array(p) for _, p in wit]
    bad_w = base[1].copy()
    bad_w[4, n // 2, 0] ^= np.uint64(1)
    emit({"library": cg.lib_path(), "version": cg.load().capgpu_version().decode(), "steps": steps, "warmup": WARM})

    def run_arms(arms, unit, per_call):
        times = {name: [] for name, _ in arms}
        for rep in range(3):
            for name, fn in arms:
                for _ in range(WARM):
                    fn()
                t = []
                for _ in range(steps):
                    t0 = time.perf_counter()
                    fn()
                    t.append(1e3 * (time.perf_counter() - t0))
                med = statistics.median(t)
                times[name].append(med)
                emit({"arm": name, "rep": rep, "median_ms": round(med, 3), "min_ms": round(min(t), 3),
                      "max_ms": round(max(t), 3), unit: round(per_call / med * 1e3, 1)})
        summary = {}
        for name, v in times.items():
            m = statistics.median(v)
            summary[name] = {"median_ms": round(m, 3), "spread_rel": round((max(v) - min(v)) / m, 4)}
        return summary

    if "--coalesced" in sys.argv:
        # (iii) 64 callers, one bad witness, precheck off
        bl = [bu.to_mont_array(bu.blinders(9000 + t)) for t in range(CALLERS)]
        src = [(bad_w if t == 37 else base[t % 4], pubs4[1] if t == 37 else pubs4[t % 4]) for t in range(CALLERS)]
        errors = []

        def round_of_calls():
            start = threading.Barrier(CALLERS)
            errors.clear()

            def worker(t):
                start.wait()
                try:
                    cg.plonk_prove(pk, src[t][0], src[t][1], bl[t], b"ab")
                except cg.CapGpuError as e:
                    errors.append((t, e.code))

            th = [threading.Thread(target=worker, args=(t,)) for t in range(CALLERS)]
            for x in th:
                x.start()
            for x in th:
                x.join()
            assert errors == [(37, -7)], errors

        for mode in ("host", "device"):
            cg.plonk_set_transcript(mode)
            cg.plonk_set_coalescing(2000, CALLERS)
            c0, b0 = cg.plonk_sync_stats()[0], cg.plonk_coalescing_stats()[0]
            s = run_arms([("coalesced64_one_bad_" + mode, round_of_calls)], "proofs_per_s", CALLERS)
            c1, b1 = cg.plonk_sync_stats()[0], cg.plonk_coalescing_stats()[0]
            cg.plonk_set_coalescing(0)
            emit({"summary": s, "prove_calls": c1 - c0, "gathered_batches": b1 - b0, "rounds": 3 * (WARM + steps)})
    else:
        wires = np.stack([base[i % 4] for i in range(P)])
        pubs = np.stack([pubs4[i % 4] for i in range(P)])
        blind = np.stack([bu.to_mont_array(bu.blinders(7000 + i)) for i in range(P)])
        handles = [pk] * P
        d_good = cg.DevBuf.from_numpy(wires)
        BAD = 101
        wires[BAD] = bad_w
        pubs_bad = pubs.copy()
        pubs_bad[BAD] = pubs4[1]
        d_bad = cg.DevBuf.from_numpy(wires)
        keep = [i for i in range(P) if i != BAD]
        d_255 = cg.DevBuf.from_numpy(wires[keep])
        pubs_255, blind_255 = pubs_bad[keep], blind[keep]
        del wires
        cg.set_device(0)
        cg.plonk_set_precheck(True)
        cg.plonk_reserve(pk, P, "evals", slot=0)    # (sized with the check's scratch too; the check is off while proving)
        cg.plonk_set_precheck(False)

        def multi():
            assert len(cg.plonk_prove_multi(handles, d_good, pubs, blind)) == P

        def each():
            _, oc = cg.plonk_prove_each_dev(handles, d_good, pubs, blind)
            assert all(o.status == 0 for o in oc)

        def each_one_bad():
            _, oc = cg.plonk_prove_each_dev(handles, d_bad, pubs_bad, blind)
            assert [i for i, o in enumerate(oc) if o.status] == [BAD]

        def check_then_multi():
            faults = cg.plonk_check_witness_batch(pk, d_bad, pubs_bad, P)
            assert [i for i, f in enumerate(faults) if f.kind] == [BAD]
            assert len(cg.plonk_prove_multi(handles[:P - 1], d_255, pubs_255, blind_255)) == P - 1

        for mode in ("host", "device"):
            cg.plonk_set_transcript(mode)
            g0 = cg.scratch_stats()
            s1 = run_arms([("multi_dev_all_good_" + mode, multi), ("each_dev_all_good_" + mode, each)], "proofs_per_s", P)
            s2 = run_arms([("each_dev_one_bad_" + mode, each_one_bad), ("check_then_multi_255_" + mode, check_then_multi)],
                          "proofs_per_s", P)
            g1 = cg.scratch_stats()
            a, b = s1["multi_dev_all_good_" + mode]["median_ms"], s1["each_dev_all_good_" + mode]["median_ms"]
            c, d = s2["each_dev_one_bad_" + mode]["median_ms"], s2["check_then_multi_255_" + mode]["median_ms"]
            emit({"transcript": mode, "summary": {**s1, **s2}, "each_over_multi_all_good": round(b / a, 4),
                  "each_over_check_then_multi_one_bad": round(c / d, 4), "grow_events": g1["grow_events"] - g0["grow_events"]})
        for x in (d_good, d_bad, d_255):
            x.free()
    cg.plonk_free_key(pk)
    cg.srs_free(srs)
    cg.shutdown()
    out.close()


if __name__ == "__main__":
    main()
