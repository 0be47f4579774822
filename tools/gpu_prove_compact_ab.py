#!/usr/bin/env python3
"""Same-session A/B of batch compaction (capgpu_plonk_set_compaction) at the transfer shape (n = 2^15, 27 public inputs),
256 witnesses per outcome call, the witness check on: compaction off against on, with 0, 1, 32 and 255 of the 256
witnesses refused (the refused slots spread evenly), for
  host_evals   plonk_prove_each of host-resident columns (rows move inside the staging buffer),
  dev_evals    plonk_prove_each_dev of device-resident columns (the survivors are copied: the route kCompactCopyRatio gates),
  dev_vars     plonk_prove_each_dev of device-resident value vectors (rows move inside the gathered columns),
under the host transcript, and dev_evals under the device transcript as well.  Each arm runs 3 warm-up + 10 timed calls;
the two arms are interleaved and the round is repeated 3 times; context 0 is sized ahead.  One process, the library loaded
first (no torch).  One JSON line per arm and repetition, then per row the medians of the repetitions' medians, their
spread, on / off, P' / P, and k_move_rows' own time from one profiled call of the on arm; everything is also appended to
--out (default profiles/prove_compact_ab.txt).
--rows dev_evals:host,.. and --refused 1,2,4 pick rows and counts (with CAPGPU_LIBRARY naming a build made with
-DCAP_COMPACT_COPY_RATIO=<large>, the copy route below the threshold: the measurement the constant is set from).
  python tools/gpu_prove_compact_ab.py [--steps 10] [--out FILE] [--rows form:transcript,..] [--refused k,..]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from cap_amd import bench_utils as bu  # noqa: E402
from cap_amd import lib as cg  # noqa: E402

P, WARM = 256, 3
REFUSED = (0, 1, 32, 255)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def spread(k):
    return [int((i + 0.5) * P / k) for i in range(k)]


def main():
    steps = int(arg("--steps", 10))
    out = open(arg("--out", os.path.join(ROOT, "profiles", "prove_compact_ab.txt")), "a")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    cg.init(0)
    cg.set_device(0)
    sc = bu.cap_like_circuit("transfer_2x2")
    n, ni, nv = sc.n, sc.num_inputs, sc.num_vars
    assert sc.log_n == 15 and ni == 27
    tau = bu.SplitMix64(0xCA9).field()
    srs = cg.srs_generate(tau, n + 3)
    wv = np.array(sc.wire_vars, dtype=np.int64)
    pk, _ = cg.plonk_preprocess_vars(srs, n, ni, sc.selectors_mont(), wv, nv)
    w4, p4 = sc.witnesses_mont([3, 4, 5, 6])
    v4 = np.zeros((4, nv, 4), np.uint64)
    v4[:, wv.reshape(-1)] = w4.reshape(4, 5 * n, 4)
    pubs = np.ascontiguousarray(p4[np.arange(P) % 4])
    blind = np.stack([bu.to_mont_array(bu.blinders(7000 + i)) for i in range(P)])
    handles = [pk] * P
    emit({"library": cg.lib_path(), "version": cg.load().capgpu_version().decode(), "steps": steps, "warmup": WARM, "P": P,
          "n": n, "num_inputs": ni, "num_vars": nv, "refused": list(REFUSED)})
    cg.plonk_set_precheck(True)

    # a witness the check refuses, in either form: one variable of witness 1 changed until a gate fails
    bad_v = bad_w = None
    for var in wv[0, n // 2:n // 2 + 64]:
        cand = v4[1].copy()
        cand[var, 0] ^= np.uint64(1)
        d = cg.DevBuf.from_numpy(cand)
        _, oc = cg.plonk_prove_each_dev([pk], d, p4[1:2], blind[:1], input_form="vars")
        d.free()
        if oc[0].status != 0:
            bad_v, bad_w = cand, cand[wv.reshape(-1)].reshape(5, n, 4)
            break
    assert bad_v is not None, "no variable whose change fails a gate"

    cg.plonk_reserve(pk, P, "evals", slot=0)
    cg.plonk_reserve(pk, P, "vars", slot=0)

    def run_arms(arms):
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
                emit({"arm": name, "rep": rep, "median_ms": round(med, 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)})
        return {name: {"median_ms": round(statistics.median(v), 3),
                       "spread_rel": round((max(v) - min(v)) / statistics.median(v), 4)} for name, v in times.items()}

    rows = [("host_evals", "host"), ("dev_evals", "host"), ("dev_vars", "host"), ("dev_evals", "device")]
    if "--rows" in sys.argv:
        rows = [tuple(r.split(":")) for r in arg("--rows", "").split(",")]
    refused = tuple(int(k) for k in arg("--refused", ",".join(map(str, REFUSED))).split(","))
    for form, mode in rows:
        cg.plonk_set_transcript(mode)
        for k in refused:
            slots = spread(k)
            pubs_k = pubs.copy()
            pubs_k[slots] = p4[1]
            if form == "dev_vars":
                data = np.ascontiguousarray(v4[np.arange(P) % 4])
                data[slots] = bad_v
            else:
                data = np.ascontiguousarray(w4[np.arange(P) % 4])
                data[slots] = bad_w
            dev = None if form == "host_evals" else cg.DevBuf.from_numpy(data)
            if dev is not None:
                del data

            def call():
                if dev is None:
                    _, oc = cg.plonk_prove_each(handles, data, pubs_k, blind)
                else:
                    _, oc = cg.plonk_prove_each_dev(handles, dev, pubs_k, blind, input_form="vars" if form == "dev_vars" else "evals")
                assert [i for i, o in enumerate(oc) if o.status] == slots
                return oc

            def arm(on):
                def fn():
                    cg.plonk_set_compaction(on)
                    call()
                return fn

            name = "%s_%s_refused%d" % (form, mode, k)
            g0, c0 = cg.scratch_stats(), cg.plonk_compaction_stats()
            s = run_arms([(name + "_off", arm(False)), (name + "_on", arm(True))])
            g1, c1 = cg.scratch_stats(), cg.plonk_compaction_stats()
            # k_move_rows' own time: one profiled call of the on arm (HIP events around every launch)
            cg.plonk_set_compaction(True)
            cg.profile_enable(True)
            cg.profile_reset()
            call()
            prof = cg.profile_stats().get("k_move_rows", (0.0, 0))
            cg.profile_enable(False)
            cg.plonk_set_compaction(False)
            off, on = s[name + "_off"], s[name + "_on"]
            emit({"row": name, "off_ms": off["median_ms"], "on_ms": on["median_ms"], "off_spread_rel": off["spread_rel"],
                  "on_spread_rel": on["spread_rel"], "on_over_off": round(on["median_ms"] / off["median_ms"], 4),
                  "survivors_over_P": round((P - k) / P, 4), "k_move_rows_ms": round(prof[0], 4), "k_move_rows_launches": prof[1],
                  "compacted_calls": c1[0] - c0[0], "rows_moved_per_call": (c1[2] - c0[2]) // max(c1[0] - c0[0], 1),
                  "grow_events": g1["grow_events"] - g0["grow_events"]})
            if dev is not None:
                dev.free()
    cg.plonk_set_precheck(False)
    cg.plonk_free_key(pk)
    cg.srs_free(srs)
    cg.shutdown()
    out.close()


if __name__ == "__main__":
    main()
