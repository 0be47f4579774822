#!/usr/bin/env python3
"""Measurements of the witness solver (capgpu_plonk_solve_vars_dev, kernel k_solve_vars) on cap_like_circuit("transfer_2x2"),
n = 2^15: 2 425 given values per witness, 18 193 defined ones, 584 levels, 5 840 inversions.
  (a) solve     capgpu_plonk_solve_vars_dev at 1, 256, 1024 and 4096 resident witnesses: wall time per call and the
                kernel's own time (capgpu_profile_dump);
  (b) cpu_fill  capwit_fill_many on 16 threads for 256 witnesses - the CPU figure.  The harness inverts on EVERY defining
                row (18 193 inversions per witness where the solver inverts on 5 840 and multiplies by a constant on the
                rest), so this arm flatters the device;
  (c) solve_prove  solve + plonk_prove_batch_dev(vars) of 256 from resident given values, against
      host_vars    plonk_prove_batch(vars) of 256 host-resident variable-form witnesses (context 0, like the other arm).
  (d) --packed: the solve arms at every witnesses-per-workgroup setting (capgpu_plonk_set_solve_pack 1, 2, 4, 8, 16 and 0 =
      automatic; arm solve_<count>_w<setting>, "auto" for 0) instead of (a), and the proving arms from given values:
      prove_given_256          one synchronous plonk_prove_given of 256 from resident given values, context 0;
      prove_given_async_2x256  plonk_prove_given_async of 256 host-resident given values, two tickets kept in flight from an
                               unbound thread (a call = one ticket: wait for the oldest, submit the next);
      host_vars_async_2x256    the same with plonk_prove_multi_async(vars) of 256 host-resident value vectors - its comparison;
      beside solve_prove_256 and host_vars_prove_256 as above.  Default --out profiles/solve_packed.txt.
  (e) --hinted: cap_like_hinted_circuit("transfer_2x2") - scalars, amounts and roots given; bits, inverses and zero flags
      hinted (capgpu_plonk_key_set_given_hints) - beside the unhinted model in ONE session, arms interleaved:
      solve_<count> / solve_<count>_hinted at --counts (default 1,256,4096) and prove_given_256 / prove_given_256_hinted
      from resident given values.  Prints each key's given count, bytes per proof, capgpu_solver_info and capgpu_hint_info.
      Default --out profiles/solve_hints.txt.
  (f) a comparison of two LIBRARIES (CAPGPU_LIBRARY names the one a process loads): one process per library and turn, each
      with --label NAME --append --out FILE, e.g. for NAME in parent_1 tree_1 parent_2 tree_2
          python tools/gpu_solve_ab.py --counts 256,4096 --arms solve_256,solve_4096 --label NAME --append --out profiles/solve_hints_ab.txt
      then  python tools/gpu_solve_ab.py --ab-summary profiles/solve_hints_ab.txt  appends each label's medians and spreads.
  --arms a,b runs those arms only (no summary lines), --reps N instead of three repetitions, --no-profile leaves the
  library's kernel timer off: for a run of one arm under an external profiler.
Protocol: per arm 3 warm-up + 10 timed calls, the arms interleaved, three repetitions; the median of the three medians and
their spread (max - min over the median).  One process, the library loaded first (no torch).  Writes the lines it prints to
--out (default profiles/solve_vars.txt).   python tools/gpu_solve_ab.py [--out FILE] [--counts 1,256,1024,4096] [--steps 10]"""
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

P, WARM, DISTINCT = 256, 3, 64


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def hinted_main():
    steps, reps = int(arg("--steps", 10)), int(arg("--reps", 3))
    counts = [int(c) for c in arg("--counts", "1,256,4096").split(",")]
    out = open(arg("--out", os.path.join(ROOT, "profiles", "solve_hints.txt")), "w")

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    cg.init(0)
    cg.set_device(0)
    tau = bu.SplitMix64(0xCA9).field()
    top = max(counts + [P])
    idx = np.arange(top) % DISTINCT
    blind = np.stack([bu.to_mont_array(bu.blinders(7000 + i)) for i in range(P)])
    msgs = [b"ab"] * P
    keys = {}
    srs = None
    for name in ("", "_hinted"):
        if name:
            sc, given, hints = bu.cap_like_hinted_circuit("transfer_2x2")
            gv = np.stack([bu.to_mont_array(bu.cap_like_given_values(sc, 5000 + i)) for i in range(DISTINCT)])
        else:
            sc = bu.cap_like_circuit("transfer_2x2")
            given, hints = [0, 1] + list(sc.free_vars), []
            w, _ = sc.witnesses_mont(np.arange(5000, 5000 + DISTINCT, dtype=np.uint64), threads=16)
            vals = np.zeros((DISTINCT, sc.num_vars, 4), np.uint64)
            vals[:, np.array(sc.wire_vars).reshape(-1)] = w.reshape(DISTINCT, 5 * sc.n, 4)
            vals[:, 0], vals[:, 1] = bu.to_mont_array([0])[0], bu.to_mont_array([1])[0]
            gv = np.ascontiguousarray(vals[:, given])
        n, nv = sc.n, sc.num_vars
        srs = srs if srs is not None else cg.srs_generate(tau, n + 3)
        pk, _ = cg.plonk_preprocess_vars(srs, n, sc.num_inputs, sc.selectors_mont(), np.array(sc.wire_vars, dtype=np.int64), nv)
        t0 = time.perf_counter()
        info, hinfo = cg.plonk_key_set_given_hints(pk, given, hints)
        set_s = time.perf_counter() - t0
        at = {v: k for k, v in enumerate(given)}
        pubs = np.ascontiguousarray(gv[idx[:P]][:, [at[v] for v in sc.pub_vars]])
        d_given = cg.DevBuf.from_numpy(gv[idx])
        d_vars = cg.DevBuf(top * nv * 32)
        # every solved witness passes the witness check (once, outside every timed part)
        _, st = cg.plonk_solve_vars(pk, d_given.view(0, P * len(given) * 32), P, out=d_vars)
        faults = cg.plonk_check_witness_batch(pk, d_vars.view(0, P * nv * 32), pubs, P, input_form="vars")
        assert all(s.kind == 0 for s in st) and all(f.kind == 0 for f in faults)
        cg.plonk_reserve_given(pk, P, slot=-1)
        keys[name] = (pk, len(given), nv, pubs, d_given, d_vars)
        emit({"circuit": "transfer_2x2" + name, "n": n, "num_vars": nv, "gate_rows": sc.gate_rows, "num_hints": len(hints),
              "solver_info": info.as_dict(), "hint_info": hinfo.as_dict(), "set_given_s": round(set_s, 3),
              "bytes_per_proof": {"given": len(given) * 32, "vars": nv * 32, "columns": 5 * n * 32}, "steps": steps, "warmup": WARM})

    def solve_arm(name, count):
        pk, ng, _, _, d_given, d_vars = keys[name]
        g = d_given.view(0, count * ng * 32)

        def run(k):
            for _ in range(k):
                cg.plonk_solve_vars(pk, g, count, out=d_vars)
        return run

    def prove_arm(name):
        pk, ng, _, pubs, d_given, _ = keys[name]
        g = d_given.view(0, P * ng * 32)

        def run(k):
            for _ in range(k):
                cg.plonk_prove_given([pk] * P, g, pubs, blind, msgs)
        return run

    arms = [(f"solve_{c}{name}", solve_arm(name, c), c) for c in counts for name in keys]
    arms += [(f"prove_given_256{name}", prove_arm(name), P) for name in keys]
    only = arg("--arms", None)
    if only:
        arms = [a for a in arms if a[0] in only.split(",")]
    call_ms = {name: [] for name, _, _ in arms}
    for rep in range(reps):
        for name, fn, count in arms:
            fn(WARM)
            t0 = time.perf_counter()
            fn(steps)
            dt = time.perf_counter() - t0
            call_ms[name].append(1e3 * dt / steps)
            emit({"arm": name, "rep": rep, "witnesses": count, "call_ms": round(1e3 * dt / steps, 3)})
    med = {k: statistics.median(v) for k, v in call_ms.items()}
    emit({"median_call_ms": {k: round(v, 3) for k, v in med.items()},
          "spread_rel": {k: round((max(v) - min(v)) / med[k], 4) for k, v in call_ms.items()},
          "hinted_over_unhinted_call_time": {a: round(med[a + "_hinted"] / med[a], 4) for a in med if a + "_hinted" in med},
          "solve_stats": cg.plonk_solve_stats()})
    for pk, _, _, _, d_given, d_vars in keys.values():
        d_given.free()
        d_vars.free()
        cg.plonk_free_key(pk)
    cg.srs_free(srs)
    cg.shutdown()
    out.close()


def ab_summary(path):
    """per label and arm of a file of labelled runs: the median of the repetitions' call times and their spread"""
    calls = {}
    for line in open(path):
        r = json.loads(line)
        if "label" in r and "arm" in r:
            calls.setdefault(f"{r['label']}_{r['arm']}", []).append(r["call_ms"])
    summary = {k: {"median_call_ms": statistics.median(v), "spread_rel": round((max(v) - min(v)) / statistics.median(v), 4)}
               for k, v in sorted(calls.items())}
    line = json.dumps({"ab_summary": summary})
    print(line)
    with open(path, "a") as out:
        out.write(line + "\n")


def main():
    if "--ab-summary" in sys.argv:
        return ab_summary(arg("--ab-summary", None))
    if "--hinted" in sys.argv:
        return hinted_main()
    steps = int(arg("--steps", 10))
    counts = [int(c) for c in arg("--counts", "1,256,1024,4096").split(",")]
    packed = "--packed" in sys.argv
    out_path = arg("--out", os.path.join(ROOT, "profiles", "solve_packed.txt" if packed else "solve_vars.txt"))
    out = open(out_path, "a" if "--append" in sys.argv else "w")
    label = arg("--label", None)

    def emit(obj):
        line = json.dumps({"label": label, **obj} if label else obj)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    cg.init(0)
    cg.set_device(0)
    sc = bu.cap_like_circuit("transfer_2x2")
    n, ni, nv = sc.n, sc.num_inputs, sc.num_vars
    tau = bu.SplitMix64(0xCA9).field()
    srs = cg.srs_generate(tau, n + 3)
    wv = np.array(sc.wire_vars, dtype=np.int64)
    pk, _ = cg.plonk_preprocess_vars(srs, n, ni, sc.selectors_mont(), wv, nv)
    given = [0, 1] + list(sc.free_vars)
    t0 = time.perf_counter()
    info = cg.plonk_key_set_given(pk, given)
    set_given_s = time.perf_counter() - t0
    seeds = np.arange(5000, 5000 + DISTINCT, dtype=np.uint64)
    w, p = sc.witnesses_mont(seeds, threads=16)
    vals = np.zeros((DISTINCT, nv, 4), np.uint64)
    vals[:, wv.reshape(-1)] = w.reshape(DISTINCT, 5 * n, 4)
    vals[:, 0], vals[:, 1] = bu.to_mont_array([0])[0], bu.to_mont_array([1])[0]
    gv = np.ascontiguousarray(vals[:, given])
    emit({"circuit": "transfer_2x2", "n": n, "num_vars": nv, "solver_info": info.as_dict(), "set_given_s": round(set_given_s, 3),
          "bytes_per_witness": {"given": len(given) * 32, "vars": nv * 32, "columns": 5 * n * 32}, "steps": steps, "warmup": WARM})

    top = max(counts + [P])
    idx = np.arange(top) % DISTINCT
    d_given = cg.DevBuf.from_numpy(gv[idx])
    d_vars = cg.DevBuf(top * nv * 32)
    # the result is the generator's assignment (checked once, outside every timed part)
    _, st = cg.plonk_solve_vars(pk, d_given.view(0, P * len(given) * 32), P, out=d_vars)
    got = d_vars.to_numpy(count=P * nv * 4).reshape(P, nv, 4)
    assert all(s.kind == 0 for s in st) and np.array_equal(got[:, wv.reshape(-1)].reshape(P, 5, n, 4), w[idx[:P]])
    pubs = np.ascontiguousarray(p[idx[:P]])
    blind = np.stack([bu.to_mont_array(bu.blinders(7000 + i)) for i in range(P)])
    host_vars = np.ascontiguousarray(vals[idx[:P]])
    cg.plonk_reserve(pk, P, "vars", slot=0)
    if packed:
        cg.plonk_reserve_given(pk, P, slot=-1)
    host_given = np.ascontiguousarray(gv[idx[:P]])
    msgs = [b"ab"] * P

    def solve_arm(count, w=None):
        g = d_given.view(0, count * len(given) * 32)

        def run(k):
            if w is not None:
                cg.plonk_set_solve_pack(w)
            try:
                for _ in range(k):
                    cg.plonk_solve_vars(pk, g, count, out=d_vars)
            finally:
                cg.plonk_set_solve_pack(0)
        return run

    def prove_given(k):
        g = d_given.view(0, P * len(given) * 32)
        for _ in range(k):
            cg.plonk_prove_given([pk] * P, g, pubs, blind, msgs)

    def in_flight(submit):
        """k tickets, two kept in flight, from an unbound thread (a bound thread's tickets all run on its context)"""
        def run(k):
            cg.set_device(-1)
            try:
                live = [submit()]
                for i in range(k):
                    if i + 1 < k:
                        live.append(submit())
                    assert live.pop(0).wait() is not None
            finally:
                cg.set_device(0)
        return run

    given_async = in_flight(lambda: cg.plonk_prove_given_async([pk] * P, host_given, pubs, blind, msgs))
    vars_async = in_flight(lambda: cg.plonk_prove_multi_async([pk] * P, host_vars, pubs, blind, msgs, input_form="vars"))

    def cpu_fill(k):
        for _ in range(k):
            sc.witnesses_mont(np.arange(9000, 9000 + P, dtype=np.uint64), threads=16)

    def solve_prove(k):
        g = d_given.view(0, P * len(given) * 32)
        for _ in range(k):
            cg.plonk_solve_vars(pk, g, P, out=d_vars)
            cg.plonk_prove_batch_dev(pk, d_vars.view(0, P * nv * 32), pubs, blind, b"ab", P, input_form="vars")

    def host_vars_arm(k):
        for _ in range(k):
            cg.plonk_prove_batch(pk, host_vars, pubs, blind, b"ab", P, input_form="vars")

    if packed:
        arms = [(f"solve_{c}_w{w or 'auto'}", solve_arm(c, w), c) for c in counts for w in (1, 2, 4, 8, 16, 0)]
        arms += [("prove_given_256", prove_given, P), ("prove_given_async_2x256", given_async, P),
                 ("host_vars_async_2x256", vars_async, P)]
    else:
        arms = [(f"solve_{c}", solve_arm(c), c) for c in counts] + [("cpu_fill_256_16_threads", cpu_fill, P)]
    arms += [("solve_prove_256", solve_prove, P), ("host_vars_prove_256", host_vars_arm, P)]
    only = arg("--arms", None)
    if only:
        arms = [a for a in arms if a[0] in only.split(",")]
    reps, timer = int(arg("--reps", 3)), "--no-profile" not in sys.argv
    call_ms = {name: [] for name, _, _ in arms}
    kern_ms = {name: [] for name, _, _ in arms}
    cg.profile_enable(timer)
    for rep in range(reps):
        for name, fn, count in arms:
            fn(WARM)
            cg.profile_reset()
            t0 = time.perf_counter()
            fn(steps)
            dt = time.perf_counter() - t0
            solver = [v for name_, v in cg.profile_stats().items() if name_.startswith("k_solve_vars")]
            k_ms, k_n = sum(v[0] for v in solver), sum(v[1] for v in solver)
            call_ms[name].append(1e3 * dt / steps)
            kern_ms[name].append(k_ms / k_n if k_n else 0.0)
            emit({"arm": name, "rep": rep, "witnesses": count, "call_ms": round(1e3 * dt / steps, 3),
                  "witnesses_per_s": round(count * steps / dt, 1), "k_solve_vars_ms": round(k_ms / k_n, 3) if k_n else None})
    cg.profile_enable(False)
    med = {k: statistics.median(v) for k, v in call_ms.items()}
    if not only:
        emit({"median_call_ms": {k: round(v, 3) for k, v in med.items()},
              "spread_rel": {k: round((max(v) - min(v)) / med[k], 4) for k, v in call_ms.items()},
              "median_k_solve_vars_ms": {k: round(statistics.median(v), 3) for k, v in kern_ms.items() if any(v)},
              "witnesses_per_s": {name: round(count / med[name] * 1e3, 1) for name, _, count in arms},
              "solve_prove_over_host_vars": round(med["solve_prove_256"] / med["host_vars_prove_256"], 4)})
    if packed and not only:
        top_count = max(counts)
        emit({"given_tickets_over_vars_tickets_proofs_per_s": round(med["host_vars_async_2x256"] / med["prove_given_async_2x256"], 4),
              "spread_rel_of_the_two": [round((max(call_ms[a]) - min(call_ms[a])) / med[a], 4)
                                        for a in ("prove_given_async_2x256", "host_vars_async_2x256")],
              f"solve_{top_count}_auto_over_w1_call_time": round(med[f"solve_{top_count}_wauto"] / med[f"solve_{top_count}_w1"], 4),
              "prove_given_over_solve_prove": round(med["prove_given_256"] / med["solve_prove_256"], 4),
              "prove_given_over_host_vars": round(med["prove_given_256"] / med["host_vars_prove_256"], 4),
              "solve_stats": cg.plonk_solve_stats()})
    for d in (d_given, d_vars):
        d.free()
    cg.plonk_free_key(pk)
    cg.srs_free(srs)
    cg.shutdown()
    out.close()


if __name__ == "__main__":
    main()
