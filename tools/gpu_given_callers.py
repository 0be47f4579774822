#!/usr/bin/env python3
"""How far gathering moves single-note callers on GIVEN values: cap_amd.io_model.cap_like_io_circuit("transfer_2x2") - the
hinted transfer model at n = 2^15 with derived public inputs - and closed-loop Python threads that each call
plonk_prove_given_io_one for one note, again and again.  Arms, interleaved in ONE session:
  off_<T>                (a) coalescing off: every call is a lone capgpu_plonk_prove_given_io of one witness
  on_direct_<T>          (b) coalescing (500 us, 256), the key's solver in the direct form
  on_deferred_<T>        (b) the same with the deferred-fraction form
  ceiling_tickets        (c) one thread keeping two plonk_prove_given_io_async tickets of 128 in flight
  wire_vars_<T>          (d) the existing pattern: T threads on plonk_prove(input_form='vars') with the whole assignment, coalesced
for T in --threads (default 64,128; (d) at the first only).  Protocol (profiles/prove_compact_ab.txt's): per arm 3 warm-up +
10 timed rounds - a round is one call of every thread (one ticket for (c)); the threads run closed-loop, the clock covers
the timed rounds from a barrier to the last return -, arms interleaved, three repetitions, the median of the three and their
spread (max - min over the median).  (a) pays a whole solve per call and runs --off-steps timed rounds after one warm-up.
Reported per arm: proofs/s, batches and mean batch size, solver launches per batch and capgpu_scratch_stats events inside
the timed part (every context is reserved first with capgpu_plonk_reserve_given); (b)/(c) and (b)/(d); and, from the phase
trace (capgpu_trace_enable) of one extra round of (b), the mean time a leader spends in its window, waiting for a context,
and in the part it runs (packing, solve and proof).  One process, the library loaded first (no torch).
  python tools/gpu_given_callers.py [--out profiles/given_callers.txt] [--threads 64,128] [--steps 10] [--reps 3] [--off-steps 2]"""
import json
import os
import statistics
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from cap_amd import bench_utils as bu  # noqa: E402
from cap_amd import lib as cg  # noqa: E402
from cap_amd.io_model import cap_like_io_circuit  # noqa: E402

WARM, DISTINCT, TICKET, WINDOW = 3, 64, 128, (500, 256)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def counters():
    b, p = cg.plonk_coalescing_stats()
    return {"batches": b, "proofs": p, "launches": cg.plonk_solve_stats()["launches"], "grow_events": cg.scratch_stats()["grow_events"]}


def closed_loop(T, call, warm, steps):
    """T threads, each warm + steps calls of call(t, k) back to back -> (seconds of the timed part, counter deltas, errors)"""
    gate = threading.Barrier(T + 1)
    errors = []

    def worker(t):
        try:
            for k in range(warm):
                call(t, k)
            gate.wait()
            for k in range(steps):
                call(t, warm + k)
        except Exception as e:                                       # noqa: BLE001
            errors.append(repr(e))
            gate.abort()

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
    for th in threads:
        th.start()
    try:
        gate.wait()
    except threading.BrokenBarrierError:
        pass
    c0, t0 = counters(), time.perf_counter()
    for th in threads:
        th.join()
    dt = time.perf_counter() - t0
    c1 = counters()
    return dt, {k: c1[k] - c0[k] for k in c0}, errors


def phases(path):
    """the leaders' phases from a trace dump: mean microseconds from co_lead to co_window_end (window), from there to co_acquired
    (waiting for a part to end and a free context), from co_run to co_run_end (the part: packing, solve, proof)"""
    last, spans = {}, {"window_us": [], "context_wait_us": [], "part_us": [], "part_proofs": []}
    for line in open(path):
        f = line.split()
        if len(f) < 5 or not f[2].startswith("co_"):
            continue
        t, tid, tag = float(f[0]), f[1], f[2]
        if tag == "co_window_end" and (tid, "co_lead") in last:
            spans["window_us"].append(t - last[(tid, "co_lead")])
        if tag == "co_acquired" and (tid, "co_window_end") in last:
            spans["context_wait_us"].append(t - last[(tid, "co_window_end")])
        if tag == "co_run_end" and (tid, "co_run") in last:
            spans["part_us"].append(t - last[(tid, "co_run")])
            spans["part_proofs"].append(int(f[3]))
        last[(tid, tag)] = t
    return {k: round(statistics.mean(v), 1) if v else None for k, v in spans.items()} | {"leaders": len(spans["part_us"])}


def main():
    steps, reps, off_steps = int(arg("--steps", 10)), int(arg("--reps", 3)), int(arg("--off-steps", 2))
    Ts = [int(t) for t in arg("--threads", "64,128").split(",")]
    out = open(arg("--out", os.path.join(ROOT, "profiles", "given_callers.txt")), "w")

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    cg.init(0)
    tau = bu.SplitMix64(0xCA9).field()
    sc, given, hints = cap_like_io_circuit("transfer_2x2")
    n, nv, ni = sc.n, sc.num_vars, sc.num_inputs
    srs = cg.srs_generate(tau, n + 3)
    pk, _ = cg.plonk_preprocess_vars(srs, n, ni, sc.selectors_mont(), np.array(sc.wire_vars, dtype=np.int64), nv)
    cg.plonk_key_set_solver(pk, given, hints, cg.SOLVER_LINEAR | cg.SOLVER_DERIVE_PUBLIC)
    gv = np.stack([bu.to_mont_array(bu.cap_like_given_values(sc, 5000 + i)) for i in range(DISTINCT)])
    blind = np.stack([bu.to_mont_array(bu.blinders(7000 + i)) for i in range(DISTINCT)])
    # the whole assignments and public inputs arm (d) brings, solved once (untimed); every witness proves
    vars_h, st = cg.plonk_solve_vars(pk, gv, DISTINCT)
    pubs = cg.plonk_pub_inputs(pk, vars_h, DISTINCT)
    assert all(s.kind == 0 for s in st)
    idx = np.arange(TICKET) % DISTINCT
    gv_t, bl_t, msgs_t = np.ascontiguousarray(gv[idx]), np.ascontiguousarray(blind[idx]), [b"ab"] * TICKET
    _, outcomes, _, got = cg.plonk_prove_given_io([pk] * TICKET, gv_t, bl_t, msgs_t)
    assert all(o.status == 0 for o in outcomes) and np.array_equal(got, pubs[idx])
    cg.plonk_reserve_given(pk, 256, slot=-1)
    cg.plonk_reserve(pk, 256, "vars", slot=-1)
    emit({"circuit": "transfer_2x2_io", "n": n, "num_vars": nv, "num_given": len(given), "num_inputs": ni, "version": cg.load().capgpu_version().decode(),
          "contexts": cg.device_count(), "coalescing": WINDOW, "steps": steps, "warmup": WARM, "off_steps": off_steps,
          "bytes_per_caller": {"given": 32 * len(given), "vars": 32 * nv}})

    def io_one(t, k):
        i = (t + k) % DISTINCT
        _, o, _, _ = cg.plonk_prove_given_io_one(pk, gv[i], blind[i], b"ab", num_inputs=ni)
        assert o.status == 0

    def wire_vars(t, k):
        i = (t + k) % DISTINCT
        cg.plonk_prove(pk, vars_h[i], pubs[i], blind[i], b"ab", input_form="vars")

    def thread_arm(T, call, window, form, warm, timed):
        def run():
            cg.plonk_key_set_solve_form(pk, form)
            cg.plonk_set_coalescing(*window) if window else cg.plonk_set_coalescing(0)
            try:
                dt, d, errors = closed_loop(T, call, warm, timed)
            finally:
                cg.plonk_set_coalescing(0)
                cg.plonk_key_set_solve_form(pk, cg.SOLVE_FORM_DIRECT)
            assert not errors, errors[:3]
            return T * timed / dt, d
        return run

    def ceiling():
        def submit():
            return cg.plonk_prove_given_io_async([pk] * TICKET, gv_t, bl_t, msgs_t)
        flight = [submit(), submit()]
        done, t0, c0 = 0, None, None
        while done < WARM + steps:
            if done == WARM:
                c0, t0 = counters(), time.perf_counter()
            _, outcomes, _, _ = flight.pop(0).wait()
            assert all(o.status == 0 for o in outcomes)
            flight.append(submit())
            done += 1
        dt = time.perf_counter() - t0
        c1 = counters()
        for tk in flight:
            tk.wait()
        return TICKET * steps / dt, {k: c1[k] - c0[k] for k in c0}

    arms = []
    for T in Ts:
        arms.append((f"off_{T}", thread_arm(T, io_one, None, cg.SOLVE_FORM_DIRECT, 1, off_steps)))
        arms.append((f"on_direct_{T}", thread_arm(T, io_one, WINDOW, cg.SOLVE_FORM_DIRECT, WARM, steps)))
        arms.append((f"on_deferred_{T}", thread_arm(T, io_one, WINDOW, cg.SOLVE_FORM_DEFERRED, WARM, steps)))
    arms.append(("ceiling_tickets", ceiling))
    arms.append((f"wire_vars_{Ts[0]}", thread_arm(Ts[0], wire_vars, WINDOW, cg.SOLVE_FORM_DIRECT, WARM, steps)))
    rate = {name: [] for name, _ in arms}
    last = {}
    for rep in range(reps):
        for name, fn in arms:
            r, d = fn()
            rate[name].append(r)
            last[name] = d
            row = {"arm": name, "rep": rep, "proofs_per_s": round(r, 1), "grow_events": d["grow_events"],
                   "solver_launches": d["launches"]}
            if d["batches"]:
                row |= {"batches": d["batches"], "mean_batch": round(d["proofs"] / d["batches"], 2),
                        "launches_per_batch": round(d["launches"] / d["batches"], 3)}
            emit(row)
    med = {k: statistics.median(v) for k, v in rate.items()}
    summary = {"median_proofs_per_s": {k: round(v, 1) for k, v in med.items()},
               "spread_rel": {k: round((max(v) - min(v)) / med[k], 4) for k, v in rate.items()}}
    for T in Ts:
        for form in ("direct", "deferred"):
            summary[f"on_{form}_{T}_over_ceiling"] = round(med[f"on_{form}_{T}"] / med["ceiling_tickets"], 4)
            summary[f"on_{form}_{T}_over_off"] = round(med[f"on_{form}_{T}"] / med[f"off_{T}"], 2)
    for form in ("direct", "deferred"):
        summary[f"on_{form}_{Ts[0]}_over_wire_vars"] = round(med[f"on_{form}_{Ts[0]}"] / med[f"wire_vars_{Ts[0]}"], 4)
    emit(summary)
    # where the time of a gathered caller goes: the leaders' phases over one extra run of (b)
    for T in Ts:
        for form, tag in ((cg.SOLVE_FORM_DIRECT, "direct"), (cg.SOLVE_FORM_DEFERRED, "deferred")):
            cg.trace_enable(True)
            r, d = thread_arm(T, io_one, WINDOW, form, 1, 4)()
            cg.trace_enable(False)
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "t.trace")
                cg.trace_dump(path)
                emit({"phase_trace": f"on_{tag}_{T}", "proofs_per_s": round(r, 1)} | phases(path))
    cg.plonk_free_key(pk)
    cg.srs_free(srs)
    cg.shutdown()
    out.close()


if __name__ == "__main__":
    main()
