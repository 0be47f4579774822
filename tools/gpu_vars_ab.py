#!/usr/bin/env python3
"""Same-session A/B of the evals form against the variable form (CAPGPU_INPUT_VARS) for 256 host-resident witnesses per
step at n = 2^15 on cap_like_circuit("transfer_2x2"), after capgpu_plonk_reserve on every context:
  evals          plonk_prove_batch(256) with the five wire columns (5.24 MB per proof over the link);
  vars           the same call with one value per variable (num_vars x 32 B per proof), gathered on the device;
  evals_tickets  the evals form as two tickets of 128 in flight;
  vars_tickets   the variable form likewise.
Each arm runs 3 warm-up + 10 timed steps; the arms are interleaved and the round is repeated 3 times; the resident rate
(plonk_prove_batch_dev on columns already in device memory) is taken in the same session.  One process, the library loaded
first (no torch).  Prints one JSON line per arm and repetition (proofs/s, witness_bytes_h2d per step, scratch_stats deltas
over the timed part - they must be zero), then the medians and the spread.   python tools/gpu_vars_ab.py [--steps 10]"""
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

P, HALF, WARM = 256, 128, 3


def main():
    steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 10
    cg.init(0)
    sc = bu.cap_like_circuit("transfer_2x2")
    n, ni, nv = sc.n, sc.num_inputs, sc.num_vars
    assert sc.log_n == 15
    tau = bu.SplitMix64(0xCA9).field()
    srs = cg.srs_generate(tau, n + 3)
    wv = np.array(sc.wire_vars, dtype=np.int64)
    pk, _ = cg.plonk_preprocess_vars(srs, n, ni, sc.selectors_mont(), wv, nv)
    w4, p4 = sc.witnesses_mont([3, 4, 5, 6])
    wires = np.ascontiguousarray(w4[np.arange(P) % 4])
    pubs = np.ascontiguousarray(p4[np.arange(P) % 4])
    blind = np.stack([bu.to_mont_array(bu.blinders(7000 + i)) for i in range(P)])
    # one value per variable: what the columns hold, read back through the table (unused ids stay zero)
    v4 = np.zeros((4, nv, 4), np.uint64)
    v4[:, wv.reshape(-1)] = w4.reshape(4, 5 * n, 4)
    assert np.array_equal(v4[:, wv.reshape(-1)].reshape(w4.shape), w4)
    values = np.ascontiguousarray(v4[np.arange(P) % 4])
    inputs = {"evals": wires, "vars": values}
    t0 = time.perf_counter()
    # the unbound call of 256 is cut 144 + 112: every context is sized for the larger part in both forms (that covers the
    # tickets of 128 too); context 0 also for the resident batch of 256
    cg.plonk_reserve(pk, 144, "evals", slot=-1)
    cg.plonk_reserve(pk, 144, "vars", slot=-1)
    cg.plonk_reserve(pk, P, "evals", slot=0)
    print(json.dumps({"reserve_s": round(time.perf_counter() - t0, 3), "scratch_stats": cg.scratch_stats(), "n": n,
                      "num_vars": nv, "bytes_per_proof": {"evals": 5 * n * 32, "vars": nv * 32}}), flush=True)

    def arm_batch(form):
        def run(k):
            for _ in range(k):
                cg.plonk_prove_batch(pk, inputs[form], pubs, blind, b"ab", P, input_form=form)
        return run

    def arm_tickets(form):
        src = inputs[form]
        halves = [(src[h * HALF:(h + 1) * HALF], pubs[h * HALF:(h + 1) * HALF], blind[h * HALF:(h + 1) * HALF]) for h in (0, 1)]

        def run(k):
            flight = []
            for i in range(2 * k):  # 2 k tickets of 128, two in flight at any time
                if len(flight) == 2:
                    assert len(flight.pop(0).wait()) == HALF
                w, p, b = halves[i % 2]
                flight.append(cg.plonk_prove_batch_async(pk, w, p, b, b"ab", HALF, input_form=form))
            for t in flight:
                assert len(t.wait()) == HALF
        return run

    # the two forms give the same proofs (checked once, outside every timed part)
    a = cg.plonk_prove_batch(pk, wires[:4], pubs[:4], blind[:4], b"ab", 4)
    b = cg.plonk_prove_batch(pk, values[:4], pubs[:4], blind[:4], b"ab", 4, input_form="vars")
    assert [bytes(x) for x in a] == [bytes(x) for x in b]

    d_wires = cg.DevBuf.from_numpy(wires)

    def arm_resident(k):
        cg.set_device(0)
        for _ in range(k):
            cg.plonk_prove_batch_dev(pk, d_wires, pubs, blind, b"ab", P)
        cg.set_device(-1)

    arms = (("evals", arm_batch("evals")), ("vars", arm_batch("vars")), ("evals_tickets", arm_tickets("evals")),
            ("vars_tickets", arm_tickets("vars")), ("resident", arm_resident))
    rates = {name: [] for name, _ in arms}
    h2d = {}
    grew = 0
    for rep in range(3):
        for name, fn in arms:
            fn(WARM)
            g0, i0 = cg.scratch_stats(), cg.plonk_input_stats()
            t0 = time.perf_counter()
            fn(steps)
            dt = time.perf_counter() - t0
            g1, i1 = cg.scratch_stats(), cg.plonk_input_stats()
            rate = P * steps / dt
            rates[name].append(rate)
            h2d[name] = (i1["witness_bytes_h2d"] - i0["witness_bytes_h2d"]) // steps
            grew += g1["grow_events"] - g0["grow_events"]
            print(json.dumps({"arm": name, "rep": rep, "proofs_per_s": round(rate, 1), "step_ms": round(1e3 * dt / steps, 2),
                              "witness_bytes_h2d_per_step": h2d[name],
                              "gather_launches": i1["gather_launches"] - i0["gather_launches"],
                              "grow_events": g1["grow_events"] - g0["grow_events"]}), flush=True)
    med = {k: statistics.median(v) for k, v in rates.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in rates.items()}
    print(json.dumps({"median_proofs_per_s": {k: round(v, 1) for k, v in med.items()},
                      "spread_rel": {k: round(v, 4) for k, v in spread.items()},
                      "of_resident": {k: round(v / med["resident"], 4) for k, v in med.items()},
                      "vars_over_evals": round(med["vars"] / med["evals"], 4),
                      "vars_tickets_over_evals_tickets": round(med["vars_tickets"] / med["evals_tickets"], 4),
                      "witness_bytes_h2d_per_step": h2d, "grow_events_in_timed_parts": grew}), flush=True)
    assert grew == 0, "an allocation landed inside a timed part after the reserve"
    d_wires.free()
    cg.plonk_free_key(pk)
    cg.srs_free(srs)
    cg.shutdown()


if __name__ == "__main__":
    main()
