#!/usr/bin/env python3
"""Same-session A/B of the three ways to prove 256 host-resident witnesses per step at n = 2^15 (transfer shape, 27 public
inputs), after capgpu_plonk_reserve on every context:
  sync     plonk_prove_batch(256) from one unbound thread (the library cuts it over two contexts: bench.py's pcie_inclusive);
  tickets  one thread keeping two tickets of 128 in flight (plonk_prove_batch_async / Ticket.wait);
  threads  two threads bound to contexts 0 and 1 (set_device), 128 per call each.
Each arm runs 3 warm-up + 10 timed steps; the arms are interleaved and the round is repeated 3 times.  One process, the
library loaded first (no torch).  Prints one JSON line per arm and repetition (proofs/s, scratch_stats deltas over the timed
part - they must be zero -, async_stats), then the medians and the spread.   python tools/gpu_async_ab.py [--steps 10]"""
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

P, HALF, WARM = 256, 128, 3


def main():
    steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 10
    cg.init(0)
    log_n, ni = 15, 27
    n = 1 << log_n
    tau = bu.SplitMix64(0xCA9).field()
    srs = cg.srs_generate(tau, n + 3)
    sc = bu.synthetic_circuit(log_n, ni, seed=2 + log_n + ni)
    pk, _ = cg.plonk_preprocess(srs, n, ni, sc.selectors_mont(), sc.sigma_mont())
    wit = [sc.witness(3 + i) for i in range(4)]
    wires = np.stack([sc.wires_mont(wit[i % 4][0]) for i in range(P)])
    pubs = np.stack([bu.to_mont_array(wit[i % 4][1]) for i in range(P)])
    blind = np.stack([bu.to_mont_array(bu.blinders(7000 + i)) for i in range(P)])
    halves = [(wires[h * HALF:(h + 1) * HALF], pubs[h * HALF:(h + 1) * HALF], blind[h * HALF:(h + 1) * HALF]) for h in (0, 1)]
    # the unbound call of 256 is cut 144 + 112: every context is sized for the larger part, which covers the halves too
    t0 = time.perf_counter()
    cg.plonk_reserve(pk, 144, "evals", slot=-1)
    print(json.dumps({"reserve_s": round(time.perf_counter() - t0, 3), "scratch_stats": cg.scratch_stats(),
                      "contexts": cg.device_count()}), flush=True)

    def arm_sync(k):
        for _ in range(k):
            cg.plonk_prove_batch(pk, wires, pubs, blind, b"ab", P)

    def arm_tickets(k):
        flight = []
        for i in range(2 * k):  # 2 k tickets of 128, two in flight at any time
            if len(flight) == 2:
                assert len(flight.pop(0).wait()) == HALF
            w, p, b = halves[i % 2]
            flight.append(cg.plonk_prove_batch_async(pk, w, p, b, b"ab", HALF))
        for t in flight:
            assert len(t.wait()) == HALF

    def arm_threads(k):
        def body(slot):
            cg.set_device(slot)
            w, p, b = halves[slot]
            for _ in range(k):
                cg.plonk_prove_batch(pk, w, p, b, b"ab", HALF)
        th = [threading.Thread(target=body, args=(s,)) for s in (0, 1)]
        for x in th:
            x.start()
        for x in th:
            x.join()

    arms = (("sync", arm_sync), ("tickets", arm_tickets), ("threads", arm_threads))
    rates = {name: [] for name, _ in arms}
    grew = 0
    for rep in range(3):
        for name, fn in arms:
            fn(WARM)
            g0, a0 = cg.scratch_stats(), cg.async_stats()
            t0 = time.perf_counter()
            fn(steps)
            dt = time.perf_counter() - t0
            g1, a1 = cg.scratch_stats(), cg.async_stats()
            rate = P * steps / dt
            rates[name].append(rate)
            grew += g1["grow_events"] - g0["grow_events"]
            print(json.dumps({"arm": name, "rep": rep, "proofs_per_s": round(rate, 1), "step_ms": round(1e3 * dt / steps, 2),
                              "grow_events": g1["grow_events"] - g0["grow_events"],
                              "grow_bytes": g1["grow_bytes"] - g0["grow_bytes"],
                              "grow_ms": round(g1["grow_ms"] - g0["grow_ms"], 3),
                              "tickets": a1["completed"] - a0["completed"], "max_running": a1["max_running"]}), flush=True)
    med = {k: statistics.median(v) for k, v in rates.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in rates.items()}
    print(json.dumps({"median_proofs_per_s": {k: round(v, 1) for k, v in med.items()},
                      "spread_rel": {k: round(v, 4) for k, v in spread.items()},
                      "tickets_over_sync": round(med["tickets"] / med["sync"], 4),
                      "tickets_over_threads": round(med["tickets"] / med["threads"], 4),
                      "grow_events_in_timed_parts": grew}), flush=True)
    assert grew == 0, "an allocation landed inside a timed part after the reserve"
    cg.plonk_free_key(pk)
    cg.srs_free(srs)
    cg.shutdown()


if __name__ == "__main__":
    main()
