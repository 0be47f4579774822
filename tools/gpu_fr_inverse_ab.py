#!/usr/bin/env python3
"""Fermat against GCD: the two forms of the Fr inversion (capgpu_fr_set_inverse_form) in one process, arms interleaved.
  solve_<count>[_hinted]_<form>   capgpu_plonk_solve_vars_dev of cap_like_circuit("transfer_2x2") / its hinted model at
                                  --counts resident witnesses (584 levels, 509 of them with an inversion, no root rows)
  roots_256_<form>                the same call on tests/test_gpu_solve.py's hand_circuit(10): a circuit that HAS fifth-root
                                  rows, which keep their 254-bit power in either form
  prove_given_256_<form>          one synchronous plonk_prove_given of 256 from resident given values
  given_async_2x256_<form>        plonk_prove_given_async of 256 host-resident given values, two tickets in flight, against
  vars_async_2x256                plonk_prove_multi_async(vars) of 256 host-resident value vectors (no solver: one arm)
  batch_<n>_<form>                capgpu_fr_inverse_batch_dev over n resident elements, in place; k_fr_inverse's own time
                                  from capgpu_profile_dump beside the call time (the call does not wait: the arm syncs)
A library without the setting (CAPGPU_LIBRARY naming a build of the parent commit) runs the unhinted solve arms alone, as
form "parent": one process per turn, each with --label NAME --append, then --ab-summary FILE.
Protocol: per arm 3 warm-up + 10 timed calls, arms interleaved, three repetitions; the median of the three and their spread
(max - min over the median).  A form is faster where its median beats the other's by more than 3 x the larger spread.
  python tools/gpu_fr_inverse_ab.py [--out profiles/fr_inverse_ab.txt] [--counts 1,256,1024,4096] [--arms a,b] [--label NAME --append]"""
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


def ab_summary(path):
    calls, kern = {}, {}
    for line in open(path):
        r = json.loads(line)
        if "arm" in r and "call_ms" in r:
            k = f"{r['label']}:{r['arm']}" if r.get("label") else r["arm"]
            calls.setdefault(k, []).append(r["call_ms"])
            if r.get("kernel_ms") is not None:
                kern.setdefault(k, []).append(r["kernel_ms"])
    summary = {k: {"median_call_ms": round(statistics.median(v), 3), "spread_rel": round((max(v) - min(v)) / statistics.median(v), 4),
                   **({"median_kernel_ms": round(statistics.median(kern[k]), 3)} if k in kern else {})}
               for k, v in sorted(calls.items())}
    line = json.dumps({"ab_summary": summary})
    print(line)
    with open(path, "a") as out:
        out.write(line + "\n")


def main():
    if "--ab-summary" in sys.argv:
        return ab_summary(arg("--ab-summary", None))
    steps, reps = int(arg("--steps", 10)), int(arg("--reps", 3))
    counts = [int(c) for c in arg("--counts", "1,256,1024,4096").split(",")]
    sizes = [int(c) for c in arg("--sizes", "1024,65536,1048576").split(",")]
    out = open(arg("--out", os.path.join(ROOT, "profiles", "fr_inverse_ab.txt")), "a" if "--append" in sys.argv else "w")
    label = arg("--label", None)

    def emit(obj):
        line = json.dumps({"label": label, **obj} if label else obj)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    has_forms = hasattr(cg.load(), "capgpu_fr_set_inverse_form")
    forms = ["fermat", "gcd"] if has_forms else ["parent"]
    cg.init(0)
    cg.set_device(0)
    tau = bu.SplitMix64(0xCA9).field()
    top = max(counts + [P])
    idx = np.arange(top) % DISTINCT
    blind = np.stack([bu.to_mont_array(bu.blinders(7000 + i)) for i in range(P)])
    msgs = [b"ab"] * P
    keys, srs = {}, {}

    def add_key(name, sc, given, hints, gv):
        n, nv = sc.n, sc.num_vars
        if n not in srs:
            srs[n] = cg.srs_generate(tau, n + 3)
        pk, _ = cg.plonk_preprocess_vars(srs[n], n, sc.num_inputs, sc.selectors_mont(), np.array(sc.wire_vars, dtype=np.int64), nv)
        info, hinfo = cg.plonk_key_set_given_hints(pk, given, hints)
        at = {v: k for k, v in enumerate(given)}
        rows = gv[np.arange(top) % gv.shape[0]]
        pubs = np.ascontiguousarray(rows[:P][:, [at[v] for v in sc.pub_vars]])
        keys[name] = dict(pk=pk, ng=len(given), nv=nv, pubs=pubs, d_given=cg.DevBuf.from_numpy(rows), d_vars=cg.DevBuf(top * nv * 32),
                          host_given=np.ascontiguousarray(rows[:P]))
        emit({"circuit": name, "n": n, "num_vars": nv, "num_given": len(given), "num_hints": len(hints),
              "solver_info": info.as_dict(), "hint_info": hinfo.as_dict()})

    sc = bu.cap_like_circuit("transfer_2x2")
    given = [0, 1] + list(sc.free_vars)
    w, _ = sc.witnesses_mont(np.arange(5000, 5000 + DISTINCT, dtype=np.uint64), threads=16)
    vals = np.zeros((DISTINCT, sc.num_vars, 4), np.uint64)
    vals[:, np.array(sc.wire_vars).reshape(-1)] = w.reshape(DISTINCT, 5 * sc.n, 4)
    vals[:, 0], vals[:, 1] = bu.to_mont_array([0])[0], bu.to_mont_array([1])[0]
    add_key("transfer_2x2", sc, given, [], np.ascontiguousarray(vals[:, given]))
    host_vars = np.ascontiguousarray(vals[idx[:P]])
    if has_forms:
        hsc, hgiven, hhints = bu.cap_like_hinted_circuit("transfer_2x2")
        add_key("transfer_2x2_hinted", hsc, hgiven, hhints,
                np.stack([bu.to_mont_array(bu.cap_like_given_values(hsc, 5000 + i)) for i in range(DISTINCT)]))
        from tests.test_gpu_solve import given_values, hand_circuit, mont_rows
        rsc, rgiven = hand_circuit(10)
        add_key("hand_circuit_10", rsc, rgiven, [], mont_rows(given_values(rsc, rgiven, DISTINCT, 99)))
        # both forms give the same words (once, outside every timed part)
        for k in keys.values():
            got = {}
            for f in forms:
                cg.fr_set_inverse_form(f)
                _, st = cg.plonk_solve_vars(k["pk"], k["d_given"].view(0, 3 * k["ng"] * 32), 3, out=k["d_vars"])
                got[f] = (k["d_vars"].to_numpy(count=3 * k["nv"] * 4), [(s.kind, s.row) for s in st])
            assert np.array_equal(got["fermat"][0], got["gcd"][0]) and got["fermat"][1] == got["gcd"][1]
        cg.fr_set_inverse_form("fermat")
        cg.plonk_reserve(keys["transfer_2x2"]["pk"], P, "vars", slot=0)
        cg.plonk_reserve_given(keys["transfer_2x2"]["pk"], P, slot=-1)

    def with_form(f, fn):
        def run(k):
            if has_forms:
                cg.fr_set_inverse_form(f)
            try:
                fn(k)
            finally:
                if has_forms:
                    cg.fr_set_inverse_form("fermat")
        return run

    def solve_arm(name, count):
        k = keys[name]
        g = k["d_given"].view(0, count * k["ng"] * 32)

        def run(n):
            for _ in range(n):
                cg.plonk_solve_vars(k["pk"], g, count, out=k["d_vars"])
        return run

    def prove_given(n):
        k = keys["transfer_2x2"]
        g = k["d_given"].view(0, P * k["ng"] * 32)
        for _ in range(n):
            cg.plonk_prove_given([k["pk"]] * P, g, k["pubs"], blind, msgs)

    def in_flight(submit):
        """n tickets, two kept in flight, from an unbound thread (a bound thread's tickets all run on its context)"""
        def run(n):
            cg.set_device(-1)
            try:
                live = [submit()]
                for i in range(n):
                    if i + 1 < n:
                        live.append(submit())
                    assert live.pop(0).wait() is not None
            finally:
                cg.set_device(0)
        return run

    k0 = keys["transfer_2x2"]
    given_async = in_flight(lambda: cg.plonk_prove_given_async([k0["pk"]] * P, k0["host_given"], k0["pubs"], blind, msgs))
    vars_async = in_flight(lambda: cg.plonk_prove_multi_async([k0["pk"]] * P, host_vars, k0["pubs"], blind, msgs, input_form="vars"))

    def batch_arm(d_buf, n):
        def run(k):
            for _ in range(k):
                cg.fr_inverse_batch(d_buf, count=n)
            cg.sync_all()
        return run

    arms = []
    for c in counts:
        for name, tag in (("transfer_2x2", ""), ("transfer_2x2_hinted", "_hinted")):
            if name in keys:
                arms += [(f"solve_{c}{tag}_{f}", with_form(f, solve_arm(name, c)), c) for f in forms]
    bufs = []
    if has_forms:
        arms += [(f"roots_256_{f}", with_form(f, solve_arm("hand_circuit_10", P)), P) for f in forms]
        arms += [(f"prove_given_256_{f}", with_form(f, prove_given), P) for f in forms]
        arms += [(f"given_async_2x256_{f}", with_form(f, given_async), P) for f in forms]
        arms += [("vars_async_2x256", vars_async, P)]
        rng = np.random.default_rng(5)
        for n in sizes:
            x = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)     # any word pattern below 2^254 is a field image
            bufs.append(cg.DevBuf.from_numpy(x))
            arms += [(f"batch_{n}_{f}", with_form(f, batch_arm(bufs[-1], n)), n) for f in forms]
    only = arg("--arms", None)
    if only:
        arms = [a for a in arms if a[0] in only.split(",")]
    call_ms = {name: [] for name, _, _ in arms}
    kern_ms = {name: [] for name, _, _ in arms}
    cg.profile_enable(True)
    for rep in range(reps):
        for name, fn, count in arms:
            fn(WARM)
            cg.profile_reset()
            t0 = time.perf_counter()
            fn(steps)
            dt = time.perf_counter() - t0
            ks = [v for kn, v in cg.profile_stats().items() if kn.startswith("k_solve_vars") or kn.startswith("k_fr_inverse")]
            k_ms, k_n = sum(v[0] for v in ks), sum(v[1] for v in ks)
            call_ms[name].append(1e3 * dt / steps)
            kern_ms[name].append(k_ms / k_n if k_n else 0.0)
            emit({"arm": name, "rep": rep, "items": count, "call_ms": round(1e3 * dt / steps, 3),
                  "kernel_ms": round(k_ms / k_n, 4) if k_n else None})
    cg.profile_enable(False)
    med = {k: statistics.median(v) for k, v in call_ms.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in call_ms.items()}
    emit({"median_call_ms": {k: round(v, 3) for k, v in med.items()}, "spread_rel": {k: round(v, 4) for k, v in spread.items()},
          "median_kernel_ms": {k: round(statistics.median(v), 4) for k, v in kern_ms.items() if any(v)}})
    if has_forms:
        verdict = {}
        for a in med:
            if a.endswith("_gcd") and a[:-4] + "_fermat" in med:
                f = a[:-4] + "_fermat"
                s = max(spread[a] * med[a], spread[f] * med[f])
                verdict[a[:-4]] = {"fermat_over_gcd": round(med[f] / med[a], 3),
                                   "faster": "gcd" if med[f] - med[a] > 3 * s else "fermat" if med[a] - med[f] > 3 * s else "neither"}
        emit({"verdict_3x_larger_spread": verdict})
        if "vars_async_2x256" in med:
            emit({"given_tickets_over_vars_tickets_proofs_per_s":
                  {f: round(med["vars_async_2x256"] / med[f"given_async_2x256_{f}"], 4) for f in forms if f"given_async_2x256_{f}" in med},
                  "inverse_stats": cg.fr_inverse_stats()})
    for b in bufs:
        b.free()
    for k in keys.values():
        k["d_given"].free()
        k["d_vars"].free()
        cg.plonk_free_key(k["pk"])
    for h in srs.values():
        cg.srs_free(h)
    cg.shutdown()
    out.close()


if __name__ == "__main__":
    main()
