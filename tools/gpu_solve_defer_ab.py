#!/usr/bin/env python3
"""The witness solver's DEFERRED form (capgpu_plonk_key_set_solve_form) beside the DIRECT form: a sibling of
tools/gpu_solve_ab.py with its protocol - per arm 3 warm-up + 10 timed calls, the arms interleaved, three repetitions, raw
lines to --out (appended), the median of the repetitions and their spread (max - min over the median) by --ab-summary.
One process per LIBRARY and turn (CAPGPU_LIBRARY names the one a process loads; a library without the call runs the direct
arms only):
    for NAME in parent_1 tree_1 parent_2 tree_2: python tools/gpu_solve_defer_ab.py --label NAME --out profiles/solve_defer.txt
    python tools/gpu_solve_defer_ab.py --ab-summary profiles/solve_defer.txt
Arms (the name carries model, count, inverse form and schedule form):
  solve_<model>_<count>_<fermat|gcd>_<direct|deferred>   capgpu_plonk_solve_vars_dev at --counts (default 1,256,1024,4096)
      resident witnesses; model hinted = cap_like_hinted_circuit("transfer_2x2"), io = cap_like_io_circuit("transfer_2x2")
      (public inputs derived), root = tests' hand_circuit(10), the fifth-root family, at 256
  prove_given_256_<inv>_<form>          one synchronous plonk_prove_given of 256 from resident given values (hinted model)
  prove_given_async_2x256_<inv>_<form>  plonk_prove_given_async of 256 host-resident rows, two tickets kept in flight
  host_vars_async_2x256                 plonk_prove_multi_async(vars) of 256, two tickets in flight: no solver at all
Every deferred key's result is compared with the direct key's, word for word, once, outside every timed part; the plan
figures (capgpu_solve_form_info) are printed per model.  --arms a,b: those arms only (substring match); --reps N; --steps N."""
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
from cap_amd.io_model import cap_like_io_circuit  # noqa: E402

P, WARM, DISTINCT = 256, 3, 16


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def ab_summary(path):
    calls = {}
    for line in open(path):
        r = json.loads(line)
        if "label" in r and "arm" in r:
            calls.setdefault(f"{r['label']} {r['arm']}", []).append(r["call_ms"])
    summary = {k: {"median_call_ms": statistics.median(v), "spread_rel": round((max(v) - min(v)) / statistics.median(v), 4)}
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
    label = arg("--label", "tree")
    out = open(arg("--out", os.path.join(ROOT, "profiles", "solve_defer.txt")), "a")
    has_form = hasattr(cg.load(), "capgpu_plonk_key_set_solve_form")
    forms = ("direct", "deferred") if has_form else ("direct",)

    def emit(obj):
        line = json.dumps({"label": label, **obj})
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    cg.init(0)
    cg.set_device(0)
    tau = bu.SplitMix64(0xCA9).field()
    top = max(counts + [P])
    idx = np.arange(top) % DISTINCT
    keys, srs = {}, {}
    models = [("hinted", lambda: bu.cap_like_hinted_circuit("transfer_2x2") + (0,)),
              ("io", lambda: cap_like_io_circuit("transfer_2x2") + (3,))]
    if "--no-root" not in sys.argv:
        from tests.test_gpu_solve import given_values, hand_circuit
        models.append(("root", lambda: hand_circuit(10) + ([], 0)))
    for name, make in models:
        sc, given, hints, flags = make()
        if name == "root":
            gv = np.stack([bu.to_mont_array(v) for v in given_values(sc, given, DISTINCT, 3)])
        else:
            gv = np.stack([bu.to_mont_array(bu.cap_like_given_values(sc, 5000 + i)) for i in range(DISTINCT)])
        n, nv = sc.n, sc.num_vars
        if n not in srs:
            srs[n] = cg.srs_generate(tau, n + 3)
        pk, _ = cg.plonk_preprocess_vars(srs[n], n, sc.num_inputs, sc.selectors_mont(), np.array(sc.wire_vars, dtype=np.int64), nv)
        info, _ = cg.plonk_key_set_solver(pk, given, hints, flags)
        cnt = top if name != "root" else P
        d_given = cg.DevBuf.from_numpy(gv[idx[:cnt]])
        d_vars = cg.DevBuf(cnt * nv * 32)
        _, st = cg.plonk_solve_vars(pk, d_given.view(0, P * len(given) * 32), P, out=d_vars)
        direct = d_vars.to_numpy(count=P * nv * 4).copy()
        rec = {"model": name, "n": n, "num_vars": nv, "num_given": len(given), "solver_info": info.as_dict()}
        if has_form:
            t0 = time.perf_counter()
            finfo = cg.plonk_key_set_solve_form(pk, cg.SOLVE_FORM_DEFERRED)
            rec["set_solve_form_s"] = round(time.perf_counter() - t0, 3)
            rec["solve_form_info"] = finfo.as_dict()
            for inv in ("fermat", "gcd"):
                cg.fr_set_inverse_form(inv)
                _, st2 = cg.plonk_solve_vars(pk, d_given.view(0, P * len(given) * 32), P, out=d_vars)
                assert np.array_equal(d_vars.to_numpy(count=P * nv * 4), direct), (name, inv)
                assert [(s.kind, s.row) for s in st2] == [(s.kind, s.row) for s in st], (name, inv)
            cg.fr_set_inverse_form("fermat")
            rec["deferred_equals_direct"] = True
            cg.plonk_reserve_given(pk, P, slot=-1)
            cg.plonk_key_set_solve_form(pk, cg.SOLVE_FORM_DIRECT)
        if name == "hinted":
            at = {v: k for k, v in enumerate(given)}
            pubs = np.ascontiguousarray(gv[idx[:P]][:, [at[v] for v in sc.pub_vars]])
            wv = np.array(sc.wire_vars).reshape(-1)
            host_vars = np.ascontiguousarray(d_vars.to_numpy(count=P * nv * 4).reshape(P, nv, 4))
            assert wv.max() < nv
            cg.plonk_reserve_given(pk, P, slot=-1)
            keys["prove"] = (pk, len(given), pubs, d_given, np.ascontiguousarray(gv[idx[:P]]), host_vars)
        keys[name] = (pk, len(given), nv, d_given, d_vars)
        emit(rec)

    def with_forms(pk, inv, form, fn):
        def run(k):
            cg.fr_set_inverse_form(inv)
            if has_form:
                cg.plonk_key_set_solve_form(pk, cg.SOLVE_FORM_DEFERRED if form == "deferred" else cg.SOLVE_FORM_DIRECT)
            try:
                fn(k)
            finally:
                cg.fr_set_inverse_form("fermat")
        return run

    def solve_arm(model, count):
        pk, ng, _, d_given, d_vars = keys[model]
        g = d_given.view(0, count * ng * 32)

        def run(k):
            for _ in range(k):
                cg.plonk_solve_vars(pk, g, count, out=d_vars)
        return pk, run

    blind = np.stack([bu.to_mont_array(bu.blinders(7000 + i)) for i in range(P)])
    msgs = [b"ab"] * P
    ppk, png, pubs, pd_given, host_given, host_vars = keys["prove"]

    def prove_given(k):
        g = pd_given.view(0, P * png * 32)
        for _ in range(k):
            cg.plonk_prove_given([ppk] * P, g, pubs, blind, msgs)

    def in_flight(submit):
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

    given_async = in_flight(lambda: cg.plonk_prove_given_async([ppk] * P, host_given, pubs, blind, msgs))
    vars_async = in_flight(lambda: cg.plonk_prove_multi_async([ppk] * P, host_vars, pubs, blind, msgs, input_form="vars"))

    arms = []
    for model in [m[0] for m in models]:
        for count in (counts if model != "root" else [P]):
            for inv in ("fermat", "gcd"):
                for form in forms:
                    pk, run = solve_arm(model, count)
                    arms.append((f"solve_{model}_{count}_{inv}_{form}", with_forms(pk, inv, form, run), count))
    for inv in ("fermat", "gcd"):
        for form in forms:
            arms.append((f"prove_given_256_{inv}_{form}", with_forms(ppk, inv, form, prove_given), P))
            arms.append((f"prove_given_async_2x256_{inv}_{form}", with_forms(ppk, inv, form, given_async), P))
    arms.append(("host_vars_async_2x256", vars_async, P))
    only = arg("--arms", None)
    if only:
        arms = [a for a in arms if any(o in a[0] for o in only.split(","))]
    for rep in range(reps):
        for name, fn, count in arms:
            fn(WARM)
            t0 = time.perf_counter()
            fn(steps)
            dt = time.perf_counter() - t0
            emit({"arm": name, "rep": rep, "witnesses": count, "call_ms": round(1e3 * dt / steps, 3)})
    emit({"solve_stats": cg.plonk_solve_stats(), "scratch_stats": cg.scratch_stats()})
    cg.shutdown()
    out.close()


if __name__ == "__main__":
    main()
