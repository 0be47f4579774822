"""BASELINE config 4's 64 notes - 32 transfer_2x3 and 19 freeze_3 at n = 2^15, 13 mint at n = 2^14, in note order 5:2:3
interleaved, witnesses in host memory - proved three ways in ONE session:

  (a) one capgpu_plonk_prove_each per domain, one after the other, from one thread;
  (b) bench.py's "domains on two contexts": two threads, each bound to a context, one per domain;
  (c) ONE capgpu_plonk_prove_notes call from one unbound thread.

(a) and (b) get their per-domain arrays sorted ahead of the clock; (c) takes the notes as they come.  The arms are
interleaved: per repetition every arm makes --warmup untimed and --calls timed calls; --reps repetitions; median and spread
(max - min over the repetitions, relative to the median) per arm.  One line per (repetition, arm) and the summary go to
stdout and to --out.

    python tools/gpu_notes_mix.py --out profiles/notes_mix.txt
"""
import argparse
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cap_amd import bench_utils as bu  # noqa: E402
from cap_amd import lib as cg  # noqa: E402

MIX = [("transfer_2x3", 32), ("mint", 13), ("freeze_3", 19)]


def note_order():
    """64 kinds, every prefix as close to 32:13:19 as whole notes allow"""
    total = sum(c for _, c in MIX)
    given = [0] * len(MIX)
    order = []
    for i in range(total):
        k = max(range(len(MIX)), key=lambda j: (MIX[j][1] * (i + 1) / total - given[j], -j) if given[j] < MIX[j][1] else (-1e9, 0))
        given[k] += 1
        order.append(k)
    return order


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cg.init(0)
    assert cg.device_count() >= 2, "arm (b) needs two contexts"
    tau = bu.SplitMix64(0xCA9).field()
    srs = cg.srs_generate(tau, (1 << 15) + 3)
    keys = []
    for kind, cnt in MIX:
        ln, ni = bu.NOTE_SHAPES[kind]
        sc = bu.synthetic_circuit(ln, ni, seed=2 + ln + ni)
        pk, _ = cg.plonk_preprocess(srs, 1 << ln, ni, sc.selectors_mont(), sc.sigma_mont())
        wm, pm = sc.witnesses_mont([3 + i for i in range(cnt)])
        keys.append({"pk": pk, "n": 1 << ln, "ni": ni, "wires": wm, "pubs": pm, "used": 0})
    max_in = max(k["ni"] for k in keys)
    order = note_order()
    notes = []                                            # (key index, witness index)
    for k in order:
        notes.append((k, keys[k]["used"]))
        keys[k]["used"] += 1
    count = len(notes)
    msg = bytes(range(32))
    handles = [keys[k]["pk"] for k, _ in notes]
    wires = [keys[k]["wires"][i] for k, i in notes]     # one block per note, where the witness generator left it
    pub = np.zeros((count, max_in, 4), np.uint64)
    for j, (k, i) in enumerate(notes):
        pub[j, :keys[k]["ni"]] = keys[k]["pubs"][i]
    blind = np.stack([bu.to_mont_array(bu.blinders(7000 + j)) for j in range(count)])
    msgs = [msg] * count
    # arms (a) and (b): the caller's own sort by domain, ahead of the clock
    domains = []
    for dom in sorted({k["n"] for k in keys}, reverse=True):
        idx = [j for j, (k, _) in enumerate(notes) if keys[k]["n"] == dom]
        ni = max(keys[k]["ni"] for k, _ in (notes[j] for j in idx))
        domains.append({"idx": idx, "handles": [handles[j] for j in idx], "wires": np.stack([wires[j] for j in idx]),
                        "pub": np.ascontiguousarray(pub[idx][:, :ni]), "blind": np.ascontiguousarray(blind[idx]),
                        "msgs": [msg] * len(idx)})
    say(f"# notes {count}: " + " ".join(f"{kind} x{c}" for kind, c in MIX) + f"; domains {[len(d['idx']) for d in domains]}; "
        f"contexts {cg.device_count()}; calls {args.calls} warmup {args.warmup} reps {args.reps}")

    def each(d):
        return cg.plonk_prove_each(d["handles"], d["wires"], d["pub"], d["blind"], d["msgs"])

    def arm_a(calls):
        t0 = time.perf_counter()
        for _ in range(calls):
            out = [each(d) for d in domains]
        return time.perf_counter() - t0, out

    def arm_b(calls):
        bar = threading.Barrier(len(domains) + 1)
        res, errs = [None] * len(domains), []

        def run(i):
            try:
                cg.set_device(i)
                bar.wait()
                for _ in range(calls):
                    res[i] = each(domains[i])
                bar.wait()
            except Exception as e:                       # noqa: BLE001
                errs.append(str(e))
                bar.abort()
            finally:
                cg.set_device(-1)

        th = [threading.Thread(target=run, args=(i,)) for i in range(len(domains))]
        for t in th:
            t.start()
        bar.wait()
        t0 = time.perf_counter()
        bar.wait()
        dt = time.perf_counter() - t0
        for t in th:
            t.join()
        assert not errs, errs
        return dt, res

    def arm_c(calls):
        t0 = time.perf_counter()
        for _ in range(calls):
            out = cg.plonk_prove_notes(handles, wires, pub, blind, msgs)
        return time.perf_counter() - t0, out

    def in_note_order(per_domain):
        got = [None] * count
        for d, (proofs, outcomes) in zip(domains, per_domain):
            assert all(o.status == 0 for o in outcomes)
            for j, p in zip(d["idx"], proofs):
                got[j] = bytes(p)
        return got

    arms = [("a_each_per_domain_in_turn", arm_a), ("b_domains_on_two_bound_threads", arm_b), ("c_one_prove_notes_call", arm_c)]
    cg.plonk_reserve_notes(handles, slot=-1)
    ms = {name: [] for name, _ in arms}
    for rep in range(args.reps):
        for name, fn in arms:
            fn(args.warmup)
            g0 = cg.scratch_stats()["grow_events"]
            dt, out = fn(args.calls)
            grew = cg.scratch_stats()["grow_events"] - g0
            per_call = dt / args.calls * 1e3
            ms[name].append(per_call)
            say(f"rep {rep} {name}: {per_call:.3f} ms per {count} notes ({count / per_call * 1e3:.1f} proofs/s), scratch growths {grew}")
            if rep == 0:
                got = [bytes(p) for p in out[0]] if name.startswith("c_") else in_note_order(out)
                if name.startswith("a_"):
                    want = got
                assert got == want, f"{name}: not the proofs of arm (a)"
    say("# same proofs in all three arms: yes")
    for name, _ in arms:
        v = sorted(ms[name])
        med = v[len(v) // 2]
        say(f"summary {name}: median {med:.3f} ms, spread {(v[-1] - v[0]) / med * 100:.2f} % ({', '.join('%.3f' % x for x in ms[name])})")
    b, c = sorted(ms[arms[1][0]]), sorted(ms[arms[2][0]])
    mb, mc = b[len(b) // 2], c[len(c) // 2]
    say(f"summary c / b: {mc / mb:.4f} (b's own spread {(b[-1] - b[0]) / mb * 100:.2f} %); notes_stats {cg.plonk_notes_stats()}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
