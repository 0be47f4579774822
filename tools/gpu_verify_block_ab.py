#!/usr/bin/env python3
"""Same-session A/B of the ways to verify a block of transfer-shape proofs (n = 2^15, 27 public inputs) for blocks of
1, 16, 64 and 256 proofs:
  host         capgpu_plonk_batch_verify (host threads);
  dev_lane     capgpu_plonk_batch_verify_dev with the pairing form LANE (final product on the host);
  dev_wave     capgpu_plonk_batch_verify_dev with the pairing form WAVE;
  block        capgpu_plonk_verify_block_dev (host proofs and public inputs);
  resident     capgpu_plonk_verify_block_resident (both already in device memory).
One process, the library loaded first (no torch), the kernel profiler off, wall clock.  Per count: the arms interleaved,
3 warm-up + 10 timed calls per arm, the round repeated 3 times; the table gives the median call of each repetition's timed
part as median [min .. max of the three medians] in milliseconds.  Every call must accept.
    python tools/gpu_verify_block_ab.py [--out profiles/verify_block_ab.txt] [--counts 1,16,64,256] [--steps 10]"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from cap_amd import bench_utils as bu  # noqa: E402
from cap_amd import lib as cg  # noqa: E402

WARM, REPS = 3, 3
ARMS = ("host", "dev_lane", "dev_wave", "block", "resident")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "verify_block_ab.txt"))
    ap.add_argument("--counts", default="1,16,64,256")
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    counts = [int(c) for c in args.counts.split(",")]
    cg.init(0)
    log_n, ni = 15, 27
    n = 1 << log_n
    tau = bu.SplitMix64(0xCA9).field()
    srs = cg.srs_generate(tau, n + 3)
    sc = bu.synthetic_circuit(log_n, ni, seed=2 + log_n + ni)
    pk, vk = cg.plonk_preprocess(srs, n, ni, sc.selectors_mont(), sc.sigma_mont())
    vkh = cg.plonk_vk_upload(vk)
    h2 = cg.g2_generator()
    bh = cg.g2_mul(h2, tau)
    top = max(counts)
    wit = [sc.witness(3 + i) for i in range(4)]
    wires = np.stack([sc.wires_mont(wit[i % 4][0]) for i in range(top)])
    pubs = np.stack([bu.to_mont_array(wit[i % 4][1]) for i in range(top)])
    blind = np.stack([bu.to_mont_array(bu.blinders(7000 + i)) for i in range(top)])
    proofs = cg.plonk_prove_batch(pk, wires, pubs, blind, b"ab", top)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# " + " ".join(__doc__.split("\n")[0:1]))
    emit(f"# arms interleaved, {WARM} warm-up + {args.steps} timed calls per arm, {REPS} repetitions; ms per call: "
         "median [min .. max] of the repetitions' medians")
    emit(f"{'count':>6} " + " ".join(f"{a:>26}" for a in ARMS))
    for cnt in counts:
        pr, pb, msgs = proofs[:cnt], [pubs[i] for i in range(cnt)], [b"ab"] * cnt
        arr = (cg.Proof * cnt)()
        for i, p in enumerate(pr):
            ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(p), ctypes.sizeof(cg.Proof))
        d_pr = cg.DevBuf(ctypes.sizeof(arr))
        cg.check(cg.load().capgpu_memcpy_h2d(d_pr.ptr, ctypes.byref(arr), ctypes.c_size_t(ctypes.sizeof(arr))))
        d_pub = cg.DevBuf.from_numpy(pubs[:cnt])
        handles = [vkh] * cnt

        def run(arm):
            if arm == "host":
                return cg.plonk_batch_verify([vk] * cnt, h2, bh, pb, pr, msgs)
            if arm in ("dev_lane", "dev_wave"):
                cg.pairing_set_form(cg.PAIRING_WAVE if arm == "dev_wave" else cg.PAIRING_LANE)
                return cg.plonk_batch_verify([vk] * cnt, h2, bh, pb, pr, msgs, on_device=True)
            if arm == "block":
                return cg.plonk_verify_block(handles, h2, bh, pubs[:cnt], arr, msgs, num_inputs=ni)
            return cg.plonk_verify_block(handles, h2, bh, d_pub, d_pr, msgs, num_inputs=ni)

        med = {a: [] for a in ARMS}
        for _ in range(REPS):
            for a in ARMS:
                for _ in range(WARM):
                    assert run(a)
                ts = []
                for _ in range(args.steps):
                    t0 = time.perf_counter()
                    ok = run(a)
                    ts.append((time.perf_counter() - t0) * 1e3)
                    assert ok
                med[a].append(statistics.median(ts))
        cg.pairing_set_form(cg.PAIRING_LANE)

        def cell(a):
            return f"{statistics.median(med[a]):8.2f} [{min(med[a]):7.2f} .. {max(med[a]):7.2f}]"
        emit(f"{cnt:>6} " + " ".join(f"{cell(a):>26}" for a in ARMS))
        d_pr.free()
        d_pub.free()
    # one profiled block call of the largest count: where the device time of the new path goes
    cg.profile_reset()
    cg.profile_enable(True)
    cg.plonk_verify_block([vkh] * top, h2, bh, pubs[:top], proofs[:top], [b"ab"] * top, num_inputs=ni)
    cg.profile_enable(False)
    st = cg.profile_stats()
    emit(f"# kernel profile of one block call of {top} proofs (library profiler, ms): " +
         ", ".join(f"{k}={v}" for k, v in sorted(st.items()) if "verify" in k or "msm_var" in k or "pairing" in k))
    os.makedirs(os.path.dirname(os.path.join(ROOT, args.out)), exist_ok=True)
    with open(os.path.join(ROOT, args.out), "w") as f:
        f.write("\n".join(lines) + "\n")
    cg.plonk_vk_release(vkh)
    cg.plonk_free_key(pk)
    cg.srs_free(srs)


if __name__ == "__main__":
    main()
