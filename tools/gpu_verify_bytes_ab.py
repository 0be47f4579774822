#!/usr/bin/env python3
"""Same-session A/B of the ways to verify a block of transfer-shape proofs (n = 2^15, 27 public inputs) that a validator
holds as note bytes (769 per proof), for blocks of 1, 16, 64 and 256 proofs:
  deser+block  a loop of capgpu_proof_deserialize on one host thread, then capgpu_plonk_verify_block_dev; the loop's own
               milliseconds are reported beside the whole (column deser);
  bytes        capgpu_plonk_verify_block_bytes (host bytes and public inputs, decoded on the device);
  resident     capgpu_plonk_verify_block_bytes_resident (both already in device memory).
One process, the library loaded first (no torch), the kernel profiler off, wall clock.  Per count: the arms interleaved,
3 warm-up + 10 timed calls per arm, the round repeated 3 times; the table gives the median call of each repetition's timed
part as median [min .. max of the three medians] in milliseconds.  Every call must accept.  Then k_proof_decode's own
kernel time per count from the library's profiler (capgpu_profile_get), 10 launches each.
    python tools/gpu_verify_bytes_ab.py [--out profiles/verify_bytes_ab.txt] [--counts 1,16,64,256] [--steps 10]"""
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
ARMS = ("deser+block", "bytes", "resident")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "verify_bytes_ab.txt"))
    ap.add_argument("--counts", default="1,16,64,256")
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    counts = [int(c) for c in args.counts.split(",")]
    cg.init(0)
    L = cg.load()
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
    records = np.frombuffer(cg.proof_encode_batch(proofs), dtype=np.uint8)
    assert records.size == top * cg.PROOF_BYTES and records[:cg.PROOF_BYTES].tobytes() == cg.proof_serialize(proofs[0])
    u8p = ctypes.POINTER(ctypes.c_uint8)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# " + " ".join(__doc__.split("\n")[0:2]))
    emit(f"# arms interleaved, {WARM} warm-up + {args.steps} timed calls per arm, {REPS} repetitions; ms per call: "
         "median [min .. max] of the repetitions' medians; deser: the deserialise loop's share of deser+block")
    emit(f"{'count':>6} {'deser':>26} " + " ".join(f"{a:>26}" for a in ARMS))
    for cnt in counts:
        rec = np.ascontiguousarray(records[:cnt * cg.PROOF_BYTES])
        msgs = [b"ab"] * cnt
        handles = [vkh] * cnt
        d_rec = cg.DevBuf.from_numpy(rec)
        d_pub = cg.DevBuf.from_numpy(pubs[:cnt])
        arr = (cg.Proof * cnt)()
        used = ctypes.c_size_t(0)
        deser_ms = [0.0]

        def run(arm):
            if arm == "deser+block":
                t0 = time.perf_counter()
                for i in range(cnt):       # the C call alone: no Python object is made per proof
                    rc = L.capgpu_proof_deserialize(ctypes.cast(rec.ctypes.data + i * cg.PROOF_BYTES, u8p),
                                                    ctypes.c_size_t(cg.PROOF_BYTES), ctypes.byref(arr[i]), ctypes.byref(used))
                    assert rc == 0
                deser_ms[0] = (time.perf_counter() - t0) * 1e3
                return cg.plonk_verify_block(handles, h2, bh, pubs[:cnt], arr, msgs, num_inputs=ni)
            if arm == "bytes":
                return cg.plonk_verify_block_bytes(handles, h2, bh, pubs[:cnt], rec, msgs, num_inputs=ni)
            return cg.plonk_verify_block_bytes(handles, h2, bh, d_pub, d_rec, msgs, num_inputs=ni)

        med = {a: [] for a in ARMS + ("deser",)}
        for _ in range(REPS):
            for a in ARMS:
                for _ in range(WARM):
                    assert run(a)
                ts, ds = [], []
                for _ in range(args.steps):
                    t0 = time.perf_counter()
                    ok = run(a)
                    ts.append((time.perf_counter() - t0) * 1e3)
                    ds.append(deser_ms[0])
                    assert ok
                med[a].append(statistics.median(ts))
                if a == "deser+block":
                    med["deser"].append(statistics.median(ds))

        def cell(a):
            return f"{statistics.median(med[a]):8.2f} [{min(med[a]):7.2f} .. {max(med[a]):7.2f}]"
        emit(f"{cnt:>6} {cell('deser'):>26} " + " ".join(f"{cell(a):>26}" for a in ARMS))
        d_rec.free()
        d_pub.free()
    # the decode kernel on its own, per count (profiler on: every launch is bracketed by events)
    emit("# k_proof_decode / k_proof_decode_finish, library profiler, ms per launch (10 launches of capgpu_proof_decode_batch_dev):")
    for cnt in counts:
        d_rec = cg.DevBuf.from_numpy(np.ascontiguousarray(records[:cnt * cg.PROOF_BYTES]))
        d_pr, d_st = cg.proof_decode_batch(d_rec, count=cnt)      # warm
        cg.sync()
        cg.profile_reset()
        cg.profile_enable(True)
        for _ in range(10):
            cg.check(L.capgpu_proof_decode_batch_dev(d_rec.ptr, ctypes.c_size_t(cg.PROOF_BYTES), ctypes.c_size_t(cnt), d_pr.ptr,
                                                     d_st.ptr))
        cg.sync()
        cg.profile_enable(False)
        st = cg.profile_stats()
        assert not d_st.to_numpy(np.int32, cnt).any()
        emit(f"{cnt:>6} " + "  ".join(f"{k} {st[k][0] / st[k][1]:.4f}" for k in ("k_proof_decode", "k_proof_decode_finish")))
        for b in (d_rec, d_pr, d_st):
            b.free()
    os.makedirs(os.path.dirname(os.path.join(ROOT, args.out)), exist_ok=True)
    with open(os.path.join(ROOT, args.out), "w") as f:
        f.write("\n".join(lines) + "\n")
    cg.plonk_vk_release(vkh)
    cg.plonk_free_key(pk)
    cg.srs_free(srs)


if __name__ == "__main__":
    main()
