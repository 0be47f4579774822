"""A/B of the one-shot MSM (capgpu_msm_g1_var: caller points, no table) against the upload route (capgpu_srs_upload +
capgpu_msm_g1 + capgpu_srs_free) on the same host data, at n = 2^10, 2^13, 2^15, 2^17 and 2^20: wall-clock per call, host
buffers in, host result out, for both arms; the device-resident form alone (capgpu_msm_g1_var_dev + sync); and the
per-kernel time of one call from the library profiler (the Horner tail among them).  One process, 3 warm-up and 10 timed
calls per arm, arms interleaved, three repetitions; medians and the spread of the repetitions' medians are reported.
Usage: python tools/gpu_msm_var_ab.py [--out profiles/msm_var_ab.txt] [--logs 10,13,15,17,20]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cap_amd import bench_utils as bu  # noqa: E402
from cap_amd import lib as cg  # noqa: E402

P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
WARM, TIMED, REPS = 3, 10, 3


def ints(w):
    w = np.asarray(w, dtype=np.uint64).reshape(-1, 4)
    return [int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192 for r in w]


def same_point(a, b):
    x1, y1, z1 = ints(a)
    x2, y2, z2 = ints(b)
    if z1 == 0 or z2 == 0:
        return z1 == z2
    return (x1 * z2 * z2 - x2 * z1 * z1) % P == 0 and (y1 * z2 ** 3 - y2 * z1 ** 3) % P == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "msm_var_ab.txt"))
    ap.add_argument("--logs", default="10,13,15,17,20")
    args = ap.parse_args()
    cg.init(0)
    lines = ["one-shot MSM (var) against srs_upload + msm_g1 + srs_free (upload), ms per call, host data in, host result out",
             f"{WARM} warm-up + {TIMED} timed calls per arm, arms interleaved, {REPS} repetitions: median of the repetitions' "
             "medians [spread = max - min of them]",
             "var_dev: capgpu_msm_g1_var_dev on resident points and scalars + sync; horner / sort / accumulate: library "
             "profiler, one call", ""]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"{'n':>8} {'var':>16} {'upload':>16} {'var_dev':>16} {'horner':>8} {'sort':>8} {'accum':>8}  plan")
    for log_n in [int(x) for x in args.logs.split(",")]:
        n = 1 << log_n
        h = cg.srs_generate_affine_seq(12345, 67, n)
        bases = cg.srs_download(h, 0, n)
        cg.srs_free(h)
        sc = bu.random_canonical_scalars(log_n, n)
        d_b, d_s = cg.DevBuf.from_numpy(bases), cg.DevBuf.from_numpy(sc)

        def arm_var():
            return cg.msm_g1_var(bases, sc)

        def arm_upload():
            hh = cg.srs_upload(bases)
            out = cg.msm_g1(hh, sc)
            cg.srs_free(hh)
            return out

        def arm_dev():
            out = cg.msm_g1_var_dev(d_b, d_s, n)
            cg.sync()
            return out

        arms = {"var": arm_var, "upload": arm_upload, "var_dev": arm_dev}
        assert same_point(arm_var(), arm_upload()), "the two routes disagree"
        med = {k: [] for k in arms}
        for _ in range(REPS):
            t = {k: [] for k in arms}
            for i in range(WARM + TIMED):
                for k, fn in arms.items():          # interleaved: one call of every arm per round
                    t0 = time.perf_counter()
                    fn()
                    dt = (time.perf_counter() - t0) * 1e3
                    if i >= WARM:
                        t[k].append(dt)
            for k in arms:
                med[k].append(statistics.median(t[k]))
        cg.profile_enable(True)
        cg.profile_reset()
        arm_dev()
        st = cg.profile_stats()
        cg.profile_enable(False)
        cell = lambda k: f"{statistics.median(med[k]):8.3f} [{max(med[k]) - min(med[k]):5.3f}]"   # noqa: E731
        kern = lambda name: f"{st[name][0]:8.3f}" if name in st else "       -"                  # noqa: E731
        pl = cg.msm_var_plan(n)
        emit(f"{n:>8} {cell('var'):>16} {cell('upload'):>16} {cell('var_dev'):>16} {kern('msm_var_horner')} "
             f"{kern('msm_var_sort')} {kern('msm_accumulate')}  c={pl['c']} windows={pl['windows']} parts={pl['parts']} "
             f"workspace={pl['workspace_bytes'] / 2**20:.1f}MiB")
        d_b.free()
        d_s.free()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
