"""Whole-output conformance of the NTT entry point at a given plan: every element of every array of a batch against the C
restatement (oracle/), for inputs chosen to reach what uniformly random data never does - the zero-operand shortcuts of the
butterflies (lds_ntt: fl_any) with the zeros on either operand, and limbs at their maximum (r - 1 everywhere, x + r as
the raw image of x).  The plan (tile size, digits, tile widths, persistent launches) is read back through cg.ntt_plan and
reported, so that a caller can assert which path ran.

The three environment variables that steer the plan (CAPGPU_NTT_TILE_LOG, CAPGPU_NTT_TILE_ADAPT, CAPGPU_NTT_PERSISTENT)
are read once per process, so a forced configuration is one fresh process of this module:

    CAPGPU_NTT_TILE_LOG=11 python -m tools.ntt_conformance 10:512 13:64 16:8 21:1

Each argument is log_n:count[:stride], or plan=log_n:count to report the plan of that shape without running it.  One JSON
line per shape ({"log_n", "count", "plan", "mismatches", ...}); the exit code is 1 when anything differed and 3 when an
exception ended the run (a HIP error among them: nothing more is started on the device after one).  (tests/test_gpu_ntt_plans.py runs the default environment in-process and the forced
ones through this command line.)"""
import collections
import concurrent.futures
import json
import os
import sys
import traceback

import numpy as np

from oracle import bn254 as bn
from oracle import capref as cr

MODES = [(False, False), (False, True), (True, False), (True, True)]        # (inverse, coset)
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)
R_LIMBS = cr.int_to_limbs(bn.R)
RM1 = cr.int_to_limbs(bn.R - 1)
ONE = cr.int_to_limbs(1)

# The inputs of every shape, as raw 256-bit images (the transform is linear, so any image below r is "a field element
# in Montgomery form"; what matters to the kernels is the bit pattern).  An odd number of them, so that in a batch that
# cycles through them no two arrays a power of two apart are equal.
INPUTS = ["random", "zero", "all_rm1", "alt_rm1_one", "zeros90", "rm1_90", "impulse_0", "impulse_1", "impulse_half_m1",
          "impulse_half", "impulse_last", "impulse_seeded", "padded_half_plus_2", "odd_only", "three_mod_four_only",
          "x_plus_r", "random_b"]


def add_r(a: np.ndarray) -> np.ndarray:
    """a + r limb by limb (a < r, so the sum stays below 2^255)"""
    out = np.empty_like(a)
    carry = np.zeros(a.shape[0], dtype=np.uint64)
    for j in range(4):
        s = a[:, j] + R_LIMBS[j]
        c1 = s < a[:, j]
        s2 = s + carry
        c2 = s2 < s
        out[:, j] = s2
        carry = (c1 | c2).astype(np.uint64)
    assert not carry.any()
    return out


def impulse_positions(log_n: int, seed: int):
    n = 1 << log_n
    return {"impulse_0": 0, "impulse_1": 1 % n, "impulse_half_m1": max(n // 2 - 1, 0), "impulse_half": n // 2,
            "impulse_last": n - 1, "impulse_seeded": bn.SplitMix64(seed ^ 0x1357).next() % n}


def make_input(log_n: int, k: int, seed: int):
    """-> (raw image the device is given, the array the oracle transforms: the same, except for x + r)"""
    n = 1 << log_n
    name = INPUTS[k]
    rnd = lambda s: cr.random_field(seed * 64 + s, 1, n, True)
    idx = np.arange(n)
    if name == "random":
        x = rnd(0)
    elif name == "random_b":
        x = rnd(1)
    elif name == "zero":
        x = np.zeros((n, 4), dtype=np.uint64)
    elif name == "all_rm1":
        x = np.tile(RM1, (n, 1))
    elif name == "alt_rm1_one":
        x = np.tile(RM1, (n, 1))
        x[1::2] = ONE
    elif name in ("zeros90", "rm1_90"):
        x = rnd(2 if name == "zeros90" else 3)
        mask = np.random.default_rng(seed + k).random(n) < 0.9
        x[mask] = 0 if name == "zeros90" else RM1
    elif name.startswith("impulse_"):
        x = np.zeros((n, 4), dtype=np.uint64)
        x[impulse_positions(log_n, seed)[name]] = cr.random_field(seed * 64 + 4 + k, 1, 1, True)[0]
    elif name == "padded_half_plus_2":               # the prover's shape: n/2 + 2 coefficients on an n-point domain
        x = rnd(5)
        x[min(n, n // 2 + 2):] = 0
    elif name == "odd_only":
        x = rnd(6)
        x[idx % 2 == 0] = 0
    elif name == "three_mod_four_only":
        x = rnd(7)
        x[idx % 4 != 3] = 0
    elif name == "x_plus_r":
        x = rnd(8)
        return add_r(x), x
    else:
        raise ValueError(name)
    return x, x


def closed_form(log_n, name, inverse, coset, seed):
    """the transform of the impulses and of the constant inputs in closed form (Python integers on the raw images; None
    for the other inputs): an impulse v at k -> v omega^(jk), times 5^k on the coset; its inverse v omega^(-jk) / n,
    times 5^-j on the coset; a constant c -> n c at index 0 and zero elsewhere, its inverse c at index 0 (coset or not);
    the coset transform of a constant is not sparse and has no entry here."""
    n = 1 << log_n
    k_of = impulse_positions(log_n, seed)
    raw, _ = make_input(log_n, INPUTS.index(name), seed)
    first = int.from_bytes(raw[k_of.get(name, 0)].tobytes(), "little")
    w, g = bn.root_of_unity(log_n), bn.FR_GENERATOR
    if inverse:
        w, g = pow(w, bn.R - 2, bn.R), pow(g, bn.R - 2, bn.R)
    n_inv = pow(n, bn.R - 2, bn.R)
    if name in k_of:
        k = k_of[name]
        step, out, x = pow(w, k, bn.R), [], first * (n_inv if inverse else pow(g, k, bn.R) if coset else 1) % bn.R
        for j in range(n):
            out.append(x * (pow(g, j, bn.R) if inverse and coset else 1) % bn.R)
            x = x * step % bn.R
        return out
    if name in ("zero", "all_rm1") and (inverse or not coset):
        return [first if inverse else n * first % bn.R] + [0] * (n - 1)
    return None


def expected_stream(log_n, seed, inverse, coset, pool, window):
    """(k, raw input, oracle output) for every input, the oracle calls running `window` ahead in the pool"""
    def job(k):
        raw, ref = make_input(log_n, k, seed)
        exp = cr.ntt_fr(ref, log_n, inverse, coset).reshape(-1, 4)
        if log_n <= 10:                                                 # where Python integers cost nothing
            cf = closed_form(log_n, INPUTS[k], inverse, coset, seed)
            assert cf is None or cf == cr.array_to_ints(exp), f"closed form of {INPUTS[k]} differs from the oracle"
        return k, raw, exp
    pending, k_next = collections.deque(), 0
    while k_next < len(INPUTS) or pending:
        while k_next < len(INPUTS) and len(pending) < window:
            pending.append(pool.submit(job, k_next))
            k_next += 1
        yield pending.popleft().result()


def run_shape(cg, log_n, count, stride=None, modes=MODES, seed=1, threads=None):
    """Runs `count` arrays of 2^log_n per call through cg.ntt_fr_dev, array b of a call holding input (first + b) mod
    len(INPUTS), in as many calls as it takes to use every input, in each of `modes`.  -> {"plan": cg.ntt_plan(...),
    "mismatches": [text, ...], "arrays": arrays compared}.  Padding between arrays (stride > n) holds SENTINEL and must
    come back untouched."""
    n = 1 << log_n
    stride = n if stride is None else stride
    assert stride >= n
    threads = threads or min(16, os.cpu_count() or 1)
    K = len(INPUTS)
    bad, compared = [], 0
    with concurrent.futures.ThreadPoolExecutor(threads) as pool:
        for inverse, coset in modes:
            chunk = []

            def flush():
                nonlocal compared
                idx = np.arange(count) % len(chunk)
                host = np.full((count, stride, 4), SENTINEL, dtype=np.uint64)
                want = host.copy()
                raws = np.stack([c[1] for c in chunk])
                exps = np.stack([c[2] for c in chunk])
                host[:, :n] = raws[idx]
                want[:, :n] = exps[idx]
                d = cg.DevBuf.from_numpy(host)
                cg.ntt_fr_dev(d, log_n, count=count, stride=stride, inverse=inverse, coset=coset)
                got = d.to_numpy().reshape(count, stride, 4)
                d.free()
                compared += count
                if not np.array_equal(got, want):
                    rows = np.nonzero((got != want).any(axis=(1, 2)))[0]
                    for b in rows[:4]:
                        where = np.nonzero((got[b] != want[b]).any(axis=1))[0]
                        bad.append(f"inverse={inverse} coset={coset} array {b} ({INPUTS[chunk[idx[b]][0]]}): "
                                   f"{len(where)} of {stride} elements differ, first at {where[0]}"
                                   f"{' (padding)' if where[0] >= n else ''}")
                    if len(rows) > 4:
                        bad.append(f"inverse={inverse} coset={coset}: {len(rows)} of {count} arrays differ")

            for item in expected_stream(log_n, seed, inverse, coset, pool, threads):
                chunk.append(item)
                if count < K and len(chunk) == count:
                    flush()
                    chunk = []
            if chunk:
                flush()
    return {"log_n": log_n, "count": count, "stride": stride, "plan": cg.ntt_plan(log_n, count), "arrays": compared,
            "mismatches": bad}


def main(argv):
    try:
        from cap_amd import lib as cg
        cg.init(0)
        failed = False
        for arg in argv:
            parts = [int(x) for x in arg.split("=")[-1].split(":")]
            if arg.startswith("plan="):
                res = {"log_n": parts[0], "count": parts[1], "plan_only": True, "plan": cg.ntt_plan(parts[0], parts[1])}
            else:
                res = run_shape(cg, parts[0], parts[1], parts[2] if len(parts) > 2 else None)
                failed = failed or bool(res["mismatches"])
            print(json.dumps(res), flush=True)
        return 1 if failed else 0
    except Exception:
        traceback.print_exc()
        return 3


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
