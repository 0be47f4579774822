"""Inputs and expectations for the Lagrange key builder (cap_amd/csrc/lagrange.hip) at degenerate SRS contents, in
Python integers only.

An SRS is given by the discrete logs s_i of its n + 3 points, P_i = [s_i] G (0 stands for the point at infinity), so every
point the builder makes is [integer] G with the integer known here:
    L_j = (1/n) sum_i omega^(-ij) s_i        j < n        (an integer inverse DFT)
    Z_e = s_(n+e) - s_e                      e = 0, 1, 2  (the blinding points)
The families are the inputs a random tau never produces: at a tau inside the domain every butterfly of the group FFT is a
doubling paired with a cancellation or infinity +- infinity; at tau = 0 every butterfly adds infinity; `single` puts A at
infinity with B live; `sparse_random` mixes infinity, duplicates and opposite points.
tests/test_lagrange_model.py checks this module; tests/test_lagrange_host.py and tests/test_gpu_lagrange_edges.py use it."""
import random

from oracle import bn254 as bn

R = bn.R

# the roster, by label: the argument of a label is resolved per size in family_logs (at small n some coincide)
FAMILIES = ("root:0", "root:1", "root:5", "root:n/2", "root:n-1", "order_2n", "zero", "single:1", "single:n/2",
            "single:n-1", "all_zero", "sparse_random")
GENERATED = ("root:0", "root:1", "root:5", "root:n/2", "root:n-1", "order_2n", "zero")   # those with a tau
SPARSE_SEED = 0x5EED


def omega(log_n: int) -> int:
    return bn.root_of_unity(log_n)


def _index(label: str, n: int) -> int:
    arg = label.split(":")[1]
    return {"0": 0, "1": 1, "5": 5, "n/2": n // 2, "n-1": n - 1}[arg]


def family_tau(label: str, log_n: int):
    """tau of a family that is a sequence of powers, or None"""
    n = 1 << log_n
    if label.startswith("root:"):
        return pow(omega(log_n), _index(label, n) % n, R)
    if label == "order_2n":
        return omega(log_n + 1)
    if label == "zero":
        return 0
    return None


def root_index(label: str, log_n: int) -> int:
    """k of root(k): tau = omega_n^k"""
    n = 1 << log_n
    return _index(label, n) % n


def family_logs(label: str, log_n: int) -> list:
    """the n + 3 discrete logs of the family's SRS"""
    n = 1 << log_n
    m = n + 3
    tau = family_tau(label, log_n)
    if tau is not None:
        out, x = [], 1
        for _ in range(m):
            out.append(x)
            x = x * tau % R
        return out
    if label.startswith("single:"):
        i0 = _index(label, n)
        out = [0] * m
        out[i0] = random.Random(100 + i0).randrange(1, R)
        return out
    if label == "all_zero":
        return [0] * m
    if label == "sparse_random":
        rng = random.Random(SPARSE_SEED + log_n)
        out = []
        for i in range(m):
            u = rng.random()
            if u < 0.25:
                out.append(0)
            elif u < 0.40 and i:
                out.append(out[rng.randrange(i)])                 # a duplicate
            elif u < 0.55 and i:
                out.append((R - out[rng.randrange(i)]) % R)       # an opposite point
            else:
                out.append(rng.randrange(1, R))
        return out
    raise ValueError(label)


def bitrev(i: int, log_n: int) -> int:
    r = 0
    for b in range(log_n):
        r |= ((i >> b) & 1) << (log_n - 1 - b)
    return r


def inverse_dft(s, log_n: int) -> list:
    """(1/n) sum_i omega^(-ij) s_i for j < n: radix-2, decimation in time, integers mod r"""
    n = 1 << log_n
    a = [0] * n
    for i in range(n):
        a[bitrev(i, log_n)] = s[i] % R
    w_inv = pow(omega(log_n), R - 2, R)
    half = 1
    while half < n:
        step = n // (2 * half)
        tw = [pow(w_inv, j * step, R) for j in range(half)]
        for base in range(0, n, 2 * half):
            for j in range(half):
                u, v = a[base + j], a[base + j + half] * tw[j] % R
                a[base + j], a[base + j + half] = (u + v) % R, (u - v) % R
        half *= 2
    n_inv = pow(n, R - 2, R)
    return [x * n_inv % R for x in a]


def expected_logs(s, log_n: int) -> list:
    """the discrete logs of the n + 3 points of the key built from the SRS with logs s"""
    n = 1 << log_n
    assert len(s) >= n + 3
    return inverse_dft(s, log_n) + [(s[n + e] - s[e]) % R for e in range(3)]


def commit_log(key_logs, scalars) -> int:
    """the discrete log of the commitment to `scalars` (values, then blinders) on a key"""
    return sum(c * k for c, k in zip(scalars, key_logs)) % R


def points(logs):
    """[s] G for every log, (len, 8) Montgomery affine words, infinity as zeros (the CPU oracle's fixed-base table)"""
    from oracle import capref as cr
    return cr.g1_fixed_base_batch(cr.ints_to_array([x % R for x in logs]))
