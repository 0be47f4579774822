"""Cases and expected values for tests/hip/nttcheck (the NttIo addressing forms of cap::ntt_run and the 3 * 2^k
transforms of cap_amd/csrc/ntt.hpp), and the file format the two sides share.

Expected values come from the oracle only: the addressing is modelled here in Python - gather the elements an array is
made of, zero-extend beyond src_len, pre-scale - and oracle.capref.ntt_fr transforms the result.  For the 3 * 2^k
transforms the reference is three coset transforms with the shifts s_a = 5 omega_N^a (omega_N built as in
tests/test_quotient_domain.py::root_6n), block a at index a M + k.  tests/test_ntt_expectations.py checks this model
against direct evaluations on a machine without a GPU.

Data are raw 256-bit images throughout ((k, 4) uint64).  "arkworks form" is x 2^256 mod r, the kernels' internal form
x 2^261 mod r: as integers the second is 32 times the first, and since every transform here is linear the model never
needs the value x itself."""
import concurrent.futures
import functools
import operator
import os
import struct

import numpy as np

from oracle import bn254 as bn
from oracle import capref as cr
from tests.test_quotient_domain import root_6n
from tools.ntt_conformance import add_r

R = bn.R
MAGIC_IN, MAGIC_OUT = 0x4e54544943415345, 0x4e54544f55545055
NTT_RUN, NTT3_FORWARD, NTT3_INVERSE, NTT3_ROUND_TRIP = 0, 1, 2, 3
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)
REFUSED = 1000000
INV_2_261 = pow(1 << 261, R - 2, R)
FIELDS = ["kind", "log_n", "count", "dir", "coset", "src_elems", "dst_elems", "pre_elems", "dst_offset", "src_outer",
          "src_inner", "src_len", "src_group", "dst_outer", "dst_inner", "dst_group", "src_elem_stride", "src_group2",
          "src_inner2", "dst_group2", "dst_inner2", "pre_inner", "lazy_out"]
DEFAULTS = {"dir": 0, "coset": 0, "pre_elems": 0, "dst_offset": 0, "src_inner": 0, "src_group": 1, "dst_inner": 0,
            "dst_group": 1, "src_elem_stride": 1, "src_group2": 1, "src_inner2": 0, "dst_group2": 1, "dst_inner2": 0,
            "pre_inner": 0, "lazy_out": 0}


_from_le = functools.partial(int.from_bytes, byteorder="little")
_to_le = operator.methodcaller("to_bytes", 32, "little")


def to_ints(a):
    raw = np.ascontiguousarray(a, dtype=np.uint64).tobytes()
    return list(map(_from_le, (raw[i:i + 32] for i in range(0, len(raw), 32))))


def from_ints(vals):
    return np.frombuffer(b"".join(map(_to_le, vals)), dtype=np.uint64).reshape(-1, 4).copy()


def random_raw(seed, k):
    return cr.random_field(seed, 1, k, True)


_pool = concurrent.futures.ThreadPoolExecutor(min(16, os.cpu_count() or 1))


def oracle_transforms(arrays, log_n, inverse, coset):
    """cr.ntt_fr on every array (the C oracle runs outside the interpreter lock, so a few at a time)"""
    return list(_pool.map(lambda x: cr.ntt_fr(x, log_n, inverse, coset).reshape(-1, 4), arrays))


class Case:
    """header fields as attributes, src / pre buffers, and `regions`: [(start, expected (len, 4), lazy)] - the expected
    content of the destination buffer; everything outside the regions must still hold the sentinel"""

    def __init__(self, name, src, pre=None, **h):
        self.name = name
        self.src = np.ascontiguousarray(src, dtype=np.uint64).reshape(-1, 4)
        self.pre = np.zeros((0, 4), dtype=np.uint64) if pre is None else np.ascontiguousarray(pre).reshape(-1, 4)
        self.h = dict(DEFAULTS)
        self.h.update(h)
        self.h["src_elems"], self.h["pre_elems"] = len(self.src), len(self.pre)
        self.regions = []

    def __getattr__(self, k):
        try:
            return self.__dict__["h"][k]
        except KeyError:
            raise AttributeError(k)


# ---- the addressing of ntt_run(..., &io) ---------------------------------------------------------------------------
def array_base(q, outer, inner, group, group2, inner2):
    q2, a = divmod(q, group)
    return (q2 // group2) * outer + (q2 % group2) * inner2 + a * inner


def gather_array(c, q):
    """the 2^log_n input elements of array q after zero extension and pre-scaling (raw images)"""
    n = 1 << c.log_n
    a = q % c.src_group
    base = array_base(q, c.src_outer, c.src_inner, c.src_group, c.src_group2, c.src_inner2)
    es = c.src_elem_stride
    pos = np.arange(n) * es + (a * c.src_inner if es != 1 else 0)       # position inside the source array
    valid = pos < c.src_len
    x = np.zeros((n, 4), dtype=np.uint64)
    x[valid] = c.src[base + np.arange(n)[valid] * es]
    if len(c.pre):                                                     # v * pre * 2^-261: a Montgomery product
        f = to_ints(c.pre[pos[valid] + a * c.pre_inner])
        xi = to_ints(x)
        for j, g in enumerate(np.nonzero(valid)[0]):
            xi[g] = xi[g] * f[j] % R * INV_2_261 % R
        x = from_ints(xi)
    return x


def expect_ntt_run(c):
    n = 1 << c.log_n
    coset = bool(c.coset) and not (len(c.pre) and not c.dir)            # a caller's table replaces the coset table
    ys = oracle_transforms([gather_array(c, q) for q in range(c.count)], c.log_n, bool(c.dir), coset)
    for q, y in enumerate(ys):
        start = c.dst_offset + array_base(q, c.dst_outer, c.dst_inner, c.dst_group, c.dst_group2, c.dst_inner2)
        c.regions.append((start, y, bool(c.lazy_out)))
    return c


# ---- N = 3 M ---------------------------------------------------------------------------------------------------------
def shifts(log_m):
    """s_a = 5 omega_N^a, a = 0, 1, 2 (canonical integers), and omega_M"""
    w, m = root_6n(log_m - 1) if log_m >= 1 else (None, None)
    assert m == 1 << log_m
    return [bn.FR_GENERATOR * pow(w, a, R) % R for a in range(3)], bn.root_of_unity(log_m)


@functools.lru_cache(maxsize=None)
def shift_powers(log_m):
    """s_a^i, i < M, for the three shifts"""
    out = []
    for s in shifts(log_m)[0]:
        pw = [1] * (1 << log_m)
        for i in range(1, len(pw)):
            pw[i] = pw[i - 1] * s % R
        out.append(pw)
    return out


def eval_blocks(coeffs_raw, log_m):
    """evaluations of a polynomial of up to 3 M coefficients (raw images, any scaling) on the three cosets s_a <omega_M>,
    block order: [a][k] <-> s_a omega_M^k.  Chunk b of M coefficients contributes s_a^(M b) * NTT(c_i s_a^i)."""
    M = 1 << log_m
    cs = to_ints(coeffs_raw)
    cs += [0] * (3 * M - len(cs))
    used = [b for b in range(3) if any(cs[b * M:(b + 1) * M])]
    scaled = [from_ints([v * p % R for v, p in zip(cs[b * M:(b + 1) * M], pw)])
              for pw in shift_powers(log_m) for b in used]
    ys = iter(oracle_transforms(scaled, log_m, False, False))
    out = []
    for s, pw in zip(shifts(log_m)[0], shift_powers(log_m)):
        s_m = pw[-1] * s % R
        acc = [0] * M
        for b in used:
            lead = pow(s_m, b, R)
            acc = [(t + lead * v) % R for t, v in zip(acc, to_ints(next(ys)))]
        out.append(acc)
    return out


def expect_ntt3_forward(c, then_inverse=False):
    """arkworks-form coefficients -> internal-form evaluations (32 x the arkworks image), weakly reduced"""
    M = 1 << c.log_n
    for q in range(c.count):
        base = (q // c.src_group) * c.src_outer + (q % c.src_group) * c.src_inner
        coeffs = c.src[base:base + min(c.src_len, M)]
        start = c.dst_offset + (q // c.dst_group) * c.dst_outer + (q % c.dst_group) * c.dst_inner
        if then_inverse:                                                # back to the coefficients, zero-extended to 3 M
            y = np.zeros((3 * M, 4), dtype=np.uint64)
            y[:len(coeffs)] = coeffs
            c.regions.append((start, y, False))
            continue
        for a, blk in enumerate(eval_blocks(coeffs, c.log_n)):
            c.regions.append((start + a * M, from_ints([32 * v % R for v in blk]), True))
    return c


def ntt3_inverse_case(name, log_m, count, degree, seed):
    """`count` polynomials of the given degree: their internal-form evaluations in, arkworks-form coefficients out"""
    M = 1 << log_m
    N = 3 * M
    src = np.zeros((count * N, 4), dtype=np.uint64)
    c = Case(name, src, kind=NTT3_INVERSE, log_n=log_m, count=count, dst_elems=count * N, src_outer=N, src_len=M,
             dst_outer=N)
    for q in range(count):
        t = np.zeros((N, 4), dtype=np.uint64)
        t[:degree + 1] = random_raw(seed * 1000 + q, degree + 1)
        ev = [32 * v % R for blk in eval_blocks(t, log_m) for v in blk]
        c.src[q * N:(q + 1) * N] = from_ints(ev)
        c.regions.append((q * N, t, False))
    c.degree = degree
    return c


# ---- the case list ---------------------------------------------------------------------------------------------------
def _src_for(h, seed):
    """a random source buffer just large enough for the addressing h (every element non-zero: an element read from
    beyond src_len, instead of the zero it stands for, shows)"""
    c = Case("probe", np.zeros((0, 4)), **h)
    n = 1 << c.log_n
    top = 0
    for q in range(c.count):
        base = array_base(q, c.src_outer, c.src_inner, c.src_group, c.src_group2, c.src_inner2)
        top = max(top, base + (n - 1) * c.src_elem_stride + 1)
    return random_raw(seed, top + 3)


def _dst_elems(h):
    c = Case("probe", np.zeros((0, 4)), **h)
    top = 0
    for q in range(c.count):
        top = max(top, array_base(q, c.dst_outer, c.dst_inner, c.dst_group, c.dst_group2, c.dst_inner2) + (1 << c.log_n))
    return c.dst_offset + top + 5


def ntt_run_case(name, seed, pre=None, **h):
    h.setdefault("kind", NTT_RUN)
    h["dst_elems"] = _dst_elems(h)
    return expect_ntt_run(Case(name, _src_for(h, seed), pre, **h))


def internal_table(vals):
    """canonical integers -> the internal-form images x 2^261 mod r"""
    return from_ints([v * (1 << 261) % R for v in vals])


def ntt_io_cases(sizes=((6, 3), (10, 5), (12, 4), (12, 64))):
    """sizes: (log_n, count); at log_n = 12 count 4 takes the 256-element tile and count 64 the 1024-element one"""
    out, seed = [], 100
    modes = [(0, 0), (0, 1), (1, 0), (1, 1)]
    for log_n, count in sizes:
        n = 1 << log_n
        tag = f"2^{log_n}x{count}"
        for i, src_len in enumerate((0, 1, n // 2 + 2, n - 1, n)):
            d, cs = modes[(i + log_n) % 4]
            seed += 1
            out.append(ntt_run_case(f"src_len={src_len} {tag}", seed, log_n=log_n, count=count, dir=d, coset=cs,
                                    src_outer=n + 3, src_len=src_len, dst_outer=n + 5, lazy_out=i % 2))
        for i, (sg, dg) in enumerate(((3, 1), (1, 3), (5, 3), (3, 5))):
            d, cs = modes[i]
            seed += 1
            out.append(ntt_run_case(f"groups {sg}/{dg} {tag}", seed, log_n=log_n, count=count, dir=d, coset=cs,
                                    src_outer=sg * (n + 1) + 2, src_inner=n + 1, src_group=sg, src_len=n // 2 + 2,
                                    dst_outer=dg * (n + 2) + 1, dst_inner=n + 2, dst_group=dg, lazy_out=(i + 1) % 2))
        seed += 1
        out.append(ntt_run_case(f"second grouping level {tag}", seed, log_n=log_n, count=count, coset=1, src_len=n - 1,
                                src_group=3, src_inner=n + 1, src_group2=2, src_inner2=3 * (n + 1) + 1,
                                src_outer=6 * (n + 1) + 5, dst_group=3, dst_inner=n + 2, dst_group2=2,
                                dst_inner2=3 * (n + 2) + 2, dst_outer=6 * (n + 2) + 7))
        rng = bn.SplitMix64(seed)
        for d, cs in ((0, 0), (0, 1), (1, 0)):
            seed += 1
            pre = internal_table([rng.field(R) for _ in range(3 * n)])
            out.append(ntt_run_case(f"pre-scale table, pre_inner = n, dir={d} coset={cs} {tag}", seed, pre, log_n=log_n,
                                    count=count, dir=d, coset=cs, src_group=3, src_inner=n + 1, src_outer=3 * (n + 1),
                                    src_len=n - 3, dst_outer=n, pre_inner=n, lazy_out=d))
        for with_pre in (False, True):
            # decimated input: array q = (q2, a) reads elements 3 g + a of polynomial q2 (src_inner = 1 is the group
            # offset), src_len and the table are indexed by that position
            seed += 1
            pre = internal_table([rng.field(R) for _ in range(3 * n + 2 * 7)]) if with_pre else None
            out.append(ntt_run_case(f"src_elem_stride = 3{' with a table' if with_pre else ''} {tag}", seed, pre,
                                    log_n=log_n, count=count, src_elem_stride=3, src_group=3, src_inner=1,
                                    src_outer=3 * n + 2, src_len=3 * n - 4, dst_outer=n + 1,
                                    pre_inner=7 if with_pre else 0, lazy_out=int(with_pre)))
    return out


def prover_cases():
    """the NttIo initialisers of prove_run.hpp (compute_pk_coset, r3_wire_cosets, z_cosets) at n = 2^5, P = 3"""
    n, P, NW = 32, 3, 5
    M, m, ps, log_m = 2 * n, 6 * n, n + 8, 6
    mk = lambda name, seed, count, elems, dst_elems, off, io: expect_ntt3_forward(Case(
        name, random_raw(seed, elems), kind=NTT3_FORWARD, log_n=log_m, count=count, dst_elems=dst_elems, dst_offset=off,
        src_outer=io[0], src_inner=io[1], src_len=io[2], src_group=io[3], dst_outer=io[4], dst_inner=io[5],
        dst_group=io[6]))
    return [mk("compute_pk_coset", 11, 18, 18 * ps, 18 * m + 4, 0, (ps, 0, n, 1, m, 0, 1)),
            mk("r3_wire_cosets: wires", 12, P * NW, P * NW * ps, P * 7 * m + 4, 0, (NW * ps, ps, n + 2, NW, 7 * m, m, NW)),
            mk("r3_wire_cosets: public inputs", 13, P, P * n, P * 7 * m + 4, 6 * m, (n, 0, n, 1, 7 * m, 0, 1)),
            mk("z_cosets", 14, P, P * ps, P * 7 * m + 4, 5 * m, (ps, 0, n + 3, 1, 7 * m, 0, 1))]


def ntt3_cases(log_ms=(1, 2, 5, 6, 11, 12), counts=(1, 4, 18)):
    out, seed = [], 500
    for log_m in log_ms:
        M = 1 << log_m
        N = 3 * M
        for count in counts:
            tag = f"M=2^{log_m} x{count}"
            for src_len in sorted({1, min(M, M // 2 + 2), M}):
                seed += 1
                out.append(expect_ntt3_forward(Case(
                    f"ntt3 forward src_len={src_len} {tag}", random_raw(seed, count * (M + 1)), kind=NTT3_FORWARD,
                    log_n=log_m, count=count, dst_elems=count * (N + 2) + 3, dst_offset=1, src_outer=M + 1,
                    src_len=src_len, dst_outer=N + 2)))
            # the quotient's degree, 5 n + 7 with n = M / 2 (where 3 M points carry it), and the full 3 M - 1
            for degree in sorted({min(5 * (M // 2) + 7, N - 1), N - 1}):
                seed += 1
                out.append(ntt3_inverse_case(f"ntt3 inverse degree={degree} {tag}", log_m, count, degree, seed))
            seed += 1
            out.append(expect_ntt3_forward(Case(
                f"ntt3 round trip {tag}", random_raw(seed, count * M), kind=NTT3_ROUND_TRIP, log_n=log_m, count=count,
                dst_elems=count * N + 2, src_outer=M, src_len=M, dst_outer=N), then_inverse=True))
    return out


# ---- files -----------------------------------------------------------------------------------------------------------
def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", MAGIC_IN, len(cases)))
        for c in cases:
            f.write(struct.pack(f"<{len(FIELDS)}Q", *[int(c.h[k]) for k in FIELDS]))
            f.write(c.src.tobytes())
            f.write(c.pre.tobytes())


def read_results(path, cases):
    out = []
    with open(path, "rb") as f:
        magic, k = struct.unpack("<QQ", f.read(16))
        assert magic == MAGIC_OUT and k == len(cases)
        for c in cases:
            rc, elems = struct.unpack("<QQ", f.read(16))
            assert elems == c.dst_elems
            out.append((rc, np.frombuffer(f.read(32 * elems), dtype=np.uint64).reshape(-1, 4)))
    return out


def below(a, bound):
    """elementwise a < bound for (k, 4) limb arrays"""
    lim = cr.int_to_limbs(bound)
    lt = np.zeros(len(a), dtype=bool)
    eq = np.ones(len(a), dtype=bool)
    for j in (3, 2, 1, 0):
        lt |= eq & (a[:, j] < lim[j])
        eq &= a[:, j] == lim[j]
    return lt


def check_case(c, rc, dst):
    """-> list of complaints: wrong values, a representation outside its contract (lazy results below 2 r, all others
    canonical), bytes outside the destination arrays that changed"""
    if rc != 0:
        return [f"{c.name}: rc = {rc}{' (refused: the case addresses memory outside its buffers)' if rc == REFUSED else ''}"]
    bad = []
    untouched = np.ones(len(dst), dtype=bool)
    for start, exp, lazy in c.regions:
        got = dst[start:start + len(exp)]
        assert untouched[start:start + len(exp)].all(), f"{c.name}: the case's own destination arrays overlap"
        untouched[start:start + len(exp)] = False
        assert below(exp, R).all()
        same = (got == exp).all(axis=1)
        if lazy:
            same |= (got == add_r(exp)).all(axis=1)                     # any representative below 2 r
        elif not below(got, R).all():
            bad.append(f"{c.name}: {int((~below(got, R)).sum())} results at {start} are not canonical")
        if not same.all():
            bad.append(f"{c.name}: {int((~same).sum())} of {len(exp)} elements of the array at {start} differ, "
                       f"first at {int(np.nonzero(~same)[0][0])}")
    if not (dst[untouched] == SENTINEL).all():
        bad.append(f"{c.name}: {int((dst[untouched] != SENTINEL).any(axis=1).sum())} elements outside the destination "
                   f"arrays were written")
    return bad
