"""The one-wavefront point sums - g1_sum_kernel (cap_amd/csrc/capgpu.hip) behind cg.g1_sum and g1_sum_ranks_kernel
(cap_amd/csrc/comm.hip) behind the sharded MSM's exchange - and the affine-sequence SRS generator, at the inputs where
the group law leaves its common path: lane partials that are equal (the shuffle tree doubles) or opposite (it cancels),
points at infinity anywhere, a single live entry, and sequences a + i b that pass through 0.  Every input is [s] G with
s known, so every expected result is [integer] G: the integer from Python, the point from the CPU oracle's fixed-base
table; a result at infinity is compared as Z = 0.  All comparisons are exact.

Lane l of either kernel adds up the entries l, l + 64, l + 128, ...; the tree then adds lane l + d to lane l for
d = 32, 16, ..., 1.  An input of period p <= 64 therefore makes the partials of lanes l and l + p equal: the tree doubles
at the levels d >= p and adds distinct points below.

A pattern with one live entry runs only at the sizes that have its index (index 63 from n = 64, index 64 from n = 65, index
0 and n - 1 from n = 1); each size asserts which of them it ran.

Wall time on the MI355X: 1.7 s for the whole module run alone (21 tests), no test above 0.1 s (MEASURED_S)."""
import random

import numpy as np
import pytest

from oracle import bn254 as bn
from oracle import capref as cr
from tests import lagrange_model as M

pytestmark = pytest.mark.gpu

R, P = bn.R, bn.P
SUM_SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)
PERIODS = (1, 2, 16, 32, 64)
LIVE_AT = (0, 63, 64, "n-1")
RANKS = (2, 3, 64, 65, 130)
SEQ = ((0, 0), (R - 1, 1), (0, 1), (5, 0))
SEQ_SIZES = (1, 255, 256, 257)
MEASURED_S = 1.7


class Jac:
    """Jacobian triples (x z^2, y z^3, z) of [s] G with a fresh random z per entry, arkworks' Montgomery words"""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.affine = {}

    def rows(self, logs):
        new = sorted({s % R for s in logs if s % R} - set(self.affine))
        if new:
            for s, p in zip(new, M.points(new)):
                self.affine[s] = cr.affine_to_ints(p)
        vals = []
        for s in logs:
            if s % R == 0:                                     # infinity: (t^2, t^3, 0)
                t = self.rng.randrange(1, P)
                vals += [t * t % P, t * t * t % P, 0]
            else:
                x, y = self.affine[s % R]
                z = self.rng.randrange(1, P)
                vals += [x * z * z % P, y * z * z * z % P, z]
        return cr.ints_to_array([bn.to_mont(v, P) for v in vals]).reshape(-1, 12)


def check_sum(got, want_log, what):
    got = np.asarray(got, np.uint64).reshape(12)
    if want_log % R == 0:
        assert not got[8:12].any(), what                       # infinity: Z = 0
    else:
        assert got[8:12].any(), what
        assert np.array_equal(cr.g1_to_affine(got), M.points([want_log])[0]), what


def sum_patterns(n, rng):
    """(name, logs) for one size"""
    pool = [rng.randrange(1, R) for _ in range(64)]
    out = [(f"period:{p}", [pool[i % p] for i in range(n)]) for p in PERIODS]
    s = rng.randrange(1, R)
    out.append(("alternating", [s if i % 2 == 0 else R - s for i in range(n)]))
    out.append(("all_infinity", [0] * n))
    for at in LIVE_AT:                                         # only where the size has that index
        i0 = n - 1 if at == "n-1" else at
        if 0 <= i0 < n:
            out.append((f"live:{at}", [pool[3] if i == i0 else 0 for i in range(n)]))
    out.append(("random_sparse", [0 if rng.random() < 0.25 else rng.randrange(1, R) for _ in range(n)]))
    return out


@pytest.mark.parametrize("n", SUM_SIZES)
def test_g1_sum_patterns(cg, n):
    rng = random.Random(9000 + n)
    jac = Jac(n)
    ran = []
    for name, logs in sum_patterns(n, rng):
        assert len(logs) == n
        pts = jac.rows(logs) if n else np.zeros((0, 12), np.uint64)
        if name.startswith("live:"):
            assert sum(1 for x in logs if x) == 1, name
        check_sum(cg.g1_sum(pts), sum(logs) % R, (n, name))
        ran.append(name)
    live = [f"live:{a}" for a, from_n in zip(LIVE_AT, (1, 64, 65, 1)) if n >= from_n]     # index 63 exists from n = 64 ...
    assert ran == [f"period:{p}" for p in PERIODS] + ["alternating", "all_infinity"] + live + ["random_sparse"]
    assert len(live) == {0: 0, 1: 2, 2: 2, 63: 2, 64: 3}.get(n, 4)


def test_g1_sum_same_point_in_different_representatives(cg):
    """64 representatives of ONE point: every level of the tree is a doubling that the coordinates do not show"""
    jac = Jac(1)
    s = 0x1234567
    pts = jac.rows([s] * 64)
    assert len({bytes(r) for r in pts}) == 64
    check_sum(cg.g1_sum(pts), 64 * s, "64 x P")


@pytest.mark.parametrize("k", RANKS)
def test_rank_sums_of_equal_opposite_and_empty_partials(cg, k):
    """g1_sum_ranks_kernel through the loopback communicator: this process plays the k ranks in turn, each with its own
    copy of one block of points, two MSMs per exchange (the gather buffer's stride is three slots)"""
    m, count = 5, 2
    rng = random.Random(40 + k)
    block = [rng.randrange(1, R) for _ in range(m)]
    h = cg.srs_upload(np.tile(M.points(block), (k, 1)))          # the same block once per rank
    c = [[rng.randrange(1, R) for _ in range(m)] for _ in range(count)]
    q = [sum(ci * bi for ci, bi in zip(c[i], block)) % R for i in range(count)]      # log of one rank's partial
    neg = [[R - x for x in row] for row in c]
    cases = {
        "equal": ([c] * k, [k * q[i] % R for i in range(count)]),
        "opposite": ([c if r % 2 == 0 else neg for r in range(k)], [q[i] * (k % 2) % R for i in range(count)]),
        "every_second_empty": ([c if r % 2 == 0 else None for r in range(k)], [(k + 1) // 2 * q[i] % R for i in range(count)]),
    }
    ran, bufs = [], []
    cg.comm_init_loopback(k)
    try:
        for name, (per_rank, want) in cases.items():
            d_out = cg.DevBuf(96 * count)
            bufs.append(d_out)
            for rank in range(k):
                cg.comm_loopback_set_rank(rank)
                sc = per_rank[rank]
                if sc is None:                                    # an empty rank: no points, its partials are infinity
                    d = cg.DevBuf.from_numpy(np.zeros((count, 4), np.uint64))
                    bufs.append(d)
                    cg.msm_g1_sharded_dev(h, d, 0, count=count, stride=1, offset=rank * m, d_out=d_out)
                else:
                    d = cg.DevBuf.from_numpy(cr.ints_to_array([x for row in sc for x in row]))
                    bufs.append(d)
                    cg.msm_g1_sharded_dev(h, d, m, count=count, offset=rank * m, d_out=d_out)
                bufs.pop().free()
            out = d_out.to_numpy().reshape(count, 12)
            for i in range(count):
                check_sum(out[i], want[i], (k, name, i))
            ran.append(name)
    finally:
        cg.comm_destroy()
        for d in bufs:
            d.free()
        cg.srs_free(h)
    assert ran == ["equal", "opposite", "every_second_empty"] and q[0] != q[1]


@pytest.mark.parametrize("n", SEQ_SIZES)
def test_affine_sequence_through_zero(cg, n):
    """P_i = [a + i b] G: all at infinity, the sequence r - 1, 0, 1, ... whose point 1 is at infinity, 0, 1, 2, ... whose
    point 0 is, and a constant one; 256 points are one block of srs_fixed_base_kernel"""
    ran = []
    for a, b in SEQ:
        logs = [(a + i * b) % R for i in range(n)]
        h = cg.srs_generate_affine_seq(a, b, n)
        got = cg.srs_download(h, 0, n)
        cg.srs_free(h)
        assert np.array_equal(got, M.points(logs)), (a, b, n)
        if (a, b) == (R - 1, 1) and n > 1:
            assert not got[1].any() and got[0].any() and got[2].any()
        ran.append((a, b))
    assert tuple(ran) == SEQ


def test_the_roster():
    assert SUM_SIZES == (0, 1, 2, 63, 64, 65, 127, 128, 129, 200) and PERIODS == (1, 2, 16, 32, 64)
    assert RANKS == (2, 3, 64, 65, 130) and SEQ_SIZES == (1, 255, 256, 257)
    assert SEQ == ((0, 0), (R - 1, 1), (0, 1), (5, 0)) and LIVE_AT == (0, 63, 64, "n-1")
