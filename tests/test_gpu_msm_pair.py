"""The first addition of a bucket-accumulation item is an affine + affine addition (G1L::add_affine_pair, peeled in front
of the loop of msm_accumulate).  Point and scalar sets that put the peeled block in every state - no pair, the pair alone,
the pair and one mixed addition, a doubling or a cancellation as the pair, a point at infinity on either side, every sign
combination - through the table MSM (srs_upload + msm_g1) and the one-shot MSM (msm_g1_var), bit-exact in affine form
against the C oracle."""
import numpy as np
import pytest

from oracle import bn254 as bn
from oracle import capref as cr

pytestmark = pytest.mark.gpu

NPTS = 1 << 11
ONE, RM1 = cr.int_to_limbs(1), cr.int_to_limbs(bn.R - 1)


def neg(pt):
    """-P of a Montgomery affine point (8 words): y -> p - y"""
    out = pt.copy()
    y = cr.array_to_ints(pt[4:])[0]
    out[4:] = cr.int_to_limbs((bn.P - y) % bn.P)
    return out


def const(n, k):
    return np.tile(cr.int_to_limbs(k), (n, 1))


@pytest.fixture(scope="module")
def pts():
    b = cr.g1_fixed_base_batch(cr.random_field(4711, 1, NPTS, False))
    b.setflags(write=False)
    return b


def _cases(pts):
    k = 0x2B5F3 << 90 | 0x1D3
    yield "one point: no pair", pts[:1], const(1, k)
    yield "two points, equal scalars: the pair alone", pts[:2], const(2, k)
    yield "three points, equal scalars: the pair and one mixed addition", pts[:3], const(3, k)
    for copies in (8, 64):
        yield f"{copies} copies of one point: the pair is a doubling", np.tile(pts[3], (copies, 1)), const(copies, k)
    alt = np.stack([pts[4] if i % 2 == 0 else neg(pts[4]) for i in range(8)] + [pts[5]])
    yield "P, -P alternating: the pair cancels, on from infinity", alt, const(9, k)
    for where in (0, 1):
        b = pts[8:12].copy()
        b[where] = 0
        yield f"infinity as entry {where}", b, const(4, k)
    # the scalars the list of cases names; r - 1 is a full-width scalar (the MSM does not negate it), so these put no two
    # points with opposite signs into one bucket - the digit cases below do
    for name, a, c in (("1, 1", ONE, ONE), ("r-1, r-1", RM1, RM1), ("1, r-1", ONE, RM1), ("r-1, 1", RM1, ONE)):
        yield f"scalars {name}, and 1", pts[12:15], np.stack([a, c, ONE])
        yield f"scalars {name}", pts[12:14], np.stack([a, c])
    # signed digits: with windows of w bits the scalar d has the digit +d in window 0 and 2^w - d the digit -d there (and
    # a carry of 1 into window 1), so two points with these scalars meet in bucket d with the signs chosen here.  The
    # window width is the plan's, not the test's: every w a plan uses (9 .. 16), all four sign combinations, the pair
    # alone and followed by one mixed addition.
    d = 5
    for w in range(9, 17):
        plus, minus = cr.int_to_limbs(d), cr.int_to_limbs((1 << w) - d)
        for s0, s1 in ((plus, plus), (plus, minus), (minus, plus), (minus, minus)):
            name = f"digits {'+' if s0 is plus else '-'}{d}, {'+' if s1 is plus else '-'}{d} of a {w}-bit window"
            yield name + ": the pair alone", pts[20:22], np.stack([s0, s1])
            yield name + ", then +", pts[20:23], np.stack([s0, s1, plus])
    mixed = cr.random_field(99, 1, 48, False)
    mixed[0::3] = ONE
    mixed[1::3] = RM1
    yield "1, r-1 and random scalars mixed", pts[16:64], mixed
    yield "random, 2^11 points", pts, cr.random_field(100, 1, NPTS, False)


@pytest.fixture(scope="module")
def cases(pts):
    """(name, bases, scalars, oracle result in affine form), computed once"""
    return [(name, b, s, cr.g1_to_affine(cr.msm_g1(b, s))) for name, b, s in _cases(pts)]


def test_cases_cover_what_they_claim(cases):
    names = [c[0] for c in cases]
    assert len(names) == 18 + 8 * 4 * 2 and len(set(names)) == len(names)
    # the digit cases: -d in window 0 of a w-bit recoding is 2^w - d, whose value the oracle sums like any other
    for name, b, s, want in cases:
        if name.startswith("digits -5, -5 of a 13-bit") and name.endswith("alone"):
            k = (1 << 13) - 5
            assert cr.array_to_ints(s) == [k, k]
    cancel = next(c for c in cases if c[0].startswith("P, -P"))
    assert np.array_equal(cr.g1_to_affine(cr.g1_mul(cancel[1][8], cr.array_to_ints(cancel[2][8])[0])), cancel[3])


def test_table_msm(cg, cases):
    for name, b, s, want in cases:
        h = cg.srs_upload(b)
        try:
            assert np.array_equal(cr.g1_to_affine(cg.msm_g1(h, s)), want), name
        finally:
            cg.srs_free(h)


def test_one_shot_msm(cg, cases):
    for name, b, s, want in cases:
        assert np.array_equal(cr.g1_to_affine(cg.msm_g1_var(b, s)), want), name
