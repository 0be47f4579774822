"""capgpu_srs_check on the device: is a resident SRS a power sequence [tau^i] g under the open key (h, [tau] h)?

Sizes sit at the launch boundaries, not at the workload's size: 64 / 65 / 257 are the wavefront and block edges of
k_srs_points, 1025 puts a second 1024-scalar tile under the fold (whose second MSM starts at point offset 1), 4097 is the
first size that builds the wide window table, 2^15 + 3 is the prover's own SRS (consistent verdict only).  SRS come from
capgpu_srs_generate(tau, n) with beta_h = [tau] h; tampering is download, edit, upload.  Every verdict is exact for these
inputs: a consistent SRS is accepted by an identity, and every rejected one is inconsistent by construction (a wrong
acceptance has probability about 2^-128).

The weights are pinned against the documented rule - r_i = the first 16 bytes, little-endian, of
Keccak-256(seed || le64(i)) - by comparing the report's folds with the oracle's MSM over weights recomputed here: a fold
with equal or zero weights would still pass every tamper case, or pass everything."""
import ctypes

import numpy as np
import pytest

from oracle import bn254 as bn
from oracle import capref as cr

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 64, 65, 257, 1025, 4097]
NONE = 2**64 - 1
SEED_A = bytes(range(32))
SEED_B = bytes(255 - i for i in range(32))
TAU2 = 0x1234567  # the "other ceremony"


class Srs:
    def __init__(self, cg, tau, n):
        self.n = n
        self.handle = cg.srs_generate(tau, n)
        self.points = cg.srs_download(self.handle, 0, n).reshape(n, 8)
        self.h = cg.g2_generator()
        self.beta_h = cg.g2_mul(self.h, tau)


@pytest.fixture(scope="module")
def srs_of(cg, tau):
    made = {}

    def get(n):
        if n not in made:
            made[n] = Srs(cg, tau, n)
        return made[n]
    yield get
    for s in made.values():
        cg.srs_free(s.handle)


def weights(seed: bytes, count: int) -> np.ndarray:
    """(count, 4) canonical scalars below 2^128: the rule of cap_amd/csrc/srs_check.hpp, restated"""
    vals = [int.from_bytes(cr.keccak256(seed + i.to_bytes(8, "little"))[:16], "little") for i in range(count)]
    return cr.ints_to_array(vals) if vals else np.zeros((0, 4), np.uint64)


def fold(rep, which):
    return np.array(list(getattr(rep, which)), dtype=np.uint64)


def checked(cg, points, s, locate=True, seed=SEED_A):
    """upload `points`, check them under s's open key, free them"""
    h = cg.srs_upload(np.ascontiguousarray(points))
    try:
        return cg.srs_check(h, s.h, s.beta_h, seed, locate=locate)
    finally:
        cg.srs_free(h)


def other_points(count: int, first: int = 0xC0FFEE) -> np.ndarray:
    """curve points that belong to no SRS of these tests: [first + j] g"""
    return cr.g1_fixed_base_batch(cr.ints_to_array([first + j for j in range(count)]))


def log2_ceil(n: int) -> int:
    return (n - 1).bit_length()


# ---- 1. consistent -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES + [(1 << 15) + 3])
def test_consistent_srs_is_accepted(cg, srs_of, n):
    s = srs_of(n)
    probe = cr.random_field(n, 1, min(n, 64), False)
    before = cr.g1_to_affine(cg.msm_g1(s.handle, probe))
    reps = [cg.srs_check(s.handle, s.h, s.beta_h, seed, locate=locate)
            for seed, locate in ((SEED_A, False), (SEED_B, True), (None, False))]
    for rep in reps:
        assert (rep.verdict, rep.point_fault, rep.first_bad_point, rep.first_bad_link) == (0, 0, NONE, NONE), str(rep)
        assert (rep.points_checked, rep.links_checked) == (n, n - 1)
        assert rep.pairing_checks == (1 if n > 1 else 0)
    again = cg.srs_check(s.handle, s.h, s.beta_h, SEED_A)
    assert bytes(again) == bytes(reps[0]), "the same inputs and seed give the same report"
    if n > 1:
        assert not np.array_equal(fold(reps[0], "fold_a"), fold(reps[1], "fold_a")), "the seed reaches the weights"
    else:
        assert not fold(reps[0], "fold_a").any() and not fold(reps[0], "fold_b").any()
    assert np.array_equal(cr.g1_to_affine(cg.msm_g1(s.handle, probe)), before), "the check leaves the table as it was"


@pytest.mark.parametrize("n", [n for n in SIZES if 1 < n <= 1025])
def test_folds_are_the_oracles_msm_over_the_documented_weights(cg, srs_of, n):
    s = srs_of(n)
    for seed in (SEED_A, SEED_B):
        rep = cg.srs_check(s.handle, s.h, s.beta_h, seed)
        w = weights(seed, n - 1)
        assert np.array_equal(fold(rep, "fold_a"), cr.g1_to_affine(cr.msm_g1(s.points[:n - 1], w))), (n, "A")
        assert np.array_equal(fold(rep, "fold_b"), cr.g1_to_affine(cr.msm_g1(s.points[1:], w))), (n, "B")


# ---- 2. wrong open key ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES[1:])
def test_open_key_of_another_tau(cg, srs_of, tau, n):
    s = srs_of(n)
    wrong = cg.g2_mul(s.h, (tau + 1) % bn.R)
    rep = cg.srs_check(s.handle, s.h, wrong, SEED_A)
    assert (rep.verdict, rep.first_bad_link, rep.pairing_checks) == (2, NONE, 1)
    rep = cg.srs_check(s.handle, s.h, wrong, SEED_A, locate=True)
    assert (rep.verdict, rep.first_bad_link) == (2, 0), str(rep)
    assert 1 <= rep.pairing_checks <= 1 + log2_ceil(n)
    assert (rep.points_checked, rep.links_checked) == (n, n - 1)


# ---- 3. one point replaced -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES[1:])
def test_one_point_replaced(cg, srs_of, n):
    s = srs_of(n)
    for k in sorted({0, 1, n // 2, n - 1}):
        pts = s.points.copy()
        pts[k] = other_points(1, 0xABC + k)[0]
        rep = checked(cg, pts, s, locate=False)
        assert (rep.verdict, rep.first_bad_link, rep.pairing_checks) == (2, NONE, 1), (n, k)
        rep = checked(cg, pts, s)
        assert (rep.verdict, rep.first_bad_link) == (2, max(k - 1, 0)), (n, k, str(rep))
        assert rep.pairing_checks <= 1 + log2_ceil(n)


# ---- 4. the tail under another tau -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 257, 1025, 4097])
def test_tail_under_another_tau(cg, srs_of, tau, n):
    s = srs_of(n)
    for k in (1, 63, 64, 1024):
        if k + 1 >= n:      # the tail needs a point behind P[k]
            continue
        base = pow(tau, k, bn.R)
        tail = cr.g1_fixed_base_batch(cr.ints_to_array([base * pow(TAU2, i - k, bn.R) % bn.R for i in range(k, n)]))
        assert np.array_equal(tail[0], s.points[k])
        pts = np.concatenate([s.points[:k], tail])
        rep = checked(cg, pts, s)
        assert (rep.verdict, rep.first_bad_link) == (2, k), (n, k, str(rep))
        assert rep.pairing_checks <= 1 + log2_ceil(n)


# ---- 5. two points swapped -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES[2:])
def test_two_points_swapped(cg, srs_of, n):
    s = srs_of(n)
    a, b = n // 3, n - 1
    pts = s.points.copy()
    pts[[a, b]] = pts[[b, a]]
    rep = checked(cg, pts, s)
    assert (rep.verdict, rep.first_bad_link) == (2, max(a - 1, 0)), str(rep)


# ---- 6. point faults -------------------------------------------------------------------------------------------------------
def off_curve(pt):
    q = pt.copy()
    q[4] += np.uint64(1)      # (x, y + 1), in the words a caller edits
    return q


@pytest.mark.parametrize("n", SIZES)
def test_point_faults_name_the_lowest_index_and_its_kind(cg, srs_of, n):
    s = srs_of(n)
    for k in sorted({k for k in (0, 63, 64, 255, 256, n - 1) if k < n}):
        for kind, bad in ((2, off_curve(s.points[k])), (1, np.zeros(8, np.uint64))):
            pts = s.points.copy()
            pts[k] = bad
            rep = checked(cg, pts, s)
            assert (rep.verdict, rep.point_fault, rep.first_bad_point) == (1, kind, k), (n, k, kind, str(rep))
            assert (rep.pairing_checks, rep.links_checked, rep.first_bad_link, rep.points_checked) == (0, 0, NONE, n)
            assert not fold(rep, "fold_a").any() and not fold(rep, "fold_b").any(), "no fold on what is no group element"


@pytest.mark.parametrize("n", [1025, 4097])
def test_two_faults_in_different_workgroups_report_the_lower(cg, srs_of, n):
    s = srs_of(n)
    for lo, hi, kind_lo in ((70, 900, 1), (300, n - 1, 2), (255, 256, 2)):
        pts = s.points.copy()
        pts[lo] = off_curve(s.points[lo]) if kind_lo == 2 else 0
        pts[hi] = 0 if kind_lo == 2 else off_curve(s.points[hi])
        rep = checked(cg, pts, s)
        assert (rep.verdict, rep.point_fault, rep.first_bad_point, rep.pairing_checks) == (1, kind_lo, lo, 0), str(rep)


# ---- 7. pairing checks, 8. scratch -------------------------------------------------------------------------------------------
def test_pairing_checks_are_counted(cg, srs_of):
    s = srs_of(257)
    pts = s.points.copy()
    pts[200] = other_points(1)[0]
    w0 = cg.pairing_stats()["wave_checks"]
    plain = checked(cg, pts, s, locate=False)
    w1 = cg.pairing_stats()["wave_checks"]
    located = checked(cg, pts, s)
    w2 = cg.pairing_stats()["wave_checks"]
    assert plain.pairing_checks == 1 and w1 - w0 == 1
    assert 2 <= located.pairing_checks <= 1 + log2_ceil(257) and w2 - w1 == located.pairing_checks
    assert located.first_bad_link == 199


def test_arguments_and_the_scratch_limit(cg, srs_of):
    s = srs_of(4097)
    with pytest.raises(cg.CapGpuError) as e:
        cg.srs_check(0xDEAD0000, s.h, s.beta_h)
    assert e.value.code == -4
    L = cg.load()
    rep = cg.SrsReport()
    p16 = lambda a: a.ctypes.data_as(cg.u64p)  # noqa: E731
    assert L.capgpu_srs_check(ctypes.c_uint64(s.handle), p16(s.h), p16(s.beta_h), None, ctypes.c_uint32(4),
                              ctypes.byref(rep)) == -1
    g0 = cg.scratch_stats()
    cg.trim()
    assert cg.srs_check(s.handle, s.h, s.beta_h, SEED_A).verdict == 0
    g1 = cg.scratch_stats()
    assert g1["grow_events"] > g0["grow_events"], "the workspace is the context's scratch"
    cg.trim()
    cg.set_memory_limit(4096)      # the 4096 weights alone are 128 KiB
    try:
        with pytest.raises(cg.CapGpuError) as e:
            cg.srs_check(s.handle, s.h, s.beta_h, SEED_A)
        assert e.value.code == -5 and "bytes" in str(e.value) and "capgpu_set_memory_limit" in str(e.value)
    finally:
        cg.set_memory_limit(0)
    assert cg.srs_check(s.handle, s.h, s.beta_h, SEED_A).verdict == 0
