"""The Lagrange key builder (cap_amd/csrc/lagrange.hip: lag_load, lag_stage, lag_finish) and the SRS generator
(srs_fixed_base_kernel, fr_powers_kernel) on the MI355X at the inputs a random tau never produces: tau inside the domain
(every live butterfly of the group FFT a doubling paired with a cancellation, all others infinity +- infinity), tau of
order 2n, tau = 0, a single live point, nothing but infinity, and a sparse SRS with duplicates and opposite points.
Every SRS point is [s_i] G with s_i known, so every point of the key is [integer] G with the integer from
tests/lagrange_model.py (checked without a GPU by tests/test_lagrange_model.py) and the point from the CPU oracle's
fixed-base table.  The key is read through cg.lagrange_commit: a unit vector returns one of its points; a result at
infinity is compared as Z = 0, never through an affine conversion.  All comparisons are exact.

cg.lagrange_commit accepts log_n = 0 (a key of 1 + 3 points), so the sizes start there.

Which MSM tables msm_precompute builds for a key of n + 3 points (cap_amd/csrc/msm.hip): the primary table, on 9-bit
windows up to 1024 points and on 13-bit windows above, and from 4096 points the wide table on 15-bit windows as well.  The
small-launch table its rule also names (13-bit primary, at least 1024 points) exists only under CAPGPU_MSM_SMALL_C, which
is off by default and which nothing in the suite sets: it is not built here and not covered.  So the key of 2^10 + 3
points is the first with a 13-bit primary table, and the key of 2^12 + 3 points has the primary and the wide table, each
built from points of which all but one are at infinity in the root(5) cases below.  A single MSM reads the primary table
whatever the key's size; the wide table is read by launches of at least 24 MSMs (choose_plan), which only the prover
makes on this key: test_wide_table_of_a_key_with_one_live_point proves a batch of 24 for that.

Wall time on the MI355X: 9.3 s for the whole module run alone (13 tests; MEASURED_S), 2.7 s of it the library's start-up
in the first test's set-up; the slowest are the batch of 24 proofs at 2^12 (1.9 s) and the whole proofs at log_n = 9
(1.5 s for five SRS, keys and oracle proofs) and at log_n = 6 (0.7 s); every key test is below 0.4 s, and the key of
2^12 + 3 points with its two tables takes 0.13 s."""
import random

import numpy as np
import pytest

from cap_amd import bench_utils as bu
from oracle import capref as cr
from tests import helpers as H
from tests import lagrange_model as M
from tests.test_gpu_lagrange import both_modes

pytestmark = pytest.mark.gpu

R = M.R
SMALL = (0, 1, 2, 6)          # every one of the n + 3 points; 64 + 3 points are two lag_finish blocks
MID = (7, 8, 9)               # one full lag_stage block, two, and a second lag_load block
BIG = (10, 12)                # root(5) only: the first 13-bit primary table, then the wide table beside it
PROOF_TAUS = ("root:5", "order_2n", "root:0", "root:n/2", "zero")       # omega_n^5, omega_2n, 1, r - 1, 0
PROOF_SIZES = (6, 9)
MEASURED_S = 9.3


@pytest.fixture(autouse=True)
def _default_mode_after(cg):
    yield
    cg.plonk_set_wire_commit_from_evals(None)


def make_srs(cg, label, log_n):
    """the family's SRS on the device and its discrete logs; the families with a tau go through cg.srs_generate, and what
    it generated must be the model's points (this pins srs_fixed_base_kernel and fr_powers_kernel at these tau)"""
    n = 1 << log_n
    s = M.family_logs(label, log_n)
    pts = M.points(s)
    if label in M.GENERATED:
        h = cg.srs_generate(M.family_tau(label, log_n), n + 3)
    else:
        h = cg.srs_upload(pts)
    assert np.array_equal(cg.srs_download(h, 0, n + 3), pts), (label, log_n)
    return h, s


def check_point(cg, h, log_n, scalars_mont, want_log, what):
    got = cg.lagrange_commit(h, log_n, scalars_mont)
    if want_log % R == 0:
        assert not got[8:12].any(), what                       # infinity: Z = 0
    else:
        assert got[8:12].any(), what
        assert np.array_equal(cr.g1_to_affine(got), M.points([want_log])[0]), what


ONE = bu.to_mont_array([1])[0]


def unit(j):
    e = np.zeros((j + 1, 4), np.uint64)
    e[j] = ONE
    return e


@pytest.mark.parametrize("log_n", SMALL)
def test_every_key_point_by_unit_vectors(cg, log_n):
    n = 1 << log_n
    ran = []
    for label in M.FAMILIES:
        h, s = make_srs(cg, label, log_n)
        want = M.expected_logs(s, log_n)
        for j in range(n + 3):
            check_point(cg, h, log_n, unit(j), want[j], (label, log_n, j))
        cg.srs_free(h)
        ran.append(label)
    assert tuple(ran) == M.FAMILIES


@pytest.mark.parametrize("log_n", MID)
def test_key_points_and_a_dense_commitment(cg, log_n):
    n = 1 << log_n
    ran = []
    rng = random.Random(700 + log_n)
    for label in M.FAMILIES:
        h, s = make_srs(cg, label, log_n)
        want = M.expected_logs(s, log_n)
        k = M.root_index(label, log_n) if label.startswith("root:") else 5
        idx = [0, 1, k, n // 2, n - 1, n, n + 1, n + 2] + [rng.randrange(n + 3) for _ in range(8)]
        for j in idx:
            check_point(cg, h, log_n, unit(j), want[j], (label, log_n, j))
        c = [rng.randrange(1, R) for _ in range(n + 3)]        # n values and three blinders, none of them zero
        check_point(cg, h, log_n, bu.to_mont_array(c), M.commit_log(want, c), (label, log_n, "dense"))
        cg.srs_free(h)
        ran.append(label)
    assert tuple(ran) == M.FAMILIES


@pytest.mark.parametrize("log_n", BIG)
def test_key_of_one_live_point_read_from_its_primary_table(cg, log_n):
    """root(5): the key is delta_5 and the blinding points are at infinity - n + 2 of the n + 3 points its tables are built
    from.  Every call here is ONE MSM, which reads the 13-bit primary table (see the module docstring)"""
    n = 1 << log_n
    assert n + 3 >= 1024 and (log_n == 10) == (n + 3 < 4096)
    h, s = make_srs(cg, "root:5", log_n)
    assert cg.msm_plan(h, n + 3, 1)["c"] == 13              # (the SRS table has the key's size and follows the same rule)
    want = M.expected_logs(s, log_n)
    assert want == [1 if j == 5 else 0 for j in range(n)] + [0, 0, 0]
    rng = random.Random(log_n)
    for j in [0, 1, 5, n // 2, n - 1, n, n + 1, n + 2] + [rng.randrange(n + 3) for _ in range(8)]:
        check_point(cg, h, log_n, unit(j), want[j], (log_n, j))
    c = [rng.randrange(1, R) for _ in range(n + 3)]
    check_point(cg, h, log_n, bu.to_mont_array(c), c[5], (log_n, "dense"))
    cg.srs_free(h)


def test_wide_table_of_a_key_with_one_live_point(cg):
    """The wide (15-bit) table of the root(5) key at 2^12 + 3 points is read by launches of at least 24 MSMs only: a batch
    of 24 proofs commits its wires in one launch of 120 MSMs and its permutation products in one of 24, from values on the
    Lagrange key.  With L = delta_5 and the blinding points at infinity a wire commitment is [w_5] G, w_5 the wire's value
    in row 5: an integer.  The permutation products have no such closed form here; they are pinned by the equality of the
    proof bytes with the coefficient mode (which never touches the key) and by the C oracle for the first proof."""
    log_n, nin, P = 12, 3, 24
    sc = bu.synthetic_circuit(log_n, nin, seed=72)
    n = sc.n
    h, s = make_srs(cg, "root:5", log_n)
    assert M.expected_logs(s, log_n) == [1 if j == 5 else 0 for j in range(n)] + [0, 0, 0]
    # the SRS table has the key's size and follows the same rule: 13-bit windows for a lone MSM, the wide table from 24
    assert cg.msm_plan(h, n + 2, 5 * P)["c"] == 15 and cg.msm_plan(h, n + 3, P)["c"] == 15
    assert cg.msm_plan(h, n + 3, P - 1)["c"] == 13
    ws, ps = sc.witnesses_mont([800 + p for p in range(P)])
    bls = np.stack([bu.to_mont_array(bu.blinders(850 + p)) for p in range(P)])
    pk, _ = cg.plonk_preprocess(h, n, nin, sc.selectors_mont(), sc.sigma_mont())
    try:
        kept = []

        def prove():
            kept[:] = cg.plonk_prove_batch(pk, ws, ps, bls, b"wide", P)
            return kept
        a, b = both_modes(cg, prove)                           # from coefficients, then from values on the Lagrange key
        assert a == b and len(set(a)) == P
        w5 = [H.fr_to_ints(ws[p][:, 5])[i] for p in range(P) for i in range(5)]
        want = M.points(w5)
        assert len({x for x in w5}) > P                        # not a degenerate row
        for p in range(P):
            for i in range(5):
                got = np.ctypeslib.as_array(kept[p].wires_poly_comms[i]).reshape(-1)
                assert np.array_equal(got, want[5 * p + i].reshape(-1)), (p, i)
        key = cr.PlonkKey(cg.srs_download(h, 0, n + 3), n, nin, sc.selectors_mont(), sc.sigma_mont())
        rc, comms, evals = key.prove(ws[0], ps[0], bls[0], b"wide")
        assert rc == 0 and H.proof_points(kept[0]) == H.cref_proof_points(comms, evals)
    finally:
        cg.plonk_free_key(pk)
        cg.srs_free(h)


@pytest.mark.parametrize("log_n", PROOF_SIZES)
def test_whole_proofs_at_degenerate_tau(cg, log_n):
    nin, P = 3, 2
    sc = bu.synthetic_circuit(log_n, nin, seed=60 + log_n)
    n = sc.n
    ws, ps = sc.witnesses_mont([300 + p for p in range(P)])
    bls = np.stack([bu.to_mont_array(bu.blinders(400 + p)) for p in range(P)])
    g2h = cg.g2_generator()
    ran = []
    for label in PROOF_TAUS:
        tau = M.family_tau(label, log_n)
        h, _ = make_srs(cg, label, log_n)
        pk, vk = cg.plonk_preprocess(h, n, nin, sc.selectors_mont(), sc.sigma_mont())
        kept = []

        def prove():
            kept[:] = cg.plonk_prove_batch(pk, ws, ps, bls, b"edge", P)
            return kept
        a, b = both_modes(cg, prove)                           # from coefficients, then from values on the Lagrange key
        assert a == b and len(set(a)) == P, label
        proofs = list(kept)
        key = cr.PlonkKey(cg.srs_download(h, 0, n + 3), n, nin, sc.selectors_mont(), sc.sigma_mont())
        rc, comms, evals = key.prove(ws[0], ps[0], bls[0], b"edge")
        assert rc == 0 and H.proof_points(proofs[0]) == H.cref_proof_points(comms, evals), label
        if tau != 0:
            bh = cg.g2_mul(g2h, tau)
            for p in range(P):
                assert cg.plonk_verify(vk, g2h, bh, ps[p], proofs[p], b"edge"), (label, p)
            assert not cg.plonk_verify(vk, g2h, bh, ps[1], proofs[0], b"edge"), label
        # tau = 0: beta_h = [0] h is the point at infinity of G2, which the pairing check has no encoding for, so
        # verification is left out; the proof is pinned by the two comparisons above
        cg.plonk_free_key(pk)
        cg.srs_free(h)
        ran.append(label)
    assert tuple(ran) == PROOF_TAUS
    assert [M.family_tau(t, log_n) for t in PROOF_TAUS] == [pow(M.omega(log_n), 5, R), M.omega(log_n + 1), 1, R - 1, 0]


def test_the_roster():
    assert (SMALL, MID, BIG, PROOF_SIZES) == ((0, 1, 2, 6), (7, 8, 9), (10, 12), (6, 9))
    assert len(M.FAMILIES) == 12 and len(set(M.FAMILIES)) == 12
