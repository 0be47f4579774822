"""The one-shot MSM (capgpu_msm_g1_var*: caller points, no SRS handle, no window table) on a real MI355X against the C
oracle, bit-exact in affine form."""
import contextlib
import ctypes
import os
import threading

import numpy as np
import pytest

from oracle import bn254 as bn
from oracle import capref as cr

pytestmark = pytest.mark.gpu

NMAX = (1 << 16) + 1
SIZES = [0, 1, 2, 3, 31, 32, 33, 1000, 1024, 1025, 4099, 8192, NMAX]


def aff(jac):
    return cr.g1_to_affine(jac)


@contextlib.contextmanager
def env(**kv):
    """the plan's overrides are read per call"""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def bases():
    b = cr.g1_fixed_base_batch(cr.random_field(311, 1, NMAX, False))
    b[5] = 0              # point at infinity among the bases
    b[7] = b[6]           # duplicate base (forces P + P in a bucket)
    b.setflags(write=False)
    return b


def edge_scalars(n, seed):
    sc = cr.random_field(seed + n, 1, max(n, 1), False)[:n]
    if n >= 16:
        sc[0] = 0
        sc[1] = cr.int_to_limbs(1)
        sc[2] = cr.int_to_limbs(bn.R - 1)
        sc[3] = cr.int_to_limbs(2**13 - 1)
        sc[4] = cr.int_to_limbs(2**13)
        sc[6] = cr.int_to_limbs(5)
        sc[7] = cr.int_to_limbs(bn.R - 5)     # P and -P cancel to infinity inside one bucket
        sc[8] = cr.int_to_limbs(2**12)
        sc[9] = cr.int_to_limbs(2**12 + 1)
    return sc


@pytest.fixture(scope="module")
def cases(bases):
    """(scalars, oracle result) per size, computed once"""
    out = {}
    for n in SIZES:
        sc = edge_scalars(n, 40)
        sc.setflags(write=False)
        out[n] = (sc, aff(cr.msm_g1(bases[:n], sc)) if n else None)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_var_msm_vs_c_oracle(cg, bases, cases, n):
    sc, want = cases[n]
    got = cg.msm_g1_var(bases[:n], sc)
    if n == 0:
        assert not got[8:].any()              # Z = 0: infinity
    else:
        assert np.array_equal(aff(got), want)


def test_degenerate_scalar_sets(cg, bases):
    n = 2000
    assert cr.affine_to_ints(aff(cg.msm_g1_var(bases[:n], np.zeros((n, 4), np.uint64)))) is None
    same = np.tile(cr.int_to_limbs(0x1234567 << 100 | 0xABCDE), (n, 1))   # every point of a window in ONE bucket
    assert np.array_equal(aff(cg.msm_g1_var(bases[:n], same)), aff(cr.msm_g1(bases[:n], same)))
    # any 256-bit integer is taken: k and k mod r give the same point
    big = np.full((40, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    red = cr.ints_to_array([((1 << 256) - 1) % bn.R] * 40)
    got = aff(cg.msm_g1_var(bases[:40], big))
    assert np.array_equal(got, aff(cg.msm_g1_var(bases[:40], red)))
    assert np.array_equal(got, aff(cr.msm_g1(bases[:40], red)))


def test_stride_72_and_canonical_coordinates(cg, bases, cases):
    n = 1000
    sc, want = cases[n]
    canon = cr.vec_from_mont(0, bases[:n].reshape(-1, 4)).reshape(n, 8)
    assert np.array_equal(aff(cg.msm_g1_var(canon, sc, montgomery=False)), want)
    wide = np.zeros((n, 72), np.uint8)
    wide[:, :64] = bases[:n].copy().view(np.uint8).reshape(n, 64)
    wide[5, :64] = 0xA5                        # garbage coordinates behind a set infinity flag: the flag wins
    wide[5, 64] = 1
    assert np.array_equal(aff(cg.msm_g1_var(wide, sc)), want)
    wide_canon = np.zeros((n, 72), np.uint8)
    wide_canon[:, :64] = canon.view(np.uint8).reshape(n, 64)
    wide_canon[5, 64] = 1
    assert np.array_equal(aff(cg.msm_g1_var(wide_canon, sc, montgomery=False)), want)


def test_batch_of_ragged_msms_over_their_own_bases(cg, bases):
    ns = [10, 700, 1000, 1, 0]
    starts = [0, 100, 2000, 6, 0]             # distinct base ranges (the fourth: the duplicated point alone)
    bl = [bases[s:s + n] for s, n in zip(starts, ns)]
    sl = [cr.random_field(900 + i, 1, max(n, 1), False)[:n] for i, n in enumerate(ns)]
    got = cg.msm_g1_var_batch(bl, sl)
    for i, n in enumerate(ns):
        if n == 0:
            assert not got[i][8:].any()
            continue
        want = aff(cr.msm_g1(bl[i], sl[i]))
        assert np.array_equal(aff(got[i]), want), i
        assert np.array_equal(aff(cg.msm_g1_var(bl[i], sl[i])), want), i


def test_device_resident_form_leaves_the_bases_alone(cg, bases):
    n, stride, count = 1500, 1700, 3
    scs = [cr.random_field(700 + i, 1, n, False) for i in range(count)]
    mont = np.zeros((count, stride, 4), np.uint64)
    mont[:] = 0xDEADBEEF                      # the slack between the arrays is never read as scalars
    for i in range(count):
        mont[i, :n] = cr.vec_to_mont(1, scs[i])
    d_b = cg.DevBuf.from_numpy(bases[:n])
    d_s = cg.DevBuf.from_numpy(mont)
    out = cg.msm_g1_var_dev(d_b, d_s, n, count=count, stride=stride, montgomery=True).to_numpy().reshape(count, 12)
    for i in range(count):
        assert np.array_equal(aff(out[i]), aff(cr.msm_g1(bases[:n], scs[i]))), i
    assert np.array_equal(d_b.to_numpy().reshape(n, 8), bases[:n])
    d_b.free()
    d_s.free()


def test_agrees_with_the_fixed_base_path(cg, bases, cases):
    n = 4099
    sc, want = cases[n]
    h = cg.srs_upload(bases[:n])
    fixed = aff(cg.msm_g1(h, sc))
    cg.srs_free(h)
    assert np.array_equal(aff(cg.msm_g1_var(bases[:n], sc)), fixed)
    assert np.array_equal(fixed, want)


@pytest.mark.parametrize("knobs", [
    {"CAPGPU_MSM_VAR_SUB": 1024},                                   # parts: 5 sub-ranges per window, summed by the tail
    {"CAPGPU_MSM_VAR_SUB": 1024, "CAPGPU_MSM_VAR_RANGE": 2048},      # range split: three launches, results added
    {"CAPGPU_MSM_VAR_SLICE": 1},                                     # MSMs of a batch launch by launch
    {"CAPGPU_MSM_VAR_C": 11},                                        # another window size
], ids=lambda k: "-".join(f"{a[15:].lower()}{b}" for a, b in k.items()))
def test_forced_branches(cg, bases, cases, knobs):
    n = 4099
    sc, want = cases[n]
    plain = cg.msm_var_plan(n, 2)
    with env(**knobs):
        pl = cg.msm_var_plan(n, 2)
        assert pl != plain, "the override did not change the plan"
        if "CAPGPU_MSM_VAR_SUB" in knobs:
            assert pl["parts"] == 5
        if "CAPGPU_MSM_VAR_RANGE" in knobs:
            assert pl["ranges"] == 3
        if "CAPGPU_MSM_VAR_SLICE" in knobs:
            assert pl["slice"] == 1
        if "CAPGPU_MSM_VAR_C" in knobs:
            assert pl["c"] == 11
        assert np.array_equal(aff(cg.msm_g1_var(bases[:n], sc)), want)
        sc2 = cases[1000][0]
        got = cg.msm_g1_var_batch([bases[:n], bases[:1000]], [sc, sc2])
        assert np.array_equal(aff(got[0]), want) and np.array_equal(aff(got[1]), cases[1000][1])


def test_no_table_is_built(cg, bases, cases):
    n = 1 << 16
    pl = cg.msm_var_plan(n, 1)
    assert pl["workspace_bytes"] < 20 * 64 * n     # the smallest window table capgpu_srs_upload builds for n points
    sc = cases[NMAX][0][:n]
    first = cg.msm_g1_var(bases[:n], sc)
    before = cg.scratch_stats()
    second = cg.msm_g1_var(bases[:n], sc)
    assert cg.scratch_stats() == before            # nothing grew: the second call found its scratch in place
    assert np.array_equal(aff(first), aff(second))


def test_two_contexts_at_once(cg, bases, cases):
    n_ctx = ctypes.c_int(0)
    cg.check(cg.load().capgpu_context_count(ctypes.byref(n_ctx)))
    assert n_ctx.value >= 2, "this case needs two contexts: capgpu_init gives a device four by default"
    sizes = (4099, 1025)
    got, errs = [[None] * 3 for _ in sizes], []
    start = threading.Barrier(len(sizes))

    def worker(t):
        try:
            cg.set_device(t)
            start.wait()
            for r in range(3):
                got[t][r] = aff(cg.msm_g1_var(bases[:sizes[t]], cases[sizes[t]][0]))
        except Exception as e:                          # noqa: BLE001
            errs.append(e)
            start.abort()
        finally:
            cg.set_device(-1)
    th = [threading.Thread(target=worker, args=(t,)) for t in range(len(sizes))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for t, n in enumerate(sizes):
        for r in range(3):
            assert np.array_equal(got[t][r], cases[n][1]), (t, r)
