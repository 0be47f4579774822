"""The packed witness solver (k_solve_vars_packed<W>, capgpu_plonk_set_solve_pack): W witnesses per workgroup, the lanes
striding over a level's (row, witness) items.  Whatever W, vars_out equals the walk of tests/test_gpu_solve.py word for
word and the statuses are the unpacked kernel's; capgpu_plonk_solve_stats tells which kernel ran."""
import contextlib

import numpy as np
import pytest

from cap_amd import bench_utils as bu
from tests.test_gpu_solve import (Builder, Q_ECC, Q_O, R, given_values, hand_circuit, harness_given, key_for, mont_rows,
                                  solve_host_and_dev, status_tuples, walk, wide_circuit)

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def pack(cg, w):
    old = cg.plonk_get_solve_pack()
    cg.plonk_set_solve_pack(w)
    try:
        yield
    finally:
        cg.plonk_set_solve_pack(old)


def stats_delta(cg, fn):
    s0 = cg.plonk_solve_stats()
    out = fn()
    s1 = cg.plonk_solve_stats()
    return out, {k: s1[k] - s0[k] for k in s0}


@pytest.fixture(scope="module", params=[4, 6], ids=lambda n: "log%d" % n)
def hand(request, cg, tau):
    """the circuit, its key and - computed once - the walk of the 35 witnesses the largest count needs"""
    sc, given = hand_circuit(request.param)
    h, pk, _ = key_for(cg, tau, sc)
    cg.plonk_key_set_given(pk, given)
    vals = given_values(sc, given, 2 * 16 + 3, 321)
    want = [walk(sc, given, v) for v in vals]
    assert all(w[1] == (0, 0) for w in want)
    yield sc, pk, mont_rows(vals), mont_rows([w[0] for w in want])
    cg.plonk_free_key(pk)
    cg.srs_free(h)


@pytest.mark.parametrize("W", [2, 4, 8, 16])
def test_forced_w_equals_the_walk(cg, hand, W):
    sc, pk, gv, want = hand
    with pack(cg, W):
        for count in (1, W - 1, W + 1, 2 * W + 3):
            (got, st), d = stats_delta(cg, lambda: solve_host_and_dev(cg, pk, gv[:count]))
            assert np.array_equal(got, want[:count]), (W, count)
            assert status_tuples(st) == [(0, 0)] * count
            # the host call and the _dev call: two launches, packed unless the launch holds one witness
            assert d == dict(launches=2, witnesses=2 * count, packed_launches=2 if count > 1 else 0), (W, count)


def test_wide_levels_at_sixteen_per_workgroup(cg, tau):
    """levels of 600 and 300 rows: 9 600 and 4 800 items at W = 16, inversions and fifth roots inside one level; 5 of the
    one workgroup's 16 slots hold a witness"""
    sc, given = wide_circuit()
    h, pk, _ = key_for(cg, tau, sc)
    cg.plonk_key_set_given(pk, given)
    vals = given_values(sc, given, 5, 55)
    with pack(cg, 16):
        (got, st), d = stats_delta(cg, lambda: solve_host_and_dev(cg, pk, mont_rows(vals)))
    assert np.array_equal(got, mont_rows([walk(sc, given, v)[0] for v in vals])) and status_tuples(st) == [(0, 0)] * 5
    assert d["packed_launches"] == 2
    cg.plonk_free_key(pk)
    cg.srs_free(h)


def zero_denominator_circuit():
    """the circuit of tests/test_gpu_solve.py::test_zero_denominators_name_the_lowest_row, from the same recipe: rows A < B
    invert q_o - q_ecc w0 w1 w2 w3 with w0 a given variable of their own -> (circuit, given, values of 5 witnesses whose
    denominators vanish for witness 1 at B and for witness 3 at A and B, row_a, row_b, ya, yb)"""
    b = Builder(6, 1, 23)
    g = [b.var(given=True) for _ in range(8)]
    x, _ = b.out([g[0], g[1], g[2], g[3]])
    ya, row_a = b.out([g[4], g[1], g[2], g[3]], ecc=True)
    z, _ = b.out([ya, x, g[0], g[1]])
    yb, row_b = b.out([g[5], g[2], g[3], g[6]], ecc=True)
    b.root([g[0], yb, g[1], g[2]], 2, z)
    sc, given = b.finish(), b.given
    vals = given_values(sc, given, 5, 77)

    def vanish(v, row, own):
        w = [v[given.index(sc.wire_vars[i][row])] for i in range(1, 4)]
        v[given.index(own)] = sc.selectors[Q_O][row] * pow(sc.selectors[Q_ECC][row] * w[0] * w[1] * w[2] % R, R - 2, R) % R

    vanish(vals[1], row_b, g[5])
    vanish(vals[3], row_b, g[5])
    vanish(vals[3], row_a, g[4])
    return sc, given, vals, row_a, row_b, ya, yb


@pytest.mark.parametrize("W", [4, 8])
def test_a_zero_denominator_stays_in_its_slot(cg, tau, W):
    sc, given, vals, row_a, row_b, ya, yb = zero_denominator_circuit()
    assert row_a < row_b
    h, pk, _ = key_for(cg, tau, sc)
    cg.plonk_key_set_given(pk, given)
    want = [walk(sc, given, v) for v in vals]
    assert [w[1] for w in want] == [(0, 0), (1, row_b), (0, 0), (1, row_a), (0, 0)]
    with pack(cg, W):
        (got, st), d = stats_delta(cg, lambda: solve_host_and_dev(cg, pk, mont_rows(vals)))
    assert d["packed_launches"] == 2
    assert status_tuples(st) == [w[1] for w in want]
    assert np.array_equal(got, mont_rows([w[0] for w in want]))
    assert not got[1, yb].any() and not got[3, ya].any() and not got[3, yb].any() and got[1, ya].any()
    with pack(cg, 1):
        for p in (0, 2, 4):                                      # the neighbours equal their lone solves
            lone, st1 = cg.plonk_solve_vars(pk, mont_rows([vals[p]]), 1)
            assert np.array_equal(lone[0], got[p]) and status_tuples(st1) == [(0, 0)]
    cg.plonk_free_key(pk)
    cg.srs_free(h)


def test_automatic_mode_packs_and_changes_nothing(cg, tau):
    assert cg.plonk_get_solve_pack() == 0, "the default is the automatic rule"
    sc = bu.synthetic_circuit(8, 5)
    wires, _ = sc.witnesses_mont(list(range(500, 564)), threads=4)
    given, gv = harness_given(sc, wires)
    h, pk, _ = key_for(cg, tau, sc)
    cg.plonk_key_set_given(pk, given)
    (got, st), d = stats_delta(cg, lambda: cg.plonk_solve_vars(pk, gv, 64))
    assert d == dict(launches=1, witnesses=64, packed_launches=1)
    with pack(cg, 1):
        (one, st1), d1 = stats_delta(cg, lambda: cg.plonk_solve_vars(pk, gv, 64))
    assert d1 == dict(launches=1, witnesses=64, packed_launches=0)
    assert np.array_equal(got, one) and status_tuples(st) == status_tuples(st1) == [(0, 0)] * 64
    wv = np.array(sc.wire_vars).reshape(-1)
    assert np.array_equal(got[:, wv].reshape(64, 5, sc.n, 4), wires)
    # a lone witness runs the unpacked kernel whatever the schedule says
    _, d = stats_delta(cg, lambda: cg.plonk_solve_vars(pk, gv[:1], 1))
    assert d == dict(launches=1, witnesses=1, packed_launches=0)
    cg.plonk_free_key(pk)
    cg.srs_free(h)
