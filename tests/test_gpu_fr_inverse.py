"""Fr inversion in two forms on the device (capgpu_fr_set_inverse_form): Fermat's power - the default - and the constant-time
GCD of cap_amd/csrc/invgcd29.hpp.  The batch call (capgpu_fr_inverse_batch[_dev]) against pow(x, -1, r) in Python integers;
the witness solver, the hints and capgpu_plonk_prove_given under the GCD form against the walk / the model AND against the
Fermat form of the same call, word for word; capgpu_fr_inverse_stats shows which kernel ran."""
import contextlib

import numpy as np
import pytest

from cap_amd import bench_utils as bu
from cap_amd.lib import HINT_INV0, HINT_ISZERO
from tests.solve_hints_model import walk_hints
from tests.test_gpu_prove_each import ERR_PROOF, modes, signature
from tests.test_gpu_solve import (given_values, hand_circuit, harness_given, key_for, mont_rows, solve_host_and_dev,
                                  status_tuples, walk, wide_circuit)
from tests.test_gpu_solve_hints import HBuilder
from tests.test_gpu_solve_packed import pack, zero_denominator_circuit

pytestmark = pytest.mark.gpu

R = bu.R
FORMS = ["fermat", "gcd"]
KEY = {"fermat": "fermat_launches", "gcd": "gcd_launches"}


@contextlib.contextmanager
def form(cg, f):
    old = cg.fr_get_inverse_form()
    cg.fr_set_inverse_form(f)
    try:
        yield
    finally:
        cg.fr_set_inverse_form(old)


def launches(cg, fn):
    """-> (fn(), launches it made by form)"""
    s0 = cg.fr_inverse_stats()
    out = fn()
    s1 = cg.fr_inverse_stats()
    return out, {k: s1[k] - s0[k] for k in s0}


def only(f, n):
    return {KEY[f]: n, KEY["gcd" if f == "fermat" else "fermat"]: 0}


# ---- 1. the batch call -------------------------------------------------------------------------------------------------
def edge_values():
    v = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2]
    for k in range(254):
        v += [1 << k, (1 << k) - 1, R - (1 << k)]
    return v


@pytest.fixture(scope="module")
def pool():
    """the edge values, then random ones, 1000 in all: (integers, Montgomery words, inverses' words) - computed once"""
    rng = bu.SplitMix64(0x1A7)
    x = edge_values()
    x += [rng.field() for _ in range(1000 - len(x))]
    inv = [pow(a, -1, R) if a else 0 for a in x]
    return x, bu.to_mont_array(x), bu.to_mont_array(inv)


def test_default_form_is_fermat(cg):
    assert cg.fr_get_inverse_form() == cg.INVERSE_FERMAT == 0


@pytest.mark.parametrize("count", [1, 63, 64, 65, 256, 257, 1000])
@pytest.mark.parametrize("f", FORMS)
def test_batch_inverse_equals_python(cg, pool, f, count):
    _, words, inv = pool
    off = {1: 0, 63: 1, 64: 64, 65: 128, 256: 193, 257: 449, 1000: 706}[count]      # every edge value falls in some window
    idx = [(off + i) % 1000 for i in range(count)]
    x, want = np.ascontiguousarray(words[idx]), inv[idx]
    with form(cg, f):
        got, d = launches(cg, lambda: cg.fr_inverse_batch(x))
        assert d == only(f, 1)
        assert np.array_equal(got, want)
        # device arrays: out of place (the input stays), then in place
        d_in, d_out = cg.DevBuf.from_numpy(x), cg.DevBuf(count * 32)
        _, d = launches(cg, lambda: cg.fr_inverse_batch(d_in, out=d_out))
        assert d == only(f, 1)
        assert np.array_equal(d_out.to_numpy().reshape(-1, 4), want)
        assert np.array_equal(d_in.to_numpy().reshape(-1, 4), x)
        _, d = launches(cg, lambda: cg.fr_inverse_batch(d_in))
        assert d == only(f, 1)
        assert np.array_equal(d_in.to_numpy().reshape(-1, 4), want)
        # ... and the inverse of the inverse is the input (0 stays 0)
        cg.fr_inverse_batch(d_in)
        assert np.array_equal(d_in.to_numpy().reshape(-1, 4), x)
        d_in.free()
        d_out.free()


@pytest.mark.parametrize("f", FORMS)
def test_batch_inverse_edges_and_a_callers_stream(cg, pool, f):
    import torch
    _, words, inv = pool
    x = np.ascontiguousarray(words[:300])
    cg.set_device(0)
    try:
        with form(cg, f):
            # count 0 launches nothing and needs no array; a prefix of a buffer leaves the rest alone
            (_, d) = launches(cg, lambda: cg.load().capgpu_fr_inverse_batch_dev(None, None, 0))
            assert d == only(f, 0)
            assert cg.fr_inverse_batch(np.zeros((0, 4), np.uint64)).shape == (0, 4)
            d_in = cg.DevBuf.from_numpy(x)
            S = torch.cuda.Stream()
            with cg.on_stream(S):
                _, d = launches(cg, lambda: cg.fr_inverse_batch(d_in, count=257))
            cg.sync_all()
            assert d == only(f, 1)
            got = d_in.to_numpy().reshape(-1, 4)
            assert np.array_equal(got[:257], inv[:257]) and np.array_equal(got[257:], x[257:])
            d_in.free()
            # an image that is not canonical (x + r < 2^256) is taken mod r
            val = sum(int(w) << (64 * i) for i, w in enumerate(bu.to_mont_array([5])[0])) + R
            assert val < 1 << 256
            raw = np.array([[(val >> (64 * i)) & (2**64 - 1) for i in range(4)]], np.uint64)
            assert np.array_equal(cg.fr_inverse_batch(raw), bu.to_mont_array([pow(5, -1, R)]))
    finally:
        cg.set_stream(None)
        cg.set_device(-1)


# ---- 2. the solver -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[4, 6], ids=lambda n: "log%d" % n)
def hand(request, cg, tau):
    """the circuit, its key and - computed once - the walk of the 65 witnesses the largest count needs"""
    sc, given = hand_circuit(request.param)
    h, pk, _ = key_for(cg, tau, sc)
    info = cg.plonk_key_set_given(pk, given)
    assert info.inv_rows >= 2 and info.root_rows >= 5
    vals = given_values(sc, given, 65, 4321)
    want = [walk(sc, given, v) for v in vals]
    assert all(w[1] == (0, 0) for w in want)
    yield sc, pk, mont_rows(vals), mont_rows([w[0] for w in want])
    cg.plonk_free_key(pk)
    cg.srs_free(h)


def both_forms(cg, pk, gv):
    """host and _dev solve under each form -> {form: (vars, statuses)}; two launches each, in the form set and no other"""
    out = {}
    for f in ("gcd", "fermat"):
        with form(cg, f):
            out[f], d = launches(cg, lambda: solve_host_and_dev(cg, pk, gv))
        assert d == only(f, 2), (f, d)
    return out


@pytest.mark.parametrize("count", [1, 2, 3, 32, 65])
def test_solver_under_gcd_equals_the_walk_and_fermat(cg, hand, count):
    sc, pk, gv, want = hand
    got = both_forms(cg, pk, np.ascontiguousarray(gv[:count]))
    assert np.array_equal(got["gcd"][0], want[:count])
    assert np.array_equal(got["gcd"][0], got["fermat"][0])
    assert status_tuples(got["gcd"][1]) == status_tuples(got["fermat"][1]) == [(0, 0)] * count


@pytest.mark.parametrize("W", [1, 2, 4, 8, 16])
def test_solver_under_gcd_at_every_forced_pack(cg, hand, W):
    sc, pk, gv, want = hand
    with pack(cg, W):
        s0 = cg.plonk_solve_stats()
        got = both_forms(cg, pk, np.ascontiguousarray(gv[:17]))
        s1 = cg.plonk_solve_stats()
    assert s1["packed_launches"] - s0["packed_launches"] == (4 if W > 1 else 0)
    assert np.array_equal(got["gcd"][0], want[:17]) and np.array_equal(got["gcd"][0], got["fermat"][0])
    assert status_tuples(got["gcd"][1]) == status_tuples(got["fermat"][1]) == [(0, 0)] * 17


def test_wide_levels_under_gcd(cg, tau):
    """levels of 600 rows (200 of them inverted) and of 300 fifth roots: lanes stride, wavefronts hold one kind or mix two"""
    sc, given = wide_circuit()
    h, pk, _ = key_for(cg, tau, sc)
    cg.plonk_key_set_given(pk, given)
    vals = given_values(sc, given, 2, 5)
    got = both_forms(cg, pk, mont_rows(vals))
    assert np.array_equal(got["gcd"][0], mont_rows([walk(sc, given, v)[0] for v in vals]))
    assert np.array_equal(got["gcd"][0], got["fermat"][0])
    assert status_tuples(got["gcd"][1]) == status_tuples(got["fermat"][1]) == [(0, 0)] * 2
    cg.plonk_free_key(pk)
    cg.srs_free(h)


# ---- 3. zero denominators ------------------------------------------------------------------------------------------------
def test_zero_denominators_under_both_forms(cg, tau):
    sc, given, vals, row_a, row_b, ya, yb = zero_denominator_circuit()
    assert row_a < row_b
    h, pk, _ = key_for(cg, tau, sc)
    cg.plonk_key_set_given(pk, given)
    want = [walk(sc, given, v) for v in vals]
    assert [w[1] for w in want] == [(0, 0), (1, row_b), (0, 0), (1, row_a), (0, 0)]
    got = both_forms(cg, pk, mont_rows(vals))
    for f in FORMS:
        vars_out, st = got[f]
        assert status_tuples(st) == [w[1] for w in want], f
        assert np.array_equal(vars_out, mont_rows([w[0] for w in want])), f
        assert not vars_out[1, yb].any() and not vars_out[3, ya].any() and not vars_out[3, yb].any() and vars_out[1, ya].any()
    cg.plonk_free_key(pk)
    cg.srs_free(h)


# ---- 4. hints ---------------------------------------------------------------------------------------------------------------
def test_inv0_hints_under_both_forms(cg, tau):
    """is_zero gadgets on computed values: INV0 sources 0, 1 and random, beside an inverted row and a fifth root"""
    b = HBuilder(6, 1, 77)
    g = [b.var(given=True) for _ in range(8)]
    d, _ = b.lin([g[0], g[1]], [1, -1])
    d_inv, d_zero = b.is_zero(d)
    e, _ = b.lin([g[2]], [1])
    e_inv, e_zero = b.is_zero(e)
    y, _ = b.out([g[3], g[4], g[5], g[6]], ecc=True)
    y_inv, _ = b.is_zero(y)                                      # the inverse of an inverted row's output
    b.root([g[0], y_inv, g[1], g[2]], 2, d_inv)
    b.hints.append((HINT_INV0, g[7], [b.var()]))                 # a given source, its target in no cell
    sc, given, hints = b.finish(), b.given, b.hints
    at = {v: k for k, v in enumerate(given)}
    vals = given_values(sc, given, 4, 19)
    vals[0][at[g[1]]] = vals[0][at[g[0]]]                        # d = 0
    vals[1][at[g[1]]] = (vals[1][at[g[0]]] - 1) % R              # d = 1
    vals[2][at[g[2]]] = 0                                        # e = 0
    vals[3][at[g[2]]] = 1                                        # e = 1
    vals[3][at[g[7]]] = 0
    want = [walk_hints(sc, given, v, hints) for v in vals]
    assert [w[0][d] for w in want[:2]] == [0, 1] and [w[0][d_inv] for w in want[:2]] == [0, 1]
    assert [w[0][d_zero] for w in want] == [1, 0, 0, 0] and [w[0][e_zero] for w in want] == [0, 0, 1, 0]
    assert want[2][0][e_inv] == 0 and want[3][0][e_inv] == 1 and want[2][0][d_inv] == pow(want[2][0][d], -1, R)
    h, pk, _ = key_for(cg, tau, sc)
    _, hinfo = cg.plonk_key_set_given_hints(pk, given, hints)
    assert hinfo.inv_hints == 4 and hinfo.iszero_hints == 3
    got = both_forms(cg, pk, mont_rows(vals))
    assert np.array_equal(got["gcd"][0], mont_rows([w[0] for w in want]))
    assert np.array_equal(got["gcd"][0], got["fermat"][0])
    assert status_tuples(got["gcd"][1]) == status_tuples(got["fermat"][1]) == [w[1] for w in want]
    with pack(cg, 4):                                            # ... and the packed kernel with the hint code
        packed = both_forms(cg, pk, mont_rows(vals))
    assert np.array_equal(packed["gcd"][0], got["gcd"][0]) and np.array_equal(packed["fermat"][0], got["gcd"][0])
    cg.plonk_free_key(pk)
    cg.srs_free(h)


# ---- 5. capgpu_plonk_prove_given, 6. switching forms between calls on one key ----------------------------------------------
def test_prove_given_and_switching_forms_on_one_key(cg, tau):
    sc = bu.synthetic_circuit(6, 5)
    seeds = (11, 12, 13)
    wires, pubs = sc.witnesses_mont(list(seeds), threads=3)
    given, gv = harness_given(sc, wires)
    h, pk, _ = key_for(cg, tau, sc)
    info = cg.plonk_key_set_given(pk, given)
    assert info.inv_rows == 7
    bad = gv.copy()
    bad[1, given.index(sc.pub_vars[0])] = bu.to_mont_array([12345])[0]       # witness 1 does not satisfy the circuit
    bls = np.stack([bu.to_mont_array(bu.blinders(s + 1000)) for s in seeds])
    runs = []
    with modes(cg, "device", True):
        for f in ("fermat", "gcd", "fermat", "gcd"):             # one key, no set-up call between the forms
            with form(cg, f):
                (proofs, outcomes, solved), d = launches(cg, lambda: cg.plonk_prove_given([pk] * 3, bad, pubs, bls, [b"note"] * 3))
                assert d == only(f, 1), (f, d)
                vars_out, st = cg.plonk_solve_vars(pk, gv, 3)
                tick = cg.plonk_prove_given_async([pk] * 3, bad, pubs, bls, [b"note"] * 3).wait()
            runs.append((signature(proofs, outcomes), status_tuples(solved), [bytes(p) for p in proofs],
                         [o.status for o in outcomes], vars_out, status_tuples(st), signature(tick[0], tick[1])))
    first = runs[0]
    assert first[3] == [0, ERR_PROOF, 0] and first[1] == [(0, 0)] * 3
    wv = np.array(sc.wire_vars).reshape(-1)
    assert np.array_equal(first[4][:, wv].reshape(3, 5, sc.n, 4), wires)
    for r in runs[1:]:
        assert r[0] == first[0] and r[1] == first[1] and r[2] == first[2] and r[3] == first[3]
        assert np.array_equal(r[4], first[4]) and r[5] == first[5]
        assert r[6] == first[0], "the ticket reads the form too, and proves the same bytes"
    cg.plonk_free_key(pk)
    cg.srs_free(h)
