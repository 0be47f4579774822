"""Proving from the values a circuit is given (capgpu_plonk_prove_given[_dev,_async], capgpu_plonk_reserve_given): the
witness solver and the variable-form outcome call in one.  The contract: proofs and outcomes are bit for bit those of
capgpu_plonk_solve_vars followed by capgpu_plonk_prove_each_dev(..., CAPGPU_INPUT_VARS, ...) in the same modes, and
solved_out is that solve's status."""
import ctypes

import numpy as np
import pytest

from cap_amd import bench_utils as bu
from tests.test_gpu_prove_each import ERR_PROOF, ONES, bound, modes, signature
from tests.test_gpu_solve import given_values, harness_given, key_for, mont_rows, status_tuples, walk
from tests.test_gpu_solve_packed import zero_denominator_circuit

pytestmark = pytest.mark.gpu

TRANSCRIPTS = ["host", "device"]


def two_step(cg, pks, gv_rows, pubs, bls, msgs):
    """the definition: solve every witness under its key (device buffers), then the variable-form outcome call on the
    solved buffer -> (proofs, outcomes, statuses).  gv_rows[i]: proof i's given values, as long as ITS key's list."""
    nv = max(cg.plonk_key_num_vars(pk) for pk in set(pks))
    rows, sts = [], []
    for pk, g in zip(pks, gv_rows):
        d_g = cg.DevBuf.from_numpy(np.ascontiguousarray(g))
        d_v, st = cg.plonk_solve_vars(pk, d_g, 1)
        row = np.zeros((nv, 4), np.uint64)
        v = d_v.to_numpy().reshape(-1, 4)
        row[:v.shape[0]] = v
        rows.append(row)
        sts += status_tuples(st)
        d_g.free()
        d_v.free()
    d = cg.DevBuf.from_numpy(np.stack(rows))
    try:
        proofs, outcomes = cg.plonk_prove_each_dev(list(pks), d, pubs, bls, msgs, input_form="vars")
    finally:
        d.free()
    return proofs, outcomes, sts


class Syn:
    def __init__(self, cg, tau, log_n, nin=5, seeds=(901, 7, 31, 44, 45), seed=None):
        self.sc = bu.synthetic_circuit(log_n, nin) if seed is None else bu.synthetic_circuit(log_n, nin, seed=seed)
        self.P = len(seeds)
        self.wires, self.pubs = self.sc.witnesses_mont(list(seeds), threads=4)
        self.given, self.gv = harness_given(self.sc, self.wires)
        self.h, self.pk, self.vk = key_for(cg, tau, self.sc)
        self.info = cg.plonk_key_set_given(self.pk, self.given)
        self.bls = np.stack([bu.to_mont_array(bu.blinders(s + 1000)) for s in seeds])
        self.msgs = [b"note"] * self.P
        self.cg = cg

    def free(self):
        self.cg.plonk_free_key(self.pk)
        self.cg.srs_free(self.h)


@pytest.fixture(scope="module", params=[6, 8], ids=lambda n: "log%d" % n)
def syn(request, cg, tau):
    s = Syn(cg, tau, request.param)
    yield s
    s.free()


@pytest.fixture(scope="module")
def syn6(cg, tau):
    s = Syn(cg, tau, 6, seeds=(11, 12, 13))
    yield s
    s.free()


# ---- 1. the contract, by every entry point ----------------------------------------------------------------------------------
@pytest.mark.parametrize("transcript", TRANSCRIPTS)
def test_three_entry_points_equal_solve_then_prove(cg, tau, syn, transcript):
    s, P = syn, syn.P
    pks = [s.pk] * P
    with modes(cg, transcript, False):
        want = two_step(cg, pks, s.gv, s.pubs, s.bls, s.msgs)
        batch = [bytes(p) for p in cg.plonk_prove_batch(s.pk, s.wires, s.pubs, s.bls, b"note", P)]
        host = cg.plonk_prove_given(pks, s.gv, s.pubs, s.bls, s.msgs)
        d_g = cg.DevBuf.from_numpy(s.gv)
        dev = cg.plonk_prove_given(pks, d_g, s.pubs, s.bls, s.msgs)
        unchanged = np.array_equal(d_g.to_numpy().reshape(s.gv.shape), s.gv)
        d_g.free()
        tick = cg.plonk_prove_given_async(pks, s.gv, s.pubs, s.bls, s.msgs).wait()
    assert unchanged, "the _dev form must not write d_given"
    assert want[2] == [(0, 0)] * P
    for name, (proofs, outcomes, solved) in (("host", host), ("dev", dev), ("async", tick)):
        assert signature(proofs, outcomes) == signature(want[0], want[1]), name
        assert [bytes(p) for p in proofs] == batch, name
        assert [o.status for o in outcomes] == [0] * P and status_tuples(solved) == [(0, 0)] * P, name
    g2h = cg.g2_generator()
    bh = cg.g2_mul(g2h, tau)
    assert all(cg.plonk_verify(s.vk, g2h, bh, s.pubs[p], host[0][p], b"note") for p in range(P))


# ---- 2. a wrong given value: the batch runs past it ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["nocheck", "precheck", "compact"])
@pytest.mark.parametrize("transcript", TRANSCRIPTS)
def test_one_changed_public_input_of_three(cg, syn6, transcript, mode):
    s, P = syn6, 3
    pks = [s.pk] * P
    bad = s.gv.copy()
    bad[1, s.given.index(s.sc.pub_vars[0])] = bu.to_mont_array([12345])[0]   # the value the solver is given; pubs stay
    with modes(cg, transcript, mode != "nocheck"), bound(cg, 0):
        clean = cg.plonk_prove_given(pks, s.gv, s.pubs, s.bls, s.msgs)
        cg.plonk_set_compaction(mode == "compact")
        try:
            c0 = cg.plonk_compaction_stats()
            proofs, outcomes, solved = cg.plonk_prove_given(pks, bad, s.pubs, s.bls, s.msgs)      # returns: the batch ran
            c1 = cg.plonk_compaction_stats()
            want = two_step(cg, pks, bad, s.pubs, s.bls, s.msgs)
        finally:
            cg.plonk_set_compaction(False)
    assert status_tuples(solved) == [(0, 0)] * P                 # the solver checks nothing
    assert signature(proofs, outcomes) == signature(want[0], want[1])
    for p in (0, 2):
        assert outcomes[p].status == 0 and bytes(proofs[p]) == bytes(clean[0][p])
    o = outcomes[1]
    assert o.status == ERR_PROOF and bytes(proofs[1]) == ONES
    if mode == "nocheck":
        assert o.fault.kind == 0 and o.degree_flags != 0 and c1 == c0
    else:
        assert (o.fault.kind, o.fault.row) == (1, 0)             # the public-input gate of row 0
    if mode == "precheck":
        assert o.degree_flags != 0 and c1 == c0
    if mode == "compact":
        assert o.degree_flags == 0
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, 1)          # one call ran compacted and dropped one proof


# ---- 3. a zero denominator inside a proving call --------------------------------------------------------------------------------
def test_zero_denominator_inside_a_proving_call(cg, tau):
    sc, given, vals, row_a, row_b, ya, yb = zero_denominator_circuit()
    vals = vals[:3]                                              # witness 1: the denominator of row B vanishes
    h, pk, _ = key_for(cg, tau, sc)
    cg.plonk_key_set_given(pk, given)
    gv = mont_rows(vals)
    pubs = mont_rows([[v[given.index(sc.pub_vars[0])]] for v in vals])
    bls = np.stack([bu.to_mont_array(bu.blinders(70 + p)) for p in range(3)])
    msgs = [b"z0", None, b"z2"]
    with modes(cg, "device", False):
        proofs, outcomes, solved = cg.plonk_prove_given([pk] * 3, gv, pubs, bls, msgs)
        want = two_step(cg, [pk] * 3, gv, pubs, bls, msgs)
        assert status_tuples(solved) == want[2] == [(0, 0), (1, row_b), (0, 0)]
        assert signature(proofs, outcomes) == signature(want[0], want[1])
        for p in (0, 2):                                         # the neighbours equal their lone calls
            lone = cg.plonk_prove_given([pk], gv[p:p + 1], pubs[p:p + 1], bls[p:p + 1], msgs[p:p + 1])
            assert signature(lone[0], lone[1]) == signature(proofs[p:p + 1], outcomes[p:p + 1])
            assert outcomes[p].status == 0 and status_tuples(lone[2]) == [(0, 0)]
    # (its variable is 0 and the witness goes on as it is: row B's gate does not hold, the degree check says so)
    assert walk(sc, given, vals[1])[0][yb] == 0 and outcomes[1].status == ERR_PROOF and bytes(proofs[1]) == ONES
    cg.plonk_free_key(pk)
    cg.srs_free(h)


# ---- 4. two keys in one call ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transcript", TRANSCRIPTS)
def test_two_keys_with_given_lists_of_different_lengths(cg, tau, transcript):
    sa, sb = bu.synthetic_circuit(6, 2, seed=71), bu.synthetic_circuit(6, 2, seed=72)
    h = cg.srs_generate(tau, sa.n + 3)
    keys = []
    for sc, seeds, extra in ((sa, [1, 2, 3], False), (sb, [4, 5], True)):
        wires, pubs = sc.witnesses_mont(seeds, threads=2)
        given, gv = harness_given(sc, wires)
        if extra:                                                # the first OUT row's variable is given too: one more value
            first_out = sc.wire_vars[4][sc.num_inputs]
            given = given + [first_out]
            gv = np.concatenate([gv, wires[:, 4, sc.num_inputs][:, None, :]], axis=1)
        pk, _ = cg.plonk_preprocess_vars(h, sc.n, sc.num_inputs, sc.selectors_mont(), np.array(sc.wire_vars), sc.num_vars)
        cg.plonk_key_set_given(pk, given)
        keys.append((pk, gv, pubs, wires))
    (pa, ga, pua, wa), (pb, gb, pub_b, wb) = keys
    assert ga.shape[1] != gb.shape[1]
    order = [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2)]              # A B A B A
    pks = [keys[k][0] for k, _ in order]
    rows = np.zeros((5, max(ga.shape[1], gb.shape[1]), 4), np.uint64)   # rows of the larger list; the other key uses the first of its row
    own = []
    for i, (k, j) in enumerate(order):
        g = keys[k][1][j]
        rows[i, :g.shape[0]] = g
        own.append(g)
    pubs = np.stack([keys[k][2][j] for k, j in order])
    bls = np.stack([bu.to_mont_array(bu.blinders(200 + i)) for i in range(5)])
    msgs = [b"m%d" % i for i in range(5)]
    with modes(cg, transcript, False), bound(cg, 0):
        s0 = cg.plonk_solve_stats()
        proofs, outcomes, solved = cg.plonk_prove_given(pks, rows, pubs, bls, msgs)
        s1 = cg.plonk_solve_stats()
        want = two_step(cg, pks, own, pubs, bls, msgs)
        assert s1["launches"] - s0["launches"] == 2 and s1["witnesses"] - s0["witnesses"] == 5   # one launch per key
        assert signature(proofs, outcomes) == signature(want[0], want[1])
        assert [o.status for o in outcomes] == [0] * 5 and status_tuples(solved) == [(0, 0)] * 5
        for i, (k, j) in enumerate(order):                       # each proof equals its single-key call
            lone = cg.plonk_prove_given([pks[i]], own[i][None], pubs[i:i + 1], bls[i:i + 1], msgs[i:i + 1])
            assert bytes(lone[0][0]) == bytes(proofs[i]), i
            assert bytes(proofs[i]) == bytes(cg.plonk_prove(pks[i], keys[k][3][j], pubs[i], bls[i], msgs[i])), i
    cg.plonk_free_key(pa)
    cg.plonk_free_key(pb)
    cg.srs_free(h)


# ---- 5. counters ------------------------------------------------------------------------------------------------------------------
def test_counters_and_reserve(cg, syn6):
    s, P = syn6, 3
    pks = [s.pk] * P
    with modes(cg, "device", False), bound(cg, 0):
        d_g = cg.DevBuf.from_numpy(s.gv)
        vars_h, _ = cg.plonk_solve_vars(s.pk, s.gv, P)
        d_v = cg.DevBuf.from_numpy(vars_h)
        cg.plonk_prove_given(pks, d_g, s.pubs, s.bls, s.msgs)   # (warm: the first call of a shape may grow scratch)
        i0, w0 = cg.plonk_input_stats(), cg.plonk_sync_stats()
        cg.plonk_prove_given(pks, s.gv, s.pubs, s.bls, s.msgs)
        i1, w1 = cg.plonk_input_stats(), cg.plonk_sync_stats()
        cg.plonk_prove_given(pks, d_g, s.pubs, s.bls, s.msgs)
        i2, w2 = cg.plonk_input_stats(), cg.plonk_sync_stats()
        cg.plonk_prove_each_dev(pks, d_v, s.pubs, s.bls, s.msgs, input_form="vars")
        w3 = cg.plonk_sync_stats()
        assert i1["witness_bytes_h2d"] - i0["witness_bytes_h2d"] == P * len(s.given) * 32
        assert i2["witness_bytes_h2d"] == i1["witness_bytes_h2d"]
        # the status words come back with the proofs: no wait beyond the variable-form call's
        assert w1[1] - w0[1] == w2[1] - w1[1] == w3[1] - w2[1] and (w1[0] - w0[0], w3[0] - w2[0]) == (1, 1)
        # a context sized ahead does not grow
        cg.trim()
        cg.plonk_reserve_given(s.pk, P, 0)
        before = cg.scratch_stats()
        a = cg.plonk_prove_given(pks, s.gv, s.pubs, s.bls, s.msgs)
        b = cg.plonk_prove_given(pks, d_g, s.pubs, s.bls, s.msgs)
        after = cg.scratch_stats()
        assert after["grow_events"] == before["grow_events"], (before, after)
        assert signature(a[0], a[1]) == signature(b[0], b[1])
        d_g.free()
        d_v.free()


# ---- 6. refusals, and a caller's stream ---------------------------------------------------------------------------------------------
def refused(cg, fn, *texts):
    with pytest.raises(cg.CapGpuError) as e:
        fn()
    assert e.value.code == -1
    for t in texts:
        assert t in str(e.value), str(e.value)


def test_refusals_name_the_call(cg, tau, syn6):
    s = syn6
    no_solver = "capgpu_plonk_prove_given: the key has no solver (capgpu_plonk_key_set_given gives it one)"
    sc = s.sc
    # a key with a table and no given list; a key without a table
    pk_t, _ = cg.plonk_preprocess_vars(s.h, sc.n, sc.num_inputs, sc.selectors_mont(), np.array(sc.wire_vars), sc.num_vars)
    pk_s, _ = cg.plonk_preprocess(s.h, sc.n, sc.num_inputs, sc.selectors_mont(), sc.sigma_mont())
    # (the Python wrapper sizes `given` from the key's schedule: the C entry points are called with the arrays as they are)
    L = cg.load()
    b = np.ascontiguousarray(s.bls[:1]).reshape(-1)
    p = np.ascontiguousarray(s.pubs[:1]).reshape(-1)
    g = np.ascontiguousarray(s.gv[:1]).reshape(-1)
    pr, oc, t = (cg.Proof * 1)(), (cg.ProveOutcome * 1)(), ctypes.c_uint64(9)

    def raw(name, pk, *tail):
        h = (ctypes.c_uint64 * 1)(pk)
        given = g.ctypes.data_as(ctypes.c_void_p) if name.endswith("_dev") else cg._p(g)
        return getattr(L, name)(h, 1, given, cg._p(p), ctypes.c_size_t(sc.num_inputs), None, None, cg._p(b), pr, oc, None, *tail)

    for pk in (pk_t, pk_s):
        for name, tail in (("capgpu_plonk_prove_given", ()), ("capgpu_plonk_prove_given_dev", ()),
                           ("capgpu_plonk_prove_given_async", (ctypes.byref(t),))):
            assert raw(name, pk, *tail) == -1 and L.capgpu_last_error().decode() == no_solver, name
    assert t.value == 0, "a refused submission leaves no ticket"
    refused(cg, lambda: cg.plonk_reserve_given(pk_t, 2, 0), "capgpu_plonk_reserve_given: the key has no solver")
    # mixed domain sizes, at submission for tickets (the Python wrapper has a check of its own: the C entry points again)
    other = Syn(cg, tau, 4, nin=1, seeds=(3,))
    try:
        h2 = (ctypes.c_uint64 * 2)(s.pk, other.pk)
        g2 = np.zeros(2 * s.gv.shape[1] * 4, np.uint64)
        p2, b2 = np.zeros(2 * sc.num_inputs * 4, np.uint64), np.ascontiguousarray(s.bls[:2]).reshape(-1)
        pr2, oc2 = (cg.Proof * 2)(), (cg.ProveOutcome * 2)()
        text = "capgpu_plonk_prove_multi: the keys of one batch must share the domain size and the SRS"
        for name, tail in (("capgpu_plonk_prove_given", ()), ("capgpu_plonk_prove_given_async", (ctypes.byref(t),))):
            assert getattr(L, name)(h2, 2, cg._p(g2), cg._p(p2), ctypes.c_size_t(sc.num_inputs), None, None, cg._p(b2), pr2,
                                    oc2, None, *tail) == -1, name
            assert L.capgpu_last_error().decode() == text, name
    finally:
        other.free()
    # an unknown handle
    with pytest.raises(cg.CapGpuError) as e:
        cg.plonk_prove_given([s.pk + 12345], s.gv[:1], s.pubs[:1], s.bls[:1])
    assert e.value.code == -4
    # count == 0: CAPGPU_OK, nothing written
    assert L.capgpu_plonk_prove_given(None, 0, None, None, ctypes.c_size_t(0), None, None, None, None, None, None) == 0
    assert cg.plonk_prove_given([], np.zeros((0, 4), np.uint64), np.zeros((0, 4), np.uint64),
                                np.zeros((0, 4), np.uint64)) == ([], [], [])
    cg.plonk_free_key(pk_t)
    cg.plonk_free_key(pk_s)


def test_on_a_callers_stream(cg, syn6):
    import torch
    s, P = syn6, 3
    pks = [s.pk] * P
    with modes(cg, "device", False), bound(cg, 0):
        d_g = cg.DevBuf.from_numpy(s.gv)
        own = cg.plonk_prove_given(pks, d_g, s.pubs, s.bls, s.msgs)
        S = torch.cuda.Stream()
        try:
            with cg.on_stream(S):
                on_s = cg.plonk_prove_given(pks, d_g, s.pubs, s.bls, s.msgs)
                host_s = cg.plonk_prove_given(pks, s.gv, s.pubs, s.bls, s.msgs)
            cg.sync_all()
        finally:
            cg.set_stream(None)
        d_g.free()
    assert signature(on_s[0], on_s[1]) == signature(host_s[0], host_s[1]) == signature(own[0], own[1])
    assert [o.status for o in own[1]] == [0] * P and status_tuples(on_s[2]) == [(0, 0)] * P
