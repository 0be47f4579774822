"""Proving from the circuit's variable assignment (CAPGPU_INPUT_VARS): the witness is one value per variable, the key
holds the wire -> variable table, the five columns are gathered on the device.  Expected proofs are those of the evals
form on the expanded columns, which tests/test_gpu_input_forms.py pins to the C oracle."""
import mmap
import threading

import numpy as np
import pytest

from cap_amd import bench_utils as bu
from tests.test_gpu_input_forms import instance

pytestmark = pytest.mark.gpu


def var_values(sc, wires, num_vars=None, fill_seed=1):
    """the value vector behind `wires` (5 x n ints, sc.witness): value of variable v at index v, Montgomery (num_vars, 4);
    variables that occur in no cell get arbitrary values"""
    nv = sc.num_vars if num_vars is None else num_vars
    rng = bu.SplitMix64(0xF111 + fill_seed)
    vals = [rng.field() for _ in range(nv)]
    for i in range(5):
        col, ids = wires[i], sc.wire_vars[i]
        for j in range(sc.n):
            vals[ids[j]] = col[j]
    return bu.to_mont_array(vals)


def batch(sc, seeds, num_vars=None):
    """-> columns (P, 5, n, 4), variable values (P, num_vars, 4), public inputs, blinders"""
    ws, vs, ps, bls = [], [], [], []
    for s in seeds:
        w, pubs = sc.witness(s)
        ws.append(sc.wires_mont(w))
        vs.append(var_values(sc, w, num_vars, s))
        ps.append(bu.to_mont_array(pubs) if pubs else np.zeros((0, 4), np.uint64))
        bls.append(bu.to_mont_array(bu.blinders(s + 1000)))
    return np.stack(ws), np.stack(vs), np.stack(ps), np.stack(bls)


def two_keys(cg, h, sc):
    """a key made from the table, and a key made from sigma that got the table afterwards"""
    wv = np.array(sc.wire_vars)
    pk_v, _ = cg.plonk_preprocess_vars(h, sc.n, sc.num_inputs, sc.selectors_mont(), wv, sc.num_vars)
    pk_s, _ = cg.plonk_preprocess(h, sc.n, sc.num_inputs, sc.selectors_mont(), sc.sigma_mont())
    cg.plonk_key_set_vars(pk_s, wv, sc.num_vars)
    return pk_v, pk_s


def as_bytes(proofs):
    return [bytes(p) for p in proofs]


@pytest.mark.parametrize("log_n,nin,P", [(4, 1, 1), (6, 0, 3), (9, 27, 5), (12, 7, 9)])
def test_same_proof_bytes_in_every_entry_point(cg, tau, log_n, nin, P):
    sc = bu.synthetic_circuit(log_n, nin, seed=40 + log_n)
    h = cg.srs_generate(tau, sc.n + 3)
    ws, vs, ps, bls = batch(sc, [300 + p for p in range(P)])
    for pk in two_keys(cg, h, sc):
        want = as_bytes(cg.plonk_prove_batch(pk, ws, ps, bls, b"memo", P))
        assert bytes(cg.plonk_prove(pk, vs[P - 1], ps[P - 1], bls[P - 1], b"memo", input_form="vars")) == want[P - 1]
        assert as_bytes(cg.plonk_prove_batch(pk, vs, ps, bls, b"memo", P, input_form="vars")) == want
        d = cg.DevBuf.from_numpy(vs)
        assert as_bytes(cg.plonk_prove_batch_dev(pk, d, ps, bls, b"memo", P, input_form="vars")) == want
        assert np.array_equal(d.to_numpy().reshape(vs.shape), vs), "the caller's device buffer must stay untouched"
        d.free()
        assert as_bytes(cg.plonk_prove_batch_async(pk, vs, ps, bls, b"memo", P, input_form="vars").wait()) == want
        cg.plonk_free_key(pk)
    cg.srs_free(h)


def test_modes_and_replay(cg, tau):
    sc = bu.synthetic_circuit(9, 27, seed=49)
    h = cg.srs_generate(tau, sc.n + 3)
    P = 3
    ws, vs, ps, bls = batch(sc, [400 + p for p in range(P)])
    pk, pk2 = two_keys(cg, h, sc)
    want = as_bytes(cg.plonk_prove_batch(pk, ws, ps, bls, b"memo", P))
    mode = cg.plonk_get_transcript()
    try:
        cg.plonk_set_transcript("device")
        assert as_bytes(cg.plonk_prove_batch(pk, vs, ps, bls, b"memo", P, input_form="vars")) == want
    finally:
        cg.plonk_set_transcript(mode)
    cg.plonk_set_precheck(True)
    try:
        assert as_bytes(cg.plonk_prove_batch(pk, vs, ps, bls, b"memo", P, input_form="vars")) == want
    finally:
        cg.plonk_set_precheck(False)
    for _ in range(3):  # direct launches, graph capture, graph replay (where the runtime allows replay)
        assert as_bytes(cg.plonk_prove_batch(pk, vs, ps, bls, b"memo", P, input_form="vars")) == want
    # other values behind the same signature: a replayed graph must read this call's gather, not the last one's
    ws2, vs2, ps2, _ = batch(sc, [450 + p for p in range(P)])
    assert as_bytes(cg.plonk_prove_batch(pk, vs2, ps2, bls, b"memo", P, input_form="vars")) == \
        as_bytes(cg.plonk_prove_batch(pk, ws2, ps2, bls, b"memo", P))
    for k in (pk, pk2):
        cg.plonk_free_key(k)
    cg.srs_free(h)


def test_multi_rows_padded_to_the_largest_key(cg, tau):
    log_n = 6
    n = 1 << log_n
    h = cg.srs_generate(tau, n + 3)
    scs = [bu.synthetic_circuit(log_n, nin, seed=60 + nin) for nin in (0, 3, 5)]
    extra = [0, 40, 7]  # unused ids on top: three different num_vars whatever the circuits' own counts are
    nvs = [sc.num_vars + e for sc, e in zip(scs, extra)]
    assert len(set(nvs)) == 3
    pks = [cg.plonk_preprocess_vars(h, n, sc.num_inputs, sc.selectors_mont(), np.array(sc.wire_vars), nv)[0]
           for sc, nv in zip(scs, nvs)]
    order = [0, 1, 2, 1, 0, 2, 2]
    stride, max_in = max(nvs), 5
    rows = np.zeros((len(order), stride, 4), np.uint64)
    rows[:] = bu.to_mont_array([12345])[0]  # whatever lies behind a shorter key's values must not matter
    pubs = np.zeros((len(order), max_in, 4), np.uint64)
    bls, single = [], []
    for p, k in enumerate(order):
        sc = scs[k]
        _, vs, ps, bl = batch(sc, [500 + p], nvs[k])
        rows[p, :nvs[k]] = vs[0]
        pubs[p, :sc.num_inputs] = ps[0]
        bls.append(bl[0])
        single.append(bytes(cg.plonk_prove(pks[k], vs[0], ps[0], bl[0], b"m%d" % p, input_form="vars")))
    msgs = [b"m%d" % p for p in range(len(order))]
    keys = [pks[k] for k in order]
    assert as_bytes(cg.plonk_prove_multi(keys, rows, pubs, np.stack(bls), msgs, input_form="vars")) == single
    d = cg.DevBuf.from_numpy(rows)
    assert as_bytes(cg.plonk_prove_multi(keys, d, pubs, np.stack(bls), msgs, input_form="vars")) == single
    d.free()
    assert as_bytes(cg.plonk_prove_multi_async(keys, rows, pubs, np.stack(bls), msgs, input_form="vars").wait()) == single
    for pk in pks:
        cg.plonk_free_key(pk)
    cg.srs_free(h)


def test_key_without_a_table_refuses_the_form(cg, tau):
    sc = bu.synthetic_circuit(6, 2, seed=47)
    h = cg.srs_generate(tau, sc.n + 3)
    pk, _ = cg.plonk_preprocess(h, sc.n, 2, sc.selectors_mont(), sc.sigma_mont())
    _, vs, ps, bls = batch(sc, [1, 2])
    L = cg.load()
    import ctypes
    proofs = (cg.Proof * 2)()
    flat = np.ascontiguousarray(vs.reshape(-1))
    args = (ctypes.c_uint64(pk), 2, flat.ctypes.data_as(cg.u64p), np.ascontiguousarray(ps.reshape(-1)).ctypes.data_as(cg.u64p),
            ctypes.c_size_t(2), None, ctypes.c_size_t(0), np.ascontiguousarray(bls.reshape(-1)).ctypes.data_as(cg.u64p),
            ctypes.c_int(cg.INPUT_VARS), proofs)
    assert L.capgpu_plonk_prove_batch_ex(*args) == -1
    assert b"key has no variable table" in L.capgpu_last_error()
    with pytest.raises(cg.CapGpuError) as e:
        cg.plonk_prove_batch(pk, vs, ps, bls, b"memo", 2, input_form="vars")
    assert e.value.code == -1 and "key has no variable table" in str(e.value)
    with pytest.raises(cg.CapGpuError) as e:
        cg.plonk_reserve(pk, 2, "vars")
    assert e.value.code == -1
    # a ticket submission with such a key creates no ticket
    before = cg.async_stats()["submitted"]
    t = ctypes.c_uint64(77)
    assert L.capgpu_plonk_prove_batch_async(*args, ctypes.byref(t)) == -1
    assert t.value == 0 and cg.async_stats()["submitted"] == before
    with pytest.raises(cg.CapGpuError) as e:
        cg.plonk_prove_batch_async(pk, vs, ps, bls, b"memo", 2, input_form="vars")
    assert e.value.code == -1 and cg.async_stats()["submitted"] == before
    # values 3 and above stay unknown forms
    with pytest.raises(cg.CapGpuError) as e:
        cg.plonk_prove_batch(pk, np.zeros((2, 5, sc.n, 4), np.uint64), ps, bls, b"memo", 2, input_form=3)
    assert e.value.code == -1
    cg.plonk_free_key(pk)
    cg.srs_free(h)


def test_copy_counter_and_reserve(cg, tau):
    sc = bu.synthetic_circuit(9, 27, seed=49)
    n, P = sc.n, 5
    h = cg.srs_generate(tau, n + 3)
    pk, _ = cg.plonk_preprocess_vars(h, n, 27, sc.selectors_mont(), np.array(sc.wire_vars), sc.num_vars)
    ws, vs, ps, bls = batch(sc, [600 + p for p in range(P)])

    def moved(fn):
        a = cg.plonk_input_stats()
        out = fn()
        b = cg.plonk_input_stats()
        return out, b["witness_bytes_h2d"] - a["witness_bytes_h2d"], b["gather_launches"] - a["gather_launches"]

    want, by, g = moved(lambda: as_bytes(cg.plonk_prove_batch(pk, ws, ps, bls, b"c", P)))
    assert by == P * 5 * n * 32 and g == 0
    got, by, g = moved(lambda: as_bytes(cg.plonk_prove_batch(pk, vs, ps, bls, b"c", P, input_form="vars")))
    assert got == want and by == P * sc.num_vars * 32 and g >= 1
    dv, dw = cg.DevBuf.from_numpy(vs), cg.DevBuf.from_numpy(ws)
    got, by, g = moved(lambda: as_bytes(cg.plonk_prove_batch_dev(pk, dv, ps, bls, b"c", P, input_form="vars")))
    assert got == want and by == 0 and g == 1
    got, by, g = moved(lambda: as_bytes(cg.plonk_prove_batch_dev(pk, dw, ps, bls, b"c", P)))
    assert got == want and by == 0 and g == 0
    dv.free()
    dw.free()
    # reserve: a bound context sized for 8 variable-form proofs grows nothing when they come
    ws8, vs8, ps8, bls8 = batch(sc, [700 + p for p in range(8)])
    want8 = as_bytes(cg.plonk_prove_batch(pk, ws8, ps8, bls8, b"r", 8))
    cg.set_device(0)
    try:
        cg.trim()
        cg.plonk_reserve(pk, 8, "vars", 0)
        g0 = cg.scratch_stats()
        got8 = as_bytes(cg.plonk_prove_batch(pk, vs8, ps8, bls8, b"r", 8, input_form="vars"))
        g1 = cg.scratch_stats()
        assert got8 == want8
        assert g1["grow_events"] == g0["grow_events"] and g1["grow_bytes"] == g0["grow_bytes"], (g0, g1)
    finally:
        cg.set_device(-1)
    cg.plonk_free_key(pk)
    cg.srs_free(h)


def at_end_of_a_mapping(a):
    """a copy of `a` whose last byte is the last byte of an allocation of its own (whole pages): a read past the array
    leaves the allocation"""
    size = (a.nbytes + mmap.PAGESIZE - 1) // mmap.PAGESIZE * mmap.PAGESIZE
    m = mmap.mmap(-1, size)
    out = np.frombuffer(m, dtype=np.uint64, count=a.size, offset=size - a.nbytes).reshape(a.shape)
    out[...] = a
    return out, m


def test_coalesced_calls_of_keys_with_different_num_vars(cg, tau):
    """Concurrent single-proof calls of two keys of one domain are gathered into one batch whose rows have the larger
    num_vars; every caller brings only the num_vars values of ITS key, and no more than those may be read."""
    log_n = 6
    n = 1 << log_n
    h = cg.srs_generate(tau, n + 3)
    scs = [bu.synthetic_circuit(log_n, 2, seed=71), bu.synthetic_circuit(log_n, 4, seed=72)]
    nvs = [scs[0].num_vars, scs[1].num_vars + 300]
    assert nvs[0] < nvs[1]
    pks = [cg.plonk_preprocess_vars(h, n, sc.num_inputs, sc.selectors_mont(), np.array(sc.wire_vars), nv)[0]
           for sc, nv in zip(scs, nvs)]
    T = 8
    calls, keep = [], []
    for t in range(T):
        k = t % 2
        _, vs, ps, bl = batch(scs[k], [900 + t], nvs[k])
        v, m = at_end_of_a_mapping(vs[0])
        keep.append(m)
        calls.append((pks[k], v, ps[0], bl[0], b"c%d" % t))
    alone = [bytes(cg.plonk_prove(pk, v, ps, bl, msg, input_form="vars")) for pk, v, ps, bl, msg in calls]
    results = [None] * T
    start = threading.Barrier(T)

    def worker(t):
        pk, v, ps, bl, msg = calls[t]
        start.wait()
        try:
            results[t] = cg.plonk_prove(pk, v, ps, bl, msg, input_form="vars")
        except cg.CapGpuError as err:
            results[t] = err

    cg.plonk_set_precheck(False)
    cg.plonk_set_coalescing(5000, 16)
    try:
        b0 = cg.plonk_coalescing_stats()
        i0 = cg.plonk_input_stats()
        threads = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(timeout=300)
        i1 = cg.plonk_input_stats()
        b1 = cg.plonk_coalescing_stats()
    finally:
        cg.plonk_set_coalescing(0)
    print("batches", b1[0] - b0[0], "proofs", b1[1] - b0[1])
    for t in range(T):
        assert not isinstance(results[t], Exception), results[t]
        assert bytes(results[t]) == alone[t], f"caller {t}"
    assert b1[1] - b0[1] == T
    # every caller's own values went over the link, and nothing beyond them
    assert i1["witness_bytes_h2d"] - i0["witness_bytes_h2d"] == sum(32 * nvs[t % 2] for t in range(T))
    del calls
    for pk in pks:
        cg.plonk_free_key(pk)
    cg.srs_free(h)
