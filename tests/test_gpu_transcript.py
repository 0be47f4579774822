"""The prover's Fiat-Shamir transcript on the device (capgpu_plonk_set_transcript; cap_amd/csrc/transcript_dev.hpp): the
device sponge against the oracle's Keccak, and device-mode proofs against host-mode proofs - the same capgpu_proof and
the same 769 serialised bytes on identical inputs and blinders - over input forms, wire-commit modes, mixed keys, every
residue of the transcript length mod 136, refusals, synchronisation counts, graph replay and concurrent callers."""
import contextlib
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from cap_amd import bench_utils as bu
from oracle import bn254 as bn
from oracle import capref as cr
from tests import helpers as H

pytestmark = pytest.mark.gpu


def pubs_arr(pubs):
    return bu.to_mont_array(pubs) if pubs else np.zeros((0, 4), np.uint64)


def instance(sc, seed):
    w, pubs = sc.witness(seed)
    return sc.wires_mont(w), pubs_arr(pubs), bu.to_mont_array(bu.blinders(seed + 500))


@contextlib.contextmanager
def transcript(cg, mode):
    old = cg.plonk_get_transcript()
    cg.plonk_set_transcript(mode)
    try:
        yield
    finally:
        cg.plonk_set_transcript(old)


def both_modes(cg, fn):
    """fn() under the host and under the device transcript -> (host result, device result)"""
    with transcript(cg, "host"):
        a = fn()
    with transcript(cg, "device"):
        b = fn()
    return a, b


def same_proofs(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert bytes(x) == bytes(y), f"proof {i}: the capgpu_proof structs differ between the modes"


def key_of(cg, tau, sc):
    h = cg.srs_generate(tau, sc.n + 3)
    pk, vk = cg.plonk_preprocess(h, sc.n, sc.num_inputs, sc.selectors_mont(), sc.sigma_mont())
    return h, pk, vk


def verifies(cg, tau, vk, pubs, proof, msg):
    g2h = cg.g2_generator()
    return cg.plonk_verify(vk, g2h, cg.g2_mul(g2h, tau), pubs, proof, msg)


# ---- 1. the sponge -------------------------------------------------------------------------------------------------------
def test_keccak_known_answers(cg):
    assert cg.keccak256_batch_dev([b""])[0].hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    rng = np.random.default_rng(7)
    msgs = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in list(range(274)) + [2000, 4096, 4097]]
    got = cg.keccak256_batch_dev(msgs)
    for m, d in zip(msgs, got):
        assert d == bn.keccak256(m), f"message of {len(m)} bytes"
    assert cg.keccak256_batch_dev([]) == []


def test_keccak_1024_messages_in_one_call(cg):
    rng = np.random.default_rng(8)
    msgs = [rng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes() for n in rng.integers(0, 700, size=1024)]
    got = cg.keccak256_batch_dev(msgs)
    assert len(got) == 1024
    for i in list(range(0, 1024, 37)) + [1023]:
        assert got[i] == bn.keccak256(msgs[i]), f"message {i}"
    assert len(set(got)) > 1000


# ---- 2. mode parity ------------------------------------------------------------------------------------------------------
def test_golden_proof_log5_in_device_mode(cg, tau):
    from oracle import plonk as pl
    g = H.load_golden("proof_log5.json")
    sc = bu.synthetic_circuit(g["log_n"], g["num_inputs"], seed=g["circuit_seed"])
    w, pubs = sc.witness(g["witness_seed"])
    bl = bu.to_mont_array(bu.blinders(g["blinder_seed"]))
    h, pk, vk = key_of(cg, tau, sc)
    msg = g["ext_msg"].encode()
    a, b = both_modes(cg, lambda: cg.plonk_prove_batch(pk, sc.wires_mont(w)[None], pubs_arr(pubs)[None], bl[None], msg, 1))
    same_proofs(a, b)
    assert cg.proof_serialize(a[0]) == cg.proof_serialize(b[0]) and len(cg.proof_serialize(b[0])) == 769
    pts, ev = H.proof_points(b[0])
    exp_pts = [H.unhex_pt(p) for p in g["wires_poly_comms"]] + [H.unhex_pt(g["prod_perm_poly_comm"])] + \
        [H.unhex_pt(p) for p in g["split_quot_poly_comms"]] + [H.unhex_pt(g["opening_proof"]),
                                                              H.unhex_pt(g["shifted_opening_proof"])]
    assert pts == exp_pts
    assert ev == [int(x, 16) for x in g["wires_evals"] + g["wire_sigma_evals"] + [g["perm_next_eval"]]]
    o = pl.Proof(pts[0:5], pts[5], pts[6:11], pts[11], pts[12], ev[0:5], ev[5:9], ev[9])
    vk_pts = [cr.affine_to_ints(np.ctypeslib.as_array(vk.selector_comms[i])) for i in range(13)] + \
             [cr.affine_to_ints(np.ctypeslib.as_array(vk.sigma_comms[i])) for i in range(5)]
    assert pl.verify(sc.n, sc.num_inputs, vk_pts[:13], vk_pts[13:], pubs, o, tau, ext_msg=msg)
    assert verifies(cg, tau, vk, pubs_arr(pubs), b[0], msg)
    cg.plonk_free_key(pk)
    cg.srs_free(h)


@pytest.fixture(scope="module")
def log10(cg, tau):
    sc = bu.synthetic_circuit(10, 5, seed=41)
    h, pk, vk = key_of(cg, tau, sc)
    insts = [instance(sc, 300 + i) for i in range(33)]
    yield sc, pk, vk, insts
    cg.plonk_free_key(pk)
    cg.srs_free(h)


@pytest.mark.parametrize("P", [1, 3, 16, 33])
def test_modes_agree_log10(cg, tau, log10, P):
    sc, pk, vk, insts = log10
    ws, ps, bs = (np.stack([i[k] for i in insts[:P]]) for k in range(3))
    msg = b"mode-parity-%d" % P
    a, b = both_modes(cg, lambda: cg.plonk_prove_batch(pk, ws, ps, bs, msg, P))
    same_proofs(a, b)
    for p in range(P):
        assert len(cg.proof_serialize(b[p])) == 769 and cg.proof_serialize(a[p]) == cg.proof_serialize(b[p])
        assert verifies(cg, tau, vk, ps[p], b[p], msg)
    # resident wires, and the coefficient input form of the same witnesses
    d = cg.DevBuf.from_numpy(ws)
    with transcript(cg, "device"):
        same_proofs(a, cg.plonk_prove_batch_dev(pk, d, ps, bs, msg, P))
        wc = np.stack([np.stack([cr.ntt_fr(c, 10, True, False).reshape(-1, 4) for c in w]) for w in ws])
        same_proofs(a, cg.plonk_prove_batch(pk, wc, ps, bs, msg, P, input_form="coeffs"))
        # no init message at all
        none_dev = cg.plonk_prove_batch_dev(pk, d, ps, bs, None, P)
    with transcript(cg, "host"):
        same_proofs(cg.plonk_prove_batch_dev(pk, d, ps, bs, None, P), none_dev)
    d.free()


def test_modes_agree_under_both_wire_commit_modes(cg, tau, log10):
    sc, pk, vk, insts = log10
    ws, ps, bs = (np.stack([i[k] for i in insts[:3]]) for k in range(3))
    try:
        for from_evals in (False, True):
            cg.plonk_set_wire_commit_from_evals(from_evals)
            a, b = both_modes(cg, lambda: cg.plonk_prove_batch(pk, ws, ps, bs, b"wc", 3))
            same_proofs(a, b)
            for p in range(3):
                assert verifies(cg, tau, vk, ps[p], b[p], b"wc")
    finally:
        cg.plonk_set_wire_commit_from_evals(None)


def mixed_batch(cg, tau, log_n, order, msg_of):
    n = 1 << log_n
    srs = cg.srs_generate(tau, n + 3)
    circuits = [bu.synthetic_circuit(log_n, ni, seed=seed) for ni, seed in ((3, 31), (9, 32), (0, 33))]
    keys = [cg.plonk_preprocess(srs, n, sc.num_inputs, sc.selectors_mont(), sc.sigma_mont()) for sc in circuits]
    cache = {}
    wires, rows, blinds, msgs = [], [], [], []
    for i, k in enumerate(order):
        if (k, i % 4) not in cache:
            cache[(k, i % 4)] = instance(circuits[k], 800 + 10 * k + i % 4)
        wm, pm, _ = cache[(k, i % 4)]
        row = np.zeros((9, 4), np.uint64)
        row[:len(pm)] = pm
        wires.append(wm); rows.append(row); blinds.append(bu.to_mont_array(bu.blinders(4000 + i))); msgs.append(msg_of(i))
    return srs, keys, [keys[k][0] for k in order], np.stack(wires), np.stack(rows), np.stack(blinds), msgs


def test_modes_agree_for_mixed_keys_and_input_counts(cg, tau):
    order = [0, 1, 2, 1, 0, 2, 2]
    srs, keys, handles, wires, rows, blinds, msgs = mixed_batch(cg, tau, 9, order, lambda i: b"note-%d" % i if i % 3 else b"")
    a, b = both_modes(cg, lambda: cg.plonk_prove_multi(handles, wires, rows, blinds, msgs))
    same_proofs(a, b)
    ni = [3, 9, 0]
    for i, k in enumerate(order):
        assert verifies(cg, tau, keys[k][1], rows[i][:ni[k]], b[i], msgs[i])
    for pk, _ in keys:
        cg.plonk_free_key(pk)
    cg.srs_free(srs)


@pytest.mark.parametrize("kind", sorted(bu.NOTE_SHAPES))
def test_modes_agree_on_note_shapes_full_size(cg, tau, kind):
    sc = bu.note_circuit(kind)
    h, pk, vk = key_of(cg, tau, sc)
    P = 8
    wm, pm, _ = instance(sc, 5)
    wm2, pm2, _ = instance(sc, 6)
    ws = np.stack([wm if p % 2 == 0 else wm2 for p in range(P)])
    ps = np.stack([pm if p % 2 == 0 else pm2 for p in range(P)])
    bs = np.stack([bu.to_mont_array(bu.blinders(900 + p)) for p in range(P)])
    a, b = both_modes(cg, lambda: cg.plonk_prove_batch(pk, ws, ps, bs, kind.encode(), P))
    same_proofs(a, b)
    for p in range(P):
        assert verifies(cg, tau, vk, ps[p], b[p], kind.encode())
    cg.plonk_free_key(pk)
    cg.srs_free(h)


def test_modes_agree_log15_batch_256(cg, tau):
    sc = bu.synthetic_circuit(15, 27, seed=75)
    h, pk, vk = key_of(cg, tau, sc)
    P = 256
    wm, pm, _ = instance(sc, 1)
    d = cg.DevBuf.from_numpy(np.ascontiguousarray(np.broadcast_to(wm, (P,) + wm.shape)))
    ps = np.ascontiguousarray(np.broadcast_to(pm, (P,) + pm.shape))
    bs = np.stack([bu.to_mont_array(bu.blinders(100 + p)) for p in range(P)])
    a, b = both_modes(cg, lambda: cg.plonk_prove_batch_dev(pk, d, ps, bs, b"big", P))
    same_proofs(a, b)
    assert len({bytes(x) for x in b}) == P
    ok = cg.plonk_verify_each([vk] * P, cg.g2_generator(), cg.g2_mul(cg.g2_generator(), tau), [pm] * P, list(b), [b"big"] * P)
    assert ok.all(), "every device-mode proof verifies"
    d.free()
    cg.plonk_free_key(pk)
    cg.srs_free(h)


# ---- 3. block boundaries -------------------------------------------------------------------------------------------------
def test_every_residue_of_the_transcript_length(cg, tau):
    """137 proofs of three keys in one batch, init messages of 0..136 bytes: with the prefixes' three lengths every
    residue mod 136 of the absorbed length is crossed at every challenge."""
    order = [i % 3 for i in range(137)]
    rng = np.random.default_rng(3)
    srs, keys, handles, wires, rows, blinds, msgs = mixed_batch(
        cg, tau, 5, order, lambda i: rng.integers(0, 256, size=i, dtype=np.uint8).tobytes())
    assert [len(m) for m in msgs] == list(range(137))
    d = cg.DevBuf.from_numpy(wires)
    a, b = both_modes(cg, lambda: cg.plonk_prove_multi(handles, d, rows, blinds, msgs))
    same_proofs(a, b)
    ni = [3, 9, 0]
    for i, k in enumerate(order):
        assert verifies(cg, tau, keys[k][1], rows[i][:ni[k]], b[i], msgs[i]), f"proof {i}"
    d.free()
    for pk, _ in keys:
        cg.plonk_free_key(pk)
    cg.srs_free(srs)


# ---- 4. refusal ----------------------------------------------------------------------------------------------------------
def test_unsatisfied_witness_is_refused_as_in_host_mode(cg, tau, log10):
    sc, pk, vk, insts = log10
    ws, ps, bs = (np.stack([i[k] for i in insts[:5]]) for k in range(3))
    good = ws.copy()
    ws[3, 4, sc.n // 2, 0] ^= 1
    d = cg.DevBuf.from_numpy(ws)
    cg.plonk_set_precheck(False)
    seen = []
    for mode in ("host", "device"):
        with transcript(cg, mode):
            with pytest.raises(cg.CapGpuError) as e:
                cg.plonk_prove_batch_dev(pk, d, ps, bs, b"r", 5)
            seen.append((e.value.code, str(e.value)))
    assert seen[0] == seen[1] and seen[0][0] == -7 and "proof 3" in seen[0][1]
    d.upload(good)
    a, b = both_modes(cg, lambda: cg.plonk_prove_batch_dev(pk, d, ps, bs, b"r", 5))
    same_proofs(a, b)
    d.free()


# ---- 5. synchronisation count --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [4, 64])
def test_one_stream_wait_per_call(cg, tau, log10, P):
    sc, pk, vk, insts = log10
    ws, ps, bs = (np.stack([insts[i % 33][k] for i in range(P)]) for k in range(3))
    d = cg.DevBuf.from_numpy(ws)
    cg.plonk_set_precheck(False)
    waits = {}
    for mode in ("host", "device"):
        with transcript(cg, mode):
            # the first call after a trim sizes the scratch buffers and the pinned result area - ahead of its first launch:
            # it, too, waits for its own kernels once
            cg.trim()
            c0, w0 = cg.plonk_sync_stats()
            cg.plonk_prove_batch_dev(pk, d, ps, bs, b"s", P)
            c1, w1 = cg.plonk_sync_stats()
            assert c1 - c0 == 1 and (w1 - w0 == 1 if mode == "device" else w1 - w0 >= 6), (mode, w1 - w0)
            per_call = []
            for _ in range(3):
                c0, w0 = cg.plonk_sync_stats()
                cg.plonk_prove_batch_dev(pk, d, ps, bs, b"s", P)
                c1, w1 = cg.plonk_sync_stats()
                assert c1 - c0 == 1
                per_call.append(w1 - w0)
            waits[mode] = per_call
    assert waits["device"] == [1, 1, 1], waits
    assert min(waits["host"]) >= 6, waits
    d.free()


# ---- 6. graphs -----------------------------------------------------------------------------------------------------------
def graphs_in_this_process(cg):
    return cg.runtime_info()[0] >= 70200000 or os.environ.get("CAPGPU_GRAPH_FORCE") == "1"


def test_graph_replay_in_a_process_on_the_build_runtime(cg):
    """test_one_segment_per_call_under_replay once more in a child process that loads the library BEFORE torch (the way
    tests/test_gpu_graphs.py arranges it): there the library runs on the HIP runtime it was built with and replays."""
    if graphs_in_this_process(cg):
        return
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CAPGPU_TEST_LIBRARY_FIRST="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "--timeout=300",
                        "-p", "no:cacheprovider", "-k", "one_segment_per_call_under_replay"], cwd=root, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-500:]
    assert " passed" in r.stdout and "skipped" not in r.stdout.splitlines()[-1], r.stdout[-300:]


def test_one_segment_per_call_under_replay(cg, tau):
    sc = bu.synthetic_circuit(9, 3, seed=31)
    h, pk, vk = key_of(cg, tau, sc)
    P = 4
    insts = [instance(sc, 20 + i) for i in range(P)]
    ws, ps, bs = (np.stack([i[k] for i in insts]) for k in range(3))
    d = cg.DevBuf.from_numpy(ws)
    old = os.environ.get("CAPGPU_GRAPH_MAX_BATCH")
    os.environ["CAPGPU_GRAPH_MAX_BATCH"] = "0"
    try:
        with transcript(cg, "host"):
            want = [bytes(p) for p in cg.plonk_prove_batch_dev(pk, d, ps, bs, b"g", P)]
    finally:
        if old is None:
            del os.environ["CAPGPU_GRAPH_MAX_BATCH"]
        else:
            os.environ["CAPGPU_GRAPH_MAX_BATCH"] = old
    replays = []
    with transcript(cg, "device"):
        for call in range(6):
            r0 = cg.plonk_graph_stats()[1]
            assert [bytes(p) for p in cg.plonk_prove_batch_dev(pk, d, ps, bs, b"g", P)] == want, f"call {call}"
            replays.append(cg.plonk_graph_stats()[1] - r0)
    if graphs_in_this_process(cg):
        assert replays[2:] == [1, 1, 1, 1], replays
    else:
        assert replays == [0] * 6, replays
    # The mode switched between calls.  The mode is part of a set's signature AND of the rule that picks the slot a new
    # signature replaces, so each mode keeps its own set: the host mode's is captured on its second call here and replayed
    # from the third (6-8 segments per call), the device mode's - captured above - is still there after the host calls
    # (one segment per call), and so is the host mode's after those.  No call replays the other mode's set: the proofs.
    seq = ["host"] * 3 + ["device"] * 3 + ["host"] * 2 + ["device", "host", "device"]
    per_call = []
    for call, mode in enumerate(seq):
        with transcript(cg, mode):
            r0 = cg.plonk_graph_stats()[1]
            assert [bytes(p) for p in cg.plonk_prove_batch_dev(pk, d, ps, bs, b"g", P)] == want, f"switching, call {call}"
            per_call.append(cg.plonk_graph_stats()[1] - r0)
    if graphs_in_this_process(cg):
        assert per_call[0] == 0 and per_call[1] == 0 and 6 <= per_call[2] <= 8, per_call
        assert per_call[3:6] == [1, 1, 1], per_call
        assert all(6 <= x <= 8 for x in per_call[6:8]), per_call
        assert per_call[8] == 1 and 6 <= per_call[9] <= 8 and per_call[10] == 1, per_call
    else:
        assert per_call == [0] * len(seq), per_call
    d.free()
    cg.plonk_free_key(pk)
    cg.srs_free(h)


# ---- 7. callers ----------------------------------------------------------------------------------------------------------
def test_coalesced_callers_and_trim(cg, tau, log10):
    sc, pk, vk, insts = log10
    T = 16

    def run():
        out, errs = [None] * T, []

        def one(i):
            try:
                wm, pm, bm = insts[i]
                out[i] = bytes(cg.plonk_prove(pk, wm, pm, bm, b"caller-%d" % i))
            except Exception as e:                      # noqa: BLE001
                errs.append(e)
        cg.plonk_set_coalescing(2000, 0)
        try:
            th = [threading.Thread(target=one, args=(i,)) for i in range(T)]
            for t in th:
                t.start()
            for t in th:
                t.join()
        finally:
            cg.plonk_set_coalescing(0, 0)
        assert not errs, errs
        cg.trim()
        return out, cg.scratch_info()[0]
    (a, left_host), (b, left_dev) = both_modes(cg, run)
    assert a == b
    assert left_dev == left_host, "capgpu_trim releases what the device transcript allocated"


def test_two_threads_on_two_contexts(cg, tau, log10):
    """Two threads, each bound to a context of its own, prove side by side: two device-mode calls, each enqueued whole,
    run at once on the two contexts' streams and workspaces.  Batches of two sizes, several rounds, so that the calls
    overlap in every phase; every proof equals host mode's."""
    assert cg.device_count() >= 2, \
        "this case needs two contexts: the suite's capgpu_init gives a device four unless CAPGPU_CONTEXTS_PER_DEVICE says less"
    sc, pk, vk, insts = log10
    sizes = (5, 24)
    jobs = []
    for t, P in enumerate(sizes):
        ws, ps, bs = (np.stack([insts[(7 * t + i) % 33][k] for i in range(P)]) for k in range(3))
        jobs.append((P, ws, ps, bs, b"thread-%d" % t))
    with transcript(cg, "host"):
        want = [[bytes(p) for p in cg.plonk_prove_batch(pk, ws, ps, bs, msg, P)] for P, ws, ps, bs, msg in jobs]
    rounds = 4
    got, errs = [[None] * rounds for _ in sizes], []
    start = threading.Barrier(len(sizes))

    def worker(t):
        try:
            cg.set_device(t)
            P, ws, ps, bs, msg = jobs[t]
            d = cg.DevBuf.from_numpy(ws)
            start.wait()
            for r in range(rounds):
                fn = cg.plonk_prove_batch_dev if r % 2 == 0 else cg.plonk_prove_batch
                got[t][r] = [bytes(p) for p in fn(pk, d if r % 2 == 0 else ws, ps, bs, msg, P)]
            d.free()
        except Exception as e:                          # noqa: BLE001
            errs.append(e)
            start.abort()
        finally:
            cg.set_device(-1)
    with transcript(cg, "device"):
        c0, w0 = cg.plonk_sync_stats()
        th = [threading.Thread(target=worker, args=(t,)) for t in range(len(sizes))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        c1, w1 = cg.plonk_sync_stats()
    assert not errs, errs
    for t in range(len(sizes)):
        for r in range(rounds):
            assert got[t][r] == want[t], f"thread {t}, round {r}"
    assert (c1 - c0, w1 - w0) == (len(sizes) * rounds, len(sizes) * rounds), "one wait per call on either context"


def test_modes_agree_for_a_key_that_recomputes_its_coset_columns(cg, tau):
    """CAPGPU_RECOMPUTE_PK_COSET is read when a key is made: such a key re-transforms its 18 fixed polynomials inside
    round 3 - in device mode inside the call's one segment - instead of reading cached columns."""
    sc = bu.synthetic_circuit(8, 3, seed=12)
    os.environ["CAPGPU_RECOMPUTE_PK_COSET"] = "1"
    try:
        h, pk, vk = key_of(cg, tau, sc)
    finally:
        del os.environ["CAPGPU_RECOMPUTE_PK_COSET"]
    h2, pk2, _ = key_of(cg, tau, sc)                     # the same circuit with cached columns
    P = 3
    insts = [instance(sc, 40 + i) for i in range(P)]
    ws, ps, bs = (np.stack([i[k] for i in insts]) for k in range(3))
    a, b = both_modes(cg, lambda: [cg.plonk_prove_batch(pk, ws, ps, bs, b"rc", P) for _ in range(3)])   # (direct, captured, replayed)
    for x, y in zip(a, b):
        same_proofs(x, y)
    with transcript(cg, "device"):
        same_proofs(b[0], cg.plonk_prove_batch(pk2, ws, ps, bs, b"rc", P))
    for p in range(P):
        assert verifies(cg, tau, vk, ps[p], b[2][p], b"rc")
    for k in (pk, pk2):
        cg.plonk_free_key(k)
    for x in (h, h2):
        cg.srs_free(x)
