"""Asynchronous prove tickets (capgpu_plonk_prove_batch_async / _multi_async / capgpu_wait), scratch reserved ahead
(capgpu_plonk_reserve) and the allocator's counters (capgpu_scratch_stats) on the device: a ticket's proofs are the bytes of
the synchronous call on the same inputs, two tickets of one thread run side by side, a bound submitter's ticket stays on
its context, a failure travels with its ticket, argument errors are refused at submission, a reserved context grows nothing
in the proving call, and capgpu_shutdown with a ticket outstanding ends cleanly.  The protocol itself (queue, limit,
waiters, drain) runs on the host under ThreadSanitizer: tests/test_tickets_host.py."""
import contextlib
import ctypes
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from cap_amd import bench_utils as bu
from oracle import capref as cr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pubs_arr(pubs):
    return bu.to_mont_array(pubs) if pubs else np.zeros((0, 4), np.uint64)


def instance(sc, seed):
    w, pubs = sc.witness(seed)
    return sc.wires_mont(w), pubs_arr(pubs), bu.to_mont_array(bu.blinders(seed + 500))


def key_of(cg, tau, sc):
    h = cg.srs_generate(tau, sc.n + 3)
    pk, vk = cg.plonk_preprocess(h, sc.n, sc.num_inputs, sc.selectors_mont(), sc.sigma_mont())
    return h, pk, vk


@contextlib.contextmanager
def transcript(cg, mode):
    old = cg.plonk_get_transcript()
    cg.plonk_set_transcript(mode)
    try:
        yield
    finally:
        cg.plonk_set_transcript(old)


@contextlib.contextmanager
def bound(cg, slot):
    cg.set_device(slot)
    try:
        yield
    finally:
        cg.set_device(-1)


def same_proofs(a, b):
    assert a is not None and len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert bytes(x) == bytes(y), f"proof {i}: the ticket's proof differs from the synchronous call's"


def stack(insts):
    return tuple(np.stack([i[k] for i in insts]) for k in range(3))


def to_coeffs(ws, log_n):
    return np.stack([np.stack([cr.ntt_fr(c, log_n, True, False).reshape(-1, 4) for c in w]) for w in ws])


@pytest.fixture(scope="module")
def log6(cg, tau):
    """n = 2^6, 3 public inputs: 8 witnesses; the synchronous proofs are computed per test (they depend on the mode only
    through the code path - the bytes do not)"""
    sc = bu.synthetic_circuit(6, 3, seed=21)
    h, pk, vk = key_of(cg, tau, sc)
    insts = [instance(sc, 700 + i) for i in range(8)]
    yield sc, pk, vk, insts
    cg.plonk_free_key(pk)
    cg.srs_free(h)


@pytest.fixture(scope="module")
def log10(cg, tau):
    """n = 2^10, 5 public inputs: 16 witnesses (two batches of 8 that share nothing)"""
    sc = bu.synthetic_circuit(10, 5, seed=41)
    h, pk, vk = key_of(cg, tau, sc)
    insts = [instance(sc, 300 + i) for i in range(16)]
    yield sc, pk, vk, insts
    cg.plonk_free_key(pk)
    cg.srs_free(h)


# ---- 2. two tickets from one thread (first in the file: max_running is a high-water mark since init) ------------------------
def test_two_tickets_from_one_thread_run_side_by_side(cg, log10):
    sc, pk, vk, insts = log10
    wa, pa, ba = stack(insts[:8])
    wb, pb, bb = stack(insts[8:])
    cg.plonk_set_precheck(False)
    sync_a = cg.plonk_prove_batch(pk, wa, pa, ba, b"A", 8)
    sync_b = cg.plonk_prove_batch(pk, wb, pb, bb, b"B", 8)
    s0 = cg.async_stats()
    ta = cg.plonk_prove_batch_async(pk, wa, pa, ba, b"A", 8)
    tb = cg.plonk_prove_batch_async(pk, wb, pb, bb, b"B", 8)
    assert ta.ticket != 0 and tb.ticket != 0 and ta.ticket != tb.ticket
    got_b = tb.wait()  # waited for in the reverse of the submission order
    got_a = ta.wait()
    same_proofs(got_a, sync_a)
    same_proofs(got_b, sync_b)
    s1 = cg.async_stats()
    print("async_stats", s0, "->", s1)
    assert s1["submitted"] - s0["submitted"] == 2 and s1["completed"] - s0["completed"] == 2
    assert s1["submitted"] == s1["completed"]
    # a condition, not a timing: submission takes microseconds, a batch of 8 at n = 2^10 milliseconds
    assert s1["max_running"] == 2


# ---- 1. same bytes as the synchronous call -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("form", ["evals", "coeffs"])
def test_ticket_proofs_are_the_synchronous_proofs(cg, tau, log6, form, mode):
    sc, pk, vk, insts = log6
    cg.plonk_set_precheck(False)
    for count in (1, 3, 8):
        ws, ps, bs = stack(insts[:count])
        if form == "coeffs":
            ws = to_coeffs(ws, 6)
        msg = b"async-%d" % count
        with transcript(cg, mode):
            sync = cg.plonk_prove_batch(pk, ws, ps, bs, msg, count, input_form=form)
            got = cg.plonk_prove_batch_async(pk, ws, ps, bs, msg, count, input_form=form).wait()
        same_proofs(got, sync)
    g2h = cg.g2_generator()
    assert cg.plonk_verify(vk, g2h, cg.g2_mul(g2h, tau), ps[2], got[2], msg)


@pytest.mark.parametrize("mode", ["host", "device"])
def test_multi_ticket_with_two_keys_of_one_domain(cg, tau, mode):
    n = 1 << 6
    srs = cg.srs_generate(tau, n + 3)
    circuits = [bu.synthetic_circuit(6, ni, seed=seed) for ni, seed in ((3, 31), (5, 32))]
    keys = [cg.plonk_preprocess(srs, n, sc.num_inputs, sc.selectors_mont(), sc.sigma_mont()) for sc in circuits]
    order = [0, 1, 1, 0, 1]
    wires, rows, blinds, msgs = [], [], [], []
    for i, k in enumerate(order):
        wm, pm, bm = instance(circuits[k], 900 + i)
        row = np.zeros((5, 4), np.uint64)
        row[:len(pm)] = pm
        wires.append(wm); rows.append(row); blinds.append(bm); msgs.append(b"m%d" % i if i % 2 else b"")
    wires, rows, blinds = np.stack(wires), np.stack(rows), np.stack(blinds)
    handles = [keys[k][0] for k in order]
    cg.plonk_set_precheck(False)
    try:
        with transcript(cg, mode):
            sync = cg.plonk_prove_multi(handles, wires, rows, blinds, msgs)
            got = cg.plonk_prove_multi_async(handles, wires, rows, blinds, msgs).wait()
            same_proofs(got, sync)
            same_proofs(cg.plonk_prove_multi_async(handles, wires, rows, blinds, None).wait(),
                        cg.plonk_prove_multi(handles, wires, rows, blinds, None))
        # keys of different domains: refused at submission with the synchronous call's code, no ticket
        sc7 = bu.synthetic_circuit(7, 3, seed=34)
        srs7 = cg.srs_generate(tau, sc7.n + 3)
        pk7, _ = cg.plonk_preprocess(srs7, sc7.n, 3, sc7.selectors_mont(), sc7.sigma_mont())
        s0 = cg.async_stats()
        with pytest.raises(cg.CapGpuError) as e:
            cg.plonk_prove_multi_async([keys[0][0], pk7], wires[:2], rows[:2, :3], blinds[:2], None)
        assert e.value.code == -1 and "share the domain size and the SRS" in str(e.value)
        assert cg.async_stats()["submitted"] == s0["submitted"]
        cg.plonk_free_key(pk7)
        cg.srs_free(srs7)
    finally:
        for pk, _ in keys:
            cg.plonk_free_key(pk)
        cg.srs_free(srs)


# ---- 3. a bound submitter's ticket runs on its context ----------------------------------------------------------------------
def test_bound_submitter_keeps_its_ticket_on_its_context(cg, log6, tmp_path):
    sc, pk, vk, insts = log6
    assert cg.device_count() >= 2
    ws, ps, bs = stack(insts[:3])
    cg.plonk_set_precheck(False)
    sync = cg.plonk_prove_batch(pk, ws, ps, bs, b"bound", 3)
    cg.trim()                                   # every context is empty ...
    cg.plonk_reserve(pk, 3, "evals", slot=1)    # ... and only slot 1 is sized for this batch
    cg.trace_enable(True)
    try:
        with bound(cg, 1):
            g0 = cg.scratch_stats()
            got = cg.plonk_prove_batch_async(pk, ws, ps, bs, b"bound", 3).wait()
            g1 = cg.scratch_stats()
    finally:
        cg.trace_enable(False)
    same_proofs(got, sync)
    # on any other context the batch would have had to grow its buffers
    assert g1["grow_events"] == g0["grow_events"], (g0, g1)
    path = str(tmp_path / "async_bound_trace.txt")
    assert cg.trace_dump(path) > 0
    runs = [ln.split() for ln in open(path) if " tk_run " in ln]
    assert len(runs) == 1 and runs[0][3] == "1" and runs[0][4] == "3", runs  # "t tid tk_run slot count"


# ---- 4. failure travels with the ticket -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,precheck", [("host", False), ("device", False), ("host", True)])
def test_unsatisfied_witness_fails_its_ticket_like_the_synchronous_call(cg, log6, mode, precheck):
    sc, pk, vk, insts = log6
    ws, ps, bs = stack(insts[:3])
    bad = ws.copy()
    bad[1, 4, sc.n // 2, 0] ^= 1
    cg.plonk_set_precheck(precheck)
    try:
        with transcript(cg, mode):
            with pytest.raises(cg.CapGpuError) as es:
                cg.plonk_prove_batch(pk, bad, ps, bs, b"f", 3)
            t = cg.plonk_prove_batch_async(pk, bad, ps, bs, b"f", 3)
            with pytest.raises(cg.CapGpuError) as ea:
                t.wait()
            print("sync :", es.value.code, es.value, "\nasync:", ea.value.code, ea.value)
            assert (ea.value.code, str(ea.value)) == (es.value.code, str(es.value))
            assert ea.value.code == -7 and "proof 1" in str(ea.value)
            # a valid ticket right after still succeeds
            same_proofs(cg.plonk_prove_batch_async(pk, ws, ps, bs, b"f", 3).wait(), cg.plonk_prove_batch(pk, ws, ps, bs, b"f", 3))
    finally:
        cg.plonk_set_precheck(False)


# ---- 5. argument errors at submission; double wait; poll --------------------------------------------------------------------
def test_argument_errors_are_refused_at_submission(cg, log6):
    sc, pk, vk, insts = log6
    ws, ps, bs = stack(insts[:3])
    L = cg.load()
    u64p = ctypes.POINTER(ctypes.c_uint64)
    proofs = (cg.Proof * 3)()
    ticket = ctypes.c_uint64(77)
    wp, pp, bp = (a.reshape(-1).ctypes.data_as(u64p) for a in (ws, ps, bs))

    def both(pk_handle, form, blinders):
        """(code, message) of the synchronous call and of the submission on the same arguments"""
        out = []
        for fn, tail in ((L.capgpu_plonk_prove_batch_ex, ()), (L.capgpu_plonk_prove_batch_async, (ctypes.byref(ticket),))):
            rc = fn(ctypes.c_uint64(pk_handle), 3, wp, pp, ctypes.c_size_t(3), None, ctypes.c_size_t(0), blinders,
                    ctypes.c_int(form), proofs, *tail)
            out.append((rc, L.capgpu_last_error().decode()))
        return out

    s0 = cg.async_stats()
    for args, code in (((0xDEAD0000, 0, bp), -4), ((pk, 7, bp), -1), ((pk, 0, None), -1)):
        ticket.value = 77
        sync, sub = both(*args)
        assert sync == sub and sub[0] == code, (sync, sub)
        assert ticket.value in (0, 77)  # no ticket was handed out
    assert cg.async_stats()["submitted"] == s0["submitted"]
    # an empty batch: ticket 0, which is done
    assert L.capgpu_plonk_prove_batch_async(ctypes.c_uint64(pk), 0, None, None, ctypes.c_size_t(3), None, ctypes.c_size_t(0),
                                            None, 0, None, ctypes.byref(ticket)) == 0 and ticket.value == 0
    done = ctypes.c_int(0)
    assert L.capgpu_wait(ctypes.c_uint64(0), ctypes.c_uint32(0), ctypes.byref(done)) == 0 and done.value == 1
    # a ticket is consumed by the wait that returns its result
    t = cg.plonk_prove_batch_async(pk, ws, ps, bs, b"w", 3)
    assert len(t.wait()) == 3
    with pytest.raises(cg.CapGpuError) as e:
        t.wait()
    assert e.value.code == -4
    assert L.capgpu_wait(ctypes.c_uint64(1 << 40), ctypes.c_uint32(0), ctypes.byref(done)) == -4 and done.value == 0


def test_poll_right_after_submission_never_raises(cg, log10):
    sc, pk, vk, insts = log10
    ws, ps, bs = stack(insts[:8])
    t = cg.plonk_prove_batch_async(pk, ws, ps, bs, b"poll", 8)
    first = t.wait(timeout_ms=0)
    assert first is None or len(first) == 8
    if first is None:
        later = t.wait(timeout_ms=1)  # a bounded wait: None again, or the proofs
        got = later if later is not None else t.wait()
        assert len(got) == 8


def test_two_threads_wait_for_one_ticket(cg, log10):
    sc, pk, vk, insts = log10
    ws, ps, bs = stack(insts[:8])
    t = cg.plonk_prove_batch_async(pk, ws, ps, bs, b"two", 8)
    L = cg.load()
    res = []

    def waiter():
        done = ctypes.c_int(0)
        res.append((L.capgpu_wait(ctypes.c_uint64(t.ticket), ctypes.c_uint32(0xFFFFFFFF), ctypes.byref(done)), done.value))

    th = [threading.Thread(target=waiter) for _ in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    t._consumed = True
    assert sorted(res) == [(-4, 0), (0, 1)], res


def test_free_key_with_a_ticket_outstanding(cg, tau):
    sc = bu.synthetic_circuit(10, 5, seed=43)
    h, pk, vk = key_of(cg, tau, sc)
    ws, ps, bs = stack([instance(sc, 40 + i) for i in range(8)])
    sync = cg.plonk_prove_batch(pk, ws, ps, bs, b"k", 8)
    t = cg.plonk_prove_batch_async(pk, ws, ps, bs, b"k", 8)
    cg.plonk_free_key(pk)  # the ticket holds its own reference
    same_proofs(t.wait(), sync)
    cg.srs_free(h)


# ---- 6. reserve -------------------------------------------------------------------------------------------------------------
# (log n, proofs, form, transcript, precheck, wire commitments from evaluations: None = the library default)
RESERVE_CASES = [
    pytest.param(10, 8, "evals", "host", False, None, id="evals-host"),
    pytest.param(10, 8, "coeffs", "host", False, None, id="coeffs-host"),
    pytest.param(10, 8, "evals", "device", False, None, id="evals-device"),
    # the witness check: stage_a, the whole batch copied up front, round 1 unchunked
    pytest.param(10, 8, "evals", "host", True, None, id="precheck-evals"),
    pytest.param(10, 8, "coeffs", "host", True, None, id="precheck-coeffs"),
    pytest.param(10, 8, "evals", "host", False, False, id="wire-commit-coeffs"),
    # <= CAPGPU_R1_OVERLAP_MAX (default 3): rounds 1-2 beside the side stream, segments replayed as graphs
    pytest.param(10, 2, "evals", "host", False, None, id="batch2-side-stream"),
    # round 1 in chunks: 32 proofs are the fewest that make two, 64 make four with the short first chunk
    pytest.param(6, 32, "evals", "host", False, None, id="batch32-two-chunks"),
    pytest.param(6, 64, "evals", "host", False, None, id="batch64-four-chunks"),
    pytest.param(10, 4, "vars", "host", False, None, id="vars-host"),
]


@pytest.mark.parametrize("log_n,P,form,mode,precheck,wire_evals", RESERVE_CASES)
def test_reserved_context_grows_nothing_in_the_proving_call(request, cg, tau, log_n, P, form, mode, precheck, wire_evals):
    sc, pk, vk, insts = request.getfixturevalue("log%d" % log_n)
    h = None
    if form == "vars":  # a key that knows its variable table; the values still on the host
        from tests.test_gpu_vars_prove import batch
        h = cg.srs_generate(tau, sc.n + 3)
        pk, _ = cg.plonk_preprocess_vars(h, sc.n, sc.num_inputs, sc.selectors_mont(), np.array(sc.wire_vars), sc.num_vars)
        _, ws, ps, bs = batch(sc, [300 + i for i in range(P)])
    else:
        ws, ps, bs = stack([insts[i % len(insts)] for i in range(P)])
    if form == "coeffs":
        ws = to_coeffs(ws, log_n)
    try:
        cg.plonk_set_precheck(precheck)
        cg.plonk_set_wire_commit_from_evals(wire_evals)
        with transcript(cg, mode), bound(cg, 0):
            cg.trim()
            c0 = cg.plonk_sync_stats()
            cg.plonk_reserve(pk, P, form, slot=0)
            assert cg.plonk_sync_stats()[0] == c0[0], "reserve proves nothing"
            g0 = cg.scratch_stats()
            with_reserve = cg.plonk_prove_batch(pk, ws, ps, bs, b"reserve", P, input_form=form)
            g1 = cg.scratch_stats()
            print(form, mode, P, "after reserve:", g0, "->", g1)
            assert g1["grow_events"] == g0["grow_events"] and g1["grow_bytes"] == g0["grow_bytes"], (g0, g1)
            # ... and a ticket of the bound thread finds the same context ready
            same_proofs(cg.plonk_prove_batch_async(pk, ws, ps, bs, b"reserve", P, input_form=form).wait(), with_reserve)
            assert cg.scratch_stats()["grow_events"] == g0["grow_events"]
            # control: the same proof on a trimmed context allocates
            cg.trim()
            g2 = cg.scratch_stats()
            same_proofs(cg.plonk_prove_batch(pk, ws, ps, bs, b"reserve", P, input_form=form), with_reserve)
            g3 = cg.scratch_stats()
            print(form, mode, P, "without    :", g2, "->", g3)
            assert g3["grow_events"] - g2["grow_events"] >= 1 and g3["grow_bytes"] - g2["grow_bytes"] > 0
            assert g3["grow_ms"] > g2["grow_ms"]
    finally:
        cg.plonk_set_precheck(False)
        cg.plonk_set_wire_commit_from_evals(None)
        if h is not None:
            cg.plonk_free_key(pk)
            cg.srs_free(h)


def test_reserve_respects_the_memory_limit(cg, log10):
    sc, pk, vk, insts = log10
    with bound(cg, 0):
        cg.trim()
        cg.set_memory_limit(1 << 20)  # the workspace of 8 proofs at n = 2^10 alone is several MiB
        try:
            with pytest.raises(cg.CapGpuError) as e:
                cg.plonk_reserve(pk, 8, "evals", slot=0)
            assert e.value.code == -5 and "bytes" in str(e.value) and "capgpu_set_memory_limit" in str(e.value)
        finally:
            cg.set_memory_limit(0)
        cg.plonk_reserve(pk, 8, "evals", slot=-1)  # every context, now that the cap is lifted
        with pytest.raises(cg.CapGpuError) as e:
            cg.plonk_reserve(pk, 8, "evals", slot=cg.device_count())
        assert e.value.code == -1
        with pytest.raises(cg.CapGpuError) as e:
            cg.plonk_reserve(0xDEAD0000, 8, "evals", slot=0)
        assert e.value.code == -4
    cg.trim()


# ---- 7. shutdown with a ticket outstanding --------------------------------------------------------------------------------
CHILD = r"""
import numpy as np
from cap_amd import bench_utils as bu, lib as cg
from oracle import bn254 as bn
cg.init(0)
tau = bn.SplitMix64(0xCA9).field(bn.R)
sc = bu.synthetic_circuit(10, 5, seed=41)
h = cg.srs_generate(tau, sc.n + 3)
pk, vk = cg.plonk_preprocess(h, sc.n, sc.num_inputs, sc.selectors_mont(), sc.sigma_mont())
w, pubs = sc.witness(300)
ws = np.ascontiguousarray(np.broadcast_to(sc.wires_mont(w), (8, 5, sc.n, 4)))
ps = np.ascontiguousarray(np.broadcast_to(bu.to_mont_array(pubs), (8, 5, 4)))
bs = np.stack([bu.to_mont_array(bu.blinders(p)) for p in range(8)])
tickets = [cg.plonk_prove_batch_async(pk, ws, ps, bs, b"bye", 8) for _ in range(4)]
cg.shutdown()
print("shutdown returned")
"""


def test_shutdown_with_tickets_outstanding_in_a_child_process():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "shutdown returned" in r.stdout, (r.returncode, r.stdout[-800:], r.stderr[-1500:])
