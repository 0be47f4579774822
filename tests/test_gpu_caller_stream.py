"""capgpu_set_stream: every family of entry points on a caller's HIP stream (a torch.cuda.Stream), bit-exact against the C
oracle and against the same call on the library's own stream.

A  parity of every family on a caller's stream S, then on the own stream, then on S again (tables built under the other)
B  the prover's caller-stream schedule: no graphs, no side stream - the same proof bytes through every entry point
C  capgpu_plonk_reserve (which plans with the side stream) covers the run on S (which has none)
D  stream ordering: the input is produced ON S behind a delay that is still running when the library is called, and the
   output is consumed on S; S.synchronize() is the only wait.  A launch or copy on any other stream reads the decoy the
   buffer held before, or leaves the pattern the output held
E  switching streams, two contexts at once, the timer

The delay of D is a chain of element-wise torch kernels on a 1 GiB tensor, sized per case from two measurements made in
this module: the device time of one such kernel (events on S) and the host time of steps 3-6 of the case (perf_counter,
in a pass without the delay).  The chain is at least ten times that host time and at least 20 ms; a case whose chain
would pass 200 ms fails instead.  Both measurements are printed by every run.  Measured on an MI355X: one delay kernel
takes 0.360 ms; host time of steps 3-6 and the delay chosen from it:
    ntt_fr_dev log_n = 10 / 12          0.025 / 0.027 ms  ->  56 kernels = 20.1 ms (the 20 ms floor)
    msm_g1_dev, msm_g1_var_dev          0.047 ms          ->  56 kernels = 20.1 ms
    plonk_prove_batch_dev (P = 2)       1.950 ms          ->  56 kernels = 20.1 ms (ten times: 19.5 ms)
    plonk_check_witness_batch_dev       0.102 ms          ->  56 kernels = 20.1 ms
"""
import copy
import ctypes
import math
import threading
import time

import numpy as np
import pytest
import torch

from cap_amd import bench_utils as bu
from oracle import bn254 as bn
from oracle import capref as cr
from oracle import plonk as pl
from tests import helpers as H
from tests.test_gpu_check_witness import got_tuple, numpy_verdict, position_index

pytestmark = pytest.mark.gpu


# ---- plumbing -------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def bound_and_own_stream_afterwards(cg):
    """the thread is bound to context 0 - an unbound thread's host-buffer calls are dealt to ANY context, and only context
    0's stream is switched here - and whatever a test did, the context is back on its own stream afterwards.  A device
    error met on the way out ends the session: nothing more is started on a GPU that has faulted"""
    cg.set_device(0)
    try:
        yield
    finally:
        try:
            cg.set_stream(None)
            cg.sync_all()
        except cg.CapGpuError as e:
            pytest.exit(f"device error after a caller-stream test: {e}", returncode=3)
        finally:
            cg.set_device(-1)


@pytest.fixture(scope="module")
def S(cg):
    return torch.cuda.Stream()


def thrice(cg, S, fn):
    """fn() with S set, with the own stream, with S again -> the three results"""
    out = []
    for s in (S, None, S):
        with cg.on_stream(s):
            out.append(fn())
    return out


def aff(jac):
    return cr.g1_to_affine(jac)


def pubs_arr(pubs):
    return bu.to_mont_array(pubs) if pubs else np.zeros((0, 4), np.uint64)


def as_i64(a: np.ndarray) -> torch.Tensor:
    """a uint64 array as a torch int64 tensor on the device (same bits)"""
    return torch.from_numpy(np.array(a, dtype=np.uint64).reshape(-1).view(np.int64)).cuda()


def as_u64(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def wrap(cg, t: torch.Tensor):
    return cg.DevBuf.from_ptr(t.data_ptr(), t.numel() * t.element_size())


def test_python_plumbing(cg, S):
    d = cg.DevBuf(64)
    v = cg.DevBuf.from_ptr(d.ptr.value, 64)
    assert v.ptr.value == d.ptr.value and v.nbytes == 64
    v.free()
    assert not v.ptr.value
    d.upload(np.arange(8, dtype=np.uint64))                      # ... and the owner's memory is still there
    assert list(d.to_numpy()) == list(range(8))
    del v
    assert list(d.to_numpy()) == list(range(8))
    d.free()
    cg.set_stream(S)                                             # an object with .cuda_stream
    cg.set_stream(int(S.cuda_stream))                            # an int
    cg.set_stream(None)
    cg.set_stream(None)                                          # twice is harmless
    cg.set_stream(0)
    with pytest.raises(RuntimeError, match="inside"):
        with cg.on_stream(S):
            raise RuntimeError("inside")
    # restored on the way out of the exception: a proof-sized piece of work runs and the own stream's sync sees it
    x = H.seeded_fr(3, 1 << 10)
    assert np.array_equal(cg.ntt_fr(x, 10).reshape(-1), cr.ntt_fr(x, 10, False, False).reshape(-1))


# ---- A. parity of every family ---------------------------------------------------------------------------------------------
NTT_FORMS = [(False, False), (True, False), (False, True), (True, True)]


@pytest.fixture(scope="module")
def ntt_cases():
    """log_n -> (three seeded arrays, {(inverse, coset): their oracle transforms}); 10 and 12: either side of ntt.hip's
    log_n <= 10 branch"""
    out = {}
    for log_n in (10, 12):
        arrs = [H.seeded_fr(7000 + 10 * log_n + i, 1 << log_n) for i in range(3)]
        want = {f: [cr.ntt_fr(a, log_n, *f).reshape(-1) for a in arrs] for f in NTT_FORMS}
        for a in arrs:
            a.setflags(write=False)
        out[log_n] = (arrs, want)
    return out


@pytest.mark.parametrize("log_n", [10, 12])
def test_ntt_parity(cg, S, ntt_cases, log_n):
    arrs, want = ntt_cases[log_n]
    n, stride = 1 << log_n, (1 << log_n) + 8
    host = np.zeros((3, stride, 4), dtype=np.uint64)
    for i in range(3):
        host[i, :n] = arrs[i]

    def run():
        got = {}
        for inv, coset in NTT_FORMS:
            one = cg.ntt_fr(arrs[0], log_n, inv, coset).reshape(-1)
            many = [o.reshape(-1) for o in cg.ntt_fr_batch(arrs, log_n, inverse=inv, coset=coset)]
            d = cg.DevBuf.from_numpy(host)
            cg.ntt_fr_dev(d, log_n, count=3, stride=stride, inverse=inv, coset=coset)
            back = d.to_numpy().reshape(3, stride, 4)
            d.free()
            got[(inv, coset)] = (one, many, back)
        return got

    for r, got in enumerate(thrice(cg, S, run)):
        for f in NTT_FORMS:
            one, many, back = got[f]
            assert np.array_equal(one, want[f][0]), (r, f)
            for i in range(3):
                assert np.array_equal(many[i], want[f][i]), (r, f, i)
                assert np.array_equal(back[i, :n].reshape(-1), want[f][i]), (r, f, i)
                assert not back[i, n:].any(), (r, f, i)


MSM_N, MSM_WIDE_N, MSM_WIDE_BATCH = 4099, 4096, 40


@pytest.fixture(scope="module")
def msm_env(cg):
    """an SRS of 4099 points (infinity and a duplicate among them), the scalars of one MSM over all of it and of 40 over
    its first 4096 points, and the oracle's results in affine form"""
    bases = cr.g1_fixed_base_batch(cr.random_field(911, 1, MSM_N, False))
    bases[5] = 0
    bases[7] = bases[6]
    h = cg.srs_upload(bases)
    one = cr.random_field(912, 1, MSM_N, False)
    one[0] = 0
    one[1] = cr.int_to_limbs(bn.R - 1)
    wide = np.stack([cr.random_field(920 + b, 1, MSM_WIDE_N, False) for b in range(MSM_WIDE_BATCH)])
    wide[1, :17] = 0
    want_one = aff(cr.msm_g1(bases, one))
    want_wide = [aff(cr.msm_g1(bases[:MSM_WIDE_N], wide[b])) for b in range(MSM_WIDE_BATCH)]
    for a in (bases, one, wide):
        a.setflags(write=False)
    yield {"h": h, "bases": bases, "one": one, "wide": wide, "want_one": want_one, "want_wide": want_wide}
    cg.srs_free(h)


def test_msm_parity(cg, S, msm_env):
    e = msm_env
    h = e["h"]
    assert cg.msm_plan(h, MSM_N, 1)["c"] == 13
    wide_plan = cg.msm_plan(h, MSM_WIDE_N, MSM_WIDE_BATCH)
    assert wide_plan["c"] == 15 and wide_plan["sort"] == "two-level", wide_plan

    def run():
        d_one = cg.DevBuf.from_numpy(e["one"])
        d_wide = cg.DevBuf.from_numpy(e["wide"])
        got = {
            "one": aff(cg.msm_g1(h, e["one"])),
            "one_dev": aff(cg.msm_g1_dev(h, d_one, MSM_N).to_numpy()),
            "wide": [aff(p) for p in cg.msm_g1_batch(h, list(e["wide"]))],
            "wide_dev": [aff(p) for p in cg.msm_g1_dev(h, d_wide, MSM_WIDE_N, count=MSM_WIDE_BATCH).to_numpy().reshape(-1, 12)],
        }
        d_one.free()
        d_wide.free()
        return got

    for r, got in enumerate(thrice(cg, S, run)):
        assert np.array_equal(got["one"], e["want_one"]), r
        assert np.array_equal(got["one_dev"], e["want_one"]), r
        for b in range(MSM_WIDE_BATCH):
            assert np.array_equal(got["wide"][b], e["want_wide"][b]), (r, b)
            assert np.array_equal(got["wide_dev"][b], e["want_wide"][b]), (r, b)


VAR_N = 1000


@pytest.fixture(scope="module")
def var_env(msm_env):
    bases = msm_env["bases"][:VAR_N]
    sc = cr.random_field(931, 1, VAR_N, False)
    sc[0] = 0
    sc[2] = cr.int_to_limbs(bn.R - 1)
    sc.setflags(write=False)
    return {"bases": bases, "sc": sc, "want": aff(cr.msm_g1(bases, sc))}


def test_var_msm_parity(cg, S, var_env):
    v = var_env

    def run():
        d_b, d_s = cg.DevBuf.from_numpy(v["bases"]), cg.DevBuf.from_numpy(v["sc"])
        got = aff(cg.msm_g1_var(v["bases"], v["sc"])), aff(cg.msm_g1_var_dev(d_b, d_s, VAR_N).to_numpy())
        d_b.free()
        d_s.free()
        return got

    for r, (host, dev) in enumerate(thrice(cg, S, run)):
        assert np.array_equal(host, v["want"]) and np.array_equal(dev, v["want"]), r


def test_lagrange_commit_parity(cg, S, tau):
    log_n, n = 9, 1 << 9
    h = cg.srs_generate(tau, n + 3)
    srs = cg.srs_download(h, 0, n + 3)
    col = H.seeded_fr(941, n)
    blind = [12345678901234567890, 98765432109876543210987654321]
    # what jf-plonk commits to: the blinded polynomial's n + 2 coefficients on the monomial key
    cf = H.fr_to_ints(cr.ntt_fr(col.copy(), log_n, True, False).reshape(n, 4)) + [0, 0]
    cf[0] = (cf[0] - blind[0]) % bn.R
    cf[1] = (cf[1] - blind[1]) % bn.R
    cf[n] = (cf[n] + blind[0]) % bn.R
    cf[n + 1] = (cf[n + 1] + blind[1]) % bn.R
    want = aff(cr.msm_g1(srs[:n + 2], bu.to_canonical_array(cf)))
    sc = np.concatenate([col, bu.to_mont_array(blind)])
    # (the first run builds the Lagrange-form key on S; the second and third use it from the other stream)
    for r, got in enumerate(thrice(cg, S, lambda: aff(cg.lagrange_commit(h, log_n, sc)))):
        assert np.array_equal(got, want), r
    cg.srs_free(h)


def test_keccak_parity(cg, S):
    msgs = [bytes((7 * j + ln) & 0xFF for j in range(ln)) for ln in (0, 1, 135, 136, 137, 300, 1000)]
    want = [cr.keccak256(m) for m in msgs]
    for r, got in enumerate(thrice(cg, S, lambda: cg.keccak256_batch_dev(msgs))):
        assert got == want, r


# ---- the circuit of B, C, D and of A's witness check and verifiers -----------------------------------------------------------
LOG_N, NIN = 9, 4
SEED_A, SEED_B = 100, 200                # witness seeds: A is what is proved, B the decoy of D


class Prover:
    def __init__(self, cg, tau):
        self.cg, self.tau = cg, tau
        self.sc = bu.synthetic_circuit(LOG_N, NIN)
        self.sc2 = bu.synthetic_circuit(LOG_N, NIN, seed=3)          # a second key of the same domain (prove_multi)
        sc = self.sc
        self.srs = cg.srs_generate(tau, sc.n + 3)
        self.pk, self.vk = cg.plonk_preprocess(self.srs, sc.n, NIN, sc.selectors_mont(), sc.sigma_mont())
        self.pk2, self.vk2 = cg.plonk_preprocess(self.srs, sc.n, NIN, self.sc2.selectors_mont(), self.sc2.sigma_mont())
        self.srs_host = cg.srs_download(self.srs, 0, sc.n + 3)
        # five distinct instances per key, cycled through the larger batches
        self.w, self.p = sc.witnesses_mont([SEED_A + i for i in range(5)], threads=4)
        self.w2, self.p2 = self.sc2.witnesses_mont([SEED_A + 50 + i for i in range(5)], threads=4)
        self.wB, self.pB = sc.witnesses_mont([SEED_B + i for i in range(5)], threads=4)
        self.bl = np.stack([bu.to_mont_array(bu.blinders(300 + i)) for i in range(33)])
        self.msg = b"caller-stream"
        self._want = {}

    def batch(self, P, multi=False):
        """(keys, wires, pubs, blinders) of a batch of P; multi: proofs 1, 3, 5, ... under the second key"""
        ks, ws, ps = [], [], []
        for i in range(P):
            second = multi and i % 2 == 1
            ks.append(self.pk2 if second else self.pk)
            ws.append((self.w2 if second else self.w)[i % 5])
            ps.append((self.p2 if second else self.p)[i % 5])
        return ks, np.stack(ws), np.stack(ps), self.bl[:P]

    def want(self, P, multi=False):
        """the proofs of batch(P, multi) made on the library's own stream in the default modes, proofs 0 and (multi) 1
        pinned to the oracle's; computed once per shape.  The first call for a shape must come with the own stream in force:
        the tests ask before they set S."""
        key = (P, multi)
        if key not in self._want:
            cg = self.cg
            ks, ws, ps, bs = self.batch(P, multi)
            if multi:
                got = cg.plonk_prove_multi(ks, ws, ps, bs, [self.msg] * P)
            else:
                got = cg.plonk_prove_batch(self.pk, ws, ps, bs, self.msg, P)
            ck = cr.PlonkKey(self.srs_host, self.sc.n, NIN, self.sc.selectors_mont(), self.sc.sigma_mont())
            rc, comms, evals = ck.prove(ws[0], ps[0], bs[0], self.msg)
            assert rc == 0 and H.proof_points(got[0]) == H.cref_proof_points(comms, evals)
            if multi and P > 1:
                ck2 = cr.PlonkKey(self.srs_host, self.sc.n, NIN, self.sc2.selectors_mont(), self.sc2.sigma_mont())
                rc, comms, evals = ck2.prove(ws[1], ps[1], bs[1], self.msg)
                assert rc == 0 and H.proof_points(got[1]) == H.cref_proof_points(comms, evals)
            self._want[key] = [bytes(p) for p in got]
        return self._want[key]

    def free(self):
        self.cg.plonk_free_key(self.pk)
        self.cg.plonk_free_key(self.pk2)
        self.cg.srs_free(self.srs)


@pytest.fixture(scope="module")
def pv(cg, tau):
    p = Prover(cg, tau)
    yield p
    p.free()


class Modes:
    """transcript mode and wire-commit mode for a scope (both process-wide)"""

    def __init__(self, cg, transcript, wire_evals):
        self.cg, self.transcript, self.wire_evals = cg, transcript, wire_evals

    def __enter__(self):
        self.old = self.cg.plonk_get_transcript()
        self.cg.plonk_set_transcript(self.transcript)
        self.cg.plonk_set_wire_commit_from_evals(self.wire_evals)

    def __exit__(self, *exc):
        self.cg.plonk_set_transcript(self.old)
        self.cg.plonk_set_wire_commit_from_evals(None)


def unsatisfied(w):
    bad = w.copy()
    bad[4, 20, 0] ^= np.uint64(1)
    return bad


def test_witness_check_parity(cg, S, pv):
    sc = pv.sc
    W = np.stack([pv.w[0], unsatisfied(pv.w[1]), pv.w[2]])
    Pb = pv.p[:3]
    idx = position_index(sc)
    sel = [np.array(col, dtype=object) for col in sc.selectors]
    want = [numpy_verdict(sc, idx, sel, [bu.from_mont_array(W[k, i]) for i in range(5)], bu.from_mont_array(Pb[k]))
            for k in range(3)]
    assert [v[0] != 0 for v in want] == [False, True, False]

    def run():
        d = cg.DevBuf.from_numpy(W)
        got = [got_tuple(f) for f in cg.plonk_check_witness_batch(pv.pk, d, Pb, 3)]
        d.free()
        return got

    for r, got in enumerate(thrice(cg, S, run)):
        assert got == want, r


@pytest.fixture(scope="module")
def block(cg, tau, pv):
    """three proofs under pv's key, the middle one spoilt, and what the oracle's verifier and the host verifier say"""
    proofs = [cg.Proof.from_buffer_copy(b) for b in pv.want(3)]
    proofs[1] = copy.deepcopy(proofs[1])
    proofs[1].perm_next_eval[0] ^= 1
    pubs = [pv.p[i] for i in range(3)]
    h2 = cg.g2_generator()
    bh = cg.g2_mul(h2, tau)
    vk_pts = [cr.affine_to_ints(np.ctypeslib.as_array(pv.vk.selector_comms[i])) for i in range(13)] + \
             [cr.affine_to_ints(np.ctypeslib.as_array(pv.vk.sigma_comms[i])) for i in range(5)]
    want = []
    for i in range(3):
        pts, ev = H.proof_points(proofs[i])
        o = pl.Proof(pts[0:5], pts[5], pts[6:11], pts[11], pts[12], ev[0:5], ev[5:9], ev[9])
        want.append(bool(pl.verify(pv.sc.n, NIN, vk_pts[:13], vk_pts[13:], bu.from_mont_array(pubs[i]), o, tau, ext_msg=pv.msg)))
    assert want == [True, False, True]
    assert [cg.plonk_verify(pv.vk, h2, bh, pubs[i], proofs[i], pv.msg) for i in range(3)] == want
    vkh = cg.plonk_vk_upload(pv.vk)
    yield {"proofs": proofs, "pubs": pubs, "h2": h2, "bh": bh, "vkh": vkh, "want": want}
    cg.plonk_vk_release(vkh)


def test_verifier_parity(cg, S, pv, block):
    b = block
    rows = np.stack(b["pubs"])
    arr = (cg.Proof * 3)()
    for i, p in enumerate(b["proofs"]):
        ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(p), ctypes.sizeof(cg.Proof))
    msgs = [pv.msg] * 3

    def run():
        each_dev = [cg.plonk_verify_dev(pv.vk, b["h2"], b["bh"], b["pubs"][i], b["proofs"][i], pv.msg) for i in range(3)]
        host_in = cg.plonk_verify_block([b["vkh"]] * 3, b["h2"], b["bh"], rows, b["proofs"], msgs, each=True, num_inputs=NIN)
        d_pr = cg.DevBuf(ctypes.sizeof(arr))
        cg.check(cg.load().capgpu_memcpy_h2d(d_pr.ptr, ctypes.byref(arr), ctypes.c_size_t(ctypes.sizeof(arr))))
        d_pub = cg.DevBuf.from_numpy(rows)
        resident = cg.plonk_verify_block([b["vkh"]] * 3, b["h2"], b["bh"], d_pub, d_pr, msgs, each=True, num_inputs=NIN)
        good = cg.plonk_verify_block([b["vkh"]] * 2, b["h2"], b["bh"], rows[[0, 2]], [b["proofs"][0], b["proofs"][2]], msgs[:2],
                                     each=True, num_inputs=NIN)
        d_pr.free()
        d_pub.free()
        return each_dev, host_in, resident, good

    for r, (each_dev, host_in, resident, good) in enumerate(thrice(cg, S, run)):
        assert each_dev == b["want"], r
        for ok, each in (host_in, resident):
            assert ok is False and list(each) == b["want"], r
        assert good[0] is True and list(good[1]) == [True, True], r


# ---- B. the prover's caller-stream schedule --------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 3, 5, 33])
@pytest.mark.parametrize("transcript,wire_evals", [("host", False), ("host", True), ("device", False), ("device", True)])
def test_prover_entry_points_make_the_same_proofs(cg, S, pv, P, transcript, wire_evals):
    want, want_multi = pv.want(P), pv.want(P, multi=True)
    ks, ws, ps, bs = pv.batch(P)
    mk, mw, mp, mb = pv.batch(P, multi=True)
    d = cg.DevBuf.from_numpy(ws)
    with Modes(cg, transcript, wire_evals):
        for s in (S, None):
            with cg.on_stream(s):
                where = "S" if s is not None else "own"
                assert [bytes(cg.plonk_prove(pv.pk, ws[i], ps[i], bs[i], pv.msg)) for i in range(P)] == want, where
                assert [bytes(p) for p in cg.plonk_prove_batch(pv.pk, ws, ps, bs, pv.msg, P)] == want, where
                assert [bytes(p) for p in cg.plonk_prove_batch_dev(pv.pk, d, ps, bs, pv.msg, P)] == want, where
                assert [bytes(p) for p in cg.plonk_prove_multi(mk, mw, mp, mb, [pv.msg] * P)] == want_multi, where
    d.free()


def test_nothing_is_captured_on_a_callers_stream(cg, S, pv):
    """make_plan turns graphs (and the side stream) off under a caller's stream: three calls of one shape - on the own
    stream the second captures and the third replays where the runtime allows graphs - count nothing"""
    want = pv.want(1)
    _, ws, ps, bs = pv.batch(1)
    d = cg.DevBuf.from_numpy(ws)
    with cg.on_stream(S):
        g0 = cg.plonk_graph_stats()
        for _ in range(3):
            assert [bytes(p) for p in cg.plonk_prove_batch_dev(pv.pk, d, ps, bs, pv.msg, 1)] == want
            assert [bytes(p) for p in cg.plonk_prove_batch(pv.pk, ws, ps, bs, pv.msg, 1)] == want
        assert cg.plonk_graph_stats() == g0
    d.free()


def test_unsatisfied_witness_is_refused_alike_and_leaves_nothing_behind(cg, S, pv):
    want = pv.want(3)
    _, ws, ps, bs = pv.batch(3)
    bad = ws.copy()
    bad[1] = unsatisfied(ws[1])
    d_bad, d_good = cg.DevBuf.from_numpy(bad), cg.DevBuf.from_numpy(ws)
    seen = []
    for s in (None, S, None):
        with cg.on_stream(s):
            for call in (lambda: cg.plonk_prove_batch(pv.pk, bad, ps, bs, pv.msg, 3),
                         lambda: cg.plonk_prove_batch_dev(pv.pk, d_bad, ps, bs, pv.msg, 3)):
                with pytest.raises(cg.CapGpuError) as e:
                    call()
                seen.append((e.value.code, str(e.value)))
    assert seen[0][0] == -7 and "proof 1" in seen[0][1], seen[0]
    assert all(x == seen[0] for x in seen), seen
    # the context still proves, on either stream
    for s in (S, None):
        with cg.on_stream(s):
            assert [bytes(p) for p in cg.plonk_prove_batch_dev(pv.pk, d_good, ps, bs, pv.msg, 3)] == want
            assert [bytes(p) for p in cg.plonk_prove_batch(pv.pk, ws, ps, bs, pv.msg, 3)] == want
    d_bad.free()
    d_good.free()


def test_tickets_under_a_callers_stream(cg, S, pv):
    """include/capgpu.h: a ticket of a bound thread runs on its context and on the stream that context has when the worker
    starts it; the proofs are the synchronous call's"""
    want5, want2 = pv.want(5), pv.want(2)
    _, ws, ps, bs = pv.batch(5)
    with cg.on_stream(S):
        first = cg.plonk_prove_batch_async(pv.pk, ws, ps, bs, pv.msg, 5)
        second = cg.plonk_prove_batch_async(pv.pk, ws[:2], ps[:2], bs[:2], pv.msg, 2)
        assert [bytes(p) for p in first.wait()] == want5
        assert [bytes(p) for p in second.wait()] == want2
    # the thread unbound: the ticket goes to a free context, which may be context 0 on S or another on its own stream
    cg.set_device(-1)
    with cg.on_stream(S):
        assert [bytes(p) for p in cg.plonk_prove_batch_async(pv.pk, ws, ps, bs, pv.msg, 5).wait()] == want5


def test_device_transcript_waits_once_per_call_on_a_callers_stream(cg, S, pv):
    P = 4
    want = pv.want(P)
    _, ws, ps, bs = pv.batch(P)
    d = cg.DevBuf.from_numpy(ws)
    waits = {}
    with Modes(cg, "device", None):
        for name, s in (("own", None), ("S", S)):
            with cg.on_stream(s):
                cg.plonk_prove_batch_dev(pv.pk, d, ps, bs, pv.msg, P)             # sizes what has to be sized
                c0, w0 = cg.plonk_sync_stats()
                assert [bytes(p) for p in cg.plonk_prove_batch_dev(pv.pk, d, ps, bs, pv.msg, P)] == want
                c1, w1 = cg.plonk_sync_stats()
                waits[name] = (c1 - c0, w1 - w0)
    d.free()
    assert waits["own"] == waits["S"] == (1, 1), waits


# ---- C. reserve covers the caller-stream run -----------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [2, 16])
def test_reserve_covers_the_run_on_a_callers_stream(cg, S, pv, P):
    """capgpu_plonk_reserve plans with sizing = true (a side stream); the run on S plans without one"""
    want = pv.want(P)
    _, ws, ps, bs = pv.batch(P)
    cg.trim()
    cg.plonk_reserve(pv.pk, P, "evals", slot=0)
    g0 = cg.scratch_stats()
    with cg.on_stream(S):
        got = [bytes(p) for p in cg.plonk_prove_batch(pv.pk, ws, ps, bs, pv.msg, P)]
    g1 = cg.scratch_stats()
    print("reserve", P, g0, "->", g1)
    assert got == want
    assert g1["grow_events"] == g0["grow_events"] and g1["grow_bytes"] == g0["grow_bytes"], (g0, g1)


# ---- D. stream ordering ------------------------------------------------------------------------------------------------------
DELAY_ELEMS = 1 << 28                    # float32: 1 GiB, read and written by every kernel of the chain
DELAY_MIN_MS, DELAY_MAX_MS = 20.0, 200.0


class Delay:
    def __init__(self, S):
        self.S = S
        self.t = torch.zeros(DELAY_ELEMS, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        self.enqueue(4)
        S.synchronize()
        ops = 40
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(S):
            e0.record()
        self.enqueue(ops)
        with torch.cuda.stream(S):
            e1.record()
        S.synchronize()
        self.op_ms = e0.elapsed_time(e1) / ops
        print(f"delay calibration: one element-wise kernel over {DELAY_ELEMS * 4 >> 20} MiB takes {self.op_ms:.3f} ms")
        assert self.op_ms > 0.05, "the delay kernel is too short to build a chain from"

    def enqueue(self, ops):
        with torch.cuda.stream(self.S):
            for _ in range(ops):
                self.t.add_(1.0)

    def ops_for(self, host_ms):
        """the chain for a case whose steps 3-6 take host_ms on the host"""
        want_ms = max(DELAY_MIN_MS, 10.0 * host_ms)
        ops = math.ceil(want_ms / self.op_ms)
        assert ops * self.op_ms <= DELAY_MAX_MS, \
            f"a delay of ten times the host time ({host_ms:.2f} ms) would be {ops * self.op_ms:.0f} ms (> {DELAY_MAX_MS:.0f})"
        return ops


@pytest.fixture(scope="module")
def delay(S):
    return Delay(S)


def ordered(cg, S, delay, name, buf, decoy, real, call, out=None, pattern=None, after_call=None):
    """Steps 1-8 of the ordering check.  buf: the tensor the library reads (and, out is None, writes); decoy / real:
    device tensors of its content; call(): the library call under test, made with S set; out: the tensor the library
    writes, pre-filled with `pattern`.  -> (call's return value, the output as consumed on S)"""
    result = buf if out is None else out

    def steps_3_to_6(ev):
        with torch.cuda.stream(S):
            buf.copy_(real, non_blocking=True)                                   # 3
            ev.record()                                                          # 4
        pending = not ev.query()                                                 # 5
        return pending, call()                                                   # 6

    def reset():
        with torch.cuda.stream(S):
            buf.copy_(decoy)                                                     # 1
            if out is not None:
                out.copy_(pattern)
        S.synchronize()

    with cg.on_stream(S):
        # a pass without the delay: sizes the library's scratch (a growth drains the stream) and times steps 3-6
        reset()
        steps_3_to_6(torch.cuda.Event())
        S.synchronize()
        reset()
        t0 = time.perf_counter()
        steps_3_to_6(torch.cuda.Event())
        host_ms = (time.perf_counter() - t0) * 1e3
        S.synchronize()
        ops = delay.ops_for(host_ms)
        print(f"ordering {name}: host time of steps 3-6 {host_ms:.3f} ms -> delay of {ops} kernels = {ops * delay.op_ms:.1f} ms")
        reset()
        ev = torch.cuda.Event()
        delay.enqueue(ops)                                                       # 2
        pending, ret = steps_3_to_6(ev)
        assert pending, "delay too short: the producer had finished before the library was called"
        if after_call is not None:
            after_call(ev)
        with torch.cuda.stream(S):
            consumed = torch.empty_like(result)
            consumed.copy_(result, non_blocking=True)                            # 7
        S.synchronize()                                                          # 8: the only wait
    return ret, as_u64(consumed)


@pytest.mark.parametrize("log_n", [10, 12])
def test_ordering_ntt_dev(cg, S, delay, ntt_cases, log_n):
    arrs, want = ntt_cases[log_n]
    real, decoy = as_i64(arrs[0]), as_i64(arrs[1])
    buf = torch.empty_like(real)
    torch.cuda.synchronize()
    d = wrap(cg, buf)
    _, got = ordered(cg, S, delay, f"ntt_fr_dev log_n={log_n}", buf, decoy, real,
                     lambda: cg.ntt_fr_dev(d, log_n, coset=True))
    assert np.array_equal(got, want[(False, True)][0])


def jac_pattern(count):
    """`count` copies of a valid point no MSM here results in: 7 G in Jacobian form with Z = 1"""
    g = cr.points_to_array([bn.g1_mul(bn.G1_GEN, 7)]).reshape(8)
    one = cr.vec_to_mont(0, cr.ints_to_array([1])).reshape(4)
    return np.tile(np.concatenate([g, one]), count)


def test_ordering_msm_dev(cg, S, delay, msm_env):
    e = msm_env
    real, decoy = as_i64(e["one"]), as_i64(np.zeros_like(e["one"]))
    buf, out, pattern = torch.empty_like(real), torch.zeros(12, dtype=torch.int64, device="cuda"), as_i64(jac_pattern(1))
    torch.cuda.synchronize()
    d_sc, d_out = wrap(cg, buf), wrap(cg, out)
    _, got = ordered(cg, S, delay, "msm_g1_dev", buf, decoy, real, lambda: cg.msm_g1_dev(e["h"], d_sc, MSM_N, d_out=d_out),
                     out=out, pattern=pattern)
    assert np.array_equal(aff(got), e["want_one"])


def test_ordering_var_msm_dev_and_it_does_not_wait(cg, S, delay, var_env):
    v = var_env
    real, decoy = as_i64(v["sc"]), as_i64(np.zeros_like(v["sc"]))
    bases = as_i64(v["bases"])
    buf, out, pattern = torch.empty_like(real), torch.zeros(12, dtype=torch.int64, device="cuda"), as_i64(jac_pattern(1))
    torch.cuda.synchronize()
    d_b, d_sc, d_out = wrap(cg, bases), wrap(cg, buf), wrap(cg, out)

    def still_pending(ev):
        assert not ev.query(), "capgpu_msm_g1_var_dev waited for the stream: its input's producer is done on its return"

    _, got = ordered(cg, S, delay, "msm_g1_var_dev", buf, decoy, real,
                     lambda: cg.msm_g1_var_dev(d_b, d_sc, VAR_N, d_out=d_out), out=out, pattern=pattern,
                     after_call=still_pending)
    assert np.array_equal(aff(got), v["want"])


def test_ordering_prove_batch_dev(cg, S, delay, pv):
    P = 2
    want = pv.want(P)
    _, ws, ps, bs = pv.batch(P)
    real, decoy = as_i64(ws), as_i64(pv.wB[:P])
    buf = torch.empty_like(real)
    torch.cuda.synchronize()
    d = wrap(cg, buf)
    # (the decoy: satisfying witnesses of the same circuit from other seeds - a run that read them makes other proofs, or is
    # refused over A's public inputs)
    proofs, _ = ordered(cg, S, delay, "plonk_prove_batch_dev", buf, decoy, real,
                        lambda: cg.plonk_prove_batch_dev(pv.pk, d, ps, bs, pv.msg, P))
    assert [bytes(p) for p in proofs] == want


def test_ordering_check_witness_dev(cg, S, delay, pv):
    W = np.stack([pv.w[0], unsatisfied(pv.w[1]), pv.w[2]])
    all_good = pv.w[:3]
    Pb = pv.p[:3]
    real, decoy = as_i64(W), as_i64(all_good)
    buf = torch.empty_like(real)
    torch.cuda.synchronize()
    d = wrap(cg, buf)
    with cg.on_stream(None):
        d_own = cg.DevBuf.from_numpy(W)
        want = [got_tuple(f) for f in cg.plonk_check_witness_batch(pv.pk, d_own, Pb, 3)]
        d_own.free()
    assert [v[0] != 0 for v in want] == [False, True, False]
    faults, _ = ordered(cg, S, delay, "plonk_check_witness_batch_dev", buf, decoy, real,
                        lambda: cg.plonk_check_witness_batch(pv.pk, d, Pb, 3))
    assert [got_tuple(f) for f in faults] == want


# ---- E. switching and scope -----------------------------------------------------------------------------------------------------
def test_switching_streams_between_calls(cg, S, ntt_cases, msm_env):
    """S1 -> S2 -> own with nothing of the test's in between: capgpu_set_stream drains the stream it leaves, so work
    enqueued on the next one may read what the last one wrote"""
    arrs, want = ntt_cases[12]
    e = msm_env
    S2 = torch.cuda.Stream()
    d = cg.DevBuf.from_numpy(arrs[0])
    d_sc = cg.DevBuf.from_numpy(e["one"])
    cg.set_stream(S)
    cg.ntt_fr_dev(d, 12, coset=True)                           # not waited for
    out1 = cg.msm_g1_dev(e["h"], d_sc, MSM_N)
    cg.set_stream(S2)
    fwd = d.to_numpy()                                          # on S2: what S wrote
    cg.ntt_fr_dev(d, 12, inverse=True, coset=True)
    out2 = cg.msm_g1_dev(e["h"], d_sc, MSM_N)
    cg.set_stream(None)
    cg.set_stream(None)
    back = d.to_numpy()
    own = cg.ntt_fr(arrs[1], 12)
    assert np.array_equal(fwd, want[(False, True)][0])
    assert np.array_equal(back.reshape(-1, 4), arrs[0])
    assert np.array_equal(own.reshape(-1), want[(False, False)][1])
    assert np.array_equal(aff(out1.to_numpy()), e["want_one"]) and np.array_equal(aff(out2.to_numpy()), e["want_one"])
    for b in (d, d_sc, out1, out2):
        b.free()


def test_two_contexts_one_on_a_callers_stream(cg, S, pv, ntt_cases, msm_env):
    """thread A binds context 0 and sets S, thread B binds context 1 and sets nothing: capgpu_set_stream is per context"""
    n_ctx = ctypes.c_int(0)
    cg.check(cg.load().capgpu_context_count(ctypes.byref(n_ctx)))
    assert n_ctx.value >= 2, "this case needs two contexts: capgpu_init gives a device four by default"
    arrs, want_ntt = ntt_cases[12]
    e = msm_env
    _, ws, ps, bs = pv.batch(2)
    want = pv.want(2)

    def work():
        return (cg.ntt_fr(arrs[0], 12, False, True).reshape(-1), aff(cg.msm_g1(e["h"], e["one"])),
                [bytes(p) for p in cg.plonk_prove_batch(pv.pk, ws, ps, bs, pv.msg, 2)])

    def on_b(fn):
        res = []
        t = threading.Thread(target=lambda: (cg.set_device(1), res.append(fn()), cg.set_device(-1)))
        t.start()
        t.join()
        return res[0]

    # what one P = 2 proof on B's context counts once its shape has been seen three times (where the runtime allows graphs:
    # replays; elsewhere nothing) - with A on S beside it, it must count the same
    def graph_delta():
        g0 = cg.plonk_graph_stats()
        cg.plonk_prove_batch(pv.pk, ws, ps, bs, pv.msg, 2)
        g1 = cg.plonk_graph_stats()
        return (g1[0] - g0[0], g1[1] - g0[1])
    for _ in range(3):
        on_b(graph_delta)
    alone = on_b(graph_delta)

    got, errs = [None, None], []
    start = threading.Barrier(2)
    g0 = cg.plonk_graph_stats()

    def worker(t):
        try:
            cg.set_device(t)
            if t == 0:
                cg.set_stream(S)
            start.wait()
            got[t] = work()
        except Exception as ex:                          # noqa: BLE001
            errs.append(ex)
            start.abort()
        finally:
            if t == 0:
                cg.set_stream(None)
            cg.set_device(-1)
    th = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    g1 = cg.plonk_graph_stats()
    assert not errs, errs
    for t in range(2):
        assert np.array_equal(got[t][0], want_ntt[(False, True)][0]), t
        assert np.array_equal(got[t][1], e["want_one"]), t
        assert got[t][2] == want, t
    assert (g1[0] - g0[0], g1[1] - g0[1]) == alone, "A's stream changed what B's context captures or replays"


def test_timer_on_a_callers_stream_and_across_a_switch(cg, S, ntt_cases):
    arrs, want = ntt_cases[12]
    d = cg.DevBuf.from_numpy(arrs[0])
    with cg.on_stream(S):
        cg.timer_begin()
        cg.ntt_fr_dev(d, 12, coset=True)
        ms = cg.timer_end()
        assert ms > 0
        assert np.array_equal(d.to_numpy(), want[(False, True)][0])
    # include/capgpu.h: capgpu_set_stream with a measurement open is allowed; the measurement then runs from _begin's
    # place in the stream that was left (drained by the switch) to _end's place in the stream in force at _end
    S2 = torch.cuda.Stream()
    cg.set_stream(S)
    cg.timer_begin()
    cg.ntt_fr_dev(d, 12, inverse=True, coset=True)
    cg.set_stream(S2)
    cg.ntt_fr_dev(d, 12, coset=True)
    ms2 = cg.timer_end()
    cg.set_stream(None)
    assert ms2 > 0
    assert np.array_equal(d.to_numpy(), want[(False, True)][0])
    with pytest.raises(cg.CapGpuError) as e:
        cg.timer_end()                                # closed by the _end above
    assert e.value.code == -1
    d.free()
