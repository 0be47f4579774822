"""Round 3 on five of the six n-cosets of the quotient domain (CAPGPU_QUOT_COSETS=5, the default):
the transforms of block 2 shrink to n points, k_quotient runs over 5n points, the quotient's top 8 coefficients come from
k_quotient_top and the inverse solves a fixed 5 x 5 system per coefficient index.  The quotient is the same polynomial,
so every proof is, word for word, the proof of CAPGPU_QUOT_COSETS=6 - the parent's path - and the C oracle's; an
unsatisfied witness is refused with the same code (the row test stands in for the degree test's bit 1).  The identities:
tests/test_quot5_identity.py.

No entry point hands out the quotient's coefficients, so k_quotient_top's output is pinned through what is made of it:
coefficients 5n .. 5n + 7 are scalars of the fifth split-quotient commitment (it covers 4n + 8 .. 5n + 9), which is
compared on its own below, and m_j h_i enters coefficients j n + i of all five."""
import os
import subprocess
import sys
from contextlib import contextmanager

import numpy as np
import pytest

from cap_amd import bench_utils as bu
from oracle import capref as cr
from tests import helpers as H

pytestmark = pytest.mark.gpu
P = 3


def pubs_arr(pubs):
    return bu.to_mont_array(pubs) if pubs else np.zeros((0, 4), np.uint64)


@contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@contextmanager
def transcript(cg, mode):
    old = cg.plonk_get_transcript()
    cg.plonk_set_transcript(mode)
    try:
        yield
    finally:
        cg.plonk_set_transcript(old)


class Case:
    def __init__(self, cg, tau, log_n, nin, seed):
        self.sc = sc = bu.synthetic_circuit(log_n, nin, seed=seed)
        self.h = cg.srs_generate(tau, sc.n + 3)
        self.pk, self.vk = cg.plonk_preprocess(self.h, sc.n, nin, sc.selectors_mont(), sc.sigma_mont())
        self.key = cr.PlonkKey(cg.srs_download(self.h, 0, sc.n + 3), sc.n, nin, sc.selectors_mont(), sc.sigma_mont())
        ws, ps, bls = [], [], []
        for p in range(P):
            w, pubs = sc.witness(300 + p)                      # distinct witnesses
            assert all(pubs)
            ws.append(sc.wires_mont(w)); ps.append(pubs_arr(pubs)); bls.append(bu.to_mont_array(bu.blinders(400 + p)))
        self.ws, self.ps, self.bls = np.stack(ws), np.stack(ps), np.stack(bls)

    def oracle(self, msg):
        out = []
        for p in range(P):
            rc, comms, evals = self.key.prove(self.ws[p], self.ps[p], self.bls[p], msg)
            assert rc == 0
            out.append(H.cref_proof_points(comms, evals))
        return out

    def free(self, cg):
        cg.plonk_free_key(self.pk)
        cg.srs_free(self.h)


# n = 2^4: the smallest domain that takes the five-coset form, every transform one pass (8 of its 16 rows are public
# inputs: 27 do not fit); n = 2^10: blocks 0 and 1 run two passes, block 2 one; n = 2^11: everything runs two passes and
# the folded coefficients land in row 0 of a column tile
@pytest.mark.parametrize("log_n,nin", [(4, 8), (10, 27), (11, 27)])
def test_five_cosets_give_the_proofs_of_six(cg, tau, log_n, nin):
    c = Case(cg, tau, log_n, nin, seed=30 + log_n)
    msg = b"quot5"
    want = c.oracle(msg)
    g2h = cg.g2_generator()
    bh = cg.g2_mul(g2h, tau)
    for tr in ("host", "device"):
        for fold in (0, 1, 2):
            got = {}
            for cosets in (5, 6):
                with transcript(cg, tr), env(CAPGPU_QUOT_COSETS=cosets, CAPGPU_QUOT_FOLD=fold):
                    got[cosets] = cg.plonk_prove_batch(c.pk, c.ws, c.ps, c.bls, msg, P)
            for p in range(P):
                where = f"{tr} transcript, fold {fold}, proof {p}"
                a5, a6 = cg.proof_to_arrays(got[5][p]), cg.proof_to_arrays(got[6][p])
                assert np.array_equal(a5["split_quot_poly_comms"][4], a6["split_quot_poly_comms"][4]), where  # holds h
                assert bytes(got[5][p]) == bytes(got[6][p]), where
                assert H.proof_points(got[5][p]) == want[p], where
            assert cg.plonk_verify(c.vk, g2h, bh, c.ps[1], got[5][1], msg), f"{tr} transcript, fold {fold}"
    c.free(cg)


@pytest.mark.parametrize("log_n", [10, 11])
def test_mixed_keys(cg, tau, log_n):
    """Two keys on one domain in one batch: each proof reads its own key's columns, coefficients (k_quotient_top) and
    selector values (the row test); every proof equals its single-key call's under six cosets."""
    n = 1 << log_n
    srs = cg.srs_generate(tau, n + 3)
    circuits = [bu.synthetic_circuit(log_n, ni, seed=seed) for ni, seed in ((27, 61), (3, 62))]
    keys = [cg.plonk_preprocess(srs, n, sc.num_inputs, sc.selectors_mont(), sc.sigma_mont())[0] for sc in circuits]
    order = [1, 0, 1]
    wires, rows, blinds, msgs, alone = [], [], [], [], []
    for i, k in enumerate(order):
        sc = circuits[k]
        w, pubs = sc.witness(700 + i)
        bl = bu.to_mont_array(bu.blinders(800 + i))
        row = np.full((27, 4), 0xFFFF, np.uint64)
        row[:len(pubs)] = bu.to_mont_array(pubs)
        wires.append(sc.wires_mont(w)); rows.append(row); blinds.append(bl); msgs.append(b"note-%d" % i)
        with env(CAPGPU_QUOT_COSETS=6):
            alone.append(cg.plonk_prove_batch(keys[k], sc.wires_mont(w)[None], pubs_arr(pubs)[None], bl[None], msgs[i], 1)[0])
    for tr in ("host", "device"):
        for cosets in (5, 6):
            with transcript(cg, tr), env(CAPGPU_QUOT_COSETS=cosets):
                got = cg.plonk_prove_multi([keys[k] for k in order], np.stack(wires), np.stack(rows), np.stack(blinds), msgs)
            for i in range(len(order)):
                assert bytes(got[i]) == bytes(alone[i]), (tr, cosets, i)
    for pkh in keys:
        cg.plonk_free_key(pkh)
    cg.srs_free(srs)


def test_no_key_below_sixteen_rows(cg, tau):
    """Below n = 16 the quotient's top coefficients would reach into gamma and beta k_j X, and the prover would have to take
    six cosets (ProvePlan::five asks for log n >= 4).  No such key exists: preprocess refuses n = 8 as it always did."""
    sc = bu.synthetic_circuit(3, 2, seed=33)
    h = cg.srs_generate(tau, sc.n + 3)
    with env(CAPGPU_QUOT_COSETS=5), pytest.raises(cg.CapGpuError) as e:
        cg.plonk_preprocess(h, sc.n, 2, sc.selectors_mont(), sc.sigma_mont())
    assert e.value.code == -1 and ">= 16" in str(e.value)
    cg.srs_free(h)


def test_zero_z_blinders_are_refused_alike(cg, tau):
    """With z's three blinders zero the quotient's top coefficients vanish (h_7 = 0: the degree test's bit 2).  Both forms
    refuse the proof of that witness, with the same flags, and prove the others alike."""
    c = Case(cg, tau, 6, 5, seed=34)
    bls = c.bls.copy()
    bls[1, 10:13] = 0
    seen = {}
    for tr in ("host", "device"):
        for cosets in (5, 6):
            with transcript(cg, tr), env(CAPGPU_QUOT_COSETS=cosets):
                proofs, outcomes = cg.plonk_prove_each([c.pk] * P, c.ws, c.ps, bls, [b"zb"] * P)
            seen[tr, cosets] = [(bytes(p), o.status, o.degree_flags) for p, o in zip(proofs, outcomes)]
            assert [o.status for o in outcomes] == [0, -7, 0] and outcomes[1].degree_flags == 2, (tr, cosets)
    assert len({tuple(v) for v in seen.values()}) == 1
    c.free(cg)


def test_unsatisfied_witnesses_are_refused_alike(cg, tau):
    """Five cosets carry no redundancy: a numerator that Z_H does not divide shows on the rows (k_check_gates and the grand
    product's closing, k_rows_verdict), not above degree 5n + 7.  A wrong public input and a changed cell are
    each refused under both forms and both transcripts; the good proof of the batch is the same proof."""
    c = Case(cg, tau, 6, 5, seed=35)
    n = c.sc.n
    for what in ("public input", "gate"):
        ws, ps = c.ws.copy(), c.ps.copy()
        if what == "public input":
            ps[1, 0, 0] ^= 1
        else:
            ws[1, 0, n // 2, 0] ^= 1                       # one cell: its gate and its copies break
        seen = {}
        for tr in ("host", "device"):
            for cosets in (5, 6):
                with transcript(cg, tr), env(CAPGPU_QUOT_COSETS=cosets):
                    proofs, outcomes = cg.plonk_prove_each([c.pk] * P, ws, ps, c.bls, [b"bad"] * P)
                assert [o.status for o in outcomes] == [0, -7, 0] and outcomes[1].degree_flags & 1, (what, tr, cosets)
                seen[tr, cosets] = [bytes(p) for p in proofs]
                with transcript(cg, tr), env(CAPGPU_QUOT_COSETS=cosets), pytest.raises(cg.CapGpuError) as e:
                    cg.plonk_prove_batch(c.pk, ws, ps, c.bls, b"bad", P)
                assert e.value.code == -7
        assert len({tuple(v) for v in seen.values()}) == 1, what
    c.free(cg)


def test_a_closed_grand_product_is_required(cg, tau):
    """Every gate holds and the copy constraints do not: a satisfied witness proved under a key of the same selectors whose
    sigma has the columns of wires 0 and 1 exchanged - still a permutation, not the witness's.  The gates hold row by row;
    z does not close (prod num != prod den), which k_rows_verdict reads off the ends of the two scans."""
    sc_a = bu.synthetic_circuit(6, 0, seed=36)
    w, _pubs = sc_a.witness(5)
    h = cg.srs_generate(tau, sc_a.n + 3)
    sigma = np.array(sc_a.sigma_mont(), copy=True)
    sigma[[0, 1]] = sigma[[1, 0]]                          # a permutation the witness does not respect
    pk, _vk = cg.plonk_preprocess(h, sc_a.n, 0, sc_a.selectors_mont(), sigma)
    wm, bm = sc_a.wires_mont(w)[None], bu.to_mont_array(bu.blinders(6))[None]
    for tr in ("host", "device"):
        for cosets in (5, 6):
            with transcript(cg, tr), env(CAPGPU_QUOT_COSETS=cosets), pytest.raises(cg.CapGpuError) as e:
                cg.plonk_prove_batch(pk, wm, np.zeros((1, 0, 4), np.uint64), bm, None, 1)
            assert e.value.code == -7, (tr, cosets)
    cg.plonk_free_key(pk)
    cg.srs_free(h)


def graphs_in_this_process(cg):
    return cg.runtime_info()[0] >= 70200000 or os.environ.get("CAPGPU_GRAPH_FORCE") == "1"


def test_graph_replay(cg, tau):
    """Captured segments keep the launches of their capture: the coset count is part of a graph set's signature.  The same
    device buffer proved six times under each form, replayed from the third call on, gives the same proofs.  Where this
    process runs on a HIP runtime older than the library's build (tests/conftest.py: torch first) replay is off and the test
    runs once more in a child process that loads the library first."""
    if not graphs_in_this_process(cg):
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-k",
                            "test_graph_replay", "-p", "no:cacheprovider"], cwd=root,
                           env=dict(os.environ, CAPGPU_TEST_LIBRARY_FIRST="1"), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-500:]
        assert " passed" in r.stdout and "skipped" not in r.stdout.splitlines()[-1], r.stdout[-300:]
        return
    c = Case(cg, tau, 10, 27, seed=37)
    d = cg.DevBuf.from_numpy(c.ws[:1])
    got = {}
    for cosets in (5, 6):
        cap0, rep0 = cg.plonk_graph_stats()
        with env(CAPGPU_QUOT_COSETS=cosets):
            for rnd in range(6):
                d.upload(c.ws[rnd % P])
                got[cosets, rnd] = bytes(cg.plonk_prove_batch_dev(c.pk, d, c.ps[rnd % P][None], c.bls[rnd % P][None], b"g", 1)[0])
        cap1, rep1 = cg.plonk_graph_stats()
        assert cap1 > cap0 and rep1 > rep0, (cosets, cap0, cap1, rep0, rep1)    # a set of its own per form
    want = c.oracle(b"g")
    for rnd in range(6):
        assert got[5, rnd] == got[6, rnd], rnd
    proofs = cg.plonk_prove_batch(c.pk, c.ws, c.ps, c.bls, b"g", P)
    for p in range(P):
        assert H.proof_points(proofs[p]) == want[p] and bytes(proofs[p]) == got[5, p]
    c.free(cg)
