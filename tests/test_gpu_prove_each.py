"""Per-proof outcomes (capgpu_plonk_prove_each / _dev / _async, capgpu_prove_outcome_text): a batch is proved PAST its
unsatisfied witnesses.  Every witness of tests/test_gpu_check_witness.py's case mix - 18 mutated cells, satisfied witnesses
between bad ones, one wrong public input - goes through one call: a proof fails exactly where the oracle refuses the
witness, a surviving proof is word for word the lone capgpu_plonk_prove's, a failed record is all-ones words, the text is
the lone call's message; by host buffers, device buffers and tickets, bound and dealt, in both transcript homes, with and
without the witness check, from values, coefficients and variables, under graph replay, on a caller's stream, after a
reserve - and the coalescer, which takes its verdicts from the outcomes, proves a gathered batch once."""
import contextlib
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from cap_amd import bench_utils as bu
from oracle.bn254 import R
from tests.test_gpu_check_witness import build_cases, check_case_mix, got_tuple, numpy_verdict, position_index
from tests.test_gpu_input_forms import to_coeffs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(4, 1), (6, 0), (9, 27)]
ERR_PROOF = -7
ONES = b"\xff" * (13 * 64 + 10 * 32)


@contextlib.contextmanager
def modes(cg, transcript, precheck, wire_evals=None):
    old = cg.plonk_get_transcript()
    cg.plonk_set_transcript(transcript)
    cg.plonk_set_precheck(precheck)
    cg.plonk_set_wire_commit_from_evals(wire_evals)
    try:
        yield
    finally:
        cg.plonk_set_wire_commit_from_evals(None)
        cg.plonk_set_precheck(False)
        cg.plonk_set_transcript(old)


@contextlib.contextmanager
def bound(cg, slot):
    cg.set_device(slot)
    try:
        yield
    finally:
        cg.set_device(-1)


class Cases:
    """one circuit's key, the 22 cases, their blinders and messages, and - computed once - the lone proof of every
    satisfied witness"""

    def __init__(self, cg, tau, log_n, nin, srs=None, **kw):
        self.cg, self.log_n, self.nin = cg, log_n, nin
        self.sc = bu.synthetic_circuit(log_n, nin, seed=log_n + nin)
        self.own_srs = srs is None
        self.h = srs if srs is not None else cg.srs_generate(tau, self.sc.n + 3)
        self.pk, self.vk = cg.plonk_preprocess(self.h, self.sc.n, nin, self.sc.selectors_mont(), self.sc.sigma_mont())
        self.W, self.Pb, self.exp, self.lab = build_cases(self.sc, 900 + log_n, **kw)
        check_case_mix(self.exp, self.lab)
        self.P = len(self.exp)
        self.bl = np.stack([bu.to_mont_array(bu.blinders(3000 + p)) for p in range(self.P)])
        self.msgs = [b"note-%d" % p if p % 4 else None for p in range(self.P)]
        self.good = [p for p in range(self.P) if self.exp[p][0] == 0]
        self.bad = [p for p in range(self.P) if self.exp[p][0] != 0]
        self.lone = {p: bytes(cg.plonk_prove(self.pk, self.W[p], self.Pb[p], self.bl[p], self.msgs[p])) for p in self.good}
        self._wc = None

    @property
    def Wc(self):
        if self._wc is None:
            self._wc = to_coeffs(self.W, self.log_n)
        return self._wc

    def lone_error(self, p):
        with pytest.raises(self.cg.CapGpuError) as e:
            self.cg.plonk_prove(self.pk, self.W[p], self.Pb[p], self.bl[p], self.msgs[p])
        assert e.value.code == ERR_PROOF
        return str(e.value)

    def free(self):
        self.cg.plonk_free_key(self.pk)
        if self.own_srs:
            self.cg.srs_free(self.h)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "log%d-nin%d" % s)
def shape(request, cg, tau):
    c = Cases(cg, tau, *request.param)
    yield c
    c.free()


@pytest.fixture(scope="module")
def log9(cg, tau):
    c = Cases(cg, tau, 9, 27)
    yield c
    c.free()


def check_outcomes(c, proofs, outcomes, precheck, idx=None):
    """the assertions of test 1 for the proofs `idx` (default: all) of the cases c"""
    idx = list(range(c.P)) if idx is None else idx
    assert len(proofs) == len(outcomes) == len(idx)
    for k, p in enumerate(idx):
        o, e = outcomes[k], c.exp[p]
        print(p, c.lab[p], "status", o.status, "flags", o.degree_flags, "fault", got_tuple(o.fault), "expected", e)
        assert (o.status != 0) == (e[0] != 0), f"proof {p} ({c.lab[p]})"
        assert o.status in (0, ERR_PROOF)
        if e[0] == 0:
            assert o.degree_flags == 0 and o.fault.kind == 0
            assert bytes(proofs[k]) == c.lone[p], f"proof {p}: not the lone call's proof"
            continue
        assert bytes(proofs[k]) == ONES, f"proof {p}: a failed record is all-ones words"
        assert o.degree_flags != 0, f"proof {p}: the degree test must agree with the check"
        if precheck:
            assert got_tuple(o.fault) == e, f"proof {p} ({c.lab[p]})"
        else:
            assert got_tuple(o.fault) == (0,) * 7


def signature(proofs, outcomes):
    return [(bytes(p), o.status, o.degree_flags, got_tuple(o.fault)) for p, o in zip(proofs, outcomes)]


# ---- 1. outcomes and survivors ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["evals", "coeffs"])
@pytest.mark.parametrize("precheck", [False, True], ids=["nocheck", "precheck"])
@pytest.mark.parametrize("transcript", ["host", "device"])
def test_outcomes_and_survivors(cg, tau, shape, transcript, precheck, form):
    c = shape
    wires = c.W if form == "evals" else c.Wc
    with modes(cg, transcript, precheck):
        # (the only way the all-or-nothing entry points prove this batch raises for all 22)
        with pytest.raises(cg.CapGpuError) as e:
            cg.plonk_prove_multi([c.pk] * c.P, wires, c.Pb, c.bl, c.msgs, input_form=form)
        assert e.value.code == ERR_PROOF
        proofs, outcomes = cg.plonk_prove_each([c.pk] * c.P, wires, c.Pb, c.bl, c.msgs, input_form=form)
    check_outcomes(c, proofs, outcomes, precheck)
    if transcript == "host" and not precheck and form == "evals":   # one per shape through the verifier as well
        g2h = cg.g2_generator()
        bh = cg.g2_mul(g2h, tau)
        p = c.good[0]
        assert cg.plonk_verify(c.vk, g2h, bh, c.Pb[p], proofs[p], c.msgs[p])
        assert not cg.plonk_verify(c.vk, g2h, bh, c.Pb[c.bad[0]], proofs[c.bad[0]], c.msgs[c.bad[0]])


# ---- 2. the text is the lone call's message -----------------------------------------------------------------------------------
@pytest.mark.parametrize("precheck", [False, True], ids=["nocheck", "precheck"])
@pytest.mark.parametrize("transcript", ["host", "device"])
def test_text_is_the_lone_calls_message(cg, log9, transcript, precheck):
    c = log9
    gate = next(p for p in c.bad if c.exp[p][0] == 1 and c.lab[p] != "public input")
    copy = next(p for p in c.bad if c.exp[p][0] == 2 and c.lab[p] == "targeted")
    pub = next(p for p in c.bad if c.lab[p] == "public input")
    pick = [gate, c.good[0], copy, pub]
    with modes(cg, transcript, precheck):
        proofs, outcomes = cg.plonk_prove_each([c.pk] * 4, c.W[pick], c.Pb[pick], c.bl[pick], [c.msgs[p] for p in pick])
        for k, p in enumerate(pick):
            text = cg.prove_outcome_text(outcomes[k])
            print(p, c.lab[p], repr(text))
            if p in c.good:
                assert text == "" and outcomes[k].status == 0
                continue
            # str() of the CapGpuError the lone call raises: the code's name, then the library's message
            assert str(cg.CapGpuError(ERR_PROOF, text)) == c.lone_error(p)
            assert ("witnesses do not satisfy their circuit; first: proof 0: " in text) == precheck
            assert ("proof 0: quotient polynomial has the wrong degree (flags %d)" % outcomes[k].degree_flags in text) == (not precheck)


# ---- 3. the same results by every road ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precheck", [False, True], ids=["nocheck", "precheck"])
@pytest.mark.parametrize("transcript", ["host", "device"])
def test_same_results_by_every_road(cg, log9, transcript, precheck):
    c = log9
    handles = [c.pk] * c.P
    half = c.P // 2
    assert half >= 8 and cg.device_count() >= 2             # an unbound host call of this size is dealt over two contexts

    def roads():
        out = {"host": cg.plonk_prove_each(handles, c.W, c.Pb, c.bl, c.msgs)}
        d = cg.DevBuf.from_numpy(c.W)
        out["dev"] = cg.plonk_prove_each_dev(handles, d, c.Pb, c.bl, c.msgs)
        assert np.array_equal(d.to_numpy(), c.W.reshape(-1))  # the caller's buffer is never written
        d.free()
        t1 = cg.plonk_prove_each_async(handles[:half], c.W[:half], c.Pb[:half], c.bl[:half], c.msgs[:half])
        t2 = cg.plonk_prove_each_async(handles[half:], c.W[half:], c.Pb[half:], c.bl[half:], c.msgs[half:])
        (p1, o1), (p2, o2) = t1.wait(), t2.wait()          # capgpu_wait: CAPGPU_OK for a ticket that ran
        out["async"] = (p1 + p2, o1 + o2)
        return out

    with modes(cg, transcript, precheck):
        unbound = roads()
        with bound(cg, 0):
            one_part = roads()
        with modes(cg, transcript, precheck, wire_evals=False):   # the wire commitments from coefficients
            coeff_commit = cg.plonk_prove_each(handles, c.W, c.Pb, c.bl, c.msgs)
    check_outcomes(c, *unbound["host"], precheck)
    want = signature(*unbound["host"])
    for name, got in list(unbound.items()) + list(one_part.items()) + [("wire-commit-coeffs", coeff_commit)]:
        assert signature(*got) == want, name


# ---- 4. several keys of one domain --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precheck", [False, True], ids=["nocheck", "precheck"])
@pytest.mark.parametrize("transcript", ["host", "device"])
def test_two_keys_of_one_domain(cg, tau, transcript, precheck):
    h = cg.srs_generate(tau, 64 + 3)
    a, b = Cases(cg, tau, 6, 0, srs=h, n_random=4, n_targeted=2), Cases(cg, tau, 6, 3, srs=h, n_random=4, n_targeted=2)
    try:
        cnt = min(a.P, b.P)
        assert any(e[0] for e in a.exp[:cnt]) and any(e[0] for e in b.exp[:cnt])      # bad witnesses under both keys
        handles, W, rows, bl, msgs = [], [], [], [], []
        for p in range(cnt):
            for c in (a, b):
                row = np.zeros((3, 4), np.uint64)            # rows of the larger input count, as _multi uses them
                row[:c.nin] = c.Pb[p]
                handles.append(c.pk); W.append(c.W[p]); rows.append(row); bl.append(c.bl[p]); msgs.append(c.msgs[p])
        with modes(cg, transcript, precheck):
            proofs, outcomes = cg.plonk_prove_each(handles, np.stack(W), np.stack(rows), np.stack(bl), msgs)
        for c, off in ((a, 0), (b, 1)):
            check_outcomes(c, proofs[off::2], outcomes[off::2], precheck, idx=list(range(cnt)))
    finally:
        a.free()
        b.free()
        cg.srs_free(h)


# ---- 5. variable form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precheck", [False, True], ids=["nocheck", "precheck"])
@pytest.mark.parametrize("transcript", ["host", "device"])
def test_variable_form(cg, tau, transcript, precheck):
    from tests.test_gpu_vars_prove import batch
    sc = bu.synthetic_circuit(6, 3, seed=66)
    h = cg.srs_generate(tau, sc.n + 3)
    pk, _ = cg.plonk_preprocess_vars(h, sc.n, 3, sc.selectors_mont(), np.array(sc.wire_vars), sc.num_vars)
    P = 5
    ws, vs, ps, bls = batch(sc, [400 + i for i in range(P)])
    msgs = [b"v%d" % i for i in range(P)]
    lone = [bytes(cg.plonk_prove(pk, ws[i], ps[i], bls[i], msgs[i])) for i in range(P)]      # the evals-form proofs
    # one variable of witness 2 changed so that a gate fails: the verdict of the expanded columns, from the oracle's loops
    idx, sel = position_index(sc), [np.array(col, dtype=object) for col in sc.selectors]
    wv = np.array(sc.wire_vars)
    vals = bu.from_mont_array(vs[2])
    want = None
    for var in range(sc.num_vars):
        mutated = list(vals)
        mutated[var] = (mutated[var] + 12345) % R
        cols = [[mutated[wv[i][j]] for j in range(sc.n)] for i in range(5)]
        v = numpy_verdict(sc, idx, sel, cols, bu.from_mont_array(ps[2]))
        if v[0] == 1:
            want = v
            vs = vs.copy()
            vs[2, var] = bu.to_mont_array([mutated[var]])[0]
            break
    assert want is not None, "no variable whose change fails a gate"
    try:
        with modes(cg, transcript, precheck):
            proofs, outcomes = cg.plonk_prove_each([pk] * P, vs, ps, bls, msgs, input_form="vars")
        for i in range(P):
            o = outcomes[i]
            print(i, o.status, o.degree_flags, got_tuple(o.fault))
            if i != 2:
                assert o.status == 0 and bytes(proofs[i]) == lone[i]
                continue
            assert o.status == ERR_PROOF and o.degree_flags != 0 and bytes(proofs[i]) == ONES
            # (a gathered witness satisfies every copy constraint: the gate verdict of the expanded columns)
            assert got_tuple(o.fault) == ((want[:6] + (0,)) if precheck else (0,) * 7)
    finally:
        cg.plonk_free_key(pk)
        cg.srs_free(h)


# ---- 6. edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precheck", [False, True], ids=["nocheck", "precheck"])
@pytest.mark.parametrize("transcript", ["host", "device"])
def test_edges(cg, log9, transcript, precheck):
    c = log9
    g, b = c.good[0], c.bad[0]
    with modes(cg, transcript, precheck):
        proofs, outcomes = cg.plonk_prove_each([c.pk], c.W[[g]], c.Pb[[g]], c.bl[[g]], [c.msgs[g]])
        check_outcomes(c, proofs, outcomes, precheck, idx=[g])
        proofs, outcomes = cg.plonk_prove_each([c.pk], c.W[[b]], c.Pb[[b]], c.bl[[b]], [c.msgs[b]])
        assert outcomes[0].status == ERR_PROOF and bytes(proofs[0]) == ONES
        if precheck:  # the only witness is refused by the check: nothing was proved, no degree was tested
            assert got_tuple(outcomes[0].fault) == c.exp[b] and outcomes[0].degree_flags == 0
        else:
            check_outcomes(c, proofs, outcomes, precheck, idx=[b])
        allbad = (c.bad * 3)[:22]
        calls0 = cg.plonk_sync_stats()[0]
        with bound(cg, 0):
            proofs, outcomes = cg.plonk_prove_each([c.pk] * 22, c.W[allbad], c.Pb[allbad], c.bl[allbad],
                                                   [c.msgs[p] for p in allbad])
        calls1 = cg.plonk_sync_stats()[0]
        assert all(o.status == ERR_PROOF for o in outcomes) and all(bytes(p) == ONES for p in proofs)
        if precheck:  # every witness refused: the call returns after the check, nothing is proved
            assert calls1 == calls0
            assert [got_tuple(o.fault) for o in outcomes] == [c.exp[p] for p in allbad]
        else:
            assert calls1 == calls0 + 1 and all(o.degree_flags != 0 and o.fault.kind == 0 for o in outcomes)
        assert cg.plonk_prove_each([], np.zeros((0, 5, c.sc.n, 4), np.uint64), np.zeros((0, 27, 4), np.uint64),
                                   np.zeros((0, 13, 4), np.uint64)) == ([], [])
    # a null outcome array is an argument error, as a null proof array is
    import ctypes
    L = cg.load()
    hd = (ctypes.c_uint64 * 1)(c.pk)
    pr = (cg.Proof * 1)()
    rc = L.capgpu_plonk_prove_each(hd, 1, cg._p(c.W[g].reshape(-1)), cg._p(c.Pb[g].reshape(-1)), ctypes.c_size_t(27), None,
                                   None, cg._p(c.bl[g].reshape(-1)), 0, pr, None)
    assert rc == -1
    # the reference's Vec<Result<..>>
    from cap_amd import proof as capi
    pick = [g, b]
    keys = [capi.ProvingKey(c.pk, c.sc.n, 27, None)] * 2
    res = capi.prove_each(keys, c.W[pick], c.Pb[pick], c.bl[pick], [c.msgs[p] for p in pick])
    assert bytes(res[0]) == c.lone[g] and isinstance(res[1], capi.TxnApiError) and "proof 0" in str(res[1])


# ---- 7. graphs: a child process that loads the library before torch -----------------------------------------------------------
GRAPH_CHILD = r"""
import numpy as np
from cap_amd import lib as cg
cg.load()
from cap_amd import bench_utils as bu
from oracle import bn254 as bn
cg.init(0)
assert cg.runtime_info()[0] >= 70200000, "the child runs on the runtime the library was built with"
tau = bn.SplitMix64(0xCA9).field(bn.R)
sc = bu.synthetic_circuit(6, 3, seed=21)
h = cg.srs_generate(tau, sc.n + 3)
pk, vk = cg.plonk_preprocess(h, sc.n, 3, sc.selectors_mont(), sc.sigma_mont())
W, Pb, Bl = [], [], []
for i in range(6):
    w, pubs = sc.witness(700 + i)
    W.append(sc.wires_mont(w)); Pb.append(bu.to_mont_array(pubs)); Bl.append(bu.to_mont_array(bu.blinders(800 + i)))
W, Pb, Bl = np.stack(W), np.stack(Pb), np.stack(Bl)
bad = (1, 4)
for p in bad:
    W[p, 4, sc.n // 2, 0] ^= np.uint64(1)
good = [p for p in range(6) if p not in bad]
msgs = [b"g%d" % i for i in range(6)]
ones = b"\xff" * 1152
d6, d4 = cg.DevBuf.from_numpy(W), cg.DevBuf.from_numpy(W[good])
for mode in ("host", "device"):
    for precheck in (False, True):
        cg.plonk_set_transcript(mode)
        cg.plonk_set_precheck(precheck)
        cap0, rep0 = cg.plonk_graph_stats()
        seen = []
        for rnd in range(4):
            proofs, outcomes = cg.plonk_prove_each_dev([pk] * 6, d6, Pb, Bl, msgs)
            seen.append([(bytes(p), o.status, o.degree_flags, o.fault.kind) for p, o in zip(proofs, outcomes)])
            # a plain call of the four good ones in between: its graphs are its own
            plain = cg.plonk_prove_multi([pk] * 4, d4, Pb[good], Bl[good], [msgs[p] for p in good])
            assert [bytes(p) for p in plain] == [seen[-1][p][0] for p in good], (mode, precheck, rnd)
        cap1, rep1 = cg.plonk_graph_stats()
        assert seen[0] == seen[1] == seen[2] == seen[3], (mode, precheck)
        for p in range(6):
            assert (seen[0][p][1] == -7) == (p in bad) and (seen[0][p][0] == ones) == (p in bad), (mode, precheck, p)
            assert (seen[0][p][2] != 0) == (p in bad) and (seen[0][p][3] != 0) == (p in bad and precheck)
        assert cap1 > cap0 and rep1 > rep0, (mode, precheck, cap0, cap1, rep0, rep1)
        print(mode, precheck, "captured", cap1 - cap0, "replayed", rep1 - rep0)
cg.plonk_set_precheck(False)
print("graphs OK")
"""


def test_graph_replay_keeps_outcome_calls_and_plain_calls_apart():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), CAPGPU_TEST_LIBRARY_FIRST="1")
    r = subprocess.run([sys.executable, "-c", GRAPH_CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "graphs OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


# ---- 8. a reserved call grows nothing -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("transcript,precheck,form", [("host", True, "evals"), ("device", True, "coeffs")])
def test_reserved_context_grows_nothing(cg, log9, transcript, precheck, form):
    c = log9
    wires = c.W if form == "evals" else c.Wc
    handles = [c.pk] * c.P
    with modes(cg, transcript, precheck), bound(cg, 0):
        cg.trim()
        cg.plonk_reserve(c.pk, c.P, form, slot=0)
        g0 = cg.scratch_stats()
        proofs, outcomes = cg.plonk_prove_each(handles, wires, c.Pb, c.bl, c.msgs, input_form=form)
        g1 = cg.scratch_stats()
        print(transcript, form, "after reserve:", g0, "->", g1)
        assert g1["grow_events"] == g0["grow_events"] and g1["grow_bytes"] == g0["grow_bytes"], (g0, g1)
        check_outcomes(c, proofs, outcomes, precheck)
        cg.trim()                                          # control: on a trimmed context the same call allocates
        g2 = cg.scratch_stats()
        again = cg.plonk_prove_each(handles, wires, c.Pb, c.bl, c.msgs, input_form=form)
        g3 = cg.scratch_stats()
        assert g3["grow_events"] - g2["grow_events"] >= 1 and g3["grow_bytes"] - g2["grow_bytes"] > 0
        assert signature(*again) == signature(proofs, outcomes)


# ---- 9. a caller's stream -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transcript", ["host", "device"])
def test_on_a_callers_stream(cg, log9, transcript):
    import torch
    c = log9
    S = torch.cuda.Stream()
    handles = [c.pk] * c.P
    t = torch.from_numpy(c.W.reshape(-1).view(np.int64)).cuda()
    d = cg.DevBuf.from_ptr(t.data_ptr(), t.numel() * t.element_size())
    cg.set_device(0)
    try:
        with modes(cg, transcript, True):
            with cg.on_stream(S):
                on_s = cg.plonk_prove_each_dev(handles, d, c.Pb, c.bl, c.msgs)
            own = cg.plonk_prove_each_dev(handles, d, c.Pb, c.bl, c.msgs)
        check_outcomes(c, *on_s, True)
        assert signature(*on_s) == signature(*own)
        assert np.array_equal(t.cpu().numpy().view(np.uint64), c.W.reshape(-1))
    finally:
        cg.set_stream(None)
        cg.sync_all()
        cg.set_device(-1)


# ---- 10. the coalescer takes its verdicts from the outcomes -------------------------------------------------------------------
@pytest.mark.parametrize("transcript", ["host", "device"])
def test_coalescer_proves_a_gathered_batch_once(cg, log9, transcript):
    c = log9
    T = 12
    bad_callers = {2: c.bad[0], 6: c.bad[1], 9: next(p for p in c.bad if c.lab[p] == "public input")}
    src = [bad_callers.get(t, c.good[t % len(c.good)]) for t in range(T)]
    with modes(cg, transcript, False):
        lone_err = {t: c.lone_error(src[t]) for t in bad_callers}
        results = [None] * T
        start = threading.Barrier(T)

        def worker(t):
            p = src[t]
            start.wait()
            try:
                results[t] = cg.plonk_prove(c.pk, c.W[p], c.Pb[p], c.bl[p], c.msgs[p])
            except cg.CapGpuError as e:
                results[t] = e

        cg.plonk_set_coalescing(20000, 16)
        try:
            b0, p0 = cg.plonk_coalescing_stats()
            calls0 = cg.plonk_sync_stats()[0]
            threads = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
            for th in threads:
                th.start()
            for th in threads:
                th.join(timeout=300)
            b1, p1 = cg.plonk_coalescing_stats()
            calls1 = cg.plonk_sync_stats()[0]
        finally:
            cg.plonk_set_coalescing(0)
    print("batches", b1 - b0, "proofs", p1 - p0, "prove calls", calls1 - calls0)
    for t in range(T):
        if t in bad_callers:
            assert isinstance(results[t], cg.CapGpuError) and results[t].code == ERR_PROOF
            assert str(results[t]) == lone_err[t], f"caller {t}"
        else:
            assert bytes(results[t]) == c.lone[src[t]], f"caller {t}"
    assert p1 - p0 == T and b1 - b0 >= 1
    # every gathered batch is proved ONCE - no request-by-request re-run of a batch that held a bad witness
    assert calls1 - calls0 == b1 - b0
