"""capgpu_plonk_prove_given_one / _io_one: ONE proof per call from the values its circuit is given, gathered by the
coalescer into one solve and one device batch.  The contract: whatever shared the batch, every caller's proof, outcome,
solver status and - _io - public inputs are bit for bit those of capgpu_plonk_prove_given[_io] with count = 1 on its inputs
alone in the same modes (with degree_flags 0 beside a fault); a request that cannot run fails alone."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from cap_amd import bench_utils as bu
from cap_amd.lib import SOLVER_DERIVE_PUBLIC, SOLVER_LINEAR
from tests.test_gpu_check_witness import got_tuple
from tests.test_gpu_prove_each import ERR_PROOF, ONES, modes
from tests.test_gpu_solve import harness_given, mont_rows, status_tuples
from tests.test_gpu_solve_io import IoHand
from tests.test_gpu_solve_packed import zero_denominator_circuit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRANSCRIPTS = ["host", "device"]
WINDOW = (20000, 16)


class Caller:
    """one caller's inputs: its key and the rows as long as ITS key's lists"""

    def __init__(self, key, g, pubs, bl, msg):
        self.key, self.pk, self.vk = key, key["pk"], key["vk"]
        self.g, self.pubs, self.bl, self.msg = np.ascontiguousarray(g), np.ascontiguousarray(pubs), np.ascontiguousarray(bl), msg


def sig(proof, outcome, solved):
    return (bytes(proof), outcome.status, outcome.degree_flags, got_tuple(outcome.fault), (solved.kind, solved.row))


def lone(cg, c):
    """the comparison call: capgpu_plonk_prove_given with count = 1 on this caller's inputs alone"""
    proofs, outcomes, solved = cg.plonk_prove_given([c.pk], c.g[None], c.pubs[None], c.bl[None], [c.msg])
    return sig(proofs[0], outcomes[0], solved[0])


def lone_io(cg, c):
    proofs, outcomes, solved, pubs = cg.plonk_prove_given_io([c.pk], c.g[None], c.bl[None], [c.msg])
    return sig(proofs[0], outcomes[0], solved[0]), pubs[0].copy()


def one(cg, c):
    return sig(*cg.plonk_prove_given_one(c.pk, c.g, c.pubs, c.bl, c.msg))


def io_one(cg, c):
    proof, outcome, solved, pubs = cg.plonk_prove_given_io_one(c.pk, c.g, c.bl, c.msg)
    return sig(proof, outcome, solved), pubs


def counters(cg):
    b, p = cg.plonk_coalescing_stats()
    return {"batches": b, "proofs": p, "launches": cg.plonk_solve_stats()["launches"],
            "bytes": cg.plonk_input_stats()["witness_bytes_h2d"], "prove_calls": cg.plonk_sync_stats()[0]}


def at_once(cg, calls, window=WINDOW):
    """every call from a thread of its own, released together, with coalescing on -> (results, counter deltas); a
    CapGpuError is a result"""
    T = len(calls)
    results = [None] * T
    start = threading.Barrier(T)

    def worker(t):
        start.wait()
        try:
            results[t] = calls[t]()
        except cg.CapGpuError as e:
            results[t] = e

    cg.plonk_set_coalescing(*window)
    try:
        c0 = counters(cg)
        threads = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(timeout=300)
        alive = [th.is_alive() for th in threads]
        c1 = counters(cg)
    finally:
        cg.plonk_set_coalescing(0)
    assert not any(alive), alive
    return results, {k: c1[k] - c0[k] for k in c0}


class Keys6:
    """three keys of one SRS at n = 2^6 with different (num_given, num_inputs): A and B from the synthetic generator (B with
    one more given value), Z the zero-denominator circuit of tests/test_gpu_solve_packed.py; six witnesses of A and of B"""

    def __init__(self, cg, tau):
        self.cg = cg
        sa, sb = bu.synthetic_circuit(6, 5, seed=71), bu.synthetic_circuit(6, 2, seed=72)
        zc, zgiven, zvals, _, self.row_b, _, _ = zero_denominator_circuit()
        assert sa.n == sb.n == zc.n
        self.h = cg.srs_generate(tau, sa.n + 3)
        self.keys = []
        for sc, seeds, extra in ((sa, [1, 2, 3, 4, 5, 6], False), (sb, [7, 8, 9, 10, 11, 12], True)):
            wires, pubs = sc.witnesses_mont(seeds, threads=2)
            given, gv = harness_given(sc, wires)
            if extra:                                                # the first OUT row's variable is given too
                given = given + [sc.wire_vars[4][sc.num_inputs]]
                gv = np.concatenate([gv, wires[:, 4, sc.num_inputs][:, None, :]], axis=1)
            self.keys.append(self.make_key(sc, given, gv, pubs))
        zg = mont_rows(zvals[:3])                                    # witness 1: the denominator of row B vanishes
        zp = mont_rows([[v[zgiven.index(zc.pub_vars[0])]] for v in zvals[:3]])
        self.keys.append(self.make_key(zc, zgiven, zg, zp))
        self.A, self.B, self.Z = self.keys
        assert len({k["gv"].shape[1] for k in self.keys}) == 3 and len({k["sc"].num_inputs for k in self.keys}) == 3
        # a key of the same shape without a solver
        self.no_solver, _ = cg.plonk_preprocess_vars(self.h, sa.n, sa.num_inputs, sa.selectors_mont(), np.array(sa.wire_vars),
                                                     sa.num_vars)

    def make_key(self, sc, given, gv, pubs):
        pk, vk = self.cg.plonk_preprocess_vars(self.h, sc.n, sc.num_inputs, sc.selectors_mont(), np.array(sc.wire_vars),
                                               sc.num_vars)
        self.cg.plonk_key_set_given(pk, given)
        return {"pk": pk, "vk": vk, "sc": sc, "given": given, "gv": gv, "pubs": pubs}

    def caller(self, key, j, t):
        return Caller(key, key["gv"][j], key["pubs"][j], bu.to_mont_array(bu.blinders(500 + t)), b"note %d" % t)

    def callers(self, T):
        """A B A B ...: caller t proves witness t // 2 of its key"""
        return [self.caller(self.keys[t % 2], (t // 2) % 6, t) for t in range(T)]

    def free(self):
        for k in self.keys:
            self.cg.plonk_free_key(k["pk"])
        self.cg.plonk_free_key(self.no_solver)
        self.cg.srs_free(self.h)


@pytest.fixture(scope="module")
def keys6(cg, tau):
    k = Keys6(cg, tau)
    yield k
    k.free()


@pytest.fixture(scope="module")
def key8(cg, tau):
    """one key at n = 2^8, six witnesses"""
    sc = bu.synthetic_circuit(8, 5)
    h = cg.srs_generate(tau, sc.n + 3)
    wires, pubs = sc.witnesses_mont([21, 22, 23, 24, 25, 26], threads=2)
    given, gv = harness_given(sc, wires)
    pk, vk = cg.plonk_preprocess_vars(h, sc.n, sc.num_inputs, sc.selectors_mont(), np.array(sc.wire_vars), sc.num_vars)
    cg.plonk_key_set_given(pk, given)
    key = {"pk": pk, "vk": vk, "sc": sc, "given": given, "gv": gv, "pubs": pubs}
    yield [Caller(key, gv[t % 6], pubs[t % 6], bu.to_mont_array(bu.blinders(800 + t)), b"n8 %d" % t) for t in range(12)]
    cg.plonk_free_key(pk)
    cg.srs_free(h)


def verify_all(cg, tau, callers, results):
    g2h = cg.g2_generator()
    bh = cg.g2_mul(g2h, tau)
    for t, (c, r) in enumerate(zip(callers, results)):
        proof = cg.Proof.from_buffer_copy(r[0])
        assert cg.plonk_verify(c.vk, g2h, bh, c.pubs, proof, c.msg), t


def check_gathered(callers, results, want, d, launches=True):
    T = len(callers)
    print("deltas", d)
    for t in range(T):
        assert results[t] == want[t], f"caller {t}"
    assert d["proofs"] == T and 1 <= d["batches"] < T
    if launches:                                                     # at most two keys: two solver launches per batch
        assert d["launches"] <= 2 * d["batches"] and d["launches"] < T
    assert d["bytes"] == sum(32 * c.g.shape[0] for c in callers)
    assert d["prove_calls"] == d["batches"]


# ---- 1. coalescing off: the count-1 call ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("transcript", TRANSCRIPTS)
def test_off_is_the_count_one_call(cg, keys6, transcript):
    cs = keys6.callers(2) + [keys6.caller(keys6.Z, 1, 2)]           # (the last: a zero denominator)
    with modes(cg, transcript, False):
        s0 = cg.plonk_coalescing_stats()
        for c in cs:
            assert one(cg, c) == lone(cg, c)
            got, want = io_one(cg, c), lone_io(cg, c)
            assert got[0] == want[0] and np.array_equal(got[1], want[1])
        assert cg.plonk_coalescing_stats() == s0
        assert one(cg, cs[0])[1] == 0 and one(cg, cs[2])[1] == ERR_PROOF and one(cg, cs[2])[0] == ONES


# ---- 2. gathered, all good ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transcript", TRANSCRIPTS)
def test_gathered_two_keys_at_log6(cg, tau, keys6, transcript):
    cs = keys6.callers(12)
    with modes(cg, transcript, False):
        want = [lone(cg, c) for c in cs]
        results, d = at_once(cg, [lambda c=c: one(cg, c) for c in cs])
    check_gathered(cs, results, want, d)
    assert all(r[1] == 0 and r[4] == (0, 0) for r in results)
    verify_all(cg, tau, cs, results)


@pytest.mark.parametrize("transcript", TRANSCRIPTS)
def test_gathered_one_key_at_log8(cg, tau, key8, transcript):
    cs = key8
    with modes(cg, transcript, False):
        want = [lone(cg, c) for c in cs]
        results, d = at_once(cg, [lambda c=c: one(cg, c) for c in cs])
    check_gathered(cs, results, want, d)
    assert d["launches"] == d["batches"]                           # one key: one solver launch per batch
    verify_all(cg, tau, cs, results)


# ---- 3. a gathered batch past its bad members ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["nocheck", "precheck", "compact"])
def test_gathered_past_bad_members(cg, keys6, mode):
    cs = keys6.callers(12)
    clean = list(cs)
    for t in (2, 9):                                                 # the value the solver is given; the public inputs stay
        c, key = cs[t], cs[t].key
        g = c.g.copy()
        g[key["given"].index(key["sc"].pub_vars[0])] = bu.to_mont_array([12345 + t])[0]
        cs[t] = Caller(key, g, c.pubs, c.bl, c.msg)
    cs[6] = keys6.caller(keys6.Z, 1, 6)                              # the denominator of its row B vanishes
    bad = (2, 6, 9)
    with modes(cg, "device", mode != "nocheck"):
        cg.plonk_set_compaction(mode == "compact")
        try:
            want = [lone(cg, c) for c in cs]
            want_clean = {t: lone(cg, clean[t]) for t in range(12) if t not in bad}
            results, d = at_once(cg, [lambda c=c: one(cg, c) for c in cs])
        finally:
            cg.plonk_set_compaction(False)
    print(mode, "deltas", d, "bad outcomes", [results[t][1:] for t in bad])
    for t in range(12):
        assert results[t] == want[t], f"caller {t}"
        if t in bad:
            assert results[t][0] == ONES and results[t][1] == ERR_PROOF
            if mode == "nocheck":
                assert results[t][3][0] == 0 and results[t][2] != 0
            else:                                                    # the lone call returns after the check: never proved
                assert results[t][3][0] != 0 and results[t][2] == 0
        else:
            assert results[t][1] == 0 and results[t] == want_clean[t]
    assert results[6][4] == (1, keys6.row_b) and results[2][4] == (0, 0)
    assert d["proofs"] == 12 and d["launches"] < 12


# ---- 4. _io gathered, and _one beside _io_one ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def io_keys(cg, tau):
    """two keys of one SRS at n = 2^9 whose public inputs are derived (SOLVER_LINEAR | SOLVER_DERIVE_PUBLIC)"""
    hands = [IoHand(9, 301), IoHand(9, 302)]
    h = cg.srs_generate(tau, hands[0].sc.n + 3)
    keys = []
    for c in hands:
        pk, vk = cg.plonk_preprocess_vars(h, c.sc.n, 6, c.sc.selectors_mont(), np.array(c.sc.wire_vars), c.sc.num_vars)
        cg.plonk_key_set_solver(pk, c.given, c.hints, SOLVER_LINEAR | SOLVER_DERIVE_PUBLIC)
        vals = [v for p, v in enumerate(c.values(5)) if p != 2]      # (witness 2 has a zero denominator)
        keys.append({"pk": pk, "vk": vk, "sc": c.sc, "given": c.given, "gv": mont_rows(vals)})
    yield keys
    for k in keys:
        cg.plonk_free_key(k["pk"])
    cg.srs_free(h)


def io_callers(keys, T, pubs_of=None):
    out = []
    for t in range(T):
        key = keys[t % 2]
        g = key["gv"][(t // 2) % 4]
        pubs = np.zeros((6, 4), np.uint64) if pubs_of is None else pubs_of[t]
        out.append(Caller(key, g, pubs, bu.to_mont_array(bu.blinders(4100 + t)), b"io %d" % t))
    return out


def derived_pubs(cg, c):
    """capgpu_plonk_pub_inputs of the caller's solved assignment"""
    d_g = cg.DevBuf.from_numpy(np.ascontiguousarray(c.g[None]))
    d_v, _ = cg.plonk_solve_vars(c.pk, d_g, 1)
    d_p = cg.plonk_pub_inputs(c.pk, d_v, 1)
    cg.sync_all()
    pubs = d_p.to_numpy().reshape(-1, 4).copy()
    for d in (d_g, d_v, d_p):
        d.free()
    return pubs


def test_io_gathered(cg, tau, io_keys):
    cs = io_callers(io_keys, 8)
    with modes(cg, "device", False):
        want = [lone_io(cg, c) for c in cs]
        pubs = [derived_pubs(cg, c) for c in cs]
        results, d = at_once(cg, [lambda c=c: io_one(cg, c) for c in cs])
    print("deltas", d)
    g2h = cg.g2_generator()
    bh = cg.g2_mul(g2h, tau)
    for t, c in enumerate(cs):
        assert results[t][0] == want[t][0] and results[t][0][1] == 0, t
        assert np.array_equal(results[t][1], pubs[t]) and np.array_equal(want[t][1], pubs[t]), t
        assert cg.plonk_verify(c.vk, g2h, bh, pubs[t], cg.Proof.from_buffer_copy(results[t][0][0]), c.msg), t
    assert d["proofs"] == 8 and d["launches"] <= 2 * d["batches"] and d["launches"] < 8
    assert d["bytes"] == sum(32 * c.g.shape[0] for c in cs) and d["prove_calls"] == d["batches"]


def test_one_and_io_one_never_share_a_batch(cg, io_keys):
    with modes(cg, "device", False):
        pubs = [derived_pubs(cg, c) for c in io_callers(io_keys[:1] * 2, 8)]
        cs = io_callers(io_keys[:1] * 2, 8, pubs)                    # one key; the plain callers pass the derived inputs
        want = [lone(cg, c) if t % 2 else lone_io(cg, c) for t, c in enumerate(cs)]
        calls = [(lambda c=c: one(cg, c)) if t % 2 else (lambda c=c: io_one(cg, c)) for t, c in enumerate(cs)]
        results, d = at_once(cg, calls)
    print("deltas", d)
    for t in range(8):
        if t % 2:
            assert results[t] == want[t], t
        else:
            assert results[t][0] == want[t][0] and np.array_equal(results[t][1], want[t][1]), t
    assert d["proofs"] == 8 and d["batches"] >= 2


# ---- 5. one request fails alone -----------------------------------------------------------------------------------------------------
def test_a_request_that_cannot_run_fails_alone(cg, keys6):
    cs = keys6.callers(6)
    with modes(cg, "device", False):
        want = [lone(cg, c) for c in cs]
        calls = [lambda c=c: one(cg, c) for c in cs]
        c1, c4 = cs[1], cs[4]
        calls[1] = lambda: sig(*cg.plonk_prove_given_one(keys6.no_solver, c1.g, keys6.A["pubs"][0], c1.bl, c1.msg))
        calls[4] = lambda: one(cg, Caller(c4.key, c4.g[:-1], c4.pubs, c4.bl, c4.msg))      # one given value short
        results, d = at_once(cg, calls)
    print("deltas", d, results[1], results[4])
    for t in (1, 4):
        assert isinstance(results[t], cg.CapGpuError) and results[t].code == -1, results[t]
    assert "capgpu_plonk_prove_given_one: the key has no solver (capgpu_plonk_key_set_given gives it one)" in str(results[1])
    ng, ni = c4.g.shape[0], c4.pubs.shape[0]
    assert (f"capgpu_plonk_prove_given_one: {ng - 1} given values and {ni} public inputs passed, the key has {ng} and {ni}"
            in str(results[4]))
    for t in (0, 2, 3, 5):
        assert results[t] == want[t], t
    assert d["proofs"] == 4 and d["bytes"] == sum(32 * cs[t].g.shape[0] for t in (0, 2, 3, 5))


# ---- 6. a cut batch: a child process with two contexts ---------------------------------------------------------------------------------
CUT_CHILD = r"""
import os
import tempfile
from cap_amd import lib as cg
cg.load()
from oracle import bn254 as bn
from tests import test_gpu_prove_given_one as M
from tests.test_gpu_prove_each import modes
cg.init(0)
assert cg.device_count() == 2
tau = bn.SplitMix64(0xCA9).field(bn.R)
keys = M.Keys6(cg, tau)
cs = keys.callers(16)
for transcript in ("host", "device"):
    with modes(cg, transcript, False):
        want = [M.lone(cg, c) for c in cs]
        cg.trace_enable(True)
        results, d = M.at_once(cg, [lambda c=c: M.one(cg, c) for c in cs], (20000, 16))
        cg.trace_enable(False)
    M.check_gathered(cs, results, want, d)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cut.trace")
        cg.trace_dump(path)
        cuts = [l.split() for l in open(path) if " co_run " in l]
    print(transcript, "batches", d["batches"], "co_run", [(int(l[3]), int(l[4])) for l in cuts])
    assert any(int(l[4]) > 0 and int(l[3]) >= 2 for l in cuts), "no batch was cut"
    assert d["batches"] >= 2
    M.verify_all(cg, tau, cs, results)
keys.free()
print("cut OK")
"""


def test_a_cut_batch():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), CAPGPU_TEST_LIBRARY_FIRST="1",
               CAPGPU_CONTEXTS_PER_DEVICE="2", CAPGPU_DEAL_MIN="2", CAPGPU_COALESCE_SPLIT="3")
    r = subprocess.run([sys.executable, "-c", CUT_CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "cut OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


# ---- 7. solve form and inverse form ----------------------------------------------------------------------------------------------------
def test_gathered_under_the_deferred_form_and_gcd_inversion(cg, keys6):
    cs = keys6.callers(12)
    with modes(cg, "device", False):
        plain = [lone(cg, c) for c in cs]
        inverse = cg.fr_get_inverse_form()
        try:
            for key in (keys6.A, keys6.B):
                cg.plonk_key_set_solve_form(key["pk"], cg.SOLVE_FORM_DEFERRED)
            cg.fr_set_inverse_form("gcd")
            assert cg.fr_get_inverse_form() == cg.INVERSE_GCD
            want = [lone(cg, c) for c in cs]
            results, d = at_once(cg, [lambda c=c: one(cg, c) for c in cs])
        finally:
            cg.fr_set_inverse_form(inverse)
            for key in (keys6.A, keys6.B):
                cg.plonk_key_set_solve_form(key["pk"], cg.SOLVE_FORM_DIRECT)
    check_gathered(cs, results, want, d, launches=False)
    assert want == plain                                            # (either form gives the same assignments and proofs)


# ---- 8. wire-form and given-value callers at once on one key ------------------------------------------------------------------------------
def test_wire_form_and_given_value_callers_at_once(cg, keys6):
    cs = [keys6.caller(keys6.A, t % 6, t) for t in range(8)]
    with modes(cg, "device", False):
        vars_h = [np.ascontiguousarray(cg.plonk_solve_vars(c.pk, c.g[None], 1)[0]).reshape(-1, 4) for c in cs]
        want = [lone(cg, c) for c in cs]
        calls = [(lambda c=c: one(cg, c)) if t % 2 else
                 (lambda c=c, v=vars_h[t]: bytes(cg.plonk_prove(c.pk, v, c.pubs, c.bl, c.msg, input_form="vars")))
                 for t, c in enumerate(cs)]
        results, d = at_once(cg, calls)
    print("deltas", d)
    for t in range(8):
        if t % 2:
            assert results[t] == want[t], t
        else:
            assert results[t] == want[t][0], t                      # the same proof by either road
    assert d["proofs"] == 8 and d["batches"] >= 2                    # the two kinds never share a batch
