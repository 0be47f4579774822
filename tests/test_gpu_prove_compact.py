"""Batch compaction of the outcome calls (capgpu_plonk_set_compaction): with the witness check on, the witnesses the check
refused leave the batch before round 1 and the survivors are proved as a smaller batch.  Survivors are word for word the
lone capgpu_plonk_prove's proofs and sit at the caller's indices; a refused proof has its fault, an all-ones record and -
never proved - no degree flags; capgpu_plonk_compaction_stats counts the calls, the proofs dropped and the witness rows
k_move_rows was handed.  By host buffers, device buffers (whose columns are copied, never written), variables, two keys,
tickets and graph replay, for every shape of refusal mask; and nothing moves while the mode or the check is off."""
import contextlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from cap_amd import bench_utils as bu
from oracle.bn254 import R
from tests.test_gpu_check_witness import got_tuple, numpy_verdict, position_index
from tests.test_gpu_prove_each import ERR_PROOF, ONES, Cases, bound, check_outcomes, modes, signature

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(4, 1), (6, 0)]           # a row of 2560 B (not a multiple of k_move_rows' 4096 B tile), and one of 10 KB
TRANSCRIPTS = ["host", "device"]


def copy_ratio():
    src = open(os.path.join(ROOT, "cap_amd", "csrc", "compact.hpp")).read()
    return int(re.search(r"#define CAP_COMPACT_COPY_RATIO (\d+)", src).group(1))


def plan_moves(refused):
    """what compact_plan does with this mask: (P', moves) - one move per refused slot below P'"""
    survivors = len(refused) - sum(refused)
    return survivors, sum(refused[:survivors])


@contextlib.contextmanager
def compacting(cg, transcript, precheck=True, on=True):
    """the modes of one test, context 0 (an unbound host call would be dealt over two contexts and compact per part)"""
    with modes(cg, transcript, precheck), bound(cg, 0):
        cg.plonk_set_compaction(on)
        try:
            yield
        finally:
            cg.plonk_set_compaction(False)


def stats_delta(cg, fn):
    s0 = cg.plonk_compaction_stats()
    out = fn()
    s1 = cg.plonk_compaction_stats()
    return out, tuple(b - a for a, b in zip(s0, s1))


def check_compacted(c, proofs, outcomes, idx=None, lone=None):
    """a compacted call's results for the cases `idx` of c: survivors are the lone proofs (lone[k] when given), refused
    ones carry the oracle's fault, an all-ones record and no degree flags"""
    idx = list(range(c.P)) if idx is None else idx
    assert len(proofs) == len(outcomes) == len(idx)
    for k, p in enumerate(idx):
        o, e = outcomes[k], c.exp[p]
        print(k, p, c.lab[p], "status", o.status, "flags", o.degree_flags, "fault", got_tuple(o.fault), "expected", e)
        if e[0] == 0:
            assert o.status == 0 and o.degree_flags == 0 and o.fault.kind == 0, f"slot {k} (case {p})"
            assert bytes(proofs[k]) == (lone[k] if lone else c.lone[p]), f"slot {k} (case {p}): not the lone call's proof"
            continue
        assert o.status == ERR_PROOF and bytes(proofs[k]) == ONES, f"slot {k} (case {p})"
        assert got_tuple(o.fault) == e, f"slot {k} (case {p})"
        assert o.degree_flags == 0, f"slot {k} (case {p}): a dropped proof was never proved"


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "log%d-nin%d" % s)
def shape(request, cg, tau):
    c = Cases(cg, tau, *request.param)
    yield c
    c.free()


@pytest.fixture(scope="module")
def log4(cg, tau):
    c = Cases(cg, tau, 4, 1)
    yield c
    c.free()


# ---- 1. the same results as the uncompacted call ------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["evals", "coeffs"])
@pytest.mark.parametrize("transcript", TRANSCRIPTS)
def test_same_results_as_uncompacted(cg, shape, transcript, form):
    c = shape
    wires = c.W if form == "evals" else c.Wc
    handles = [c.pk] * c.P
    refused = [int(e[0] != 0) for e in c.exp]
    assert 0 < sum(refused) < c.P

    def call():
        return cg.plonk_prove_each(handles, wires, c.Pb, c.bl, c.msgs, input_form=form)

    assert cg.plonk_get_compaction() is False
    with compacting(cg, transcript, on=False):
        off, d_off = stats_delta(cg, call)
    with compacting(cg, transcript):
        assert cg.plonk_get_compaction() is True
        on, d_on = stats_delta(cg, call)
    print("stats off", d_off, "on", d_on, "mask", refused)
    check_outcomes(c, *off, True)                          # (asserts degree_flags != 0 for every refused proof)
    check_compacted(c, *on)
    for p in range(c.P):
        assert bytes(on[0][p]) == bytes(off[0][p]) and on[1][p].status == off[1][p].status
        assert got_tuple(on[1][p].fault) == got_tuple(off[1][p].fault)
    assert d_off == (0, 0, 0)
    assert d_on == (1, len(c.bad), plan_moves(refused)[1])


# ---- 2. every shape of mask ---------------------------------------------------------------------------------------------------
MASKS = {
    "tail": [0, 0, 0, 0, 0, 1, 1, 1],            # nothing moves
    "front": [1, 1, 1, 0, 0, 0, 0, 0],           # min(bad, P') moves
    "alternating": [1, 0, 1, 0, 1, 0, 1, 0],
    "all-but-last": [1, 1, 1, 1, 1, 1, 1, 0],    # P' = 1
    "all": [1] * 8,                              # the early return
    "none": [0] * 8,
}


@pytest.mark.parametrize("mask", list(MASKS), ids=list(MASKS))
@pytest.mark.parametrize("transcript", TRANSCRIPTS)
def test_mask_geometry(cg, log4, transcript, mask):
    c = log4
    refused = MASKS[mask]
    # slot k takes good / bad cases in turn, with blinders and a message of its OWN: two survivors made from the same
    # witness are still different proofs, so a survivor that lands in the wrong slot is seen
    idx = [(c.bad if r else c.good)[k % (len(c.bad) if r else len(c.good))] for k, r in enumerate(refused)]
    bl = c.bl[:8]
    msgs = [b"slot-%d" % k for k in range(8)]
    lone = [None if r else bytes(cg.plonk_prove(c.pk, c.W[p], c.Pb[p], bl[k], msgs[k]))
            for k, (p, r) in enumerate(zip(idx, refused))]
    bad = sum(refused)
    with compacting(cg, transcript):
        (proofs, outcomes), d = stats_delta(
            cg, lambda: cg.plonk_prove_each([c.pk] * 8, c.W[idx], c.Pb[idx], bl, msgs))
        if not bad:
            plain = cg.plonk_prove_multi([c.pk] * 8, c.W[idx], c.Pb[idx], bl, msgs)
            assert [bytes(p) for p in plain] == [bytes(p) for p in proofs]
    print(mask, "stats", d)
    check_compacted(c, proofs, outcomes, idx, lone)
    survivors, moves = plan_moves(refused)
    assert d == ((1, bad, moves) if 0 < bad < 8 else (0, 0, 0))
    if mask == "tail":
        assert moves == 0
    if mask == "front":
        assert moves == min(bad, survivors)


# ---- 3. device buffers: the caller's columns are copied, never written --------------------------------------------------------
@pytest.mark.parametrize("form", ["evals", "coeffs"])
@pytest.mark.parametrize("transcript", TRANSCRIPTS)
def test_dev_columns_take_the_copy_route(cg, shape, transcript, form):
    c = shape
    wires = c.W if form == "evals" else c.Wc
    idx = [c.bad[0], c.good[0], c.bad[1], c.good[1], c.good[2], c.bad[2], c.bad[3], c.good[0]]   # 4 of 8 refused
    d = cg.DevBuf.from_numpy(wires[idx])
    before = d.to_numpy()
    msgs = [c.msgs[p] for p in idx]
    try:
        with compacting(cg, transcript):
            (proofs, outcomes), delta = stats_delta(
                cg, lambda: cg.plonk_prove_each_dev([c.pk] * 8, d, c.Pb[idx], c.bl[idx], msgs, input_form=form))
        assert np.array_equal(d.to_numpy(), before), "the caller's device buffer must stay untouched"
    finally:
        d.free()
    check_compacted(c, proofs, outcomes, idx)
    assert delta == (1, 4, 4)                              # the P' surviving rows are what the kernel copies


@pytest.mark.parametrize("transcript", TRANSCRIPTS)
def test_dev_columns_below_the_copy_threshold_run_uncompacted(cg, log4, transcript):
    c = log4
    ratio = copy_ratio()
    P = ratio + 3                                          # 1 refused: bad * ratio < P' = ratio + 2
    idx = [c.good[k % len(c.good)] for k in range(P)]
    idx[P // 2] = c.bad[0]
    d = cg.DevBuf.from_numpy(c.W[idx])
    msgs = [c.msgs[p] for p in idx]
    try:
        with compacting(cg, transcript):
            (proofs, outcomes), delta = stats_delta(
                cg, lambda: cg.plonk_prove_each_dev([c.pk] * P, d, c.Pb[idx], c.bl[idx], msgs))
            # the same witness among seven good ones: the copy pays whenever the ratio is at least 7
            idx2 = [c.good[k % len(c.good)] for k in range(7)] + [c.bad[0]]
            d2 = cg.DevBuf.from_numpy(c.W[idx2])
            _, delta2 = stats_delta(cg, lambda: cg.plonk_prove_each_dev([c.pk] * 8, d2, c.Pb[idx2], c.bl[idx2],
                                                                        [c.msgs[p] for p in idx2]))
            d2.free()
    finally:
        d.free()
    print("ratio", ratio, "P", P, "stats", delta, delta2)
    assert delta == (0, 0, 0)
    check_outcomes(c, proofs, outcomes, True, idx=idx)     # as the mode off: the refused one rode along (flags != 0)
    assert delta2 == ((1, 1, 7) if ratio >= 7 else (0, 0, 0))


# ---- 4. variable form ---------------------------------------------------------------------------------------------------------
def gate_breaking_change(sc, idx, sel, vals, pubs):
    """one variable changed so that a gate fails -> (variable, new value, the oracle's verdict of the expanded columns)"""
    wv = np.array(sc.wire_vars)
    for var in range(sc.num_vars):
        mutated = list(vals)
        mutated[var] = (mutated[var] + 12345) % R
        cols = [[mutated[wv[i][j]] for j in range(sc.n)] for i in range(5)]
        v = numpy_verdict(sc, idx, sel, cols, pubs)
        if v[0] == 1:
            return var, mutated[var], v
    raise AssertionError("no variable whose change fails a gate")


@pytest.fixture(scope="module")
def vars_batch(cg, tau):
    from tests.test_gpu_vars_prove import batch
    sc = bu.synthetic_circuit(6, 3, seed=66)
    h = cg.srs_generate(tau, sc.n + 3)
    pk, _ = cg.plonk_preprocess_vars(h, sc.n, 3, sc.selectors_mont(), np.array(sc.wire_vars), sc.num_vars)
    P = 5
    ws, vs, ps, bls = batch(sc, [400 + i for i in range(P)])
    msgs = [b"v%d" % i for i in range(P)]
    lone = [bytes(cg.plonk_prove(pk, ws[i], ps[i], bls[i], msgs[i])) for i in range(P)]
    idx, sel = position_index(sc), [np.array(col, dtype=object) for col in sc.selectors]
    vs, want = vs.copy(), {}
    for i in (0, 2):                                       # slot 0 among them: both refused slots lie below P' = 3
        var, val, want[i] = gate_breaking_change(sc, idx, sel, bu.from_mont_array(vs[i]), bu.from_mont_array(ps[i]))
        vs[i, var] = bu.to_mont_array([val])[0]
    yield pk, P, vs, ps, bls, msgs, lone, want
    cg.plonk_free_key(pk)
    cg.srs_free(h)


@pytest.mark.parametrize("where", ["host", "dev"])
@pytest.mark.parametrize("transcript", TRANSCRIPTS)
def test_variable_form(cg, vars_batch, transcript, where):
    pk, P, vs, ps, bls, msgs, lone, want = vars_batch
    d = cg.DevBuf.from_numpy(vs) if where == "dev" else None

    def call():
        if d is not None:
            return cg.plonk_prove_each_dev([pk] * P, d, ps, bls, msgs, input_form="vars")
        return cg.plonk_prove_each([pk] * P, vs, ps, bls, msgs, input_form="vars")

    try:
        with compacting(cg, transcript, on=False):
            off, d_off = stats_delta(cg, call)
        with compacting(cg, transcript):
            (proofs, outcomes), d_on = stats_delta(cg, call)
        if d is not None:
            assert np.array_equal(d.to_numpy().reshape(vs.shape), vs), "the caller's value vectors must stay untouched"
    finally:
        if d is not None:
            d.free()
    for i in range(P):
        o = outcomes[i]
        print(i, o.status, o.degree_flags, got_tuple(o.fault))
        assert bytes(proofs[i]) == bytes(off[0][i]) and o.status == off[1][i].status
        assert got_tuple(o.fault) == got_tuple(off[1][i].fault)
        if i not in want:
            assert o.status == 0 and o.degree_flags == 0 and bytes(proofs[i]) == lone[i]
            continue
        assert o.status == ERR_PROOF and bytes(proofs[i]) == ONES
        assert got_tuple(o.fault) == want[i][:6] + (0,)    # (gathered columns satisfy every copy constraint)
        assert o.degree_flags == 0 and off[1][i].degree_flags != 0
    assert d_off == (0, 0, 0) and d_on == (1, 2, 2)        # gathered columns are library scratch: two rows move in place


# ---- 5. two keys of one domain: the batch's first key changes -------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_keys(cg, tau):
    h = cg.srs_generate(tau, 512 + 3)
    a = Cases(cg, tau, 9, 27, srs=h, n_random=4, n_targeted=2)
    b = Cases(cg, tau, 9, 3, srs=h, n_random=4, n_targeted=2)
    yield a, b
    a.free()
    b.free()
    cg.srs_free(h)


@pytest.mark.parametrize("transcript", TRANSCRIPTS)
def test_two_keys_of_one_domain(cg, two_keys, transcript):
    a, b = two_keys
    cnt = min(a.P, b.P)
    assert a.exp[0][0] and b.exp[0][0], "slots 0 and 1 are refused: the compacted batch starts with another proof"
    handles, W, rows, bl, msgs, refused = [], [], [], [], [], []
    for p in range(cnt):
        for c in (a, b):
            row = np.zeros((27, 4), np.uint64)             # rows of the larger input count, as _multi uses them
            row[:c.nin] = c.Pb[p]
            handles.append(c.pk); W.append(c.W[p]); rows.append(row); bl.append(c.bl[p]); msgs.append(c.msgs[p])
            refused.append(int(c.exp[p][0] != 0))
    survivors, moves = plan_moves(refused)
    first = next(k for k, r in enumerate(refused) if not r)
    print("mask", refused, "first survivor", first, "moves", moves)
    with compacting(cg, transcript):
        (proofs, outcomes), d = stats_delta(
            cg, lambda: cg.plonk_prove_each(handles, np.stack(W), np.stack(rows), np.stack(bl), msgs))
        # the survivors of the 3-input key alone: the compacted rows are 3 inputs wide, not 27
        only_b = [k for k in range(2 * cnt) if k % 2 == 1 or refused[k]]
        sub, d_b = stats_delta(cg, lambda: cg.plonk_prove_each(
            [handles[k] for k in only_b], np.stack(W)[only_b], np.stack(rows)[only_b], np.stack(bl)[only_b],
            [msgs[k] for k in only_b]))
    for c, off in ((a, 0), (b, 1)):
        check_compacted(c, proofs[off::2], outcomes[off::2], idx=list(range(cnt)))
    assert d == (1, sum(refused), moves) and moves > 0
    assert signature(*sub) == [signature(proofs, outcomes)[k] for k in only_b]
    assert d_b[0] == 1


# ---- 6. tickets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transcript", TRANSCRIPTS)
def test_two_tickets_in_flight(cg, shape, transcript):
    c = shape
    half = c.P // 2
    parts = [list(range(half)), list(range(half, c.P))]
    masks = [[int(c.exp[p][0] != 0) for p in part] for part in parts]
    assert masks[0] != masks[1] and all(0 < sum(m) < len(m) for m in masks)

    def args(part):
        return [c.pk] * len(part), c.W[part], c.Pb[part], c.bl[part], [c.msgs[p] for p in part]

    with compacting(cg, transcript):
        sync = [cg.plonk_prove_each(*args(part)) for part in parts]
        s0 = cg.plonk_compaction_stats()
        t1, t2 = (cg.plonk_prove_each_async(*args(part)) for part in parts)   # the mode is read when a ticket starts
        got = [t1.wait(), t2.wait()]
        s1 = cg.plonk_compaction_stats()
    for part, mask, g, s in zip(parts, masks, got, sync):
        check_compacted(c, *g, idx=part)
        assert signature(*g) == signature(*s)
    assert tuple(y - x for x, y in zip(s0, s1)) == (2, sum(map(sum, masks)), sum(plan_moves(m)[1] for m in masks))


# ---- 7. graphs: a child process that loads the library before torch -------------------------------------------------------------
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
for i in range(4):
    w, pubs = sc.witness(700 + i)
    W.append(sc.wires_mont(w)); Pb.append(bu.to_mont_array(pubs)); Bl.append(bu.to_mont_array(bu.blinders(800 + i)))
W, Pb, Bl = np.stack(W), np.stack(Pb), np.stack(Bl)
msgs = [b"g%d" % i for i in range(4)]
lone = [bytes(cg.plonk_prove(pk, W[i], Pb[i], Bl[i], msgs[i])) for i in range(4)]
ones = b"\xff" * 1152
cg.set_device(0)
cg.plonk_set_precheck(True)
cg.plonk_set_compaction(True)
# one refused of four, at slot 0, 3, 0 - then 1 and 2: in place the move table is (3 -> 0), none, (3 -> 0), (3 -> 1),
# (3 -> 2) under ONE signature; replayed segments that had kept a table would put the wrong witness into a slot
SLOTS = (0, 3, 0, 1, 2)
for mode in ("host", "device"):
    cg.plonk_set_transcript(mode)
    for road in ("host", "dev"):
        cap0, rep0 = cg.plonk_graph_stats()
        s0 = cg.plonk_compaction_stats()
        for rnd, slot in enumerate(SLOTS):
            Wb = W.copy()
            Wb[slot, 4, sc.n // 2, 0] ^= np.uint64(1)
            if road == "dev":
                d = cg.DevBuf.from_numpy(Wb)
                proofs, outcomes = cg.plonk_prove_each_dev([pk] * 4, d, Pb, Bl, msgs)
                assert np.array_equal(d.to_numpy(), Wb.reshape(-1))
                d.free()
            else:
                proofs, outcomes = cg.plonk_prove_each([pk] * 4, Wb, Pb, Bl, msgs)
            for p in range(4):
                o = outcomes[p]
                if p == slot:
                    assert o.status == -7 and o.fault.kind != 0 and o.degree_flags == 0 and bytes(proofs[p]) == ones, (mode, road, rnd, p)
                else:
                    assert o.status == 0 and bytes(proofs[p]) == lone[p], (mode, road, rnd, p)
        cap1, rep1 = cg.plonk_graph_stats()
        s1 = cg.plonk_compaction_stats()
        moved = sum(3 if road == "dev" else int(slot < 3) for slot in SLOTS)
        assert tuple(b - a for a, b in zip(s0, s1)) == (len(SLOTS), len(SLOTS), moved), (mode, road, s0, s1)
        # (the copy route's staging is where host-resident witnesses were staged: the second road finds the first one's
        # segments under its own signature and only replays)
        assert rep1 > rep0 and (cap1 > cap0 or road == "dev"), (mode, road, cap0, cap1, rep0, rep1)
        print(mode, road, "captured", cap1 - cap0, "replayed", rep1 - rep0)
cg.plonk_set_compaction(False)
cg.plonk_set_precheck(False)
print("compact graphs OK")
"""


def test_graph_replay_does_not_keep_the_move_table():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), CAPGPU_TEST_LIBRARY_FIRST="1")
    r = subprocess.run([sys.executable, "-c", GRAPH_CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "compact graphs OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


# ---- 8. without the witness check nothing is compacted ------------------------------------------------------------------------
@pytest.mark.parametrize("transcript", TRANSCRIPTS)
def test_precheck_off_compacts_nothing(cg, shape, transcript):
    c = shape
    handles = [c.pk] * c.P

    def call():
        return cg.plonk_prove_each(handles, c.W, c.Pb, c.bl, c.msgs)

    with compacting(cg, transcript, precheck=False, on=False):
        off = call()
    with compacting(cg, transcript, precheck=False):
        on, d = stats_delta(cg, call)
    assert d == (0, 0, 0)
    check_outcomes(c, *on, False)
    assert signature(*on) == signature(*off)               # degree flags included
