"""capgpu_plonk_prove_notes / _dev / _async, _notes_plan, _reserve_notes, _notes_stats: one call over keys of SEVERAL domain
sizes.  The fixture is three keys (log n = 4, 6, 9) under ONE SRS of 2^9 + 3 points and a fourth key at log n = 6 under a
SECOND SRS - four groups: two differ by domain size, two same-sized ones only by SRS.  Each key keeps its cases of
tests/test_gpu_prove_each.py (unsatisfied witnesses and the wrong public input among them), and the notes are interleaved
so that no group is contiguous.  THE CONTRACT is checked word for word: every note's proof and outcome are what one
capgpu_plonk_prove_each call over its group alone writes, and a surviving proof is the lone capgpu_plonk_prove's."""
import ctypes
import os

import numpy as np
import pytest

from cap_amd import bench_utils as bu
from tests.test_gpu_prove_each import ERR_PROOF, ONES, Cases, bound, check_outcomes, modes, signature
from tests.test_gpu_vars_prove import at_end_of_a_mapping, batch

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, BAD_HANDLE = 0, -1, -4
UNKNOWN = 999999
NOTES = "capgpu_plonk_prove_notes"


class World:
    """the four Cases, the interleaved notes and their per-note arrays in the block verifier's layout"""

    def __init__(self, cg, tau):
        self.cg = cg
        self.h1 = cg.srs_generate(tau, 512 + 3)
        self.h2 = cg.srs_generate(tau, 64 + 3)
        self.cases = [Cases(cg, tau, 4, 1, srs=self.h1), Cases(cg, tau, 6, 0, srs=self.h1), Cases(cg, tau, 9, 27, srs=self.h1),
                      Cases(cg, tau, 6, 3, srs=self.h2)]
        self.nin = max(c.nin for c in self.cases)
        # the notes: witness p of every case in turn - no two members of a group are neighbours
        self.who = [(g, p) for p in range(max(c.P for c in self.cases)) for g, c in enumerate(self.cases) if p < c.P]
        self.count = len(self.who)
        self.handles = [self.cases[g].pk for g, _ in self.who]
        self.pub = np.zeros((self.count, self.nin, 4), np.uint64)
        for k, (g, p) in enumerate(self.who):
            self.pub[k, :self.cases[g].nin] = self.cases[g].Pb[p]
        self.bl = np.stack([self.cases[g].bl[p] for g, p in self.who])
        self.msgs = [self.cases[g].msgs[p] for g, p in self.who]
        self.members = [[k for k, (g, _) in enumerate(self.who) if g == gi] for gi in range(4)]

    def wires(self, form="evals"):
        return [(self.cases[g].W if form == "evals" else self.cases[g].Wc)[p] for g, p in self.who]

    def per_group(self, form="evals"):
        """one plonk_prove_each per group -> the signatures in note order"""
        out = [None] * self.count
        for gi, c in enumerate(self.cases):
            w = c.W if form == "evals" else c.Wc
            sig = signature(*self.cg.plonk_prove_each([c.pk] * c.P, w, c.Pb, c.bl, c.msgs, input_form=form))
            for p, k in enumerate(self.members[gi]):
                out[k] = sig[p]
        return out

    def check(self, proofs, outcomes, precheck):
        for gi, c in enumerate(self.cases):
            check_outcomes(c, [proofs[k] for k in self.members[gi]], [outcomes[k] for k in self.members[gi]], precheck)

    def free(self):
        for c in self.cases:
            c.free()
        self.cg.srs_free(self.h1)
        self.cg.srs_free(self.h2)


@pytest.fixture(scope="module")
def world(cg, tau):
    w = World(cg, tau)
    yield w
    w.free()


def delta(cg, before):
    now = cg.plonk_notes_stats()
    return {k: now[k] - before[k] for k in now}


# ---- 3. the contract, 7. into the verifier ------------------------------------------------------------------------------------
@pytest.mark.parametrize("precheck", [False, True], ids=["nocheck", "precheck"])
@pytest.mark.parametrize("transcript", ["host", "device"])
def test_contract(cg, tau, world, transcript, precheck):
    w = world
    with modes(cg, transcript, precheck):
        s0 = cg.plonk_notes_stats()
        proofs, outcomes = cg.plonk_prove_notes(w.handles, w.wires(), w.pub, w.bl, w.msgs)
        d = delta(cg, s0)
        want = w.per_group()
    assert d["calls"] == 1 and d["groups"] == 4
    w.check(proofs, outcomes, precheck)
    for k, o in enumerate(outcomes):
        g, p = w.who[k]
        text = cg.prove_outcome_text(o)
        assert (text == "") == (o.status == 0)
        if o.status:
            assert (bytes(proofs[k]) == ONES) and ("proof 0" in text)
    assert signature(proofs, outcomes) == want
    if transcript == "host" and not precheck:
        # the arrays the call took and the proofs it wrote go into the block verifier as they are
        vks = [cg.plonk_vk_upload(c.vk) for c in w.cases]
        try:
            g2h = cg.g2_generator()
            bh = cg.g2_mul(g2h, tau)
            handles = [vks[g] for g, _ in w.who]
            block_ok, each_ok = cg.plonk_verify_block(handles, g2h, bh, w.pub, proofs, w.msgs, each=True)
            assert [bool(e) for e in each_ok[:w.count]] == [o.status == 0 for o in outcomes]
            assert not block_ok
            good = [k for k, o in enumerate(outcomes) if o.status == 0]
            assert len(good) < w.count
            assert cg.plonk_verify_block([handles[k] for k in good], g2h, bh, w.pub[good], [proofs[k] for k in good],
                                         [w.msgs[k] for k in good])
        finally:
            for v in vks:
                cg.plonk_vk_release(v)


# ---- 4. input forms -----------------------------------------------------------------------------------------------------------
def test_from_coefficients(cg, world):
    w = world
    with modes(cg, "device", True):
        proofs, outcomes = cg.plonk_prove_notes(w.handles, w.wires("coeffs"), w.pub, w.bl, w.msgs, input_form="coeffs")
        want = w.per_group("coeffs")
    w.check(proofs, outcomes, True)
    assert signature(proofs, outcomes) == want


class VarsWorld:
    """the four circuits as variable-form keys of different num_vars (one of them odd), a few witnesses each - one of
    every key with a variable changed -, interleaved, every row of exact length and the last at the end of a mapping"""

    def __init__(self, cg, tau, world):
        self.cg = cg
        self.scs = [c.sc for c in world.cases]
        srs = [world.h1, world.h1, world.h1, world.h2]
        self.nvs = [sc.num_vars + extra for sc, extra in zip(self.scs, (0, 7, 2, 300))]
        if not any(nv % 2 for nv in self.nvs):
            self.nvs[1] += 1
        assert len(set(self.nvs)) == 4 and any(nv % 2 for nv in self.nvs)
        self.pks = [cg.plonk_preprocess_vars(h, sc.n, sc.num_inputs, sc.selectors_mont(), np.array(sc.wire_vars), nv)[0]
                    for h, sc, nv in zip(srs, self.scs, self.nvs)]
        self.P = 3
        self.group = []
        for gi, (sc, nv) in enumerate(zip(self.scs, self.nvs)):
            ws, vs, ps, bls = batch(sc, [700 + 10 * gi + i for i in range(self.P)], nv)
            vs = vs.copy()
            vs[1, int(sc.wire_vars[4][sc.n // 2]), 0] ^= np.uint64(1)  # the output of a gate row: witness 1 fails that gate
            self.group.append((ws, vs, ps, bls))
        self.who = [(k % 4, k // 4) for k in range(4 * self.P)]
        self.count = len(self.who)
        self.handles = [self.pks[g] for g, _ in self.who]
        self.nin = max(sc.num_inputs for sc in self.scs)
        self.pub = np.zeros((self.count, self.nin, 4), np.uint64)
        for k, (g, p) in enumerate(self.who):
            self.pub[k, :self.scs[g].num_inputs] = self.group[g][2][p]
        self.bl = np.stack([self.group[g][3][p] for g, p in self.who])
        self.msgs = [b"v%d" % k if k % 3 else None for k in range(self.count)]
        self.members = [[k for k, (g, _) in enumerate(self.who) if g == gi] for gi in range(4)]

    def free(self):
        for pk in self.pks:
            self.cg.plonk_free_key(pk)


@pytest.fixture(scope="module")
def vworld(cg, tau, world):
    v = VarsWorld(cg, tau, world)
    yield v
    v.free()


def vars_reference(cg, v):
    """one plonk_prove_each per group from variables -> signatures in note order; the unchanged witnesses' proofs are the
    evals-form lone proofs"""
    out = [None] * v.count
    for gi in range(4):
        ws, vs, ps, bls = v.group[gi]
        msgs = [v.msgs[k] for k in v.members[gi]]
        proofs, outcomes = cg.plonk_prove_each([v.pks[gi]] * v.P, vs, ps, bls, msgs, input_form="vars")
        for p, k in enumerate(v.members[gi]):
            if p != 1:
                assert outcomes[p].status == 0
                assert bytes(proofs[p]) == bytes(cg.plonk_prove(v.pks[gi], ws[p], ps[p], bls[p], msgs[p]))
            else:
                assert outcomes[p].status == ERR_PROOF and bytes(proofs[p]) == ONES
        sig = signature(proofs, outcomes)
        for p, k in enumerate(v.members[gi]):
            out[k] = sig[p]
    return out


@pytest.mark.parametrize("precheck", [False, True], ids=["nocheck", "precheck"])
def test_from_variables(cg, vworld, precheck):
    v = vworld
    rows, keep = [], []
    for g, p in v.who:
        r, m = at_end_of_a_mapping(v.group[g][1][p])  # exact length: a read past a note's own row leaves the mapping
        assert r.shape[0] == v.nvs[g]
        rows.append(r)
        keep.append(m)
    with modes(cg, "device", precheck):
        want = vars_reference(cg, v)
        proofs, outcomes = cg.plonk_prove_notes(v.handles, rows, v.pub, v.bl, v.msgs, input_form="vars")
    assert signature(proofs, outcomes) == want


# ---- 5. dealt, bound, ticket --------------------------------------------------------------------------------------------------
def test_dealt_bound_ticket_and_one_group(cg, world):
    w = world
    assert cg.device_count() >= 2
    wires = w.wires()
    with modes(cg, "device", False):
        want = w.per_group()
        s0 = cg.plonk_notes_stats()
        dealt = cg.plonk_prove_notes(w.handles, wires, w.pub, w.bl, w.msgs)
        d = delta(cg, s0)
        print("dealt", d)
        # min(groups, the parts a batch is dealt in): two per device by default, and no more than there are contexts
        devices = cg.physical_device_count()
        per = min(int(os.environ.get("CAPGPU_DEAL_PARTS_PER_DEVICE", "2")), max(cg.device_count() // devices, 1))
        assert d["groups"] == 4 and d["groups_dealt"] == 4 and d["contexts_dealt"] == min(4, cg.device_count(), devices * per)
        with bound(cg, 1):
            s0 = cg.plonk_notes_stats()
            on_one = cg.plonk_prove_notes(w.handles, wires, w.pub, w.bl, w.msgs)
            d = delta(cg, s0)
        assert d["groups"] == 4 and d["groups_dealt"] == 0 and d["contexts_dealt"] == 0
        half = w.count // 2
        t1 = cg.plonk_prove_notes_async(w.handles[:half], wires[:half], w.pub[:half], w.bl[:half], w.msgs[:half])
        t2 = cg.plonk_prove_notes_async(w.handles[half:], wires[half:], w.pub[half:], w.bl[half:], w.msgs[half:])
        (p1, o1), (p2, o2) = t1.wait(), t2.wait()
        # one group: one group reported, and capgpu_plonk_prove_each's bytes (rows of the call's own 27 inputs)
        c = w.cases[2]
        s0 = cg.plonk_notes_stats()
        one = cg.plonk_prove_notes([c.pk] * c.P, list(c.W), c.Pb, c.bl, c.msgs)
        d = delta(cg, s0)
        assert d["calls"] == 1 and d["groups"] == 1 and d["groups_dealt"] == 0
        each = cg.plonk_prove_each([c.pk] * c.P, c.W, c.Pb, c.bl, c.msgs)
        # ... and with rows longer than the group needs (re-packed)
        small = w.cases[0]
        wide = np.zeros((small.P, 5, 4), np.uint64)
        wide[:, :small.nin] = small.Pb
        one_wide = cg.plonk_prove_notes([small.pk] * small.P, list(small.W), wide, small.bl, small.msgs)
        each_small = cg.plonk_prove_each([small.pk] * small.P, small.W, small.Pb, small.bl, small.msgs)
    assert signature(*dealt) == want
    assert signature(*on_one) == want
    assert signature(p1 + p2, o1 + o2) == want
    assert signature(*one) == signature(*each)
    assert signature(*one_wide) == signature(*each_small)
    groups, group_of, num = cg.plonk_notes_plan(w.handles)
    assert num == 4 and group_of == [g for g, _ in w.who]
    P = [c.P for c in w.cases]
    assert [(g.srs_handle, g.domain_size, g.count, g.first, g.max_inputs) for g in groups] == [
        (w.h1, 16, P[0], 0, 1), (w.h1, 64, P[1], 1, 0), (w.h1, 512, P[2], 2, 27), (w.h2, 64, P[3], 3, 3)]
    # count * n descending, ties in group order
    weight = [P[0] * 16, P[1] * 64, P[2] * 512, P[3] * 64]
    order = sorted(range(4), key=lambda g: (-weight[g], g))
    assert [g.run_order for g in groups] == [order.index(g) for g in range(4)]


# ---- 6. device form -----------------------------------------------------------------------------------------------------------
def layouts(w, wires, rng):
    """-> {name: (buffer as a flat element array, offsets per note)} for (a) every group contiguous, (b) blocks shuffled
    with gaps, (c) the first two groups contiguous and the others shuffled"""
    sizes = [x.shape[0] * x.shape[1] if x.ndim == 3 else x.shape[0] for x in wires]  # elements per block
    out = {}
    for name in ("contiguous", "shuffled", "mixed"):
        order = []
        for gi in range(4):
            mem = list(w.members[gi])
            if name == "shuffled" or (name == "mixed" and gi >= 2):
                rng.shuffle(mem)
                if mem == sorted(mem):
                    mem.reverse()
            order.append(mem)
        if name != "contiguous":
            weave = lambda lists: [m[i] for i in range(max(map(len, lists))) for m in lists if i < len(m)]   # noqa: E731
            seq = order[0] + order[1] + weave(order[2:]) if name == "mixed" else weave(order)[::-1]
        else:
            seq = [k for mem in order for k in mem]
        offsets, at = [0] * w.count, 0
        for k in seq:
            gap = 0 if (name == "contiguous" or (name == "mixed" and w.who[k][0] < 2)) else int(rng.integers(1, 4))
            at += gap
            offsets[k] = at
            at += sizes[k]
        buf = np.full((at + 2, 4), 0xA5A5A5A5A5A5A5A5, np.uint64)
        for k in range(w.count):
            buf[offsets[k]:offsets[k] + sizes[k]] = wires[k].reshape(-1, 4)
        out[name] = (buf, offsets)
    return out


def test_device_form(cg, world):
    w = world
    wires = w.wires()
    lay = layouts(w, wires, np.random.default_rng(5))
    expect = {"contiguous": (4, 0, 0), "shuffled": (0, 4, w.count), "mixed": (2, 2, w.cases[2].P + w.cases[3].P)}
    with modes(cg, "device", False):
        want = signature(*cg.plonk_prove_notes(w.handles, wires, w.pub, w.bl, w.msgs))
        for name, (buf, offsets) in lay.items():
            d_buf = cg.DevBuf.from_numpy(buf)
            s0 = cg.plonk_notes_stats()
            got = cg.plonk_prove_notes_dev(w.handles, d_buf, offsets, w.pub, w.bl, w.msgs)
            d = delta(cg, s0)
            print(name, d)
            assert np.array_equal(d_buf.to_numpy(), buf.reshape(-1)), "the caller's buffer is never written"
            assert (d["dev_groups_direct"], d["dev_groups_gathered"], d["rows_gathered"]) == expect[name], name
            assert d["groups_dealt"] == 0
            assert signature(*got) == want, name
            if name == "shuffled":
                # a misaligned d_wires is refused
                with pytest.raises(cg.CapGpuError) as e:
                    cg.plonk_prove_notes_dev(w.handles, d_buf.ptr.value + 8, offsets, w.pub, w.bl, w.msgs)
                assert e.value.code == INVALID_ARG and "not 16-byte aligned" in str(e.value)
            d_buf.free()
    # precheck and compaction on: a gathered group drops its refused witnesses, the survivors' proofs are unchanged
    buf, offsets = lay["shuffled"]
    d_buf = cg.DevBuf.from_numpy(buf)
    old = cg.plonk_get_compaction()
    try:
        with modes(cg, "device", True):
            plain = cg.plonk_prove_notes_dev(w.handles, d_buf, offsets, w.pub, w.bl, w.msgs)
            cg.plonk_set_compaction(True)
            c0 = cg.plonk_compaction_stats()
            packed = cg.plonk_prove_notes_dev(w.handles, d_buf, offsets, w.pub, w.bl, w.msgs)
            c1 = cg.plonk_compaction_stats()
    finally:
        cg.plonk_set_compaction(old)
    bad = sum(len(c.bad) for c in w.cases)
    assert c1[0] - c0[0] == 4 and c1[1] - c0[1] == bad and c1[2] - c0[2] > 0
    assert np.array_equal(d_buf.to_numpy(), buf.reshape(-1))
    d_buf.free()
    w.check(*plain, True)
    for k in range(w.count):
        if plain[1][k].status == 0:
            assert bytes(packed[0][k]) == bytes(plain[0][k]) and packed[1][k].status == 0
        else:
            assert bytes(packed[0][k]) == ONES and packed[1][k].status == ERR_PROOF


def test_device_form_from_variables(cg, vworld):
    """variable form: a constant stride larger than the group's largest num_vars is proved where it lies; shuffled blocks
    of exact length, the last of which ends the buffer, are gathered"""
    v = vworld
    with modes(cg, "device", True):
        want = vars_reference(cg, v)
        for name in ("strided", "shuffled"):
            offsets, at = [0] * v.count, 0
            if name == "strided":
                for gi in range(4):
                    for k in v.members[gi]:
                        offsets[k] = at
                        at += v.nvs[gi] + 5
            else:
                for k in sorted(range(v.count), key=lambda k: (k * 7) % v.count, reverse=True):
                    offsets[k] = at
                    at += v.nvs[v.who[k][0]]
            buf = np.full((at, 4), 0x5A5A5A5A5A5A5A5A, np.uint64)
            for k, (g, p) in enumerate(v.who):
                buf[offsets[k]:offsets[k] + v.nvs[g]] = v.group[g][1][p]
            d_buf = cg.DevBuf.from_numpy(buf)
            s0 = cg.plonk_notes_stats()
            got = cg.plonk_prove_notes_dev(v.handles, d_buf, offsets, v.pub, v.bl, v.msgs, input_form="vars")
            d = delta(cg, s0)
            assert np.array_equal(d_buf.to_numpy(), buf.reshape(-1))
            d_buf.free()
            assert (d["dev_groups_direct"], d["dev_groups_gathered"]) == ((4, 0) if name == "strided" else (0, 4)), name
            assert signature(*got) == want, name


# ---- 8. arguments -------------------------------------------------------------------------------------------------------------
def raw(cg, w, kind="host", null="", **over):
    """one call through ctypes: null names the NULL pointers (h w x(offsets) p b r o t l), over replaces arguments"""
    L = cg.load()
    count = over.get("count", 4)
    k = max(count, 1)
    handles = (ctypes.c_uint64 * k)(*over.get("handles", w.handles[:k]))
    rows = [np.ascontiguousarray(x).reshape(-1) for x in w.wires()[:k]]
    ptrs = (ctypes.c_void_p * k)(*[r.ctypes.data for r in rows])
    if "row" in over:
        ptrs[over["row"]] = None
    pub, bl = np.ascontiguousarray(w.pub[:k]).reshape(-1), np.ascontiguousarray(w.bl[:k]).reshape(-1)
    msgs = (ctypes.c_char_p * k)(*[w.msgs[i] for i in range(k)])
    lens = (ctypes.c_size_t * k)(*[len(w.msgs[i] or b"") for i in range(k)])
    proofs, outcomes, ticket = (cg.Proof * k)(), (cg.ProveOutcome * k)(), ctypes.c_uint64(7)
    N = lambda c, x: None if c in null else x                                       # noqa: E731
    args = [N("h", handles), count]
    dbuf = None
    if kind == "dev":
        flat = np.concatenate(rows)
        dbuf = cg.DevBuf.from_numpy(flat)
        offs = (ctypes.c_uint64 * k)(*np.cumsum([0] + [r.size // 4 for r in rows[:-1]]).tolist())
        args += [N("w", ctypes.c_void_p(dbuf.ptr.value + over.get("misalign", 0))), N("x", offs)]
    else:
        args += [N("w", ptrs)]
    args += [N("p", cg._p(pub)), ctypes.c_size_t(over.get("nin", w.nin)), msgs, N("l", lens), N("b", cg._p(bl)),
             ctypes.c_int(over.get("form", 0)), N("r", proofs), N("o", outcomes)]
    if kind == "async":
        args.append(N("t", ctypes.byref(ticket)))
    name = {"host": NOTES, "dev": NOTES + "_dev", "async": NOTES + "_async"}[kind]
    rc = getattr(L, name)(*args)
    err = L.capgpu_last_error().decode() if rc else ""
    if kind == "async" and rc == OK and "t" not in null and ticket.value:
        done = ctypes.c_int(0)
        assert L.capgpu_wait(ticket, ctypes.c_uint32(0xFFFFFFFF), ctypes.byref(done)) == OK and done.value == 1
    if dbuf:
        dbuf.free()
    print(kind, null, {k_: v for k_, v in over.items() if k_ != "handles"}, "->", rc, repr(err))
    return rc, err, proofs, outcomes


def test_arguments(cg, world, tau):
    w = world
    BADARG = NOTES + ": bad argument"
    FORM7 = "capgpu_plonk: input_form 7 is none of"
    for kind in ("host", "dev", "async"):
        pointers = "hwpbro" + ("x" if kind == "dev" else "") + ("t" if kind == "async" else "") + "l"
        for c in pointers:
            rc, err, _, _ = raw(cg, w, kind, null=c)
            assert rc == INVALID_ARG and err.startswith(BADARG), (kind, c)
        assert raw(cg, w, kind, count=-1)[:2] == (INVALID_ARG, BADARG)
        # the order: form < pointers < rows / alignment < count == 0 < keys < row length
        rc, err, _, _ = raw(cg, w, kind, null="b", form=7)
        assert rc == INVALID_ARG and err.startswith(FORM7)
        bad_h = [UNKNOWN] + w.handles[1:4]
        if kind != "dev":
            rc, err, _, _ = raw(cg, w, kind, row=2)
            assert rc == INVALID_ARG and err.startswith(NOTES + ": wires[2] is NULL")
            rc, err, _, _ = raw(cg, w, kind, row=2, null="o")
            assert rc == INVALID_ARG and err.startswith(BADARG)
            rc, err, _, _ = raw(cg, w, kind, row=2, handles=bad_h)
            assert rc == INVALID_ARG and err.startswith(NOTES + ": wires[2] is NULL")
        else:
            rc, err, _, _ = raw(cg, w, kind, misalign=8, handles=bad_h)
            assert rc == INVALID_ARG and "not 16-byte aligned" in err
            rc, err, _, _ = raw(cg, w, kind, misalign=8, null="x")
            assert rc == INVALID_ARG and err.startswith(BADARG)
        rc, err, _, _ = raw(cg, w, kind, handles=bad_h)
        assert rc == BAD_HANDLE and err.startswith("capgpu: unknown proving key handle 999999")
        rc, err, _, _ = raw(cg, w, kind, handles=bad_h, nin=w.nin - 1)   # the keys before the row length
        assert rc == BAD_HANDLE
        rc, err, _, _ = raw(cg, w, kind, handles=w.handles[:3] + [UNKNOWN], form=2)   # note 0's missing table before note 3's handle
        assert rc == INVALID_ARG and err.startswith("capgpu_plonk: CAPGPU_INPUT_VARS: key has no variable table")
        rc, err, _, _ = raw(cg, w, kind, nin=w.nin - 1)
        assert rc == INVALID_ARG and err.startswith(NOTES + ": rows of 26 public inputs given, the keys need 27")
        # count == 0: CAPGPU_OK, nothing written - whatever else is wrong behind the pointer checks
        rc, err, proofs, outcomes = raw(cg, w, kind, count=0, handles=[UNKNOWN], nin=0)
        assert rc == OK and bytes(proofs[0]) == bytes(len(ONES)) and outcomes[0].status == 0
        rc, err, proofs, outcomes = raw(cg, w, kind)
        assert rc == OK
        for k in range(4):
            g, p = w.who[k]
            assert (outcomes[k].status == 0) == (w.cases[g].exp[p][0] == 0)
            if outcomes[k].status == 0:
                assert bytes(proofs[k]) == w.cases[g].lone[p]
    # a key of the reference-schedule test mode (the environment is read when a key is made) is refused, after an unknown
    # handle in front of it and before one behind it
    c = w.cases[0]
    os.environ["CAPGPU_RECOMPUTE_PK_COSET"] = "1"
    try:
        rk, _ = cg.plonk_preprocess(w.h1, c.sc.n, c.nin, c.sc.selectors_mont(), c.sc.sigma_mont())
    finally:
        del os.environ["CAPGPU_RECOMPUTE_PK_COSET"]
    try:
        for kind in ("host", "dev", "async"):
            rc, err, _, _ = raw(cg, w, kind, handles=[w.handles[0], w.handles[1], rk, UNKNOWN])
            assert rc == INVALID_ARG and err.startswith(NOTES + ": the key of note 2 re-transforms its columns")
            rc, err, _, _ = raw(cg, w, kind, handles=[w.handles[0], UNKNOWN, rk, w.handles[3]])
            assert rc == BAD_HANDLE
    finally:
        cg.plonk_free_key(rk)
    groups, group_of, num = cg.plonk_notes_plan(w.handles, cap=2)
    assert num == 4 and len(groups) == 2 and [g.domain_size for g in groups] == [16, 64] and len(group_of) == w.count
    groups, group_of, num = cg.plonk_notes_plan(w.handles, cap=0)
    assert num == 4 and groups == []
    with pytest.raises(cg.CapGpuError) as e:
        cg.plonk_notes_plan([UNKNOWN])
    assert e.value.code == BAD_HANDLE
    assert cg.plonk_notes_plan([]) == ([], [], 0)


def test_refused_while_sharding(cg, world):
    """capgpu_plonk_shard_msm on (a loopback world of two ranks): the three calls are refused, behind the pointer checks
    and count == 0, before the keys are looked at"""
    w = world
    assert cg.comm_info() == (0, 0)
    cg.comm_init_loopback(2)
    try:
        cg.plonk_shard_msm(True)
        for kind in ("host", "dev", "async"):
            rc, err, _, _ = raw(cg, w, kind, handles=[UNKNOWN] + w.handles[1:4])
            assert rc == INVALID_ARG and err.startswith(NOTES + ": not available while capgpu_plonk_shard_msm is on")
            assert raw(cg, w, kind, null="b")[1].startswith(NOTES + ": bad argument")
            assert raw(cg, w, kind, count=0)[0] == OK
    finally:
        cg.plonk_shard_msm(False)
        cg.comm_destroy()


# ---- 9. reserve ---------------------------------------------------------------------------------------------------------------
def test_reserve(cg, world):
    w = world
    wires = w.wires()
    buf, offsets = layouts(w, wires, np.random.default_rng(6))["shuffled"]
    d_buf = cg.DevBuf.from_numpy(buf)
    try:
        with modes(cg, "device", False):
            # sanity: on a trimmed library the counter sees this path
            cg.trim()
            e0 = cg.scratch_stats()["grow_events"]
            cg.plonk_prove_notes(w.handles, wires, w.pub, w.bl, w.msgs)
            assert cg.scratch_stats()["grow_events"] > e0
            cg.trim()
            e0 = cg.scratch_stats()["grow_events"]
            cg.plonk_prove_notes_dev(w.handles, d_buf, offsets, w.pub, w.bl, w.msgs)
            assert cg.scratch_stats()["grow_events"] > e0
            cg.trim()
            cg.plonk_reserve_notes(w.handles, slot=-1)
            e0 = cg.scratch_stats()["grow_events"]
            host = cg.plonk_prove_notes(w.handles, wires, w.pub, w.bl, w.msgs)
            e1 = cg.scratch_stats()["grow_events"]
            dev = cg.plonk_prove_notes_dev(w.handles, d_buf, offsets, w.pub, w.bl, w.msgs)
            e2 = cg.scratch_stats()["grow_events"]
            print("grow events", e0, e1, e2)
            assert e1 == e0, "the host-form call grew scratch after the reserve"
            assert e2 == e1, "the device-form call grew scratch after the reserve"
            assert signature(*host) == signature(*dev)
    finally:
        d_buf.free()


# ---- 10. on a caller's stream -------------------------------------------------------------------------------------------------
def test_on_a_callers_stream(cg, world):
    """the device form behind a producer that is still writing the buffer when the call is made: the gather and the
    provers run on the caller's stream, so they see the producer's bytes"""
    import torch
    w = world
    wires = w.wires()
    buf, offsets = layouts(w, wires, np.random.default_rng(7))["mixed"]
    with modes(cg, "device", False):
        want = signature(*cg.plonk_prove_notes(w.handles, wires, w.pub, w.bl, w.msgs))
        src = torch.from_numpy(buf.view(np.int64).reshape(-1)).cuda()
        dst = torch.zeros_like(src)
        spin = torch.zeros(1 << 24, device="cuda")
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for _ in range(20):          # work ahead of the producer's copy: the buffer is still zeros when the call is made
                spin.add_(1.0)
            dst.copy_(src, non_blocking=True)
            with cg.on_stream(stream.cuda_stream):
                got = cg.plonk_prove_notes_dev(w.handles, dst.data_ptr(), offsets, w.pub, w.bl, w.msgs)
        stream.synchronize()
    assert signature(*got) == want
    assert torch.equal(dst, src)
