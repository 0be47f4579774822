"""The solver's DEFERRED form on the device (capgpu_plonk_key_set_solve_form): the variables of OUT rows with q_ecc carried as
pairs (numerator, denominator) and a chain's denominators inverted together by flush items.  The form gives the same words
and the same statuses: vars_out must equal tests/solve_io_model.walk_io - the rule in Python integers - AND the same key
solved in the DIRECT form on the device, word for word; the info figures must equal tests/solve_defer_model.py."""
import numpy as np
import pytest

from cap_amd import bench_utils as bu
from cap_amd.io_model import cap_like_io_circuit
from cap_amd.lib import SOLVE_FORM_DEFERRED, SOLVE_FORM_DIRECT, SOLVER_DERIVE_PUBLIC, SOLVER_LINEAR
from tests.solve_defer_model import GROUP, defer_model
from tests.solve_io_model import pub_inputs_of, walk_io
from tests.test_gpu_prove_each import bound, modes, signature
from tests.test_gpu_solve import (Q_C, Q_ECC, Q_HASH, Q_LC, Q_MUL, Q_O, given_values, key_for, mont_rows, solve_host_and_dev,
                                  status_tuples)
from tests.test_gpu_solve_hints import HBuilder

pytestmark = pytest.mark.gpu

R = bu.R
BOTH = SOLVER_LINEAR | SOLVER_DERIVE_PUBLIC
EDGES = (0, 1, R - 1, 1 << 253, None)
NO_HASH = [Q_LC, Q_LC + 1, Q_LC + 2, Q_LC + 3, Q_MUL, Q_MUL + 1, Q_C, Q_O, Q_ECC]


class ChainHand:
    """Two public inputs (variables 2 and 3; 3 is derived).  A chain of 12 additions - two OUT_INV rows each over the cells
    (x, y, qx, qy), every third one a doubling (x, y, x, y) - with a select (an OUT_MUL row on pending inputs) and a linear row
    between them; a Rescue-style row that raises the chain's x to the fifth power (flush 1); a chain of 4 behind it; a BITS hint
    and an is_zero gadget on its last addition's outputs (flush 2); one more addition whose outputs a ROOT5 row and the LIN
    equality row of public input 1 read (flush 3).  No row of a chain has a q_hash."""
    FLUSHES = 3

    def __init__(self, log_n=9, seed=91):
        b = self.b = HBuilder(log_n, 2, seed)
        b.given = [0, 1, 2]
        self.e = b.var(given=True)                                         # the edge values: a summand of every linear row
        self.adds = []                                                     # (row of x3, row of y3, qx, qy) per addition
        x, y = b.var(given=True), b.var(given=True)
        x, y = self.chain(x, y, 12)
        self.x1 = x
        h = b.var()
        b.row([x, b.var(given=True), 0, 0, h], **b.rand_sels([Q_HASH, Q_LC + 1, Q_O]))     # x^5: a pending variable on a hash cell
        x, y = self.chain(h, y, 4, last_plain=True)
        self.bits, _ = b.unpack(x, 254)                                    # BITS on a pending source ...
        self.inv, self.flag = b.is_zero(y)                                 # ... INV0 and ISZERO on another
        x, y = self.add(x, y, b.var(given=True), b.var(given=True))
        g = [b.var(given=True) for _ in range(4)]
        self.root, _ = b.root(g, 1, x)                                     # ROOT5 with a pending variable on wire 4
        b.row([y, 3, 0, 0, 0], **{f"s{Q_LC}": 1, f"s{Q_LC + 1}": -1})      # public input 1 = y, by a LIN row
        self.y_last = y
        self.sc, self.given, self.hints = b.finish(), b.given, b.hints

    def add(self, x, y, qx, qy):
        b = self.b
        x3, y3 = b.var(), b.var()
        rx = b.row([x, y, qx, qy, x3], **b.rand_sels(NO_HASH))
        ry = b.row([x, y, qx, qy, y3], **b.rand_sels(NO_HASH))
        self.adds.append((rx, ry, qx, qy))
        return x3, y3

    def chain(self, x, y, count, last_plain=False):
        b = self.b
        for k in range(count):
            qx, qy = (x, y) if k % 3 == 2 else (b.var(given=True), b.var(given=True))
            x3, y3 = self.add(x, y, qx, qy)
            if last_plain and k == count - 1:
                return x3, y3                                              # the addition's own outputs
            s = b.var()
            b.row([x3, y3, b.var(given=True), 0, s], **b.rand_sels([Q_MUL, Q_LC + 2, Q_O]))   # a select: OUT_MUL on pending inputs
            t, _ = b.lin([s, y3, self.e], [b.rng.field() | 1 for _ in range(3)])
            x, y = s, t
        return x, y

    def vanish(self, v, row, own):
        """the given value of variable `own`, which this row alone reads, at which its denominator is 0"""
        sc, at = self.sc, {g: k for k, g in enumerate(self.given)}
        vals = walk_io(sc, self.given, v, self.hints, BOTH)[0]
        w = [vals[sc.wire_vars[i][row]] for i in range(4) if sc.wire_vars[i][row] != own]
        assert len(w) == 3 and all(w), "a zero among the row's other cells"
        sel = sc.selectors
        v[at[own]] = sel[Q_O][row] * pow(sel[Q_ECC][row] * w[0] * w[1] * w[2] % R, R - 2, R) % R

    def values(self, count=5):
        at = {g: k for k, g in enumerate(self.given)}
        vals = given_values(self.sc, self.given, count, 29)
        for p in range(count):
            if EDGES[p % 5] is not None:
                vals[p][at[self.e]] = EDGES[p % 5]
        if count > 2:   # witness 2: the x row of addition 6 - the MIDDLE of the first chain - has a zero denominator
            self.vanish(vals[2], self.adds[6][0], self.adds[6][2])
        if count > 4:   # witness 4: that row and, further down, the y row of addition 9: the lower row is reported
            self.vanish(vals[4], self.adds[6][0], self.adds[6][2])
            self.vanish(vals[4], self.adds[9][1], self.adds[9][3])
        return vals


@pytest.fixture(scope="module")
def ch(cg, tau):
    c = ChainHand()
    c.h, c.pk, c.vk = key_for(cg, tau, c.sc)
    c.vals = c.values()
    c.want = [walk_io(c.sc, c.given, v, c.hints, BOTH) for v in c.vals]    # computed once, shared, left unchanged
    c.pubs = [pub_inputs_of(c.sc, w[0]) for w in c.want]
    c.model = defer_model(c.sc, c.given, c.hints, BOTH)
    yield c
    cg.plonk_free_key(c.pk)
    cg.srs_free(c.h)


def set_up(cg, c, form=SOLVE_FORM_DEFERRED):
    cg.plonk_key_set_solver(c.pk, c.given, c.hints, BOTH)
    return cg.plonk_key_set_solve_form(c.pk, form)


# ---- 1. the chain circuit against the model and against the direct form, by every entry point, form and width ----------------
@pytest.mark.parametrize("pack", [0, 1, 2, 16])
def test_chain_circuit_equals_the_model_and_the_direct_form(cg, ch, pack):
    c = ch
    assert [w[1] for w in c.want] == [(0, 0), (0, 0), (1, c.adds[6][0]), (0, 0), (1, c.adds[6][0])]
    assert c.adds[6][0] < c.adds[9][1] and c.want[4][0][c.sc.wire_vars[4][c.adds[9][1]]] == 0    # both rows left a 0
    assert [w[0][c.e] for w in c.want][:4] == [0, 1, R - 1, 1 << 253]
    rows = [p % 5 for p in range(17)]
    gv17, want17 = mont_rows([c.vals[p] for p in rows]), mont_rows([c.want[p][0] for p in rows])
    old_pack, old_form = cg.plonk_get_solve_pack(), cg.fr_get_inverse_form()
    cg.plonk_set_solve_pack(pack)
    try:
        for form in ("fermat", "gcd"):
            cg.fr_set_inverse_form(form)
            for count in (1, 3, 17):
                gv = np.ascontiguousarray(gv17[:count])
                assert set_up(cg, c, SOLVE_FORM_DIRECT).form == SOLVE_FORM_DIRECT
                direct, st_direct = solve_host_and_dev(cg, c.pk, gv)
                assert set_up(cg, c).form == SOLVE_FORM_DEFERRED
                got, st = solve_host_and_dev(cg, c.pk, gv)
                assert np.array_equal(got, want17[:count]), (form, count)
                assert np.array_equal(got, direct), (form, count)
                assert status_tuples(st) == status_tuples(st_direct) == [c.want[p][1] for p in rows[:count]], (form, count)
                pubs = cg.plonk_pub_inputs(c.pk, got, count)
                assert np.array_equal(pubs, mont_rows([c.pubs[p] for p in rows[:count]])), (form, count)
    finally:
        cg.plonk_set_solve_pack(old_pack)
        cg.fr_set_inverse_form(old_form)


# ---- 2. the figures ------------------------------------------------------------------------------------------------------------
def test_info_figures_equal_the_model(cg, ch):
    c, m = ch, ch.model
    solver = cg.plonk_key_set_solver(c.pk, c.given, c.hints, BOTH)
    assert cg.plonk_key_solve_form_info(c.pk).as_dict() == m["info_direct"]
    info = cg.plonk_key_set_solve_form(c.pk, SOLVE_FORM_DEFERRED)
    assert info.as_dict() == cg.plonk_key_solve_form_info(c.pk).as_dict() == m["info_deferred"]
    # the other info calls keep reporting the direct plan
    assert cg.plonk_key_solver_info(c.pk).as_dict() == solver[0].as_dict() == c.want[0][2]
    assert cg.plonk_key_hint_info(c.pk).as_dict() == solver[1].as_dict() == c.want[0][3]
    assert cg.plonk_key_solver_rules_info(c.pk).as_dict() == c.want[0][4]
    # 17 additions, a level each - the INV0 item stands in the last addition's level; three flushes were built in, none is
    # left for the end
    inv0_levels = 1
    assert info.inv_levels_direct == 17 and info.inv_levels_direct >= 16
    assert info.flush_levels == c.FLUSHES and m["flush_before"][-1] < info.levels - info.flush_levels
    assert info.inv_levels_deferred == c.FLUSHES + inv0_levels
    assert info.levels == solver[0].levels + info.flush_levels
    # every row with q_ecc is a fraction row, and the chains' selects (12 + 3) and linear rows (11 + 3: the first chain's last
    # one stands in the level of the Rescue row, behind flush 1)
    assert info.frac_rows == info.deferred_vars == len(m["deferred"]) == 2 * 17 + 15 + 14
    assert any(mask & (mask >> 2) & 3 == 3 for mask in m["masks"].values())          # a doubling: both pairs pending
    assert info.flush_items == sum((s + GROUP - 1) // GROUP for s in m["flush_sizes"]) == 4 and max(m["flush_sizes"]) > GROUP
    assert cg.plonk_key_set_solve_form(c.pk, SOLVE_FORM_DIRECT).as_dict() == m["info_direct"]


# ---- 3. the form's lifetime ----------------------------------------------------------------------------------------------------
def test_the_form_is_per_key_and_every_set_up_call_resets_it(cg, tau, ch):
    c = ch
    gv = mont_rows(c.vals[:3])
    want = mont_rows([w[0] for w in c.want[:3]])

    def solves(deferred):
        f0 = cg.plonk_key_solve_form_info(c.pk).form
        got, st = cg.plonk_solve_vars(c.pk, gv, 3)
        assert np.array_equal(got, want) and status_tuples(st) == [w[1] for w in c.want[:3]]
        assert f0 == (SOLVE_FORM_DEFERRED if deferred else SOLVE_FORM_DIRECT)

    def moved():
        s0 = cg.plonk_solve_stats()
        cg.plonk_solve_vars(c.pk, gv, 3)
        s1 = cg.plonk_solve_stats()
        return {k: s1[k] - s0[k] for k in s0}

    set_up(cg, c, SOLVE_FORM_DIRECT)
    as_direct = moved()
    assert as_direct["launches"] == 1 and as_direct["witnesses"] == 3
    set_up(cg, c)
    solves(True)
    assert moved() == as_direct                                            # the counters do not know of the form
    # a second key of the same circuit stays DIRECT
    h2, pk2, _ = key_for(cg, tau, c.sc)
    cg.plonk_key_set_solver(pk2, c.given, c.hints, BOTH)
    assert cg.plonk_key_solve_form_info(pk2).form == SOLVE_FORM_DIRECT and cg.plonk_key_solve_form_info(c.pk).form == SOLVE_FORM_DEFERRED
    # a key without a solver is refused and reports zeros
    h3, pk3, _ = key_for(cg, tau, c.sc)
    assert cg.plonk_key_solve_form_info(pk3).as_dict() == cg.SolveFormInfo().as_dict()
    with pytest.raises(cg.CapGpuError) as e:
        cg.plonk_key_set_solve_form(pk3, SOLVE_FORM_DEFERRED)
    assert e.value.code == -1 and "capgpu_plonk_key_set_solve_form: the key has no solver" in str(e.value)
    assert "the key is unchanged" in str(e.value)
    for pk, h in ((pk2, h2), (pk3, h3)):
        cg.plonk_free_key(pk)
        cg.srs_free(h)
    # refusals leave the key solving as before, in the form it had
    for form in (2, -1):
        with pytest.raises(cg.CapGpuError) as e:
            cg.plonk_key_set_solve_form(c.pk, form)
        assert e.value.code == -1 and "capgpu_plonk_key_set_solve_form: bad argument (form" in str(e.value)
        solves(True)
    with pytest.raises(cg.CapGpuError):                                    # a refused set-up call keeps schedule and form
        cg.plonk_key_set_solver(c.pk, c.given, c.hints, 0)
    solves(True)
    # set_solve_form(DIRECT) gives back the direct schedule ...
    cg.plonk_key_set_solve_form(c.pk, SOLVE_FORM_DIRECT)
    solves(False)
    # ... and so does every older set-up call
    cg.plonk_key_set_solve_form(c.pk, SOLVE_FORM_DEFERRED)
    cg.plonk_key_set_solver(c.pk, c.given, c.hints, BOTH)
    solves(False)
    assert moved() == as_direct
    cg.plonk_key_set_solve_form(c.pk, SOLVE_FORM_DEFERRED)
    cg.plonk_key_set_vars(c.pk, np.array(c.sc.wire_vars), c.sc.num_vars)   # the table leaves, and the solver with it
    assert cg.plonk_key_solve_form_info(c.pk).as_dict() == cg.SolveFormInfo().as_dict()
    # the two calls that cannot take this circuit (no flags) on one they can: a deferred key comes back DIRECT
    b = HBuilder(9, 1, 5)
    g = [b.var(given=True) for _ in range(4)]
    u, _ = b.out(g, ecc=True)
    b.out([u, g[0], g[1], g[2]], ecc=True)
    sc = b.finish()
    h4, pk4, _ = key_for(cg, tau, sc)
    for call in (lambda: cg.plonk_key_set_given(pk4, b.given), lambda: cg.plonk_key_set_given_hints(pk4, b.given, [])):
        call()
        assert cg.plonk_key_set_solve_form(pk4, SOLVE_FORM_DEFERRED).flush_levels >= 1
        call()
        assert cg.plonk_key_solve_form_info(pk4).form == SOLVE_FORM_DIRECT
    cg.plonk_free_key(pk4)
    cg.srs_free(h4)


# ---- 4. proving ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transcript", ["host", "device"])
def test_prove_given_io_on_a_deferred_key_is_the_direct_keys(cg, tau, ch, transcript):
    c = ch
    picked = [0, 1, 3]                                                     # the witnesses without a zero denominator
    gv = mont_rows([c.vals[p] for p in picked])
    bls = np.stack([bu.to_mont_array(bu.blinders(5100 + p)) for p in range(3)])
    msgs = [b"defer-0", None, b"defer-2"]
    pks = [c.pk] * 3
    with modes(cg, transcript, False), bound(cg, 0):
        set_up(cg, c, SOLVE_FORM_DIRECT)
        want = cg.plonk_prove_given_io(pks, gv, bls, msgs)
        set_up(cg, c)
        sync = cg.plonk_prove_given_io(pks, gv, bls, msgs)
        t1 = cg.plonk_prove_given_io_async(pks, gv, bls, msgs)             # two tickets in flight
        t2 = cg.plonk_prove_given_io_async(pks, gv, bls, msgs)
        tick1, tick2 = t1.wait(), t2.wait()
    assert [o.status for o in want[1]] == [0] * 3 and status_tuples(want[2]) == [(0, 0)] * 3
    assert np.array_equal(want[3], mont_rows([c.pubs[p] for p in picked]))   # the model's public inputs
    for name, (proofs, outcomes, solved, pubs) in (("sync", sync), ("async 1", tick1), ("async 2", tick2)):
        assert signature(proofs, outcomes) == signature(want[0], want[1]), name
        assert [bytes(p) for p in proofs] == [bytes(p) for p in want[0]], name
        assert status_tuples(solved) == status_tuples(want[2]), name
        assert np.array_equal(pubs, want[3]), name
    g2h = cg.g2_generator()
    bh = cg.g2_mul(g2h, tau)
    for i in range(3):
        assert cg.plonk_verify(c.vk, g2h, bh, sync[3][i], sync[0][i], msgs[i]), i


# ---- 5. scratch -------------------------------------------------------------------------------------------------------------------
def test_a_reserved_deferred_key_allocates_nothing(cg, ch):
    c = ch
    gv = mont_rows([c.vals[p] for p in (0, 1, 3)])
    pubs = mont_rows([c.pubs[p] for p in (0, 1, 3)])
    bls = np.stack([bu.to_mont_array(bu.blinders(5200 + p)) for p in range(3)])
    with modes(cg, "device", False), bound(cg, 0):
        set_up(cg, c)
        cg.trim()
        s0 = cg.scratch_stats()
        cg.plonk_reserve_given(c.pk, 3, 0)
        before = cg.scratch_stats()
        assert before["grow_events"] > s0["grow_events"]                   # capgpu_scratch_stats counts what the reserve grew
        first = cg.plonk_prove_given([c.pk] * 3, gv, pubs, bls)
        again = cg.plonk_prove_given([c.pk] * 3, gv, pubs, bls)
        after = cg.scratch_stats()
    assert after["grow_events"] - before["grow_events"] == 0, (before, after)
    assert [o.status for o in first[1]] == [0] * 3 and signature(first[0], first[1]) == signature(again[0], again[1])


def test_reserve_given_sizes_the_side_buffer(cg, ch):
    """What the form adds to a reserve on a trimmed context: 64 bytes per witness and deferred slot - at least that, and,
    with the carver's 256-byte alignment and the 25 % a growing buffer may add, less than twice that."""
    c = ch
    count, side = 64, 64 * 64 * c.model["slots"]

    def grown(form):
        set_up(cg, c, form)
        cg.trim()
        s0 = cg.scratch_stats()
        cg.plonk_reserve_given(c.pk, count, 0)
        return cg.scratch_stats()["grow_bytes"] - s0["grow_bytes"]

    grown(SOLVE_FORM_DIRECT)                                               # (the first reserve brings the key's tables)
    direct, deferred = grown(SOLVE_FORM_DIRECT), grown(SOLVE_FORM_DEFERRED)
    assert direct > 0 and side <= deferred - direct < 2 * side, (direct, deferred, side)


# ---- 6. the transfer model at its own size -----------------------------------------------------------------------------------------
def test_io_transfer_model_deferred_equals_direct(cg, tau):
    """cap_like_io_circuit('transfer_2x2'), n = 2^15: the only place the wide flush - thousands of variables - is met"""
    sc, given, hints = cap_like_io_circuit("transfer_2x2")
    gv = mont_rows([bu.cap_like_given_values(sc, s) for s in (11, 12, 13)])
    m = defer_model(sc, given, hints, BOTH)
    h, pk, _ = key_for(cg, tau, sc)
    cg.plonk_key_set_solver(pk, given, hints, BOTH)
    assert cg.plonk_key_solve_form_info(pk).as_dict() == m["info_direct"]
    d_g = cg.DevBuf.from_numpy(gv)
    d_v, st = cg.plonk_solve_vars(pk, d_g, 3)
    direct = d_v.to_numpy().reshape(3, sc.num_vars, 4)
    d_v.free()
    info = cg.plonk_key_set_solve_form(pk, SOLVE_FORM_DEFERRED)
    assert info.as_dict() == m["info_deferred"]
    assert max(m["flush_sizes"]) > 1000 and info.inv_levels_deferred < info.inv_levels_direct
    d_v, st2 = cg.plonk_solve_vars(pk, d_g, 3)
    deferred = d_v.to_numpy().reshape(3, sc.num_vars, 4)
    assert status_tuples(st) == status_tuples(st2) == [(0, 0)] * 3
    assert np.array_equal(deferred, direct)
    d_p = cg.plonk_pub_inputs(pk, d_v, 3)
    cg.sync_all()
    pubs = d_p.to_numpy().reshape(3, 27, 4)
    assert [f.kind for f in cg.plonk_check_witness_batch(pk, d_v, pubs, 3, input_form="vars")] == [0, 0, 0]
    for d in (d_g, d_v, d_p):
        d.free()
    cg.plonk_free_key(pk)
    cg.srs_free(h)
