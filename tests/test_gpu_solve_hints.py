"""Solver hints on the device (capgpu_plonk_key_set_given_hints): bits, inverses and zero flags computed in the solver's own
kernel from a source variable, so that circuits which lay unpack / is_zero / is_equal on COMPUTED values follow from their
inputs alone.  tests/solve_hints_model.py is the rule in Python integers - the definition; vars_out must equal it word for
word.  The completed buffer is a CAPGPU_INPUT_VARS witness: checked and proved in place."""
import ctypes

import numpy as np
import pytest

from cap_amd import bench_utils as bu
from cap_amd.lib import HINT_BITS, HINT_INV0, HINT_ISZERO
from tests.solve_hints_model import walk_hints
from tests.test_gpu_solve import (Builder, Q_C, Q_ECC, Q_LC, Q_MUL, Q_O, given_values, key_for, mont_rows, solve_host_and_dev,
                                  status_tuples, walk)

pytestmark = pytest.mark.gpu

R = bu.R


# ---- the hinted gadgets on tests/test_gpu_solve.py's Builder (variable 0 holds 0, variable 1 holds 1) -------------------
class HBuilder(Builder):
    def __init__(self, log_n, num_inputs, seed):
        super().__init__(log_n, num_inputs, seed)
        self.hints = []

    def lin(self, ids, coeffs, out=None):
        """out = sum coeffs_i ids_i: an OUT row, or - out an existing variable - a constraint; -> (out, row)"""
        ids = list(ids) + [0] * (4 - len(ids))
        out = self.var() if out is None else out
        sels = {f"s{Q_LC + i}": c for i, c in enumerate(coeffs)}
        return out, self.row(ids + [out], **sels, **{f"s{Q_O}": 1})

    def booleans(self, bits):
        for b in bits:
            self.row([b, b, 0, 0, b], **{f"s{Q_MUL}": 1, f"s{Q_O}": 1})

    def unpack(self, v, nbits, close=True):
        """nbits hinted bits of v on wires 0, 1 and 4 of their boolean rows; the recomposition chain, three bits a row, the
        running sum on wire 3, whose last row outputs v itself -> (bits, the closing row)"""
        bits = [self.var() for _ in range(nbits)]
        self.hints.append((HINT_BITS, v, bits))
        self.booleans(bits)
        acc, row = 0, None
        for k in range(0, nbits if close else 0, 3):
            grp = bits[k:k + 3]
            acc, row = self.lin(grp + [0] * (3 - len(grp)) + [acc], [1 << (k + i) for i in range(len(grp))] + [0] * (3 - len(grp)) + [1],
                                out=v if k + 3 >= nbits else None)
        return bits, row

    def is_zero(self, a):
        inv, y = self.var(), self.var()
        self.hints.append((HINT_INV0, a, [inv]))
        self.hints.append((HINT_ISZERO, a, [y]))
        self.row([a, inv, 0, 0, y], **{f"s{Q_MUL}": 1, f"s{Q_C}": -1, f"s{Q_O}": -1})      # y = 1 - a a_inv
        self.row([a, y, 0, 0, 0], **{f"s{Q_MUL}": 1, f"s{Q_O}": 1})                        # a y = 0
        return inv, y

    def is_equal(self, a, b):
        d, _ = self.lin([a, b], [1, -1])
        return self.is_zero(d)


class Hand:
    """Test 1's circuit, n = 2^9.  Every hint source is the output of an OUT row."""

    def __init__(self):
        b = self.b = HBuilder(9, 2, 41)
        g = self.g = [b.var(given=True) for _ in range(12)]
        x, _ = b.lin([g[0], g[1]], [1, 1])                       # two values below 128: x < 256
        self.x_bits, self.x_close = b.unpack(x, 8)
        full, _ = b.lin([g[2]], [1])                             # a full-width value: 0, 1, r - 1, 2^253, random
        self.full = full
        self.full_bits, _ = b.unpack(full, 254)                  # is_in_range(full, 254): eight chunks, the last of 30 bits
        d, _ = b.lin([g[3], g[4]], [1, -1])
        self.d_inv, self.d_zero = b.is_zero(d)
        a, _ = b.lin([g[5], g[6]], [3, 1])
        c, _ = b.lin([g[7]], [1])
        _, self.eq = b.is_equal(a, c)
        inv, _ = b.is_zero(full)                                 # an INV0 whose target feeds a BITS hint: the low 17 bits of
        self.inv17, _ = b.unpack(inv, 17, close=False)           # an inverse (boolean rows only: no chain closes on them)
        b.unpack(self.eq, 1)                                     # a flag's own bit: ISZERO -> BITS, count 1
        two, _ = b.lin([g[8]], [1])
        b.unpack(two, 2)
        three, _ = b.lin([g[9]], [1])
        b.unpack(three, 3)
        self.ya, self.row_a = b.out([g[10], g[1], g[2], g[3]], ecc=True)      # OUT_INV; witness 2 makes its denominator 0
        b.out([self.ya, self.eq, self.x_bits[0], self.inv17[16]])                # hinted variables on input wires of an OUT row
        self.sc, self.given, self.hints = b.finish(), b.given, b.hints

    def values(self):
        """five witnesses; the full-width source is 0, 1, r - 1, 2^253 and random; the tests hold on both sides"""
        g, given = self.g, self.given
        vals = given_values(self.sc, given, 5, 17)
        at = {v: k for k, v in enumerate(given)}
        for p, full in enumerate((0, 1, R - 1, 1 << 253, None)):
            v = vals[p]
            v[at[g[0]]], v[at[g[1]]] = (p * 31) % 128, 127 - p
            if full is not None:
                v[at[g[2]]] = full
            if p in (1, 3):
                v[at[g[4]]] = v[at[g[3]]]                        # d = 0
            if p in (0, 4):
                v[at[g[7]]] = (3 * v[at[g[5]]] + v[at[g[6]]]) % R   # a = c
            v[at[g[8]]], v[at[g[9]]] = p % 4, (p + 3) % 8
        # witness 2: the OUT_INV row's own given value chosen so that q_o - q_ecc w0 w1 w2 w3 vanishes
        sel, row, v = self.sc.selectors, self.row_a, vals[2]
        w = [v[at[self.sc.wire_vars[i][row]]] for i in range(1, 4)]
        v[at[g[10]]] = sel[Q_O][row] * pow(sel[Q_ECC][row] * w[0] * w[1] * w[2] % R, R - 2, R) % R
        return vals


@pytest.fixture(scope="module")
def hand(cg, tau):
    c = Hand()
    c.h, c.pk, c.vk = key_for(cg, tau, c.sc)
    c.vals = c.values()
    c.want = [walk_hints(c.sc, c.given, v, c.hints) for v in c.vals]   # computed once, shared, left unchanged
    yield c
    cg.plonk_free_key(c.pk)
    cg.srs_free(c.h)


# ---- 1. a hand-built circuit against the model, by every entry point -------------------------------------------------------
@pytest.mark.parametrize("pack", [1, 16, 0])
def test_hand_built_circuit_equals_the_model(cg, hand, pack):
    c = hand
    info, hinfo = cg.plonk_key_set_given_hints(c.pk, c.given, c.hints)
    assert info.as_dict() == c.want[0][2] and hinfo.as_dict() == c.want[0][3]
    assert cg.plonk_key_hint_info(c.pk).as_dict() == hinfo.as_dict() and cg.plonk_key_solver_info(c.pk).as_dict() == info.as_dict()
    assert sorted(len(h[2]) for h in c.hints if h[0] == HINT_BITS) == [1, 2, 3, 8, 17, 254]
    assert hinfo.hint_items == 1 + 1 + 1 + 1 + 1 + 8 + 2 * 3 and hinfo.inv_hints == hinfo.iszero_hints == 3
    assert info.inv_rows == 1 and info.num_defined + hinfo.num_hinted + len(c.given) == c.sc.num_vars - 3
    # the sides of the tests, by the model: d = 0 in witnesses 1 and 3, a = c in 0 and 4, full = 0 in 0
    assert [w[0][c.d_zero] for w in c.want] == [0, 1, 0, 1, 0] and [w[0][c.eq] for w in c.want] == [1, 0, 0, 0, 1]
    assert [w[0][c.full] for w in c.want][:4] == [0, 1, R - 1, 1 << 253]
    assert [w[1] for w in c.want] == [(0, 0), (0, 0), (1, c.row_a), (0, 0), (0, 0)]
    # one list of 17 witnesses - the five value sets in turn, the zero denominator at 2, 7 and 12 - solved at counts 1, 2, 3
    # and 17: at W = 16 the last is a full workgroup and one with a single slot taken
    rows = [p % 5 for p in range(17)]
    gv17, want17 = mont_rows([c.vals[p] for p in rows]), mont_rows([c.want[p][0] for p in rows])
    old = cg.plonk_get_solve_pack()
    cg.plonk_set_solve_pack(pack)
    try:
        solved = {count: solve_host_and_dev(cg, c.pk, np.ascontiguousarray(gv17[:count])) for count in (1, 2, 3, 17)}
    finally:
        cg.plonk_set_solve_pack(old)
    for count, (got, st) in solved.items():
        assert np.array_equal(got, want17[:count]), count
        assert status_tuples(st) == [c.want[p][1] for p in rows[:count]], count
    got, _ = solved[17]
    assert not got[2, c.ya].any() and not got[12, c.ya].any() and not got[:, -3:].any()
    # bit 253 of 2^253 sits in the last chunk; r - 1 has its low word's top nibble set
    one = bu.to_mont_array([1])[0]
    assert np.array_equal(got[3, c.full_bits[253]], one) and not got[3, c.full_bits[:253]].any()
    assert np.array_equal(got[2, c.full_bits[28:32]], np.stack([one] * 4))


def test_hand_built_circuit_is_checked_and_proved_in_place(cg, tau, hand):
    c = hand
    cg.plonk_key_set_given_hints(c.pk, c.given, c.hints)
    gv = mont_rows(c.vals)
    at = {v: k for k, v in enumerate(c.given)}
    pubs = np.ascontiguousarray(gv[:, [at[v] for v in c.sc.pub_vars]])
    d_g = cg.DevBuf.from_numpy(gv)
    d_v, st = cg.plonk_solve_vars(c.pk, d_g, 5)
    faults = cg.plonk_check_witness_batch(c.pk, d_v, pubs, 5, input_form="vars")
    # every SOLVED witness is accepted; the one whose denominator vanished holds 0 there and fails at that row
    assert [f.kind for f in faults] == [0, 0, 1, 0, 0] and faults[2].row == c.row_a
    d_g.free()
    d_v.free()
    ok = [0, 1, 3, 4]
    bls = np.stack([bu.to_mont_array(bu.blinders(2000 + p)) for p in ok])
    proofs, outcomes, solved = cg.plonk_prove_given([c.pk] * 4, np.ascontiguousarray(gv[ok]), pubs[ok], bls, [b"note"] * 4)
    assert [o.status for o in outcomes] == [0] * 4 and status_tuples(solved) == [(0, 0)] * 4
    model = mont_rows([c.want[p][0] for p in ok])
    want = cg.plonk_prove_batch(c.pk, model, pubs[ok], bls, b"note", 4, input_form="vars")
    assert [bytes(p) for p in proofs] == [bytes(p) for p in want]
    g2h = cg.g2_generator()
    bh = cg.g2_mul(g2h, tau)
    assert all(cg.plonk_verify(c.vk, g2h, bh, pubs[ok][i], proofs[i], b"note") for i in range(4))


# ---- 2. a value that does not fit its unpack --------------------------------------------------------------------------------
def test_a_value_beyond_its_unpack_is_solved_and_then_refused_by_the_check(cg, tau):
    b = HBuilder(6, 1, 5)
    g = [b.var(given=True) for _ in range(2)]
    x, _ = b.lin(g, [1, 1])
    bits, close = b.unpack(x, 8)
    sc, given = b.finish(), b.given
    h, pk, _ = key_for(cg, tau, sc)
    cg.plonk_key_set_given_hints(pk, given, b.hints)
    vals = [[0, 1, 9, 200, 100], [0, 1, 9, 200, 55]]              # x = 300 = 0b1_0010_1100 and x = 255
    want = [walk_hints(sc, given, v, b.hints) for v in vals]
    assert [want[0][0][t] for t in bits] == [0, 0, 1, 1, 0, 1, 0, 0] and want[0][0][x] == 300
    got, st = solve_host_and_dev(cg, pk, mont_rows(vals))
    assert status_tuples(st) == [(0, 0)] * 2                     # no hint sets a status
    assert np.array_equal(got, mont_rows([w[0] for w in want]))
    pubs = mont_rows([[9], [9]])
    d_v = cg.DevBuf.from_numpy(got)
    faults = cg.plonk_check_witness_batch(pk, d_v, pubs, 2, input_form="vars")
    assert (faults[0].kind, faults[0].row) == (1, close) and faults[1].kind == 0
    d_v.free()
    cg.plonk_free_key(pk)
    cg.srs_free(h)


# ---- 3. levels wider than a workgroup --------------------------------------------------------------------------------------
def test_wide_levels_of_hint_items(cg, tau):
    """off 12 given sources: 300 INV0, 300 ISZERO, 300 BITS(254) and 40 BITS(2) hints whose targets occur in no cell, and
    five OUT rows: one level of 5 + 600 + 300 * 8 + 40 items"""
    b = HBuilder(6, 1, 9)
    g = [b.var(given=True) for _ in range(12)]
    rng = b.rng
    for _ in range(5):
        b.out([g[rng.next() % 12] for _ in range(4)])
    for k in range(300):
        b.hints.append((HINT_INV0, g[k % 12], [b.var()]))
        b.hints.append((HINT_BITS, g[(k + 5) % 12], [b.var() for _ in range(254)]))
        b.hints.append((HINT_ISZERO, g[(k + 7) % 12], [b.var()]))
    for k in range(40):
        b.hints.append((HINT_BITS, g[k % 12], [b.var(), b.var()]))
    sc, given = b.finish(), b.given
    h, pk, _ = key_for(cg, tau, sc)
    info, hinfo = cg.plonk_key_set_given_hints(pk, given, b.hints)
    assert info.as_dict() == dict(num_given=len(given), num_defined=5, levels=1, widest_level=3045, inv_rows=0, root_rows=0)
    assert hinfo.as_dict() == dict(num_hints=940, num_hinted=600 + 300 * 254 + 80, bits_hints=340, inv_hints=300,
                                   iszero_hints=300, hint_items=600 + 2400 + 40)
    vals = given_values(sc, given, 2, 3)
    vals[1][given.index(g[0])] = 0                               # a zero source: inverse 0, flag 1
    want = [walk_hints(sc, given, v, b.hints) for v in vals]
    assert want[0][2] == info.as_dict() and want[0][3] == hinfo.as_dict()
    got, st = solve_host_and_dev(cg, pk, mont_rows(vals))
    assert np.array_equal(got, mont_rows([w[0] for w in want])) and status_tuples(st) == [(0, 0)] * 2
    cg.plonk_free_key(pk)
    cg.srs_free(h)


# ---- 4. refusals through the ABI, and the schedule's lifetime --------------------------------------------------------------
def test_refusals_leave_the_previous_schedule_working(cg, tau, hand):
    c = hand
    sc, given, hints = c.sc, c.given, c.hints
    info, hinfo = cg.plonk_key_set_given_hints(c.pk, given, hints)
    want3 = mont_rows([c.want[3][0]])

    def still_solves():
        got, st = cg.plonk_solve_vars(c.pk, mont_rows(c.vals[3:4]), 1)
        assert np.array_equal(got, want3) and status_tuples(st) == [(0, 0)]
        assert cg.plonk_key_hint_info(c.pk).as_dict() == hinfo.as_dict()

    def refused(hs, *texts, g=given):
        with pytest.raises(cg.CapGpuError) as e:
            cg.plonk_key_set_given_hints(c.pk, g, hs)
        msg = str(e.value)
        assert e.value.code == -1 and "capgpu_plonk_key_set_given_hints" in msg and "the key is unchanged" in msg
        for t in texts:
            assert t in msg, msg
        with pytest.raises(ValueError) as w:                     # the model refuses the same list, for the same reason
            walk_hints(sc, g, [0] * len(g), hs)
        assert str(w.value).split(":")[0] in msg, (str(w.value), msg)
        still_solves()

    nv, k = sc.num_vars, len(hints)
    free1, free2, free3 = nv - 1, nv - 2, nv - 3                 # the three ids that occur in no cell
    refused(hints + [(3, c.full, [free1])], f"hint {k}: unknown kind 3", f"variable {c.full}")
    refused(hints + [(HINT_INV0, nv, [free1])], f"hint {k}: its source variable {nv}")
    refused(hints + [(HINT_BITS, c.full, [free1, nv + 4])], f"hint {k}: its target 1, variable {nv + 4}")
    refused(hints + [(HINT_INV0, c.full, [free1, free2])], f"hint {k}: count 2 is out of range")
    refused(hints + [(HINT_ISZERO, c.full, [])], f"hint {k}: count 0 is out of range")
    refused(hints + [(HINT_BITS, c.full, [free1, free2, free1])], f"hint {k}: its target variable {free1} is listed twice",
            f"hint {k} has it too")
    refused(hints + [(HINT_INV0, c.full, [c.x_bits[2]])], f"hint {k}: its target variable {c.x_bits[2]} is listed twice",
            "hint 0 has it too")
    refused(hints + [(HINT_BITS, free1, [free2, free1])], f"hint {k}: its target 1 is its own source variable {free1}")
    refused(hints + [(HINT_ISZERO, c.full, [given[5]])], f"hint {k}: its target variable {given[5]} is given", "given_vars[5]")
    refused(hints + [(HINT_INV0, c.ya, [c.full])], f"hint {k}: its target variable {c.full} already has a value",
            f"row {[j for j in range(sc.n) if sc.wire_vars[4][j] == c.full][0]} defines it")
    refused(hints + [(HINT_INV0, free1, [free2])], f"hint {k}: its source variable {free1} never gets a value")
    refused(hints, "variable 5 is given twice", g=given + [5])   # the list's own refusals come through the new call too
    # first + count beyond the targets: only the raw call can say that
    L = cg.load()
    tab = (cg.Hint * 1)(cg.Hint(HINT_BITS, c.full, 1, 3))
    tg = np.array([free1, free2, free3], np.uint32)
    gi = np.array(given, np.uint32)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    rc = L.capgpu_plonk_key_set_given_hints(ctypes.c_uint64(c.pk), gi.ctypes.data_as(u32p), ctypes.c_size_t(gi.size), tab,
                                            ctypes.c_size_t(1), tg.ctypes.data_as(u32p), ctypes.c_size_t(3), None, None)
    err = L.capgpu_last_error()
    assert rc == -1 and b"hint 0: first + count = 4, num_targets is 3" in err and b"the key is unchanged" in err
    still_solves()
    # capgpu_plonk_key_set_given alone refuses this circuit, naming the row it names today: the first boolean row
    with pytest.raises(ValueError) as w:
        walk(sc, given, [0] * len(given))
    with pytest.raises(cg.CapGpuError) as e:
        cg.plonk_key_set_given(c.pk, given)
    first_bool = [j for j in range(sc.n) if sc.wire_vars[0][j] == c.x_bits[0]][0]
    assert str(w.value) == f"row {first_bool} cannot define its variable {c.x_bits[0]}"
    assert "capgpu_plonk_key_set_given:" in str(e.value) and str(w.value) in str(e.value) and "the key is unchanged" in str(e.value)
    still_solves()
    # ... and takes it with every hinted variable given: the hints leave the key
    all_given = given + [t for h_ in hints for t in h_[2]]
    info2 = cg.plonk_key_set_given(c.pk, all_given)
    zero = cg.HintInfo().as_dict()
    assert cg.plonk_key_hint_info(c.pk).as_dict() == zero and set(zero.values()) == {0}
    assert info2.num_given == len(all_given) and info2.num_defined == info.num_defined
    full = c.want[3][0]
    got, _ = cg.plonk_solve_vars(c.pk, mont_rows([[full[v] for v in all_given]]), 1)
    assert np.array_equal(got, want3)
    # a second hinted set-up replaces it; capgpu_plonk_key_set_vars drops schedule and hints
    cg.plonk_key_set_given_hints(c.pk, given, hints)
    still_solves()
    cg.plonk_key_set_vars(c.pk, np.array(sc.wire_vars), sc.num_vars)
    assert cg.plonk_key_hint_info(c.pk).as_dict() == zero
    assert cg.plonk_key_solver_info(c.pk).as_dict() == cg.SolverInfo().as_dict()
    cg.plonk_key_set_given_hints(c.pk, given, hints)             # (the module's other tests find the key as they expect it)
    # a key without a table
    sy = bu.synthetic_circuit(4, 1)
    h3 = cg.srs_generate(tau, sy.n + 3)
    pk_s, _ = cg.plonk_preprocess(h3, sy.n, sy.num_inputs, sy.selectors_mont(), sy.sigma_mont())
    with pytest.raises(cg.CapGpuError) as e:
        cg.plonk_key_set_given_hints(pk_s, [0, 1] + list(sy.free_vars), [(HINT_INV0, 0, [1])])
    assert "capgpu_plonk_key_set_given_hints: the key has no wire -> variable table" in str(e.value)
    assert "the key is unchanged" in str(e.value)
    cg.plonk_free_key(pk_s)
    cg.srs_free(h3)


# ---- 5. the transfer model with its hints -----------------------------------------------------------------------------------
def test_hinted_transfer_model_follows_from_its_inputs(cg, tau):
    """cap_like_hinted_circuit('transfer_2x2') - n = 2^15, the smallest NOTE_SHAPES entry that holds it: 208 given values
    instead of the unhinted model's 2 425"""
    sc, given, hints = bu.cap_like_hinted_circuit("transfer_2x2")
    assert sc.n == 1 << 15 and len(given) == 208 and len(hints) == 22
    vals = [bu.cap_like_given_values(sc, s) for s in (11, 12, 13)]
    want = [walk_hints(sc, given, v, hints) for v in vals]
    h, pk, _ = key_for(cg, tau, sc)
    info, hinfo = cg.plonk_key_set_given_hints(pk, given, hints)
    assert info.as_dict() == want[0][2] and hinfo.as_dict() == want[0][3]
    gv = mont_rows(vals)
    d_g = cg.DevBuf.from_numpy(gv)
    d_v, st = cg.plonk_solve_vars(pk, d_g, 3)
    assert status_tuples(st) == [w[1] for w in want] == [(0, 0)] * 3
    assert np.array_equal(d_v.to_numpy().reshape(3, sc.num_vars, 4), mont_rows([w[0] for w in want]))
    at = {v: k for k, v in enumerate(given)}
    pubs = np.ascontiguousarray(gv[:, [at[v] for v in sc.pub_vars]])
    assert [f.kind for f in cg.plonk_check_witness_batch(pk, d_v, pubs, 3, input_form="vars")] == [0, 0, 0]
    d_g.free()
    d_v.free()
    cg.plonk_free_key(pk)
    cg.srs_free(h)
