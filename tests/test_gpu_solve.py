"""The witness solver on the device (capgpu_plonk_key_set_given, capgpu_plonk_solve_vars[_dev]): a key with a wire -> variable
table completes assignments from the values its circuit is GIVEN.  `walk` below is the rule of include/capgpu.h in Python
integers - the definition; the device's vars_out must equal it word for word, and for the harness circuits the columns
bench_utils' witness generator makes.  The completed buffer is a CAPGPU_INPUT_VARS witness: it is checked and proved in
place."""
import ctypes

import numpy as np
import pytest

from cap_amd import bench_utils as bu

pytestmark = pytest.mark.gpu

R = bu.R
Q_LC, Q_MUL, Q_HASH, Q_O, Q_C, Q_ECC = 0, 4, 6, 10, 11, 12
E5 = pow(5, -1, R - 1)
assert (R - 1) % 5 == 1 and 5 * E5 % (R - 1) == 1


# ---- the definition --------------------------------------------------------------------------------------------------
def rest_of(sel, j, w):
    """q_c + sum q_lc_i w_i + q_mul0 w0 w1 + q_mul1 w2 w3 + sum q_hash_i w_i^5 over wires 0 .. 3"""
    r = sel[Q_C][j] + sel[Q_MUL][j] * w[0] * w[1] + sel[Q_MUL + 1][j] * w[2] * w[3]
    for i in range(4):
        r += sel[Q_LC + i][j] * w[i] + sel[Q_HASH + i][j] * pow(w[i], 5, R)
    return r % R


def walk(sc, given_ids, given_vals):
    """-> (value per variable, status (kind, row), info dict); raises ValueError(text) where the rule refuses"""
    n, sel, wv = sc.n, sc.selectors, sc.wire_vars
    if len(set(given_ids)) != len(given_ids):
        raise ValueError("given twice")
    if any(v >= sc.num_vars for v in given_ids):
        raise ValueError("num_vars is")
    val = [None] * sc.num_vars
    level = [0] * sc.num_vars
    for v, x in zip(given_ids, given_vals):
        val[v] = x % R
    first_zero = None
    widths, inv_rows, root_rows, defined = {}, 0, 0, 0
    for j in range(n):
        ids = [wv[i][j] for i in range(5)]
        unknown = []
        for v in ids:
            if val[v] is None and v not in unknown:
                unknown.append(v)
        if not unknown:
            continue
        if j < sc.num_inputs:
            raise ValueError(f"row {j} is a public-input row and its variable {unknown[0]} is not given")
        if len(unknown) >= 2:
            raise ValueError(f"row {j} holds two variables without a value, {unknown[0]} and {unknown[1]}")
        u = unknown[0]
        where = [i for i in range(5) if ids[i] == u]
        w = [0 if ids[i] == u else val[ids[i]] for i in range(5)]
        q = lambda s: sel[s][j] % R                              # noqa: E731
        if where == [4] and (q(Q_O) or q(Q_ECC)):
            den = (q(Q_O) - q(Q_ECC) * w[0] * w[1] * w[2] * w[3]) % R
            if q(Q_ECC):
                inv_rows += 1
            if den == 0:
                val[u] = 0
                first_zero = j if first_zero is None else first_zero
            else:
                val[u] = rest_of(sel, j, w) * pow(den, R - 2, R) % R
        elif len(where) == 1 and where[0] < 4 and q(Q_HASH + where[0]) and not q(Q_LC + where[0]) \
                and not q(Q_MUL + where[0] // 2) and not q(Q_ECC):
            i = where[0]
            t = (q(Q_O) * w[4] - rest_of(sel, j, w)) * pow(q(Q_HASH + i), R - 2, R) % R    # (w[i] = 0 in rest_of)
            val[u] = pow(t, E5, R)
            root_rows += 1
        else:
            raise ValueError(f"row {j} cannot define its variable {u}")
        level[u] = 1 + max(level[v] for v in ids if v != u)
        widths[level[u]] = widths.get(level[u], 0) + 1
        defined += 1
    info = dict(num_given=len(given_ids), num_defined=defined, levels=len(widths), widest_level=max(widths.values(), default=0),
                inv_rows=inv_rows, root_rows=root_rows)
    status = (0, 0) if first_zero is None else (1, first_zero)
    return [0 if x is None else x for x in val], status, info


# ---- circuits --------------------------------------------------------------------------------------------------------
class Builder:
    """rows of a circuit in Python integers; variables 0 and 1 hold the constants, 2 .. 1 + num_inputs the public inputs"""

    def __init__(self, log_n, num_inputs, seed):
        self.log_n, self.n, self.num_inputs = log_n, 1 << log_n, num_inputs
        self.rng = bu.SplitMix64(seed)
        self.sel = [[0] * self.n for _ in range(13)]
        self.wv = [[0] * self.n for _ in range(5)]
        self.num_vars, self.given, self.j = 2 + num_inputs, list(range(2 + num_inputs)), num_inputs
        for j in range(num_inputs):
            self.wv[4][j] = 2 + j
            self.sel[Q_O][j] = 1

    def var(self, given=False):
        self.num_vars += 1
        if given:
            self.given.append(self.num_vars - 1)
        return self.num_vars - 1

    def row(self, ids, **sels):
        j = self.j
        self.j += 1
        assert j < self.n
        for i in range(5):
            self.wv[i][j] = ids[i]
        for name, x in sels.items():
            self.sel[int(name[1:])][j] = x % R
        return j

    def rand_sels(self, which):
        return {f"s{s}": self.rng.field() | 1 for s in which}

    def out(self, ins, ecc=False, q_o=None):
        """an OUT row on fresh variable u"""
        u = self.var()
        sels = self.rand_sels(range(13 if ecc else 12))
        if q_o is not None:
            sels[f"s{Q_O}"] = q_o
        return u, self.row(list(ins) + [u], **sels)

    def root(self, ins, wire, known):
        """a ROOT5 row: fresh u on `wire`, `known` on wire 4"""
        u = self.var()
        ids = list(ins) + [known]
        ids[wire] = u
        sels = self.rand_sels(range(12))
        sels[f"s{Q_LC + wire}"] = 0
        sels[f"s{Q_MUL + wire // 2}"] = 0
        return u, self.row(ids, **sels)

    def finish(self):
        return bu.SyntheticCircuit(log_n=self.log_n, num_inputs=self.num_inputs, selectors=self.sel, wire_vars=self.wv,
                                   num_vars=self.num_vars + 3, free_vars=self.given[2:], pub_vars=list(range(2, 2 + self.num_inputs)),
                                   gate_rows=self.j, sigma=None)   # (three ids that occur in no cell: they come out as 0)


def hand_circuit(log_n, seed=7):
    """every shape of the rule in the first rows; a larger domain continues with random rows of all kinds"""
    b = Builder(log_n, 2, seed)
    g = [b.var(given=True) for _ in range(4)]
    a, _ = b.out([2, 3, g[0], g[1]])                             # OUT without q_ecc
    e1, _ = b.out([g[0], g[1], g[2], g[3]], ecc=True)            # OUT with q_ecc
    e2, _ = b.out([2, g[1], 3, g[3]], ecc=True, q_o=0)           # ... and q_o = 0
    roots = [b.root([g[0], g[1], g[2], g[3]], wire, g[(wire + 1) % 4])[0] for wire in range(4)]   # ROOT5 on each wire
    r2, _ = b.root([a, e1, roots[0], g[2]], 1, e2)               # ROOT5 whose wire-4 variable was defined a level earlier
    b.row([a, e1, e2, r2, roots[3]], s10=1, s0=5)                # a constraint (not evaluated, not satisfied)
    pool = g + [a, e1, e2, r2] + roots
    rng = b.rng
    while b.j < b.n - max(2, b.n // 8):
        ins = [pool[-1 - rng.next() % min(len(pool), 10)] if rng.next() & 3 else pool[rng.next() % len(pool)] for _ in range(4)]
        kind = rng.next() % 8
        if kind < 3:
            u, _ = b.out(ins)
        elif kind < 5:
            u, _ = b.out(ins, ecc=True)
        elif kind < 7:
            u, _ = b.root(ins, rng.next() % 4, pool[rng.next() % len(pool)])
        else:
            b.row(ins + [pool[rng.next() % len(pool)]], s10=1)
            continue
        pool.append(u)
    return b.finish(), b.given


def wide_circuit():
    """n = 1024: a level of 600 independent OUT rows (400 without, 200 with q_ecc) and a level of 300 ROOT5 rows"""
    b = Builder(10, 3, 11)
    g = [b.var(given=True) for _ in range(12)]
    rng = b.rng
    outs = []
    for k in range(600):
        outs.append(b.out([g[rng.next() % 12] for _ in range(4)], ecc=(k % 3 == 2))[0])
    for k in range(300):
        b.root([g[rng.next() % 12] for _ in range(4)], k % 4, outs[rng.next() % 600])
    return b.finish(), b.given


def key_for(cg, tau, sc):
    h = cg.srs_generate(tau, sc.n + 3)
    pk, vk = cg.plonk_preprocess_vars(h, sc.n, sc.num_inputs, sc.selectors_mont(), np.array(sc.wire_vars), sc.num_vars)
    return h, pk, vk


def given_values(sc, given, count, seed):
    """count x len(given) random values (0 and 1 for the constants) as integers"""
    rng = bu.SplitMix64(seed)
    return [[v if v < 2 else rng.field() for v in given] for _ in range(count)]


def mont_rows(rows):
    return np.stack([bu.to_mont_array(r) for r in rows])


def status_tuples(st):
    return [(s.kind, s.row) for s in st]


def solve_host_and_dev(cg, pk, gv):
    """both entry points on (count, num_given, 4) given values; they must agree -> (vars array, statuses)"""
    count = gv.shape[0]
    vars_h, st_h = cg.plonk_solve_vars(pk, gv, count)
    d_g = cg.DevBuf.from_numpy(gv)
    d_v, st_d = cg.plonk_solve_vars(pk, d_g, count)
    vars_d = d_v.to_numpy().reshape(vars_h.shape)
    d_g.free()
    d_v.free()
    assert np.array_equal(vars_h, vars_d) and status_tuples(st_h) == status_tuples(st_d)
    return vars_h, st_h


# ---- hand-built circuits against the walk ------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [4, 6])
def test_hand_built_circuits_equal_the_walk(cg, tau, log_n):
    sc, given = hand_circuit(log_n)
    h, pk, _ = key_for(cg, tau, sc)
    info = cg.plonk_key_set_given(pk, given)
    for count in (1, 3, 65):
        vals = given_values(sc, given, count, 100 + count)
        want = [walk(sc, given, v) for v in vals]
        assert info.as_dict() == want[0][2] and info.root_rows >= 5 and info.inv_rows >= 2
        got, st = solve_host_and_dev(cg, pk, mont_rows(vals))
        assert np.array_equal(got, mont_rows([w[0] for w in want]))
        assert status_tuples(st) == [w[1] for w in want] == [(0, 0)] * count
        assert not got[:, -3:].any()                             # variables in no cell
    cg.plonk_free_key(pk)
    cg.srs_free(h)


def test_wide_levels_stride_over_the_lanes(cg, tau):
    sc, given = wide_circuit()
    h, pk, _ = key_for(cg, tau, sc)
    info = cg.plonk_key_set_given(pk, given)
    assert info.as_dict() == dict(num_given=len(given), num_defined=900, levels=2, widest_level=600, inv_rows=200, root_rows=300)
    vals = given_values(sc, given, 2, 5)
    got, st = solve_host_and_dev(cg, pk, mont_rows(vals))
    assert np.array_equal(got, mont_rows([walk(sc, given, v)[0] for v in vals])) and status_tuples(st) == [(0, 0)] * 2
    cg.plonk_free_key(pk)
    cg.srs_free(h)


# ---- the harness circuits: against the witness generator, the witness check and the prover ------------------------------
def harness_given(sc, wires):
    """the given list [0, 1] + free_vars and, per witness, its values taken from the generator's columns (count, 5, n, 4)"""
    given = [0, 1] + list(sc.free_vars)
    wv = np.array(sc.wire_vars).reshape(-1)
    vals = np.zeros((wires.shape[0], sc.num_vars, 4), np.uint64)
    vals[:, wv] = wires.reshape(wires.shape[0], -1, 4)
    vals[:, 0], vals[:, 1] = bu.to_mont_array([0])[0], bu.to_mont_array([1])[0]
    return given, np.ascontiguousarray(vals[:, given])


def gathered(sc, vars_out):
    return vars_out[:, np.array(sc.wire_vars).reshape(-1)].reshape(vars_out.shape[0], 5, sc.n, 4)


@pytest.mark.parametrize("log_n", [6, 8, 10])
def test_synthetic_circuits_solved_checked_and_proved(cg, tau, log_n):
    """synthetic_circuit(log_n, 5): by the walk, depths 14 / 44 / 167 and 7 / 25 / 116 rows with q_ecc"""
    sc = bu.synthetic_circuit(log_n, 5)
    seeds = [900 + log_n, 7, 31]
    P = len(seeds)
    wires, pubs = sc.witnesses_mont(seeds, threads=4)
    given, gv = harness_given(sc, wires)
    h, pk, vk = key_for(cg, tau, sc)
    info = cg.plonk_key_set_given(pk, given)
    assert info.as_dict() == walk(sc, given, bu.from_mont_array(gv[0]))[2]
    assert (info.levels, info.inv_rows, info.root_rows) == {6: (14, 7, 0), 8: (44, 25, 0), 10: (167, 116, 0)}[log_n]
    assert info.num_given == len(given) and info.num_defined == sc.gate_rows - sc.num_inputs
    d_g = cg.DevBuf.from_numpy(gv)
    d_v, st = cg.plonk_solve_vars(pk, d_g, P)
    assert status_tuples(st) == [(0, 0)] * P
    vars_out = d_v.to_numpy().reshape(P, sc.num_vars, 4)
    assert np.array_equal(gathered(sc, vars_out), wires)
    faults = cg.plonk_check_witness_batch(pk, d_v, pubs, P, input_form="vars")
    assert [f.kind for f in faults] == [0] * P
    # the solved buffer proves in place: the proof bytes of the column form, in both transcript modes, and they verify
    bls = np.stack([bu.to_mont_array(bu.blinders(s + 1000)) for s in seeds])
    h2 = cg.g2_generator()
    bh = cg.g2_mul(h2, tau)
    mode = cg.plonk_get_transcript()
    try:
        for m in ("host", "device"):
            cg.plonk_set_transcript(m)
            want = [bytes(p) for p in cg.plonk_prove_batch(pk, wires, pubs, bls, b"note", P)]
            proofs = cg.plonk_prove_batch_dev(pk, d_v, pubs, bls, b"note", P, input_form="vars")
            assert [bytes(p) for p in proofs] == want, m
            assert all(cg.plonk_verify(vk, h2, bh, pubs[p], proofs[p], b"note") for p in range(P))
    finally:
        cg.plonk_set_transcript(mode)
    assert np.array_equal(d_v.to_numpy().reshape(vars_out.shape), vars_out), "check and prover must leave the buffer alone"
    # a changed given value: the solver checks nothing (status 0); the witness check then names a constraint row
    if sc.num_inputs:
        bad = gv.copy()
        k = given.index(sc.pub_vars[0])
        bad[1, k] = bu.to_mont_array([12345])[0]
        d_b, st = cg.plonk_solve_vars(pk, cg.DevBuf.from_numpy(bad), P)
        assert status_tuples(st) == [(0, 0)] * P
        faults = cg.plonk_check_witness_batch(pk, d_b, pubs, P, input_form="vars")
        assert [f.kind for f in faults] == [0, 1, 0] and faults[1].row == 0     # the public-input gate of row 0
        d_b.free()
    d_g.free()
    d_v.free()
    cg.plonk_free_key(pk)
    cg.srs_free(h)


# ---- zero denominators ---------------------------------------------------------------------------------------------------
def test_zero_denominators_name_the_lowest_row(cg, tau):
    """rows A < B invert q_o - q_ecc w0 w1 w2 w3 with w0 a given variable of their own: its value is chosen so that the
    denominator vanishes - for witness 1 at B, for witness 3 at A and B"""
    b = Builder(6, 1, 23)
    g = [b.var(given=True) for _ in range(8)]
    x, _ = b.out([g[0], g[1], g[2], g[3]])
    ya, row_a = b.out([g[4], g[1], g[2], g[3]], ecc=True)
    z, _ = b.out([ya, x, g[0], g[1]])                            # reads A's output
    yb, row_b = b.out([g[5], g[2], g[3], g[6]], ecc=True)
    b.root([g[0], yb, g[1], g[2]], 2, z)
    sc, given = b.finish(), b.given
    assert row_a < row_b
    h, pk, _ = key_for(cg, tau, sc)
    cg.plonk_key_set_given(pk, given)
    vals = given_values(sc, given, 5, 77)

    def vanish(v, row, own):
        """v[own] := q_o / (q_ecc w1 w2 w3) at `row`"""
        w = [v[given.index(sc.wire_vars[i][row])] for i in range(1, 4)]
        v[given.index(own)] = sc.selectors[Q_O][row] * pow(sc.selectors[Q_ECC][row] * w[0] * w[1] * w[2] % R, R - 2, R) % R

    vanish(vals[1], row_b, g[5])
    vanish(vals[3], row_b, g[5])
    vanish(vals[3], row_a, g[4])
    want = [walk(sc, given, v) for v in vals]
    assert [w[1] for w in want] == [(0, 0), (1, row_b), (0, 0), (1, row_a), (0, 0)]
    got, st = solve_host_and_dev(cg, pk, mont_rows(vals))
    assert status_tuples(st) == [w[1] for w in want]
    assert np.array_equal(got, mont_rows([w[0] for w in want]))
    assert not got[1, yb].any() and not got[3, ya].any() and not got[3, yb].any() and got[1, ya].any()
    for p in (0, 2, 4):                                          # the neighbours equal their lone solves
        lone, st1 = cg.plonk_solve_vars(pk, mont_rows([vals[p]]), 1)
        assert np.array_equal(lone[0], got[p]) and status_tuples(st1) == [(0, 0)]
    cg.plonk_free_key(pk)
    cg.srs_free(h)


# ---- set-up: refusals, figures, lifetime -----------------------------------------------------------------------------------
def refused(cg, pk, given, *texts):
    with pytest.raises(cg.CapGpuError) as e:
        cg.plonk_key_set_given(pk, given)
    assert e.value.code == -1 and "capgpu_plonk_key_set_given" in str(e.value) and "the key is unchanged" in str(e.value)
    for t in texts:
        assert t in str(e.value), str(e.value)


def test_set_up_refusals_and_the_schedules_lifetime(cg, tau):
    sc, given = hand_circuit(4)
    h, pk, _ = key_for(cg, tau, sc)
    zero = cg.SolverInfo().as_dict()
    assert cg.plonk_key_solver_info(pk).as_dict() == zero
    with pytest.raises(cg.CapGpuError) as e:
        cg.plonk_solve_vars(pk, np.zeros((1, len(given), 4), np.uint64), 1)
    assert e.value.code == -1 and "no solver" in str(e.value)
    st = (cg.SolveStatus * 1)()
    buf = np.zeros(sc.num_vars * 4, np.uint64)
    assert cg.load().capgpu_plonk_solve_vars(ctypes.c_uint64(pk), 1, cg._p(buf), cg._p(buf), st) == -1
    assert b"no solver" in cg.load().capgpu_last_error()
    # count == 0: CAPGPU_OK, nothing written, no pointer needed
    assert cg.load().capgpu_plonk_solve_vars(ctypes.c_uint64(pk), 0, None, None, None) == 0
    assert cg.load().capgpu_plonk_solve_vars_dev(ctypes.c_uint64(pk), 0, None, None, None) == 0
    # the list
    refused(cg, pk, given + [given[3]], f"variable {given[3]} is given twice")
    refused(cg, pk, given + [sc.num_vars], f"= {sc.num_vars}, num_vars is {sc.num_vars}")
    # the rule, each with the lowest offending row: what the walk says, the library says
    cases = [[v for v in given if v != 3],                       # a public-input variable
             [v for v in given if v not in (given[4], given[5])],   # two unknowns in one row
             given[:-1]]                                         # the last given value: it meets the row's own output
    for g in cases:
        with pytest.raises(ValueError) as w:
            walk(sc, g, [0] * len(g))
        refused(cg, pk, g, str(w.value))
    assert cg.plonk_key_solver_info(pk).as_dict() == zero, "a refused list leaves the key as it was"
    # a fifth-root row with q_lc set on the root's wire is no defining row
    b = Builder(4, 1, 3)
    g = [b.var(given=True) for _ in range(4)]
    u = b.var()
    row = b.row([g[0], u, g[2], g[3], g[1]], **{f"s{Q_HASH + 1}": 9, f"s{Q_LC + 1}": 1, f"s{Q_O}": 1})
    sc_bad = b.finish()
    h2, pk_bad, _ = key_for(cg, tau, sc_bad)
    refused(cg, pk_bad, b.given, f"row {row} cannot define its variable {u}")
    cg.plonk_free_key(pk_bad)
    cg.srs_free(h2)
    # a key without a table
    sy = bu.synthetic_circuit(4, 1)
    h3 = cg.srs_generate(tau, sy.n + 3)
    pk_s, _ = cg.plonk_preprocess(h3, sy.n, sy.num_inputs, sy.selectors_mont(), sy.sigma_mont())
    refused(cg, pk_s, [0, 1] + list(sy.free_vars), "has no wire -> variable table")
    # ... gets one, then a schedule; key_set_vars drops the schedule again
    cg.plonk_key_set_vars(pk_s, np.array(sy.wire_vars), sy.num_vars)
    info = cg.plonk_key_set_given(pk_s, [0, 1] + list(sy.free_vars))
    assert info.num_defined == sy.gate_rows - sy.num_inputs and cg.plonk_key_solver_info(pk_s).as_dict() == info.as_dict()
    cg.plonk_key_set_vars(pk_s, np.array(sy.wire_vars), sy.num_vars)
    assert cg.plonk_key_solver_info(pk_s).as_dict() == zero
    cg.plonk_free_key(pk_s)
    cg.srs_free(h3)
    # a second list replaces the first: with the first OUT row's variable given too, one row less is defined
    info1 = cg.plonk_key_set_given(pk, given)
    vals = given_values(sc, given, 2, 9)
    full = [walk(sc, given, v)[0] for v in vals]
    got1, _ = cg.plonk_solve_vars(pk, mont_rows(vals), 2)
    first_out = sc.wire_vars[4][sc.num_inputs]
    given2 = given + [first_out]
    info2 = cg.plonk_key_set_given(pk, given2)
    assert info2.num_defined == info1.num_defined - 1 and info2.num_given == info1.num_given + 1
    assert cg.plonk_key_solver_info(pk).as_dict() == info2.as_dict()
    vals2 = [v + [f[first_out]] for v, f in zip(vals, full)]
    got2, _ = cg.plonk_solve_vars(pk, mont_rows(vals2), 2)
    assert np.array_equal(got1, got2) and np.array_equal(got1, mont_rows(full))
    # freed with the key
    cg.plonk_free_key(pk)
    with pytest.raises(cg.CapGpuError) as e:
        cg.plonk_key_solver_info(pk)
    assert e.value.code == -4
    assert cg.load().capgpu_plonk_solve_vars(ctypes.c_uint64(pk), 1, cg._p(buf), cg._p(buf), st) == -4
    cg.srs_free(h)


def test_scratch_goes_through_the_contexts_counters(cg, tau):
    sc = bu.synthetic_circuit(8, 2, seed=5)
    wires, _ = sc.witnesses_mont(list(range(40, 72)), threads=4)
    given, gv = harness_given(sc, wires)
    h, pk, _ = key_for(cg, tau, sc)
    cg.plonk_key_set_given(pk, given)
    cg.set_device(0)
    try:
        cg.trim()
        before = cg.scratch_stats()
        got, _ = cg.plonk_solve_vars(pk, gv, 32)
        after = cg.scratch_stats()
    finally:
        cg.set_device(-1)
    assert after["grow_events"] > before["grow_events"]
    assert after["grow_bytes"] - before["grow_bytes"] >= 32 * (len(given) + sc.num_vars) * 32
    assert np.array_equal(gathered(sc, got), wires)
    cg.plonk_free_key(pk)
    cg.srs_free(h)


def test_on_a_callers_stream(cg, tau):
    import torch
    sc = bu.synthetic_circuit(8, 3, seed=6)
    wires, _ = sc.witnesses_mont([1, 2, 3], threads=3)
    given, gv = harness_given(sc, wires)
    h, pk, _ = key_for(cg, tau, sc)
    cg.plonk_key_set_given(pk, given)
    cg.set_device(0)
    try:
        d_g = cg.DevBuf.from_numpy(gv)
        d_own, st_own = cg.plonk_solve_vars(pk, d_g, 3)
        own = d_own.to_numpy()
        S = torch.cuda.Stream()
        with cg.on_stream(S):
            d_s, st_s = cg.plonk_solve_vars(pk, d_g, 3)
        cg.sync_all()
        assert np.array_equal(d_s.to_numpy(), own) and status_tuples(st_s) == status_tuples(st_own) == [(0, 0)] * 3
        assert np.array_equal(gathered(sc, own.reshape(3, sc.num_vars, 4)), wires)
        for d in (d_g, d_own, d_s):
            d.free()
    finally:
        cg.set_stream(None)
        cg.set_device(-1)
    cg.plonk_free_key(pk)
    cg.srs_free(h)


# ---- full size -------------------------------------------------------------------------------------------------------------
def test_transfer_circuit_at_full_size(cg, tau):
    """cap_like_circuit('transfer_2x2'), n = 2^15: depth 584, widest level 3 056, 5 840 inversions per witness"""
    sc = bu.cap_like_circuit("transfer_2x2")
    wires, pubs = sc.witnesses_mont([11, 12], threads=2)
    given, gv = harness_given(sc, wires)
    h, pk, _ = key_for(cg, tau, sc)
    info = cg.plonk_key_set_given(pk, given)
    assert sc.n == 1 << 15 and (info.levels, info.widest_level, info.inv_rows, info.root_rows) == (584, 3056, 5840, 0)
    assert (info.num_given, info.num_defined) == (2425, 18193)
    d_g = cg.DevBuf.from_numpy(gv)
    d_v, st = cg.plonk_solve_vars(pk, d_g, 2)
    assert status_tuples(st) == [(0, 0)] * 2
    assert np.array_equal(gathered(sc, d_v.to_numpy().reshape(2, sc.num_vars, 4)), wires)
    assert [f.kind for f in cg.plonk_check_witness_batch(pk, d_v, pubs, 2, input_form="vars")] == [0, 0]
    d_g.free()
    d_v.free()
    cg.plonk_free_key(pk)
    cg.srs_free(h)
