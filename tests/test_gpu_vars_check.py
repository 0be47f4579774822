"""The witness check in variable form (CAPGPU_INPUT_VARS): values gathered through the key's table satisfy every copy
constraint by construction, so only gates can fail - with the verdict the evals-form check gives for the expanded,
equally corrupted columns.  A key with a table keeps reporting broken copy constraints of evals-form columns."""
import threading

import numpy as np
import pytest

from cap_amd import bench_utils as bu
from tests.test_gpu_vars_prove import as_bytes, batch, var_values

pytestmark = pytest.mark.gpu


def keys_for(cg, tau, sc):
    h = cg.srs_generate(tau, sc.n + 3)
    pk_v, _ = cg.plonk_preprocess_vars(h, sc.n, sc.num_inputs, sc.selectors_mont(), np.array(sc.wire_vars), sc.num_vars)
    pk_s, _ = cg.plonk_preprocess(h, sc.n, sc.num_inputs, sc.selectors_mont(), sc.sigma_mont())
    return h, pk_v, pk_s


def verdict(f):
    return (f.kind, f.wire, f.row, f.wire2, f.row2, f.gates_failed, f.copies_failed)


def busy_variable(sc):
    """a variable that feeds several gates: the one (beyond the constants 0 and 1) that most rows below gate_rows read"""
    wv = np.array(sc.wire_vars)[:4, sc.num_inputs:sc.gate_rows]
    counts = np.bincount(wv.reshape(-1), minlength=sc.num_vars)
    counts[:2] = 0
    return int(counts.argmax())


def corrupted(sc, seed, var):
    """(columns, variable values, public inputs) of witness `seed` with one variable's value changed everywhere"""
    w, pubs = sc.witness(seed)
    w = [list(col) for col in w]
    for i in range(5):
        for j in range(sc.n):
            if sc.wire_vars[i][j] == var:
                w[i][j] = (w[i][j] + 1) % bu.R
    pubs = [w[4][j] for j in range(sc.num_inputs)]  # (public inputs sit on wire 4 of the first rows)
    return sc.wires_mont(w), var_values(sc, w, fill_seed=seed), (bu.to_mont_array(pubs) if pubs else np.zeros((0, 4), np.uint64))


@pytest.mark.parametrize("log_n,nin", [(6, 0), (9, 27)])
def test_satisfied_and_one_variable_changed(cg, tau, log_n, nin):
    sc = bu.synthetic_circuit(log_n, nin, seed=40 + log_n)
    h, pk_v, pk_s = keys_for(cg, tau, sc)
    ws, vs, ps, _ = batch(sc, [800, 801, 802])
    ev = cg.plonk_check_witness_batch(pk_s, ws, ps, 3)
    va = cg.plonk_check_witness_batch(pk_v, vs, ps, 3, input_form="vars")
    assert [verdict(f) for f in va] == [verdict(f) for f in ev]
    assert all(f.kind == 0 and f.copies_failed == 0 and f.gates_failed == 0 for f in va)
    d = cg.DevBuf.from_numpy(vs)
    assert [verdict(f) for f in cg.plonk_check_witness_batch(pk_v, d, ps, 3, input_form="vars")] == [verdict(f) for f in ev]
    assert np.array_equal(d.to_numpy().reshape(vs.shape), vs)
    d.free()
    # one variable's value changed: a gate fault, the same first row and count as for the expanded columns
    var = busy_variable(sc)
    wb, vb, pb = corrupted(sc, 801, var)
    ws[1], vs[1], ps[1] = wb, vb, pb
    ev = cg.plonk_check_witness_batch(pk_s, ws, ps, 3)
    va = cg.plonk_check_witness_batch(pk_v, vs, ps, 3, input_form="vars")
    assert ev[1].kind == 1 and ev[1].gates_failed >= 2 and ev[1].copies_failed == 0
    assert [verdict(f) for f in va] == [verdict(f) for f in ev]
    assert [f.kind for f in va] == [0, 1, 0]
    for pk in (pk_v, pk_s):
        cg.plonk_free_key(pk)
    cg.srs_free(h)


def test_precheck_names_the_proof_and_the_gate(cg, tau):
    sc = bu.synthetic_circuit(9, 27, seed=49)
    h, pk_v, pk_s = keys_for(cg, tau, sc)
    ws, vs, ps, bls = batch(sc, [810, 811, 812, 813])
    wb, vb, pb = corrupted(sc, 812, busy_variable(sc))
    row = cg.plonk_check_witness_batch(pk_s, wb[None], pb[None], 1)[0].row
    want = as_bytes(cg.plonk_prove_batch(pk_s, ws, ps, bls, b"m", 4))
    vs_bad, ps_bad = vs.copy(), ps.copy()
    vs_bad[2], ps_bad[2] = vb, pb
    cg.plonk_set_precheck(True)
    try:
        with pytest.raises(cg.CapGpuError) as e:
            cg.plonk_prove_batch(pk_v, vs_bad, ps_bad, bls, b"m", 4, input_form="vars")
        assert e.value.code == -7
        assert "1 of 4 witnesses" in str(e.value) and f"proof 2: gate {row} not satisfied" in str(e.value)
        assert as_bytes(cg.plonk_prove_batch(pk_v, vs, ps, bls, b"m", 4, input_form="vars")) == want
        # coalesced calls: the bad witness fails alone, with its own message
        T, bad_caller = 4, 2
        results = [None] * T
        start = threading.Barrier(T)

        def worker(t):
            start.wait()
            try:
                results[t] = cg.plonk_prove(pk_v, vs_bad[t], ps_bad[t], bls[t], b"m", input_form="vars")
            except cg.CapGpuError as err:
                results[t] = err

        cg.plonk_set_coalescing(2000, 16)
        try:
            threads = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
            for th in threads:
                th.start()
            for th in threads:
                th.join(timeout=300)
        finally:
            cg.plonk_set_coalescing(0)
        for t in range(T):
            if t == bad_caller:
                assert isinstance(results[t], cg.CapGpuError) and results[t].code == -7, results[t]
                assert f"proof 0: gate {row} not satisfied" in str(results[t])
            else:
                assert bytes(results[t]) == want[t], f"caller {t}"
    finally:
        cg.plonk_set_precheck(False)
    for pk in (pk_v, pk_s):
        cg.plonk_free_key(pk)
    cg.srs_free(h)


def test_key_with_a_table_still_reports_copy_faults_of_columns(cg, tau):
    sc = bu.synthetic_circuit(6, 3, seed=46)
    h, pk_v, pk_s = keys_for(cg, tau, sc)
    ws, _, ps, _ = batch(sc, [820, 821])
    # break one copy constraint and no gate: a cell of a padding row (all selectors zero) whose variable sits in other cells too
    wv = np.array(sc.wire_vars)
    counts = np.bincount(wv.reshape(-1))
    i, j = next((i, j) for i in range(5) for j in range(sc.n - 1, -1, -1) if counts[wv[i, j]] >= 2 and j >= sc.gate_rows)
    ws[1, i, j, 0] ^= 1
    a = cg.plonk_check_witness_batch(pk_s, ws, ps, 2)
    b = cg.plonk_check_witness_batch(pk_v, ws, ps, 2)
    assert [verdict(f) for f in a] == [verdict(f) for f in b]
    assert a[1].kind == 2 and a[1].copies_failed >= 1 and (a[1].wire, a[1].row) != (a[1].wire2, a[1].row2)
    assert a[0].kind == 0
    for pk in (pk_v, pk_s):
        cg.plonk_free_key(pk)
    cg.srs_free(h)
