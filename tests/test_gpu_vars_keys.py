"""Keys that know their circuit's wire -> variable table (capgpu_plonk_preprocess_vars / capgpu_plonk_key_set_vars).
The extended permutation is built on the device from the table; the expected one always comes from
bench_utils._permutation / SyntheticCircuit.sigma_mont() - CPU code on Python integers - through the key that
capgpu_plonk_preprocess makes of it: vk and serialised key must be the same bytes."""
import numpy as np
import pytest

from cap_amd import bench_utils as bu
from tests.test_gpu_input_forms import instance, to_coeffs

pytestmark = pytest.mark.gpu


def sigma_of(wv, num_vars, log_n):
    n = 1 << log_n
    return np.concatenate([bu.to_mont_array(col) for col in bu._permutation(wv, num_vars, log_n)]).reshape(5, n, 4)


def key_bytes(cg, pk):
    return bytes(cg.plonk_key_serialize(pk, cg.g2_generator(), cg.g2_generator()))


@pytest.mark.parametrize("log_n,nin", [(4, 1), (6, 0), (9, 27), (12, 7)])
def test_key_from_table_equals_key_from_host_sigma(cg, tau, log_n, nin):
    sc = bu.synthetic_circuit(log_n, nin, seed=40 + log_n)
    n = sc.n
    h = cg.srs_generate(tau, n + 3)
    pk_s, vk_s = cg.plonk_preprocess(h, n, nin, sc.selectors_mont(), sc.sigma_mont())
    want_vk, want_key = bytes(vk_s), key_bytes(cg, pk_s)
    assert cg.plonk_key_num_vars(pk_s) == 0
    for form, sel in (("evals", sc.selectors_mont()), ("coeffs", to_coeffs(sc.selectors_mont(), log_n))):
        pk_v, vk_v = cg.plonk_preprocess_vars(h, n, nin, sel, np.array(sc.wire_vars), sc.num_vars, selector_form=form)
        assert bytes(vk_v) == want_vk, form
        assert key_bytes(cg, pk_v) == want_key, form
        assert cg.plonk_key_num_vars(pk_v) == sc.num_vars
        cg.plonk_free_key(pk_v)
    cg.plonk_free_key(pk_s)
    cg.srs_free(h)


def grouping_table(name):
    """(log_n, wire_vars 5 x n, num_vars): tables chosen to break a kernel that groups cells by variable"""
    n = 16
    if name == "one_cycle_of_80":
        return 4, [[0] * n for _ in range(5)], 1
    if name == "identity":
        return 4, [[i * n + j for j in range(n)] for i in range(5)], 5 * n
    if name == "one_cycle_of_5120":     # one run of the sorted keys over two and a half tiles of 2048
        return 10, [[0] * 1024 for _ in range(5)], 1
    if name == "padding_above_1024":    # the padding variable holds more than 1024 cells
        sc = bu.synthetic_circuit(9, 27, seed=5, fill=0.5)
        assert np.bincount(np.array(sc.wire_vars).reshape(-1)).max() > 1024
        return 9, sc.wire_vars, sc.num_vars
    if name == "padding_above_a_tile":  # ... and here more than one tile of the sort (2048 keys)
        sc = bu.synthetic_circuit(10, 27, seed=5, fill=0.5)
        assert np.bincount(np.array(sc.wire_vars).reshape(-1)).max() > 2048
        return 10, sc.wire_vars, sc.num_vars
    if name == "cycles_span_tiles":     # 20480 cells: ten tiles, cycles across them
        sc = bu.synthetic_circuit(12, 7, seed=52)
        return 12, sc.wire_vars, sc.num_vars
    sc = bu.synthetic_circuit(6, 0, seed=46)
    return 6, sc.wire_vars, 5 * sc.n + 1000  # "unused_ids"


@pytest.mark.parametrize("name", ["one_cycle_of_80", "identity", "one_cycle_of_5120", "padding_above_1024", "padding_above_a_tile",
                                  "cycles_span_tiles", "unused_ids"])
def test_tables_that_stress_the_grouping(cg, tau, name):
    log_n, wv, num_vars = grouping_table(name)
    n = 1 << log_n
    sel = bu.synthetic_circuit(log_n, 0, seed=40 + log_n).selectors_mont()  # any selectors: the permutation is under test
    h = cg.srs_generate(tau, n + 3)
    pk_s, vk_s = cg.plonk_preprocess(h, n, 0, sel, sigma_of(wv, num_vars, log_n))
    pk_v, vk_v = cg.plonk_preprocess_vars(h, n, 0, sel, np.array(wv), num_vars)
    assert bytes(vk_v) == bytes(vk_s)
    assert key_bytes(cg, pk_v) == key_bytes(cg, pk_s)
    # the same table twice gives the same key: nothing depends on the order blocks ran in
    pk_w, _ = cg.plonk_preprocess_vars(h, n, 0, sel, np.array(wv), num_vars)
    assert key_bytes(cg, pk_w) == key_bytes(cg, pk_v)
    for pk in (pk_s, pk_v, pk_w):
        cg.plonk_free_key(pk)
    cg.srs_free(h)


def test_bad_ids_and_set_vars(cg, tau):
    log_n, nin = 6, 3
    sc = bu.synthetic_circuit(log_n, nin, seed=46)
    n = sc.n
    h = cg.srs_generate(tau, n + 3)
    wv = np.array(sc.wire_vars, dtype=np.int64)
    # an id equal to num_vars is refused, naming the cell
    bad = wv.copy()
    bad[3, 17] = sc.num_vars
    with pytest.raises(cg.CapGpuError) as e:
        cg.plonk_preprocess_vars(h, n, nin, sc.selectors_mont(), bad, sc.num_vars)
    assert e.value.code == -1 and "(wire 3, row 17)" in str(e.value)
    # a key made from sigma takes the right table ...
    pk, _ = cg.plonk_preprocess(h, n, nin, sc.selectors_mont(), sc.sigma_mont())
    w, ps, bl = instance(sc, 7)
    want = bytes(cg.plonk_prove(pk, w, ps, bl, b"memo"))
    # ... but not one in which two cells of different variables are swapped: the key stays as it was and still proves
    swapped = wv.copy()
    cells = [(i, j) for i in range(5) for j in range(n)]
    shared = np.bincount(wv.reshape(-1)) >= 2  # (two lone cells swapped would be a renumbering, not another permutation)
    a = next(c for c in cells if shared[wv[c]])
    b = next(c for c in cells if wv[c] != wv[a])
    swapped[a], swapped[b] = wv[b], wv[a]
    with pytest.raises(cg.CapGpuError) as e:
        cg.plonk_key_set_vars(pk, swapped, sc.num_vars)
    assert e.value.code == -1 and "wire" in str(e.value) and "row" in str(e.value)
    assert cg.plonk_key_num_vars(pk) == 0
    assert bytes(cg.plonk_prove(pk, w, ps, bl, b"memo")) == want
    cg.plonk_key_set_vars(pk, wv, sc.num_vars)
    assert cg.plonk_key_num_vars(pk) == sc.num_vars
    assert bytes(cg.plonk_prove(pk, w, ps, bl, b"memo")) == want
    # a key that has a table takes a renumbered one (same grouping), and refuses a regrouped one
    cg.plonk_key_set_vars(pk, wv + 5, sc.num_vars + 5)
    assert cg.plonk_key_num_vars(pk) == sc.num_vars + 5
    with pytest.raises(cg.CapGpuError) as e:
        cg.plonk_key_set_vars(pk, swapped, sc.num_vars)
    assert e.value.code == -1
    assert cg.plonk_key_num_vars(pk) == sc.num_vars + 5
    cg.plonk_free_key(pk)
    cg.srs_free(h)
