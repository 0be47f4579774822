"""k_quotient's permutation terms with beta folded out: u_j = (w_j + gamma) / beta, the factors u_j + k_j x (k_j x from
columns 18 .. 21 of the key's coset table) and u_j + sigma_j, and alpha beta^5 in front (cap_amd/csrc/plonk_kernels.hpp; the
identity itself: tests/test_quotient_fold_identity.py).  The quotient is the same polynomial, so every proof must stay what it
was, byte for byte: the C oracle's - under both transcripts (each derives 1 / beta and alpha beta^5 itself), for a two-key
batch (every key brings its own table), for a key made under the reference schedule (the four columns are filled per
launch), with CAPGPU_QUOT_FOLD=0 (the direct form for every proof) and =2 (every 1 / beta zeroed: the route a proof with beta = 0
takes), and a run after capgpu_plonk_reserve still grows nothing."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from cap_amd import bench_utils as bu
from tests import helpers as H
from tests.test_gpu_pi_fold import make_case, oracle_points, pubs_arr, transcript

pytestmark = pytest.mark.gpu


@contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def check_against_oracle(cg, case, msg, P):
    sc, h, pkh, key, ws, ps, bls = case
    proofs = cg.plonk_prove_batch(pkh, ws, ps, bls, msg, P)
    want = oracle_points(key, ws, ps, bls, msg)
    for p in range(P):
        assert H.proof_points(proofs[p]) == want[p], f"proof {p}"


def free(cg, case):
    cg.plonk_free_key(case[2])
    cg.srs_free(case[1])


# the shapes of tests/test_gpu_pi_fold.py
@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("log_n,nin,P", [(4, 1, 1), (5, 0, 2), (6, 27, 3), (11, 5, 2)])
def test_proofs_equal_the_c_oracles(cg, tau, log_n, nin, P, mode):
    case = make_case(cg, tau, log_n, nin, P, seed=170 + log_n)
    with transcript(cg, mode):
        check_against_oracle(cg, case, b"quot-fold", P)
    free(cg, case)


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("fold", [0, 2])
def test_direct_form(cg, tau, fold, mode):
    """CAPGPU_QUOT_FOLD (read per call) = 0: the direct form for every proof and no folded launch; = 2: every proof's
    1 / beta is zeroed, so the folded launch leaves all of them to the direct launch behind it - the route of a proof with
    beta = 0.  The instantiations are counted under their own names: k_quotient is k_quotient<true>, k_quotient_direct
    is k_quotient<false>."""
    log_n, nin, P = 6, 27, 3
    case = make_case(cg, tau, log_n, nin, P, seed=176)
    cg.profile_enable(True)
    try:
        with env(CAPGPU_QUOT_FOLD=fold), transcript(cg, mode):
            cg.profile_reset()
            check_against_oracle(cg, case, b"quot-fold", P)
            st = cg.profile_stats()
    finally:
        cg.profile_enable(False)
    folded = st.get("k_quotient", (0.0, 0))[1]
    direct = st.get("k_quotient_direct", (0.0, 0))[1]
    assert direct >= 1, st
    assert folded == (direct if fold == 2 else 0), (folded, direct)
    free(cg, case)


def test_default_is_the_folded_form(cg, tau):
    """no variable set: the folded launch; under the host transcript, outside a captured graph, no direct launch behind it
    (no beta is 0) - a batch above the largest one replayed as a graph"""
    log_n, nin, P = 5, 2, 66
    case = make_case(cg, tau, log_n, nin, 2, seed=179)
    sc, h, pkh, key, ws, ps, bls = case
    ws, ps, bls = (np.concatenate([a] * (P // 2)) for a in (ws, ps, bls))
    cg.profile_enable(True)
    try:
        with transcript(cg, "host"):
            cg.profile_reset()
            proofs = cg.plonk_prove_batch(pkh, ws, ps, bls, b"default", P)
            st = cg.profile_stats()
    finally:
        cg.profile_enable(False)
    want = oracle_points(key, ws[:2], ps[:2], bls[:2], b"default")
    for p in range(P):
        assert H.proof_points(proofs[p]) == want[p % 2], f"proof {p}"
    assert st["k_quotient"][1] >= 1 and st.get("k_quotient_direct", (0.0, 0))[1] == 0, st
    free(cg, case)


def test_key_of_the_reference_schedule(cg, tau):
    """CAPGPU_RECOMPUTE_PK_COSET=1 at preprocessing: the key holds no coset table, the columns are made per launch"""
    log_n, nin, P = 5, 2, 2
    with env(CAPGPU_RECOMPUTE_PK_COSET=1):
        case = make_case(cg, tau, log_n, nin, P, seed=177)
    check_against_oracle(cg, case, b"recompute", P)
    free(cg, case)


def test_two_keys_in_one_batch(cg, tau):
    """one batch, one domain, two circuits: a proof reads the k_j x columns of its own key's table; each proof equals the
    oracle's for its key"""
    log_n, n = 5, 1 << 5
    srs = cg.srs_generate(tau, n + 3)
    from oracle import capref as cr
    srs_host = cg.srs_download(srs, 0, n + 3)
    circuits = [bu.synthetic_circuit(log_n, ni, seed=seed) for ni, seed in ((3, 191), (1, 192))]
    keys = [cg.plonk_preprocess(srs, n, sc.num_inputs, sc.selectors_mont(), sc.sigma_mont())[0] for sc in circuits]
    okeys = [cr.PlonkKey(srs_host, n, sc.num_inputs, sc.selectors_mont(), sc.sigma_mont()) for sc in circuits]
    order = [1, 0, 0, 1]
    wires, rows, blinds, msgs, want = [], [], [], [], []
    for i, k in enumerate(order):
        sc = circuits[k]
        w, pubs = sc.witness(700 + i)
        bl = bu.to_mont_array(bu.blinders(800 + i))
        row = np.full((3, 4), 0xFFFF, np.uint64)
        row[:len(pubs)] = bu.to_mont_array(pubs)
        wires.append(sc.wires_mont(w)); rows.append(row); blinds.append(bl); msgs.append(b"note-%d" % i)
        want.append(oracle_points(okeys[k], [sc.wires_mont(w)], [pubs_arr(pubs)], [bl], msgs[i])[0])
    got = cg.plonk_prove_multi([keys[k] for k in order], np.stack(wires), np.stack(rows), np.stack(blinds), msgs)
    for i in range(len(order)):
        assert H.proof_points(got[i]) == want[i], i
    for pkh in keys:
        cg.plonk_free_key(pkh)
    cg.srs_free(srs)


@pytest.mark.parametrize("recompute", [0, 1])
def test_a_reserved_run_grows_nothing(cg, tau, recompute):
    """the four columns are part of what capgpu_plonk_reserve sizes (the reference schedule carries them in the batch's
    workspace)"""
    log_n, nin, P = 6, 4, 4
    with env(CAPGPU_RECOMPUTE_PK_COSET=recompute):
        case = make_case(cg, tau, log_n, nin, P, seed=178 + recompute)
    sc, h, pkh, key, ws, ps, bls = case
    cg.set_device(0)
    try:
        cg.trim()
        cg.plonk_reserve(pkh, P, "evals", slot=0)
        g0 = cg.scratch_stats()
        check_against_oracle(cg, case, b"reserve", P)
        g1 = cg.scratch_stats()
        assert g1["grow_events"] == g0["grow_events"] and g1["grow_bytes"] == g0["grow_bytes"], (g0, g1)
    finally:
        cg.set_device(-1)
    free(cg, case)
