"""One proof at n = 2^16, the size bench.py reports a rate for ("the reference's own bench depth") and the first at which
k_scan_totals takes a second trip round its 64-block loop (round 5's suffix scan: 65539 elements, 65 blocks; round 2's
scans: exactly 64), k_powers_small reaches exponents of 2^16, k_eval_partial runs 16 chunks of 4097 elements and the
five-coset transforms run at log_m = 17 inside a proof.  The C oracle needs about 50 s for the key and the proof at this
size, so its values are a fixture (tests/golden/proof_log16.json, written by tests/golden/make_golden.py)."""
import numpy as np
import pytest

from cap_amd import bench_utils as bu
from oracle import capref as cr
from tests import helpers as H
from tests.test_gpu_transcript import both_modes, key_of, pubs_arr, verifies

pytestmark = pytest.mark.gpu


def test_golden_proof_log16_in_both_transcript_modes(cg, tau):
    g = H.load_golden("proof_log16.json")
    assert g["log_n"] == 16
    sc = bu.synthetic_circuit(g["log_n"], g["num_inputs"], seed=g["circuit_seed"])
    h, pk, vk = key_of(cg, tau, sc)
    vk_pts = [cr.affine_to_ints(np.ctypeslib.as_array(vk.selector_comms[i])) for i in range(13)] + \
             [cr.affine_to_ints(np.ctypeslib.as_array(vk.sigma_comms[i])) for i in range(5)]
    assert vk_pts == [H.unhex_pt(p) for p in g["selector_comms"] + g["sigma_comms"]]
    assert vk.domain_size == sc.n == 1 << 16 and vk.num_inputs == g["num_inputs"]
    insts = [sc.witness(g["witness_seed"]), sc.witness(g["witness_seed"] + 1)]
    ws = np.stack([sc.wires_mont(w) for w, _ in insts])
    ps = np.stack([pubs_arr(pubs) for _, pubs in insts])
    bs = np.stack([bu.to_mont_array(bu.blinders(g["blinder_seed"] + i)) for i in range(2)])
    msg = g["ext_msg"].encode()
    exp_pts = [H.unhex_pt(p) for p in g["wires_poly_comms"]] + [H.unhex_pt(g["prod_perm_poly_comm"])] + \
        [H.unhex_pt(p) for p in g["split_quot_poly_comms"]] + [H.unhex_pt(g["opening_proof"]),
                                                              H.unhex_pt(g["shifted_opening_proof"])]
    exp_ev = [int(x, 16) for x in g["wires_evals"] + g["wire_sigma_evals"] + [g["perm_next_eval"]]]
    for mode, proofs in zip(("host", "device"), both_modes(cg, lambda: cg.plonk_prove_batch(pk, ws, ps, bs, msg, 2))):
        pts, ev = H.proof_points(proofs[0])
        assert pts == exp_pts, f"{mode} transcript: the commitments of proof 0 differ from the oracle's"
        assert ev == exp_ev, f"{mode} transcript: the evaluations of proof 0 differ from the oracle's"
        assert verifies(cg, tau, vk, ps[1], proofs[1], msg), f"{mode} transcript: proof 1 is not accepted"
        assert not verifies(cg, tau, vk, ps[0], proofs[1], msg), f"{mode} transcript: proof 1 passes with proof 0's inputs"
    cg.plonk_free_key(pk)
    cg.srs_free(h)
