"""The block verifier's seed, weights and fold on the MI355X, kernel by kernel: capgpu_plonk_verify_block_* shows two
verdicts, and a fold whose weights were all equal - or whose seed never reached k_verify_weights - would give the same
ones on every block with at most one bad proof.  tests/hip/verifycheck - built by build() from the kernels' own header
(cap_amd/csrc/verify_kernels.hpp), launched through verify_launch.hpp as verify_block launches them, its keys made by
vf::dev_vk_fill as capgpu_plonk_vk_upload makes them - runs the cases of tests/verify_block_model.py and dumps, per case,
the validity flags, the u bytes, the 34 scalars of every proof, the seed S, the weights, the gathered points and scalars
of the two MSMs and the two sums A and -B.  Every word is compared with the model's Python integers
(tests/test_verify_block_model.py checks the model against the oracle without a GPU), and the bytes behind every buffer
must still hold the sentinel.  One case holds real proofs: there Python also checks tau A == B, and tau A != B once one
opening is W + [777] G.

The binary runs ONCE, as one fresh child process under its own time limit; the tests only parse its result file.
TIME_LIMIT_S is the floor tests/test_gpu_devcheck.py uses for a binary of this kind; MEASURED_S is the binary's wall time
on the MI355X (0.47 s for the 23 cases, 1.1 MB of case file), below a fifth of the limit."""
import os
import subprocess
import time

import pytest

from oracle import bn254 as bn
from oracle import capref as cr
from tests import verify_block_model as vm
from tests.test_gpu_verify_block import Env

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "hip", "verifycheck")
MEASURED_S = 0.47
TIME_LIMIT_S = 60.0


def real_cases(cg, tau):
    """five proofs of cg.plonk_prove under two keys (n = 2^8 with 4 inputs, n = 2^7 with none), and the same block with
    proof 3's opening moved by D = [777] G"""
    env = Env(cg, tau)
    try:
        keys = [vm.Key.from_ctypes(k[1]) for k in env.keys]
        key_of = [0, 1, 0, 0, 1]
        proofs, pubs_raw, msgs = [], [], []
        for i, k in enumerate(key_of):
            msg = b"real-%d" % i if i % 2 else None
            pr, pubs = env.prove(k, 1200 + i, msg)
            proofs.append(vm.Proof.from_bytes(bytes(pr)))
            pubs_raw.append(cr.array_to_ints(pubs) if pubs.size else [])
            msgs.append(msg)
    finally:
        for h in env.vkh:
            cg.plonk_vk_release(h)
        for pkh, _ in env.keys:
            cg.plonk_free_key(pkh)
        cg.srs_free(env.srs)
    moved = list(proofs)
    w = vm.point_value(proofs[3].pts[11])
    w = bn.g1_add(w, bn.g1_mul(bn.G1_GEN, 777))
    moved[3] = vm.Proof(list(proofs[3].pts), list(proofs[3].ev))
    moved[3].pts[11] = (vm.mont(w[0], bn.P), vm.mont(w[1], bn.P))
    return [vm.Case("real proofs", keys, key_of, pubs_raw, proofs, msgs),
            vm.Case("real proofs, one opening moved by [777] G", keys, key_of, pubs_raw, moved, msgs)]


@pytest.fixture(scope="module")
def run(cg, tau, tmp_path_factory):
    assert os.path.exists(EXE), "tests/hip/verifycheck is missing: build() makes it (make -C cap_amd/csrc)"
    d = tmp_path_factory.mktemp("verifycheck")
    cases = vm.make_cases() + real_cases(cg, tau)
    inp, res = str(d / "cases.bin"), str(d / "results.bin")
    vm.write_cases(inp, cases)
    t0 = time.time()
    try:
        out = subprocess.run([EXE, inp, res], capture_output=True, text=True, timeout=TIME_LIMIT_S)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"verifycheck did not finish within {TIME_LIMIT_S} s: {(e.stderr or b'')[-800:]}")
    wall = time.time() - t0
    print(f"verifycheck: {len(cases)} cases, {os.path.getsize(inp) / 1e6:.1f} MB, wall time {wall:.2f} s")
    assert out.returncode == 0, f"verifycheck ended with {out.returncode}: {out.stderr[-1200:]}"
    dumps = vm.read_results(res, cases)
    os.remove(inp)
    os.remove(res)
    models = [vm.block(c.keys, c.key_of, c.pubs_raw, c.proofs, c.msgs) for c in cases]
    return {"rows": list(zip(cases, dumps, models)), "wall": wall}


def test_every_dumped_word_matches_the_model(run):
    """valid, u bytes, scalars, S, weights (Montgomery images of the rule's values), gathered points and scalars, A and
    -B, bit for bit; an invalid proof's scalars, u bytes and gathered entries all zero; the guards intact"""
    bad = [line for c, d, m in run["rows"] for line in vm.check_case(c, d, m)]
    assert not bad, f"{len(bad)} complaints, first:\n" + "\n".join(bad[:12])


def test_weights_follow_the_rule_and_differ(run):
    """r_0 = 1 and every other weight is the 128-bit value of its own hash: stated here apart from the model's code, and
    all of a block's weights are distinct (a fold with equal weights accepts the forged pairs of
    tests/test_gpu_verify_forged.py)"""
    import struct
    for c, d, m in run["rows"]:
        w = [bn.from_mont(x, bn.R) for x in cr.array_to_ints(d.w)]
        assert w[0] == 1, c.name
        S = bn.keccak256(bytes(d.ubytes))
        assert d.S == S, c.name
        for i in range(1, len(w)):
            assert w[i] == int.from_bytes(bn.keccak256(S + struct.pack("<Q", i))[:16], "little"), (c.name, i)
        assert len(set(w)) == len(w), c.name


def test_invalid_proofs_leave_zeros(run):
    seen = 0
    for c, d, m in run["rows"]:
        count = len(c.proofs)
        for i in range(count):
            if m.valid[i]:
                continue
            seen += 1
            assert d.valid[i] == 0 and d.ubytes[32 * i:32 * i + 32] == bytes(32), (c.name, i)
            assert not d.sc[vm.TERMS * i:vm.TERMS * (i + 1)].any(), (c.name, i)
            own = list(range(2 * i, 2 * i + 2)) + list(range(2 * count + 13 * i, 2 * count + 13 * i + 13))
            assert not d.pts[own].any() and not d.msc[own].any(), (c.name, i)
    assert seen >= 15
    c, d, m = next(r for r in run["rows"] if r[0].name == "three keys, the middle one without a valid proof")
    at = 15 * len(c.proofs) + 19
    assert not d.msc[at:at + 19].any() and d.pts[at:at + 19].any(axis=1).all()
    c, d, m = next(r for r in run["rows"] if r[0].name == "every proof invalid")
    assert not d.ab.any() and not d.msc.any()
    c, d, m = next(r for r in run["rows"] if r[0].name.startswith("both openings at infinity"))
    assert not d.ab[0].any() and d.ab[1].any()


def test_real_proofs_pair_up_and_a_moved_opening_does_not(run, tau):
    by_name = {c.name: d for c, d, m in run["rows"]}
    good, moved = by_name["real proofs"], by_name["real proofs, one opening moved by [777] G"]
    for d in (good, moved):
        assert d.rc == 0 and list(d.valid) == [1] * 5

    def pairs_up(d):
        a, nb = cr.affine_to_ints(d.ab[0]), cr.affine_to_ints(d.ab[1])
        return bn.g1_mul(a, tau) == bn.g1_neg(nb)
    assert pairs_up(good)
    assert not pairs_up(moved)


def test_the_run_stays_below_a_fifth_of_its_limit(run):
    assert run["wall"] < TIME_LIMIT_S / 5, f"verifycheck took {run['wall']:.2f} s: split the case file"
