"""The plain inverse transforms of two or more passes take their 1/n with the inter-pass twiddles of the first column pass
(ntt.hip: tw29_inv_n) and multiply by nothing in the row pass; one-pass transforms and coset inverses keep the product of
the row pass.  Whole outputs, bit for bit against the C restatement (oracle.capref.ntt_fr), at the one-pass size 2^4, the
first two-pass size 2^11 and the first three-pass size 2^21 - asserted through cg.ntt_plan -, plain and coset, in place on
the device (cg.ntt_fr_dev) and out of place through the host entry point (cg.ntt_fr_batch: the caller's arrays are left
alone, the results arrive in copies), 1 and 3 arrays per call; and forward after inverse = identity at the three-pass size.

The inputs are three of tools/ntt_conformance.py's: random data, r - 1 everywhere (a constant: its inverse transform is
that constant at index 0 and zero elsewhere, so every other output is a sum that cancels only if each product by
omega^-e / n is right, the entries at exponent 0 included) and x + r as the raw image of x.  The oracle's transforms - at
2^21 about a second each - are made once per (size, coset, input) and shared by the cases."""
import numpy as np
import pytest

from oracle import capref as cr
from tools import ntt_conformance as nc

pytestmark = pytest.mark.gpu

PICKS = [nc.INPUTS.index(k) for k in ("random", "all_rm1", "x_plus_r")]
PASSES = {4: 1, 11: 2, 21: 3}
_cache = {}


def inputs(log_n):
    """[(raw image for the device, array for the oracle)] x 3, made once per size and never written to"""
    if log_n not in _cache:
        made = [nc.make_input(log_n, k, 7) for k in PICKS]
        for raw, ref in made:
            raw.setflags(write=False)
            ref.setflags(write=False)
        _cache[log_n] = made
    return _cache[log_n]


def expected(log_n, count, coset):
    key = (log_n, coset)
    have = _cache.setdefault(key, [])
    while len(have) < count:
        have.append(cr.ntt_fr(inputs(log_n)[len(have)][1], log_n, True, coset).reshape(-1, 4))
    return have[:count]


def run(cg, log_n, count, coset, in_place):
    n = 1 << log_n
    assert cg.ntt_plan(log_n, count)["passes"] == PASSES[log_n]
    raws = [inputs(log_n)[b][0] for b in range(count)]
    want = expected(log_n, count, coset)
    if in_place:
        d = cg.DevBuf.from_numpy(np.stack(raws))
        cg.ntt_fr_dev(d, log_n, count=count, stride=n, inverse=True, coset=coset)
        got = list(d.to_numpy().reshape(count, n, 4))
        d.free()
    else:
        got = [g.reshape(n, 4) for g in cg.ntt_fr_batch(raws, log_n, True, coset)]
    for b in range(count):
        assert np.array_equal(got[b], want[b]), f"array {b} ({nc.INPUTS[PICKS[b]]})"


@pytest.mark.parametrize("in_place", [True, False])
@pytest.mark.parametrize("coset", [False, True])
@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("log_n", [4, 11])
def test_inverse_one_and_two_passes(cg, log_n, count, coset, in_place):
    run(cg, log_n, count, coset, in_place)


@pytest.mark.parametrize("in_place", [True, False])
@pytest.mark.parametrize("coset", [False, True])
@pytest.mark.parametrize("count", [1, 3])
def test_inverse_three_passes(cg, count, coset, in_place):
    run(cg, 21, count, coset, in_place)


def test_forward_after_inverse_is_the_identity_at_three_passes(cg):
    log_n, n = 21, 1 << 21
    x = inputs(log_n)[0][0]                      # canonical random data
    d = cg.DevBuf.from_numpy(x)
    cg.ntt_fr_dev(d, log_n, inverse=True)
    cg.ntt_fr_dev(d, log_n, inverse=False)
    got = d.to_numpy().reshape(n, 4)
    d.free()
    assert np.array_equal(got, x)
