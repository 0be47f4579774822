"""The device prover never takes the public-input polynomial PI(X) to the 6n quotient domain (cap_amd/csrc/prove_run.hpp:
pi_fold).  PI enters the numerator N = N' + PI linearly, the interpolation over the coset 5 <omega_6n> is linear, and every
point of that coset has x^(6n) = C := 5^(6n), hence

    1 / (x^n - 1) = (1 + x^n + ... + x^(5n)) / (C - 1)        on the coset,

so the interpolant of PI(x) / Z_H(x) is kappa PI(X) (1 + X^n + ... + X^(5n)), kappa = 1 / (C - 1): degree < 6n, hence THE
interpolant.  In coefficients  t[j n + i] = t'[j n + i] + kappa PI_i,  j < 6, i < n,  where t' is interpolated from the
numerator without PI.  This CPU test pins that with Python integers against the oracle's quotient (which evaluates PI on
8n points like the reference), following tests/test_quotient_domain.py."""
import functools

from cap_amd import bench_utils as bu
from oracle import bn254 as bn
from oracle import plonk as pl
from tests.test_quotient_domain import root_6n

R = bn.R
LOG_N = 3
N = 1 << LOG_N
BIG = 6 * N
DEG = 5 * (N + 1) + 2


@functools.lru_cache(maxsize=None)
def quotient_without_pi(nin):
    """(t' = the 6n interpolation of the quotient identity with the PI term left out, kappa * PI coefficients [n], the
    oracle's t_poly) for a satisfied n = 8 circuit with `nin` public inputs"""
    sc = bu.synthetic_circuit(LOG_N, nin, seed=5)
    c = pl.Circuit(n=N, num_inputs=nin, selectors=sc.selectors, sigma=sc.sigma)
    pk = pl.preprocess(c, 987654321)
    w, pubs = sc.witness(11)
    tr = {}
    pl.prove(pk, w, pubs, bu.blinders(12), ext_msg=b"x", trace=tr)
    beta, gamma, alpha = tr["beta"], tr["gamma"], tr["alpha"]
    wN, _ = root_6n(LOG_N)
    g = bn.FR_GENERATOR
    pts = [g * pow(wN, i, R) % R for i in range(BIG)]
    ev = lambda poly: [bn.poly_eval(poly, x) for x in pts]
    sel_c = [ev(p) for p in pk.selector_polys]
    sig_c = [ev(p) for p in pk.sigma_polys]
    w_c = [ev(p) for p in tr["wire_polys"]]
    z_c = ev(tr["z_poly"])
    quot = []
    for i, x in enumerate(pts):
        wv = [w_c[j][i] for j in range(5)]
        t_circ = pl.gate_eval([sel_c[s][i] for s in range(13)], wv, 0)           # no PI(x)
        a, b = z_c[i], z_c[(i + 6) % BIG]
        for j in range(5):
            a = a * ((wv[j] + beta * pl.K[j] * x + gamma) % R) % R
            b = b * ((wv[j] + beta * sig_c[j][i] + gamma) % R) % R
        l1 = alpha * alpha % R * (z_c[i] - 1) % R * pow(N * (x - 1) % R, R - 2, R) % R
        zh_inv = pow((pow(x, N, R) - 1) % R, R - 2, R)
        quot.append(((t_circ + alpha * (a - b)) % R * zh_inv + l1) % R)
    inv_big = pow(BIG, R - 2, R)
    winv, ginv = pow(wN, R - 2, R), pow(g, R - 2, R)
    t6 = []
    for k in range(BIG):
        acc = 0
        for i in range(BIG):
            acc = (acc + quot[i] * pow(winv, i * k % BIG, R)) % R
        t6.append(acc * inv_big % R * pow(ginv, k, R) % R)
    kappa = pow((pow(g, BIG, R) - 1) % R, R - 2, R)
    pi = list(tr["pi_poly"]) + [0] * N
    assert all(v == 0 for v in pi[N:])                                           # PI has degree < n
    return tuple(t6), tuple(kappa * v % R for v in pi[:N]), tuple(tr["t_poly"])


def folded(t6, kpi, skip_block=None):
    return [(t6[j * N + i] + (0 if j == skip_block else kpi[i])) % R for j in range(6) for i in range(N)]


def equals_oracle(t, t_ref):
    return (t[:DEG + 1] == list(t_ref[:DEG + 1]) and t[DEG] != 0 and all(v == 0 for v in t[DEG + 1:])
            and all(v == 0 for v in t_ref[DEG + 1:]))


def test_two_public_inputs():
    t6, kpi, t_ref = quotient_without_pi(2)
    assert any(kpi)
    assert equals_oracle(folded(t6, kpi), t_ref)
    # without the addend t' is not the quotient (at n = 8 the degree 5 (n + 1) + 2 = 6n - 1 leaves no coefficient above it
    # to look at; on larger domains the addend is also what cancels the top block's coefficients)
    assert not equals_oracle(list(t6), t_ref)


def test_no_public_inputs():
    t6, kpi, t_ref = quotient_without_pi(0)
    assert not any(kpi)
    assert equals_oracle(folded(t6, kpi), t_ref) and equals_oracle(list(t6), t_ref)


def test_every_block_needs_the_addend():
    t6, kpi, t_ref = quotient_without_pi(2)
    for j in range(6):
        assert not equals_oracle(folded(t6, kpi, skip_block=j), t_ref), j
