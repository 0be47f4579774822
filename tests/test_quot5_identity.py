"""Round 3 on five of the six n-cosets (cap_amd/csrc/ntt.hpp: ntt3_forward5 / ntt3_inverse5,
plonk_kernels.hpp: k_quotient_top).  The quotient t has 5n + 8 coefficients.  With c_k = 5^n omega_6^k the value of x^n on
n-coset k, Mt(Y) = prod_{k<5} (Y - c_k) and h the top 8 coefficients, t = t_lo + Mt(X^n) h with deg t_lo < 5n, and Mt(X^n)
vanishes on the cosets k < 5: their 5n values determine t_lo.  h comes from the top coefficients of the polynomials in hand,
because t (X^n - 1) = N and t has nothing at or above degree 6n.  Python integers against the oracle's quotient, which is
interpolated on 8n points like the reference; the instance is a random satisfied circuit with blinders and public inputs."""
import functools

import pytest

from cap_amd import bench_utils as bu
from oracle import bn254 as bn
from oracle import plonk as pl
from tests.test_quotient_domain import root_6n

R = bn.R
G = bn.FR_GENERATOR
inv = lambda a: pow(a % R, R - 2, R)


@functools.lru_cache(maxsize=None)
def instance(log_n):
    n = 1 << log_n
    sc = bu.synthetic_circuit(log_n, 3, seed=40 + log_n)
    c = pl.Circuit(n=n, num_inputs=3, selectors=sc.selectors, sigma=sc.sigma)
    pk = pl.preprocess(c, 987654321)
    w, pubs = sc.witness(21)
    blind = bu.blinders(22)
    assert all(blind) and all(pubs)
    tr = {}
    pl.prove(pk, w, pubs, blind, ext_msg=b"q5", trace=tr)
    return n, pk, tr


def constants(log_n):
    n = 1 << log_n
    wN, _ = root_6n(log_n)
    c = [pow(G, n, R) * pow(wN, n * k, R) % R for k in range(6)]            # c_k = (5 omega_6n^k)^n
    mt = [1]
    for k in range(5):                                                       # Mt(Y) = prod_{k<5} (Y - c_k)
        mt = [((mt[j - 1] if j else 0) - (mt[j] if j < len(mt) else 0) * c[k]) % R for j in range(len(mt) + 1)]
    return n, wN, c, mt


def quotient_values_without_pi(log_n, k):
    """the values k_quotient computes on n-coset k: the numerator without PI over Z_H = c_k - 1, plus the L_1 term"""
    n, pk, tr = instance(log_n)
    _, wN, c, _ = constants(log_n)
    beta, gamma, alpha = tr["beta"], tr["gamma"], tr["alpha"]
    wn = pow(wN, 6, R)
    pts = [G * pow(wN, k, R) * pow(wn, m, R) % R for m in range(n)]
    ev = lambda poly: [bn.poly_eval(poly, x) for x in pts]
    sel = [ev(p) for p in pk.selector_polys]
    sig = [ev(p) for p in pk.sigma_polys]
    wv = [ev(p) for p in tr["wire_polys"]]
    z = ev(tr["z_poly"])
    zh_inv = inv(c[k] - 1)
    out = []
    for i, x in enumerate(pts):
        w = [wv[j][i] for j in range(5)]
        a, b = z[i], z[(i + 1) % n]                                          # z(omega x): the next element of the same coset
        for j in range(5):
            a = a * ((w[j] + beta * pl.K[j] * x + gamma) % R) % R
            b = b * ((w[j] + beta * sig[j][i] + gamma) % R) % R
        l1 = alpha * alpha % R * (z[i] - 1) % R * inv(n * (x - 1))
        out.append(((pl.gate_eval([sel[s][i] for s in range(13)], w, 0) + alpha * (a - b)) % R * zh_inv + l1) % R)
    return out


def series_mul(x, y, terms=8):
    return [sum(x[a] * y[k - a] for a in range(k + 1)) % R for k in range(terms)]


def top_coefficients(log_n):
    """h as k_quotient_top computes it: series from the top down, truncated at 8 terms"""
    n, pk, tr = instance(log_n)
    beta, alpha = tr["beta"], tr["alpha"]
    omega = pow(root_6n(log_n)[0], 6, R)
    coef = lambda poly, d: poly[d] if 0 <= d < len(poly) else 0
    W = [[coef(tr["wire_polys"][j], n + 1 - k) for k in range(8)] for j in range(5)]
    B = [[(W[j][k] + beta * coef(pk.sigma_polys[j], n + 1 - k)) % R for k in range(8)] for j in range(5)]
    Z = [coef(tr["z_poly"], n + 2 - k) for k in range(8)]
    Zw = [coef(tr["z_poly"], n + 2 - k) * pow(omega, n + 2 - k, R) % R for k in range(8)]
    h = [0] * 8
    for i in range(4):                                                       # q_hash_i w_i^5: degree 6n + 4 - k <-> h_(4-k)
        w2 = series_mul(W[i], W[i])
        s = series_mul(series_mul(series_mul(w2, w2), W[i]), [coef(pk.selector_polys[6 + i], n - 1 - k) for k in range(8)])
        for k in range(5):
            h[4 - k] = (h[4 - k] + s[k]) % R
    pw = functools.reduce(series_mul, W)
    s = series_mul(pw, [coef(pk.selector_polys[12], n - 1 - k) for k in range(8)])
    for k in range(5):
        h[4 - k] = (h[4 - k] + s[k]) % R
    pa = series_mul(pw, Z)                                                   # beta k_j X and gamma do not reach (n >= 16)
    pb = series_mul(functools.reduce(series_mul, B), Zw)
    for k in range(8):                                                       # degree 6n + 7 - k <-> h_(7-k)
        h[7 - k] = (h[7 - k] + alpha * (pa[k] - pb[k])) % R
    return h


@pytest.mark.parametrize("log_n", [4, 5])
def test_top_coefficients_from_the_polynomials(log_n):
    n, _, tr = instance(log_n)
    t_ref = list(tr["t_poly"])
    assert top_coefficients(log_n) == t_ref[5 * n:5 * n + 8]
    assert t_ref[5 * n + 7] != 0 and not any(t_ref[5 * n + 8:])


@pytest.mark.parametrize("log_n", [4, 5])
def test_five_cosets_and_the_addends_give_the_quotient(log_n):
    n, wN, c, mt = constants(log_n)
    _, _, tr = instance(log_n)
    t_ref = list(tr["t_poly"]) + [0] * (6 * n - len(tr["t_poly"]))   # (the oracle's array has the length of its 8n domain)
    assert not any(t_ref[6 * n:])
    t_ref = t_ref[:6 * n]
    wn_inv = inv(pow(wN, 6, R))
    rho = []
    for k in range(5):                                                       # inverse n-point transform, un-scaled
        q = quotient_values_without_pi(log_n, k)
        s_inv = inv(G * pow(wN, k, R))
        rho.append([sum(q[m] * pow(wn_inv, i * m % n, R) for m in range(n)) % R * inv(n) % R * pow(s_inv, i, R) % R
                    for i in range(n)])
    # rho_k[i] = sum_j c_k^j u[j n + i]: the fixed 5 x 5 Vandermonde system, solved by Lagrange's basis polynomials
    basis = []
    for k in range(5):
        num, den = [1], 1
        for l in range(5):
            if l != k:
                num = [((num[j - 1] if j else 0) - (num[j] if j < len(num) else 0) * c[l]) % R for j in range(len(num) + 1)]
                den = den * (c[k] - c[l]) % R
        basis.append([v * inv(den) % R for v in num])
    u = [sum(basis[k][j] * rho[k][i] for k in range(5)) % R for j in range(5) for i in range(n)]
    # the public-input addend: kappa (1 + Y + ... + Y^5) - kappa Mt(Y) = kappa D(Y), D of degree 4; d_j = 1 - mt_j
    kappa = inv(pow(G, 6 * n, R) - 1)
    pi = list(tr["pi_poly"])[:n]
    assert any(pi) and not any(list(tr["pi_poly"])[n:])
    h = top_coefficients(log_n)
    t = [0] * (6 * n)
    for j in range(5):
        for i in range(n):
            t[j * n + i] = (u[j * n + i] + kappa * (1 - mt[j]) * pi[i] + (mt[j] * h[i] if i < 8 else 0)) % R
    t[5 * n:5 * n + 8] = h
    assert mt[5] == 1 and t == t_ref
    # each part is needed: without the public-input addend, or without Mt h, it is another polynomial
    assert [(u[k] + (mt[k // n] * h[k % n] if k % n < 8 else 0)) % R for k in range(5 * n)] != t_ref[:5 * n]
    assert [(t[k] - (mt[k // n] * h[k % n] if k % n < 8 else 0)) % R for k in range(5 * n)] != t_ref[:5 * n]


@pytest.mark.parametrize("log_n", [4, 5])
def test_split_solve_of_the_two_block_route(log_n):
    """Blocks 0 and 1 as inverse 2n-point transforms: E_a = u_0 + c_a^2 u_2 + c_a^4 u_4, O_a = u_1 + c_a^2 u_3 - the odd
    coefficients from a 2 x 2 system of their own (Quot5Const::odd), the even ones from E_0, E_1 and R less its odd part."""
    n, _, c, _ = constants(log_n)
    assert c[3] == R - c[0] and c[4] == R - c[1] and len(set(c)) == 6
    rng = bn.SplitMix64(7)
    u = [rng.field(R) for _ in range(5)]
    E = [(u[0] + c[a] ** 2 * u[2] + c[a] ** 4 * u[4]) % R for a in range(2)]
    O = [(u[1] + c[a] ** 2 * u[3]) % R for a in range(2)]
    Rv = sum(pow(c[2], j, R) * u[j] for j in range(5)) % R
    # values of u on the cosets a and a + 3 are E_a +- c_a O_a: the 2n-point transform carries both
    for a in range(2):
        for sign, k in ((1, a), (-1, a + 3)):
            assert (E[a] + sign * c[a] * O[a]) % R == sum(pow(c[k], j, R) * u[j] for j in range(5)) % R
    u3 = (O[0] - O[1]) * inv(c[0] ** 2 - c[1] ** 2) % R
    u1 = (O[0] - c[0] ** 2 * u3) % R
    assert (u1, u3) == (u[1], u[3])
    rest = (Rv - c[2] * u1 - pow(c[2], 3, R) * u3) % R                       # u_0 + c_2^2 u_2 + c_2^4 u_4
    y = [c[0] ** 2 % R, c[1] ** 2 % R, c[2] ** 2 % R]
    v = [E[0], E[1], rest]
    got = [0, 0, 0]
    for k in range(3):                                                       # Lagrange on the three squares
        num, den = [1], 1
        for l in range(3):
            if l != k:
                num = [((num[j - 1] if j else 0) - (num[j] if j < len(num) else 0) * y[l]) % R for j in range(len(num) + 1)]
                den = den * (y[k] - y[l]) % R
        for j in range(3):
            got[j] = (got[j] + num[j] * inv(den) * v[k]) % R
    assert got == [u[0], u[2], u[4]]


@pytest.mark.parametrize("log_n", [4, 5])
def test_fold_of_block_two(log_n):
    """The even elements of block 2 are an n-point transform of the polynomial folded modulo X^n - s_2^n: pre-scaled
    coefficients n, n + 1 (n + 2 for z) are added onto pre-scaled coefficients 0, 1 (2)."""
    n, wN, _, _ = constants(log_n)
    _, _, tr = instance(log_n)
    s2 = G * pow(wN, 2, R) % R
    wn = pow(wN, 6, R)
    for poly in (list(tr["z_poly"]), list(tr["wire_polys"][3])):
        assert n < len(poly) <= n + 3 and poly[-1] != 0
        scaled = [v * pow(s2, i, R) % R for i, v in enumerate(poly)]
        folded = [(scaled[i] + (scaled[n + i] if n + i < len(poly) else 0)) % R for i in range(n)]
        for m in (0, 1, n // 2 + 1, n - 1):
            # element 2m of block 2 of the 2n-point transform: s_2 omega_2n^(2m) = s_2 omega_n^m
            assert sum(folded[i] * pow(wn, i * m % n, R) for i in range(n)) % R == bn.poly_eval(poly, s2 * pow(wn, m, R) % R)
