"""k_quotient's permutation terms with beta folded out (cap_amd/csrc/plonk_kernels.hpp).  With u_j = (w_j + gamma) / beta,

    w_j + gamma + beta k_j x   = beta (u_j + k_j x),        w_j + gamma + beta sigma_j = beta (u_j + sigma_j),

so  alpha (z prod_j (w_j + gamma + beta k_j x) - z_w prod_j (w_j + gamma + beta sigma_j))
      = alpha beta^5 (z prod_j (u_j + k_j x) - z_w prod_j (u_j + sigma_j)):

five products by 1 / beta where the direct form multiplies by beta ten times (beta x, four k_j (beta x), five beta sigma_j),
k_j x read from a table of the key.  Pinned here on Python integers at random values and at the edges; beta = 0 has no
inverse and is routed to the direct form, as the kernel routes it (beta_inv = 0)."""
import random

from oracle import bn254 as bn
from oracle import plonk as pl

R = bn.R


def direct(alpha, beta, gamma, w, sig, x, z, zw):
    a, b = z, zw
    for j in range(5):
        a = a * ((w[j] + gamma + beta * pl.K[j] % R * x) % R) % R
        b = b * ((w[j] + gamma + beta * sig[j]) % R) % R
    return alpha * (a - b) % R


def folded(alpha_beta5, beta_inv, gamma, w, sig, kx, z, zw):
    """what the kernel computes: kx[j] = k_j x from the key's table (kx[0] = x), beta only through beta_inv and alpha beta^5"""
    a, b = z, zw
    for j in range(5):
        u = (w[j] + gamma) * beta_inv % R
        a = a * ((u + kx[j]) % R) % R
        b = b * ((u + sig[j]) % R) % R
    return alpha_beta5 * (a - b) % R


def routed(alpha, beta, gamma, w, sig, x, z, zw):
    """the kernel's choice: beta_inv = 0 stands for beta = 0 and takes the direct form"""
    beta_inv = pow(beta, R - 2, R) if beta else 0
    if beta_inv == 0:
        return "direct", direct(alpha, beta, gamma, w, sig, x, z, zw)
    kx = [pl.K[j] * x % R for j in range(5)]
    return "folded", folded(alpha * pow(beta, 5, R) % R, beta_inv, gamma, w, sig, kx, z, zw)


def draw(rng, edge):
    pick = (lambda: rng.choice([0, 1, R - 1])) if edge else (lambda: rng.randrange(R))
    return dict(alpha=pick(), gamma=pick(), w=[pick() for _ in range(5)], sig=[pick() for _ in range(5)], x=pick(),
                z=pick(), zw=pick())


def test_k0_is_one():
    assert pl.K[0] == 1                      # column j = 0 of the table is x itself: the kernel reads xs29 for it


def test_folded_form_equals_direct_form_at_random_values():
    rng = random.Random(2024)
    for it in range(300):
        v = draw(rng, edge=it < 60)
        beta = rng.choice([1, R - 1, 2]) if it < 60 else rng.randrange(1, R)
        path, got = routed(beta=beta, **v)
        assert path == "folded"
        assert got == direct(beta=beta, **v), it


def test_beta_zero_takes_the_direct_form():
    rng = random.Random(7)
    for it in range(20):
        v = draw(rng, edge=False)
        path, got = routed(beta=0, **v)
        assert path == "direct"
        # beta = 0: both products are z resp. z_w times prod (w_j + gamma)
        prod = 1
        for j in range(5):
            prod = prod * ((v["w"][j] + v["gamma"]) % R) % R
        assert got == v["alpha"] * (v["z"] - v["zw"]) % R * prod % R
        # and the folded formula fed beta_inv = 0 would NOT give it (why the kernel must branch)
        kx = [pl.K[j] * v["x"] % R for j in range(5)]
        assert got != 0 and folded(0, 0, v["gamma"], v["w"], v["sig"], kx, v["z"], v["zw"]) == 0
