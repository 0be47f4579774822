"""tests/lagrange_model.py against what is known in closed form about the Lagrange basis (`-m "not gpu"`): the model is
what the host twin and the GPU tests of the key builder compare with, so it is checked on its own first."""
import random

import numpy as np
import pytest

from tests import lagrange_model as M

R = M.R
SIZES = (0, 1, 2, 3, 6, 9)


def _naive(s, log_n):
    n = 1 << log_n
    w_inv = pow(M.omega(log_n), R - 2, R)
    n_inv = pow(n, R - 2, R)
    return [sum(pow(w_inv, i * j, R) * s[i] for i in range(n)) * n_inv % R for j in range(n)]


@pytest.mark.parametrize("log_n", SIZES)
def test_closed_form_outside_the_domain(log_n):
    """L_j(tau) = omega^j (tau^n - 1) / (n (tau - omega^j)) for a tau that is no n-th root of unity"""
    n = 1 << log_n
    om = M.omega(log_n)
    taus = [random.Random(3 + log_n).randrange(2, R), M.omega(log_n + 1), 0, R - 1 if n == 1 else 5]
    for tau in taus:
        if pow(tau, n, R) == 1:
            continue
        s = [pow(tau, i, R) for i in range(n + 3)]
        zh = (pow(tau, n, R) - 1) % R
        want = [pow(om, j, R) * zh % R * pow(n * (tau - pow(om, j, R)) % R, R - 2, R) % R for j in range(n)]
        want += [zh * pow(tau, e, R) % R for e in range(3)]
        assert M.expected_logs(s, log_n) == want, tau


@pytest.mark.parametrize("log_n", SIZES)
def test_families(log_n):
    n = 1 << log_n
    ran = set()
    for label in M.FAMILIES:
        s = M.family_logs(label, log_n)
        assert len(s) == n + 3 and all(0 <= x < R for x in s)
        L = M.expected_logs(s, log_n)
        assert len(L) == n + 3
        assert sum(L[:n]) % R == s[0], label                       # the basis sums to one: sum_j L_j = s_0
        if log_n <= 6:
            assert L[:n] == _naive(s, log_n), label
        if label.startswith("root:"):                               # tau = omega^k: the key is delta_k, no blinding
            k = M.root_index(label, log_n)
            assert M.family_tau(label, log_n) == pow(M.omega(log_n), k, R)
            assert L == [1 if j == k else 0 for j in range(n)] + [0, 0, 0], label
        elif label == "order_2n":
            tau = M.family_tau(label, log_n)
            assert pow(tau, n, R) == R - 1
            assert L[n:] == [(-2 * pow(tau, e, R)) % R for e in range(3)] and 0 not in L
        elif label == "zero":
            assert s == [1] + [0] * (n + 2)
            assert L == [pow(n, R - 2, R)] * n + [R - 1, 0, 0]
        elif label.startswith("single:"):
            assert sum(1 for x in s if x) == 1
        elif label == "all_zero":
            assert L == [0] * (n + 3)
        elif label == "sparse_random" and log_n >= 6:
            nz = [x for x in s if x]
            assert 0.1 * len(s) < len(s) - len(nz) < 0.45 * len(s)            # about a quarter at infinity
            assert len(set(nz)) < len(nz)                                      # equal entries
            assert any((R - x) in nz for x in nz)                              # opposite entries
        ran.add(label)
    assert ran == set(M.FAMILIES) and len(M.FAMILIES) == 12
    assert set(M.GENERATED) == {f for f in M.FAMILIES if M.family_tau(f, log_n) is not None}


def test_points_encode_zero_as_infinity():
    """0 maps to the all-zero (infinity) encoding, and the rest are the multiples of G the integer oracle gives"""
    from oracle import bn254 as bn
    from oracle import capref as cr
    logs = [0, 1, 2, R - 1, 0, 12345]
    pts = M.points(logs)
    assert not pts[0].any() and not pts[4].any()
    for s, p in zip(logs, pts):
        assert cr.affine_to_ints(p) == (bn.g1_mul(bn.G1_GEN, s) if s else None)
    assert np.array_equal(pts[3][:4], pts[1][:4]) and not np.array_equal(pts[3][4:], pts[1][4:])    # -G


def test_commit_log_is_the_inner_product():
    key = [3, 0, R - 1, 7]
    assert M.commit_log(key, [5, 9, 2, 1]) == (15 - 2 + 7) % R
