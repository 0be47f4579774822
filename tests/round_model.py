"""Cases and expected values for tests/hip/roundcheck (the O(n) kernels of the five prover rounds,
cap_amd/csrc/plonk_kernels.hpp, launched through round_launch.hpp), and the file format the two sides share.

Expected values are Python integers over oracle/bn254.py.  Every model works on VALUES (canonical integers mod r) and the
forms are applied at the edges: "arkworks form" is the image x 2^256 mod r, the lazy field's "internal form" x 2^261 mod r
(tests/ntt_io_model.py).  Tables a kernel reads - xs, inv_nx1, QuotConst, tw_n, the power tables, the key columns - are
made here and passed in as data, so a kernel meets tables it did not make, and the expected value is the kernel's formula
in those tables, whatever they hold.

Edge values are chosen on the stored 32-byte image, because the image is what the 29-bit limbs see, and within each
input's contract: canonical (< r) for wires, challenges, xs, k_j x, coefficients and tables; weakly reduced (< 2 r) for
what F::store leaves - the coset evaluations `cos` and the key's coset columns.  Arrays are filled by element index:
index = 0 mod 4 the largest image of the contract whose limbs 0 .. 7 are all 2^29 - 1 (every array at once: the all-edge
rows), 1 mod 4 a draw from the edge set, 2 mod 4 edge or random by a coin, 3 mod 4 random."""
import random
import struct

import numpy as np

from oracle import bn254 as bn
from oracle import plonk as pl
from tests import ntt_io_model as io
from tools.ntt_conformance import add_r

R = bn.R
A256, I261 = (1 << 256) % R, (1 << 261) % R
A256_INV, I261_INV = pow(A256, -1, R), pow(I261, -1, R)
MAGIC_IN, MAGIC_OUT = 0x524f554e44434153, 0x524f554e444f5554
REFUSED = 1000000
NPARAMS = 20
(SCAN, PERM, KX, QUOT, QUOT_TOP, DEGREE, POWERS, EVAL, LINCOMB, DIVIDE, PAD_COPY, BLIND, STAGE) = range(13)
CANON, WEAK = R, 2 * R
NW, NS, COLS = 5, 13, 22
LIMB = (1 << 29) - 1

inv = lambda a: pow(a % R, -1, R)
ark = lambda v: v * A256 % R                      # value -> arkworks-form image
internal = lambda v: v * I261 % R                 # value -> internal-form image
ark_value = lambda img: img * A256_INV % R        # image (any representative) -> value
internal_value = lambda img: img * I261_INV % R
FORMS = {"ark": (ark, ark_value), "internal": (internal, internal_value)}


# ---- edge values -----------------------------------------------------------------------------------------------------
def limbs29(img):
    return [(img >> (29 * i)) & LIMB for i in range(9)]


def saturated(bound):
    """the largest image below `bound` whose 29-bit limbs 0 .. 7 are all 2^29 - 1"""
    low = (1 << 232) - 1
    top = bound >> 232
    return (top << 232 | low) if (top << 232 | low) < bound else ((top - 1) << 232 | low)


def edge_images(bound, form):
    """the fixed part of the edge set of a contract (bound: CANON or WEAK) for inputs of the given form"""
    to_img = FORMS[form][0]
    out = [0, 1, R - 1, to_img(1), to_img(R - 1), saturated(bound)]
    if bound == WEAK:
        out += [R, R + 1, 2 * R - 1]
    return out


def partly_saturated(rng, bound):
    """a random subset of the limbs saturated, the rest zero (limb 8: the top of saturated(bound), so below the bound)"""
    img = sum(LIMB << (29 * i) for i in range(8) if rng.random() < 0.5)
    if rng.random() < 0.5:
        img |= (saturated(bound) >> 232) << 232
    return img


def draw_edge(rng, bound, form):
    fixed = edge_images(bound, form)
    return rng.choice(fixed) if rng.random() < 0.7 else partly_saturated(rng, bound)


def fill(rng, count, bound=CANON, form="ark", phase=0):
    """`count` images by the index rule of the module docstring"""
    out = []
    for idx in range(count):
        mode = (idx + phase) % 4
        if mode == 0:
            out.append(saturated(bound))
        elif mode == 1 or (mode == 2 and rng.random() < 0.5):
            out.append(draw_edge(rng, bound, form))
        else:
            out.append(rng.randrange(bound))
    return out


def rand(rng, count, bound=CANON):
    return [rng.randrange(bound) for _ in range(count)]


# ---- cases and files -------------------------------------------------------------------------------------------------
class Case:
    """kind, params, input buffers (lists of images, or (k, 4) uint64 arrays for records), and `regions`:
    [(start, expected images, weak)] - the expected content of the destination buffer; weak regions hold any
    representative below 2 r of the expected canonical value; everything outside the regions keeps the sentinel (or,
    with dst_init, what input 0 held there)"""

    def __init__(self, name, kind, params, inputs, dst_elems, dst_init=False):
        self.name, self.kind, self.params, self.dst_elems, self.dst_init = name, kind, list(params), dst_elems, dst_init
        self.inputs = [x if isinstance(x, np.ndarray) else io.from_ints(x) if len(x) else np.zeros((0, 4), np.uint64)
                       for x in inputs]
        self.regions = []

    def expect(self, start, images, weak=False):
        self.regions.append((start, io.from_ints(images) if len(images) else np.zeros((0, 4), np.uint64), weak))
        return self


def records(rows):
    """rows of up to four integers -> one field-element-wide record each"""
    return np.array([list(r) + [0] * (4 - len(r)) for r in rows], dtype=np.uint64).reshape(-1, 4)


def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", MAGIC_IN, len(cases)))
        for c in cases:
            p = [int(v) for v in c.params] + [0] * (NPARAMS - len(c.params))
            f.write(struct.pack(f"<{4 + NPARAMS}Q", c.kind, len(c.inputs), c.dst_elems, int(c.dst_init), *p))
            for x in c.inputs:
                f.write(struct.pack("<Q", len(x)))
                f.write(np.ascontiguousarray(x, dtype=np.uint64).tobytes())


def read_results(path, cases):
    out = []
    with open(path, "rb") as f:
        magic, k = struct.unpack("<QQ", f.read(16))
        assert magic == MAGIC_OUT and k == len(cases)
        for c in cases:
            rc, elems = struct.unpack("<QQ", f.read(16))
            assert elems == c.dst_elems
            out.append((rc, np.frombuffer(f.read(32 * elems), dtype=np.uint64).reshape(-1, 4)))
    return out


def perfect_result(c):
    """the destination buffer a correct device leaves (weak regions: the canonical representative)"""
    dst = np.full((c.dst_elems, 4), io.SENTINEL, dtype=np.uint64)
    if c.dst_init:
        dst[:] = c.inputs[0]
    for start, exp, _ in c.regions:
        dst[start:start + len(exp)] = exp
    return dst


def check_case(c, rc, dst):
    """-> list of complaints: wrong values, a representation outside its contract (weak results below 2 r, all others
    canonical and exact), elements outside the regions that changed"""
    if rc != 0:
        return [f"{c.name}: rc = {rc}{' (refused: the case addresses memory outside its buffers)' if rc == REFUSED else ''}"]
    bad = []
    untouched = np.ones(len(dst), dtype=bool)
    for start, exp, weak in c.regions:
        assert start + len(exp) <= len(dst), f"{c.name}: a region leaves the destination buffer"
        got = dst[start:start + len(exp)]
        assert untouched[start:start + len(exp)].all(), f"{c.name}: the case's own regions overlap"
        untouched[start:start + len(exp)] = False
        if not len(exp):
            continue
        assert io.below(exp, R).all()
        same = (got == exp).all(axis=1)
        if weak:
            same |= (got == add_r(exp)).all(axis=1)
        if not same.all():
            k = int(np.nonzero(~same)[0][0])
            bad.append(f"{c.name}: {int((~same).sum())} of {len(exp)} elements of the region at {start} differ, first at "
                       f"{k}: got {io.to_ints(got[k:k + 1])[0]:#x}, expected {io.to_ints(exp[k:k + 1])[0]:#x}")
    rest = np.full((len(dst), 4), io.SENTINEL, dtype=np.uint64)
    if c.dst_init:
        rest[:] = c.inputs[0]
    moved = untouched & (dst != rest).any(axis=1)
    if moved.any():
        bad.append(f"{c.name}: {int(moved.sum())} elements outside the regions were written, first at "
                   f"{int(np.nonzero(moved)[0][0])}")
    return bad


# ---- what every launch of a case reads and writes: the host-side mirror of the driver's refusal -----------------------
def stays_inside(c):
    """every case of this module must pass the driver's bounds check; restated here on the regions and inputs: the
    regions lie inside the destination and the inputs have the sizes the kind's addressing needs"""
    p, n_in = c.params, [len(x) for x in c.inputs]
    ok = all(start + len(exp) <= c.dst_elems for start, exp, _ in c.regions)
    k = c.kind
    if k == SCAN:
        need = (p[4] - 1) * p[3] + p[2]
        ok &= p[2] <= p[3] and n_in[0] >= need and c.dst_elems >= need
    elif k == PERM:
        n, P, per_key, zs = p[0], p[1], p[2], p[3]
        ok &= n_in[0] >= P * 5 * n and n_in[1] >= (P if per_key else 1) * 5 * n and n_in[2] >= n and n_in[3] >= 6 * P
        ok &= n_in[4] >= 14 and (p[4] or n_in[5] >= P) and c.dst_elems >= P * zs + 8 + P + 8 + 2 * P * n and zs >= n
    elif k == KX:
        ok &= n_in[0] >= p[0] and n_in[1] >= 14 and c.dst_elems >= 4 * p[0]
    elif k == QUOT:
        m, P = p[0], p[1]
        ok &= n_in[0] >= (P if p[5] else 1) * COLS * m and n_in[1] >= P * 6 * m and n_in[2] >= m and n_in[3] >= m
        ok &= n_in[4] >= 6 * P and n_in[5] >= 14 and c.dst_elems >= P * m and m % 6 == 0
    elif k == QUOT_TOP:
        n, ps, P = p[0], p[1], p[2]
        ok &= n >= 8 and ps >= n + 3 and n_in[0] >= P * 5 * ps and n_in[1] >= P * ps and n_in[3] >= n and n_in[4] >= 6 * P
        ok &= n_in[2] >= (P if p[3] else 1) * 18 * ps and c.dst_elems >= 8 * P
    elif k == DEGREE:
        ok &= 1 <= p[1] <= p[0] and n_in[0] >= p[2] * p[0] and c.dst_elems >= p[2]
    elif k == POWERS:
        ok &= n_in[0] >= 24 * p[1] and c.dst_elems >= p[0] * p[1]
    elif k == EVAL:
        ok &= n_in[2] >= p[0] and c.dst_elems >= p[0]
        ok &= all(r[2] <= p[1] and r[0] + r[2] <= n_in[0] and r[1] + r[2] <= n_in[1] for r in c.inputs[2][:p[0]].tolist())
    elif k == LINCOMB:
        P, nt, os_, ol = p[:4]
        ok &= ol <= os_ and n_in[1] >= 2 * P * nt and c.dst_elems >= (P - 1) * os_ + ol
        ok &= all(r[0] + min(r[1], ol) <= n_in[0] for r in c.inputs[1][1::2].tolist())
    elif k == DIVIDE:
        ok &= p[0] <= p[1] and p[2] % 2 == 0 and n_in[0] >= p[2] * p[1] and n_in[1] >= p[2] // 2 * 4 * p[1]
        ok &= c.dst_elems >= p[2] * p[1]
    elif k == PAD_COPY:
        for q in range(p[5]):
            ok &= (q // p[4]) * p[0] + (q % p[4]) * p[1] + p[7] <= c.dst_elems
            ok &= (q // p[4]) * p[2] + (q % p[4]) * p[3] + min(p[6], p[7]) <= n_in[0]
    elif k == BLIND:
        ok &= c.dst_init and p[2] + p[5] <= p[1] and p[6] * p[1] <= c.dst_elems and n_in[0] == c.dst_elems
        ok &= all((q // p[3]) * 13 + p[4] + (q % p[3]) * p[5] + p[5] <= n_in[1] for q in range(p[6]))
    elif k == STAGE:
        ok &= n_in[0] >= (p[5] - 1) * p[0] + p[1] and c.dst_elems >= p[5] * (p[1] + p[4])
        ok &= all((q // p[2]) * 13 + p[3] + (q % p[2]) * p[4] + p[4] <= n_in[1] for q in range(p[5]))
    return bool(ok)


# ---- scans -----------------------------------------------------------------------------------------------------------
def scan_model(images, op, rev):
    """exclusive scan of arkworks-form images: op 0 the Montgomery product x y 2^-256, op 1 the sum"""
    xs = images[::-1] if rev else images
    out, run = [], (A256 if op == 0 else 0)
    for x in xs:
        out.append(run)
        run = run * x % R * A256_INV % R if op == 0 else (run + x) % R
    return out[::-1] if rev else out


SCAN_LENS = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049, 65536, 65537, 65539, 131073)


def scan_cases():
    """every length with every (OP, REV); batch, stride and data rotate, so that each of them meets each length and each
    (OP, REV).  At 2^16 and above the batch of 3 is kept for the prover's own two shapes: the product scan of exactly 64
    blocks (round 2) and the suffix sum of 65 (round 5)"""
    out, rng = [], random.Random(0x5CA1)
    for li, len_ in enumerate(SCAN_LENS):
        for op in (0, 1):
            for rev in (0, 1):
                turn = li + 2 * op + rev
                batch = 3 if turn % 2 else 1
                if len_ >= 65536:
                    batch = 3 if (len_, op, rev) in ((65536, 0, 0), (65536, 0, 1), (65539, 1, 1)) else 1
                stride = len_ + 8 if (li // 2 + 2 * op + rev) % 2 else len_
                kinds = ["random", "ones", "r-1"] + (["zero@0", "zero@mid", "zero@last"] if op == 0 else [])
                data = kinds[turn % len(kinds)]
                src = rand(rng, (batch - 1) * stride + len_)
                for b in range(batch):
                    row = slice(b * stride, b * stride + len_)
                    if data == "ones":
                        src[row] = [A256] * len_
                    elif data == "r-1":
                        src[row] = [R - 1] * len_
                    elif data.startswith("zero"):
                        src[b * stride + {"zero@0": 0, "zero@mid": len_ // 2, "zero@last": len_ - 1}[data]] = 0
                c = Case(f"scan op={op} rev={rev} len={len_} batch={batch} stride={stride} {data}", SCAN,
                         [op, rev, len_, stride, batch], [src], (batch - 1) * stride + len_ + 5)
                for b in range(batch):
                    c.expect(b * stride, scan_model(src[b * stride:b * stride + len_], op, rev))
                out.append(c)
    return out


# ---- round 2: the permutation grand product ----------------------------------------------------------------------------
def grand_product(wires, sig, tw, k, beta, gamma):
    """values: wires [5][n], sig [5][n], tw [n] -> num, den, z (z_j = prod_{i<j} num_i / den_i), total = prod den"""
    n = len(tw)
    num, den = [], []
    for j in range(n):
        a = b = 1
        for i in range(NW):
            a = a * (wires[i][j] + beta * k[i] % R * tw[j] + gamma) % R
            b = b * (wires[i][j] + beta * sig[i][j] + gamma) % R
        num.append(a)
        den.append(b)
    z, pn, pd = [], 1, 1
    for j in range(n):
        z.append(pn * inv(pd) % R if pd else None)
        pn, pd = pn * num[j] % R, pd * den[j] % R
    return num, den, z, pd


def quot_const(k, zh_inv, form):
    """QuotConst as 14 images: g (unused by the kernels here), k[5], zh_inv[8]"""
    f = FORMS[form][0]
    return [f(bn.FR_GENERATOR)] + [f(v) for v in k] + [f(v) for v in zh_inv]


def chal_images(form, beta, gamma, alpha, alpha2=None, beta_inv=None, alpha_beta5=None):
    f = FORMS[form][0]
    alpha2 = alpha * alpha % R if alpha2 is None else alpha2
    beta_inv = (inv(beta) if beta else 0) if beta_inv is None else beta_inv
    alpha_beta5 = alpha * pow(beta, 5, R) % R if alpha_beta5 is None else alpha_beta5
    return [f(v) for v in (beta, gamma, alpha, alpha2, beta_inv, alpha_beta5)]


def perm_case(n, per_key, inv_on_device, seed, P=3):
    """proof 0: beta = 0; proof 1: gamma = 0 and wires whose images are 0 or r - 1 only; proof 2: edge challenges.  Wires,
    sigmas and the table tw_n by the index rule.  A draw whose total would be zero is drawn again: z is not defined there
    (the prover never divides by it either - such a witness is refused by the row checks)"""
    zs = n + 8
    for attempt in range(50):
        rng = random.Random(seed * 100 + attempt)
        tw = fill(rng, n, phase=1)
        ks = [1] + [internal_value(draw_edge(rng, CANON, "internal")) if per_key else pl.K[i] for i in range(1, NW)]
        wires = [fill(rng, NW * n, phase=p) for p in range(P)]
        wires[1] = [rng.choice([0, R - 1]) for _ in range(NW * n)]
        nsig = P if per_key else 1
        sigs = [fill(rng, NW * n, phase=2 + q) for q in range(nsig)]
        betas = [0, rng.randrange(1, R), ark_value(draw_edge(rng, CANON, "ark"))]
        gammas = [rng.randrange(R), 0, ark_value(draw_edge(rng, CANON, "ark"))]
        for p in range(P):                            # a zero factor of a denominator: that sigma (beta = 0: that wire) again
            sg = sigs[p if per_key else 0]
            for e in range(NW * n):
                while (ark_value(wires[p][e]) + betas[p] * ark_value(sg[e]) + gammas[p]) % R == 0:
                    if betas[p]:
                        sg[e] = rng.randrange(R)
                    else:
                        wires[p][e] = rng.randrange(R)
        chal, exp = [], []
        for p in range(P):
            w = [[ark_value(v) for v in wires[p][i * n:(i + 1) * n]] for i in range(NW)]
            sg = sigs[p if per_key else 0]
            s = [[ark_value(v) for v in sg[i * n:(i + 1) * n]] for i in range(NW)]
            exp.append(grand_product(w, s, [ark_value(v) for v in tw], ks, betas[p], gammas[p]))
            chal += chal_images("ark", betas[p], gammas[p], rng.randrange(R))
        if all(e[3] for e in exp):
            break
    else:
        raise AssertionError("no draw with non-zero totals")
    totals = [e[3] for e in exp]
    c = Case(f"perm n={n} per_key={per_key} inv_on_device={inv_on_device}", PERM, [n, P, per_key, zs, inv_on_device],
             [sum(wires, []), sum(sigs, []), tw, chal, quot_const(ks, [0] * 8, "internal"), [ark(inv(t)) for t in totals]],
             P * zs + 8 + P + 8 + 2 * P * n + 4)
    for p in range(P):
        c.expect(p * zs, [ark(v) for v in exp[p][2]] + [0] * (zs - n))
    c.expect(P * zs + 8, [ark(inv(t)) if inv_on_device else ark(t) for t in totals])
    c.expect(P * zs + 8 + P + 8, [ark(v) for e in exp for v in e[0]] + [ark(v) for e in exp for v in e[1]])
    return c


def perm_cases():
    return [perm_case(n, per_key, dev, 7 + i) for i, (n, per_key, dev) in enumerate(
        [(16, 0, 0), (16, 1, 1), (1024, 1, 0), (1024, 0, 1), (2048, 0, 0), (2048, 1, 1)])]


# ---- round 3 ---------------------------------------------------------------------------------------------------------
def kx_case(m=96):
    rng = random.Random(0xC01)
    xs = fill(rng, m, form="internal")
    ks = [1] + [internal_value(draw_edge(rng, CANON, "internal")) for _ in range(4)]
    ks[4] = internal_value(saturated(CANON))
    c = Case(f"kx_columns m={m}", KX, [m], [xs, quot_const(ks, [0] * 8, "internal")], 4 * m + 3)
    return c.expect(0, [internal(ks[j + 1] * internal_value(x) % R) for j in range(4) for x in xs])


def quotient_indices(m, five, i):
    """k_quotient's indexing: -> (it, inext, zi): the tables' index, the index of z(omega x), the Z_H table's"""
    mm = m // 3
    blk = (i >= mm) + (i >= 2 * mm)
    half = bool(five) and blk == 2
    it = 2 * i - 2 * mm if half else i
    k1 = i - blk * mm
    inext = blk * mm + ((k1 + 1) & (mm // 2 - 1) if half else (k1 + 2) & (mm - 1))
    zi = 3 * (0 if half else k1 & 1) + blk
    return it, inext, zi


def quotient_point(fold, sel, w, z, zw, x, kx, inv_nx1, zh_inv, ch, ks):
    """values.  sel: the 18 key values, kx: columns 18 .. 21, ch: (beta, gamma, alpha, alpha2, beta_inv, alpha_beta5)"""
    beta, gamma, alpha, alpha2, beta_inv, alpha_beta5 = ch
    a, b = z, zw
    if fold:
        for j in range(NW):
            u = (w[j] + gamma) * beta_inv % R
            a = a * (u + (x if j == 0 else kx[j - 1])) % R
            b = b * (u + sel[NS + j]) % R
        perm = alpha_beta5 * (a - b) % R
    else:
        for j in range(NW):
            a = a * (w[j] + gamma + beta * (ks[j] if j else 1) % R * x) % R
            b = b * (w[j] + gamma + beta * sel[NS + j]) % R
        perm = alpha * (a - b) % R
    return ((pl.gate_eval(sel[:NS], w, 0) + perm) * zh_inv + alpha2 * (z - 1) % R * inv_nx1) % R


def quotient_model(m, five, pkc, cos, xs, inv_nx1, zh_inv, ch, ks, fold):
    """values: pkc [22][m], cos [6][m], tables [m] -> the pts values of one proof"""
    out = []
    for i in range(m - m // 6 if five else m):
        it, inext, zi = quotient_indices(m, five, i)
        out.append(quotient_point(fold, [pkc[s][it] for s in range(18)], [cos[j][i] for j in range(NW)], cos[5][i],
                                  cos[5][inext], xs[it], [pkc[18 + j][it] for j in range(4)], inv_nx1[it], zh_inv[zi], ch,
                                  ks))
    return out


def quot_case(n, five, forms, only_unfoldable, per_key, seed, P=3):
    """proof 1 has a real beta = 0 (beta_inv = 0).  forms: 1 folded launch, 2 direct launch, 3 folded then direct"""
    m, rng = 6 * n, random.Random(seed)
    val = internal_value
    xs = fill(rng, m, form="internal", phase=0)
    inv_nx1 = fill(rng, m, form="internal", phase=0)
    ks = [1] + [val(draw_edge(rng, CANON, "internal")) for _ in range(4)]
    zh_inv = [val(v) for v in fill(rng, 8, form="internal")]
    nkey = P if per_key else 1
    pkcs = []
    for q in range(nkey):
        cols = [fill(rng, m, WEAK, "internal", phase=0) for _ in range(18)]
        cols += [[internal(ks[j + 1] * val(x) % R) for x in xs] for j in range(4)]      # k_j x: canonical, as k_kx_columns
        pkcs.append(cols)
    cos = [[fill(rng, m, WEAK, "internal", phase=0) for _ in range(6)] for _ in range(P)]
    betas = [val(draw_edge(rng, CANON, "internal")) or 1, 0, rng.randrange(1, R)]
    top = val(saturated(CANON))                        # proof 0: gamma and alpha at the saturated image, beta from the edges
    chs = [(betas[0], top, top), (0, val(draw_edge(rng, CANON, "internal")), rng.randrange(R)),
           (betas[2], rng.randrange(R), rng.randrange(R))]
    chal = sum((chal_images("internal", *ch) for ch in chs), [])
    c = Case(f"quotient n={n} five={five} forms={forms} only_unfoldable={only_unfoldable} per_key={per_key}", QUOT,
             [m, P, five, forms, only_unfoldable, per_key],
             [[v for cols in pkcs for col in cols for v in col], [v for pr in cos for col in pr for v in col], xs, inv_nx1,
              chal, quot_const(ks, zh_inv, "internal")], P * m + 6)
    for p in range(P):
        folded_runs = bool(forms & 1) and betas[p] != 0
        direct_runs = bool(forms & 2) and (not only_unfoldable or betas[p] == 0)
        if not (folded_runs or direct_runs):
            continue                                   # the proof's rows keep the sentinel
        b, g, a = chs[p]
        ch = (b, g, a, a * a % R, inv(b) if b else 0, a * pow(b, 5, R) % R)
        pk_v = [[val(v) for v in col] for col in pkcs[p if per_key else 0]]
        cos_v = [[val(v) for v in col] for col in cos[p]]
        # (where both run the direct launch is the later one; the two forms give the same field element)
        vals = quotient_model(m, five, pk_v, cos_v, [val(v) for v in xs], [val(v) for v in inv_nx1], zh_inv, ch, ks,
                              fold=not direct_runs)
        c.expect(p * m, [internal(v) for v in vals], weak=True)
    return c


def quot_cases():
    out, seed = [], 300
    for n in (16, 32):
        for five in (0, 1):
            for forms, ou in ((1, 1), (2, 1), (2, 0), (3, 1)):
                seed += 1
                out.append(quot_case(n, five, forms, ou, per_key=(seed + five) % 2, seed=seed))
    return out


def top_model(n, wpolys, zpoly, sig_polys, sel_polys, tw, beta, alpha):
    """values; k_quotient_top's algorithm on whatever polynomials it is given (tests/test_quot5_identity.py:
    top_coefficients, with the table tw_n in place of the powers of omega)"""
    from tests.test_quot5_identity import series_mul
    import functools
    W = [[wpolys[j][n + 1 - k] for k in range(8)] for j in range(NW)]
    B = [[(W[j][k] + beta * sig_polys[j][n + 1 - k]) % R if k >= 2 else W[j][k] for k in range(8)] for j in range(NW)]
    Z = [zpoly[n + 2 - k] for k in range(8)]
    Zw = [zpoly[n + 2 - k] * tw[(n + 2 - k) % n] % R for k in range(8)]
    h = [0] * 8
    for i in range(4):
        w2 = series_mul(W[i], W[i])
        s = series_mul(series_mul(series_mul(w2, w2), W[i]), [sel_polys[6 + i][n - 1 - k] for k in range(8)])
        for k in range(5):
            h[4 - k] = (h[4 - k] + s[k]) % R
    pw = functools.reduce(series_mul, W)
    s = series_mul(pw, [sel_polys[12][n - 1 - k] for k in range(8)])
    for k in range(5):
        h[4 - k] = (h[4 - k] + s[k]) % R
    pa = series_mul(pw, Z)
    pb = series_mul(functools.reduce(series_mul, B), Zw)
    for k in range(8):
        h[7 - k] = (h[7 - k] + alpha * (pa[k] - pb[k])) % R
    return h


def top_inputs_of_instance(log_n):
    """the proof of tests/test_quot5_identity.py::instance as top_model's arguments"""
    from tests.test_quot5_identity import instance
    from tests.test_quotient_domain import root_6n
    n, pk, tr = instance(log_n)
    ps = n + 8
    pad = lambda poly: list(poly)[:ps] + [0] * (ps - len(poly))
    omega = pow(root_6n(log_n)[0], 6, R)
    return dict(n=n, wpolys=[pad(p) for p in tr["wire_polys"]], zpoly=pad(tr["z_poly"]),
                sig_polys=[pad(p) for p in pk.sigma_polys], sel_polys=[pad(p) for p in pk.selector_polys],
                tw=[pow(omega, e, R) for e in range(n)], beta=tr["beta"], alpha=tr["alpha"])


def top_case(log_n, per_key, seed, P=2):
    """proof 0: the oracle's proof (expected value: top_coefficients, through top_model - test_round_model.py checks that
    the two agree); proof 1: polynomials and challenges by the index rule, its own key when per_key"""
    n, ps, rng = 1 << log_n, (1 << log_n) + 8, random.Random(seed)
    a = top_inputs_of_instance(log_n)
    v = lambda imgs: [ark_value(x) for x in imgs]
    b = dict(n=n, wpolys=[v(fill(rng, ps, phase=j)) for j in range(NW)], zpoly=v(fill(rng, ps)),
             tw=a["tw"], beta=ark_value(draw_edge(rng, CANON, "ark")), alpha=ark_value(draw_edge(rng, CANON, "ark")))
    if per_key:
        b.update(sig_polys=[v(fill(rng, ps, phase=j)) for j in range(NW)], sel_polys=[v(fill(rng, ps, phase=j)) for j in range(NS)])
    else:
        b.update(sig_polys=a["sig_polys"], sel_polys=a["sel_polys"])
    proofs = [a, b]
    img = lambda polys: [ark(x) for poly in polys for x in poly]
    coef = [img(q["sel_polys"] + q["sig_polys"]) for q in (proofs if per_key else proofs[:1])]
    c = Case(f"quotient_top n={n} per_key={per_key}", QUOT_TOP, [n, ps, P, per_key],
             [sum((img(q["wpolys"]) for q in proofs), []), sum((img([q["zpoly"]]) for q in proofs), []), sum(coef, []),
              [ark(x) for x in a["tw"]], sum((chal_images("ark", q["beta"], 0, q["alpha"]) for q in proofs), [])], 8 * P + 3)
    return c.expect(0, [ark(x) for q in proofs for x in top_model(**q)])


def top_cases():
    return [top_case(4, 0, 41), top_case(4, 1, 42), top_case(5, 1, 43), top_case(5, 0, 44)]


def degree_cases():
    """flags: 1 for a non-zero coefficient at or above lo, 2 for a zero at lo - 1.  A planted non-zero coefficient has
    ONE non-zero 32-bit word (a different word each time)"""
    out, rng, word = [], random.Random(0xDE6), 0
    for n in (16, 64):
        m, lo = 6 * n, NW * (n + 1) + 3
        assert (m - (lo - 1)) % 256
        for plan in (("nothing", "at lo", "at m-1"), ("zero at lo-1", "both", "nothing"), ("at m-1", "zero at lo-1", "at lo")):
            t, flags = [], []
            for what in plan:
                row = [rng.randrange(1, R) for _ in range(lo)] + [0] * (m - lo)
                flag = 0
                if what in ("at lo", "at m-1", "both"):
                    word = (word + 3) % 8
                    row[lo if what != "at m-1" else m - 1] = 1 << (32 * word)
                    flag |= 1
                if what in ("zero at lo-1", "both"):
                    row[lo - 1] = 0
                    flag |= 2
                t += row
                flags.append(flag)
            out.append(Case(f"check_degree n={n} {plan}", DEGREE, [m, lo, 3], [t], 3 + 2).expect(0, flags))
    return out


# ---- rounds 4 and 5 ----------------------------------------------------------------------------------------------------
def power_table(x, count):
    out, v = [], 1
    for _ in range(count):
        out.append(v)
        v = v * x % R
    return out


def powers_cases():
    out, rng = [], random.Random(0x90E)
    for ps in (24, 264, 65544):
        bases = [0, 1, R - 1, ark_value(1), ark_value(saturated(CANON)), rng.randrange(R), rng.randrange(R), rng.randrange(R)]
        pw = [ark(pow(b, 1 << e, R)) for b in bases for e in range(24)]
        c = Case(f"powers ps={ps}", POWERS, [ps, len(bases)], [pw], ps * len(bases) + 4)
        out.append(c.expect(0, [ark(v) for b in bases for v in power_table(b, ps)]))
    return out


def horner(poly, x):
    acc = 0
    for v in reversed(poly):
        acc = (acc * x + v) % R
    return acc


def eval_cases():
    """six polynomials of the three lengths n + 2, n, n + 3 in one launch, two points; the power tables arrive as data"""
    out, rng = [], random.Random(0xE7A)
    for turn, n in enumerate((16, 4096, 65536)):
        ps = n + 8
        points = [rng.randrange(R), [1, R - 1, rng.randrange(R)][turn]]
        lens = [n + 2, n, n + 3, n, n + 2, n + 3]
        polys = fill(rng, 6 * ps) if n <= 4096 else rand(rng, 6 * ps)
        recs = [(e * ps, (e % 2) * ps, lens[e]) for e in range(6)]
        c = Case(f"eval n={n}", EVAL, [6, n + 3],
                 [polys, [ark(v) for x in points for v in power_table(x, ps)], records(recs)], 6 + 3)
        out.append(c.expect(0, [ark(horner([ark_value(v) for v in polys[e * ps:e * ps + lens[e]]], points[e % 2]))
                                for e in range(6)]))
    return out


def lincomb_cases():
    """scalars: edge values in the internal form; polynomials: images by the index rule (canonical, arkworks form)"""
    out, rng = [], random.Random(0x11C)
    for n, nterms in ((16, 1), (16, 6), (16, 7), (16, 29), (1024, 29)):
        ps, P = n + 8, 2
        npoly = min(nterms, 8) + 2
        pool = sum((fill(rng, ps) for q in range(npoly)), [])   # index 0 mod 4: every polynomial saturated at once
        terms, rows = [], []
        for t in range(P * nterms):
            q, len_ = rng.randrange(npoly), (n, n + 2, n + 3)[t % 3]
            s = draw_edge(rng, CANON, "internal") if t % 4 != 3 else rng.randrange(R)
            if t % 7 == 0 or t >= nterms:               # proof 1: every scalar saturated - the largest column sums
                s = saturated(CANON)
            terms.append((s, q * ps, len_))
            rows += [[s & (2 ** 64 - 1), s >> 64 & (2 ** 64 - 1), s >> 128 & (2 ** 64 - 1), s >> 192], [q * ps, len_, 0, 0]]
        c = Case(f"lincomb n={n} nterms={nterms}", LINCOMB, [P, nterms, 2 * ps, ps], [pool, records(rows)],
                 (P - 1) * 2 * ps + ps + 5)
        for p in range(P):
            mine = terms[p * nterms:(p + 1) * nterms]
            c.expect(p * 2 * ps, [sum(s * pool[off + k] for s, off, len_ in mine if k < len_) * I261_INV % R
                                  for k in range(ps)])
        out.append(c)
    return out


def synthetic_division(f, a):
    """-> quotient q and remainder r with f = q (X - a) + r"""
    q, carry = [0] * (len(f) - 1), 0
    for k in range(len(f) - 1, 0, -1):
        carry = (f[k] + a * carry) % R
        q[k - 1] = carry
    return q, (f[0] + a * carry) % R


def divide_cases():
    """P = 2: four divisions, power tables [P][4][stride] - a, a', 1 / a, 1 / a' - as data"""
    out, rng = [], random.Random(0xD17)
    for len_ in (19, 1027, 65539):
        stride = len_ + 5
        points = [rng.randrange(1, R), 1, R - 1, rng.randrange(1, R)]
        f = [rand(rng, len_) + rand(rng, stride - len_) for _ in range(4)]          # (the tail is never read)
        pows = []
        for p in range(2):
            for x in (points[2 * p], points[2 * p + 1], inv(points[2 * p]), inv(points[2 * p + 1])):
                pows += [ark(v) for v in power_table(x, stride)]
        c = Case(f"divide len={len_}", DIVIDE, [len_, stride, 4], [sum(f, []), pows], 4 * stride + 3)
        for q in range(4):
            quo, _ = synthetic_division([ark_value(v) for v in f[q][:len_]], points[q])
            c.expect(q * stride, [ark(v) for v in quo] + [0] * (stride - len_ + 1))
        out.append(c)
    return out


# ---- copies and blinders -----------------------------------------------------------------------------------------------
def blinder_index(q, inner, bl_off, nb, t):
    return (q // inner) * 13 + bl_off + (q % inner) * nb + t


def copy_cases():
    out, rng = [], random.Random(0xC09)
    n = 300
    for inner in (1, 5):
        count = 2 * inner
        # k_pad_copy: len < total, distinct inner / outer strides on both sides
        len_, total = n + 2, n + 8
        so, si, do, di = inner * (len_ + 1) + 2, len_ + 1, inner * (total + 3) + 1, total + 3
        src = rand(rng, 2 * so)
        c = Case(f"pad_copy inner={inner}", PAD_COPY, [do, di, so, si, inner, count, len_, total], [src], 2 * do + 4)
        for q in range(count):
            s = (q // inner) * so + (q % inner) * si
            c.expect((q // inner) * do + (q % inner) * di, src[s:s + len_] + [0] * (total - len_))
        out.append(c)
        # k_blind<0> (added) and k_blind<1> (set, then zeros up to the stride), in place; nb = 3 at the z polynomial's offset
        blind = fill(rng, 13 * 2 + 4, phase=1)
        for set_tail, nb, off in ((0, 2, 0), (1, 2, 0), (0, 3, 10), (1, 3, 10)):
            if off and inner != 1:
                continue
            stride = n + 5 if set_tail else n + 8        # SET_TAIL: n + t reaches the stride at t = 5 and must stop there
            polys = rand(rng, count * stride + 4)
            c = Case(f"blind<{set_tail}> inner={inner} nb={nb}", BLIND, [set_tail, stride, n, inner, off, nb, count],
                     [polys, blind], count * stride + 4, dst_init=True)
            for q in range(count):
                b = [blind[blinder_index(q, inner, off, nb, t)] for t in range(nb)]
                head = [(polys[q * stride + t] - b[t]) % R for t in range(nb)]
                c.expect(q * stride, head)
                if set_tail:
                    c.expect(q * stride + n, b + [0] * (stride - n - nb))
                else:
                    c.expect(q * stride + n, [(polys[q * stride + n + t] + b[t]) % R for t in range(nb)])
            out.append(c)
        # k_stage_evals: n values then nb blinders per column
        nb, ss = 2, n + 5
        ev = rand(rng, (count - 1) * ss + n)
        c = Case(f"stage_evals inner={inner}", STAGE, [ss, n, inner, 0, nb, count], [ev, blind], count * (n + nb) + 3)
        for q in range(count):
            c.expect(q * (n + nb), ev[q * ss:q * ss + n] + [blind[blinder_index(q, inner, 0, nb, t)] for t in range(nb)])
        out.append(c)
    return out


GROUPS = {"scans": scan_cases, "grand product": perm_cases, "kx columns": lambda: [kx_case()], "quotient": quot_cases,
          "quotient top": top_cases, "degree check": degree_cases, "powers": powers_cases, "evaluations": eval_cases,
          "lincomb": lincomb_cases, "division": divide_cases, "copies and blinders": copy_cases}
