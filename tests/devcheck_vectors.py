"""Vectors and checker of the device conformance check (tests/hip/): one seeded generator that writes the operand
records, computes what every record must give with Python integers, oracle/bn254.py and oracle/pairing.py, and checks a
result file of either driver (tests/hip/devcheck_host.cpp on the CPU, tests/hip/devcheck.hip on gfx950).  All comparisons
are exact integer comparisons.  Record layouts: tests/hip/devcheck_ops.hpp.

Operands an operation's contract excludes are dropped HERE, by the rule in FIELD_RULES / the explicit conditions of the
other groups' generators; nothing is dropped at check time.  check() asserts the floors on the number of records it has
actually checked per (group, field, schedule, op) and that no record is missing or left at the drivers' 0xFF fill."""
import os
import random
import re
import struct
from collections import defaultdict

from oracle import bn254 as bn
from oracle import pairing as op
from tests.helpers import from_tower, to_tower

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
P, R = bn.P, bn.R
RR = 1 << 261
M29, B29, B30, B31 = (1 << 29) - 1, 1 << 29, 1 << 30, 1 << 31
X_CURVE = 4965661367192848881
M_HARD = 2 * X_CURVE * (6 * X_CURVE * X_CURVE + 3 * X_CURVE + 1)    # final_exp raises to M_HARD (p^12 - 1)/r
GROUPS = ["field", "field32", "curve", "quad", "tower", "pair"]
IN_WORDS = [40, 28, 85, 76, 220, 152]
OUT_WORDS = [11, 9, 38, 110, 110, 110]
DONE, NULLQ, MAGIC, POISON = 0x600D0000, 0xFFFFFFFF, 0x4B435644, 0xFFFFFFFF
# floors on checked records per (group, field, schedule, op): random vectors, and edge vectors where edges are listed
RANDOM_FLOOR = {"field": 200, "field32": 200, "curve": 64, "quad": 64, "tower": 64, "pair": 64}
# floor 8: final_exp, miller2, check2, and pairing2, which is nothing but final_exp(miller2(..))
HEAVY_OPS = {"final_exp", "miller2", "check2", "pairing2"}
# the fewest edge records an op of the group may have (the generator's own count per op is asserted as well)
MIN_EDGES = {"field": 6, "field32": 8, "curve": 11, "quad": 2, "tower": 3, "pair": 2}
# the two chains of the curve group run on a handful of top-of-class records only: no random floor, this many edge records
CHAIN_OPS = {"item_chain": 4, "fold_chain": 4}


def _op_tables():
    src = open(os.path.join(HERE, "hip", "devcheck_ops.hpp")).read()
    out = {}
    for g, macro in zip(GROUPS, ("FIELD", "FIELD32", "CURVE", "QUAD", "TOWER", "PAIR")):
        body = re.search(r"#define DC_%s_OPS\(X\)(.*?)\n(?!\s+X)" % macro, src, re.S).group(1)
        out[g] = {n: int(c) for n, c in re.findall(r"X\((\w+),\s*(\d+)\)", body)}
    return out


OPS = _op_tables()


def _consts():
    """the inflated subtraction constants of field29.hpp (the contracts of the lazy subtractions are stated limb-wise)"""
    src = open(os.path.join(ROOT, "cap_amd", "csrc", "field29.hpp")).read()
    out = [{}, {}]
    for name in ("SUB16P", "SUB2P", "SUB4P", "SUB8P"):
        found = re.findall(r"%s\[9\] = \{(.*?)\}" % name, src, re.S)
        assert len(found) == 2
        for f, body in enumerate(found):
            out[f][name] = [int(x.rstrip("u"), 16) for x in re.findall(r"0x[0-9a-fA-F]+u?", body)]
    return out


CONST = _consts()
MODS = [P, R]


# ---- limbs -----------------------------------------------------------------------------------------------------------
def limbs(v):
    """normalized 29-bit limbs of v (limb 8 takes what is left)"""
    assert 0 <= v < (1 << (232 + 32))
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def val(l):
    return sum(x << (29 * i) for i, x in enumerate(l))


def fe_words(v):
    assert 0 <= v < (1 << 256)
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def fe_val(w):
    return sum(x << (32 * i) for i, x in enumerate(w[:8]))


def fe_slot(v):
    return fe_words(v) + [0]


def is_norm(l):
    return all(x < B29 for x in l)


def lim_lt(l, b, b8=None):
    return all(x < b for x in l[:8]) and l[8] < (b if b8 is None else b8)


class Rec:
    __slots__ = ("group", "op", "field", "sched", "aux", "words", "meta", "kind")

    def __init__(self, group, opn, field, sched, aux, words, meta, kind):
        self.group, self.op, self.field, self.sched, self.aux = group, opn, field, sched, aux
        self.words, self.meta, self.kind = words, meta, kind

    def key(self):
        return (self.group, self.field, self.sched, self.op)

    def describe(self):
        return f"{self.group}.{self.op} field={self.field} sched={self.sched} aux={self.aux} {self.kind}"


# ---- FIELD -----------------------------------------------------------------------------------------------------------
def _prod_ok(pairs, m):
    return sum(val(a) * val(b) for a, b in pairs) < (RR - m) * RR


def _sub_ok(a, b, c, amax):
    """a + c - b limb by limb (c inflated), carried: limbs(a) < amax, b below c limb-wise, the value fits 261 bits"""
    return lim_lt(a, amax) and all(x <= y for x, y in zip(b, c)) and val(a) + val(c) - val(b) < RR


# op -> (arity, rule(f, m, ops) -> admitted?, expect(f, m, ops) -> dict)
#   expect keys: exact (the integer), mod (value mod m), bound (value < bound), norm (limbs < 2^29), limb_bound, flag, fe
def _field_rules():
    inv = [pow(RR, -1, m) for m in MODS]
    c = lambda f, n: CONST[f][n]                                                    # noqa: E731
    L30 = lambda l: lim_lt(l, B30)                                                  # noqa: E731
    rules = {}

    def rule(name, arity, admit, expect):
        rules[name] = (arity, admit, expect)

    def mont(f, m, v):
        return dict(mod=v * inv[f] % m, norm=True)
    rule("mul", 2, lambda f, m, o: L30(o[0]) and L30(o[1]) and _prod_ok([(o[0], o[1])], m),
         lambda f, m, o: dict(mont(f, m, val(o[0]) * val(o[1])), bound=val(o[0]) * val(o[1]) // RR + m + 1))
    rule("sqr", 1, lambda f, m, o: L30(o[0]) and _prod_ok([(o[0], o[0])], m),
         lambda f, m, o: dict(mont(f, m, val(o[0]) ** 2), bound=val(o[0]) ** 2 // RR + m + 1))
    rule("add", 2, lambda f, m, o: L30(o[0]) and L30(o[1]),
         lambda f, m, o: dict(exact=val(o[0]) + val(o[1]), limb_bound=B31))
    rule("sub", 2, lambda f, m, o: _sub_ok(o[0], o[1], c(f, "SUB16P"), B30) and lim_lt(o[1], B30, B31),
         lambda f, m, o: dict(exact=val(o[0]) + 16 * m - val(o[1]), norm=True))
    rule("weak_reduce", 1, lambda f, m, o: is_norm(o[0]),
         lambda f, m, o: dict(mod=val(o[0]) % m, bound=2 * m, norm=True))
    rule("canonical", 1, lambda f, m, o: is_norm(o[0]), lambda f, m, o: dict(exact=val(o[0]) % m, norm=True))
    rule("is_zero", 1, lambda f, m, o: is_norm(o[0]), lambda f, m, o: dict(flag=int(val(o[0]) % m == 0)))
    rule("pack_unpack", 1, lambda f, m, o: is_norm(o[0]) and val(o[0]) < (1 << 256),
         lambda f, m, o: dict(exact=val(o[0]), norm=True))
    rule("from_ext", 1, lambda f, m, o: is_norm(o[0]) and val(o[0]) < (1 << 256),
         lambda f, m, o: dict(mod=val(o[0]) * 32 % m, norm=True))
    rule("to_ext", 1, lambda f, m, o: L30(o[0]) and val(o[0]) * ((1 << 256) % m) < (RR - m) * RR,
         lambda f, m, o: dict(exact=val(o[0]) * pow(32, -1, m) % m, fe=True))
    rule("to_mont", 1, lambda f, m, o: is_norm(o[0]) and val(o[0]) < (1 << 256),
         lambda f, m, o: dict(mod=val(o[0]) * RR % m, norm=True))
    rule("from_mont", 1, lambda f, m, o: L30(o[0]),
         lambda f, m, o: dict(exact=val(o[0]) * inv[f] % m, fe=True))
    rule("mul_add_mul", 4, lambda f, m, o: all(is_norm(x) for x in o) and _prod_ok([(o[0], o[1]), (o[2], o[3])], m),
         lambda f, m, o: mont(f, m, val(o[0]) * val(o[1]) + val(o[2]) * val(o[3])))
    rule("eq", 2, lambda f, m, o: L30(o[0]) and is_norm(o[1]) and val(o[0]) + 16 * m < RR,
         lambda f, m, o: dict(flag=int((val(o[0]) - val(o[1])) % m == 0)))
    rule("inv", 1, lambda f, m, o: is_norm(o[0]) and val(o[0]) < 8 * m,
         lambda f, m, o: dict(mod=(pow(val(o[0]), -1, m) * RR * RR % m) if val(o[0]) % m else 0, norm=True))
    rule("mul_shoup", 2, lambda f, m, o: L30(o[0]) and is_norm(o[1]) and val(o[1]) < m,
         lambda f, m, o: dict(mod=val(o[0]) * val(o[1]) % m, norm=True, bound=(4 if val(o[0]) < RR else 5) * m))
    rule("shoup_quotient", 1, lambda f, m, o: is_norm(o[0]) and val(o[0]) < m,
         lambda f, m, o: dict(exact=((val(o[0]) * inv[f] % m) << 261) // m, norm=True))
    rule("sub8p", 2, lambda f, m, o: is_norm(o[1]) and _sub_ok(o[0], o[1], c(f, "SUB8P"), B31),
         lambda f, m, o: dict(exact=val(o[0]) + 8 * m - val(o[1]), norm=True))
    rule("neg", 1, lambda f, m, o: _sub_ok([0] * 9, o[0], c(f, "SUB16P"), B30) and lim_lt(o[0], B30, B31),
         lambda f, m, o: dict(exact=16 * m - val(o[0]), norm=True))
    rule("add_norm", 2, lambda f, m, o: L30(o[0]) and L30(o[1]) and val(o[0]) + val(o[1]) < RR,
         lambda f, m, o: dict(exact=val(o[0]) + val(o[1]), norm=True))
    rule("normalize", 1, lambda f, m, o: lim_lt(o[0], (1 << 32) - 8) and val(o[0]) < RR,
         lambda f, m, o: dict(exact=val(o[0]), norm=True))
    rule("sub_from_lazy", 2, lambda f, m, o: _sub_ok(o[0], o[1], c(f, "SUB16P"), B31) and lim_lt(o[1], B30, B31),
         lambda f, m, o: dict(exact=val(o[0]) + 16 * m - val(o[1]), norm=True))
    rule("sub2p_lazy", 2, lambda f, m, o: L30(o[0]) and is_norm(o[1]) and o[1][8] <= c(f, "SUB2P")[8],
         lambda f, m, o: dict(exact=val(o[0]) + 2 * m - val(o[1]), limb_bound=B31))
    rule("load", 1, lambda f, m, o: is_norm(o[0]) and val(o[0]) < (1 << 256),
         lambda f, m, o: dict(exact=val(o[0]), norm=True))
    rule("pack", 1, lambda f, m, o: is_norm(o[0]) and val(o[0]) < (1 << 256),
         lambda f, m, o: dict(exact=val(o[0]), fe=True))
    rule("store", 1, lambda f, m, o: is_norm(o[0]),
         lambda f, m, o: dict(mod=val(o[0]) % m, bound=2 * m, fe=True))
    rule("sub2p", 2, lambda f, m, o: is_norm(o[1]) and _sub_ok(o[0], o[1], c(f, "SUB2P"), B31),
         lambda f, m, o: dict(exact=val(o[0]) + 2 * m - val(o[1]), norm=True))
    rule("neg_lazy", 1, lambda f, m, o: is_norm(o[0]) and o[0][8] <= c(f, "SUB16P")[8],
         lambda f, m, o: dict(exact=16 * m - val(o[0]), limb_bound=B31))
    rule("neg2p_lazy", 1, lambda f, m, o: is_norm(o[0]) and o[0][8] <= c(f, "SUB2P")[8],
         lambda f, m, o: dict(exact=2 * m - val(o[0]), limb_bound=B30))
    rule("neg4p_lazy", 1, lambda f, m, o: is_norm(o[0]) and o[0][8] <= c(f, "SUB4P")[8],
         lambda f, m, o: dict(exact=4 * m - val(o[0]), limb_bound=B30))
    rule("sub8p_lazy", 2, lambda f, m, o: L30(o[0]) and is_norm(o[1]) and o[1][8] <= c(f, "SUB8P")[8],
         lambda f, m, o: dict(exact=val(o[0]) + 8 * m - val(o[1]), limb_bound=B31))
    return rules


FIELD_RULES = _field_rules()
FE_INPUT = {"from_ext", "to_mont", "load"}        # operand given as 8 x 32-bit words


def field_edges(m):
    """the listed edge operands, as limb lists (each op's rule decides which of them it admits)"""
    vals = [0, 1, m - 1, m, m + 1, 2 * m - 1, 2 * m, (1 << 256) - 1, RR - 1, RR % m, (m - 1) * RR % m]
    for k in (3, 4, 5, 8, 15, 16, 17, 40, 100, 168):
        vals += [k * m - 1, k * m, k * m + 1]
    vals += [int(1.9 * m), int(3.9 * m), int(7.99 * m) - 1, int(15.9 * m) - 1, 8 * m - 1, 16 * m - 1]
    out = [limbs(v) for v in vals if v < RR]
    out.append([M29] * 9)
    out.append([B30 - 1] * 9)
    out.append([B30 - 1] * 8 + [0])
    out.append([B31 - 1] * 8 + [0])
    out.append([(1 << 32) - 9] * 8 + [0])
    for i in range(9):
        for top in (M29, B30 - 1):
            l = [0] * 9
            l[i] = top
            out.append(l)
    return out


def field_randoms(rng, m, n):
    out = []
    for it in range(n):
        k = it % 8
        if k < 5:
            out.append(limbs(rng.randrange((1, 2, 4, 17, 40)[k] * m)))
        elif k == 5:
            out.append([rng.randrange(B30) for _ in range(8)] + [rng.randrange(1 << 20)])
        elif k == 6:
            out.append([rng.randrange(B31) for _ in range(8)] + [rng.randrange(1 << 20)])
        else:
            out.append(limbs(rng.randrange(m)))
    return out


def gen_field(rng):
    recs = []
    for f, m in enumerate(MODS):
        edges = field_edges(m)
        second = [limbs(v) for v in (0, 1, m - 1, m, 2 * m - 1, int(15.9 * m) - 1)] + [[M29] * 9, [B30 - 1] * 9]
        for name, (arity, admit, _e) in FIELD_RULES.items():
            cands = []
            if arity == 1:
                cands = [((a,), "edge") for a in edges]
            elif arity == 2:
                cands = [((a, b), "edge") for a in edges for b in second] + [((b, a), "edge") for a in edges for b in second[:3]]
            else:
                cands = [((a, b, b, a), "edge") for a in edges for b in second[:5]]
            chosen = [(o, k) for o, k in cands if admit(f, m, o)]
            assert len(chosen) >= 6, (name, f, len(chosen))
            nrand, tries = 0, 0
            while nrand < RANDOM_FLOOR["field"]:
                tries += 1
                assert tries < 20000, name
                o = tuple(field_randoms(rng, m, 8)[rng.randrange(8)] for _ in range(arity))
                if name in ("mul_shoup",):
                    o = (o[0], limbs(rng.randrange(m)))
                if admit(f, m, o):
                    chosen.append((o, "random"))
                    nrand += 1
            for o, kind in chosen:
                for s in (0, 1):
                    words = []
                    for k in range(4):
                        if k < len(o):
                            words += fe_slot(val(o[k])) if (name in FE_INPUT and k == 0) else list(o[k])
                        else:
                            words += [0] * 9
                    recs.append(Rec("field", name, f, s, 0, words, o, kind))
    return recs


def check_field(r, out):
    m = MODS[r.field]
    exp = FIELD_RULES[r.op][2](r.field, m, r.meta)
    got = out[:9]
    if "flag" in exp:
        if any(got):
            return "words beside the flag are not 0"
        return None if out[9] == exp["flag"] else f"flag {out[9]} != {exp['flag']}"
    if exp.get("fe"):
        v = fe_val(got)
        if got[8] != 0:
            return "ninth word of an fe result is not 0"
    else:
        v = val(got)
    if "exact" in exp and v != exp["exact"]:
        return f"value {v:#x} != {exp['exact']:#x}"
    if "mod" in exp and v % m != exp["mod"]:
        return f"value mod p {v % m:#x} != {exp['mod']:#x}"
    if "bound" in exp and not v < exp["bound"]:
        return f"value {v:#x} not below its bound {exp['bound']:#x}"
    if exp.get("norm") and not (is_norm(got) and v < RR):
        return f"limbs not normalized: {got}"
    if "limb_bound" in exp and not all(x < exp["limb_bound"] for x in got):
        return f"limbs above {exp['limb_bound']:#x}: {got}"
    return None


# ---- FIELD32 ---------------------------------------------------------------------------------------------------------
# Operands of tests/cpp/field_host_check.cpp: its eight edge values (non-canonical ones included) and random values over
# all 256 bits, a third of them masked below 2^253.  Which ops take which operands - the one exclusion table of the group:
#   mul, sqr       any 256-bit words.  Expected: the CIOS integer T = (a b + m p) / 2^256, m = -a b / p mod 2^256, its
#                  ninth word dropped (field.hpp says so: T >= 2^256 needs both operands far above p), one conditional
#                  subtraction - congruent to a b / 2^256 whenever T < 2^256, i.e. whenever an operand is below 2^254.
#   the others     canonical operands only: add / sub / dbl / neg assume "no carry out of 256 bits" and one conditional
#                  subtraction (inputs < p), inv / pow are defined on field elements.  Non-canonical operands are dropped.
FIELD32_ANY = {"mul", "sqr"}


def gen_field32(rng):
    recs = []
    for f, m in enumerate(MODS):
        r256, top = 1 << 256, (1 << 256) - 1
        edge = [0, r256 % m, m, (m - r256 % m) % m, top, 1, m - 1, m + 5]          # field_host_check.cpp: edge[0..7]
        pairs = [(a, b, "edge") for a in edge for b in edge]
        for it in range(3 * RANDOM_FLOOR["field32"]):
            a, b = rng.randrange(r256), rng.randrange(r256)
            if it % 3 == 0:
                a, b = a & ((1 << 253) - 1), b & ((1 << 253) - 1)
            elif it % 3 == 1:
                a, b = rng.randrange(m), rng.randrange(m)
            pairs.append((a, b, "random"))
        exps = (0, 1, 2, m - 2, top, 1 << 255, 3, 65537)
        for a, b, kind in pairs:
            e = rng.randrange(r256) if kind == "random" else exps[edge.index(b)]
            for name in OPS["field32"]:
                if name not in FIELD32_ANY and not (a < m and b < m):
                    continue
                words = fe_words(a) + fe_words(b) + fe_words(e)
                recs.append(Rec("field32", name, f, 0, 0, words, (a, b, e), kind))
    return recs


def _cios(a, b, m):
    """field.hpp's product for ANY 256-bit words.  With an operand below 2^254 every intermediate sum fits its nine words
    and the result is the integer T = (a b + m' p) / 2^256 after one conditional subtraction.  With both operands at
    2^254 or above ("never field elements": field.hpp) carries leave the ninth word inside the loop; what the 32-bit
    form then returns has no arithmetic meaning and is specified by its word-level steps only, followed here."""
    r256, M = 1 << 256, 0xFFFFFFFF
    if a < (1 << 254) or b < (1 << 254):
        t = (a * b + (-a * b * pow(m, -1, r256)) % r256 * m) >> 256
        assert t < r256 and t % m == a * b * pow(r256, -1, m) % m
        return t - m if t >= m else t
    aw, bw, mw = fe_words(a), fe_words(b), fe_words(m)
    ninv = (-pow(m, -1, 1 << 32)) & M
    t = [0] * 9
    for i in range(8):
        for mult, src, shift in ((bw[i], aw, 0), (None, mw, 1)):
            k = (t[0] * ninv) & M if mult is None else mult
            r = [k * src[j] + t[j] for j in range(8)]
            c, low = 0, [r[0] & M]
            for j in range(1, 8):
                x = (r[j] & M) + (r[j - 1] >> 32) + c
                low.append(x & M)
                c = x >> 32
            x = t[8] + (r[7] >> 32) + c
            t = (low + [x & M]) if not shift else (low[1:] + [x & M, x >> 32])
    v = fe_val(t[:8])
    return v - m if v >= m else v


def check_field32(r, out):
    m = MODS[r.field]
    a, b, e = r.meta
    ri = pow(1 << 256, -1, m)
    if r.op in FIELD32_ANY:
        b = a if r.op == "sqr" else b
        exp = _cios(a, b, m)
    else:
        exp = {"add": (a + b) % m, "sub": (a - b) % m, "dbl": 2 * a % m, "neg": (-a) % m,
               "inv": (pow(a, -1, m) << 512) % m if a else 0, "pow": pow(a * ri, e, m) * (1 << 256) % m}[r.op]
    v = fe_val(out)
    return None if v == exp else f"value {v:#x} != {exp:#x}"


# ---- points ----------------------------------------------------------------------------------------------------------
def mont(v):
    return v * RR % P


def unmont(v):
    return v * pow(RR, -1, P) % P


def xyzz(pt, lam=1, lazy=False):
    """XYZZ limbs (internal Montgomery form) of an affine point scaled by lam; lazy: x, y as their + p representatives"""
    if pt is None:
        return [0] * 36
    x, y = pt
    zz, zzz = lam * lam % P, lam ** 3 % P
    cx, cy = mont(x * zz % P), mont(y * zzz % P)
    if lazy:
        cx, cy = cx + P, cy + P
    return limbs(cx) + limbs(cy) + limbs(mont(zz)) + limbs(mont(zzz))


def xyzz_top(rng, pt, ky=2, zmax=(6, 5)):
    """the top of the accumulator class (curve29.hpp: x < 2p, y < 3p, zz, zzz < 1.2p): pt scaled by lambda, x as its + p
    and y as its + ky p representative, lambda drawn until zz + p and zzz + p stay below zmax p"""
    x, y = pt
    while True:
        lam = rng.randrange(2, P)
        zz, zzz = mont(lam * lam % P) + P, mont(pow(lam, 3, P)) + P
        if zmax[1] * zz < zmax[0] * P and zmax[1] * zzz < zmax[0] * P:
            break
    return limbs(mont(x * lam * lam % P) + P) + limbs(mont(y * pow(lam, 3, P) % P) + ky * P) + limbs(zz) + limbs(zzz)


def xyzz_image(rng, pt):
    """a bucket image just below 2^256 (g1_xyzz: "any value < 2^256"): every coordinate its largest representative"""
    lam = rng.randrange(2, P)
    c = [mont(pt[0] * lam * lam % P), mont(pt[1] * pow(lam, 3, P) % P), mont(lam * lam % P), mont(pow(lam, 3, P))]
    return sum((limbs(v + ((1 << 256) - 1 - v) // P * P) for v in c), [])


def affine_of(w, ybound=2):
    """36 words of an XYZZ result -> (affine point or None, error or None); checks the invariants of a point in registers"""
    c = [w[0:9], w[9:18], w[18:27], w[27:36]]
    if not all(is_norm(l) for l in c):
        return None, "limbs not normalized"
    x, y, zz, zzz = (val(l) for l in c)
    if zz == 0:
        return None, None
    if not (x < 2 * P and y < ybound * P and 5 * zz < 6 * P and 5 * zzz < 6 * P):
        return None, "coordinate above its bound (x < 2p, y < %dp, zz, zzz < 1.2p)" % ybound
    if zz % P == 0 or zzz % P == 0:
        return None, "zz or zzz is a non-literal zero"
    if pow(zz, 3, P) != zzz * zzz * RR % P:
        return None, "zz^3 != zzz^2"
    return (x * pow(zz, -1, P) % P, y * pow(zzz, -1, P) % P), None


_POOL = {}


def rand_pt(rng):
    """a random-looking point: a running sum over a small pool of [k]G (one scalar multiplication per pool entry)"""
    st = _POOL.setdefault(id(rng), {})
    if not st:
        st["pool"] = [bn.g1_mul(bn.G1_GEN, rng.randrange(1, R)) for _ in range(24)]
        st["cur"] = bn.g1_mul(bn.G1_GEN, rng.randrange(1, R))
    while True:
        st["cur"] = bn.g1_add(st["cur"], st["pool"][rng.randrange(24)])
        if st["cur"] is not None:
            return st["cur"]


def neg_pt(p):
    return bn.g1_neg(p)


SCALAR_EDGES = [0, 1, 2, 3, 4, R - 1, R, R + 1, (1 << 256) - 1, int("55" * 32, 16), int("aa" * 32, 16)] + \
    [1 << k for k in (31, 32, 33, 63, 64, 95, 96, 127, 128, 159, 160, 191, 192, 223, 224, 254, 255)] + \
    [(1 << k) - 1 for k in (31, 32, 33, 63, 64, 65, 96, 128, 160, 192, 224, 255)] + \
    [((1 << 256) - 1) >> k for k in (1, 3, 5, 31, 33, 63, 65, 129)]


def pair_cases(rng, n_random):
    """(A, B, kind) affine operand pairs: ordinary, P + P, P - P, infinity on either side and both, (1, 2)"""
    out = []
    for _ in range(n_random):
        out.append((rand_pt(rng), rand_pt(rng), "random"))
    for _ in range(4):
        p, q = rand_pt(rng), rand_pt(rng)
        out += [(p, p, "edge:P+P"), (p, neg_pt(p), "edge:P-P"), (None, q, "edge:inf+Q"), (p, None, "edge:P+inf"),
                (None, None, "edge:inf+inf"), (bn.G1_GEN, q, "edge:(1,2)+Q"), (p, bn.G1_GEN, "edge:P+(1,2)"),
                (bn.G1_GEN, bn.G1_GEN, "edge:(1,2)+(1,2)"), (bn.G1_GEN, neg_pt(bn.G1_GEN), "edge:(1,2)-(1,2)")]
    return out


def gen_curve(rng):
    recs = []
    C = OPS["curve"]

    def add(name, s, aux, A, B, k, meta, kind):
        recs.append(Rec("curve", name, 0, s, aux, A + B + fe_words(k) + [0], meta, kind))
    cases = pair_cases(rng, RANDOM_FLOOR["curve"])
    lam = lambda: rng.randrange(2, P)                        # noqa: E731
    for i, (a, b, kind) in enumerate(cases):
        lazy = i % 3 == 1
        la, lb = lam(), lam()
        A, Bx, Ba = xyzz(a, la, lazy), xyzz(b, lb, lazy and i % 2 == 1), xyzz(b, 1, lazy)
        for s in (0, 1):
            add("add", s, 0, A, Bx, 0, (a, b), kind)
            add("add_acc", s, 0, A, Bx, 0, (a, b), kind)
            add("dbl", s, 0, A, [0] * 36, 0, (a,), kind)
            add("to_affine", s, 0, A, [0] * 36, 0, (a,), kind)
            add("store_load", s, 0, A, [0] * 36, 0, (A,), kind)
            add("from_affine", s, 0, [0] * 36, Ba, 0, (b, Ba), kind)
            add("dbl_affine", s, 0, [0] * 36, Ba, 0, (b,), kind)
            for neg in (0, 1):
                add("add_mixed", s, neg, A, Ba, 0, (a, b), kind)
                if b is not None:                            # madd_acc: q is never infinity (the caller tests that)
                    add("madd_acc", s, neg, A, Ba, 0, (a, b, A), kind)
            # load(g1_affine): any 256-bit words, e.g. the + p representatives
            mx, my = (0, 0) if b is None else (mont(b[0]) + (P if lazy else 0), mont(b[1]) + (2 * P if lazy else 0))
            recs.append(Rec("curve", "load_affine", 0, s, 0, fe_slot(mx) + fe_slot(my) + [0] * (18 + 36 + 9), (mx, my), kind))
    scal = [(k, "edge") for k in SCALAR_EDGES] + [(rng.randrange(1 << 256), "random") for _ in range(64)]
    pts = [rand_pt(rng), bn.G1_GEN, None]
    for pi, pt in enumerate(pts):
        for k, kind in scal:
            if pi == 2 and kind == "random" and k % 8:
                continue
            B = xyzz(pt, 1, lazy=(pi == 0 and k % 2 == 1))
            for s in (0, 1):
                add("term_mul", s, 0, [0] * 36, B, k, (pt, k), kind if pi < 2 else "edge")
    # edge:top - operands at the top of the classes the envelope closes from (tests/golden/lazy_envelope.json, "curve"):
    # the accumulator class A (y in [2p, 3p), zz and zzz just below 1.2p) and bucket images just below 2^256
    top = (1 << 256) - 1
    for i in range(2):
        a, b = rand_pt(rng), rand_pt(rng)
        make = xyzz_top if i == 0 else xyzz_image
        A, Bx = make(rng, a), make(rng, b)
        Ba = xyzz(b, 1, True)                                # the table point as its + p representatives (< 2p)
        Am = xyzz_top(rng, a)                                # madd_acc takes class A only (its 4p - y)
        mx, my = mont(b[0]) + (top - mont(b[0])) // P * P, mont(b[1]) + (top - mont(b[1])) // P * P
        for s in (0, 1):
            add("add", s, 0, A, Bx, 0, (a, b), "edge:top")
            add("add_acc", s, 0, A, Bx, 0, (a, b), "edge:top")
            add("dbl", s, 0, A, [0] * 36, 0, (a,), "edge:top")
            add("to_affine", s, 0, A, [0] * 36, 0, (a,), "edge:top")
            add("store_load", s, 0, A, [0] * 36, 0, (A,), "edge:top")
            add("from_affine", s, 0, [0] * 36, Ba, 0, (b, Ba), "edge:top")
            add("dbl_affine", s, 0, [0] * 36, Ba, 0, (b,), "edge:top")
            add("term_mul", s, 0, [0] * 36, Ba, top - i, (b, top - i), "edge:top")
            recs.append(Rec("curve", "load_affine", 0, s, 0, fe_slot(mx) + fe_slot(my) + [0] * (18 + 36 + 9), (mx, my),
                            "edge:top"))
            for neg in (0, 1):
                add("add_mixed", s, neg, A, Ba, 0, (a, b), "edge:top")
                add("madd_acc", s, neg, Am, Ba, 0, (a, b, Am), "edge:top")
    # the two chains: an item of msm_accumulate over four table points, and a fold of the reductions on class A
    for i in range(CHAIN_OPS["item_chain"]):
        t = [rand_pt(rng) for _ in range(4)]
        signs = (0x55, 0x66, 0x99, 0xaa, 0x33)[i % 5]        # mixed, a point keeps its sign: no partial sum is +-q
        words = sum((limbs(mont(q[0])) + limbs(mont(q[1])) for q in t), [])
        for s in (0, 1):
            add("item_chain", s, signs, words[:36], words[36:], 0, (t, signs), "edge:top")
    for i in range(CHAIN_OPS["fold_chain"]):
        a, b = rand_pt(rng), rand_pt(rng)
        A, Bx = (xyzz_top(rng, a), xyzz_top(rng, b)) if i < 3 else (xyzz_image(rng, a), xyzz_image(rng, b))
        for s in (0, 1):
            add("fold_chain", s, 0, A, Bx, 0, (a, b), "edge:top")
    assert set(r.op for r in recs) == set(C)
    return recs


def check_chain(r, out):
    """item_chain: the item's sum, in the accumulator's class, as it comes back from its memory image; fold_chain:
    2 (2a + b) as the canonical Jacobian triple of the C ABI"""
    w, flag = out[:36], out[36]
    if flag != 1:
        return "a lean addition refused ordinary operands"
    if r.op == "item_chain":
        t, signs = r.meta
        want = None
        for i in range(8):
            q = t[i & 3]
            want = bn.g1_add(want, neg_pt(q) if (signs >> i) & 1 else q)
        got, err = affine_of(w, 3)
        return err or (None if got == want else f"point {got} != {want}")
    a, b = r.meta
    s = bn.g1_add(bn.g1_add(a, b), a)
    want = bn.g1_add(s, s)
    if any(w[9 * c + 8] for c in range(3)) or any(w[27:36]):
        return "words beyond the triple are not 0"
    x, y, z = (fe_val(w[9 * c:9 * c + 8]) for c in range(3))
    if not max(x, y, z) < P:
        return "the triple is not canonical"
    i256 = pow(1 << 256, -1, P)
    x, y, z = (v * i256 % P for v in (x, y, z))
    if z == 0:
        return "infinity"
    zi = pow(z, -1, P)
    got = (x * zi * zi % P, y * pow(zi, 3, P) % P)
    return None if got == want else f"point {got} != {want}"


def check_curve(r, out):
    w, flag = out[:36], out[36]
    name, m = r.op, r.meta
    if name in CHAIN_OPS:
        return check_chain(r, out)
    if name == "store_load":
        return None if w == m[0] else "load(store(A)) != A"
    if name == "load_affine":
        if (val(w[:9]), val(w[9:18])) != m or not is_norm(w[:18]):
            return "loaded value differs"
        return None if flag == int(m == (0, 0)) else "infinity flag"
    if name == "from_affine" and m[0] is not None and w[:18] != m[1][:18]:
        return "from_affine changed the coordinates"
    if name == "to_affine":
        if not is_norm(w[:18]):
            return "limbs not normalized"
        got = (unmont(val(w[:9])), unmont(val(w[9:18])))
        want = (0, 0) if m[0] is None else m[0]
        return None if got == want else f"affine {got} != {want}"
    want = {"from_affine": lambda: m[0], "dbl_affine": lambda: bn.g1_add(m[0], m[0]), "dbl": lambda: bn.g1_add(m[0], m[0]),
            "add": lambda: bn.g1_add(m[0], m[1]), "add_acc": lambda: bn.g1_add(m[0], m[1]),
            "add_mixed": lambda: bn.g1_add(m[0], neg_pt(m[1]) if r.aux else m[1]),
            "madd_acc": lambda: bn.g1_add(m[0], neg_pt(m[1]) if r.aux else m[1]),
            "term_mul": lambda: _g1_mul(m[0], m[1]) if m[0] is not None else None}[name]()
    if name in ("madd_acc", "add_acc"):
        a, b = m[0], m[1]
        special = a is None or b is None or a[0] == b[0]      # the x-difference vanishes: every special case
        if flag != int(not special):
            return f"returned {flag} for {'a special' if special else 'the common'} case"
        if special:
            return None if w == r.words[0:36] else "the accumulator was touched on a refused addition"
    got, err = affine_of(w, 3 if name in ("madd_acc", "add_acc") else 2)
    if err:
        return err
    return None if got == want else f"point {got} != {want}"


# ---- QUAD ------------------------------------------------------------------------------------------------------------
QUAD_CASES = ["ord", "ainf", "binf", "pp", "pm"]


def gen_quad(rng):
    """full waves of 16 quads, cases mixed by construction; the last wave is partial"""
    qops = list(OPS["quad"])

    def make(case, name, s):
        a, b = rand_pt(rng), rand_pt(rng)
        if case == "ainf":
            a = None
        elif case == "binf":
            b = None
        elif case == "pp":
            b = a
        elif case == "pm":
            b = neg_pt(a)
        A, B = xyzz(a, rng.randrange(2, P)), xyzz(b, rng.randrange(2, P))
        return Rec("quad", name, 0, s, 0, A + B, (a, b), "random" if case == "ord" else "edge:" + case)
    recs = []
    for s in (0,):
        for case in QUAD_CASES[1:]:                      # exactly one odd quad in the wave, for each case
            pos = rng.randrange(16)
            name = qops[rng.randrange(4)]
            recs += [make(case if i == pos else "ord", "add" if i == pos else name, s) for i in range(16)]
        combos = [(c, n) for c in QUAD_CASES for n in qops]   # every quad a different (case, op)
        rng.shuffle(combos)
        recs += [make(c, n, s) for c, n in combos[:16]]
        recs += [make(c, n, s) for c, n in (combos[16:] + combos[:12])]
    # the same waves, same operands, under the other schedule (the two must agree limb for limb)
    recs += [Rec("quad", r.op, 0, 1, 0, r.words, r.meta, r.kind) for r in recs]
    for w in range(52):                                  # seeded mixtures, both schedules inside one wave
        for i in range(16):
            case = QUAD_CASES[rng.randrange(5)] if rng.randrange(3) == 0 else "ord"
            recs.append(make(case, qops[(w + i) % 4] if rng.randrange(4) else qops[rng.randrange(4)], rng.randrange(2)))
    # edge:top, one full wave: both operands at the top of the quad class (x, y their + p representatives, zz and zzz
    # just below 1.2p), every op under both schedules
    for i in range(16):
        a, b = rand_pt(rng), rand_pt(rng)
        recs.append(Rec("quad", qops[i % 4], 0, (i >> 2) & 1, 0, xyzz_top(rng, a, 1) + xyzz_top(rng, b, 1), (a, b),
                        "edge:top"))
    recs += [make(QUAD_CASES[i % 5], qops[i % 4], i % 2) for i in range(7)]      # the partial last wave
    assert len(recs) % 16 == 7
    return recs


def check_quad(r, out):
    a, b = r.meta
    add, dbl = bn.g1_add, lambda p: bn.g1_add(p, p)       # noqa: E731
    want = {"add": lambda: add(a, b), "dbl": lambda: dbl(a),
            "chain": lambda: add(add(dbl(add(a, b)), b), a),
            "tree": lambda: add(add(a, dbl(a)), add(b, dbl(b)))}[r.op]()
    for what, off in (("the quad result", 0), ("the quad result through its memory image", 36), ("the one-lane result", 72)):
        got, err = affine_of(out[off:off + 36])
        if err:
            return f"{what}: {err}"
        if got != want:
            return f"{what}: {got} != {want}"
    if out[108] != int(want is None):
        return "infinity flag"
    return None


# ---- TOWER -----------------------------------------------------------------------------------------------------------
# struct order of an f12's six Fq2 coefficients -> their power of w
STRUCT_POW = [0, 2, 4, 1, 3, 5]


def f12_words(f, lazy=()):
    """flat-basis element -> 108 words in struct order, internal Montgomery form; positions in `lazy` get + p"""
    t = to_tower(f)
    w = []
    for si, k in enumerate(STRUCT_POW):
        for j in (0, 1):
            v = mont(t[2 * k + j])
            if (2 * si + j) in lazy:
                v += P
            w += limbs(v)
    return w


def f12_of(w, n_f2=6):
    """108 result words -> (flat-basis element, error): every stored Fq value normalized and < 2p"""
    t = [0] * 12
    for si, k in enumerate(STRUCT_POW):
        for j in (0, 1):
            l = w[9 * (2 * si + j):9 * (2 * si + j) + 9]
            v = val(l)
            if si >= n_f2:
                if v:
                    return None, "words beyond the result are not 0"
                continue
            if not is_norm(l) or not v < 2 * P:
                return None, f"coefficient {2 * si + j} not normalized and < 2p: {v:#x}"
            t[2 * k + j] = unmont(v)
    return from_tower(t), None


def embed(coeffs, n_f2):
    """n_f2 Fq2 coefficients in struct order (2 n_f2 integers) -> flat-basis Fq12"""
    t = [0] * 12
    for si in range(n_f2):
        k = STRUCT_POW[si]
        t[2 * k], t[2 * k + 1] = coeffs[2 * si], coeffs[2 * si + 1]
    return from_tower(t)


_FROB_BASIS = {}


def frob(f, j):
    """f^(p^j) by linearity over Fq: the images of w^k, each one exponentiation"""
    if j not in _FROB_BASIS:
        _FROB_BASIS[j] = [op.f12_pow([int(i == k) for i in range(12)], P ** j) for k in range(12)]
    out = [0] * 12
    for k, c in enumerate(f):
        if c:
            for i, v in enumerate(_FROB_BASIS[j][k]):
                out[i] = (out[i] + c * v) % P
    return out


def conj6(f):
    return [(-c) % P if i % 2 else c for i, c in enumerate(f)]


def easy_part(f):
    r = op.f12_mul(conj6(f), op.f12_pow(f, P ** 12 - 2))
    return op.f12_mul(frob(r, 2), r)


TOWER_SIZE = {"f2_mul": 1, "f2_sqr": 1, "f2_inv": 1, "f2_mul_xi": 1, "f6_mul": 3, "f6_mul_01": 3, "f6_inv": 3, "f6_mul_v": 3}
TOWER_BINARY = {"f2_mul", "f6_mul", "f12_mul"}
XI_F12, V_F12 = embed([9, 1], 1), embed([0, 0, 1, 0], 2)
_FE_CACHE = {}
EDGE_COUNTS = {}        # (group, field, schedule, op) -> edge records admitted by the generator's rules


def tower_expect(name, aux, a, b):
    if name in ("f2_mul", "f6_mul", "f12_mul", "f6_mul_01", "f12_mul_line"):
        return op.f12_mul(a, b)
    if name in ("f2_sqr", "f12_sqr", "f12_cyclo_sqr"):
        return op.f12_mul(a, a)
    if name == "f2_mul_xi":
        return op.f12_mul(a, XI_F12)
    if name == "f6_mul_v":
        return op.f12_mul(a, V_F12)
    if name == "f12_conj":
        return conj6(a)
    if name == "f12_frob":
        return frob(a, aux)
    if name == "f12_exp_x":
        return op.f12_pow(a, X_CURVE)
    if name == "final_exp":
        k = tuple(a)
        if k not in _FE_CACHE:
            _FE_CACHE[k] = op.f12_pow(op.final_exponentiation(a), M_HARD)
        return _FE_CACHE[k]
    raise KeyError(name)


def gen_tower(rng):
    recs = []
    n_rand = RANDOM_FLOOR["tower"]
    cyc_base = [easy_part([rng.randrange(P) for _ in range(12)]) for _ in range(3)]

    def cyclo():
        i, j = rng.randrange(3), rng.randrange(3)
        return op.f12_mul(op.f12_pow(cyc_base[i], rng.randrange(1, 1 << 64)), op.f12_pow(cyc_base[j], rng.randrange(1 << 64)))

    def elements(n_f2, n):
        """(flat element, lazy positions, kind): random ones, then 0, 1, -1, single coefficients, all p - 1, the top of < 2p"""
        nc = 2 * n_f2
        out = [(embed([rng.randrange(P) for _ in range(nc)], n_f2), (), "random") for _ in range(n)]
        out += [(embed([0] * nc, n_f2), (), "edge:0"), (embed([1] + [0] * (nc - 1), n_f2), (), "edge:1"),
                (embed([P - 1] + [0] * (nc - 1), n_f2), (), "edge:-1"), (embed([P - 1] * nc, n_f2), (), "edge:p-1"),
                (embed([unmont(P - 1)] * nc, n_f2), tuple(range(nc)), "edge:2p-1")]   # stored: (p - 1) + p
        for i in range(nc):
            c = [0] * nc
            c[i] = (1, P - 1, rng.randrange(1, P))[i % 3]
            out.append((embed(c, n_f2), (i,) if i % 2 else (), "edge:single"))
        out.append((embed([rng.randrange(P) for _ in range(nc)], n_f2), tuple(range(nc)), "edge:lazy"))
        # every stored coefficient within 2^64 of the top of class E (2p - 1), all different
        out.append((embed([unmont(P - 1 - rng.randrange(1 << 64)) for _ in range(nc)], n_f2), tuple(range(nc)), "edge:top"))
        return out

    def add(name, aux, a, la, b, lb, kind, wb=None):
        for s in (0, 1):
            words = f12_words(a, la) + (wb if wb is not None else f12_words(b, lb))
            recs.append(Rec("tower", name, 0, s, aux, words, (a, b), kind))
    zero = [0] * 12
    for name in OPS["tower"]:
        n_f2 = TOWER_SIZE.get(name, 6)
        if name in ("f12_cyclo_sqr", "f12_exp_x"):
            n = n_rand
            for i in range(n):
                add(name, 0, cyclo(), tuple(range(12)) if i % 4 == 3 else (), zero, (), "random")
            add(name, 0, list(op.F12_ONE), (), zero, (), "edge:1")
            add(name, 0, conj6(cyc_base[0]), (), zero, (), "edge:conj")
            add(name, 0, cyclo(), tuple(range(12)), zero, (), "edge:top")      # every coefficient its + p representative
        elif name == "final_exp":
            for a, la, kind in elements(6, 8):
                add(name, 0, a, la, zero, (), kind)
        elif name == "f12_frob":
            for a, la, kind in elements(6, n_rand):
                for j in (1, 2, 3):
                    add(name, j, a, la, zero, (), kind)
        elif name == "f6_mul_01":
            for a, la, kind in elements(3, n_rand):
                c = [rng.randrange(P) for _ in range(4)] if kind == "random" else [P - 1, 0, 0, P - 1]
                add(name, 0, a, la, embed(c, 2), (0, 3) if la else (), kind)
        elif name == "f12_mul_line":
            for a, la, kind in elements(6, n_rand):
                s = rng.randrange(P) if kind == "random" else P - 1
                c = [rng.randrange(P) for _ in range(4)] if kind == "random" else [P - 1, 1, 0, P - 1]
                lz = P if la else 0
                wb = limbs(mont(s) + lz) + limbs(mont(c[0]) + lz) + limbs(mont(c[1])) + limbs(mont(c[2])) + \
                    limbs(mont(c[3]) + lz) + [0] * (108 - 45)
                line = from_tower([s, 0, c[0], c[1], 0, 0, c[2], c[3], 0, 0, 0, 0])
                add(name, 0, a, la, line, (), kind, wb)
        elif name in TOWER_BINARY:
            els = elements(n_f2, n_rand)
            for i, (a, la, kind) in enumerate(els):
                b, lb, _k = els[(i * 7 + 3) % len(els)] if kind == "random" else els[n_rand + (i * 5) % (len(els) - n_rand)]
                add(name, 0, a, la, b, lb, kind)
        else:
            for a, la, kind in elements(n_f2, n_rand):
                add(name, 0, a, la, zero, (), kind)
    return recs


def check_tower(r, out):
    a, b = r.meta
    got, err = f12_of(out[:108], TOWER_SIZE.get(r.op, 6))
    if err:
        return err
    if r.op in ("f2_inv", "f6_inv", "f12_inv"):          # the inverse is unique: a * got == 1 (and 0 -> 0)
        if a == [0] * 12:
            return None if got == a else "inverse of 0 is not 0"
        return None if op.f12_mul(a, got) == op.F12_ONE else "a * inv(a) != 1"
    want = tower_expect(r.op, r.aux, a, b)
    return None if got == want else f"element differs from the oracle: {got[:2]} .. != {want[:2]} .."


# ---- PAIR ------------------------------------------------------------------------------------------------------------
def line_values(q, p):
    """the kLines line values of the Miller loop of (q, p), in step order (oracle/pairing.py: miller_loop)"""
    out, r_pt = [], q
    for i in range(op.ATE_LOOP_COUNT.bit_length() - 2, -1, -1):
        l, r_pt = op._step(r_pt, r_pt, p)
        out.append(l)
        if (op.ATE_LOOP_COUNT >> i) & 1:
            l, r_pt = op._step(r_pt, q, p)
            out.append(l)
    q1 = (op.f2_mul(op.f2_conj(q[0]), op.GAMMA_X1), op.f2_mul(op.f2_conj(q[1]), op.GAMMA_Y1))
    nq2 = (op.f2_mul(q[0], op.GAMMA_X2), op.f2_sub((0, 0), op.f2_mul(q[1], op.GAMMA_Y2)))
    l, r_pt = op._step(r_pt, q1, p)
    out.append(l)
    out.append(op._step(r_pt, nq2, p)[0])
    return out


def g1_words(p, lazy=False):
    if p is None:
        return [0] * 18 + [1]
    lz = P if lazy else 0
    return limbs(mont(p[0]) + lz) + limbs(mont(p[1]) + lz) + [0]


def gen_pair(rng):
    """returns (records, G2 table).  Checks e(P1, Q1) e(P2, Q2) built from random scalars; Q by index, NULLQ = infinity"""
    H = op.G2_GEN
    bs = [rng.randrange(1, R) for _ in range(3)]
    g2 = [H] + [op.g2_mul(H, b) for b in bs]
    recs = []

    def add(name, aux, p1, q1, p2, q2, f, meta, kind, lazy=False):
        for s in (0, 1):
            words = g1_words(p1, lazy) + g1_words(p2, lazy) + [q1, q2] + (f12_words(f) if f else [0] * 108)
            recs.append(Rec("pair", name, 0, s, aux, words, meta, kind))
    G = bn.G1_GEN
    for i in range(8):
        a = rng.randrange(1, R)
        qi = 1 + i % 3
        pa = bn.g1_mul(G, a)
        pab = bn.g1_mul(G, a * bs[qi - 1] % R)
        f = [rng.randrange(P) for _ in range(12)]
        idx = rng.randrange(102) if i else 101
        for k in range(8):                                # eight products per point pair: other f, other line
            add("mul_prepared", idx if k == 0 else rng.randrange(102), pa, qi, None, NULLQ, f, None, "random",
                lazy=(i + k) % 2 == 1)
            recs[-1].meta = recs[-2].meta = (f, g2[qi], pa, recs[-1].aux)
            f = [rng.randrange(P) for _ in range(12)]
        add("miller2", 0, pa, qi, pab, 0, None, ((pa, g2[qi]), (pab, H)), "random", lazy=i % 2 == 1)
        add("pairing2", 0, pa, qi, None, 0, None, ((pa, g2[qi]), (None, H)), "random")
        # e(aG, bH) e(-abG, H) == 1; off by one it is not
        bad = bn.g1_mul(G, (a * bs[qi - 1] + 1) % R)
        add("check2", 0, pa, qi, neg_pt(pab), 0, None, ((pa, g2[qi]), (neg_pt(pab), H)), "random")
        add("check2", 0, pa, qi, neg_pt(bad), 0, None, ((pa, g2[qi]), (neg_pt(bad), H)), "random")
    p = bn.g1_mul(G, rng.randrange(1, R))
    edge = [((p, 1), (neg_pt(p), 1)), ((p, 1), (p, 1)), ((G, 0), (neg_pt(G), 0)), ((None, 1), (None, 0)),
            ((None, 1), (p, 0)), ((p, 1), (None, 0)), ((p, NULLQ), (p, 0)), ((p, 1), (p, NULLQ)),
            ((p, NULLQ), (neg_pt(p), NULLQ)), ((p, NULLQ), (None, 2))]
    for (p1, q1), (p2, q2) in edge:
        meta = ((p1, None if q1 == NULLQ else g2[q1]), (p2, None if q2 == NULLQ else g2[q2]))
        add("check2", 0, p1, q1, p2, q2, None, meta, "edge")
        if q1 != NULLQ or q2 != NULLQ:
            add("miller2", 0, p1, q1, p2, q2, None, meta, "edge")
    add("pairing2", 0, G, 0, None, 0, None, ((G, H), (None, H)), "edge")
    add("pairing2", 0, p, 1, neg_pt(p), 1, None, ((p, g2[1]), (neg_pt(p), g2[1])), "edge")
    add("mul_prepared", 0, None, 1, None, NULLQ, list(op.F12_ONE), (list(op.F12_ONE), g2[1], None, 0), "edge")
    add("mul_prepared", 0, G, 0, None, NULLQ, list(op.F12_ONE), (list(op.F12_ONE), H, G, 0), "edge")
    return recs, g2


_ML_CACHE, _G1MUL_CACHE, _LINES_CACHE = {}, {}, {}


def _miller(q, p):
    if (q, p) not in _ML_CACHE:
        _ML_CACHE[(q, p)] = op.miller_loop(q, p)
    return _ML_CACHE[(q, p)]


def _g1_mul(pt, k):
    if (pt, k) not in _G1MUL_CACHE:
        _G1MUL_CACHE[(pt, k)] = bn.g1_mul(pt, k)
    return _G1MUL_CACHE[(pt, k)]


def check_pair(r, out):
    m = r.meta
    if r.op == "check2":
        f = list(op.F12_ONE)
        for p, q in m:
            f = op.f12_mul(f, _miller(q, p))
        want = int(tower_expect("final_exp", 0, f, None) == op.F12_ONE)   # m < r, r prime: f^(m e) == 1 iff f^e == 1
        if any(out[:108]):
            return "words beside the verdict are not 0"
        return None if out[108] == want else f"verdict {out[108]} != {want}"
    got, err = f12_of(out[:108])
    if err:
        return err
    if r.op == "mul_prepared":
        f, q, p, idx = m
        if p is not None and (q, p) not in _LINES_CACHE:
            _LINES_CACHE[(q, p)] = line_values(q, p)
        want = f if p is None else op.f12_mul(f, _LINES_CACHE[(q, p)][idx])
    else:
        want = list(op.F12_ONE)
        for p, q in m:
            want = op.f12_mul(want, _miller(q, p))
        if r.op == "pairing2":
            want = tower_expect("final_exp", 0, want, None)
    return None if got == want else "element differs from the oracle"


# ---- files -----------------------------------------------------------------------------------------------------------
GEN = {"field": gen_field, "field32": gen_field32, "curve": gen_curve, "quad": gen_quad, "tower": gen_tower}
CHECK = {"field": check_field, "field32": check_field32, "curve": check_curve, "quad": check_quad, "tower": check_tower,
         "pair": check_pair}
_CACHE = {}


def generate(seed=0xDC29):
    """{group: [Rec]}, G2 table; deterministic in the seed"""
    if seed not in _CACHE:
        rng = random.Random(seed)
        recs = {g: GEN[g](rng) for g in GROUPS[:5]}
        recs["pair"], g2 = gen_pair(rng)
        for g in GROUPS:
            for r in recs[g]:
                if r.kind != "random":
                    EDGE_COUNTS[r.key()] = EDGE_COUNTS.get(r.key(), 0) + 1
        _CACHE[seed] = (recs, g2)
    return _CACHE[seed]


def write_vectors(path, recs, g2):
    with open(path, "wb") as f:
        f.write(struct.pack("<3I", MAGIC, len(GROUPS), len(g2)))
        r256 = 1 << 256
        for q in g2:
            for c in (q[0][0], q[0][1], q[1][0], q[1][1]):
                f.write(struct.pack("<8I", *fe_words(c * r256 % P)))
        for gi, g in enumerate(GROUPS):
            f.write(struct.pack("<2I", gi, len(recs[g])))
            for r in recs[g]:
                w = [OPS[g][r.op], r.field, r.sched, r.aux] + r.words
                assert len(w) == IN_WORDS[gi], (g, r.op, len(w))
                f.write(struct.pack("<%dI" % len(w), *w))


def read_results(path):
    """{group: [list of out words per record]}"""
    data = open(path, "rb").read()
    head = struct.unpack_from("<2I", data, 0)
    assert head == (MAGIC, len(GROUPS)), "not a devcheck result file"
    off, out = 8, {}
    for gi, g in enumerate(GROUPS):
        gid, n = struct.unpack_from("<2I", data, off)
        assert gid == gi
        off += 8
        ow = OUT_WORDS[gi]
        words = struct.unpack_from("<%dI" % (n * ow), data, off)
        off += 4 * n * ow
        out[g] = [list(words[i * ow:(i + 1) * ow]) for i in range(n)]
    assert off == len(data), "trailing bytes in the result file"
    return out


def check_group(group, recs, results):
    """-> (failures [(index, Rec, message)], counts {key: {"random": n, "edge": n}}); every record is checked"""
    fails, counts = [], defaultdict(lambda: {"random": 0, "edge": 0})
    if len(results) != len(recs):
        return [(-1, None, f"{len(results)} result records for {len(recs)} vectors")], counts
    for i, (r, out) in enumerate(zip(recs, results)):
        if all(w == POISON for w in out):
            fails.append((i, r, "record left at its 0xFF fill (never written)"))
            continue
        if out[-1] != DONE + OPS[group][r.op]:
            fails.append((i, r, f"done marker {out[-1]:#x}"))
            continue
        msg = CHECK[group](r, out)
        if msg:
            fails.append((i, r, msg))
        counts[r.key()]["random" if r.kind == "random" else "edge"] += 1
    return fails, counts


def check_floors(group, recs, counts):
    """every (field, schedule, op) of the group was checked on at least its floor of random records and on every edge
    record the generator's rules admitted for it (EDGE_COUNTS, recorded by generate(); at least MIN_EDGES)"""
    msgs = []
    fields = (0, 1) if group in ("field", "field32") else (0,)
    scheds = (0,) if group == "field32" else (0, 1)
    for f in fields:
        for s in scheds:
            for name in OPS[group]:
                key = (group, f, s, name)
                c = counts.get(key, {"random": 0, "edge": 0})
                floor = 0 if name in CHAIN_OPS else 8 if name in HEAVY_OPS else RANDOM_FLOOR[group]
                if c["random"] < floor:
                    msgs.append(f"{group}.{name} field={f} sched={s}: {c['random']} random records checked, floor {floor}")
                want = max(EDGE_COUNTS.get(key, 0), CHAIN_OPS.get(name, MIN_EDGES[group]))
                if c["edge"] < want:
                    msgs.append(f"{group}.{name} field={f} sched={s}: {c['edge']} edge records checked, {want} admitted")
    return msgs


def format_fails(fails, limit=8):
    return "\n".join(f"  #{i} {r.describe() if r else ''}: {m}" for i, r, m in fails[:limit]) + \
        (f"\n  ... {len(fails)} failures" if len(fails) > limit else "")


def compare_files(a, b, groups=GROUPS):
    """limb-for-limb comparison of two result sets -> [(group, index)] of differing records"""
    return [(g, i) for g in groups for i, (x, y) in enumerate(zip(a[g], b[g])) if x != y] + \
        [(g, -1) for g in groups if len(a[g]) != len(b[g])]


# ---- the host driver -------------------------------------------------------------------------------------------------
HOST_SRC = os.path.join(HERE, "hip", "devcheck_host.cpp")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def host_cxx():
    """a host C++ compiler, or None"""
    import shutil
    for c in ("g++", CLANG, "clang++"):
        if shutil.which(c) or os.path.exists(c):
            return c
    return None


def build_host(out, flags=(), cxx=None):
    import subprocess
    subprocess.check_call([cxx or host_cxx(), "-std=c++17", *flags, HOST_SRC, "-o", out])
    return out


def run_driver(exe, vec, res):
    import subprocess
    out = subprocess.run([exe, vec, res], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, f"{exe} exited with {out.returncode}: {out.stderr[-800:]}"
    return read_results(res)
