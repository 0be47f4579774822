"""The block verifier's front end and fold (cap_amd/csrc/verify_front.hpp, the kernels of verify_kernels.hpp) in Python
integers: the input checks, the seven challenges, the 34 scalars of a proof, the seed S, the weights r_i, the gathered
point and scalar arrays of the two MSMs, and the two sums A and -B.  It shares no code with the product: challenges come
from oracle.plonk.SolidityTranscript, hashes from oracle.bn254.keccak256, the two sums from oracle.capref.msm_g1.
tests/test_verify_block_model.py checks it against oracle.plonk.verifier_pairing_inputs without a GPU;
tests/test_gpu_verifycheck.py compares what tests/hip/verifycheck dumps with it, word for word.

Field elements travel as the product holds them - 256-bit Montgomery words - so that a non-canonical encoding (v + r,
x + p) can be written down: `raw` below always means that word as an integer, `value` the residue it stands for.

The term order (verify_front.hpp) of one proof, t = 0 .. 33, with the proof's 13 points in the order of capgpu_proof
(wires 0..4, z 5, quotient parts 6..10, opening 11, shifted opening 12):
   0 opening, 1 shifted opening                              the a-terms
   2..6 wires, 7 z, 8..12 quotient parts, 13 opening, 14 shifted opening     b-terms on the proof's own points
   15..27 selectors, 28..32 sigmas, 33 the generator         b-terms on the key's points"""
import struct
from dataclasses import dataclass, field

import numpy as np

from oracle import bn254 as bn
from oracle import capref as cr
from oracle import plonk as pl

R, P = bn.R, bn.P
TERMS, A_TERMS, OWN_TERMS, KEY_TERMS = 34, 2, 15, 19
OWN_POINT = [11, 12, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12]      # own term t -> index among the proof's 13 points
PROOF_BYTES, VK_BYTES = 1152, 16 + 32 * 5 + 64 * 18


def mont(v, m=R):
    return bn.to_mont(v % m, m)


def unmont(raw, m=R):
    return bn.from_mont(raw, m)


@dataclass
class Key:
    """a verifying key: points as canonical (x, y) / None"""
    n: int
    num_inputs: int
    sel: list
    sig: list

    def struct_bytes(self):
        """capgpu_verifying_key"""
        out = struct.pack("<QQ", self.n, self.num_inputs)
        out += b"".join(mont(k).to_bytes(32, "little") for k in pl.K)
        out += cr.points_to_array(list(self.sel) + list(self.sig)).tobytes()
        assert len(out) == VK_BYTES
        return out

    @classmethod
    def from_ctypes(cls, vk):
        pts = np.frombuffer(bytes(vk), dtype=np.uint64)[2 + 20:].reshape(18, 8)
        pts = [cr.affine_to_ints(p) for p in pts]
        return cls(int(vk.domain_size), int(vk.num_inputs), pts[:13], pts[13:])


@dataclass
class Proof:
    """a capgpu_proof as raw words: 13 points (x_raw, y_raw), 10 evaluations"""
    pts: list
    ev: list

    def struct_bytes(self):
        out = b"".join(x.to_bytes(32, "little") + y.to_bytes(32, "little") for x, y in self.pts)
        out += b"".join(e.to_bytes(32, "little") for e in self.ev)
        assert len(out) == PROOF_BYTES
        return out

    @classmethod
    def from_bytes(cls, b):
        b = bytes(b)
        assert len(b) == PROOF_BYTES
        w = [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(36)]
        return cls([(w[2 * i], w[2 * i + 1]) for i in range(13)], w[26:])

    @classmethod
    def from_values(cls, pts, ev):
        """canonical points (None = infinity) and evaluations"""
        return cls([(0, 0) if p is None else (mont(p[0], P), mont(p[1], P)) for p in pts], [mont(e) for e in ev])


def point_value(raw):
    """raw (x, y) -> "bad" (non-canonical or off the curve), None (infinity, the all-zero words) or canonical (x, y)"""
    x, y = raw
    if x >= P or y >= P:
        return "bad"
    if x == 0 and y == 0:
        return None
    xv, yv = unmont(x, P), unmont(y, P)
    return (xv, yv) if (yv * yv - xv * xv * xv - 3) % P == 0 else "bad"


@dataclass
class Front:
    """what the front end leaves for one proof that passed its checks"""
    chal: dict
    scalars: list
    points: list = field(default_factory=list)     # the proof's 13 points as values


def front(key: Key, pubs_raw, proof: Proof, msg):
    """-> Front, or None for a proof that fails its input checks (a point off the curve or non-canonical, an evaluation or
    public input >= r, zeta inside the domain).  pubs_raw: the key's num_inputs public inputs, raw words."""
    assert len(pubs_raw) == key.num_inputs
    pts = [point_value(p) for p in proof.pts]
    if any(p == "bad" for p in pts) or any(e >= R for e in proof.ev) or any(p >= R for p in pubs_raw):
        return None
    ev = [unmont(e) for e in proof.ev]
    pubs = [unmont(p) for p in pubs_raw]
    n = key.n
    tr = pl.SolidityTranscript()
    tr.append_message(bytes(msg) if msg else b"")
    tr.append_vk_and_pub_input(n, key.num_inputs, key.sel, key.sig, pubs)
    for c in pts[:5]:
        tr.append_commitment(c)
    tr.get_and_append_challenge()                     # plookup's tau
    beta = tr.get_and_append_challenge()
    gamma = tr.get_and_append_challenge()
    tr.append_commitment(pts[5])
    alpha = tr.get_and_append_challenge()
    for c in pts[6:11]:
        tr.append_commitment(c)
    zeta = tr.get_and_append_challenge()
    for e in ev:
        tr.append_fr(e)
    v = tr.get_and_append_challenge()
    tr.append_commitment(pts[11])
    tr.append_commitment(pts[12])
    u = tr.get_and_append_challenge()
    zh = (pow(zeta, n, R) - 1) % R
    if zh == 0 or zeta == 1:
        return None
    omega = bn.root_of_unity(n.bit_length() - 1)
    inv = lambda a: pow(a % R, R - 2, R)
    we, se, znext = ev[:5], ev[5:9], ev[9]
    l1 = zh * inv(n * (zeta - 1)) % R
    pi = sum(p * zh * pow(omega, j, R) * inv(n * (zeta - pow(omega, j, R))) for j, p in enumerate(pubs)) % R
    prod = 1
    for j in range(4):
        prod = prod * (we[j] + beta * se[j] + gamma) % R
    r0 = (pi - alpha * alpha * l1 - alpha * znext * (we[4] + gamma) * prod) % R
    s = [0] * TERMS
    s[0], s[1] = 1, u
    for j in range(5):
        s[2 + j] = pow(v, j + 1, R)
        s[8 + j] = -zh * pow(zeta, j * (n + 2), R) % R
    cz = alpha
    for j in range(5):
        cz = cz * (we[j] + beta * pl.K[j] * zeta + gamma) % R
    s[7] = (cz + alpha * alpha * l1 + u) % R
    s[13], s[14] = zeta, u * zeta * omega % R
    sel = 15
    for j in range(4):
        s[sel + j] = we[j]
        s[sel + 6 + j] = pow(we[j], 5, R)
    s[sel + 4], s[sel + 5] = we[0] * we[1] % R, we[2] * we[3] % R
    s[sel + 10], s[sel + 11] = -we[4] % R, 1
    s[sel + 12] = we[0] * we[1] * we[2] * we[3] * we[4] % R
    for j in range(4):
        s[28 + j] = pow(v, 6 + j, R)
    s[32] = -alpha * beta * znext * prod % R
    e_acc = (-r0 + sum(pow(v, j + 1, R) * ev[j] for j in range(9)) + u * znext) % R
    s[33] = -e_acc % R
    chal = dict(beta=beta, gamma=gamma, alpha=alpha, zeta=zeta, v=v, u=u)
    return Front(chal, s, pts)


_memo = {}


def _front_memo(key, pubs_raw, proof, msg):
    """front() once per (key, inputs, proof, message): the cases share their proofs"""
    k = (key.struct_bytes(), tuple(pubs_raw), proof.struct_bytes(), bytes(msg) if msg else b"")
    if k not in _memo:
        _memo[k] = front(key, pubs_raw, proof, msg)
    return _memo[k]


def term_point(key: Key, fr: Front, t):
    if t < OWN_TERMS:
        return fr.points[OWN_POINT[t]]
    return (list(key.sel) + list(key.sig) + [bn.G1_GEN])[t - OWN_TERMS]


def weight_seed(ubytes):
    return bn.keccak256(b"".join(ubytes))


def weight(S, i):
    if i == 0:
        return 1
    return int.from_bytes(bn.keccak256(S + struct.pack("<Q", i))[:16], "little")


def _affine_words(jac):
    return cr.g1_to_affine(jac).astype(np.uint64)


def _neg_words(aff):
    """(x, y) -> (x, -y) on raw Montgomery words; (0, 0) stays"""
    out = np.array(aff, np.uint64).copy()
    if out.any():
        y = cr.array_to_ints(out[4:8])[0]
        out[4:8] = cr.int_to_limbs((P - y) % P)
    return out


@dataclass
class Block:
    valid: list            # per proof: 0 / 1
    ubytes: list           # per proof: 32 bytes
    scalars: list          # per proof: 34 values
    fronts: list
    S: bytes
    weights: list          # values (r_i)
    pts: np.ndarray        # (15 count + 19 keys, 8) raw words: the gathered points
    sc: list               # the gathered scalars, values
    A: np.ndarray          # 8 raw words, (0, 0) = infinity
    negB: np.ndarray


def block(keys, key_of, pubs_raw, proofs, msgs):
    """keys: the call's keys in order of first appearance; key_of[i]: proof i's index among them; pubs_raw[i]: its key's
    public inputs (raw words)"""
    count, nkeys = len(proofs), len(keys)
    fronts = [_front_memo(keys[key_of[i]], pubs_raw[i], proofs[i], msgs[i]) for i in range(count)]
    valid = [0 if f is None else 1 for f in fronts]
    ubytes = [bytes(32) if f is None else bn.fr_to_bytes_le(f.chal["u"]) for f in fronts]
    scalars = [[0] * TERMS if f is None else f.scalars for f in fronts]
    S = weight_seed(ubytes)
    w = [weight(S, i) for i in range(count)]
    npts = OWN_TERMS * count + KEY_TERMS * nkeys
    pts = np.zeros((npts, 8), np.uint64)
    sc = [0] * npts
    for i, f in enumerate(fronts):
        if f is None:
            continue
        raw = np.frombuffer(proofs[i].struct_bytes()[:13 * 64], dtype=np.uint64).reshape(13, 8)
        for t in range(OWN_TERMS):
            at = A_TERMS * i + t if t < A_TERMS else A_TERMS * count + (OWN_TERMS - A_TERMS) * i + (t - A_TERMS)
            pts[at] = raw[OWN_POINT[t]]
            sc[at] = w[i] * f.scalars[t] % R
    for k, key in enumerate(keys):
        kp = cr.points_to_array(list(key.sel) + list(key.sig) + [bn.G1_GEN])
        for j in range(KEY_TERMS):
            at = OWN_TERMS * count + KEY_TERMS * k + j
            pts[at] = kp[j]
            sc[at] = sum(w[i] * fronts[i].scalars[OWN_TERMS + j] for i in range(count)
                         if key_of[i] == k and fronts[i] is not None) % R
    na = A_TERMS * count
    sc_arr = cr.ints_to_array(sc)
    A = _affine_words(cr.msm_g1(pts[:na], sc_arr[:na]))
    B = _affine_words(cr.msm_g1(pts[na:], sc_arr[na:]))
    return Block(valid, ubytes, scalars, fronts, S, w, pts, sc, A, _neg_words(B))


# ---- the case file of tests/hip/verifycheck ----------------------------------------------------------------------------
MAGIC_IN, MAGIC_OUT = 0x5645524946434153, 0x56455249464F5554
SENTINEL = 0xA5
GUARD = 256                 # sentinel bytes the driver keeps behind every dumped buffer


@dataclass
class Case:
    name: str
    keys: list
    key_of: list
    pubs_raw: list         # per proof: its key's inputs, raw words
    proofs: list
    msgs: list

    @property
    def pub_stride(self):
        return max([k.num_inputs for k in self.keys] + [0])


def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", MAGIC_IN, len(cases)))
        for c in cases:
            count, stride = len(c.proofs), c.pub_stride
            msgs = [bytes(m) if m else b"" for m in c.msgs]
            blob = b"".join(msgs)
            f.write(struct.pack("<QQQQ", count, len(c.keys), stride, len(blob)))
            for k in c.keys:
                f.write(k.struct_bytes())
            off = 0
            for i in range(count):
                f.write(struct.pack("<IIII", c.key_of[i], off, len(msgs[i]), 0))
                off += len(msgs[i])
            for p in c.proofs:
                f.write(p.struct_bytes())
            for i in range(count):
                row = list(c.pubs_raw[i]) + [0] * (stride - len(c.pubs_raw[i]))
                f.write(b"".join(v.to_bytes(32, "little") for v in row))
            f.write(blob)


@dataclass
class Dump:
    rc: int
    valid: np.ndarray      # int32, count
    ubytes: bytes          # 32 count
    sc: np.ndarray         # (count * 34, 4) u64
    S: bytes
    w: np.ndarray          # (count, 4)
    pts: np.ndarray        # (npts, 8)
    msc: np.ndarray        # (npts, 4)
    ab: np.ndarray         # (2, 8): A, -B
    guards: dict           # buffer name -> the GUARD bytes behind it


def read_results(path, cases):
    out = []
    with open(path, "rb") as f:
        magic, n = struct.unpack("<QQ", f.read(16))
        assert magic == MAGIC_OUT and n == len(cases)
        for c in cases:
            rc, count, npts = struct.unpack("<QQQ", f.read(24))
            assert count == len(c.proofs) and npts == OWN_TERMS * count + KEY_TERMS * len(c.keys)
            guards = {}

            def take(name, nbytes):
                b = f.read(nbytes + GUARD)
                assert len(b) == nbytes + GUARD, "short result file"
                guards[name] = b[nbytes:]
                return b[:nbytes]
            valid = np.frombuffer(take("valid", 4 * count), dtype=np.int32)
            ub = take("ubytes", 32 * count)
            sc = np.frombuffer(take("scalars", 32 * TERMS * count), dtype=np.uint64).reshape(-1, 4)
            S = take("S", 32)
            w = np.frombuffer(take("weights", 32 * count), dtype=np.uint64).reshape(-1, 4)
            pts = np.frombuffer(take("gathered points", 64 * npts), dtype=np.uint64).reshape(-1, 8)
            msc = np.frombuffer(take("gathered scalars", 32 * npts), dtype=np.uint64).reshape(-1, 4)
            ab = np.frombuffer(take("A and -B", 128), dtype=np.uint64).reshape(2, 8)
            out.append(Dump(rc, valid, ub, sc, S, w, pts, msc, ab, guards))
    return out


def check_case(c: Case, d: Dump, want: Block = None):
    """-> complaints (empty: every dumped word equals the model's)"""
    bad = []
    if d.rc != 0:
        return [f"{c.name}: the driver reports {d.rc}"]
    m = want or block(c.keys, c.key_of, c.pubs_raw, c.proofs, c.msgs)
    count = len(c.proofs)
    for name, g in d.guards.items():
        if g != bytes([SENTINEL]) * GUARD:
            bad.append(f"{c.name}: the bytes behind {name} lost the sentinel")
    if list(d.valid) != m.valid:
        bad.append(f"{c.name}: valid {list(d.valid)} != {m.valid}")
        return bad
    if d.ubytes != b"".join(m.ubytes):
        bad.append(f"{c.name}: u bytes differ")
    got_sc = cr.array_to_ints(d.sc)
    for i in range(count):
        for t in range(TERMS):
            raw = got_sc[TERMS * i + t]
            want_raw = mont(m.scalars[i][t]) if m.valid[i] else 0
            if raw != want_raw:
                bad.append(f"{c.name}: proof {i} scalar {t}: {raw:#x} != {want_raw:#x}")
    if d.S != m.S:
        bad.append(f"{c.name}: S {d.S.hex()} != {m.S.hex()}")
    for i, raw in enumerate(cr.array_to_ints(d.w)):
        if raw != mont(m.weights[i]):
            bad.append(f"{c.name}: weight {i}: {raw:#x} is not the Montgomery image of {m.weights[i]:#x}")
    if not np.array_equal(d.pts, m.pts):
        rows_ = sorted(set(np.nonzero(d.pts != m.pts)[0].tolist()))
        bad.append(f"{c.name}: gathered points differ at {rows_[:8]}")
    for at, raw in enumerate(cr.array_to_ints(d.msc)):
        if raw != mont(m.sc[at]):
            bad.append(f"{c.name}: gathered scalar {at}: {raw:#x} != Montgomery image of {m.sc[at]:#x}")
    if not np.array_equal(d.ab[0], m.A):
        bad.append(f"{c.name}: A differs")
    if not np.array_equal(d.ab[1], m.negB):
        bad.append(f"{c.name}: -B differs")
    return bad


# ---- cases: the fold is arithmetic on well-formed data, so the "proofs" are random points, evaluations and messages ----
def _raw_points(rng, k):
    arr = cr.g1_fixed_base_batch(cr.ints_to_array([rng.randrange(1, R) for _ in range(k)]))
    return [tuple(cr.array_to_ints(a)) for a in arr]


def random_key(rng, log_n, num_inputs):
    pts = [(unmont(x, P), unmont(y, P)) for x, y in _raw_points(rng, 18)]
    return Key(1 << log_n, num_inputs, pts[:13], pts[13:])


def random_proof(rng):
    return Proof(_raw_points(rng, 13), [mont(rng.randrange(R)) for _ in range(10)])


def random_pubs(rng, key):
    return [mont(rng.randrange(R)) for _ in range(key.num_inputs)]


MSG_LENS = (0, 135, 136, 137)          # the padded message around the sponge's 136-byte rate


def random_msg(rng, i):
    return bytes(rng.randrange(256) for _ in range(MSG_LENS[i % 4]))


def off_curve(pr, i=11):
    out = Proof(list(pr.pts), list(pr.ev))
    i %= 13
    out.pts[i] = (out.pts[i][0] ^ 1, out.pts[i][1])
    return out


def non_canonical(pr, i=2):
    out = Proof(list(pr.pts), list(pr.ev))
    out.ev[i % 10] += R
    return out


def make_cases(seed=0x5EED):
    """The smallest shapes at which each kernel can go wrong.  The counts share one list of 66 proofs (the model's front
    end is memoised per proof; 130 takes them round twice, under weights of its own): 4 and 5 proofs lie on either side
    of one 136-byte block of the seed's message, 17 and 34 fill blocks exactly, 64, 65 and 130 cover the fold's lane
    stride and its LDS tree."""
    import random
    rng = random.Random(seed)
    k1 = random_key(rng, 8, 1)
    k0 = random_key(rng, 7, 0)
    k65 = random_key(rng, 9, 65)
    distinct = 66
    pool = [random_proof(rng) for _ in range(distinct)]
    pubs1 = [random_pubs(rng, k1) for _ in range(distinct)]
    pubs65 = [random_pubs(rng, k65) for _ in range(8)] + [None] * (distinct - 9) + [random_pubs(rng, k65)]
    msgs = [random_msg(rng, i) for i in range(distinct)]
    cases = []
    for count in (1, 2, 4, 5, 17, 34, 64, 65, 130):
        at = [i % distinct for i in range(count)]
        cases.append(Case(f"one key, {count} proofs", [k1], [0] * count, [pubs1[i] for i in at], [pool[i] for i in at],
                          [msgs[i] for i in at]))
    # two keys interleaved: 0 and 65 public inputs; then 0 and 1 across the wave boundary
    key_of = [i % 2 for i in range(5)]
    cases.append(Case("two keys interleaved, 5 proofs", [k0, k65], key_of,
                      [pubs65[i] if key_of[i] else [] for i in range(5)], pool[:5], msgs[:5]))
    key_of = [i % 2 for i in range(65)]
    cases.append(Case("two keys interleaved, 65 proofs", [k0, k1], key_of,
                      [pubs1[i] if key_of[i] else [] for i in range(65)], pool[:65], msgs[:65]))
    # three keys, every proof of the middle one invalid: its 19 folded scalars are 0, its points still written
    key_of = [0, 1, 2, 1, 0, 2, 1]
    prs = [off_curve(pool[i], i) if key_of[i] == 1 and i % 2 else non_canonical(pool[i], i) if key_of[i] == 1 else pool[i]
           for i in range(7)]
    cases.append(Case("three keys, the middle one without a valid proof", [k1, k65, k0], key_of,
                      [pubs1[i] if key_of[i] == 0 else pubs65[i] if key_of[i] == 1 else [] for i in range(7)], prs, msgs[:7]))
    cases.append(Case("a key used by the last proof only", [k1, k65], [0, 0, 0, 1], pubs1[:3] + [pubs65[3]], pool[:4],
                      msgs[:4]))
    # invalid proofs of both kinds at the first, a middle and the last index; a non-canonical public input
    for name, kinds in (("off-curve, non-canonical, off-curve", (off_curve, non_canonical, off_curve)),
                        ("non-canonical, off-curve, non-canonical", (non_canonical, off_curve, non_canonical))):
        prs = list(pool[:5])
        prs[0], prs[2], prs[4] = kinds[0](pool[0], 0), kinds[1](pool[2], 9), kinds[2](pool[4], 12)
        cases.append(Case(f"invalid at 0, 2, 4: {name}", [k1], [0] * 5, pubs1[:5], prs, msgs[:5]))
    # across the wave boundary, with a key of 65 inputs that only the last proof uses
    prs = list(pool[:66])
    prs[63], prs[64] = off_curve(pool[63], 5), non_canonical(pool[64], 0)
    last = list(pubs65[65])
    last[64] += R
    cases.append(Case("invalid at 63, 64 and (public input 64 + r, the only proof of its key) 65", [k1, k65],
                      [0] * 65 + [1], pubs1[:65] + [last], prs, msgs[:66]))
    cases.append(Case("65 inputs, the key of the last of 66 proofs only", [k1, k65], [0] * 65 + [1],
                      pubs1[:65] + [pubs65[65]], pool[:66], msgs[:66]))
    cases.append(Case("every proof invalid", [k1], [0] * 3, pubs1[:3],
                      [off_curve(pool[0]), non_canonical(pool[1]), off_curve(pool[2], 0)], msgs[:3]))
    # data edges
    base = pool[:6]
    zero_ev = Proof(list(base[0].pts), [0] * 10)
    top_ev = Proof(list(base[1].pts), [mont(R - 1)] * 10)
    inf_comms = Proof([(0, 0)] * 11 + list(base[2].pts[11:]), list(base[2].ev))
    twins = Proof(list(base[3].pts), list(base[3].ev))
    twins.pts[3] = twins.pts[2]
    twins.pts[12] = twins.pts[11]
    cases.append(Case("evaluations 0 and r - 1, commitments at (0, 0), equal commitments", [k1], [0] * 6, pubs1[:6],
                      [zero_ev, top_ev, inf_comms, twins, base[4], base[5]], msgs[:6]))
    no_open = [Proof(list(p.pts[:11]) + [(0, 0), (0, 0)], list(p.ev)) for p in pool[:3]]
    cases.append(Case("both openings at infinity: A at infinity", [k1], [0] * 3, pubs1[:3], no_open, msgs[:3]))
    zero_pubs = [[0] for _ in range(2)]
    cases.append(Case("public input 0, r - 1", [k1], [0, 0], [zero_pubs[0], [mont(R - 1)]], pool[:2], [b"", b"x" * 136]))
    return cases
