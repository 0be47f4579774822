"""Records for tests/hip/elemcheck (tests/hip/elemcheck_ops.hpp): single calls of the functions of
cap_amd/csrc/ntt_elem29.hpp - stage butterflies with given twiddle pairs, the element steps of the passes, the bodies of
ntt3_combine and ntt3_combine5 - and the file format the device binary and the host twin share.

Operands are the inputs of tests/test_ntt_elem_host.py cut to single calls: values of each stage's input class
(tests/golden/lazy_envelope.json: 32-byte images into the first stages, normalized values up to the bound behind the
last but one round into the general round, up to the last round's bound into the output steps), at the class's edge -
largest magnitude, every limb saturated - at 0, 1, r - 1, r, and random; zeros on the operands whose butterflies are
copies."""
import json
import os
import random
import struct

import numpy as np

from tests import round_model as rm
from tests.lazy_bound_classes import C256, L29, M256, NORM, R, operand

MAGIC_IN, MAGIC_OUT = 0x454C4D49, 0x454C4D4F
SLOTS, OUTS = 52, 4
OPS = ["radix2", "radix4_shoup", "radix4_mont", "first4_shoup", "first4_mont", "in", "out", "combine3", "finish3",
       "combine5", "perm", "kx", "quot_fold", "quot_direct", "lincomb"]
HOWS = ["sat", "edge", "small", "random", "random", "edge", "random", "random"]
IMAGE_FL = (L29, (1 << 24) - 1, C256 + 1)          # a loaded image: limb 8 has 24 bits
# The classes of the lazy operands come from the committed envelope, so records move with it: the bound behind the
# last but one round of the longest transform into the general round, the last round's into the output steps, and
# ntt3_combine's x2 into its finish.
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lazy_envelope.json")) as _f:
    _ENV = json.load(_f)
BEFORE_LAST = {"radix4_" + short: _ENV["ntt"][form]["11"]["raw_256"]["lds"][-2]
               for short, form in (("shoup", "shoup"), ("mont", "montgomery"))}
LAST = max(_ENV["ntt"][form]["11"]["raw_256"]["lds"][-1] for form in ("shoup", "montgomery"))
X2 = max(_ENV["ntt3_combine"][k] for k in ("x0", "x1", "x2"))

class Rec:
    def __init__(self, op, a0=0, a1=0):
        self.op, self.a0, self.a1, self.slots = OPS.index(op), a0, a1, []

    def fl(self, limbs):
        self.slots.append(list(limbs))
        return self

    def image(self, v):
        self.slots.append([(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)] + [0])
        return self

    def words(self):
        s = self.slots + [[0] * 9] * (SLOTS - len(self.slots))
        assert len(s) == SLOTS
        return [self.op, self.a0, self.a1, 0] + [w for slot in s for w in slot]


def _limbs(v):
    return [(v >> (29 * i)) & L29 for i in range(8)] + [v >> 232]


def generate(per_op=320, seed=0xE1E):
    rng = random.Random(seed)
    val = lambda cls, how: operand(cls, rng, how)[1]
    image = lambda how: {"sat": M256, "edge": M256 - rng.getrandbits(rng.randrange(1, 200)),
                         "small": [0, 1, R - 1, R, R + 1][rng.randrange(5)]}.get(how) if how != "random" \
        else rng.getrandbits(256)
    twiddle = lambda how: {"sat": R - 1, "edge": R - 1 - rng.getrandbits(rng.randrange(1, 200)),
                           "small": [0, 1, 2, R - 2][rng.randrange(4)]}.get(how) if how != "random" \
        else rng.getrandbits(300) % R
    recs = []
    for i in range(per_op):
        how = HOWS[i % len(HOWS)]
        zeros = (i // len(HOWS)) % 4                  # which subtracted operands (b: bit 0, d: bit 1) are zero; 3: both
        z = [0] * 9
        recs.append(Rec("radix2").fl(val(IMAGE_FL, how)).fl(z if zeros & 1 else val(IMAGE_FL, how)))
        for op in ("radix4_shoup", "radix4_mont"):
            r = Rec(op)
            for k in range(4):
                r.fl(z if (k == 1 and zeros & 1) or (k == 3 and zeros & 2) else val(NORM(BEFORE_LAST[op]), how))
            for k in range(3):
                w = twiddle(how if k == i % 3 else "random")
                if op == "radix4_shoup":
                    r.fl(_limbs(w)).fl(_limbs((w << 261) // R))
                else:
                    r.fl(_limbs((w << 261) % R))
            recs.append(r)
        for op in ("first4_shoup", "first4_mont"):
            r = Rec(op)
            for k in range(4):
                r.fl(z if (k == 1 and zeros & 1) or (k == 3 and zeros & 2) else val(IMAGE_FL, how))
            w = twiddle(how)
            recs.append(r.fl(_limbs(w)).fl(_limbs((w << 261) // R)) if op == "first4_shoup"
                        else r.fl(_limbs((w << 261) % R)))
        recs.append(Rec("in", a0=i % 4).image(0 if zeros == 3 else image(how)).image(image("random"))
                    .image(image(how)).image(image("random")))
        form = i % 7
        recs.append(Rec("out", a0=form, a1=(i // 7) % 2).fl(val(NORM(LAST), how))
                    .image(twiddle(how) if form < 2 else image(how)))
        r = Rec("combine3")
        for k in range(6):
            r.image(image(how if k == i % 6 else "random"))
        recs.append(r)
        recs.append(Rec("finish3", a0=i % 3).fl(val(NORM(X2), how)).image(image(how)).image(image("random")))
        r = Rec("combine5", a0=(i % 3) + 16 if i % 2 else (i // 2) % 2, a1=(i // 4) % 4)
        for k in range(SLOTS):
            r.image(image(how if k % 5 == i % 5 else "random"))
        recs.append(r)
    recs += round_records(per_op, rng)
    return recs


def round_records(per_op, rng):
    """single rows and points of the round kernels' bodies (round_elem29.hpp), drawn as tests/round_model.py draws its
    cases: images by the index rule (every fourth saturated), edge challenges, beta = 0, key columns and coset
    evaluations below 2 r, tables canonical; every third record with all its images at the contract's largest"""
    recs = []
    for i in range(per_op):
        top = i % 3 == 0
        canon = lambda k, form="internal": [rm.saturated(rm.CANON)] * k if top else rm.fill(rng, k, rm.CANON, form, phase=i)
        weak = lambda k: [rm.saturated(rm.WEAK)] * k if top else rm.fill(rng, k, rm.WEAK, "internal", phase=i)
        edge = lambda form="internal": rm.draw_edge(rng, rm.CANON, form)
        r = Rec("perm")
        for v in [0 if i % 5 == 1 else edge("ark"), 0 if i % 5 == 2 else edge("ark")] + canon(1, "ark") + \
                [rm.internal(1)] + [edge() for _ in range(4)] + canon(10, "ark"):
            r.image(v)
        recs.append(r)
        recs.append(Rec("kx").image(edge()).image(canon(1)[0]))
        beta = edge() or 1
        chal = [beta, edge(), edge(), edge(), rm.internal(rm.inv(rm.internal_value(beta))), edge()]
        imgs = weak(18) + canon(4) + weak(7) + canon(2)
        recs.append(_images(Rec("quot_fold", a0=i % 6), imgs + chal + [rm.internal(1)] + [edge() for _ in range(4)] + canon(8)))
        chal = [0 if i % 2 else beta, edge(), edge(), edge(), 0, edge()]
        recs.append(_images(Rec("quot_direct", a0=i % 6), imgs + chal + [rm.internal(1)] + [edge() for _ in range(4)] + canon(8)))
        n = (1, 6, 7, 25)[i % 4]
        r = Rec("lincomb", a0=n, a1=(1 << 25) - 1 if top else rng.getrandbits(25))
        for t in range(25):
            r.image(rm.saturated(rm.CANON) if top or t % 7 == 0 else edge()).image(canon(1, "ark")[0])
        recs.append(r)
    return recs


def _images(rec, imgs):
    for v in imgs:
        rec.image(v)
    return rec


def write_records(path, recs):
    a = np.array([r.words() for r in recs], dtype=np.uint32)
    with open(path, "wb") as f:
        f.write(struct.pack("<2I", MAGIC_IN, len(recs)))
        f.write(a.tobytes())


def read_results(path, count):
    with open(path, "rb") as f:
        magic, n = struct.unpack("<2I", f.read(8))
        assert magic == MAGIC_OUT and n == count, (hex(magic), n, count)
        a = np.frombuffer(f.read(), dtype=np.uint32)
    assert a.size == count * OUTS * 9
    return a.reshape(count, OUTS * 9)
