"""What the bound table's tests share (tests/test_ntt_elem_host.py, tests/elemcheck_vectors.py): the constants of
tests/cpp/bound29.hpp as Python integers, and concrete operands inside a class (largest limb 0 .. 7, largest limb 8,
magnitude in units of p / 2^20) - at the class's edge, saturated, or random.  No imports beyond the standard library."""
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
M256 = (1 << 256) - 1
L29, L30, L31 = (1 << 29) - 1, (1 << 30) - 1, (1 << 31) - 1
U = 1 << 20
C256, C261, C262 = (1 << 276) // R, (1 << 281) // R, (1 << 282) // R
TOP = lambda mag: mag * (-(-R >> 212)) >> 40
SUB8, SUB2, SUB16, SUB4 = 0x01832272, 0x0060c89b, 0x030644e5, 0x00c19138        # limb 8 of the inflated constants


def limbs_of(v, lo, hi, rng, spread):
    """v as nine limbs, limbs 0 .. 7 at most lo and limb 8 at most hi; spread: carries pushed back down where lo allows"""
    x = [(v >> (29 * i)) & L29 for i in range(8)] + [v >> 232]
    if x[8] > hi:
        return None
    if spread:
        for i in range(7, -1, -1):
            room = (lo - x[i]) >> 29
            take = min(room, x[i + 1]) if i < 7 else min(room, x[8])
            take = rng.randrange(take + 1) if take > 0 and spread == 1 else max(take, 0)
            x[i] += take << 29
            x[i + 1] -= take
    assert sum(a << (29 * i) for i, a in enumerate(x)) == v and max(x[:8]) <= lo and x[8] <= hi
    return x


def operand(cls, rng, how):
    """a value of the class (lo, hi, mag[, canonical]) - at the edge of the magnitude, saturated limbs, or random"""
    lo, hi, mag = cls[:3]
    vmax = min(mag * R // U, sum(lo << (29 * i) for i in range(8)) + (hi << 232))
    if len(cls) > 3:
        vmax = min(vmax, R - 1)
    if how == "sat":
        x = [lo] * 8 + [hi]
        v = sum(a << (29 * i) for i, a in enumerate(x))
        if v <= vmax:
            return v, x
        how = "edge"
    for attempt in range(50):
        v = vmax - (attempt and rng.randrange(1 << rng.randrange(1, 250))) if how in ("edge", "edge_spread") \
            else rng.randrange(vmax + 1) if how == "random" else [0, 1, R - 1, R, R + 1][rng.randrange(5)]
        v = max(min(v, vmax), 0)
        x = limbs_of(v, lo, hi, rng, {"edge_spread": 2, "random": 1}.get(how, 0))
        if x is not None:
            return v, x
        vmax = min(vmax, ((hi + 1) << 232) - 1)
    raise AssertionError(f"no operand for {cls}")


NORM = lambda mag: (L29, min(TOP(mag), L29), mag)
