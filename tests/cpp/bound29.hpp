// A bound-tracking stand-in for cap::Fl (cap_amd/csrc/field29.hpp): the same static interface, but a value is not a
// number - it is an upper bound on every number a kernel can hold at that point:
//   lo    the largest value a limb 0 .. 7 can have,
//   hi    the largest value limb 8 can have,
//   mag   the magnitude: value <= mag * p / 2^20 (units of p / 2^20, always rounded UP),
//   zero  the value is known to be zero (zero padding) - everything else may or may not be.
// Every operation asserts the precondition that field29.hpp states for it and returns the postcondition stated there,
// so running a kernel's templates (ntt_elem29.hpp, round_elem29.hpp) on it checks the preconditions for ALL inputs
// of a class.  tests/test_ntt_elem_host.py ties the table to the real code: every postcondition here against the
// real operation on operands at the precondition's edge, and every stage bound against the concrete runs.
//
// Branches on a value being zero (fl_any) take the non-zero side unless the value is known to be zero.  That side
// dominates: where the kernels branch, the zero side copies an operand (a) and the other computes a + t and
// a + kp - t with bounds lo(a) + lo(t) >= lo(a) and mag(a) + kp >= mag(a) - subtracted operands have lower bound 0.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../cap_amd/csrc/field29.hpp"
#include "../../cap_amd/csrc/round_elem29.hpp"

namespace capbound {

struct bfl {
  uint64_t lo = 0, hi = 0, mag = 0;
  bool zero = true;
  bool image = false;  // known to be below 2^256 although mag, rounded up, may say C256 + 1: unpacked from 32 bytes and
                       // not touched since, or the join of such values with values of mag <= C256
};
struct bfe {  // a 32-byte image: value < 2^256 and <= mag * p / 2^20
  uint64_t mag = 0;
  bool zero = true;
};

static inline uint32_t fl_any(const bfl& a) { return a.zero ? 0u : 1u; }
static inline uint32_t fe_any(const bfe& a) { return a.zero ? 0u : 1u; }

struct BoundLog {
  static const char*& where() {
    static const char* w = "";
    return w;
  }
  static long& failures() {
    static long f = 0;
    return f;
  }
  static bool& fatal() {
    static bool f = true;
    return f;
  }
  static bool& quiet() {  // count only: a search for the largest class that still closes expects failures
    static bool q = false;
    return q;
  }
};
// Tests for zero modulo p (is_zero) cannot be decided on a bound.  The n-th test since the last reset() answers bit n of
// the plan - 0, the common side, by default - so a caller runs a function once per path; a value known to be zero
// answers true and consumes no bit.
struct BoundBranch {
  static uint32_t& plan() {
    static uint32_t p = 0;
    return p;
  }
  static int& taken() {
    static int n = 0;
    return n;
  }
  static void reset(uint32_t p = 0) {
    plan() = p;
    taken() = 0;
  }
};
#define CAP_BOUND_REQUIRE(cond, op)                                                                   \
  do {                                                                                                \
    if (!(cond)) {                                                                                    \
      capbound::BoundLog::failures()++;                                                                         \
      if (!capbound::BoundLog::quiet())                                                                         \
        fprintf(stderr, "bound violated in %s [%s]: %s\n", op, capbound::BoundLog::where(), #cond);             \
      if (capbound::BoundLog::fatal()) exit(2);                                                                 \
    }                                                                                                 \
  } while (0)

template <class PR>
struct BoundFl {
  using u128 = unsigned __int128;
  static constexpr uint64_t U = 1ull << 20;       // units of magnitude per p
  static constexpr uint64_t L29 = (1ull << 29) - 1, L30 = (1ull << 30) - 1, L31 = (1ull << 31) - 1;
  // For both BN254 moduli (they agree in their top 100 bits; tests/test_ntt_elem_host.py recomputes these):
  static constexpr uint64_t C256 = 5547124;       // floor(2^276 / p): mag <= C256  =>  value < 2^256
  static constexpr uint64_t C261 = 177507980;     // floor(2^281 / p)
  static constexpr uint64_t C262 = 355015960;     // floor(2^282 / p)
  static constexpr uint64_t RT = 3325460688404ull;        // ceil(p / 2^212): limb 8 <= value / 2^232 <= mag RT / 2^40
  static constexpr uint64_t RQ = 108968695837592834ull;   // ceil(p / 2^197): a b / 2^261 <= ma mb RQ / 2^84 units

  static uint64_t top(uint64_t mag) { return (uint64_t)(((u128)mag * RT) >> 40); }
  static uint64_t maxsub(const uint32_t (&k)[9]) {
    uint32_t m = 0;
    for (int i = 0; i < 8; i++) m = k[i] > m ? k[i] : m;
    return m;
  }
  static uint64_t mont(uint64_t ma, uint64_t mb) {  // ceil(ma mb RQ / 2^84)
    const u128 t = (u128)ma * mb;                   // < 2^58 for magnitudes below 2^29
    CAP_BOUND_REQUIRE((t >> 64) == 0, "mont");
    const u128 x = (u128)(uint64_t)t * RQ;
    return (uint64_t)((x + (((u128)1 << 84) - 1)) >> 84);
  }
  static bool normalized(const bfl& a) { return a.lo <= L29 && a.hi <= L29; }
  static bfl norm_of(uint64_t mag, bool zero = false) {  // a normalized value of that magnitude
    bfl r;
    r.zero = zero;
    if (zero) return r;
    r.lo = L29;
    r.hi = top(mag) < L29 ? top(mag) : L29;
    r.mag = mag;
    return r;
  }

  static bfl zero() { return bfl(); }
  static bfl one() { return norm_of(U); }  // a canonical constant
  static bfl konst(const uint32_t (&)[9]) { return norm_of(U); }
  // any image < 2^256: limbs 0 .. 7 < 2^29, limb 8 < 2^24
  static bfl unpack(const bfe& a) {
    bfl r = norm_of(a.mag, a.zero);
    if (!a.zero && r.hi > (1u << 24) - 1) r.hi = (1u << 24) - 1;
    r.image = true;
    return r;
  }
  static bfl load(const bfe& a) { return unpack(a); }
  // normalized value < 2^256 -> image
  static bfe pack(const bfl& a) {
    CAP_BOUND_REQUIRE(normalized(a), "pack");
    CAP_BOUND_REQUIRE(a.mag <= C256 || a.image, "pack");
    bfe r;
    r.mag = a.mag;
    r.zero = a.zero;
    return r;
  }
  // limbs up to < 2^32 - 8 -> normalized, same integer; the result's limb 8 must stay below 2^29 (value < 2^261)
  static bfl normalize(const bfl& a) {
    if (a.zero) return a;
    CAP_BOUND_REQUIRE(a.lo < (1ull << 32) - 8, "normalize");
    CAP_BOUND_REQUIRE(a.hi + 8 < (1ull << 32), "normalize");
    CAP_BOUND_REQUIRE(a.mag <= C261, "normalize");
    bfl r = norm_of(a.mag);
    const uint64_t carried = a.hi + ((a.lo + 7) >> 29);
    if (carried < r.hi) r.hi = carried;
    if (a.lo <= L29 && a.lo < r.lo) r.lo = a.lo;  // (no carry can occur below 2^29 - 1 + 0)
    return r;
  }
  static bfl add(const bfl& a, const bfl& b) {  // limb-wise: no limb may wrap
    bfl r;
    r.lo = a.lo + b.lo;
    r.hi = a.hi + b.hi;
    r.mag = a.mag + b.mag;
    r.zero = a.zero && b.zero;
    CAP_BOUND_REQUIRE(r.lo < (1ull << 32) && r.hi < (1ull << 32), "add");
    return r;
  }
  static bfl add_norm(const bfl& a, const bfl& b) { return normalize(add(a, b)); }
  // a + K p - b, limb by limb against the inflated constant
  static bfl sub_k(const bfl& a, const bfl& b, const uint32_t (&k)[9], uint64_t kp, uint64_t a_lim, uint64_t b_lim,
                   uint64_t b_mag, bool carry, const char* op) {
    CAP_BOUND_REQUIRE(a.lo <= a_lim && a.hi <= a_lim, op);  // "limbs(a)": limb 8 as well
    CAP_BOUND_REQUIRE(b.lo <= b_lim, op);
    CAP_BOUND_REQUIRE(b.hi <= k[8], op);
    CAP_BOUND_REQUIRE(b.mag <= b_mag, op);
    bfl r;
    r.zero = false;
    r.lo = a.lo + maxsub(k);
    r.hi = a.hi + k[8];
    r.mag = a.mag + kp * U;
    CAP_BOUND_REQUIRE(r.lo < (1ull << 32) && r.hi < (1ull << 32), op);
    return carry ? normalize(r) : r;
  }
  static constexpr uint64_t frac(uint64_t num, uint64_t den) { return U * num / den; }  // num / den of p, rounded down
  // a - b + 16p: limbs(a), limbs(b) < 2^30, b < 15.9p
  static bfl sub(const bfl& a, const bfl& b) { return sub_k(a, b, PR::SUB16P, 16, L30, L30, frac(159, 10), true, "sub"); }
  static bfl neg(const bfl& b) { return sub(zero(), b); }
  // a - b + 2p: b normalized < 1.9p, limbs(a) < 2^31
  static bfl sub2p(const bfl& a, const bfl& b) { return sub_k(a, b, PR::SUB2P, 2, L31, L29, frac(19, 10), true, "sub2p"); }
  static bfl sub2p_lazy(const bfl& a, const bfl& b) {
    return sub_k(a, b, PR::SUB2P, 2, L30, L29, frac(19, 10), false, "sub2p_lazy");
  }
  // a - b + 8p: b normalized < 7.99p, limbs(a) < 2^31
  static bfl sub8p(const bfl& a, const bfl& b) { return sub_k(a, b, PR::SUB8P, 8, L31, L29, frac(799, 100), true, "sub8p"); }
  static bfl sub8p_lazy(const bfl& a, const bfl& b) {
    return sub_k(a, b, PR::SUB8P, 8, L30, L29, frac(799, 100), false, "sub8p_lazy");
  }
  static bfl sub_from_lazy(const bfl& a, const bfl& b) {
    return sub_k(a, b, PR::SUB16P, 16, L31, L30, frac(159, 10), true, "sub_from_lazy");
  }
  static bfl neg_lazy(const bfl& b) { return sub_k(zero(), b, PR::SUB16P, 16, 0, L29, frac(159, 10), false, "neg_lazy"); }
  static bfl neg2p_lazy(const bfl& b) { return sub_k(zero(), b, PR::SUB2P, 2, 0, L29, frac(19, 10), false, "neg2p_lazy"); }
  static bfl neg4p_lazy(const bfl& b) { return sub_k(zero(), b, PR::SUB4P, 4, 0, L29, frac(39, 10), false, "neg4p_lazy"); }
  // normalized -> normalized, < (1 + 2^-10) p (field29.hpp: the quotient estimate falls short of x / p by less than
  // 1 + 2^-11 + 2^-21) and never larger than before
  static constexpr uint64_t WEAK = U + U / 1024;
  // Takes a normalized value or one lazy sum of two (limbs < 2^30: k_perm_numden doubles un-carried): the limb
  // differences are carried in signed 64-bit words, and a top limb that lacks one carry costs the estimate 2^-21 more.
  static bfl weak_reduce(const bfl& x) {
    CAP_BOUND_REQUIRE(lim(x) <= L30 && x.mag <= C261, "weak_reduce");
    if (x.zero) return x;
    return norm_of(x.mag < WEAK ? x.mag : WEAK);
  }
  static bfl canonical(const bfl& x) {
    CAP_BOUND_REQUIRE(normalized(x), "canonical");
    if (x.zero) return x;
    return norm_of(x.mag < U ? x.mag : U);
  }
  // The 64-bit columns of a sum of products (reduce_cols): column k holds at most 9 products per pair of operands, then
  // the reduction adds 9 products m_i p_j < 2^58 and a carry < 2^36: the sum must stay below 2^64.
  static bool columns_fit(u128 products) {
    return products + 9 * ((u128)L29 * L29) + ((u128)1 << 36) < ((u128)1 << 64);
  }
  static uint64_t lim(const bfl& a) { return a.lo > a.hi ? a.lo : a.hi; }
  // Montgomery product: limbs < 2^30 on both sides, or one operand un-carried below 2^31 (neg_lazy) against a
  // normalized one; < a b / 2^261 + p, normalized (so below 2^261)
  static bfl mul(const bfl& a, const bfl& b) {
    CAP_BOUND_REQUIRE((lim(a) <= L30 && lim(b) <= L30) || (lim(a) <= L31 && lim(b) <= L29) ||
                          (lim(a) <= L29 && lim(b) <= L31), "mul");
    CAP_BOUND_REQUIRE(columns_fit(9 * ((u128)lim(a) * lim(b))), "mul");
    const uint64_t m = mont(a.mag, b.mag) + U;
    CAP_BOUND_REQUIRE(m <= C261, "mul");
    return norm_of(m, a.zero || b.zero);
  }
  static bfl sqr(const bfl& a) {
    CAP_BOUND_REQUIRE(lim(a) <= L30, "sqr");
    return mul(a, a);
  }
  // a b + c d with one reduction: every operand a normalized value or one lazy sum / difference (limbs < 2^31), and
  // the two products of every column together within the column limit - all four normalized do, and so does a
  // normalized a against b < 1.5 * 2^30 next to c < 2^30 against a normalized d (G1Law::madd_acc)
  static bfl mul_add_mul(const bfl& a, const bfl& b, const bfl& c, const bfl& d) {
    CAP_BOUND_REQUIRE(lim(a) <= L31 && lim(b) <= L31 && lim(c) <= L31 && lim(d) <= L31, "mul_add_mul");
    CAP_BOUND_REQUIRE(columns_fit(9 * ((u128)lim(a) * lim(b) + (u128)lim(c) * lim(d))), "mul_add_mul");
    const uint64_t m = mont(a.mag, b.mag) + mont(c.mag, d.mag) + U;
    CAP_BOUND_REQUIRE(m <= C261, "mul_add_mul");
    return norm_of(m, (a.zero || b.zero) && (c.zero || d.zero));
  }
  // constant-multiplicand product: limbs(a) < 2^30, a < 2^262; w canonical, wq normalized.  < 4p for a < 2^261, < 5p
  // beyond; zero for a = 0 (q = 0, and nothing is added)
  static bfl mul_shoup(const bfl& a, const bfl& w, const bfl& wq) {
    CAP_BOUND_REQUIRE(lim(a) <= L30, "mul_shoup");
    CAP_BOUND_REQUIRE(a.mag <= C262, "mul_shoup");
    CAP_BOUND_REQUIRE(normalized(w) && w.mag <= U, "mul_shoup");
    CAP_BOUND_REQUIRE(normalized(wq), "mul_shoup");
    return norm_of(a.mag <= C261 ? 4 * U : 5 * U, a.zero);
  }
  // x == 0 (mod p)?  x normalized (the test multiplies limb 0 and then reduces a normalized value)
  static bool is_zero(const bfl& x) {
    CAP_BOUND_REQUIRE(normalized(x) && x.mag <= C261, "is_zero");
    if (x.zero) return true;
    const int n = BoundBranch::taken()++;
    return n < 32 && ((BoundBranch::plan() >> n) & 1u);
  }
  static bool eq(const bfl& a, const bfl& b) { return is_zero(sub(a, weak_reduce(b))); }
  static bfl join(const bfl& a, const bfl& b) {  // the class that holds both
    bfl r;
    r.lo = a.lo > b.lo ? a.lo : b.lo;
    r.hi = a.hi > b.hi ? a.hi : b.hi;
    r.mag = a.mag > b.mag ? a.mag : b.mag;
    r.zero = a.zero && b.zero;
    // below 2^256 on both sides - an untouched image, a zero, or mag <= C256 - is below 2^256 whichever it is
    r.image = (a.image || a.zero || a.mag <= C256) && (b.image || b.zero || b.mag <= C256) && r.mag > C256;
    return r;
  }
  // a^(p-2) by 4-bit windows: the table a^1 .. a^15, then r = r^16 * tab[d] per window - run to the fixed point of
  // the class, every product checked; a product, so < p + r tab / 169
  static bfl inv(const bfl& a) {
    bfl tab = join(one(), a), t = a;
    for (int i = 2; i < 16; i++) {
      t = mul(t, a);
      tab = join(tab, t);
    }
    bfl r = tab;
    for (int it = 0; it < 64; it++) {
      const bfl s4 = sqr(sqr(sqr(sqr(r))));
      const bfl n = join(join(r, s4), mul(s4, tab));
      if (n.lo == r.lo && n.hi == r.hi && n.mag == r.mag) break;
      r = n;
    }
    r.zero = a.zero;
    return r;
  }
  static bfl from_ext(const bfe& a) { return mul(unpack(a), konst(PR::K266)); }
  static bfe to_ext(const bfl& a) { return pack(canonical(mul(a, konst(PR::C256)))); }
  static bfe store(const bfl& a) { return pack(weak_reduce(a)); }

  // a table constant of the butterflies and an image of a class
  static bfl twiddle() { return norm_of(U); }           // canonical
  static bfl quotient() { return norm_of(C261); }       // floor(w 2^261 / p): any normalized value
  static bfe image(uint64_t mag) {
    bfe r;
    r.mag = mag;
    r.zero = false;
    return r;
  }
  static bfe image_256() { return image(C256 + 1); }    // any 32 bytes: (2^256 - 1) 2^20 / p, rounded up
};

}  // namespace capbound

// ColAcc (round_elem29.hpp) on the bound field: the sum over the mads of the largest limb product, times the 9 limb
// products a column takes per mad, must leave room for the reduction (columns_fit: reduce_cols' column limit) - six
// products of normalized operands do, a seventh does not; the result is below sum a b / 2^261 + p, normalized.
namespace cap {
template <class PR>
struct ColAcc<capbound::BoundFl<PR>, capbound::bfl> {
  using BF = capbound::BoundFl<PR>;
  unsigned __int128 products;
  uint64_t mag, mads;
  bool all_zero;
  void clear() {
    products = 0;
    mag = mads = 0;
    all_zero = true;
  }
  void mad(const capbound::bfl& a, const capbound::bfl& b) {
    products += 9 * ((unsigned __int128)BF::lim(a) * BF::lim(b));
    mag += BF::mont(a.mag, b.mag);
    mads++;
    all_zero = all_zero && (a.zero || b.zero);
  }
  capbound::bfl reduce() {
    CAP_BOUND_REQUIRE(BF::columns_fit(products), "ColAcc::reduce");
    CAP_BOUND_REQUIRE(mag + BF::U <= BF::C261, "ColAcc::reduce");
    return BF::norm_of(mag + BF::U, all_zero);
  }
};
}  // namespace cap
