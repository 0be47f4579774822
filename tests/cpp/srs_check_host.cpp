// Host-side check of cap_amd/csrc/srs_check.hpp: the CAP_HD point predicate k_srs_points runs one lane per resident base,
// run here on the host against the saturated arithmetic of field.hpp / curve.hpp.  A resident base is an image of
// x * 2^261 mod p below 2^256 ((0, 0) = infinity); the reference brings an image back to arkworks' form (x * 2^256) by its
// own reduction and one saturated product with 2^251, and tests y^2 == x^3 + 3 there.  Built with CAP_FL_CHECK: every
// bound the lazy field states is asserted on the inputs below.  Prints bad=0.
#define CAP_FL_CHECK
#include <cassert>
#include <cstdio>
#include <cstring>

#include "../../cap_amd/csrc/params.hpp"
#include "../../cap_amd/csrc/srs_check.hpp"

using namespace cap;

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd64() {
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static int bad = 0, cases = 0;
#define CHECK(cond, ...)                  \
  do {                                    \
    cases++;                              \
    if (!(cond)) {                        \
      bad++;                              \
      if (bad < 20) printf(__VA_ARGS__);  \
    }                                     \
  } while (0)

// ---- the reference: saturated field only ------------------------------------------------------------------------------
static fe reduce_image(fe v) {  // any value below 2^256 -> below p
  while (Fq::geq_mod(v)) {
    fe t;
    (void)Fq::sub_mod_raw(t, v);
    v = t;
  }
  return v;
}
static fe image_to_ext(const fe& img) {  // x 2^261 -> x 2^256: Montgomery product with the plain integer 2^251
  fe k = Fq::zero();
  k.v[7] = 1u << 27;
  return Fq::mul(reduce_image(img), k);
}
static uint32_t ref_fault(const g1_affine& img) {
  bool zero = true;
  for (int i = 0; i < 8; i++) zero = zero && img.x.v[i] == 0 && img.y.v[i] == 0;
  if (zero) return sc::kFaultInfinity;
  const fe x = image_to_ext(img.x), y = image_to_ext(img.y);
  const fe b3 = Fq::add(Fq::dbl(Fq::one()), Fq::one());
  return Fq::eq(Fq::sqr(y), Fq::add(Fq::mul(Fq::sqr(x), x), b3)) ? sc::kFaultNone : sc::kFaultOffCurve;
}

// ---- inputs -------------------------------------------------------------------------------------------------------------
// arkworks form -> the table's image, as msm_precompute_kernel stores window 0 (canonical)
static g1_affine to_image(const g1_affine& a) {
  g1_affine r;
  r.x = Fq29::pack(Fq29::canonical(Fq29::from_ext(a.x)));
  r.y = Fq29::pack(Fq29::canonical(Fq29::from_ext(a.y)));
  return r;
}
static g1_affine generator() {
  g1_affine g;
  g.x = Fq::one();
  g.y = Fq::dbl(Fq::one());
  return g;
}
static g1_affine rnd_point() {
  for (;;) {
    uint8_t b[32];
    for (int i = 0; i < 4; i++) {
      const uint64_t w = rnd64();
      memcpy(b + 8 * i, &w, 8);
    }
    b[31] &= 0x1f;                       // x below 2^253
    if (rnd64() & 1) b[31] |= 0x80;      // either root
    g1_affine p;
    if (params::g1_decompress_host(b, &p) && !G1::is_inf(p)) return p;
  }
}
// v + k p while it stays below 2^256: the other images of the same residue
static bool add_p(fe* v) {
  fe t;
  if (Fq::add_raw(t, *v, Fq::modulus())) return false;
  *v = t;
  return true;
}
static void expect(const g1_affine& img, uint32_t want, const char* what, int i) {
  const uint32_t ref = ref_fault(img), got = sc::point_fault(img);
  CHECK(ref == want, "%s %d: the reference says %u, the case was built for %u\n", what, i, ref, want);
  CHECK(got == ref, "%s %d: predicate %u, reference %u\n", what, i, got, ref);
}

int main() {
  expect(to_image(generator()), sc::kFaultNone, "generator", 0);
  g1_affine zero;
  memset(&zero, 0, sizeof zero);
  expect(zero, sc::kFaultInfinity, "(0,0)", 0);
  fe one_word = Fq::zero();
  one_word.v[0] = 1;
  for (int i = 0; i < 200; i++) {
    const g1_affine a = rnd_point(), img = to_image(a);
    expect(img, sc::kFaultNone, "curve point", i);
    // (x, -y) is the other point over x
    expect(to_image(G1::neg(a)), sc::kFaultNone, "(x,-y)", i);
    // (x, y + 1): in arkworks' words, as a caller edits a downloaded point, and in the image itself
    g1_affine t = a;
    t.y = Fq::add(a.y, one_word);
    expect(to_image(t), sc::kFaultOffCurve, "(x,y+1) words", i);
    t = img;
    (void)Fq::add_raw(t.y, img.y, one_word);
    expect(t, sc::kFaultOffCurve, "(x,y+1) image", i);
    t = img;
    (void)Fq::add_raw(t.x, img.x, one_word);
    expect(t, sc::kFaultOffCurve, "(x+1,y) image", i);
    // swapped coordinates
    t.x = img.y;
    t.y = img.x;
    expect(t, sc::kFaultOffCurve, "(y,x)", i);
    // one coordinate's image all zero words, or 1, or p - 1 (the neighbours of y = 0, which no point of the curve has):
    // not infinity, and not on the curve
    for (int which = 0; which < 2; which++)
      for (int v = 0; v < 3; v++) {
        fe c = Fq::zero();
        if (v == 1) c = one_word;
        if (v == 2) (void)Fq::sub_raw(c, Fq::modulus(), one_word);
        t = img;
        (which ? t.y : t.x) = c;
        expect(t, ref_fault(t), "zero-adjacent coordinate", 6 * i + 3 * which + v);
        CHECK(sc::point_fault(t) != sc::kFaultInfinity, "zero-adjacent coordinate %d reported as infinity\n", i);
      }
    // every image of the same residues below 2^256 (x + k p): the same verdict, for a good and for a bad point
    g1_affine up = img, upbad = img;
    (void)Fq::add_raw(upbad.y, img.y, one_word);
    for (int k = 0; k < 6; k++) {
      const bool more_x = add_p(&up.x);
      const bool more_y = add_p(&up.y);
      expect(up, sc::kFaultNone, "image + k p", i);
      if (add_p(&upbad.y)) expect(upbad, sc::kFaultOffCurve, "bad image + k p", i);
      if (!more_x && !more_y) break;
    }
  }
  // the bounds of the memory format: all-ones words, 2^256 - 1 against small values, p itself (the residue 0)
  fe ones, p = Fq::modulus();
  for (int i = 0; i < 8; i++) ones.v[i] = 0xFFFFFFFFu;
  const fe vals[5] = {ones, p, one_word, Fq::zero(), to_image(generator()).y};
  for (int a = 0; a < 5; a++)
    for (int b = 0; b < 5; b++) {
      g1_affine t;
      t.x = vals[a];
      t.y = vals[b];
      expect(t, ref_fault(t), "format bounds", 5 * a + b);
    }
  // (p, p) is the residue pair (0, 0) but not the encoding of infinity: off the curve
  g1_affine pp;
  pp.x = p;
  pp.y = p;
  expect(pp, sc::kFaultOffCurve, "(p,p)", 0);
  printf("cases=%d bad=%d\n", cases, bad);
  return bad ? 1 : 0;
}
