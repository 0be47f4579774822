// Host-side check of cap_amd/csrc/proof_codec.hpp: the CAP_HD decode and encode rule k_proof_decode / k_proof_encode run
// one lane per field, run here field by field against an independent reader made of params.hpp's g1_decompress_host and
// the bound on Fr - the pieces capgpu_proof_deserialize is made of - and an independent writer made of host_util.hpp's
// serialize_g1 / serialize_fr, the pieces of capgpu_proof_serialize.  Records are placed at byte offsets 0..7 of a buffer
// of exactly the bytes they span, with strides 769 and 776, so that a read past a record or a wide read at an odd address
// is seen by the sanitizers.  Prints bad=0.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../cap_amd/csrc/params.hpp"
#include "../../cap_amd/csrc/proof_codec.hpp"

using namespace cap;

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint64_t rnd64() {
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static int bad = 0;
#define CHECK(cond, ...)                  \
  do {                                    \
    if (!(cond)) {                        \
      bad++;                              \
      if (bad < 20) printf(__VA_ARGS__);  \
    }                                     \
  } while (0)

// ---- the reference: the record's fields in capgpu_proof_deserialize's order ----------------------------------------------
struct Field {
  uint32_t off;
  int kind;  // 0: length prefix, 1: point, 2: scalar, 3: tag
  uint32_t at;  // byte offset in capgpu_proof (points, scalars) or the expected length
};
static std::vector<Field> fields() {
  std::vector<Field> f;
  uint32_t off = 0, pt = 0, sc = 13 * 64;
  auto head = [&](uint32_t n) { f.push_back({off, 0, n}); off += 8; };
  auto point = [&]() { f.push_back({off, 1, pt}); off += 32; pt += 64; };
  auto scalar = [&]() { f.push_back({off, 2, sc}); off += 32; sc += 32; };
  head(5);
  for (int i = 0; i < 5; i++) point();
  point();
  head(5);
  for (int i = 0; i < 5; i++) point();
  point();
  point();
  head(5);
  for (int i = 0; i < 5; i++) scalar();
  head(4);
  for (int i = 0; i < 4; i++) scalar();
  scalar();
  f.push_back({off, 3, 0});
  return f;
}
static const std::vector<Field> kFields = fields();

// status and struct as the rule states them, through g1_decompress_host and cmp_words
static uint32_t ref_decode(const uint8_t* rec, capgpu_proof* out) {
  uint8_t* o = (uint8_t*)out;
  memset(o, 0, sizeof *out);
  for (const Field& f : kFields) {
    uint8_t b[32];
    bool ok = true;
    if (f.kind == 0) {
      uint64_t v;
      memcpy(&v, rec + f.off, 8);
      ok = v == f.at;
    } else if (f.kind == 1) {
      memcpy(b, rec + f.off, 32);
      g1_affine p;
      ok = params::g1_decompress_host(b, &p);
      memcpy(o + f.at, &p, 64);
    } else if (f.kind == 2) {
      fe v;
      memcpy(v.v, rec + f.off, 32);
      ok = params::cmp_words(v, params::fr_modulus()) < 0;
      const fe m = Fr::to_mont(v);
      memcpy(o + f.at, &m, 32);
    } else {
      ok = rec[f.off] == 0;
    }
    if (!ok) {
      memset(o, 0xFF, sizeof *out);
      return 1 + f.off;
    }
  }
  return 0;
}
static void ref_encode(const capgpu_proof& in, uint8_t* rec) {
  const uint8_t* s = (const uint8_t*)&in;
  for (const Field& f : kFields) {
    if (f.kind == 0) {
      const uint64_t v = f.at;
      memcpy(rec + f.off, &v, 8);
    } else if (f.kind == 1) {
      g1_affine p;
      memcpy(&p, s + f.at, 64);
      serialize_g1(p, rec + f.off);
    } else if (f.kind == 2) {
      fe v;
      memcpy(&v, s + f.at, 32);
      serialize_fr(v, rec + f.off);
    } else {
      rec[f.off] = 0;
    }
  }
}

// 32 bytes that decode: a random x on the curve with a random sign flag, or (one time in eight) infinity
static void rnd_point_bytes(uint8_t b[32]) {
  if ((rnd64() & 7) == 0) {
    memset(b, 0, 32);
    b[31] = 0x40;
    return;
  }
  for (;;) {
    fe x;
    for (int i = 0; i < 8; i++) x.v[i] = (uint32_t)rnd64();
    x.v[7] &= 0x1fffffffu;  // < 2^253 < p
    if (rnd64() & 1) x.v[7] |= 0x80000000u;
    memcpy(b, x.v, 32);
    g1_affine p;
    if (params::g1_decompress_host(b, &p)) return;
  }
}
static void rnd_scalar_bytes(uint8_t b[32]) {
  fe v;
  for (int i = 0; i < 8; i++) v.v[i] = (uint32_t)rnd64();
  v.v[7] &= 0x1fffffffu;
  memcpy(b, v.v, 32);
}
static std::vector<uint8_t> rnd_record() {
  std::vector<uint8_t> r(pc::kBytes);
  for (const Field& f : kFields) {
    if (f.kind == 0) {
      const uint64_t v = f.at;
      memcpy(&r[f.off], &v, 8);
    } else if (f.kind == 1) {
      rnd_point_bytes(&r[f.off]);
    } else if (f.kind == 2) {
      rnd_scalar_bytes(&r[f.off]);
    } else {
      r[f.off] = 0;
    }
  }
  return r;
}
static bool all_ones(const capgpu_proof& p) {
  const uint64_t* w = (const uint64_t*)&p;
  for (size_t i = 0; i < sizeof p / 8; i++)
    if (w[i] != ~0ull) return false;
  return true;
}
// pc::decode_record on `rec` against the reference: status, then the struct field by field
static uint32_t compare(const uint8_t* rec, const pc::SqrtExp& e, const char* what) {
  capgpu_proof got, want;
  memset(&got, 0x5A, sizeof got);
  const uint32_t st = pc::decode_record(rec, e, &got), want_st = ref_decode(rec, &want);
  CHECK(st == want_st, "%s: status %u, the reader's %u\n", what, st, want_st);
  for (const Field& f : kFields)
    if (f.kind == 1 || f.kind == 2)
      CHECK(!memcmp((const uint8_t*)&got + f.at, (const uint8_t*)&want + f.at, f.kind == 1 ? 64 : 32),
            "%s: the field at byte %u differs from the reader's\n", what, f.off);
  if (st) CHECK(all_ones(got), "%s: a refused record must decode to all-ones words\n", what);
  return st;
}

int main() {
  const pc::SqrtExp e = pc::sqrt_exponent();
  {
    uint32_t want[8];
    params::fq_sqrt_exponent(want);
    CHECK(!memcmp(want, e.w, 32), "the square-root exponent differs from params.hpp's\n");
  }
  // the layout functions against the reader's walk
  {
    uint32_t np = 0, ns = 0, nh = 0;
    for (const Field& f : kFields) {
      if (f.kind == 0) {
        CHECK(pc::head_offset(nh) == f.off && pc::head_value(nh) == f.at, "length prefix %u\n", nh);
        nh++;
      } else if (f.kind == 1) {
        CHECK(pc::point_offset(np) == f.off && 64 * np == f.at, "point %u\n", np);
        np++;
      } else if (f.kind == 2) {
        CHECK(pc::scalar_offset(ns) == f.off && td::kPrWireEvals + 32 * ns == f.at, "scalar %u\n", ns);
        ns++;
      }
      if (f.kind == 3) CHECK(pc::kTagOffset == f.off && f.off + 1 == pc::kBytes, "tag\n");
    }
    CHECK(np == pc::kPoints && ns == pc::kScalars && nh == pc::kHeads, "field counts\n");
  }
  // ---- valid records at every byte offset, two strides: decode equals the reader, encode gives the bytes back ----
  std::vector<std::vector<uint8_t>> recs;
  for (int i = 0; i < 3; i++) recs.push_back(rnd_record());
  for (size_t stride : {(size_t)769, (size_t)776})
    for (size_t off = 0; off < 8; off++) {
      std::vector<uint8_t> buf(off + (recs.size() - 1) * stride + pc::kBytes, 0xA5);
      for (size_t i = 0; i < recs.size(); i++) memcpy(&buf[off + i * stride], recs[i].data(), pc::kBytes);
      for (size_t i = 0; i < recs.size(); i++) {
        const uint8_t* rec = &buf[off + i * stride];
        CHECK(compare(rec, e, "valid record") == 0, "a valid record was refused (offset %zu stride %zu)\n", off, stride);
        capgpu_proof pr, back;
        (void)pc::decode_record(rec, e, &pr);
        // encode: the inverse, and the host writer's bytes, written at the same odd address into an exact buffer
        std::vector<uint8_t> out(off + pc::kBytes, 0xA5), ref(pc::kBytes);
        pc::encode_record(pr, &out[off]);
        ref_encode(pr, ref.data());
        CHECK(!memcmp(&out[off], rec, pc::kBytes), "encode(decode(record)) != record\n");
        CHECK(!memcmp(&out[off], ref.data(), pc::kBytes), "encode differs from serialize_g1 / serialize_fr\n");
        for (size_t k = 0; k < off; k++) CHECK(out[k] == 0xA5, "encode wrote in front of its record\n");
        CHECK(pc::decode_record(&out[off], e, &back) == 0 && !memcmp(&back, &pr, sizeof pr), "decode(encode(struct)) != struct\n");
      }
    }
  // ---- the corruption table: one field at a time, the status names its offset ----
  const std::vector<uint8_t> good = recs[0];
  auto expect = [&](const std::vector<uint8_t>& rec, uint32_t off, const char* what) {
    const uint32_t st = compare(rec.data(), e, what);
    CHECK(st == 1 + off, "%s at byte %u: status %u\n", what, off, st);
  };
  fe p = Fq::modulus(), r = Fr::modulus(), four = Fq::zero();
  four.v[0] = 4;
  for (const Field& f : kFields) {
    std::vector<uint8_t> rec = good;
    if (f.kind == 0) {
      rec[f.off] = (uint8_t)(f.at == 5 ? 4 : 5);
      expect(rec, f.off, "wrong length prefix");
      rec = good;
      rec[f.off + 7] = 1;  // a length no input could hold
      expect(rec, f.off, "huge length prefix");
    } else if (f.kind == 1) {
      rec[f.off + 31] |= 0xC0;
      expect(rec, f.off, "both flags");
      rec = good;
      rec[f.off + 31] = (uint8_t)((rec[f.off + 31] & 0x3F) | 0x40);
      if (!(rec[f.off] | rec[f.off + 1])) rec[f.off] = 1;
      expect(rec, f.off, "infinity flag with x != 0");
      rec = good;
      memcpy(&rec[f.off], p.v, 32);
      expect(rec, f.off, "x = p");
      rec = good;
      memcpy(&rec[f.off], four.v, 32);
      expect(rec, f.off, "x = 4 (off the curve)");
    } else if (f.kind == 2) {
      memcpy(&rec[f.off], r.v, 32);
      expect(rec, f.off, "scalar = r");
      rec = good;
      memset(&rec[f.off], 0xFF, 32);
      expect(rec, f.off, "scalar = 2^256 - 1");
    } else {
      rec[f.off] = 1;
      expect(rec, f.off, "tag 1");
      rec[f.off] = 2;
      expect(rec, f.off, "tag 2");
    }
  }
  // two corruptions: the lower offset is named, whatever the kinds
  {
    std::vector<uint8_t> rec = good;
    memcpy(&rec[pc::scalar_offset(7)], r.v, 32);
    rec[pc::point_offset(9) + 31] |= 0xC0;
    expect(rec, pc::point_offset(9), "point 9 and scalar 7");
    rec[pc::head_offset(1)] = 4;
    expect(rec, pc::head_offset(1), "prefix 1, point 9 and scalar 7");
    rec = good;
    rec[pc::kTagOffset] = 1;
    memcpy(&rec[pc::scalar_offset(9)], r.v, 32);
    expect(rec, pc::scalar_offset(9), "scalar 9 and the tag");
  }
  // ---- records that decode although a verifier must refuse them ----
  {
    std::vector<uint8_t> rec = good;
    uint32_t k = 0;
    while (rec[pc::point_offset(k) + 31] & 0x40) k++;  // a point that is not infinity
    rec[pc::point_offset(k) + 31] ^= 0x80;
    capgpu_proof a, b;
    CHECK(compare(rec.data(), e, "sign flipped") == 0, "a flipped sign still decodes\n");
    (void)pc::decode_record(good.data(), e, &a);
    (void)pc::decode_record(rec.data(), e, &b);
    const uint8_t *pa = (const uint8_t*)&a + 64 * k, *pb = (const uint8_t*)&b + 64 * k;
    fe ya, yb;
    memcpy(&ya, pa + 32, 32);
    memcpy(&yb, pb + 32, 32);
    CHECK(!memcmp(pa, pb, 32) && Fq::eq(Fq::neg(ya), yb), "the flag picks the other root\n");
    rec = good;
    fe rm1 = r;
    rm1.v[0] -= 1;
    memcpy(&rec[pc::scalar_offset(3)], rm1.v, 32);
    CHECK(compare(rec.data(), e, "scalar r - 1") == 0, "r - 1 is canonical\n");
    rec = good;
    memset(&rec[pc::point_offset(2)], 0, 32);
    rec[pc::point_offset(2) + 31] = 0x40;
    CHECK(compare(rec.data(), e, "infinity") == 0, "the infinity encoding decodes\n");
    (void)pc::decode_record(rec.data(), e, &a);
    const uint64_t* w = (const uint64_t*)&a + 8 * 2;
    CHECK(!(w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]), "infinity decodes to (0, 0)\n");
  }
  printf("bad=%d\n", bad);
  return bad ? 1 : 0;
}
