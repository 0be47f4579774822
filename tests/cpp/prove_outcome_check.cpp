// Host-side check of cap_amd/csrc/outcome.hpp, the one rule of capgpu_plonk_prove_each*: the status for every combination
// of degree flags {0,1,2,3} and fault kind {0,1,2}; blanking writes exactly sizeof(capgpu_proof) bytes of ones and nothing
// beyond (guard bytes either side, lane by lane as the device does it and in one go as the host does); the three wordings
// against literal strings, and cap 0 / 1 / exact length.  Built plain and under the sanitizers.  Prints bad=0.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../cap_amd/csrc/outcome.hpp"

using namespace cap;

static int bad = 0;
#define CHECK(cond, ...)                  \
  do {                                    \
    if (!(cond)) {                        \
      bad++;                              \
      if (bad < 20) printf(__VA_ARGS__);  \
    }                                     \
  } while (0)

static const char* kGate =
    "capgpu_plonk_prove: 1 of 1 witnesses do not satisfy their circuit; first: proof 0: gate 1234 not satisfied";
static const char* kCopy =
    "capgpu_plonk_prove: 1 of 1 witnesses do not satisfy their circuit; first: proof 0: copy constraint (2,40) -> (0,7) "
    "violated";
static const char* kDegree =
    "capgpu_plonk_prove: proof 0: quotient polynomial has the wrong degree (flags 3): the circuit is not satisfied by this "
    "witness";

static capgpu_prove_outcome outcome(uint32_t flags, uint32_t kind) {
  capgpu_prove_outcome o;
  memset(&o, 0, sizeof o);
  o.degree_flags = flags;
  o.fault.kind = kind;
  if (kind == 1) o.fault.row = 1234;
  if (kind == 2) {
    o.fault.wire = 2;
    o.fault.row = 40;
    o.fault.wire2 = 0;
    o.fault.row2 = 7;
  }
  o.status = oc::prove_status(flags, kind);
  return o;
}

static void check_text(const capgpu_prove_outcome& o, const char* want) {
  const size_t len = strlen(want);
  // ample room
  std::vector<char> big(len + 64, 'x');
  CHECK(oc::outcome_text(o, big.data(), big.size()) == (int)len && !strcmp(big.data(), want), "text: '%s'\n", big.data());
  // exactly the length + the NUL, in a buffer of exactly that size (a write past it is the sanitizer's to see)
  std::vector<char> exact(len + 1, 'x');
  oc::outcome_text(o, exact.data(), exact.size());
  CHECK(!memcmp(exact.data(), want, len + 1), "exact cap: '%s'\n", exact.data());
  // one short: truncated, terminated
  if (len) {
    std::vector<char> cut(len, 'x');
    oc::outcome_text(o, cut.data(), cut.size());
    CHECK(!memcmp(cut.data(), want, len - 1) && cut[len - 1] == 0, "cap = length: not truncated and terminated\n");
  }
  // cap 1: the NUL alone; cap 0: nothing, not even through a null pointer
  char one[2] = {'x', 'y'};
  oc::outcome_text(o, one, 1);
  CHECK(one[0] == 0 && one[1] == 'y', "cap 1 wrote '%c%c'\n", one[0], one[1]);
  char none[1] = {'z'};
  CHECK(oc::outcome_text(o, none, 0) == (int)len && none[0] == 'z', "cap 0 wrote\n");
  CHECK(oc::outcome_text(o, nullptr, 0) == (int)len, "cap 0 with a null buffer\n");
}

int main() {
  static_assert(sizeof(capgpu_prove_outcome) == 56 && offsetof(capgpu_prove_outcome, degree_flags) == 4 &&
                    offsetof(capgpu_prove_outcome, fault) == 8,
                "capgpu_prove_outcome layout");
  // status: CAPGPU_ERR_PROOF exactly when degree_flags != 0 || fault.kind != 0
  for (uint32_t flags = 0; flags < 4; flags++)
    for (uint32_t kind = 0; kind < 3; kind++) {
      const int32_t want = (flags != 0 || kind != 0) ? CAPGPU_ERR_PROOF : CAPGPU_OK;
      CHECK(oc::prove_status(flags, kind) == want, "status(%u, %u)\n", flags, kind);
      capgpu_witness_fault f;
      memset(&f, 0, sizeof f);
      f.kind = kind;
      f.row = 9;
      capgpu_prove_outcome o;
      memset(&o, 0xab, sizeof o);
      // a record between guard bytes, 8-byte aligned as a capgpu_proof is
      const size_t guard = 64;
      std::vector<uint64_t> store((2 * guard + sizeof(capgpu_proof)) / 8, 0x1111111111111111ull);
      uint8_t* base = (uint8_t*)store.data();
      capgpu_proof* rec = (capgpu_proof*)(base + guard);
      oc::finish_outcome(flags, kind ? &f : nullptr, &o, rec);
      CHECK(o.status == want && o.degree_flags == flags && o.fault.kind == kind && o.fault.row == (kind ? 9u : 0u) &&
                o.fault.reserved == 0,
            "finish_outcome(%u, %u)\n", flags, kind);
      bool guards = true, body = true;
      for (size_t i = 0; i < guard; i++) guards = guards && base[i] == 0x11 && base[guard + sizeof(capgpu_proof) + i] == 0x11;
      for (size_t i = 0; i < sizeof(capgpu_proof); i++) body = body && base[guard + i] == (want ? 0xff : 0x11);
      CHECK(guards && body, "blanking (%u, %u): guards %d body %d\n", flags, kind, (int)guards, (int)body);
    }
  // the device's way: 64 lanes, each its own words - together exactly the record
  {
    const size_t guard = 64;
    std::vector<uint64_t> store((2 * guard + sizeof(capgpu_proof)) / 8, 0x2222222222222222ull);
    uint8_t* base = (uint8_t*)store.data();
    for (uint32_t lane = 0; lane < 64; lane++) oc::blank_record(base + guard, lane, 64);
    bool ok = true;
    for (size_t i = 0; i < store.size() * 8; i++)
      ok = ok && base[i] == ((i >= guard && i < guard + sizeof(capgpu_proof)) ? 0xff : 0x22);
    CHECK(ok, "64 lanes do not blank exactly the record\n");
    CHECK(oc::kRecordWords * 8 == sizeof(capgpu_proof) && sizeof(capgpu_proof) == 1152, "record size\n");
  }
  // the wordings
  check_text(outcome(0, 1), kGate);
  check_text(outcome(3, 1), kGate);  // (a fault goes first: the check's wording in the mode the check ran in)
  check_text(outcome(0, 2), kCopy);
  check_text(outcome(3, 0), kDegree);
  check_text(outcome(0, 0), "");
  printf("bad=%d\n", bad);
  return bad != 0;
}
