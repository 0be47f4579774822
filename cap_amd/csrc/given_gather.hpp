// capgpu_plonk_prove_given_one / _io_one with coalescing on: the PACKING rule of a gathered part.  Host only, no HIP - like
// notes_plan.hpp, compact.hpp and coalescer.hpp; tests/cpp/given_gather_check.cpp runs every assignment of up to 8 requests
// to three keys through it, under the sanitizers too.
//
// A gathered part holds single-proof requests of one (domain size, SRS), all keys mixed, in ARRIVAL order.  Before the
// batch, a request that cannot run is SET ASIDE with its reason (its owner gets its own code and message, the others
// run); the rest get consecutive SLOTS in arrival order.  The part is then one given-value call with one key per proof
// (ProveCall, plonk.hip): rows of given values as long as the largest num_given among the part's keys, rows of public
// inputs as long as the largest num_inputs, a shorter row zero-filled behind its own values - the layout
// capgpu_plonk_prove_given asks of a call with several keys -, 13 blinders per slot.  After the batch every request takes
// what lies in its slot; the outcome is normalised on the way (below).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/capgpu.h"

namespace cap {
namespace gg {

constexpr size_t kWords = 4;      // 64-bit words of a field element
constexpr size_t kBlinders = 13;  // blinders of one proof
constexpr size_t kNone = ~(size_t)0;

// why a request does not ride with its part; tested in this order
enum Aside : int {
  kRuns = 0,
  kKeyGone,   // its handle names no key (freed since the call arrived, or never there)
  kNoSolver,  // its key has no solver (capgpu_plonk_key_set_given gives it one)
  kLengths,   // its num_given or num_inputs is not the key's
};

// one request: what its caller says and what its key says (the key's fields mean nothing when !key_found)
struct Ask {
  bool key_found = false, has_solver = false;
  size_t key_given = 0, key_inputs = 0;  // the key's num_given and num_inputs
  size_t num_given = 0, num_inputs = 0;  // the caller's
};

inline Aside set_aside(const Ask& a) {
  if (!a.key_found) return kKeyGone;
  if (!a.has_solver) return kNoSolver;
  if (a.num_given != a.key_given || a.num_inputs != a.key_inputs) return kLengths;
  return kRuns;
}

struct Plan {
  std::vector<Aside> why;       // [requests]
  std::vector<size_t> slot_of;  // [requests]: the request's slot, kNone when it was set aside
  std::vector<size_t> req_of;   // [slots]: the request in it - ascending: arrival order
  size_t given_stride = 0;      // elements per row of given values: the largest num_given among the keys of the slots
  size_t pub_stride = 0;        // elements per row of public inputs: the largest num_inputs among them
  size_t slots() const { return req_of.size(); }
  // where slot s lies in the packed arrays, in 64-bit words
  size_t given_at(size_t s) const { return kWords * given_stride * s; }
  size_t pub_at(size_t s) const { return kWords * pub_stride * s; }
  size_t blind_at(size_t s) const { return kWords * kBlinders * s; }
  // the arrays' lengths in words (never 0: an empty array still has an address)
  size_t given_words() const { return given_at(slots()) + kWords; }
  size_t pub_words() const { return pub_at(slots()) + kWords; }
  size_t blind_words() const { return blind_at(slots()) + kWords; }
};

inline Plan plan(const Ask* asks, size_t count) {
  Plan pl;
  pl.why.resize(count);
  pl.slot_of.assign(count, kNone);
  for (size_t i = 0; i < count; i++) {
    pl.why[i] = set_aside(asks[i]);
    if (pl.why[i] != kRuns) continue;
    pl.slot_of[i] = pl.req_of.size();
    pl.req_of.push_back(i);
    pl.given_stride = std::max(pl.given_stride, asks[i].key_given);
    pl.pub_stride = std::max(pl.pub_stride, asks[i].key_inputs);
  }
  return pl;
}

// `len` elements of `src` into a row of `stride` elements (len <= stride), zeros behind them; src may be NULL when len is 0
inline void pack_row(uint64_t* row, size_t stride, const uint64_t* src, size_t len) {
  if (len) memcpy(row, src, sizeof(uint64_t) * kWords * len);
  if (stride > len) memset(row + kWords * len, 0, sizeof(uint64_t) * kWords * (stride - len));
}
// the first `len` elements of a row back to their owner
inline void take_row(uint64_t* dst, const uint64_t* row, size_t len) {
  if (len) memcpy(dst, row, sizeof(uint64_t) * kWords * len);
}

// The one place where a gathered batch differs from a request's lone call: with the witness check on, a lone refused
// witness returns after the check and was never proved - degree_flags 0 -, while in an uncompacted batch it rides to the end
// and the degree check sets its flags as well.  The _one calls report the lone call's record: no flags beside a fault.
inline void normalise(capgpu_prove_outcome* o) {
  if (o->fault.kind != 0) o->degree_flags = 0;
}

}  // namespace gg
}  // namespace cap
