// Host-side check of cap_amd/csrc/gatecheck29.hpp (the gate constraint and the permutation's index form of the witness
// check) with field29.hpp's bound assertions enabled.  Reads one operation per line on stdin, plain hex integers below
// 2^256, prints the result; tests/test_check_witness_host.py compares with oracle/plonk.py.
//   G q0 .. q12 w0 .. w4 pi     the gate's value (canonical, plain) and 1 if it holds else 0
//   H q0 .. q12 w0 .. w4 pi     the same with every operand in a non-canonical representation (its value + r)
//   I log_n kinv0 .. kinv4 winv_0 .. winv_(log_n-1) count v_1 .. v_count     perm_index of every v (ffffffff: none)
//   E a b                       1 if the two 32-byte values are equal mod r else 0
#define CAP_FL_CHECK 1
#include "../../cap_amd/csrc/gatecheck29.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace cap;
using C = wc29::Check<CAP_FL_SCHED>;
using F = C::F;

static fe read_fe() {
  char s[160];
  if (scanf(" %159s", s) != 1) exit(2);
  fe r;
  memset(&r, 0, sizeof r);
  const int n = (int)strlen(s);
  for (int i = 0; i < n; i++) {
    const int d = n - 1 - i;  // nibble index from the low end
    char c = s[i];
    uint32_t v = c <= '9' ? c - '0' : (c | 32) - 'a' + 10;
    r.v[d / 8] |= v << (4 * (d % 8));
  }
  return r;
}
static void print_fe(const fe& a) {
  for (int i = 7; i >= 0; i--) printf("%08x", a.v[i]);
}
static fl read_operand(bool lazy) {
  fl x = F::to_mont(read_fe());
  if (lazy) x = F::add_norm(F::canonical(x), F::konst(FrP29::MOD));
  return x;
}

int main() {
  char op;
  while (scanf(" %c", &op) == 1) {
    switch (op) {
      case 'G':
      case 'H': {
        fl q[wc29::kSelectors], w[wc29::kWires];
        for (auto& x : q) x = read_operand(op == 'H');
        for (auto& x : w) x = read_operand(op == 'H');
        const fl pi = read_operand(op == 'H');
        auto sel = [&](int s) { return q[s]; };
        print_fe(F::from_mont(C::gate(sel, w, pi)));
        printf(" %d\n", C::gate_holds(sel, w, pi) ? 1 : 0);
        break;
      }
      case 'I': {
        wc29::PermConsts pc;
        memset(&pc, 0, sizeof pc);
        int count = 0;
        if (scanf(" %u", &pc.log_n) != 1 || pc.log_n > 28) return 2;
        auto internal = [] { return F::pack(F::canonical(F::to_mont(read_fe()))); };
        for (auto& k : pc.kinv) k = internal();
        for (uint32_t b = 0; b < pc.log_n; b++) pc.winv[b] = internal();
        if (scanf(" %d", &count) != 1) return 2;
        for (int i = 0; i < count; i++) printf("%x ", C::perm_index(F::to_mont(read_fe()), pc));
        printf("\n");
        break;
      }
      case 'E': {
        const fe a = read_fe(), b = read_fe();
        printf("%d\n", C::same_value(a, b) ? 1 : 0);
        break;
      }
      default: return 3;
    }
    fflush(stdout);
  }
  return 0;
}
