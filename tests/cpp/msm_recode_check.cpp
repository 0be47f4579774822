// Host harness for msm_recode.hpp (tests/test_msm_var_host.py).  stdin: lines "c k" - window size, scalar as 64 hex
// digits; stdout: one line per input, "W d_0 d_1 ... d_(W-1)" - the window count and every signed digit (decimal).
#include "../../cap_amd/csrc/msm_recode.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>

int main() {
  char hex[128];
  unsigned c;
  while (scanf("%u %127s", &c, hex) == 2) {
    const size_t len = strlen(hex);
    if (c < 2 || c > 16 || len == 0 || len > 64) return 2;
    uint32_t k[8] = {0};
    for (size_t i = 0; i < len; i++) {
      const char ch = hex[len - 1 - i];
      const uint32_t v = ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10;
      k[i / 8] |= v << (4 * (i % 8));
    }
    const cap::msm_biased kb = cap::msm_recode_add(k, cap::msm_recode_bias(c));
    const uint32_t W = cap::msm_recode_windows(c);
    printf("%u", W);
    for (uint32_t w = 0; w < W; w++) printf(" %d", cap::msm_recode_digit(kb, w, c));
    printf("\n");
  }
  return 0;
}
