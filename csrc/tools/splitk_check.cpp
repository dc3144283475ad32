// Stand-alone sweep of csrc/splitk.h, meant for a sanitizer build on the CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Icsrc csrc/tools/splitk_check.cpp -o splitk_check
//   ./splitk_check
// For units and wgs_per_split in 1..512, round_to in {1, 2, 4} and target_wgs
// in {384, 1024} it checks what the GEMM kernels and their combine kernel
// rely on. Exits non-zero if any case fails.
#include <cstdio>
#include <initializer_list>

#include "splitk.h"

namespace {

int failures = 0;

#define EXPECT(cond)                                                       \
  do {                                                                     \
    if (!(cond)) {                                                         \
      if (++failures <= 20)                                                \
        std::printf("FAIL %s:%d: %s (units=%d wgs=%d target=%d round=%d " \
                    "splits=%d)\n",                                        \
                    __FILE__, __LINE__, #cond, units, wgs, target, round,  \
                    splits);                                               \
    }                                                                      \
  } while (0)

int cdiv(int a, int b) { return (a + b - 1) / b; }

void check(int units, int wgs, int target, int round) {
  const int splits = ps_splitk_depth(units, wgs, target, round);
  EXPECT(1 <= splits && splits <= units);
  if (splits < 1) return;

  // the kernels' partition: every split owns at least one unit
  const int per_split = cdiv(units, splits);
  for (int s = 0; s < splits; ++s) {
    const int begin = s * per_split;
    const int end = begin + per_split < units ? begin + per_split : units;
    EXPECT(begin < end);
  }
  // a fixed point of that partition
  EXPECT(cdiv(units, per_split) == splits);

  // Rounding. With want = clamp(target / wgs, 1, units), the range aimed for
  // is per0 = ceil(units / want), rounded up to round_to when want > 1. The
  // fixed point never asks for more splits than `want` and never makes a
  // range longer than per0, so a split runs at most per0 / round_to loop
  // iterations. per_split itself is a whole number of iterations only where
  // the fixed-point step left per0 alone; where it did not, it shortened it.
  int want = target / wgs;
  if (want < 1) want = 1;
  if (want > units) want = units;
  int per0 = cdiv(units, want);
  if (want > 1) per0 = cdiv(per0, round) * round;
  EXPECT(splits <= want);
  EXPECT(per_split <= per0);
  if (splits > 1 && per_split % round != 0) EXPECT(per_split < per0);
  // no rounding: one step from `want` already is the fixed point
  if (round == 1) EXPECT(splits == cdiv(units, cdiv(units, want)));
}

}  // namespace

int main() {
  long cases = 0;
  for (int target : {384, 1024})
    for (int round : {1, 2, 4})
      for (int units = 1; units <= 512; ++units)
        for (int wgs = 1; wgs <= 512; ++wgs, ++cases)
          check(units, wgs, target, round);
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("splitk_check: all %ld cases passed\n", cases);
  return 0;
}
