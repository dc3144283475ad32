// Split-K depth shared by the GEMMs that reduce through an fp32 workspace
// ws[splits, M, N] (skinny_gemm*.hip, gemm8p.hip). Plain host C++ with no HIP
// include, so csrc/tools/splitk_check.cpp can sweep it on the CPU.
#pragma once

// How many K-ranges a GEMM is cut into. `units` is the K extent in the
// kernel's own unit (64-wide chunks, 128-wide groups or pairs, >= 1),
// `wgs_per_split` the workgroups one K-range launches (>= 1), `target_wgs`
// the grid size aimed for. With more than one split a range is rounded up to
// whole `round_to`-unit loop iterations.
//
// Every kernel partitions as per_split = ceil(units / splits), split s taking
// units [s * per_split, min(units, (s + 1) * per_split)), so for some counts
// the trailing splits come out empty. That is fatal: an empty split returns
// without writing its ws slice, and the combine kernel sums every slice. So
// the count is taken to the fixed point of that formula, which keeps exactly
// the non-empty splits. The result is in [1, units].
static inline int ps_splitk_depth(int units, int wgs_per_split, int target_wgs,
                                  int round_to) {
  int splits = target_wgs / wgs_per_split;
  if (splits < 1) splits = 1;
  if (splits > units) splits = units;
  int per_split = (units + splits - 1) / splits;
  if (splits > 1) per_split = (per_split + round_to - 1) / round_to * round_to;
  splits = (units + per_split - 1) / per_split;
  for (;;) {
    per_split = (units + splits - 1) / splits;
    const int s = (units + per_split - 1) / per_split;
    if (s == splits) return splits;
    splits = s;
  }
}
