// medmoe_set_option and the count of order-dependent launches: the two pieces of process-wide state that belong to no kernel family.
#include "options.h"

// keys, ranges and meanings: the table in options.h
extern "C" int medmoe_set_option(int key, int value) {
  if (key == 1) { g_use_nt256 = value; return MM_OK; }
  if (key == 2) { g_use_nt512 = value; return MM_OK; }
  if (key == 3) { g_use_tn512 = value; return MM_OK; }
  if (key == 4 && value >= 256) { g_tn_rows = value; return MM_OK; }
  if (key == 5 && value >= 1 && value <= 256) { g_nt_max_grid = value; return MM_OK; }
  if (key == 6) { g_use_scores512 = value; return MM_OK; }
  if (key == 7) { g_use_nt4w = value; return MM_OK; }
  if (key == 8) { g_use_tn4w = value; return MM_OK; }
  if (key == 9 && value >= 64) { g_tn_min_rows = value; return MM_OK; }
  if (key == 10 && value >= 0) { g_tn_rows4w = value; return MM_OK; }
  if (key == 11) { g_attn_resident = value; return MM_OK; }
  if (key == 12) { g_scores_skip_epi = value; return MM_OK; }
  if (key == 13 && value >= 0) { g_sa_rows = value; return MM_OK; }
  if (key == 15 && (value == 0 || value == 448 || value == 512)) { g_attn_rt13 = value; return MM_OK; }
  if (key == 16) { g_ln_one_row = value; return MM_OK; }
  if (key == 17) { g_use_nt_direct = value; return MM_OK; }
  return MM_ERR_ARG;
}

// launches so far that took an order-dependent form (an atomic epilogue with more than one writer per element, an atomic loss sum):
// a host-side count, one add per such launch in the extern "C" dispatch functions of gemm / moe / norm / loss / optim / embed.hip -
// deterministic mode must leave it where it is.  Library-internal (hidden); the ABI is medmoe_nondet_launches().
MM_HIDDEN long long g_mm_nondet = 0;
extern "C" long long medmoe_nondet_launches() { return g_mm_nondet; }
