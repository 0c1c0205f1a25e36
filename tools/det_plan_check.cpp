// Stand-alone host check of medmoe_amd/csrc/det_plan.h (no GPU, no HIP): for many shapes and random group sizes, walk the row ranges with
// the inline functions gemm_tn4w_kernel and tn_reduce_det_kernel themselves call and check that every partial-tile slot lies inside the
// planned scratch, that the summing kernel reads exactly the slots the GEMM stored, and that every row is covered exactly once.
//   make check-plan     (address + undefined-behaviour sanitizers, host compiler only)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "det_plan.h"

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (unsigned)(rng_state >> 11); }

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

int main() {
  long long cases = 0;
  const int dims[] = {128, 256, 384, 512, 768, 1024, 3072};
  for (int it = 0; it < 20000; ++it) {
    const int n_groups = 1 + rnd() % 16;
    const bool grouped = rnd() % 2, xm = rnd() % 3 == 0, gm = !xm && rnd() % 3 == 0;
    const int Nn = dims[rnd() % 7], Kk = dims[rnd() % 7];
    int M = 1 + rnd() % (rnd() % 4 == 0 ? 500000 : 40000);
    if (rnd() % 2) M = (M + 31) / 32 * 32;
    const int ng = grouped ? n_groups : 1;
    const det_plan::TnPlan pl = det_plan::tn_plan(M, Nn, Kk, xm, gm, grouped, ng, true, 2048, rnd() % 4 == 0 ? 32 * (1 + rnd() % 512) : 0);
    if (pl.kind == det_plan::TN_SMALL) { CHECK(pl.scratch_floats == 0); continue; }
    ++cases;
    const int ntile = pl.tiles_n * pl.tiles_k;
    CHECK(pl.tiles_n * 256 >= Nn && pl.tiles_k * 256 == Kk && pl.slots > 0);
    CHECK(pl.scratch_floats == (long long)pl.slots * (65536 + 512));
    std::vector<char> used(pl.slots, 0);
    std::vector<int> cover(M, 0);
    if (pl.kind == det_plan::TN_GROUPS) {
      std::vector<int> off(ng + 1, 0);                              // random group sizes, some empty
      std::vector<int> cut(ng - 1);
      for (int& c : cut) c = rnd() % 3 == 0 ? 0 : (int)(rnd() % (unsigned)(M + 1));
      for (int g = 1; g < ng; ++g) { int m = 0; for (int j = 0; j < g; ++j) m = cut[j] > m ? cut[j] : m; off[g] = m; }
      off[ng] = M;
      const int R = pl.nsplit;
      CHECK(R % 32 == 0 && pl.slots % ntile == 0);
      // the GEMM (gemm_tn4w_kernel<true>): workgroup id -> (range, tile) through det_plan::tn_group_range
      for (int id = 0; id < pl.slots; ++id) {
        int g = -1, ms = -1, me = -1;
        if (!det_plan::tn_group_range(off.data(), ng, R, id / ntile, g, ms, me)) continue;
        CHECK(g >= 0 && g < ng && off[g] <= ms && ms < me && me <= off[g + 1] && me - ms <= R);
        used[id] = 1;
        if (id % ntile == 0) for (int m = ms; m < me; ++m) ++cover[m];
      }
      // the summing kernel (tn_reduce_det_kernel, mode 1): a group's slots through det_plan::tn_group_ranges
      for (int g = 0; g < ng; ++g) {
        int first = 0, count = 0;
        det_plan::tn_group_ranges(off.data(), g, R, first, count);
        for (int sp = 0; sp < count; ++sp) {
          int g2 = -1, ms = -1, me = -1;                            // the range it sums is one the GEMM gave to this group
          CHECK(det_plan::tn_group_range(off.data(), ng, R, first + sp, g2, ms, me) && g2 == g);
          for (int t = 0; t < ntile; ++t) { const int s = (first + sp) * ntile + t; CHECK(s >= 0 && s < pl.slots && used[s] == 1); used[s] = 2; }
        }
      }
      for (char u : used) CHECK(u != 1);                            // every stored tile is summed, none twice
    } else {
      CHECK(pl.slots == ntile * pl.nsplit && pl.nvalid >= 1 && pl.nvalid <= pl.nsplit);
      for (int sp = 0; sp < pl.nsplit; ++sp) {                      // both kernels: det_plan::tn_split_range, the summing one stops at nvalid
        int ms, me;
        det_plan::tn_split_range(M, pl.nsplit, sp, ms, me);
        CHECK((ms < me) == (sp < pl.nvalid));
        for (int m = ms; m < me; ++m) ++cover[m];
      }
    }
    for (int m = 0; m < M; ++m) CHECK(cover[m] == 1);
    CHECK(det_plan::cols_scratch_floats(M, Nn, Kk, ng, 2048) >= 0);
  }
  std::printf("det_plan_check: %lld staged plans checked\n", cases);
  return cases > 1000 ? 0 : 1;
}
