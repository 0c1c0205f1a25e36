// Arithmetic of the deterministic (staged) weight-gradient launches: which kernel form a shape takes, how many partial-tile slots it needs,
// how large the caller's scratch must be, and the enumeration of the row ranges - the SAME inline functions in gemm_tn4w_kernel (which
// stores a range's partial tile), in tn_reduce_det_kernel (which sums a group's ranges) and on the host.  Plain C++ that also compiles
// without HIP, so that a stand-alone host program can call it (tools/det_plan_check.cpp, `make check-plan`: address + undefined-behaviour
// sanitizers on the host).
#pragma once

#if defined(__HIPCC__)
#define DET_PLAN_HD __host__ __device__ __forceinline__
#else
#define DET_PLAN_HD static inline
#endif

namespace det_plan {

// Ranges of R rows enumerated over row groups (row_off[g] .. row_off[g + 1]) in group order; every group ends in at most one ragged
// range, an empty group has none.  Range `rid` -> its group and rows [ms, me); false: rid is past the last range.
DET_PLAN_HD bool tn_group_range(const int* row_off, int n_groups, int R, int rid, int& group, int& ms, int& me) {
  for (int gq = 0; gq < n_groups; ++gq) {
    const int a = row_off[gq], b = row_off[gq + 1];
    const int nr = (b - a + R - 1) / R;
    if (rid < nr) { group = gq; ms = a + rid * R; me = b < ms + R ? b : ms + R; return true; }
    rid -= nr;
  }
  return false;
}

// the ranges of one group in that enumeration: the id of its first range and how many it has
DET_PLAN_HD void tn_group_ranges(const int* row_off, int group, int R, int& first, int& count) {
  first = 0;
  for (int gq = 0; gq < group; ++gq) first += (row_off[gq + 1] - row_off[gq] + R - 1) / R;
  count = (row_off[group + 1] - row_off[group] + R - 1) / R;
}

// even split of M rows into nsplit ranges of whole 32-row steps (TN_PLAIN / TN_ROWMAP / column groups): rows per range, and range sp's
// rows [ms, me) - empty (ms >= me) past the last valid one
DET_PLAN_HD int tn_chunk(int M, int nsplit) { return (((M + 31) / 32 + nsplit - 1) / nsplit) * 32; }
DET_PLAN_HD void tn_split_range(int M, int nsplit, int sp, int& ms, int& me) {
  const int chunk = tn_chunk(M, nsplit);
  ms = sp * chunk; me = M < ms + chunk ? M : ms + chunk;
}

enum TnKind { TN_SMALL = 0, TN_PLAIN = 1, TN_ROWMAP = 2, TN_GROUPS = 3 };

struct TnPlan {
  TnKind kind;          // TN_SMALL: gemm_tn_kernel, one workgroup per (group, tile) - no scratch;  others: gemm_tn4w_kernel, staged
  int tiles_n, tiles_k; // 256 x 256 tiles of one group's dW
  int nsplit;           // TN_PLAIN / TN_ROWMAP: row ranges per tile;  TN_GROUPS: ROWS per range (ranges are enumerated over the groups)
  int nvalid;           // TN_PLAIN / TN_ROWMAP: ranges that hold rows (the last ones of an uneven split are empty)
  int slots;            // partial tiles = workgroups of the launch
  long long scratch_floats;   // slots * (65536 + 512): the tiles, then 512 column sums of G per slot
};

// upper bound of the ranges of R rows over n_groups groups that hold M rows in all: every group adds at most one ragged range
static inline int tn_group_ranges_bound(int M, int R, int n_groups) { return M / R + n_groups; }

static inline TnPlan tn_plan(int M, int Nn, int Kk, bool x_mapped, bool g_mapped, bool grouped, int n_groups, bool fit32,
                             int min_rows, int rows4w) {
  TnPlan pl{TN_SMALL, 0, 0, 1, 1, 0, 0};
  if (M <= 0 || Nn <= 0 || Kk <= 0 || n_groups < 1 || min_rows < 1) return pl;
  const bool mapped = x_mapped || g_mapped;
  if (!fit32 || (x_mapped && g_mapped) || (Kk % 256) != 0) return pl;
  if (!mapped && !grouped && n_groups == 1) {
    if ((M % 32) != 0 || (Nn % 256) != 0 || M < 4096) return pl;
    pl.kind = TN_PLAIN;
  } else {
    if ((Nn % 128) != 0 || M / n_groups < 2048 || (!grouped && n_groups != 1)) return pl;
    pl.kind = grouped ? TN_GROUPS : TN_ROWMAP;
  }
  pl.tiles_n = (Nn + 255) / 256; pl.tiles_k = Kk / 256;
  const int ntile = pl.tiles_n * pl.tiles_k;
  if (pl.kind == TN_GROUPS) {
    // ranges of R rows (4096 measured best for the atomic form); longer ones where the partial tiles would pass ~512 slots (128 MB)
    long long R = rows4w > 0 ? (rows4w + 31) / 32 * 32 : 4096;
    while ((long long)ntile * tn_group_ranges_bound(M, (int)R, n_groups) > 512 && R < M) R *= 2;
    pl.nsplit = (int)R;
    pl.nvalid = 0;
    pl.slots = ntile * tn_group_ranges_bound(M, (int)R, n_groups);
  } else {
    int ns = 256 / ntile < M / min_rows ? 256 / ntile : M / min_rows;
    pl.nsplit = ns < 1 ? 1 : ns;
    const int chunk = tn_chunk(M, pl.nsplit);
    pl.nvalid = (M + chunk - 1) / chunk;
    pl.slots = ntile * pl.nsplit;
  }
  pl.scratch_floats = (long long)pl.slots * (65536 + 512);
  return pl;
}

// medmoe_gemm_tn_cols_det: n_groups column groups of an Nn x Kk block over all M rows
static inline long long cols_scratch_floats(int M, int Nn, int Kk, int n_groups, int min_rows) {
  if (M <= 0 || Nn <= 0 || Kk <= 0 || n_groups < 1 || min_rows < 1) return 0;
  const long long ntile = (long long)((Nn + 255) / 256) * ((Kk + 255) / 256) * n_groups;
  long long ns = 256 / ntile < M / min_rows ? 256 / ntile : M / min_rows;
  if (ns < 1) ns = 1;
  return ns > 1 ? ntile * ns * 65536 : 0;
}

}  // namespace det_plan
