// Arithmetic of the LAMB step's segmented norms (lamb.hip): the arena is cut into chunks of LAMB_CHUNK elements, a segment (one
// parameter tensor: elements [seg_end[s - 1], seg_end[s]), seg_end ascending, seg_end[n_segs - 1] == n) leaves one record - the partial sums
// of p^2 and u^2, two floats - per chunk it touches, and the records of a segment lie back to back in chunk order behind those of the
// segment in front of it.  The layout is a function of (seg_end, LAMB_CHUNK) alone: not of the grid, not of the CU count.  The SAME inline
// functions in lamb_moments_kernel (which stores a record), in lamb_ratios_kernel (which adds a segment's records in index order) and on the
// host (the record-base table, the scratch size).  Plain C++ that also compiles without HIP, so that a stand-alone host program can call it
// (tools/lamb_plan_check.cpp, `make check-lamb-plan`: address + undefined-behaviour sanitizers on the host).
#pragma once

#if defined(__HIPCC__)
#define LAMB_PLAN_HD __host__ __device__ __forceinline__
#else
#define LAMB_PLAN_HD static inline
#endif

namespace lamb_plan {

// elements per chunk: one pass of a 256-thread workgroup, LAMB_VEC float4s per thread
constexpr int LAMB_THREADS = 256;
constexpr int LAMB_VEC = 4;
constexpr long long LAMB_CHUNK = (long long)LAMB_THREADS * LAMB_VEC * 4;     // 4096
constexpr int LAMB_RATIO_THREADS = 64;                                       // lamb_ratios_kernel: one wave per segment

LAMB_PLAN_HD long long n_chunks(long long n) { return (n + LAMB_CHUNK - 1) / LAMB_CHUNK; }

// the chunks that segment [start, end) touches: the first one and how many (0 for an empty segment)
LAMB_PLAN_HD long long seg_first_chunk(long long start) { return start / LAMB_CHUNK; }
LAMB_PLAN_HD long long seg_chunks(long long start, long long end) {
  return end > start ? (end - 1) / LAMB_CHUNK - start / LAMB_CHUNK + 1 : 0;
}

// the record of (segment with first record `rec_base` that starts at element `start`, chunk c); c must be one of the segment's chunks
LAMB_PLAN_HD long long record_index(long long rec_base, long long start, long long c) { return rec_base + (c - seg_first_chunk(start)); }

// upper bound of the records of ANY table of n_segs segments over n elements: every chunk holds one record, and every segment boundary
// inside a chunk adds at most one.  Two floats per record.
LAMB_PLAN_HD long long max_records(long long n, long long n_segs) { return n_chunks(n) + n_segs; }
// behind the records: the clip coefficient the moments launch used (grad_scale * min(1, clip / norm)), kept for the host to read - one float,
// the slot padded to two
LAMB_PLAN_HD long long coef_slot(long long n, long long n_segs) { return 2 * max_records(n, n_segs); }
LAMB_PLAN_HD long long scratch_floats(long long n, long long n_segs) { return n > 0 && n_segs > 0 ? coef_slot(n, n_segs) + 2 : 0; }

// host: rec_base[s] = records of the segments in front of s; returns the number of records, or -1 for a table that is not ascending, has a
// negative end, or does not end at n
static inline long long plan(const long long* seg_end, long long n_segs, long long n, long long* rec_base) {
  long long start = 0, recs = 0;
  if (n_segs < 1 || n <= 0) return -1;
  for (long long s = 0; s < n_segs; ++s) {
    const long long end = seg_end[s];
    if (end < start || end > n) return -1;
    rec_base[s] = recs;
    recs += seg_chunks(start, end);
    start = end;
  }
  return start == n ? recs : -1;
}

}  // namespace lamb_plan
