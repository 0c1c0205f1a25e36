// Stand-alone host check of medmoe_amd/csrc/lamb_plan.h (no GPU, no HIP): random segment tables - one-element segments, empty ones,
// boundaries on and off the chunk grid - are walked through the record enumeration with the inline functions lamb_moments_kernel and
// lamb_ratios_kernel themselves call.  Every record index must lie inside the planned scratch, the records the moments launch stores must be
// exactly the records the ratios launch reads (no gaps, no overlaps), and the elements behind a segment's records must be the segment's.
//   make check-lamb-plan     (address + undefined-behaviour sanitizers, host compiler only)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lamb_plan.h"

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (unsigned)(rng_state >> 11); }

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

int main() {
  using namespace lamb_plan;
  const long long C = LAMB_CHUNK;
  long long tables = 0, records = 0;
  for (int it = 0; it < 4000; ++it) {
    // n: a multiple of 4 (the arenas are padded to 8), sometimes a whole number of chunks, sometimes less than one
    long long n = 4 * (1 + rnd() % (it % 5 == 0 ? 200000u : 6000u));
    if (it % 7 == 0) n = C * (1 + rnd() % 9);
    const int S = 1 + rnd() % (it % 3 == 0 ? 600 : 12);
    std::vector<long long> end(S);
    for (int s = 0; s + 1 < S; ++s) {
      const unsigned k = rnd() % 8;
      end[s] = k == 0 ? C * (rnd() % (unsigned)(n / C + 1)) : k == 1 ? 0 : (long long)(rnd() % (unsigned)(n + 1));
    }
    end[S - 1] = n;
    for (int s = 1; s < S; ++s) for (int j = s; j > 0 && end[j - 1] > end[j]; --j) { const long long t = end[j]; end[j] = end[j - 1]; end[j - 1] = t; }
    if (it % 11 == 0 && S > 3) end[1] = end[0] + (end[0] < end[2] ? 1 : 0);          // a one-element segment
    std::vector<long long> base(S, -1);
    const long long nrec = plan(end.data(), S, n, base.data());
    CHECK(nrec >= 1 && nrec <= max_records(n, S) && 2 * nrec <= coef_slot(n, S) && coef_slot(n, S) + 2 == scratch_floats(n, S));
    // the moments launch: chunk c meets segments sf .. sl and stores record_index(base[s], start_s, c) for each with elements in the chunk
    std::vector<int> stored(nrec, 0);
    std::vector<long long> elems(nrec, 0);
    const long long nch = n_chunks(n);
    CHECK(nch * C >= n && (nch - 1) * C < n);
    int s0 = 0;
    for (long long c = 0; c < nch; ++c) {
      const long long c0 = c * C, c1 = c0 + C < n ? c0 + C : n;
      while (end[s0] <= c0) ++s0;                                   // first segment whose end lies behind c0 (lamb_find)
      for (int s = s0; s < S; ++s) {
        const long long start = s ? end[s - 1] : 0;
        if (start >= c1) break;
        const long long lo = start > c0 ? start : c0, hi = end[s] < c1 ? end[s] : c1;
        if (hi <= lo) continue;                                     // an empty segment inside the chunk: no record
        const long long idx = record_index(base[s], start, c);
        CHECK(idx >= 0 && idx < nrec);
        CHECK(idx >= base[s] && idx < base[s] + seg_chunks(start, end[s]));
        ++stored[idx];
        elems[idx] += hi - lo;
      }
    }
    // the ratios launch: segment s reads base[s] .. base[s] + seg_chunks - 1
    std::vector<int> read(nrec, 0);
    long long next = 0;
    for (int s = 0; s < S; ++s) {
      const long long start = s ? end[s - 1] : 0, cnt = seg_chunks(start, end[s]);
      CHECK(base[s] == next);                                       // back to back: no gap, no overlap between segments
      long long covered = 0;
      for (long long r = 0; r < cnt; ++r) { CHECK(base[s] + r < nrec); ++read[base[s] + r]; covered += elems[base[s] + r]; }
      CHECK(covered == end[s] - start);                             // the records of a segment hold exactly its elements
      CHECK((cnt == 0) == (end[s] == start));
      next += cnt;
    }
    CHECK(next == nrec);
    for (long long r = 0; r < nrec; ++r) CHECK(stored[r] == 1 && read[r] == 1);
    ++tables; records += nrec;
  }
  // tables the host must refuse
  { long long e[2] = {8, 4}, b[2]; CHECK(plan(e, 2, 8, b) == -1); }
  { long long e[2] = {4, 8}, b[2]; CHECK(plan(e, 2, 16, b) == -1); }
  { long long e[1] = {8}, b[1]; CHECK(plan(e, 1, 8, b) == 1 && b[0] == 0); }
  std::printf("lamb_plan_check: %lld segment tables, %lld records checked\n", tables, records);
  return tables == 4000 ? 0 : 1;
}
