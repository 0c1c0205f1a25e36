// Stand-alone host check of medmoe_amd/csrc/topk_list.h (no GPU, no HIP): the insert and the merge the retrieval kernels run in registers,
// against std::stable_sort under the order (score descending, key index ascending) on random and tie-heavy streams, for every K from 1 to 16,
// streams shorter than K, scores of -inf and NaN, and merges of 1 .. 7 partial lists that were built from interleaved or contiguous shares.
//   make check-topk     (address + undefined-behaviour sanitizers, host compiler only)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "topk_list.h"

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (unsigned)(rng_state >> 11); }

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

struct Entry { float v; int i; };

struct List {
  float val[TOPK_MAX];
  int idx[TOPK_MAX];
  List() { topk_init(val, idx); }
};

// what the kernels do per candidate: gate on the K-th entry, then insert
static void offer(List& l, int K, float v, int i) {
  float kv; int ki;
  topk_kth(l.val, l.idx, K, kv, ki);
  if (topk_before(v, i, kv, ki)) topk_insert(l.val, l.idx, K, v, i);
}

static void expect(const List& l, int K, std::vector<Entry> all) {
  all.erase(std::remove_if(all.begin(), all.end(), [](const Entry& e) { return std::isnan(e.v); }), all.end());
  std::stable_sort(all.begin(), all.end(), [](const Entry& a, const Entry& b) { return a.i < b.i; });
  std::stable_sort(all.begin(), all.end(), [](const Entry& a, const Entry& b) { return a.v > b.v; });
  for (int k = 0; k < TOPK_MAX; ++k) {
    if (k < K && k < (int)all.size()) {
      CHECK(l.idx[k] == all[k].i);
      CHECK(l.val[k] == all[k].v);
    } else {
      CHECK(l.idx[k] == TOPK_EMPTY);
      CHECK(l.val[k] == -INFINITY);
    }
  }
}

int main() {
  long long cases = 0;
  for (int it = 0; it < 6000; ++it) {
    const int K = it < 64 ? 1 + it % 16 : (rnd() % 4 == 0 ? (rnd() % 2 ? 1 : 16) : 1 + (int)(rnd() % 16));
    const int n = rnd() % 3 == 0 ? (int)(rnd() % (unsigned)(K + 1)) : (int)(rnd() % 400);      // a third of the streams are shorter than K
    const int mode = rnd() % 4;                                                                    // 0 random, 1 / 2 tie-heavy, 3 with -inf and NaN
    std::vector<Entry> all(n);
    for (int j = 0; j < n; ++j) {
      float v;
      if (mode == 0) v = (float)(rnd() % 2000001) / 1e6f - 1.f;
      else if (mode == 1) v = (float)((int)(rnd() % 5) - 2);
      else if (mode == 2) v = 0.25f;
      else v = rnd() % 7 == 0 ? -INFINITY : (rnd() % 11 == 0 ? NAN : (float)((int)(rnd() % 9) - 4));
      all[j] = {v, j};
    }
    // one list over the whole stream, offered in index order (a lane's stream) and in a shuffled order
    List a, b;
    for (const Entry& e : all) offer(a, K, e.v, e.i);
    std::vector<Entry> sh = all;
    for (int j = n - 1; j > 0; --j) std::swap(sh[j], sh[rnd() % (unsigned)(j + 1)]);
    for (const Entry& e : sh) offer(b, K, e.v, e.i);
    expect(a, K, all);
    expect(b, K, all);
    // P partial lists over interleaved (the four lanes of a query) or contiguous (key splits) shares, merged in a random order
    const int P = 1 + rnd() % 7;
    const bool interleave = rnd() % 2;
    std::vector<List> part(P);
    const int per = (n + P - 1) / P;
    for (const Entry& e : all) offer(part[interleave ? e.i % P : (per ? e.i / per : 0)], K, e.v, e.i);
    std::vector<int> order(P);
    for (int p = 0; p < P; ++p) order[p] = p;
    for (int p = P - 1; p > 0; --p) std::swap(order[p], order[rnd() % (unsigned)(p + 1)]);
    List m;
    for (int p : order) {
      // exactly K readable entries, as the kernels pass them: reading past K would be an out-of-bounds read there
      std::vector<float> sv(part[p].val, part[p].val + K);
      std::vector<int> si(part[p].idx, part[p].idx + K);
      topk_merge(m.val, m.idx, K, sv.data(), si.data(), K);
    }
    expect(m, K, all);
    cases += 3;
  }
  std::printf("topk_list_check: %lld lists ok\n", cases);
  return 0;
}
