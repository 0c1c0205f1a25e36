// Sorted top-K lists of (score, key index) for the retrieval kernels (retrieval.hip), host and device: tools/topk_list_check.cpp runs the
// same functions on the CPU under the sanitizers (make check-topk).
//
// The order is total: a goes before b when its score is larger, or the scores are equal and its index is smaller.  A list always has
// TOPK_MAX slots so that every index into it is a compile-time constant (it lives in registers on the device); the first K are in use,
// sorted best first, and an unused slot holds (-inf, TOPK_EMPTY).  TOPK_EMPTY is INT_MAX, so an empty slot orders after every real entry,
// a real score of -inf included; the kernels store -1 in its place.  A NaN score goes before nothing and is never listed.
#pragma once
#include <limits.h>
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TOPK_HD __host__ __device__ __forceinline__
#else
#define TOPK_HD inline
#endif

#define TOPK_MAX 16
#define TOPK_EMPTY INT_MAX

TOPK_HD bool topk_before(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }

TOPK_HD void topk_init(float (&val)[TOPK_MAX], int (&idx)[TOPK_MAX]) {
#pragma unroll
  for (int i = 0; i < TOPK_MAX; ++i) { val[i] = -INFINITY; idx[i] = TOPK_EMPTY; }
}

// the K-th entry (slot K - 1): a candidate enters the list iff it goes before this one
TOPK_HD void topk_kth(const float (&val)[TOPK_MAX], const int (&idx)[TOPK_MAX], int K, float& kv, int& ki) {
  kv = val[0]; ki = idx[0];
#pragma unroll
  for (int i = 1; i < TOPK_MAX; ++i)
    if (i == K - 1) { kv = val[i]; ki = idx[i]; }
}

// Insert (cv, ci) into the first K slots: the candidate walks down the list and changes places with every entry it goes before, so the
// slots stay sorted and the former K-th entry falls off the end.  Selects only, no branch depends on the data.
TOPK_HD void topk_insert(float (&val)[TOPK_MAX], int (&idx)[TOPK_MAX], int K, float cv, int ci) {
#pragma unroll
  for (int i = 0; i < TOPK_MAX; ++i)
    if (i < K) {
      const bool b = topk_before(cv, ci, val[i], idx[i]);
      const float tv = b ? val[i] : cv;
      const int ti = b ? idx[i] : ci;
      val[i] = b ? cv : val[i];
      idx[i] = b ? ci : idx[i];
      cv = tv; ci = ti;
    }
}

// Merge a sorted list of n <= K entries (sv, si: any memory) into the list: an entry that does not go before the K-th ends the walk, since
// everything after it in its own list is ordered later still.
TOPK_HD void topk_merge(float (&val)[TOPK_MAX], int (&idx)[TOPK_MAX], int K, const float* sv, const int* si, int n) {
  for (int i = 0; i < n; ++i) {
    float kv; int ki;
    topk_kth(val, idx, K, kv, ki);
    if (!topk_before(sv[i], si[i], kv, ki)) break;
    topk_insert(val, idx, K, sv[i], si[i]);
  }
}
