// Stand-alone host check of medmoe_amd/csrc/seg_plan.h (no GPU, no HIP): for random (g, H) - H = g, H barely above g, integer and non-integer
// scales - the per-patch supports seg_grad_kernel walks are compared with the forward map every other kernel uses, through the same inline
// functions.  Along one axis:
//   - every (pixel, corner) pair with a non-zero weight lies in the support of the corner's patch, and in no other way: a pixel of patch i's
//     support reads patch i with a non-zero weight (the supports are tight), so the supports partition exactly those pairs;
//   - the supports are contiguous, inside [0, H), non-empty, and start in patch order;
//   - the adjoint in gather form (patch by patch over its support) equals the scatter form (pixel by pixel to its two corners) in EXACT
//     integer arithmetic: weights scaled to integers, random integer pixel values;
//   - a pixel's weights sum to one, and indices past the last pixel still map inside the grid (the padded lanes of a 16-pixel unit).
//   make check-seg-plan     (address + undefined-behaviour sanitizers, host compiler only)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "seg_plan.h"

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (unsigned)(rng_state >> 11); }

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed (g = %d, H = %d)\n", __FILE__, __LINE__, #c, g, H); std::exit(1); } } while (0)

static long long q(float w) { return std::llround(std::ldexp((double)w, 30)); }       // a weight as an exact integer: float -> 2^30 grid

int main() {
  long long axes = 0, pairs = 0;
  for (int it = 0; it < 6000; ++it) {
    const int g = 1 + (int)(rnd() % (it % 4 == 0 ? 64u : 24u));
    int H;
    switch (rnd() % 6) {
      case 0: H = g; break;
      case 1: H = g + 1 + (int)(rnd() % 3); break;
      case 2: H = g * (1 + (int)(rnd() % 20)); break;
      default: H = g + (int)(rnd() % 700u); break;
    }
    const float scale = seg_scale(g, H);
    std::vector<SegSrc> src(H);
    std::vector<long long> val(H), scatter(g, 0), gather(g, 0);
    std::vector<int> reads(H, 0), covered(H, 0);                                   // non-zero corners of a pixel / supports it lies in
    for (int y = 0; y < H; ++y) {
      const SegSrc s = src[y] = seg_src(y, scale, g);
      CHECK(s.i0 >= 0 && s.i0 < g && (s.i1 == s.i0 + 1 || (s.i1 == s.i0 && s.i0 == g - 1)) && s.lam >= 0.f && s.lam < 1.f);
      CHECK(y == 0 || s.i0 >= src[y - 1].i0);                                     // monotone
      val[y] = (long long)(rnd() % 2001u) - 1000;
      float total = 0.f;
      for (int i = s.i0; i <= s.i1; ++i) {
        const float w = seg_weight(s, i);
        total += w;
        reads[y] += w != 0.f;
        scatter[i] += val[y] * q(w);
        pairs += w != 0.f;
      }
      CHECK(std::fabs(total - 1.f) <= 1.2e-7f);
      CHECK(y == 0 || seg_reaches(y, scale, g, s.i0));
    }
    for (int y = H; y < H + 16; ++y) {                                            // padded lanes: inside the grid
      const SegSrc s = seg_src(y, scale, g);
      CHECK(s.i0 >= 0 && s.i0 < g && s.i1 >= 0 && s.i1 < g && s.lam >= 0.f && s.lam <= 1.f);
    }
    int prev_lo = 0, prev_hi = 0;
    for (int i = 0; i < g; ++i) {
      int lo = -1, hi = -1;
      seg_support(i, g, H, &lo, &hi);
      CHECK(0 <= lo && lo < hi && hi <= H);                                       // contiguous by construction, non-empty
      CHECK(i == 0 ? lo == 0 : (lo >= prev_lo && hi > prev_hi));
      CHECK(i + 1 < g || hi == H);
      for (int y = lo; y < hi; ++y) {
        const float w = seg_weight(src[y], i);
        CHECK(w != 0.f);                                                          // tight: nothing of zero weight is walked
        gather[i] += val[y] * q(w);
        ++covered[y];
      }
      if (lo > 0) CHECK(seg_weight(src[lo - 1], i) == 0.f);
      if (hi < H) CHECK(seg_weight(src[hi], i) == 0.f);
      if (H == g) CHECK(lo == i && hi == i + 1);                                  // scale 1: the upsample is the identity
      prev_lo = lo; prev_hi = hi;
    }
    for (int y = 0; y < H; ++y) CHECK(covered[y] == reads[y]);                    // each non-zero pair in exactly one support
    for (int i = 0; i < g; ++i) CHECK(gather[i] == scatter[i]);
    ++axes;
  }
  std::printf("seg_plan_check: %lld axes, %lld (pixel, corner) pairs ok\n", axes, pairs);
  return 0;
}
