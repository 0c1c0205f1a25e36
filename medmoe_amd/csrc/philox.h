// Counter-based random bits for dropout: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11).
// The keep mask of an element is a pure function of (seed, step, site, element index) - nothing of the launch geometry, the lane
// layout or the tile shape enters - so a backward kernel regenerates the forward's mask in registers and no mask is ever stored.
//
//   key      = (seed & 0xffffffff, seed >> 32)
//   counter  = (group & 0xffffffff, group >> 32, site, step)
//   group    = 4 consecutive elements along the fastest axis: element (row, col) of a [rows][cols_padded] array (cols_padded % 4 == 0)
//              lives in group row * (cols_padded / 4) + col / 4 as word col % 4
//   keep     = word >= thresh,  thresh = floor(p * 2^32) computed on the host;  survivors are scaled by 1 / (1 - p) in fp32
//   site     = 4 * layer + {0 attention probabilities, 1 after the output projection, 2 after FC2};  DROPOUT_SITE_EMBED for the
//              embedding LayerNorm's output
//   stochastic depth of the image tower: site = DROPOUT_SITE_VIT_DROP_PATH + 2 * layer + {0 attention branch, 1 feed-forward
//              branch}; ONE draw per sample: the keep bit of global sample g is element (row 0, column g) of a [1][cols_padded] array
//   image augmentation (augment.hip): site = DROPOUT_SITE_AUGMENT; global sample g owns the groups 4 g + {0 crop / flip / order,
//              1 affine, 2 colour jitter}, whose words are turned into integers and uniform floats there
//   LoRA adapters on the image tower: site = DROPOUT_SITE_VIT_LORA + layer, over the [B * n_tok][d_v] array of the layer's ln1
//   masked-language-model mask (mlm.hip): site = DROPOUT_SITE_MLM; token t of global sample g owns the group g * T + t: word 0
//              selects it (word < thresh), word 1 picks [MASK] / random / keep, word 2 the random id
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define DROPOUT_SITE_EMBED 0xffffffffu
#define DROPOUT_SITE_VIT_DROP_PATH 0x40000000u
#define DROPOUT_SITE_AUGMENT 0x20000000u
#define DROPOUT_SITE_VIT_LORA 0x50000000u
#define DROPOUT_SITE_MLM 0x60000000u

struct DropRng {
  uint32_t k0, k1;      // the two halves of the seed
  uint32_t step, site;
  uint32_t thresh;      // keep iff word >= thresh
  float scale;          // 1 / (1 - p)
};

static inline DropRng make_drop_rng(long long seed, long long step, long long site, long long thresh, float scale) {
  DropRng r;
  r.k0 = (uint32_t)((unsigned long long)seed & 0xffffffffull);
  r.k1 = (uint32_t)((unsigned long long)seed >> 32);
  r.step = (uint32_t)step; r.site = (uint32_t)site; r.thresh = (uint32_t)thresh; r.scale = scale;
  return r;
}

__device__ __forceinline__ uint4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1;
    c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return make_uint4(c0, c1, c2, c3);
}

// the four random words of one group
__device__ __forceinline__ uint4 drop_words(const DropRng& r, unsigned long long group) {
  return philox4x32_10((uint32_t)group, (uint32_t)(group >> 32), r.site, r.step, r.k0, r.k1);
}

// bit j set = element j of the group survives
__device__ __forceinline__ uint32_t drop_keep4(const DropRng& r, unsigned long long group) {
  const uint4 w = drop_words(r, group);
  return (w.x >= r.thresh ? 1u : 0u) | (w.y >= r.thresh ? 2u : 0u) | (w.z >= r.thresh ? 4u : 0u) | (w.w >= r.thresh ? 8u : 0u);
}
