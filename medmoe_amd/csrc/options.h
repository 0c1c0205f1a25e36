// The run-time options of medmoe_set_option(key, value) (options.hip).  Each variable is defined, with its default, in the file that
// reads it; a value outside the range given here is refused with MM_ERR_ARG and changes nothing.  All are host-side and hidden.
#pragma once
#include "common.h"

//  key  range              meaning
//    1  any                0: plain NT GEMMs stay off the 256-row tiles altogether (gemm_nt256_kernel and the 256x256 kernels)
//    2  any                0: plain NT GEMMs stay off the 256x256 tiles (gemm_nt512_kernel, gemm_nt4w_kernel)
//    3  any                0: medmoe_gemm_tn stays off the 256x256 tiles (gemm_tn512_kernel, gemm_tn4w_kernel): gemm_tn_kernel takes everything
//    4  >= 256             wgrad in groups or with a row map on the 256x256 tiles, where the ranges are not enumerated on the device
//                          (no row_off, or key 8 = 0): rows per range
//    5  1 .. 256           experiments with fewer CUs: largest grid of the plain 256x256 NT kernels
//    6  any                0: the local-loss score GEMM stays off scores512_kernel
//    7  any                0: 256x256 NT tiles on the eight-wave gemm_nt512_kernel instead of gemm_nt4w_kernel
//    8  any                0: 256x256 wgrad tiles on the eight-wave gemm_tn512_kernel instead of gemm_tn4w_kernel
//    9  >= 64              plain wgrad: fewest rows per M range
//   10  >= 0               grouped wgrad on gemm_tn4w_kernel: rows per range (0 = auto)
//   11  any                attention: 1 = resident kernels where the keys fit LDS (N <= 272), 0 = streaming kernels for every N
//   12  any                MEASUREMENT ONLY: 1 = score GEMM without its epilogue, 2 = epilogue arithmetic without its stores
//   13  >= 0               scale_attn_bwd: rows per wave (0 = auto)
//   15  0, 448, 512        attention, 13 key tiles: threads per workgroup (0 = auto)
//   16  any                LayerNorm, bit 0 the forward and bit 1 the backward kernels: one row per wave whatever the width (A/B runs)
//   17  any                0: K % 64 == 32 products on the 128x128 DMA kernel instead of gemm_nt_direct_kernel (A/B runs)
MM_HIDDEN extern int g_use_nt256;         //  1  gemm_nt.hip
MM_HIDDEN extern int g_use_nt512;         //  2  gemm_nt.hip
MM_HIDDEN extern int g_use_tn512;         //  3  gemm.hip
MM_HIDDEN extern int g_tn_rows;           //  4  gemm.hip
MM_HIDDEN extern int g_nt_max_grid;       //  5  gemm_nt.hip
MM_HIDDEN extern int g_use_scores512;     //  6  gemm_scores.hip
MM_HIDDEN extern int g_use_nt4w;          //  7  gemm_nt.hip
MM_HIDDEN extern int g_use_tn4w;          //  8  gemm.hip
MM_HIDDEN extern int g_tn_min_rows;       //  9  gemm.hip
MM_HIDDEN extern int g_tn_rows4w;         // 10  gemm.hip
MM_HIDDEN extern int g_attn_resident;     // 11  attention.hip
MM_HIDDEN extern int g_scores_skip_epi;   // 12  gemm_scores.hip
MM_HIDDEN extern int g_sa_rows;           // 13  moe.hip
MM_HIDDEN extern int g_attn_rt13;         // 15  attention.hip
MM_HIDDEN extern int g_ln_one_row;        // 16  norm.hip
MM_HIDDEN extern int g_use_nt_direct;     // 17  gemm_nt.hip
