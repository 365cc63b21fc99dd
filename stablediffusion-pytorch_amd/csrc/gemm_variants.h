// The mainloop variants of sdmi_gemm, stated once: the table of LDS-DMA variants, which kernels exist for it, and
// the host rules that choose a variant and a column tile for a descriptor. gemm.hip plans with it; the launcher of
// gemm_dma.h instantiates and dispatches the kernels from the same table.
#pragma once
#include <stdlib.h>

#include "gemm_args.h"

namespace sdmi_gemm_impl __attribute__((visibility("hidden"))) {

// Variant 0 is the register-staged kernel (gemm_staged.hip, 128 x 128 x 64). Variants 2-11 are LDS-DMA rings:
// `stages` staged tiles of `kbk`-deep k, a tbm-row tile on tbm / 64 x nwn waves per k-group, kg k-groups per
// workgroup, and the column tiles pick_tbn chooses among (0: none).
struct DmaVariant {
  int stages, tbm, nwn, kbk, kg;
  int tbn[3];
  bool red;  // also instantiated with the reductions of col-major A (RED 1 / 2)
};
constexpr int DMA_MAX_TILES = 3;
constexpr DmaVariant DMA_VARIANTS[12] = {
    {}, {},
    /* 2*/ {2, 128, 2, 64, 1, {128, 64, 192}, true},   // the default ring: 2 x <= 80 KiB of LDS, two workgroups per CU
    /* 3*/ {3, 128, 2, 64, 1, {128, 0, 0}, false},
    /* 4*/ {4, 128, 4, 32, 1, {256, 384, 0}, true},    // 8 waves, 3 tiles (96 KiB) in flight per CU: N % 256 or % 384 == 0
    /* 5*/ {3, 128, 2, 32, 1, {128, 192, 0}, true},    // two workgroups per CU
    /* 6*/ {4, 128, 2, 64, 1, {128, 0, 0}, true},      // 128 KiB ring
    /* 7*/ {6, 64, 4, 64, 1, {64, 0, 0}, false},       // 96 KiB
    /* 8*/ {6, 64, 4, 64, 1, {128, 0, 0}, false},      // 144 KiB
    // 64 x 128 with 3 / 2 stages (72 / 48 KiB: two or three workgroups per CU) -- the M = 2048-8192 GEMMs whose
    // 128 x 128 grid is one tile per CU (8192 x 512: 256 tiles)
    /* 9*/ {3, 64, 4, 64, 1, {128, 0, 0}, false},
    /*10*/ {2, 64, 4, 64, 1, {128, 0, 0}, false},
    // two k-groups of 4 waves on one 128 x 128 tile, 2-stage 64-deep rings (128 KiB): one 8-wave workgroup per CU
    /*11*/ {2, 128, 2, 64, 2, {128, 0, 0}, true},
};

// Is variant d with column tile tbn instantiated for (a_mode, b_mode, RED)? MN-contiguous LDS images (col-major A,
// [k][n] B) come in 128-wide sub-tiles, so 64-row tiles and the 64 / 192-column tiles exist only where both images
// are K-contiguous (row-major / implicit-conv A with [n][k] B) -- the latency-bound low-resolution GEMMs and the
// narrow or ragged outputs; reductions exist only with col-major A.
constexpr bool dma_instantiated(const DmaVariant& d, int tbn, int a_mode, int b_mode, int red) {
  const bool kc = a_mode != SDMI_A_COLMAJOR && b_mode == SDMI_B_NK;
  return tbn && (kc || (d.tbm % 128 == 0 && tbn % 128 == 0)) && (red == 0 || d.red);
}

inline bool has_reductions(const sdmi_gemm_desc* d) { return d->sum_out || d->sum_out2 || d->gsum_out; }

inline int reduction_groups(const sdmi_gemm_desc* d) {
  return d->gsum_out && d->sum_group > 0 ? (d->k + d->sum_group - 1) / d->sum_group : 0;
}

// columns the launch computes: n, plus the reduction columns (8 for the sums, then the groups rounded to 8)
inline int n_total(const sdmi_gemm_desc* d) {
  if (!d->gsum_out) return d->n;  // plain sums: VALU row sums (Args::rowsum), no extra columns
  return (d->n + 7) / 8 * 8 + 8 + (reduction_groups(d) + 7) / 8 * 8;
}

// Mainloop choice (SDMI_GEMM_VARIANT overrides for A/B runs): 0 or a row of DMA_VARIANTS. -1 (default) per mode: the
// DMA ring where it measured faster on the step's shapes (row-major and implicit-conv A), register staging for the
// col-major (weight-gradient) A; the per-shape table sdmi/tuned_gemm.json overrides it through variant_hint.
inline int gemm_variant() {
  static int v = -2;
  if (v == -2) {
    const char* s = getenv("SDMI_GEMM_VARIANT");
    v = s ? atoi(s) : -1;
    if (v != 0 && (v < 2 || v > 11)) v = -1;
  }
  return v;
}

// the DMA kernels form the reduction columns from synthesised B fragments: every group of 8 consecutive k in one
// group (sum_group % 8 == 0) and at most 3 reduction tiles (8 + groups <= 48)
inline bool dma_reductions_ok(const sdmi_gemm_desc* d) {
  if (!d->gsum_out) return true;
  return d->sum_group % 8 == 0 && 8 + reduction_groups(d) <= 48;
}

inline int pick_variant(const sdmi_gemm_desc* d) {
  int v = gemm_variant();
  if (v < 0 && d->variant_hint >= 1 && d->variant_hint <= 11) v = d->variant_hint == 1 ? 0 : d->variant_hint;
  if (v < 0) v = 2;  // (col-major A with [n][k] B has no DMA instantiation: register staging below)
  // (group sums the DMA kernels cannot form go to register staging whatever was requested, 3 included)
  if (has_reductions(d) && !dma_reductions_ok(d)) v = 0;
  else if (has_reductions(d) && v == 3) v = 2;
  if (has_reductions(d) && v != 0 && d->a_mode != SDMI_A_COLMAJOR) v = 0;
  // the DMA path needs a tile-uniform second source (k_split % BK == 0)
  if (d->a_mode == SDMI_A_CONV && d->a2 && d->k_split % BK) v = 0;
  if (v == 4 && d->n % 256 && d->n % 384) v = 2;  // 128 x {256, 384} tiles: N % 384 == 0 or N % 256 == 0
  if (v == 5 && d->a_mode == SDMI_A_CONV && d->a2 && d->k_split % 32) v = 0;
  if (v != 0 && d->a_mode == SDMI_A_COLMAJOR && d->b_mode == SDMI_B_NK) v = 0;  // no DMA instantiation
  // 64-row tiles: K-contiguous images only (row-major / implicit-conv A, [n][k] B), no reduction columns
  if (v >= 7 && v <= 10 && (d->a_mode == SDMI_A_COLMAJOR || d->b_mode != SDMI_B_NK || has_reductions(d))) v = 2;
  // k-groups (128 x 128 tiles of two 4-wave groups): the DMA modes; the conv A's fused second source needs whole
  // 64-deep tiles on either side of k_split (checked above for every DMA variant)
  return v;
}

inline int tile_m(int variant) { return variant ? DMA_VARIANTS[variant].tbm : BM; }

// columns the grid covers: the DMA kernels compute the reduction columns outside the column tiles
inline int n_grid(const sdmi_gemm_desc* d, int variant) { return variant == 0 ? n_total(d) : d->n; }

// Column-tile width: the variant's only tile, else among its tiles -- for variant 2, 192 (B_NK, N % 192 == 0) when it
// needs fewer rounds x columns of the 512 workgroup slots (2 per CU) than 128 -- e.g. 32768 x 384: 768 tiles = 1.5
// rounds at 128, 512 = 1 at 192.
inline int pick_tbn(const sdmi_gemm_desc* d, int variant) {
  if (variant == 0) return BN;
  const DmaVariant& dv = DMA_VARIANTS[variant];
  if (!dv.tbn[1]) return dv.tbn[0];
  if (variant == 4) return d->n % 384 == 0 ? 384 : 256;
  if (variant == 5) return d->b_mode == SDMI_B_NK && d->n % 192 == 0 ? 192 : BN;
  if (d->b_mode != SDMI_B_NK || d->a_mode == SDMI_A_COLMAJOR) return BN;
  // narrow outputs (N <= 64: the VQVAE's 64-channel convs at 256^2, 4-channel heads, DiT proj_out): a 128-column
  // tile would spend half (or more) of its MFMAs on zero-padded columns
  if (d->n <= 64) return 64;
  // ragged N whose last 128-column tile would be at most half used (DiT hidden size 288: 3 x 128 = 384 columns,
  // 25 % padding; 5 x 64 = 320, 10 %)
  if (d->tile_n_hint != 128 && d->n % 128 && d->n % 128 <= 64 && d->n % 192) return 64;
  if (d->n % 192) return BN;
  if (d->tile_n_hint == 128 || d->tile_n_hint == 192) return d->tile_n_hint;
  const long long mt = (d->m + BM - 1) / BM;
  const long long r128 = (mt * ((d->n + BN - 1) / BN) + 511) / 512, r192 = (mt * (d->n / 192) + 511) / 512;
  return r192 * 192 <= r128 * 128 ? 192 : BN;
}

}  // namespace sdmi_gemm_impl
