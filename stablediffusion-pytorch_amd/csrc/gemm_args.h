// Kernel arguments of the GEMM family (gemm.hip), shared by the host planning and by every source that holds GEMM
// kernels, and the launch functions those sources provide. The kernels themselves live in anonymous namespaces (their
// names are matched by the profiling tools); what crosses translation units is in sdmi_gemm_impl, hidden from the
// library's exported surface.
#pragma once
#include "common.h"
#include "../../include/sdmi.h"

namespace sdmi_gemm_impl __attribute__((visibility("hidden"))) {

constexpr int BM = 128, BN = 128, BK = 64, NT = 256;

struct Args {
  int M, N, K;
  const bf16_t* A; int lda;
  const bf16_t* B; int ldb;
  // gather geometry
  int ih, iw, cin, ldx, kw, sy, sx, oy0, ox0;
  FastDiv ohw_d, ow_d;  // GEMM pixel grid: pixel m -> (b, oy, ox) = (m / (oh*ow), (m % (oh*ow)) / ow, m % ow)
  int ktiles_per_split, nsplit;
  const bf16_t* A2; int lda2; int k_split;
  // reduction columns (col-major A only): B columns n >= n_x0 are synthesised instead of loaded -- column n_x0 is
  // all ones (C gets the row sums of A over k: a bias gradient), columns n_x0 + 8 + j are the indicator of
  // k / grp == j (C gets per-group row sums: the per-sample time-embedding gradient). 0 = none.
  int n_x0;
  FastDiv grp_d;
  // 1: row sums of A over k accumulated from the staged A chunks in VALU (bias gradient without the extra tile
  // column the synthesised-column path costs; used when no per-group sums are wanted)
  int rowsum;
  // implicit-im2col B (weight gradients, k = pixel): how a full k-tile of KBK consecutive pixels maps onto the output
  // grid, bit flags per staged depth (bits 0-1: KBK 64, bits 2-3: KBK 32). Form 1: the tile is KBK / ow whole rows of
  // one image (oh * ow % KBK == 0, KBK % ow == 0) -> image and first row are tile-uniform, each lane's row offset and
  // column are fixed; form 2: the tile is KBK / (oh * ow) whole images (KBK % (oh * ow) == 0) -> only the first image
  // is tile-uniform. Either way the per-piece gather needs no division (DMA kernel, issue_fast_b).
  int bfast;
  // grouped launch (sdmi_gemm_grouped): ngroups > 1 independent problems of one shape; the grid's z runs over
  // (problem, split) and problem p reads its operands from Ag[p] / Bg[p] (Ag[0] = A, Bg[0] = B)
  int ngroups;
  const bf16_t* Ag[SDMI_GEMM_GROUP_MAX];
  const bf16_t* Bg[SDMI_GEMM_GROUP_MAX];
  // the outputs of problem p (copies of EpiArgs::Cg / sum_g: indexed here, in the kernel-argument segment, so the
  // epilogue's local EpiArgs copy is never indexed dynamically -- that would put it in scratch)
  void* Cg[SDMI_GEMM_GROUP_MAX];
  float* sum_g[SDMI_GEMM_GROUP_MAX];
#ifdef SDMI_GEMM_TRACE
  // probe build only (scripts/gemm_phase_probe.py): the phase-timestamp buffer of the LDS-DMA kernels, a device
  // allocation owned by gemm.hip (8 words per workgroup, 2^17 workgroups)
  unsigned long long* trace;
#endif
};

// epilogue parameters (a separate kernel argument keeps both structs small enough to stay in SGPRs)
struct EpiArgs {
  int M, N;
  void* C; int ldc; int c_f32; long long split_stride;
  const float* bias; const float* bias2; const bf16_t* rowbias; int rb_ld;
  const bf16_t* resid; int ldr;
  float alpha; int act;
  int remap, r_oh, r_ow, r_sy, r_sx, r_oy, r_ox;
  // output-row grid of the GEMM: rows per sample (the rowbias row divisor, and gh * gw of a remap) and the remap's
  // grid width gw (fill_args rejects a remap whose rowbias divisor differs)
  FastDiv pix_d, gw_d;
  int perm, p_cin, p_taps, p_cvalid;
  unsigned p_magic;   // ceil(2^32 / p_cin): tap = umulhi(col, p_magic), exact for col < 2^32 / p_cin
  unsigned n8_magic;  // ceil(2^32 / (N / 8)) for the reducer's row split (0: N / 8 == 1)
  int m_store, n_store;
  int raw;  // 1: write raw fp32 partials (split-K) to ws, epilogue applied by the reducer
  int nsplit;
  const float* ws;  // split-K slabs [nsplit][M][N]
  int vec;          // LDS-staged 16-B row stores (no column permute, 8-aligned columns/strides)
  int n8;           // N % 8 == 0: split-K slabs are written / read as 16-B rows even when !vec
  int rb_mod;       // rowbias row = (row / rb_div) % rb_mod when > 0 (per-token tables, e.g. position embedding)
  const bf16_t* aux; int ld_aux;  // act 3: ReLU-gradient mask source (aux[orow*ld_aux + col] > 0)
  // reduction columns (Args::n_x0): column n_x0 -> sum_out[row] (and sum_out2), column n_x0 + 8 + j (j < ngrp)
  // -> gsum[j * gsum_ld + row] (bf16); rows < m_store only
  int n_x0, ngrp, gsum_ld;
  float* sum_out;
  float* sum_out2;
  bf16_t* gsum;
  int n_gemm;  // columns the MFMA tiles produce (N, or N plus the synthesised reduction columns); with split-K the
               // slab row width N is n_gemm + 8 when the VALU row sums ride along in slab column n_x0 = n_gemm
  // grouped launch: problem p stores to Cg[p] / sum_g[p], its split-K slabs start p * ws_gstride floats into ws
  void* Cg[SDMI_GEMM_GROUP_MAX];
  float* sum_g[SDMI_GEMM_GROUP_MAX];
  long long ws_gstride;
  // GroupNorm-backward statistics (sdmi_gemm_desc::gn_part): per gn_rb-row segment and column, sum dz and dz*xhat
  const bf16_t* gn_x; int gn_ldx;
  const float4* gn_tab;
  float* gn_part;
  int gn_rb, gn_silu;
  FastDiv gn_pd;  // rows per sample
  int gn_sl;      // split-K reducer: slab lanes of splitk_reduce_n8_kernel for the same launch (same summation order)
};

// the epilogue arguments of problem p of a grouped launch (C / sum read from the kernel-argument segment)
__device__ __forceinline__ void group_epi(EpiArgs& e, void* C, float* sum, int p) {
  e.C = C;
  e.sum_out = sum;
  e.ws += (long long)p * e.ws_gstride;
}

// what a launch site returns: the launch's own status is consumed, the caller sees the runtime's last error
inline hipError_t launched(hipError_t) { return hipGetLastError(); }

// gemm_staged.hip: the register-staged kernel of (a_mode, b_mode); reductions and GroupNorm statistics from a / e
hipError_t launch_staged(int a_mode, int b_mode, const Args& a, const EpiArgs& e, dim3 grid, hipStream_t s);
// gemm_dma_{rowmajor,conv,colmajor}.hip: LDS-DMA variant v (gemm_variants.h) with column tile tbn for A mode AM
template <int AM>
hipError_t launch_dma_mode(int b_mode, const Args& a, const EpiArgs& e, dim3 grid, hipStream_t s, int v, int tbn);
// gemm_reduce.hip: sum the split-K slabs of G problems and apply the epilogue
hipError_t launch_reduce(const EpiArgs& red, hipStream_t s, int G);

}  // namespace sdmi_gemm_impl

