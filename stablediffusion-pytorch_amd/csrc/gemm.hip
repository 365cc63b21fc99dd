// MFMA bf16 GEMM family for gfx950 with implicit-GEMM convolution gathers.
//
// One kernel template covers every contraction of the denoiser step (reference aten calls:
// nn.Conv2d models/blocks.py:48-53,67-72,102-109; nn.ConvTranspose2d blocks.py:457-459;
// nn.Linear blocks.py:58-61,97 and MHA in/out projections blocks.py:83,94) in forward and
// backward:
//   conv fwd / dgrad : A = im2col(NHWC activation) [m=pixel][k=(tap,cin)],  B = packed weight [n][k]
//   conv wgrad       : A = dY^T (col-major),                               B = im2col(X) [k=pixel][n=(tap,cin)]
//   linear fwd/dgrad/wgrad : plain row/col-major operands.
//
// Split-K (for the small-grid weight-gradient and deep low-resolution GEMMs) writes fp32 slabs that
// a second kernel reduces while applying the same epilogue.
//
// This file is the host side: argument marshalling, split-K planning, the launch and the C ABI. The rest:
//   gemm_args.h      kernel argument structs, tile constants, the launch functions of the sources below
//   gemm_variants.h  the table of mainloop variants and the rules choosing variant and column tile
//   gemm_device.h    gathers, swizzled LDS images and fragment readers, tile order
//   gemm_epilogue.h  the shared epilogue
//   gemm_staged.hip  the register-staged kernel (variant 0)
//   gemm_dma.h       the LDS-DMA kernel, instantiated per A mode by gemm_dma_{rowmajor,conv,colmajor}.hip
//   gemm_reduce.hip  the split-K reducers
#include <string.h>

#include <algorithm>

#include "gemm_variants.h"

using namespace sdmi_gemm_impl;

namespace {

#ifdef SDMI_GEMM_TRACE
// probe build only (scripts/gemm_phase_probe.py): the phase-timestamp buffer every launch carries in Args::trace,
// allocated (zeroed) on first use and kept for the life of the library
constexpr size_t TRACE_WORDS = 1 << 20;
unsigned long long* trace_buffer() {
  static unsigned long long* buf = [] {
    void* p = nullptr;
    if (hipMalloc(&p, TRACE_WORDS * 8) != hipSuccess || hipMemset(p, 0, TRACE_WORDS * 8) != hipSuccess) p = nullptr;
    return (unsigned long long*)p;
  }();
  return buf;
}
#endif

// slab row width with split-K: the produced columns, plus one 8-column chunk carrying the VALU row sums
int slab_n(const sdmi_gemm_desc* d) { return n_total(d) + ((has_reductions(d) && !d->gsum_out) ? 8 : 0); }

int fill_args(const sdmi_gemm_desc* d, Args& a, EpiArgs& e) {
  if (!d || d->m <= 0 || d->n <= 0 || d->k <= 0) return -1;
  // K is the contiguous (16-B chunked) dimension of row-major / conv A and of [n][k] B only
  if ((d->a_mode != SDMI_A_COLMAJOR || d->b_mode == SDMI_B_NK) && (d->k % 8)) return -2;
  if ((d->a_mode == SDMI_A_COLMAJOR) && (d->m % 8)) return -3;
  if ((d->b_mode != SDMI_B_NK) && (d->n % 8)) return -4;
  if (d->a_mode == SDMI_A_CONV || d->b_mode == SDMI_B_KN_CONV) {
    const sdmi_conv_geom& q = d->geom;
    if (q.cin <= 0 || q.cin % 8 || q.kw <= 0 || q.ldx % 8) return -5;
  }
  if (d->a2 && (d->k_split % 8 || d->lda2 % 8)) return -7;
  memset(&a, 0, sizeof(a));
  memset(&e, 0, sizeof(e));
  a.M = d->m; a.N = d->n; a.K = d->k;
  a.A = (const bf16_t*)d->a; a.lda = d->lda;
  a.B = (const bf16_t*)d->b; a.ldb = d->ldb;
  a.ih = d->geom.ih; a.iw = d->geom.iw; a.cin = d->geom.cin; a.ldx = d->geom.ldx; a.kw = d->geom.kw;
  if ((d->a_mode == SDMI_A_CONV || d->b_mode == SDMI_B_KN_CONV) && (d->geom.oh <= 0 || d->geom.ow <= 0)) return -5;
  a.ohw_d = FastDiv::make(std::max(1, d->geom.oh * d->geom.ow));
  a.ow_d = FastDiv::make(std::max(1, d->geom.ow));
  a.sy = d->geom.sy; a.sx = d->geom.sx; a.oy0 = d->geom.oy0; a.ox0 = d->geom.ox0;
  if (d->b_mode == SDMI_B_KN_CONV) {
    const int ohw = d->geom.oh * d->geom.ow, ow = d->geom.ow;
    for (int sh = 0; sh < 2; ++sh) {  // KBK 64, then 32
      const int kb = sh ? 32 : 64;
      const int f = (ohw % kb == 0 && kb % ow == 0) ? 1 : (kb % ohw == 0 ? 2 : 0);
      a.bfast |= f << (2 * sh);
    }
  }
  a.A2 = (const bf16_t*)d->a2; a.lda2 = d->lda2;
  a.k_split = (d->a_mode == SDMI_A_CONV && d->a2) ? d->k_split : d->k;
  e.M = d->m; e.N = d->n;
  e.n_gemm = n_total(d);
  e.C = d->c; e.ldc = d->ldc; e.c_f32 = d->c_f32;
  e.bias = d->bias; e.bias2 = d->bias2;
  e.rowbias = (const bf16_t*)d->rowbias; e.rb_ld = d->rb_ld;
  e.resid = (const bf16_t*)d->resid; e.ldr = d->ldr;
  e.alpha = d->alpha; e.act = d->act;
  e.remap = d->remap; e.r_oh = d->r_oh; e.r_ow = d->r_ow;
  if (d->remap && (d->r_gh <= 0 || d->r_gw <= 0)) return -11;
  if (d->remap && d->rowbias && std::max(1, d->rb_div) != d->r_gh * d->r_gw) return -12;
  e.pix_d = FastDiv::make(d->remap ? d->r_gh * d->r_gw : std::max(1, d->rb_div));
  e.gw_d = FastDiv::make(d->remap ? d->r_gw : 1);
  e.r_sy = d->r_sy; e.r_sx = d->r_sx; e.r_oy = d->r_oy; e.r_ox = d->r_ox;
  e.perm = d->perm; e.p_cin = d->p_cin; e.p_taps = d->p_taps;
  if (d->perm && (d->p_cin < 8 || d->p_cin % 8)) return -10;
  e.p_magic = d->perm ? (unsigned)(((1ULL << 32) + d->p_cin - 1) / d->p_cin) : 0u;
  {  // multiply-high division by N/8 is exact for idx < 2^32 / (N/8), i.e. when M * (N/8)^2 < 2^32
    const unsigned long long n8 = (unsigned long long)(d->n >> 3);
    e.n8_magic = (n8 > 1 && (unsigned long long)d->m * n8 * n8 < (1ULL << 32)) ? (unsigned)(((1ULL << 32) + n8 - 1) / n8)
                                                                               : 0u;
  }
  e.p_cvalid = d->p_cvalid > 0 ? d->p_cvalid : d->p_cin;
  e.m_store = d->m_store > 0 ? d->m_store : d->m;
  e.n_store = d->n_store > 0 ? d->n_store : d->n;
  e.n8 = d->n % 8 == 0;
  e.rb_mod = d->rb_mod;
  e.aux = (const bf16_t*)d->aux; e.ld_aux = d->ld_aux;
  if (has_reductions(d)) {
    if (d->a_mode != SDMI_A_COLMAJOR || d->b_mode == SDMI_B_NK) return -13;
    if (d->gsum_out && (d->sum_group <= 0 || d->gsum_ld <= 0)) return -14;
    if (d->gsum_out) {
      a.n_x0 = e.n_x0 = (d->n + 7) / 8 * 8;
      a.grp_d = FastDiv::make(std::max(1, d->sum_group));
    } else {
      a.rowsum = 1;
      e.n_x0 = d->n;  // slab chunk of the row sums (split-K); never produced by the MFMA tiles
    }
    e.ngrp = reduction_groups(d);
    e.gsum_ld = d->gsum_ld;
    e.sum_out = d->sum_out;
    e.sum_out2 = d->sum_out2;
    e.gsum = (bf16_t*)d->gsum_out;
    e.N = slab_n(d);  // split-K slabs cover the reduction columns too
    const unsigned long long n8 = (unsigned long long)(e.N >> 3);
    e.n8_magic = (n8 > 1 && (unsigned long long)d->m * n8 * n8 < (1ULL << 32)) ? (unsigned)(((1ULL << 32) + n8 - 1) / n8)
                                                                              : 0u;
  }
  if (d->act == 3 && !d->aux) return -8;
  if (d->act < 0 || d->act > 3) return -9;
  e.vec = !d->perm && d->n % 8 == 0 && e.n_store % 8 == 0 && d->ldc % 8 == 0 &&
          (!d->resid || d->ldr % 8 == 0) && (!d->rowbias || d->rb_ld % 8 == 0) &&
          ((uintptr_t)d->c % 16 == 0) && (!d->bias || (uintptr_t)d->bias % 16 == 0) &&
          (!d->bias2 || (uintptr_t)d->bias2 % 16 == 0) && (!d->resid || (uintptr_t)d->resid % 16 == 0) &&
          (!d->rowbias || (uintptr_t)d->rowbias % 16 == 0) &&
          (d->act != 3 || (d->ld_aux % 8 == 0 && (uintptr_t)d->aux % 16 == 0));
  if (d->gn_part) {  // GroupNorm-backward statistics: plain bf16 epilogue, whole segments inside one sample
    if (!d->gn_x || !d->gn_tab || d->gn_P <= 0 || d->m % d->gn_P || (d->gn_rb != 16 && d->gn_rb != 32 && d->gn_rb != 64) ||
        d->gn_P % d->gn_rb || d->gn_P >= (1 << 24))
      return -20;
    if (d->bias || d->bias2 || d->rowbias || d->resid || d->act || d->remap || d->perm || has_reductions(d) || d->c_f32 ||
        !e.vec || e.m_store != d->m || e.n_store != d->n || (uintptr_t)d->gn_part % 8 || d->gn_ldx % 8 ||
        (uintptr_t)d->gn_x % 16 || (uintptr_t)d->gn_tab % 16)
      return -21;
    e.gn_x = (const bf16_t*)d->gn_x;
    e.gn_ldx = d->gn_ldx;
    e.gn_tab = (const float4*)d->gn_tab;
    e.gn_part = d->gn_part;
    e.gn_rb = d->gn_rb;
    e.gn_silu = d->gn_silu;
    e.gn_pd = FastDiv::make(d->gn_P);
  }
  return 0;
}

// split-K slices: the measured per-shape count (splits_hint, sdmi/tuned_gemm.json) where there is one, else a shallow
// default (>= 8 k-tiles per slice, at most 16 slices, until the grid has 384 tiles)
int plan_splits(const sdmi_gemm_desc* d) {
  const int v = pick_variant(d), tbn = pick_tbn(d, v), tbm = tile_m(v);
  const long long tiles = (long long)((d->m + tbm - 1) / tbm) * ((n_grid(d, v) + tbn - 1) / tbn);
  const int nkt = (d->k + BK - 1) / BK;
  if (d->splits_hint > 0) {
    int s = std::min(d->splits_hint, nkt);
    while (s > 1 && (long long)s * d->m * slab_n(d) * 4 >= (1LL << 31)) s >>= 1;
    return std::max(s, 1);
  }
  int s = 1;
  while (tiles * s < 384 && nkt / (s * 2) >= 8 && s < 16) s *= 2;
  return s;
}

}  // namespace

// which mainloop / column-tile width a launch of this descriptor uses (variant: 0 register-staged, 2 .. 5 the LDS-DMA
// rings of gemm_variant(); tile_n: 64 .. 384) -- for profiling / roofline attribution
extern "C" int sdmi_gemm_kernel_info(const sdmi_gemm_desc* d, int* variant, int* tile_n) {
  if (!d) return -1;
  const int v = pick_variant(d);
  if (variant) *variant = v;
  if (tile_n) *tile_n = pick_tbn(d, v);
  return 0;
}

extern "C" int sdmi_gemm_plan(const sdmi_gemm_desc* d, int* splits, size_t* ws) {
  Args a;
  EpiArgs e;
  int rc = fill_args(d, a, e);
  if (rc) return rc;
  int s = plan_splits(d);
  if (splits) *splits = s;
  if (ws) *ws = s > 1 ? (size_t)s * d->m * slab_n(d) * sizeof(float) : 0;
  return 0;
}

namespace {
// descriptors that may share one grouped launch: identical in every field but the operand / output pointers
bool same_problem_shape(const sdmi_gemm_desc* a, const sdmi_gemm_desc* b) {
  sdmi_gemm_desc x = *a, y = *b;
  x.a = y.a = nullptr;
  x.b = y.b = nullptr;
  x.c = y.c = nullptr;
  x.sum_out = y.sum_out = nullptr;
  return memcmp(&x, &y, sizeof(x)) == 0;
}

// split count of a launch carrying G problems: the single problem's (tuned / heuristic) count shared out over them
int group_splits(const sdmi_gemm_desc* d, int G) {
  const int s = plan_splits(d);
  return G > 1 ? std::max(1, (s + G / 2) / G) : s;
}

int run_gemm(const sdmi_gemm_desc* d, int G, void* workspace, size_t ws_bytes, hipStream_t s) {
  Args a;
  EpiArgs e;
  int rc = fill_args(&d[0], a, e);
  if (rc) return rc;
  if (G < 1 || G > SDMI_GEMM_GROUP_MAX) return -15;
  if (G > 1) {
    // grouped: plain / bias-summing GEMMs only (no second A source, no per-row / residual / auxiliary inputs)
    if (d[0].a2 || d[0].resid || d[0].rowbias || d[0].aux || d[0].bias || d[0].bias2 || d[0].sum_out2 || d[0].gsum_out)
      return -16;
    for (int i = 1; i < G; ++i)
      if (!same_problem_shape(&d[0], &d[i]) || (!d[i].sum_out) != (!d[0].sum_out)) return -17;
  }
  a.ngroups = G;
  for (int i = 0; i < G; ++i) {
    a.Ag[i] = (const bf16_t*)d[i].a;
    a.Bg[i] = (const bf16_t*)d[i].b;
    a.Cg[i] = e.Cg[i] = d[i].c;
    a.sum_g[i] = e.sum_g[i] = d[i].sum_out;
  }
  int splits = group_splits(d, G);
  const int nt = n_total(d), ns = slab_n(d);
  const long long slab = (long long)d->m * ns;  // floats per split slab of one problem
  if (splits > 1 && (!workspace || ws_bytes < (size_t)G * splits * slab * sizeof(float))) splits = 1;
  if ((long long)G * splits * slab * 4 >= (1LL << 31)) splits = 1;  // slab offsets are 32-bit
  int nkt = (d->k + BK - 1) / BK;
  a.ktiles_per_split = (nkt + splits - 1) / splits;
  splits = (nkt + a.ktiles_per_split - 1) / a.ktiles_per_split;
  a.nsplit = splits;
  EpiArgs run = e;
  const int variant = pick_variant(d), tbn = pick_tbn(d, variant), tbm = tile_m(variant);
  const int ng = n_grid(d, variant);
  dim3 grid((ng + tbn - 1) / tbn, (d->m + tbm - 1) / tbm, splits * G);
  if (splits > 1) {
    run.raw = 1;
    run.ws = (const float*)workspace;
    run.nsplit = splits;
    run.split_stride = slab;
    run.ws_gstride = (long long)splits * slab;
  }
  const int am = d->a_mode, bm = d->b_mode;
  switch (am * 3 + bm) {  // the mode pairs that have kernels
    case SDMI_A_ROWMAJOR * 3 + SDMI_B_NK:
    case SDMI_A_ROWMAJOR * 3 + SDMI_B_KN:
    case SDMI_A_CONV * 3 + SDMI_B_NK:
    case SDMI_A_COLMAJOR * 3 + SDMI_B_KN:
    case SDMI_A_COLMAJOR * 3 + SDMI_B_KN_CONV: break;
    default: return -6;
  }
#ifdef SDMI_GEMM_TRACE
  if (!(a.trace = trace_buffer())) return -18;
#endif
  hipError_t err;
  if (variant == 0) err = launch_staged(am, bm, a, run, grid, s);
  else if (am == SDMI_A_ROWMAJOR) err = launch_dma_mode<SDMI_A_ROWMAJOR>(bm, a, run, grid, s, variant, tbn);
  else if (am == SDMI_A_CONV) err = launch_dma_mode<SDMI_A_CONV>(bm, a, run, grid, s, variant, tbn);
  else err = launch_dma_mode<SDMI_A_COLMAJOR>(bm, a, run, grid, s, variant, tbn);
  if (err != hipSuccess) return (int)err;
  if (splits > 1) {
    EpiArgs red = e;
    red.raw = 0;
    red.nsplit = splits;
    red.split_stride = slab;
    red.ws_gstride = (long long)splits * slab;
    red.ws = (const float*)workspace;
    err = launch_reduce(red, s, G);
    if (err != hipSuccess) return (int)err;
  }
  return 0;
}
}  // namespace

extern "C" int sdmi_gemm(const sdmi_gemm_desc* d, void* workspace, size_t ws_bytes, sdmi_stream_t stream) {
  if (!d) return -1;
  return run_gemm(d, 1, workspace, ws_bytes, (hipStream_t)stream);
}

extern "C" int sdmi_gemm_grouped_plan(const sdmi_gemm_desc* d, int ngroups, int* splits, size_t* ws) {
  if (!d || ngroups < 1 || ngroups > SDMI_GEMM_GROUP_MAX) return -1;
  Args a;
  EpiArgs e;
  int rc = fill_args(d, a, e);
  if (rc) return rc;
  for (int i = 1; i < ngroups; ++i)
    if (!same_problem_shape(&d[0], &d[i])) return -17;
  const int sp = group_splits(d, ngroups);
  if (splits) *splits = sp;
  if (ws) *ws = sp > 1 ? (size_t)ngroups * sp * d->m * slab_n(d) * sizeof(float) : 0;
  return 0;
}

extern "C" int sdmi_gemm_grouped(const sdmi_gemm_desc* d, int ngroups, void* workspace, size_t ws_bytes,
                                 sdmi_stream_t stream) {
  if (!d) return -1;
  return run_gemm(d, ngroups, workspace, ws_bytes, (hipStream_t)stream);
}

#ifdef SDMI_GEMM_TRACE
// probe build only: clear the phase-timestamp buffer; copy its first n_u64 words to host memory (device synchronised)
extern "C" int sdmi_gemm_trace_clear(void) {
  void* p = trace_buffer();
  if (!p) return -1;
  return hipMemset(p, 0, TRACE_WORDS * 8) == hipSuccess ? 0 : -2;
}

extern "C" int sdmi_gemm_trace_copy(void* host_dst, long long n_u64) {
  if (!host_dst || n_u64 < 0 || n_u64 > (long long)TRACE_WORDS) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -2;
  void* p = trace_buffer();
  return p && hipMemcpy(host_dst, p, (size_t)n_u64 * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -3;
}
#endif
