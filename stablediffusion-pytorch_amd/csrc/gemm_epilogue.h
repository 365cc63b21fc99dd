// The epilogue shared by the GEMM kernels and the split-K reducers: per-element and 8-column stores (Epi), the
// GroupNorm-backward statistics form, and the LDS-staged tile epilogue of the kernels (gemm_epilogue).
#pragma once
#include "gemm_args.h"

namespace sdmi_gemm_impl {

__device__ __forceinline__ long long rb_row(const EpiArgs& g, int row) {
  long long r = g.pix_d.div((unsigned)row);
  return g.rb_mod > 0 ? r % g.rb_mod : r;
}

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
constexpr int CPOL_SC1 = 16;  // buffer cache policy: device (agent) scope coherence

// activation of the epilogue: 1 SiLU, 2 ReLU, 3 ReLU gradient (v unless aux <= 0). A NaN passes both, as in torch's
// relu and threshold_backward: 2 gives NaN for a NaN v, 3 keeps v under a NaN aux.
__device__ __forceinline__ float act1(const EpiArgs& g, float v, long long orow, int col) {
  if (g.act == 1) return silu_f(v);
  if (g.act == 2) return v <= 0.f ? 0.f : v;
  if (g.act == 3) return bf2f(g.aux[orow * g.ld_aux + col]) <= 0.f ? 0.f : v;
  return v;
}

struct Epi {
  // reduction columns [col, col + nv) of one row (raw sums: no alpha / bias / activation)
  __device__ __forceinline__ static void extra(const EpiArgs& g, int row, int col, const float* v, int nv) {
    if (row >= g.m_store) return;
    for (int q = 0; q < nv; ++q) {
      const int j = col + q - g.n_x0;
      if (j == 0) {
        if (g.sum_out) g.sum_out[row] = v[q];
        if (g.sum_out2) g.sum_out2[row] = v[q];
      } else if (j >= 8 && j - 8 < g.ngrp && g.gsum) {
        g.gsum[(long long)(j - 8) * g.gsum_ld + row] = f2bf(v[q]);
      }
    }
  }

  // output row of GEMM row `row`: itself, or its pixel's place in the remap's output grid
  __device__ __forceinline__ static long long out_row(const EpiArgs& g, int row) {
    long long orow = row;
    if (g.remap) {
      const int b = (int)g.pix_d.div((unsigned)row);
      const int rr = row - b * g.pix_d.d();
      const int oy = (int)g.gw_d.div((unsigned)rr);
      const int ox = rr - oy * g.gw_d.d();
      orow = ((long long)b * g.r_oh + oy * g.r_sy + g.r_oy) * g.r_ow + ox * g.r_sx + g.r_ox;
    }
    return orow;
  }

  // one element's tail: v already holds alpha*acc + bias + bias2
  __device__ __forceinline__ static void finish(const EpiArgs& g, int row, int col, float v) {
    if (g.rowbias) v += bf2f(g.rowbias[rb_row(g, row) * g.rb_ld + col]);
    const long long orow = out_row(g, row);
    if (g.resid) v += bf2f(g.resid[orow * g.ldr + col]);
    v = act1(g, v, orow, col);
    long long ocol = col;
    if (g.perm) {
      int tap = (int)__umulhi((unsigned)col, g.p_magic);
      int c = col - tap * g.p_cin;
      if (c >= g.p_cvalid) return;
      ocol = g.perm == 2 ? (long long)tap * g.p_cvalid + c : (long long)c * g.p_taps + tap;
    }
    if (g.c_f32) ((float*)g.C)[orow * g.ldc + ocol] = v;
    else ((bf16_t*)g.C)[orow * g.ldc + ocol] = f2bf(v);
  }

  // v[0..8) += b[0..8) (16-B aligned fp32)
  __device__ __forceinline__ static void add8(float* v, const float* b) {
    const float4 b0 = *(const float4*)b, b1 = *(const float4*)(b + 4);
    v[0] += b0.x; v[1] += b0.y; v[2] += b0.z; v[3] += b0.w; v[4] += b1.x; v[5] += b1.y; v[6] += b1.z; v[7] += b1.w;
  }

  // 8 consecutive columns [col, col+8) of one row, acc values in v (alpha/bias not yet applied)
  __device__ __forceinline__ static void finish8(const EpiArgs& g, int row, int col, float* v) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] *= g.alpha;
    if (g.bias) add8(v, g.bias + col);
    if (g.bias2) add8(v, g.bias2 + col);
    if (g.rowbias) {
      float t[8];
      unpack8(*(const uint4*)(g.rowbias + rb_row(g, row) * g.rb_ld + col), t);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += t[e];
    }
    const long long orow = out_row(g, row);
    if (g.resid) {
      float t[8];
      unpack8(*(const uint4*)(g.resid + orow * g.ldr + col), t);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += t[e];
    }
    if (g.act == 1) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = silu_f(v[e]);
    } else if (g.act == 2) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = v[e] <= 0.f ? 0.f : v[e];
    } else if (g.act == 3) {
      float t[8];
      unpack8(*(const uint4*)(g.aux + orow * g.ld_aux + col), t);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = t[e] <= 0.f ? 0.f : v[e];
    }
    if (g.c_f32) {
      float* d = (float*)g.C + orow * g.ldc + col;
      *(float4*)d = make_float4(v[0], v[1], v[2], v[3]);
      *(float4*)(d + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
      *(uint4*)((bf16_t*)g.C + orow * g.ldc + col) = pack8(v);
    }
  }

  // one summed element of the split-K reducers: reduction column, or guards + bias + the tail
  __device__ __forceinline__ static void store_final(const EpiArgs& g, int row, int col, float acc) {
    if (g.n_x0 && col >= g.n_x0) {
      extra(g, row, col, &acc, 1);
      return;
    }
    if (row >= g.m_store || col >= g.n_store) return;
    float v = g.alpha * acc;
    if (g.bias) v += g.bias[col];
    if (g.bias2) v += g.bias2[col];
    finish(g, row, col, v);
  }
};

// dz and dz * xhat of one 8-column chunk of one output row (GroupNorm backward, EpiArgs::gn_part): v = the stored bf16
// dy values, x the GroupNorm input there, tb the forward table {a, s, mean, rstd} of the chunk's columns
__device__ __forceinline__ void gn_accum(const EpiArgs& e, const float* v, const uint4 xr, const float4* tb, float* u,
                                         float* w) {
  float xv[8];
  unpack8(xr, xv);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    float dz = v[q];
    if (e.gn_silu) dz *= silu_grad_f(fmaf(xv[q], tb[q].x, tb[q].y));
    u[q] += dz;
    w[q] = fmaf(dz, (xv[q] - tb[q].z) * tb[q].w, w[q]);
  }
}

// The GroupNorm-backward statistics epilogue of one staged 64-row half (m0h = its first row): thread t owns column
// chunk t % CH of rows t / CH + R k (R = NTH / CH row lanes); per gn_rb-row segment it stores bf16(alpha acc) with
// 16-B stores, accumulates dz / dz * xhat over its rows, and the R row lanes are summed in a fixed order through LDS
// (red: R x TBN x 2 floats) into the segment's column partials -- deterministic, no atomics.
template <int TBN, int NTH>
__device__ __forceinline__ void epi_gn_half(const EpiArgs& e, const float* st, float* red, int m0h, int n0) {
  constexpr int SROW = TBN + 4, CH = TBN / 8, R = NTH / CH;
  const int t = threadIdx.x, c8 = t % CH, rl0 = t / CH;
  const int col = n0 + c8 * 8;
  const bool on = rl0 < R && col < e.N;
#pragma unroll 1
  for (int s0 = 0; s0 < 64 && m0h + s0 < e.M; s0 += e.gn_rb) {
    float u[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, w[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (on) {
      const int b = (int)e.gn_pd.div((unsigned)(m0h + s0));  // a segment lies inside one sample (gn_rb | gn_P)
      float4 tb[8];
      const float4* tp = e.gn_tab + (long long)b * e.N + col;
#pragma unroll
      for (int q = 0; q < 8; ++q) tb[q] = tp[q];
      // every x row of this thread's share of the segment is loaded up front (one memory round trip per segment
      // instead of one per row); the rows are then consumed in the same order as before
      constexpr int MR = (64 + R - 1) / R;
      uint4 xr[MR];
#pragma unroll
      for (int k = 0; k < MR; ++k) {
        const int rl = s0 + rl0 + k * R, row = m0h + rl;
        if (rl < s0 + e.gn_rb && row < e.M) xr[k] = *(const uint4*)(e.gn_x + (long long)row * e.gn_ldx + col);
      }
#pragma unroll
      for (int k = 0; k < MR; ++k) {
        const int rl = s0 + rl0 + k * R, row = m0h + rl;
        if (rl >= s0 + e.gn_rb || row >= e.M) break;
        const float4 lo = *(const float4*)(st + rl * SROW + c8 * 8), hi = *(const float4*)(st + rl * SROW + c8 * 8 + 4);
        float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] *= e.alpha;
        const uint4 pk = pack8(v);
        *(uint4*)((bf16_t*)e.C + (long long)row * e.ldc + col) = pk;
        unpack8(pk, v);  // the statistics are of the stored bf16 dy, as the apply pass reads it
        gn_accum(e, v, xr[k], tb, u, w);
      }
    }
    if (rl0 < R) {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        red[(rl0 * TBN + c8 * 8 + q) * 2] = u[q];
        red[(rl0 * TBN + c8 * 8 + q) * 2 + 1] = w[q];
      }
    }
    __syncthreads();
    const long long seg = (m0h + s0) / e.gn_rb;
#pragma unroll 1
    for (int j = t; j < TBN; j += NTH) {
      if (n0 + j >= e.N) continue;
      float a1 = 0.f, a2 = 0.f;
#pragma unroll 1
      for (int r = 0; r < R; ++r) {
        a1 += red[(r * TBN + j) * 2];
        a2 += red[(r * TBN + j) * 2 + 1];
      }
      *(float2*)(e.gn_part + (seg * e.N + n0 + j) * 2) = make_float2(a1, a2);
    }
    __syncthreads();
  }
}

// Shared epilogue of the GEMM kernels: acc = this wave's 64 x (NJ*16) sub-tile (4 x NJ MFMA tiles) at (wm, wn) of a
// TBM x TBN workgroup tile computed by NT threads; smem >= 64 x (TBN + 4) fp32 of LDS that no wave reads any more (the
// caller synchronises before). GNE: the GroupNorm-statistics form (EpiArgs::gn_part, unsplit launches only) -- a
// separate instantiation, so the plain epilogue's code and registers stay those of a kernel without it (measured: the
// runtime-branch form slowed every GEMM of the step, 14.15-14.24 vs 13.90-13.94 ms/step with no statistics in use).
template <int TBN = BN, bool XCOL = false, int TBM = BM, int NJ = TBN / 32, int NTH = NT, bool GNE = false>
__device__ __forceinline__ void gemm_epilogue(const EpiArgs& e, f32x4 (&acc)[4][NJ], char* smem, int m0, int n0,
                                              int wm, int wn, int lane, int z) {
  // Stage the fp32 tile through LDS in 64-row parts; each thread then owns runs of 8 consecutive columns of one
  // row: 16-B stores (8 bf16 or 2 x 4 fp32) on the aligned paths, and a ROLLED per-element loop on the rare general
  // path (column permutes of weight gradients, unaligned outputs) instead of 4 x NJ x 4 unrolled scattered stores,
  // whose code and register footprint pushed the 192-column tile's accumulators to scratch.
  float* st = (float*)smem;      // [64][SROW] fp32, 33 KB (TBN 128) / 49 KB (TBN 192) / 97 KB (TBN 384)
  constexpr int SROW = TBN + 4;  // +4 floats: lanes of one ds_write hit distinct banks
  static_assert((64 * TBN / 8) % NTH == 0, "epilogue chunks per thread");
#pragma unroll
  for (int half = 0; half < TBM / 64; ++half) {
    if (wm == half * 64) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int cl = wn + 16 * j + (lane & 15);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) st[(16 * i + 4 * (lane >> 4) + r) * SROW + cl] = acc[i][j][r];
      }
    }
    __syncthreads();
    if constexpr (GNE) {  // GroupNorm statistics (plain bf16 epilogue, checked on the host)
      epi_gn_half<TBN, NTH>(e, st, st + 64 * SROW, m0 + half * 64, n0);
      continue;
    }
#pragma unroll 1
    for (int it = 0; it < 64 * TBN / 8 / NTH; ++it) {  // 64 rows x TBN/8 chunks of 8 columns
      const int ch = threadIdx.x + it * NTH;
      const int rl = ch / (TBN / 8), c8 = (ch - rl * (TBN / 8)) * 8;
      const int row = m0 + half * 64 + rl, col = n0 + c8;
      float v[8];
      const float4 lo = *(const float4*)(st + rl * SROW + c8), hi = *(const float4*)(st + rl * SROW + c8 + 4);
      v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
      if (XCOL && col >= e.n_gemm) continue;  // beyond the produced columns (tile padding)
      if (e.raw) {
        // only produced columns: with VALU row sums the slab column n_x0 = n_gemm belongs to those sums
        if (row >= e.M || col >= e.n_gemm) continue;
        // split-K slab, device-coherent (sc1) stores: the tile's last split may run on another XCD
        const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)e.ws, (short)0, 0x7fffffff, 0x00020000);
        const int off = (int)(((long long)z * e.split_stride + (long long)row * e.N + col) * 4);
        if (e.n8) {
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, lo), rw, off, 0, CPOL_SC1);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, hi), rw, off + 16, 0, CPOL_SC1);
        } else {
#pragma unroll 1
          for (int q = 0; q < 8 && col + q < e.N; ++q)
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[q]), rw, off + 4 * q, 0, CPOL_SC1);
        }
      } else if (XCOL && e.n_x0 && col >= e.n_x0) {
        if (row < e.M) Epi::extra(e, row, col, v, 8);
      } else if (e.vec) {
        if (row < e.m_store && col < e.n_store) Epi::finish8(e, row, col, v);
      } else if (row < e.m_store) {
#pragma unroll 1
        for (int q = 0; q < 8 && col + q < e.n_store; ++q) {
          float b = 0.f;
          if (e.bias) b += e.bias[col + q];
          if (e.bias2) b += e.bias2[col + q];
          Epi::finish(e, row, col + q, e.alpha * v[q] + b);
        }
      }
    }
    __syncthreads();
  }
}

}  // namespace sdmi_gemm_impl
