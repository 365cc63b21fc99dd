// ADC/DAC-aware compute-in-memory layers of the reference (cim_layers/layers_qn_lsq_adda_cim.py, layers_utils_adda.py)
// for gfx950: the input's integer codes go to the arrays in L = ceil((input_bit - 1) / sb) sign-magnitude slices of
// sb = dac_bit - 1 bits, the weight is mapped onto arrays of `rb` rows, and every (row block j, slice i) partial sum is
// read through an ADC -- scaled, clamped to [-R-1, R], R = 2^(adc_bit-1) - 1, and rounded -- before the sums are added:
//
//     x_q      = fl(fl(q se) / se), q the input's LSQ code (lsq_device.h): the reference's q * se / se.detach(), which in
//                fp32 is not always q; slice i = sign(x_q) (floor(|x_q| / 2^(i sb)) - 2^sb floor(|x_q| / 2^min((i+1) sb, ib-1)))
//     P_ij     = X_i[:, block j] @ W2[block j, :]          bf16 MFMA, fp32 accumulator: exact for integer codes
//     A        = fl(as P),  as = *adc_scale;  with ADC noise  n = fl(fl(A fl(1 + gain[c])) + fl(R offset[c])),
//                A <- fl(fl(n - A) + A)
//     inside   = -R-1 <= A <= R (a NaN is outside),  C = clamp(A) (a NaN passes),  Q = fl(fl(rint(C) - C) + C)
//     Z        = sum_j sum_i 2^(i sb) Q_ij,   T = sum_j sum_i (inside ? 2^(i sb) P_ij : 0)   in that order, fp32
//     pre      = fl(fl(fl(fl(Z / ws) / is) / as) + bias[c]),  ws = fl(1 / *step_w), is = fl(1 / *step_in) (raw steps)
//     mask     bit j L + i of word (j L + i) / 32 of an element = inside_ij
//
// Layouts. K is cut into nb = ceil(K / rb) row blocks, each padded with zeros to rbp = 32 ceil(rb / 32) columns, so a
// block starts on a k tile and its last tile is part zero: Kp = nb rbp. Slices: bf16 [L][Mp][Kp], Mp = 64 ceil(M / 64),
// pad rows zero. Weight: bf16 [Np][Kp], Np = 64 ceil(N / 64), row n = column n of W2; with weight noise the fp32 value is
// split into hi = bf16(w) and lo = bf16(w - hi) and both are multiplied against the same slice fragment. The padding
// makes every 16-byte tile load in bounds without a test.
//
// adda_gemm_kernel: 256 threads (4 waves, 2 x 2), a 64 x 64 output tile per workgroup, a 32 x 32 quarter per wave as
// 2 x 2 mfma_f32_16x16x32_bf16 tiles; k tile 32: thread t stages 16 bytes of row t / 4 of each operand into LDS
// (64 x 32 bf16 = 4 KiB per operand, 8 or 12 KiB in all) after loading the next tile's 16 bytes into registers. Per
// (j, i) the P accumulator is read through the ADC in registers and added into the Z accumulator; nothing but pre (and
// mask / T when the backward will run) leaves the workgroup.
//
// The backward's operands (adda_bwd_ops_kernel), from d_pre (bf16) and the mask words:
//     dZ   = fl(fl(fl(d_pre / as) / is) / ws)
//     U_j  = bf16(fl(dZ cnt_j)),  cnt_j = the number of slices of block j with inside     [nb][M][ld]
//     V_ji = bf16(inside_ij ? fl(dZ 2^(i sb)) : 0)                                         [nb][L Mp][ld], pad rows zero
//     d as = fl(S1 - fl(S2 / as)),  S1 = sum fl(dZ T),  S2 = sum fl(d_pre fl(pre - bias))  (partials as in lsq.hip)
// so that, per row block, d x_q = (as / L) U_j @ W2[block j]^T and d W2[block j] = as [X_0; X_1; ...]^T @ V_j are one
// plain data-gradient and one plain weight-gradient GEMM (the slices are already stacked along M).
// Steps and the ADC scale are read from device memory; no launch argument depends on a parameter's value; no atomics.
#include "lsq_device.h"
#include "../../include/sdmi.h"

namespace {

constexpr int AD_T = 64, AD_BK = 32, AD_NT = 256;

inline int r_up(int v, int m) { return (v + m - 1) / m * m; }

struct Geo {
  int M, N, K, rb, rbp, nb, L, sb, ib, Mp, Np, Kp;
};

// false when the sizes are unusable
inline bool make_geo(Geo& g, int M, int N, int K, int rb, int input_bit, int dac_bit) {
  if (M <= 0 || N <= 0 || K <= 0 || rb <= 0 || input_bit < 2 || input_bit > 9 || dac_bit < 2 || dac_bit > 9) return false;
  g.M = M; g.N = N; g.K = K;
  g.rb = std::min(rb, K);
  g.rbp = r_up(g.rb, AD_BK);
  g.nb = (K + g.rb - 1) / g.rb;
  g.sb = dac_bit - 1;
  g.ib = input_bit;
  g.L = (input_bit - 1 + g.sb - 1) / g.sb;
  g.Mp = r_up(M, AD_T);
  g.Np = r_up(N, AD_T);
  const long long kp = (long long)g.nb * g.rbp;
  if (kp > 0x7fffffffLL || (long long)g.L * g.Mp * kp > 0x7fffffffLL || (long long)g.Np * kp > 0x7fffffffLL) return false;
  g.Kp = (int)kp;
  return true;
}

// padded column -> source channel, or -1 for a pad column
__device__ __forceinline__ int src_col(int pc, int rb, int rbp, int K) {
  const int j = pc / rbp, w = pc - j * rbp, c = j * rb + w;
  return (w < rb && c < K) ? c : -1;
}

// slice i of x_q = fl(fl(q se) / se), the reference's q * se / se.detach(): in fp32 that round trip can land one ulp
// beside the integer q, and the reference's floor() then cuts a whole code off. Followed bit for bit.
__device__ __forceinline__ float slice_of(float xq, int i, int sb, int ib) {
  if (xq != xq) return xq;
  const float a = fabsf(xq);
  const int hi = min((i + 1) * sb, ib - 1);
  const float v = floorf(a / (float)(1 << (i * sb))) - floorf(a / (float)(1 << hi)) * (float)(1 << sb);
  return xq < 0.f ? -v : v;
}

// x fp32 (B, C, P) -> slices [L][Mp][Kp]; item = group of 8 padded columns * Mp + row
__global__ __launch_bounds__(LQ_NT) void adda_in_fwd_kernel(const float* x, int B, int C, int P, Step st, float qp, Geo g,
                                                            bf16_t* out) {
  const float se = eff_step(st);
  const long long items = (long long)g.Mp * (g.Kp / 8);
  for (long long it = (long long)blockIdx.x * LQ_NT + threadIdx.x; it < items; it += (long long)gridDim.x * LQ_NT) {
    const int grp = (int)(it / g.Mp), m = (int)(it - (long long)grp * g.Mp);
    float q[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) q[k] = 0.f;
    if (m < g.M) {
      const long long b = m / P, p = m - b * P;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int c = src_col(grp * 8 + k, g.rb, g.rbp, C);
        if (c >= 0) q[k] = div_ieee(mul_ieee(quant(x[(b * C + c) * P + p], se, qp).q, se), se);
      }
    }
    for (int i = 0; i < g.L; ++i) {
      float f[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) f[k] = slice_of(q[k], i, g.sb, g.ib);
      *(uint4*)(out + ((long long)i * g.Mp + m) * g.Kp + grp * 8) = pack8(f);
    }
  }
}

// w fp32 [N][K] -> hi (and lo) bf16 [Np][Kp]
__global__ __launch_bounds__(LQ_NT) void adda_pack_w_kernel(const float* w, Geo g, bf16_t* hi, bf16_t* lo) {
  const long long items = (long long)g.Np * (g.Kp / 8);
  for (long long it = (long long)blockIdx.x * LQ_NT + threadIdx.x; it < items; it += (long long)gridDim.x * LQ_NT) {
    const int n = (int)(it / (g.Kp / 8)), grp = (int)(it - (long long)n * (g.Kp / 8));
    float h[8], l[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = n < g.N ? src_col(grp * 8 + k, g.rb, g.rbp, g.K) : -1;
      const float v = c >= 0 ? w[(long long)n * g.K + c] : 0.f;
      h[k] = v;
      l[k] = sub_ieee(v, bf2f(f2bf(v)));
    }
    *(uint4*)(hi + (long long)n * g.Kp + grp * 8) = pack8(h);
    if (lo) *(uint4*)(lo + (long long)n * g.Kp + grp * 8) = pack8(l);
  }
}

struct GemmArgs {
  const bf16_t *xs, *whi, *wlo;
  Geo g;
  float R;
  const float *as, *gn, *on, *sw, *sin, *bias;
  float* pre;
  int ld;
  unsigned* mask;
  float* T;
};

__device__ __forceinline__ s16x8 lds_frag(const bf16_t* tile, int row, int k) {
  return __builtin_bit_cast(s16x8, *(const uint4*)(tile + row * AD_BK + k));
}

template <bool LO>
__global__ __launch_bounds__(AD_NT) void adda_gemm_kernel(GemmArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t sA[AD_T * AD_BK];
  __shared__ __attribute__((aligned(16))) bf16_t sB[AD_T * AD_BK];
  __shared__ __attribute__((aligned(16))) bf16_t sB2[LO ? AD_T * AD_BK : 8];
  const Geo& g = a.g;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int m0 = blockIdx.y * AD_T, n0 = blockIdx.x * AD_T;
  const int lr = t >> 2, lc = (t & 3) * 8;      // staging: row and k offset of this thread's 16 bytes
  const int fr = lane & 15, fk = (lane >> 4) * 8;  // fragment: row (A) / column (B) and k offset
  const float as = *a.as, lo_edge = -a.R - 1.0f, hi_edge = a.R;
  float gfac[2], goff[2];
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    const int col = n0 + wn + 16 * tn + fr;
    const bool on = a.gn && col < g.N;
    gfac[tn] = on ? add_ieee(1.0f, a.gn[col]) : 1.0f;
    goff[tn] = on ? mul_ieee(a.R, a.on[col]) : 0.0f;
  }
  f32x4 Z[2][2], Tt[2][2];
  unsigned mk[2][2][4];
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      Z[tm][tn] = f32x4{0.f, 0.f, 0.f, 0.f};
      Tt[tm][tn] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 4; ++r) mk[tm][tn][r] = 0u;
    }
  int bit = 0, word = 0;
  auto flush = [&]() {
    if (a.mask) {
#pragma unroll
      for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = m0 + wm + 16 * tm + (lane >> 4) * 4 + r, col = n0 + wn + 16 * tn + fr;
            if (row < g.M && col < g.N) a.mask[((long long)word * g.M + row) * a.ld + col] = mk[tm][tn][r];
            mk[tm][tn][r] = 0u;
          }
    }
  };
  for (int j = 0; j < g.nb; ++j) {
    for (int i = 0; i < g.L; ++i) {
      f32x4 P[2][2];
#pragma unroll
      for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) P[tm][tn] = f32x4{0.f, 0.f, 0.f, 0.f};
      const bf16_t* xa = a.xs + ((long long)i * g.Mp + m0 + lr) * g.Kp + (long long)j * g.rbp + lc;
      const long long wofs = (long long)(n0 + lr) * g.Kp + (long long)j * g.rbp + lc;
      uint4 ra = *(const uint4*)xa, rw = *(const uint4*)(a.whi + wofs), rw2 = ra;
      if (LO) rw2 = *(const uint4*)(a.wlo + wofs);
      for (int kk = 0; kk < g.rbp; kk += AD_BK) {
        __syncthreads();  // the previous tile's fragment reads are done
        *(uint4*)(sA + lr * AD_BK + lc) = ra;
        *(uint4*)(sB + lr * AD_BK + lc) = rw;
        if (LO) *(uint4*)(sB2 + lr * AD_BK + lc) = rw2;
        __syncthreads();
        if (kk + AD_BK < g.rbp) {
          ra = *(const uint4*)(xa + kk + AD_BK);
          rw = *(const uint4*)(a.whi + wofs + kk + AD_BK);
          if (LO) rw2 = *(const uint4*)(a.wlo + wofs + kk + AD_BK);
        }
        s16x8 fa[2], fb[2], fb2[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          fa[u] = lds_frag(sA, wm + 16 * u + fr, fk);
          fb[u] = lds_frag(sB, wn + 16 * u + fr, fk);
          if (LO) fb2[u] = lds_frag(sB2, wn + 16 * u + fr, fk);
        }
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
          for (int tn = 0; tn < 2; ++tn) {
            P[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[tm], fb[tn], P[tm][tn], 0, 0, 0);
            if (LO) P[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[tm], fb2[tn], P[tm][tn], 0, 0, 0);
          }
      }
      // the ADC of this (block, slice), in registers
      const float pw = (float)(1 << (i * g.sb));
#pragma unroll
      for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float p = P[tm][tn][r];
            float A = mul_ieee(as, p);
            if (a.gn) {
              const float n = add_ieee(mul_ieee(A, gfac[tn]), goff[tn]);
              A = add_ieee(sub_ieee(n, A), A);
            }
            const bool inside = A >= lo_edge && A <= hi_edge;
            const float c = A < lo_edge ? lo_edge : (A > hi_edge ? hi_edge : A);
            const float q = add_ieee(sub_ieee(rintf(c), c), c);
            Z[tm][tn][r] = add_ieee(Z[tm][tn][r], mul_ieee(pw, q));
            Tt[tm][tn][r] = add_ieee(Tt[tm][tn][r], inside ? mul_ieee(pw, p) : 0.0f);
            mk[tm][tn][r] |= (inside ? 1u : 0u) << bit;
          }
      if (++bit == 32) {
        flush();
        bit = 0;
        ++word;
      }
    }
  }
  if (bit) flush();
  const float ws = a.sw ? div_ieee(1.0f, *a.sw) : 1.0f, is = a.sin ? div_ieee(1.0f, *a.sin) : 1.0f;
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm + 16 * tm + (lane >> 4) * 4 + r, col = n0 + wn + 16 * tn + fr;
        if (row < g.M && col < g.N) {
          float z = Z[tm][tn][r];
          if (a.sw) z = div_ieee(z, ws);
          if (a.sin) z = div_ieee(z, is);
          z = div_ieee(z, as);
          if (a.bias) z = add_ieee(z, a.bias[col]);
          a.pre[(long long)row * a.ld + col] = z;
          if (a.T) a.T[(long long)row * a.ld + col] = Tt[tm][tn][r];
        }
      }
}

struct OpsArgs {
  const bf16_t* dpre;
  int ld_d;
  const float* pre;
  int ld;
  const float *bias, *T;
  const unsigned* mask;
  int M, N, Mp, nb, L, sb;
  const float *as, *sw, *sin;
  bf16_t *U, *V;
  float* partial;  // [2][LQ_CAP]
};

// item = group of 8 columns * Mp + row
__global__ __launch_bounds__(LQ_NT) void adda_bwd_ops_kernel(OpsArgs a) {
  __shared__ float red1[LQ_WAVES], red2[LQ_WAVES];
  const float as = *a.as, ws = a.sw ? div_ieee(1.0f, *a.sw) : 1.0f, is = a.sin ? div_ieee(1.0f, *a.sin) : 1.0f;
  const long long items = (long long)a.Mp * (a.ld_d / 8);
  float acc1 = 0.f, acc2 = 0.f;
  for (long long it = (long long)blockIdx.x * LQ_NT + threadIdx.x; it < items; it += (long long)gridDim.x * LQ_NT) {
    const int grp = (int)(it / a.Mp), m = (int)(it - (long long)grp * a.Mp);
    const bool live = m < a.M;
    float dz[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) dz[k] = 0.f;
    if (live) {
      float d[8];
      unpack8(*(const uint4*)(a.dpre + (long long)m * a.ld_d + grp * 8), d);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int c = grp * 8 + k;
        if (c < a.N) {
          float z = div_ieee(d[k], as);
          if (a.sin) z = div_ieee(z, is);
          if (a.sw) z = div_ieee(z, ws);
          dz[k] = z;
          const long long e = (long long)m * a.ld + c;
          acc1 = add_ieee(acc1, mul_ieee(z, a.T[e]));
          acc2 = add_ieee(acc2, mul_ieee(d[k], a.bias ? sub_ieee(a.pre[e], a.bias[c]) : a.pre[e]));
        }
      }
    }
    int bitno = 0;
    for (int j = 0; j < a.nb; ++j) {
      int cnt[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) cnt[k] = 0;
      for (int i = 0; i < a.L; ++i, ++bitno) {
        const float pw = (float)(1 << (i * a.sb));
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int c = grp * 8 + k;
          unsigned b = 0u;
          if (live && c < a.N) b = (a.mask[((long long)(bitno >> 5) * a.M + m) * a.ld + c] >> (bitno & 31)) & 1u;
          cnt[k] += (int)b;
          v[k] = b ? mul_ieee(dz[k], pw) : 0.0f;
        }
        *(uint4*)(a.V + (((long long)j * a.L + i) * a.Mp + m) * a.ld_d + grp * 8) = pack8(v);
      }
      if (live) {
        float u[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) u[k] = mul_ieee(dz[k], (float)cnt[k]);
        *(uint4*)(a.U + ((long long)j * a.M + m) * a.ld_d + grp * 8) = pack8(u);
      }
    }
  }
  block_partial(acc1, red1, a.partial);
  block_partial(acc2, red2, a.partial + LQ_CAP);
}

__global__ __launch_bounds__(LQ_NT) void adda_scale_finish_kernel(const float* partial, int parts, const float* as,
                                                                  float* out) {
  __shared__ float red[2][LQ_WAVES];
  float v1 = (int)threadIdx.x < parts ? partial[threadIdx.x] : 0.f;
  float v2 = (int)threadIdx.x < parts ? partial[LQ_CAP + threadIdx.x] : 0.f;
  v1 = wave_sum(v1);
  v2 = wave_sum(v2);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = v1;
    red[1][threadIdx.x >> 6] = v2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float s1 = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    const float s2 = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    out[0] = sub_ieee(s1, div_ieee(s2, *as));
    out[1] = s1;
    out[2] = s2;
  }
}

// the input quantiser's backward on the data-gradient GEMMs' result G [B*P][Kp] (block-padded columns): the gradient
// entering the quantiser is fl(fl(G fl(as / L)) / se), the isint form's x_q = q se / se.detach()
__global__ __launch_bounds__(LQ_NT) void adda_in_bwd_kernel(const float* x, const float* G, Geo g, int C, int P,
                                                            long long n, Step st, float qp, const float* as, float* dx,
                                                            float* partial, bool vec) {
  __shared__ float red[LQ_WAVES];
  const float se = eff_step(st), f = div_ieee(*as, (float)g.L);
  float acc = 0.f;
  LQ_FLAT_LOOP(n) {
    float xv[4], dv[4];
    load4(x, i0, n, vec, xv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long long i = i0 + k;
      dv[k] = 0.f;
      if (i < n) {
        const long long bc = i / P, p = i - bc * P, b = bc / C;
        const int c = (int)(bc - b * C), j = c / g.rb;
        const float gr = G[(b * P + p) * g.Kp + j * g.rbp + (c - j * g.rb)];
        float t;
        dv[k] = quant_bwd(quant(xv[k], se, qp), div_ieee(mul_ieee(gr, f), se), se, t);
        acc = add_ieee(acc, t);
      }
    }
    store4(dx, i0, n, vec, dv);
  }
  block_partial(acc, red, partial);
}

// out[n][k] = fl(as G2[n][padded k]) (the weight gradient in code space)
__global__ __launch_bounds__(LQ_NT) void adda_unpack_wgrad_kernel(const float* G2, Geo g, const float* as, float* out,
                                                                  long long n, bool vec) {
  const float s = *as;
  LQ_FLAT_LOOP(n) {
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long long i = i0 + k;
      v[k] = 0.f;
      if (i < n) {
        const int row = (int)(i / g.K), c = (int)(i - (long long)row * g.K), j = c / g.rb;
        v[k] = mul_ieee(s, G2[(long long)row * g.Kp + j * g.rbp + (c - j * g.rb)]);
      }
    }
    store4(out, i0, n, vec, v);
  }
}

__global__ __launch_bounds__(LQ_NT) void adda_absmax_finish_kernel(const float* partial, int parts, float* out) {
  float m;
  int nan;
  absmax_finish(partial, parts, m, nan);
  if (threadIdx.x == 0) out[0] = nan ? __int_as_float(0x7fc00000) : m;
}

}  // namespace

extern "C" size_t sdmi_adda_workspace(void) { return (size_t)2 * LQ_CAP * sizeof(float); }

extern "C" int sdmi_adda_geometry(int M, int N, int K, int rb, int input_bit, int dac_bit, int* out) {
  Geo g;
  if (!out || !make_geo(g, M, N, K, rb, input_bit, dac_bit)) return -1;
  out[0] = g.nb; out[1] = g.rbp; out[2] = g.L; out[3] = g.Mp; out[4] = g.Np; out[5] = g.Kp;
  return 0;
}

extern "C" int sdmi_adda_in_fwd(const float* x, int B, int C, int P, const float* step, float g, int input_bit,
                                int dac_bit, int rb, void* slices, sdmi_stream_t stream) {
  Geo geo;
  if (!x || !step || !slices || B <= 0 || P <= 0 || !al16(slices) || (long long)B * P > 0x7fffffffLL) return -1;
  if (!make_geo(geo, B * P, 1, C, rb, input_bit, dac_bit)) return -1;
  const int qp = (1 << (input_bit - 1)) - 1;
  sdmi_rt::launch(adda_in_fwd_kernel, dim3(item_blocks((long long)geo.Mp * (geo.Kp / 8))), dim3(LQ_NT), 0,
                  (hipStream_t)stream, x, B, C, P, Step{step, g}, (float)qp, geo, (bf16_t*)slices);
  SDMI_CHECK_LAUNCH();
  return 0;
}

extern "C" int sdmi_adda_pack_w(const float* w, int N, int K, int rb, void* hi, void* lo, sdmi_stream_t stream) {
  Geo geo;
  if (!w || !hi || !al16(hi) || (lo && !al16(lo)) || !make_geo(geo, 1, N, K, rb, 2, 2)) return -1;
  sdmi_rt::launch(adda_pack_w_kernel, dim3(item_blocks((long long)geo.Np * (geo.Kp / 8))), dim3(LQ_NT), 0,
                  (hipStream_t)stream, w, geo, (bf16_t*)hi, (bf16_t*)lo);
  SDMI_CHECK_LAUNCH();
  return 0;
}

extern "C" int sdmi_adda_gemm(const void* slices, const void* w_hi, const void* w_lo, int M, int N, int K, int rb,
                              int input_bit, int dac_bit, int adc_bit, const float* adc_scale, const float* gain_noise,
                              const float* offset_noise, const float* step_w, const float* step_in, const float* bias,
                              float* pre, int ld, unsigned* mask, float* T, sdmi_stream_t stream) {
  GemmArgs a;
  if (!slices || !w_hi || !adc_scale || !pre || ld < N || adc_bit < 2 || adc_bit > 16 || !al16(slices) || !al16(w_hi) ||
      (w_lo && !al16(w_lo)) || (!gain_noise) != (!offset_noise) || (gain_noise && N > 1000) || (!mask) != (!T) ||
      !make_geo(a.g, M, N, K, rb, input_bit, dac_bit))
    return -1;
  if ((long long)M * ld * ((a.g.nb * a.g.L + 31) / 32) > 0x7fffffffLL) return -1;
  a.xs = (const bf16_t*)slices; a.whi = (const bf16_t*)w_hi; a.wlo = (const bf16_t*)w_lo;
  a.R = (float)((1 << (adc_bit - 1)) - 1);
  a.as = adc_scale; a.gn = gain_noise; a.on = offset_noise; a.sw = step_w; a.sin = step_in; a.bias = bias;
  a.pre = pre; a.ld = ld; a.mask = mask; a.T = T;
  const dim3 grid(a.g.Np / AD_T, a.g.Mp / AD_T);
  if (w_lo) sdmi_rt::launch(adda_gemm_kernel<true>, grid, dim3(AD_NT), 0, (hipStream_t)stream, a);
  else sdmi_rt::launch(adda_gemm_kernel<false>, grid, dim3(AD_NT), 0, (hipStream_t)stream, a);
  SDMI_CHECK_LAUNCH();
  return 0;
}

extern "C" int sdmi_adda_bwd_ops(const void* dpre, int ld_d, const float* pre, int ld, const float* bias, const float* T,
                                 const unsigned* mask, int M, int N, int nb, int L, int sb, const float* adc_scale,
                                 const float* step_w, const float* step_in, void* U, void* V, float* ws, float* dscale,
                                 sdmi_stream_t stream) {
  if (!dpre || !pre || !T || !mask || !adc_scale || !U || !V || !ws || !dscale || M <= 0 || N <= 0 || nb <= 0 || L <= 0 ||
      L > 8 || sb < 1 || sb > 8 || (L - 1) * sb > 8 || ld < N || ld_d < N || ld_d % 8 || !al16(dpre) || !al16(U) || !al16(V))
    return -1;
  OpsArgs a;
  a.Mp = r_up(M, AD_T);
  if ((long long)nb * L * a.Mp * ld_d > 0x7fffffffLL || (long long)M * ld * ((nb * L + 31) / 32) > 0x7fffffffLL) return -1;
  a.dpre = (const bf16_t*)dpre; a.ld_d = ld_d; a.pre = pre; a.ld = ld; a.bias = bias; a.T = T; a.mask = mask;
  a.M = M; a.N = N; a.nb = nb; a.L = L; a.sb = sb; a.as = adc_scale; a.sw = step_w; a.sin = step_in;
  a.U = (bf16_t*)U; a.V = (bf16_t*)V; a.partial = ws;
  const int nblk = item_blocks((long long)a.Mp * (ld_d / 8));
  sdmi_rt::launch(adda_bwd_ops_kernel, dim3(nblk), dim3(LQ_NT), 0, (hipStream_t)stream, a);
  SDMI_CHECK_LAUNCH();
  sdmi_rt::launch(adda_scale_finish_kernel, dim3(1), dim3(LQ_NT), 0, (hipStream_t)stream, (const float*)ws, nblk,
                  adc_scale, dscale);
  SDMI_CHECK_LAUNCH();
  return 0;
}

extern "C" int sdmi_adda_in_bwd(const float* x, const float* G, int B, int C, int P, int rb, const float* step, float g,
                                int input_bit, int dac_bit, const float* adc_scale, float* dx, float* ws, float* ds,
                                sdmi_stream_t stream) {
  Geo geo;
  if (!x || !G || !step || !adc_scale || !dx || !ws || !ds || B <= 0 || P <= 0 || (long long)B * P > 0x7fffffffLL) return -1;
  if (!make_geo(geo, B * P, 1, C, rb, input_bit, dac_bit)) return -1;
  const long long n = (long long)B * C * P;
  if (n > 0x7fffffffLL) return -1;
  const int qp = (1 << (input_bit - 1)) - 1, nblk = flat_blocks(n);
  sdmi_rt::launch(adda_in_bwd_kernel, dim3(nblk), dim3(LQ_NT), 0, (hipStream_t)stream, x, G, geo, C, P, n, Step{step, g},
                  (float)qp, adc_scale, dx, ws, al16(x) && al16(dx));
  SDMI_CHECK_LAUNCH();
  sdmi_rt::launch(lsq_finish_kernel, dim3(1), dim3(LQ_NT), 0, (hipStream_t)stream, (const float*)ws, nblk, g, ds);
  SDMI_CHECK_LAUNCH();
  return 0;
}

extern "C" int sdmi_adda_unpack_wgrad(const float* G2, int N, int K, int rb, const float* adc_scale, float* out,
                                      sdmi_stream_t stream) {
  Geo geo;
  if (!G2 || !adc_scale || !out || !make_geo(geo, 1, N, K, rb, 2, 2)) return -1;
  const long long n = (long long)N * K;
  if (n > 0x7fffffffLL) return -1;
  sdmi_rt::launch(adda_unpack_wgrad_kernel, dim3(flat_blocks(n)), dim3(LQ_NT), 0, (hipStream_t)stream, G2, geo, adc_scale,
                  out, n, al16(out));
  SDMI_CHECK_LAUNCH();
  return 0;
}

extern "C" int sdmi_adda_absmax(const float* x, long long n, float* ws, float* out, sdmi_stream_t stream) {
  if (!x || !ws || !out || n <= 0 || n > 0x7fffffffLL) return -1;
  const int nblk = flat_blocks(n);
  sdmi_rt::launch(lsq_absmax_kernel, dim3(nblk), dim3(LQ_NT), 0, (hipStream_t)stream, x, n, ws, al16(x));
  SDMI_CHECK_LAUNCH();
  sdmi_rt::launch(adda_absmax_finish_kernel, dim3(1), dim3(LQ_NT), 0, (hipStream_t)stream, (const float*)ws, nblk, out);
  SDMI_CHECK_LAUNCH();
  return 0;
}
