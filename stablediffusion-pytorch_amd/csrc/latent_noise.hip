// Latent-range noise of the noise-robust VQVAE for gfx950 (reference models/vqvae_noise.py:155,177-183):
//
//     out = z + (z.max() - z.min()) * n_scale * eps          after quantize(), before decode()
//
// and its backward. The range is differentiable: with g = dL/d(out), autograd returns g to z and adds
// n_scale * sum(g * eps) to the elements equal to the maximum, divided evenly among them, and subtracts the same
// sum, divided among the elements equal to the minimum, from those (torch's tie rule for full reductions).
//
//  latent_range    : min, max and the number of elements equal to each over a flat fp32 tensor. One partial
//                    {min, max, cnt_min, cnt_max} per workgroup; a NaN anywhere makes both extremes NaN (counts 0).
//                    -0.0 == +0.0. Minimum, maximum and integer counts are exact in any order, so the consumers
//                    merge the at most 256 partials themselves (no finaliser launch).
//  latent_noise_fwd: out = fl(z + fl(fl(fl(max - min) * n_scale) * eps)), every operation rounded on its own (the
//                    torch expression's order). <ZIN>: the same pass also writes post_quant_conv(out) as the NHWC
//                    bf16 operand of decoder_conv_in, with the arithmetic of pointwise_in_kernel (vqvae.hip): the fma
//                    chain from the bias, ci ascending, RNE to bf16, pad columns zero.
//  latent_noise_dot: g = W_post^T dzin (the fma chain, co ascending) + dz_add, the dzq arithmetic of vq_bwd_kernel,
//                    and the per-workgroup partial of S = sum g * eps: each thread adds its pixels' rounded products
//                    in grid-stride order, channels ascending; then the butterfly, then the four waves in order.
//  latent_noise_bwd: S = the partials through one butterfly and the four waves in order; c_max = fl(fl(n_scale S) /
//                    cnt_max), c_min likewise; r = fl(dz_add + corr), corr = c_max at the maximum, -c_min at the
//                    minimum, fl(c_max - c_min) where both hold. r is what sdmi_vq_bwd takes as dzq_add (it adds
//                    W_post^T dzin itself).
//
// Host grid rules. Flat kernels (range, bwd): a workgroup of 256 threads spans 1024 consecutive elements per trip,
// min(256, ceil(n / 1024)) workgroups, grid-stride. Pixel kernels (fwd, dot): one thread per pixel (its C <= 8
// channels), min(256, ceil(P / 256)) workgroups, grid-stride. No atomics; every sum has a fixed order.
#include "common.h"
#include "../../include/sdmi.h"
#include <algorithm>

namespace {

constexpr int LN_NT = 256, LN_WAVES = LN_NT / 64, LN_SPAN = 4 * LN_NT, LN_CAP = 256, MAXC = 8;

inline int flat_blocks(long long n) { return (int)std::min<long long>(LN_CAP, (n + LN_SPAN - 1) / LN_SPAN); }
inline int pixel_blocks(long long P) { return (int)std::min<long long>(LN_CAP, (P + LN_NT - 1) / LN_NT); }

struct Range {
  float mn, mx;
  int cmn, cmx, nan;
};

__device__ __forceinline__ Range range_empty() { return Range{INFINITY, -INFINITY, 0, 0, 0}; }

__device__ __forceinline__ void range_take(Range& r, float v) {
  r.nan |= (v != v);
  if (v < r.mn) {
    r.mn = v;
    r.cmn = 1;
  } else if (v == r.mn) {
    ++r.cmn;
  }
  if (v > r.mx) {
    r.mx = v;
    r.cmx = 1;
  } else if (v == r.mx) {
    ++r.cmx;
  }
}

__device__ __forceinline__ void range_merge(Range& a, const Range& b) {
  a.nan |= b.nan;
  if (b.mn < a.mn) {
    a.mn = b.mn;
    a.cmn = b.cmn;
  } else if (b.mn == a.mn) {
    a.cmn += b.cmn;
  }
  if (b.mx > a.mx) {
    a.mx = b.mx;
    a.cmx = b.cmx;
  } else if (b.mx == a.mx) {
    a.cmx += b.cmx;
  }
}

// every thread of the workgroup gets the merged range; a NaN becomes {NaN, NaN, 0, 0}
__device__ __forceinline__ Range range_block(Range r, Range* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Range b;
    b.mn = __shfl_xor(r.mn, o, 64);
    b.mx = __shfl_xor(r.mx, o, 64);
    b.cmn = __shfl_xor(r.cmn, o, 64);
    b.cmx = __shfl_xor(r.cmx, o, 64);
    b.nan = __shfl_xor(r.nan, o, 64);
    range_merge(r, b);
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = r;
  __syncthreads();
  r = red[0];
#pragma unroll
  for (int w = 1; w < LN_WAVES; ++w) range_merge(r, red[w]);
  if (r.nan) {
    r.mn = r.mx = __int_as_float(0x7fc00000);
    r.cmn = r.cmx = 0;
  }
  return r;
}

// the partials of latent_range_kernel, merged by the whole workgroup
__device__ __forceinline__ Range range_load(const float* ws, int parts, Range* red) {
  Range r = range_empty();
  if ((int)threadIdx.x < parts) {
    const float* p = ws + 4 * threadIdx.x;
    const float mn = p[0], mx = p[1];
    if (mn != mn) {
      r.nan = 1;
    } else {
      r.mn = mn;
      r.mx = mx;
      r.cmn = __float_as_int(p[2]);
      r.cmx = __float_as_int(p[3]);
    }
  }
  return range_block(r, red);
}

__global__ __launch_bounds__(LN_NT) void latent_range_kernel(const float* z, long long n, float* ws) {
  __shared__ Range red[LN_WAVES];
  Range r = range_empty();
  for (long long base = (long long)blockIdx.x * LN_SPAN; base < n; base += (long long)gridDim.x * LN_SPAN) {
#pragma unroll
    for (int k = 0; k < LN_SPAN / LN_NT; ++k) {
      const long long i = base + k * LN_NT + threadIdx.x;
      if (i < n) range_take(r, z[i]);
    }
  }
  r = range_block(r, red);
  if (threadIdx.x == 0) {
    float* p = ws + 4 * blockIdx.x;
    p[0] = r.mn;
    p[1] = r.mx;
    p[2] = __int_as_float(r.cmn);
    p[3] = __int_as_float(r.cmx);
  }
}

struct NoiseFwdArgs {
  const float* z;    // NCHW fp32 latent
  const float* eps;  // NCHW fp32 standard-normal draw
  int B, C, HW;
  float n_scale;
  const float* ws; int parts;  // the range partials
  float* out;        // NCHW fp32 noisy latent
  const float* w; const float* b; int cout;  // post_quant_conv (cout, C), bias or null
  bf16_t* zin; int ld;                       // NHWC bf16 [P][ld]
};

template <bool ZIN>
__global__ __launch_bounds__(LN_NT) void latent_noise_fwd_kernel(const NoiseFwdArgs a) {
  __shared__ Range red[LN_WAVES];
  const Range r = range_load(a.ws, a.parts, red);
  const float s = mul_ieee(sub_ieee(r.mx, r.mn), a.n_scale);
  const int C = a.C;
  const long long P = (long long)a.B * a.HW;
  for (long long pix = (long long)blockIdx.x * LN_NT + threadIdx.x; pix < P; pix += (long long)gridDim.x * LN_NT) {
    const long long bb = pix / a.HW, p = pix - bb * a.HW;
    float o[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      o[c] = 0.f;
      if (c < C) {
        const long long i = (bb * C + c) * a.HW + p;
        o[c] = add_ieee(a.z[i], mul_ieee(s, a.eps[i]));
        a.out[i] = o[c];
      }
    }
    if constexpr (ZIN) {
#pragma unroll
      for (int co = 0; co < MAXC; ++co) {
        if (co >= a.ld) break;
        float v = 0.f;
        if (co < a.cout) {
          v = a.b ? a.b[co] : 0.f;
#pragma unroll
          for (int ci = 0; ci < MAXC; ++ci)
            if (ci < C) v = fmaf(a.w[co * C + ci], o[ci], v);
        }
        a.zin[pix * a.ld + co] = f2bf(v);
      }
      for (int co = MAXC; co < a.ld; ++co) a.zin[pix * a.ld + co] = 0;
    }
  }
}

struct NoiseDotArgs {
  const bf16_t* dzin; int ld_dzin;  // gradient of post_quant_conv's output, NHWC bf16 [P][ld], or null
  const float* w_post;              // (C, C)
  const float* dz_add;              // NCHW fp32 gradient of the noisy latent from outside the decoder, or null
  const float* eps;
  int B, C, HW;
  float* partial;                   // one per workgroup
};

__global__ __launch_bounds__(LN_NT) void latent_noise_dot_kernel(const NoiseDotArgs a) {
  __shared__ float red[LN_WAVES];
  const int C = a.C;
  const long long P = (long long)a.B * a.HW;
  float acc = 0.f;
  for (long long pix = (long long)blockIdx.x * LN_NT + threadIdx.x; pix < P; pix += (long long)gridDim.x * LN_NT) {
    const long long bb = pix / a.HW, p = pix - bb * a.HW;
    float dzin[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) dzin[c] = (a.dzin && c < C) ? bf2f(a.dzin[pix * a.ld_dzin + c]) : 0.f;
#pragma unroll
    for (int ci = 0; ci < MAXC; ++ci) {
      if (ci < C) {
        const long long i = (bb * C + ci) * a.HW + p;
        float g;
        if (a.dzin) {
          g = 0.f;
#pragma unroll
          for (int co = 0; co < MAXC; ++co)
            if (co < C) g = fmaf(a.w_post[co * C + ci], dzin[co], g);
          if (a.dz_add) g += a.dz_add[i];
        } else {
          g = a.dz_add[i];
        }
        acc = add_ieee(acc, mul_ieee(g, a.eps[i]));
      }
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) a.partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(LN_NT) void latent_noise_bwd_kernel(const float* z, const float* dz_add, long long n,
                                                                 float n_scale, const float* ws_range, int parts_range,
                                                                 const float* partial, int parts, float* r) {
  __shared__ Range red[LN_WAVES];
  __shared__ float reds[LN_WAVES];
  const Range rg = range_load(ws_range, parts_range, red);
  float v = (int)threadIdx.x < parts ? partial[threadIdx.x] : 0.f;
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) reds[threadIdx.x >> 6] = v;
  __syncthreads();
  const float S = ((reds[0] + reds[1]) + reds[2]) + reds[3];
  const float t = mul_ieee(n_scale, S);
  const float c_max = t / (float)rg.cmx, c_min = t / (float)rg.cmn;
  const float both = sub_ieee(c_max, c_min);
  for (long long base = (long long)blockIdx.x * LN_SPAN; base < n; base += (long long)gridDim.x * LN_SPAN) {
#pragma unroll
    for (int k = 0; k < LN_SPAN / LN_NT; ++k) {
      const long long i = base + k * LN_NT + threadIdx.x;
      if (i < n) {
        const float zi = z[i];
        const bool at_max = zi == rg.mx, at_min = zi == rg.mn;
        const float corr = at_max ? (at_min ? both : c_max) : (at_min ? -c_min : 0.f);
        r[i] = add_ieee(dz_add ? dz_add[i] : 0.f, corr);
      }
    }
  }
}

}  // namespace

// four floats per range workgroup; the backward's S partials (one float per pixel workgroup, never more than four
// times the range workgroups) fit the same size
extern "C" size_t sdmi_latent_noise_workspace(long long n) {
  return n > 0 ? (size_t)flat_blocks(n) * 4 * sizeof(float) : 0;
}

extern "C" int sdmi_latent_range(const float* z, long long n, float* ws, sdmi_stream_t stream) {
  if (!z || !ws || n <= 0 || n > 0x7fffffffLL) return -1;
  sdmi_rt::launch(latent_range_kernel, dim3(flat_blocks(n)), dim3(LN_NT), 0, (hipStream_t)stream, z, n, ws);
  SDMI_CHECK_LAUNCH();
  return 0;
}

extern "C" int sdmi_latent_noise_fwd(const float* z, const float* eps, int B, int C, int HW, float n_scale,
                                     const float* ws, float* out, const float* w_post, const float* b_post, int cout,
                                     void* zin, int ld, sdmi_stream_t stream) {
  if (!z || !ws || !out || B <= 0 || C <= 0 || C > MAXC || HW <= 0) return -1;
  const long long P = (long long)B * HW;
  if (P * C > 0x7fffffffLL) return -1;
  if (zin && (!w_post || cout <= 0 || cout > MAXC || ld < cout)) return -1;
  if (n_scale == 0.f) return 0;  // the caller keeps z: nothing is launched and eps is not read
  if (!eps) return -1;
  NoiseFwdArgs a;
  a.z = z; a.eps = eps; a.B = B; a.C = C; a.HW = HW; a.n_scale = n_scale; a.ws = ws; a.parts = flat_blocks(P * C);
  a.out = out; a.w = w_post; a.b = b_post; a.cout = cout; a.zin = (bf16_t*)zin; a.ld = ld;
  if (zin)
    sdmi_rt::launch(latent_noise_fwd_kernel<true>, dim3(pixel_blocks(P)), dim3(LN_NT), 0, (hipStream_t)stream, a);
  else
    sdmi_rt::launch(latent_noise_fwd_kernel<false>, dim3(pixel_blocks(P)), dim3(LN_NT), 0, (hipStream_t)stream, a);
  SDMI_CHECK_LAUNCH();
  return 0;
}

extern "C" int sdmi_latent_noise_bwd(const void* dzin, int ld_dzin, const float* w_post, const float* dz_add,
                                     const float* eps, const float* z, int B, int C, int HW, float n_scale,
                                     const float* ws_range, float* ws, float* r, sdmi_stream_t stream) {
  if ((!dzin && !dz_add) || !z || !ws_range || !ws || !r || B <= 0 || C <= 0 || C > MAXC || HW <= 0) return -1;
  const long long P = (long long)B * HW;
  if (P * C > 0x7fffffffLL) return -1;
  if (dzin && (!w_post || ld_dzin < C)) return -1;
  if (n_scale == 0.f) return 0;  // no noise was added: the caller's dz_add is the whole gradient
  if (!eps) return -1;
  NoiseDotArgs a;
  a.dzin = (const bf16_t*)dzin; a.ld_dzin = ld_dzin; a.w_post = w_post; a.dz_add = dz_add; a.eps = eps;
  a.B = B; a.C = C; a.HW = HW; a.partial = ws;
  const int pb = pixel_blocks(P);
  sdmi_rt::launch(latent_noise_dot_kernel, dim3(pb), dim3(LN_NT), 0, (hipStream_t)stream, a);
  SDMI_CHECK_LAUNCH();
  const long long n = P * C;
  sdmi_rt::launch(latent_noise_bwd_kernel, dim3(flat_blocks(n)), dim3(LN_NT), 0, (hipStream_t)stream, z, dz_add, n,
                  n_scale, ws_range, flat_blocks(n), (const float*)ws, pb, r);
  SDMI_CHECK_LAUNCH();
  return 0;
}
