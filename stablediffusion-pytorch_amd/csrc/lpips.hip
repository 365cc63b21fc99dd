// LPIPS perceptual loss (models/lpips.py) around the VGG16 convolutions, which are the library's implicit GEMMs:
// image scaling + packing, the 2x2 max-pool pair, the per-tap distance (unit-normalise, weighted squared difference,
// spatial mean) with its backward, and the image gradient out of the scaled-image gradient.
// Activations are NHWC bf16 (16 bytes = 8 channels per access), arithmetic fp32. Every reduction has a fixed order
// (lanes, waves, per-block partials, one ordered sum): results are bitwise repeatable, no atomics.
// NaN passes as in torch: through the pool pair (below), through the ReLU select of the distance backward, and -- in
// the GEMM epilogue of the convolutions (gemm_epilogue.h, act 2 and 3) -- through ReLU and its gradient; an image with a
// NaN pixel gets a NaN distance. Every entry point returns -1 before any launch for a null required pointer, a
// non-positive size, C outside {64, 128, 256, 512} (distance) or not a positive multiple of 8 (pool), H or W below 2
// (pool), a leading dimension below C or not a multiple of 8, side outside {0, 1}, B above 65535 (distance: grid.y), and
// for the image gradient no output, one of mse_pred / mse_target alone, or mse without acc_nhwc.
#include "common.h"
#include "../../include/sdmi.h"

namespace {
constexpr int NT = 256;
constexpr int DIST_PASSES = 8;  // pixel groups per workgroup of the distance kernels

int grid_for(long long work) {
  long long g = (work + NT - 1) / NT;
  return (int)(g > 65536 ? 65536 : (g < 1 ? 1 : g));
}

// ---------------------------------------------------------------------------------------------
// ScalingLayer + packing: out[(s*B + b)*HW + p][0..2] = (x_s - shift) / scale (x -> 2x - 1 first under normalize),
// channels 3..7 zero. A source is NCHW fp32 (B,3,H,W) or NHWC fp32 [B*HW][8] (the training engine's reconstruction).
// ---------------------------------------------------------------------------------------------
__global__ void lpips_prep_kernel(const float* in0, int nhwc0, const float* in1, int nhwc1, int B, int HW,
                                  const float* shift, const float* scale, int normalize, bf16_t* out) {
  const long long half = (long long)B * HW, total = 2 * half;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
    const int s = i >= half;
    const long long r = i - (s ? half : 0);
    const float* src = s ? in1 : in0;
    float x[3];
    if (s ? nhwc1 : nhwc0) {
      const float4 v = *(const float4*)(src + r * 8);
      x[0] = v.x; x[1] = v.y; x[2] = v.z;
    } else {
      const long long b = r / HW, p = r - b * HW;
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c] = src[(b * 3 + c) * HW + p];
    }
    float y[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = x[c];
      if (normalize) v = sub_ieee(mul_ieee(2.f, v), 1.f);
      y[c] = sub_ieee(v, shift[c]) / scale[c];
    }
    *(uint4*)(out + i * 8) = pack8(y);
  }
}

// Gradient of the image from the gradient of the scaled image d [B*HW][8] bf16: g_c = d_c / scale[c] (x 2 under
// normalize). nchw != NULL: written as (B,3,H,W) fp32. acc != NULL: added into channels 0..2 of the NHWC bf16
// [B*HW][8] buffer acc (sum formed in fp32, rounded once; channels 3..7 untouched) -- or, with pred (NHWC fp32
// [B*HW][8]) and target (NCHW fp32), acc is written whole: the MSE gradient 2 (pred - target) / (3 B HW) of sdmi_mse
// plus g, both fp32, rounded to bf16 once, channels 3..7 zero.
__global__ void lpips_image_grad_kernel(const bf16_t* d, int B, int HW, const float* scale, int normalize, float* nchw,
                                        bf16_t* acc, const float* pred, const float* target) {
  const long long total = (long long)B * HW;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
    float v[8];
    unpack8(*(const uint4*)(d + i * 8), v);
    float g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      g[c] = v[c] / scale[c];
      if (normalize) g[c] = mul_ieee(g[c], 2.f);
    }
    if (nchw) {
      const long long b = i / HW, p = i - b * HW;
#pragma unroll
      for (int c = 0; c < 3; ++c) nchw[(b * 3 + c) * HW + p] = g[c];
    }
    if (acc && pred) {
      const long long b = i / HW, p = i - b * HW;
      const float n = (float)(3LL * B * HW);
      const float4 pv = *(const float4*)(pred + i * 8);
      const float px[3] = {pv.x, pv.y, pv.z};
      float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = add_ieee(2.f * (px[c] - target[(b * 3 + c) * HW + p]) / n, g[c]);
      *(uint4*)(acc + i * 8) = pack8(o);
    } else if (acc) {
      const uint2 old = *(const uint2*)(acc + i * 8);  // channels 0..3; only these 8 bytes are rewritten
      uint2 o;
      o.x = pack2bf(add_ieee(__uint_as_float(old.x << 16), g[0]), add_ieee(__uint_as_float(old.x & 0xffff0000u), g[1]));
      o.y = (old.y & 0xffff0000u) | (uint32_t)f2bf(add_ieee(__uint_as_float(old.y << 16), g[2]));
      *(uint2*)(acc + i * 8) = o;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// nn.MaxPool2d(2, 2) on NHWC bf16, floor mode. The first maximum in scan order (0,0), (0,1), (1,0), (1,1) wins
// (strict > while scanning), as torch's forward records its index. A NaN replaces the running maximum as it does in
// torch (v > m || isnan(v)): any NaN in the window gives NaN, and the gradient goes to the last NaN in scan order.
// ---------------------------------------------------------------------------------------------
__global__ void maxpool2_fwd_kernel(const bf16_t* x, int N, int H, int W, int C, bf16_t* y) {
  const int OH = H >> 1, OW = W >> 1, CG = C >> 3;
  const long long total = (long long)N * OH * OW * CG;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
    const int cg = (int)(i % CG);
    long long t = i / CG;
    const int ox = (int)(t % OW);
    t /= OW;
    const int oy = (int)(t % OH);
    const long long n = t / OH;
    const bf16_t* px = x + ((n * H + 2 * oy) * W + 2 * ox) * C + cg * 8;
    float m[8], v[8];
    unpack8(*(const uint4*)px, m);
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      unpack8(*(const uint4*)(px + ((long long)(k >> 1) * W + (k & 1)) * C), v);
#pragma unroll
      for (int e = 0; e < 8; ++e) m[e] = (v[e] > m[e] || v[e] != v[e]) ? v[e] : m[e];
    }
    *(uint4*)(y + i * 8) = pack8(m);
  }
}

// dx (N,H,W,C) fully overwritten: dy goes to the window's first maximum (recomputed from x), everything else --
// the dropped odd last row / column included -- is zero. One thread per 2x2 cell of the ceil(H/2) x ceil(W/2) grid.
__global__ void maxpool2_bwd_kernel(const bf16_t* x, const bf16_t* dy, int N, int H, int W, int C, bf16_t* dx) {
  const int OH = H >> 1, OW = W >> 1, CH = (H + 1) >> 1, CW = (W + 1) >> 1, CG = C >> 3;
  const long long total = (long long)N * CH * CW * CG;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
    const int cg = (int)(i % CG);
    long long t = i / CG;
    const int ox = (int)(t % CW);
    t /= CW;
    const int oy = (int)(t % CH);
    const long long n = t / CH;
    const long long base = ((n * H + 2 * oy) * W + 2 * ox) * C + cg * 8;
    if (oy >= OH || ox >= OW) {  // cells of the dropped row / column: zero what lies inside the image
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (2 * oy + (k >> 1) < H && 2 * ox + (k & 1) < W)
          *(uint4*)(dx + base + ((long long)(k >> 1) * W + (k & 1)) * C) = make_uint4(0, 0, 0, 0);
      continue;
    }
    float m[8], v[8], g[8];
    int arg[8];
    unpack8(*(const uint4*)(x + base), m);
#pragma unroll
    for (int e = 0; e < 8; ++e) arg[e] = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      unpack8(*(const uint4*)(x + base + ((long long)(k >> 1) * W + (k & 1)) * C), v);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const bool gt = v[e] > m[e] || v[e] != v[e];
        m[e] = gt ? v[e] : m[e];
        arg[e] = gt ? k : arg[e];
      }
    }
    unpack8(*(const uint4*)(dy + (((n * OH + oy) * OW + ox) * (long long)CG + cg) * 8), g);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = arg[e] == k ? g[e] : 0.f;
      *(uint4*)(dx + base + ((long long)(k >> 1) * W + (k & 1)) * C) = pack8(o);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Layer distance of one tap f [2B*P][C] (rows [0, B*P): image 0, the rest: image 1), C in {64, 128, 256, 512}.
// C/8 lanes share a pixel (8 channels each), so a wave holds 512/C pixels and a workgroup DIST_PASSES * 4 such
// groups of one sample. Lane sums go through xor shuffles below the pixel's lane count.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float group_sum(float v, int lpp) {
  for (int o = lpp >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float inv_norm(float sumsq) { return 1.0f / fmaxf(sqrtf(sumsq), 1e-12f); }

int dist_pixels_per_block(int C) { return DIST_PASSES * (NT / 64) * (512 / C); }

// partial[b * gridDim.x + blockIdx.x] = sum over the block's pixels of sum_c w_c (u0_c - u1_c)^2; rn (nullable):
// the inverse norms 1 / max(|f|, 1e-12) of all 2B*P rows.
__global__ void lpips_dist_fwd_kernel(const bf16_t* f, int ld, const float* w, int B, int P, int C, float* rn,
                                      float* partial) {
  const int lpp = C >> 3, ppw = 64 / lpp;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / lpp, cl = lane - sub * lpp;
  const int b = blockIdx.y;
  const long long p0 = (long long)blockIdx.x * DIST_PASSES * (NT / 64) * ppw;
  float wv[8];
  *(float4*)&wv[0] = *(const float4*)(w + cl * 8);
  *(float4*)&wv[4] = *(const float4*)(w + cl * 8 + 4);
  float acc = 0.f;
  for (int k = 0; k < DIST_PASSES; ++k) {
    const long long p = p0 + (long long)(k * (NT / 64) + wave) * ppw + sub;
    const bool ok = p < P;
    const long long r0 = (long long)b * P + p, r1 = r0 + (long long)B * P;
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
    if (ok) {
      q0 = *(const uint4*)(f + r0 * ld + cl * 8);
      q1 = *(const uint4*)(f + r1 * ld + cl * 8);
    }
    float a[8], c[8];
    unpack8(q0, a);
    unpack8(q1, c);
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      s0 += a[e] * a[e];
      s1 += c[e] * c[e];
    }
    const float i0 = inv_norm(group_sum(s0, lpp)), i1 = inv_norm(group_sum(s1, lpp));
    float d = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      // both products rounded before the subtraction (no FMA contraction): identical images give exactly 0
      const float t = sub_ieee(mul_ieee(a[e], i0), mul_ieee(c[e], i1));
      d += wv[e] * t * t;
    }
    d = group_sum(d, lpp);
    if (ok && cl == 0) {
      acc += d;
      if (rn) {
        rn[r0] = i0;
        rn[r1] = i1;
      }
    }
  }
  __shared__ float red[NT / 64];
  acc = wave_sum(acc);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int i = 0; i < NT / 64; ++i) s += red[i];
    partial[(long long)b * gridDim.x + blockIdx.x] = s;
  }
}

// val[b] = (accumulate ? val[b] : 0) + (1/P) * sum of the sample's nblk partials (one wave per sample, fixed order)
__global__ void lpips_dist_sum_kernel(const float* partial, int nblk, float inv_p, int accumulate, float* val) {
  const int b = blockIdx.x;
  float acc = 0.f;
  for (int i = threadIdx.x; i < nblk; i += 64) acc += partial[(long long)b * nblk + i];
  acc = wave_sum(acc);
  // one rounding, stated (the compiler contracted the plain expression to the same fma)
  if (threadIdx.x == 0) val[b] = fmaf(acc, inv_p, accumulate ? val[b] : 0.f);
}

// Gradient of the tap rows of image `side` (a: own rows, o: the other image's):
//   t_c = 2 w_c (ua_c - uo_c),  df_c = coef * rn_a * (t_c - ua_c * sum_k t_k ua_k),  coef = (g ? g[b] : 1) * gscale / P
//   dy = f_a <= 0 ? 0 : df + addend   (the tap is a ReLU output; addend: the gradient arriving from the next slice;
//   a NaN activation passes the gradient on, as torch's threshold_backward does)
// An all-zero row has u = 0 and a huge rn; the select keeps its output an exact zero.
__global__ void lpips_dist_bwd_kernel(const bf16_t* f, int ld, const float* w, const float* rn, const float* g,
                                      float gscale, int B, int P, int C, int side, const bf16_t* addend, int ld_add,
                                      bf16_t* dy, int ld_dy) {
  const int lpp = C >> 3, ppw = 64 / lpp;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / lpp, cl = lane - sub * lpp;
  const int b = blockIdx.y;
  const long long p0 = (long long)blockIdx.x * DIST_PASSES * (NT / 64) * ppw;
  const float coef = (g ? g[b] : 1.f) * gscale / (float)P;
  float wv[8];
  *(float4*)&wv[0] = *(const float4*)(w + cl * 8);
  *(float4*)&wv[4] = *(const float4*)(w + cl * 8 + 4);
  for (int k = 0; k < DIST_PASSES; ++k) {
    const long long p = p0 + (long long)(k * (NT / 64) + wave) * ppw + sub;
    const bool ok = p < P;
    const long long r = (long long)b * P + p;  // row within one image's half
    const long long ra = r + (side ? (long long)B * P : 0), ro = r + (side ? 0 : (long long)B * P);
    uint4 qa = make_uint4(0, 0, 0, 0), qo = qa, qd = qa;
    float ia = 0.f, io = 0.f;
    if (ok) {
      qa = *(const uint4*)(f + ra * ld + cl * 8);
      qo = *(const uint4*)(f + ro * ld + cl * 8);
      if (addend) qd = *(const uint4*)(addend + r * ld_add + cl * 8);
      ia = rn[ra];
      io = rn[ro];
    }
    float a[8], o[8], ad[8], t[8];
    unpack8(qa, a);
    unpack8(qo, o);
    unpack8(qd, ad);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float ua = mul_ieee(a[e], ia);
      t[e] = 2.f * wv[e] * sub_ieee(ua, mul_ieee(o[e], io));  // as the forward: exactly 0 for identical images
      s += t[e] * ua;
    }
    s = group_sum(s, lpp);
    float out[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float df = coef * ia * (t[e] - a[e] * ia * s);
      out[e] = a[e] <= 0.f ? 0.f : df + ad[e];
    }
    if (ok) *(uint4*)(dy + r * ld_dy + cl * 8) = pack8(out);
  }
}

// out[0] = scale * sum_b val[b] (ordered): the trainer's weighted mean of the per-sample distances
__global__ void lpips_mean_kernel(const float* val, int B, float scale, float* out) {
  if (threadIdx.x) return;
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += val[b];
  out[0] = s * scale;
}

bool tap_channels_ok(int C) { return C == 64 || C == 128 || C == 256 || C == 512; }
}  // namespace

extern "C" int sdmi_lpips_prep(const float* in0, int in0_nhwc, const float* in1, int in1_nhwc, int B, int H, int W,
                               const float* shift, const float* scale, int normalize, void* out,
                               sdmi_stream_t stream) {
  if (!in0 || !in1 || !shift || !scale || !out || B < 1 || H < 1 || W < 1) return -1;
  sdmi_rt::launch(lpips_prep_kernel, dim3(grid_for(2LL * B * H * W)), dim3(NT), 0, (hipStream_t)stream, in0, in0_nhwc,
                  in1, in1_nhwc, B, H * W, shift, scale, normalize, (bf16_t*)out);
  SDMI_CHECK_LAUNCH();
  return 0;
}

extern "C" int sdmi_lpips_image_grad(const void* d, int B, int H, int W, const float* scale, int normalize,
                                     float* out_nchw, void* acc_nhwc, const float* mse_pred, const float* mse_target,
                                     sdmi_stream_t stream) {
  if (!d || !scale || (!out_nchw && !acc_nhwc) || B < 1 || H < 1 || W < 1) return -1;
  if ((mse_pred != nullptr) != (mse_target != nullptr) || (mse_pred && !acc_nhwc)) return -1;
  sdmi_rt::launch(lpips_image_grad_kernel, dim3(grid_for((long long)B * H * W)), dim3(NT), 0, (hipStream_t)stream,
                  (const bf16_t*)d, B, H * W, scale, normalize, out_nchw, (bf16_t*)acc_nhwc, mse_pred, mse_target);
  SDMI_CHECK_LAUNCH();
  return 0;
}

extern "C" int sdmi_maxpool2_fwd(const void* x, int N, int H, int W, int C, void* y, sdmi_stream_t stream) {
  if (!x || !y || N < 1 || H < 2 || W < 2 || C < 8 || C % 8) return -1;
  sdmi_rt::launch(maxpool2_fwd_kernel, dim3(grid_for((long long)N * (H / 2) * (W / 2) * (C / 8))), dim3(NT), 0,
                  (hipStream_t)stream, (const bf16_t*)x, N, H, W, C, (bf16_t*)y);
  SDMI_CHECK_LAUNCH();
  return 0;
}

extern "C" int sdmi_maxpool2_bwd(const void* x, const void* dy, int N, int H, int W, int C, void* dx,
                                 sdmi_stream_t stream) {
  if (!x || !dy || !dx || N < 1 || H < 2 || W < 2 || C < 8 || C % 8) return -1;
  sdmi_rt::launch(maxpool2_bwd_kernel, dim3(grid_for((long long)N * ((H + 1) / 2) * ((W + 1) / 2) * (C / 8))),
                  dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)dy, N, H, W, C, (bf16_t*)dx);
  SDMI_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t sdmi_lpips_dist_workspace(int B, int P, int C) {
  if (!tap_channels_ok(C) || B < 1 || P < 1) return 0;
  const int ppb = dist_pixels_per_block(C);
  return (size_t)B * ((P + ppb - 1) / ppb) * sizeof(float);
}

extern "C" int sdmi_lpips_dist_fwd(const void* f, int ld, const float* w, int B, int P, int C, float* rn, float* ws,
                                   int accumulate, float* val, sdmi_stream_t stream) {
  if (!f || !w || !ws || !val || !tap_channels_ok(C) || ld < C || ld % 8 || B < 1 || B > 65535 || P < 1) return -1;
  const int ppb = dist_pixels_per_block(C);
  const int nblk = (P + ppb - 1) / ppb;
  hipStream_t s = (hipStream_t)stream;
  sdmi_rt::launch(lpips_dist_fwd_kernel, dim3(nblk, B), dim3(NT), 0, s, (const bf16_t*)f, ld, w, B, P, C, rn, ws);
  SDMI_CHECK_LAUNCH();
  sdmi_rt::launch(lpips_dist_sum_kernel, dim3(B), dim3(64), 0, s, (const float*)ws, nblk, 1.0f / (float)P, accumulate,
                  val);
  SDMI_CHECK_LAUNCH();
  return 0;
}

extern "C" int sdmi_lpips_dist_bwd(const void* f, int ld, const float* w, const float* rn, const float* g, float gscale,
                                   int B, int P, int C, int side, const void* addend, int ld_add, void* dy, int ld_dy,
                                   sdmi_stream_t stream) {
  if (!f || !w || !rn || !dy || !tap_channels_ok(C) || ld < C || ld % 8 || ld_dy < C || ld_dy % 8 || B < 1 ||
      B > 65535 || P < 1 || (side != 0 && side != 1) || (addend && (ld_add < C || ld_add % 8)))
    return -1;
  const int ppb = dist_pixels_per_block(C);
  sdmi_rt::launch(lpips_dist_bwd_kernel, dim3((P + ppb - 1) / ppb, B), dim3(NT), 0, (hipStream_t)stream,
                  (const bf16_t*)f, ld, w, rn, g, gscale, B, P, C, side, (const bf16_t*)addend, ld_add, (bf16_t*)dy,
                  ld_dy);
  SDMI_CHECK_LAUNCH();
  return 0;
}

extern "C" int sdmi_lpips_mean(const float* val, int B, float scale, float* out, sdmi_stream_t stream) {
  if (!val || !out || B < 1) return -1;
  sdmi_rt::launch(lpips_mean_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, val, B, scale, out);
  SDMI_CHECK_LAUNCH();
  return 0;
}
