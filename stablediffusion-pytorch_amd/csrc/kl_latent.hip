// Latent interface of the KL autoencoder for gfx950 (reference models/vae.py:96-100 and the closed-form KL term):
//
//     moments = pre_quant_conv(h)                  (B, 2z, h, w): channels [0, z) the mean, [z, 2z) the log-variance
//     sample  = mean + exp(0.5 logvar) * eps
//     KL      = (1 / B) sum_b 0.5 sum_{c,h,w} (exp(logvar) + mean^2 - 1 - logvar)
//
// and their backward. z = z_channels, M = 2z <= 8 moment channels; P = B * HW pixels; fl() is one fp32 rounding.
//
//  kl_sample  : one thread per pixel. moments[co] = the fma chain from the bias (0 without one) over ci ascending of
//               w_pre[co][ci] * h[pix][ci], fp32 (never through bf16), written NCHW. std = expf(fl(0.5 * logvar));
//               sample = fl(mean + fl(std * eps)), nothing contracted; without eps the sample is the mean. With zin the
//               same pass writes post_quant_conv(sample) as the NHWC bf16 operand of decoder_conv_in with the arithmetic
//               of pointwise_in_kernel (vqvae.hip): the fma chain from the bias, ci ascending, RNE, pad columns zero.
//               With kl: term = fl(fl(fl(expf(logvar) + fl(mean * mean)) - 1) - logvar); a thread adds its terms in
//               grid-stride order, channels ascending; then the butterfly, then the four waves in order; one partial per
//               workgroup in ws.
//  kl_loss    : S = the partials through one butterfly and the four waves in order; kl = fl(fl(0.5 * S) / B).
//  kl_bwd     : per pixel, with c = fl(kw / B), kw = kl_weight (times the device scalar loss_w[0] when given):
//                 g       = W_post^T dzin (the fma chain from 0, co ascending), then fl(g + dsample_add)
//                 dmean   = fl(g + dmom_add_mean), then fl(dmean + fl(c * mean))                    (KL part only if c != 0)
//                 dlogvar = fl(fl(fl(g * eps) * 0.5) * std), then fl(. + dmom_add_logvar), then
//                           fl(. + fl(fl(c * 0.5) * fl(expf(logvar) - 1)))                         (0 from g without eps)
//                 dh[ci]  = the fma chain from 0 over co ascending of w_pre[co][ci] * dmom[co], RNE to bf16, pad columns 0
//               std is recomputed as in kl_sample (the same bits). Parameter gradients dW_post = sum_p dzin (x) sample,
//               db_post = sum_p dzin, dW_pre = sum_p dmom (x) h, db_pre = sum_p dmom: a thread accumulates its pixels
//               in grid-stride order (fma for the products), then the butterfly, then the four waves in order; one
//               partial row per workgroup in ws.
//  kl_bwd_finish: every gradient element = its partials added in workgroup order; every output fully overwritten.
//
// Host grid rule (both pixel kernels): 256 threads, min(256, ceil(P / 256)) workgroups, grid-stride. The two finishers are
// one workgroup of 256 threads. No atomics; every sum has a fixed order, so a second call repeats every bit.
#include "common.h"
#include "../../include/sdmi.h"
#include <algorithm>

namespace {

constexpr int KL_NT = 256, KL_WAVES = KL_NT / 64, KL_CAP = 256, MAXC = 8, MAXZ = MAXC / 2;
// per-workgroup partial row of the backward: dW_post (z x z), db_post (z), dW_pre (M x M), db_pre (M), at the caps
constexpr int KLB_WPOST = 0, KLB_BPOST = MAXZ * MAXZ, KLB_WPRE = KLB_BPOST + MAXZ, KLB_BPRE = KLB_WPRE + MAXC * MAXC,
              KLB_PART = KLB_BPRE + MAXC;

inline int pixel_blocks(long long P) { return (int)std::min<long long>(KL_CAP, (P + KL_NT - 1) / KL_NT); }

__device__ __forceinline__ float kl_std(float logvar) { return expf(mul_ieee(0.5f, logvar)); }

struct KlSampleArgs {
  const float* h; int ldh;          // encoder_conv_out output, NHWC fp32 [P][ldh], M valid channels
  const float* w_pre; const float* b_pre;  // pre_quant_conv (M, M), bias (M) or null
  const float* eps;                 // NCHW fp32 (B, z, HW) or null (the sample is the mean)
  int B, Z, HW;
  float* moments;                   // NCHW fp32 (B, M, HW)
  float* sample;                    // NCHW fp32 (B, z, HW)
  const float* w_post; const float* b_post;  // post_quant_conv (z, z), bias or null
  bf16_t* zin; int ld;              // NHWC bf16 [P][ld] or null
  float* partial;                   // one KL partial per workgroup, or null
};

__global__ __launch_bounds__(KL_NT) void kl_sample_kernel(const KlSampleArgs a) {
  __shared__ float red[KL_WAVES];
  const int Z = a.Z, M = 2 * a.Z;
  const long long P = (long long)a.B * a.HW;
  float acc = 0.f;
  for (long long pix = (long long)blockIdx.x * KL_NT + threadIdx.x; pix < P; pix += (long long)gridDim.x * KL_NT) {
    const long long bb = pix / a.HW, p = pix - bb * a.HW;
    float hin[MAXC], mom[MAXC], s[MAXZ];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) hin[c] = c < M ? a.h[pix * a.ldh + c] : 0.f;
#pragma unroll
    for (int co = 0; co < MAXC; ++co) {
      float v = 0.f;
      if (co < M) {
        v = a.b_pre ? a.b_pre[co] : 0.f;
#pragma unroll
        for (int ci = 0; ci < MAXC; ++ci)
          if (ci < M) v = fmaf(a.w_pre[co * M + ci], hin[ci], v);
        a.moments[(bb * M + co) * a.HW + p] = v;
      }
      mom[co] = v;
    }
#pragma unroll
    for (int c = 0; c < MAXZ; ++c) {
      s[c] = 0.f;
      if (c < Z) {
        // (mom[c + Z] with Z a runtime value would index the array dynamically: select instead)
        float lv = 0.f;
#pragma unroll
        for (int k = 0; k < MAXC; ++k) lv = (k == c + Z) ? mom[k] : lv;
        const float mean = mom[c];
        const long long i = (bb * Z + c) * a.HW + p;
        s[c] = a.eps ? add_ieee(mean, mul_ieee(kl_std(lv), a.eps[i])) : mean;
        a.sample[i] = s[c];
        if (a.partial) {
          const float t = sub_ieee(sub_ieee(add_ieee(expf(lv), mul_ieee(mean, mean)), 1.0f), lv);
          acc = add_ieee(acc, t);
        }
      }
    }
    if (a.zin) {
#pragma unroll
      for (int co = 0; co < MAXC; ++co) {
        if (co >= a.ld) break;
        float v = 0.f;
        if (co < Z) {
          v = a.b_post ? a.b_post[co] : 0.f;
#pragma unroll
          for (int ci = 0; ci < MAXZ; ++ci)
            if (ci < Z) v = fmaf(a.w_post[co * Z + ci], s[ci], v);
        }
        a.zin[pix * a.ld + co] = f2bf(v);
      }
      for (int co = MAXC; co < a.ld; ++co) a.zin[pix * a.ld + co] = 0;
    }
  }
  if (a.partial) {  // (kernel-uniform)
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) a.partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
  }
}

__global__ __launch_bounds__(KL_NT) void kl_loss_kernel(const float* partial, int parts, int B, float* kl) {
  __shared__ float red[KL_WAVES];
  float v = (int)threadIdx.x < parts ? partial[threadIdx.x] : 0.f;
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float S = ((red[0] + red[1]) + red[2]) + red[3];
    *kl = mul_ieee(0.5f, S) / (float)B;
  }
}

struct KlBwdArgs {
  const bf16_t* dzin; int ld_dzin;  // gradient of post_quant_conv's output, NHWC bf16 [P][ld], or null
  const float* w_post;              // (z, z)
  const float* sample;              // NCHW fp32 (B, z, HW): post_quant_conv's input
  const float* moments;             // NCHW fp32 (B, M, HW)
  const float* eps;                 // NCHW fp32 (B, z, HW) or null
  const float* h; int ldh;          // pre_quant_conv's input, NHWC fp32 [P][ldh], or null (no dW_pre)
  const float* w_pre;               // (M, M), or null (no dh)
  int B, Z, HW;
  float kl_weight; const float* loss_w;
  const float* dsample_add;         // NCHW fp32 (B, z, HW) or null
  const float* dmom_add;            // NCHW fp32 (B, M, HW) or null
  bf16_t* dh; int ld_out;           // NHWC bf16 [P][ld_out] or null
  float* dmom;                      // NCHW fp32 (B, M, HW) or null
  float* partial;                   // [workgroups][KLB_PART]
};

__global__ __launch_bounds__(KL_NT) void kl_bwd_kernel(const KlBwdArgs a) {
  __shared__ float red[KL_WAVES][KLB_PART];
  const int Z = a.Z, M = 2 * a.Z;
  const long long P = (long long)a.B * a.HW;
  const float kw = a.loss_w ? mul_ieee(a.kl_weight, a.loss_w[0]) : a.kl_weight;
  const float c = kw / (float)a.B, ch = mul_ieee(c, 0.5f);
  float acc[KLB_PART];
#pragma unroll
  for (int i = 0; i < KLB_PART; ++i) acc[i] = 0.f;
  for (long long pix = (long long)blockIdx.x * KL_NT + threadIdx.x; pix < P; pix += (long long)gridDim.x * KL_NT) {
    const long long bb = pix / a.HW, p = pix - bb * a.HW;
    float dzin[MAXZ], smp[MAXZ], dmom[MAXC], hin[MAXC];
#pragma unroll
    for (int k = 0; k < MAXZ; ++k) {
      const bool on = k < Z && a.dzin;
      dzin[k] = on ? bf2f(a.dzin[pix * a.ld_dzin + k]) : 0.f;
      smp[k] = on ? a.sample[(bb * Z + k) * a.HW + p] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < MAXC; ++k) {
      dmom[k] = 0.f;
      hin[k] = (a.h && k < M) ? a.h[pix * a.ldh + k] : 0.f;
    }
#pragma unroll
    for (int ci = 0; ci < MAXZ; ++ci) {
      if (ci < Z) {
        const long long i = (bb * Z + ci) * a.HW + p;
        const long long im = (bb * M + ci) * a.HW + p, il = im + (long long)Z * a.HW;
        float g = 0.f;
        if (a.dzin) {
#pragma unroll
          for (int co = 0; co < MAXZ; ++co)
            if (co < Z) g = fmaf(a.w_post[co * Z + ci], dzin[co], g);
        }
        if (a.dsample_add) g = add_ieee(g, a.dsample_add[i]);
        const float mean = a.moments[im], lv = a.moments[il];
        float dm = g, dl = 0.f;
        if (a.eps) dl = mul_ieee(mul_ieee(mul_ieee(g, a.eps[i]), 0.5f), kl_std(lv));
        if (a.dmom_add) {
          dm = add_ieee(dm, a.dmom_add[im]);
          dl = add_ieee(dl, a.dmom_add[il]);
        }
        if (c != 0.f) {
          dm = add_ieee(dm, mul_ieee(c, mean));
          dl = add_ieee(dl, mul_ieee(ch, sub_ieee(expf(lv), 1.0f)));
        }
        if (a.dmom) {
          a.dmom[im] = dm;
          a.dmom[il] = dl;
        }
#pragma unroll
        for (int k = 0; k < MAXC; ++k) {  // (static indices: dmom[ci] and dmom[ci + Z])
          dmom[k] = (k == ci) ? dm : dmom[k];
          dmom[k] = (k == ci + Z) ? dl : dmom[k];
        }
      }
    }
#pragma unroll
    for (int co = 0; co < MAXZ; ++co) {
#pragma unroll
      for (int ci = 0; ci < MAXZ; ++ci)
        acc[KLB_WPOST + co * MAXZ + ci] = fmaf(dzin[co], smp[ci], acc[KLB_WPOST + co * MAXZ + ci]);
      acc[KLB_BPOST + co] = add_ieee(acc[KLB_BPOST + co], dzin[co]);
    }
#pragma unroll
    for (int co = 0; co < MAXC; ++co) {
#pragma unroll
      for (int ci = 0; ci < MAXC; ++ci)
        acc[KLB_WPRE + co * MAXC + ci] = fmaf(dmom[co], hin[ci], acc[KLB_WPRE + co * MAXC + ci]);
      acc[KLB_BPRE + co] = add_ieee(acc[KLB_BPRE + co], dmom[co]);
    }
    if (a.dh) {
#pragma unroll
      for (int ci = 0; ci < MAXC; ++ci) {
        if (ci >= a.ld_out) break;
        float s = 0.f;
        if (ci < M) {
#pragma unroll
          for (int co = 0; co < MAXC; ++co)
            if (co < M) s = fmaf(a.w_pre[co * M + ci], dmom[co], s);
        }
        a.dh[pix * a.ld_out + ci] = f2bf(s);
      }
      for (int ci = MAXC; ci < a.ld_out; ++ci) a.dh[pix * a.ld_out + ci] = 0;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < KLB_PART; ++i) {
    const float v = wave_sum(acc[i]);
    if (lane == 0) red[wave][i] = v;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < KLB_PART; i += KL_NT)
    a.partial[(long long)blockIdx.x * KLB_PART + i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
}

// the partial rows added in workgroup order, scattered to the four gradient tensors (z x z, z, M x M, M)
__global__ __launch_bounds__(KL_NT) void kl_bwd_finish_kernel(const float* partial, int blocks, int Z, float* dw_post,
                                                              float* db_post, float* dw_pre, float* db_pre) {
  const int M = 2 * Z;
  for (int i = threadIdx.x; i < KLB_PART; i += KL_NT) {
    float v = 0.f;
    for (int b = 0; b < blocks; ++b) v = add_ieee(v, partial[(long long)b * KLB_PART + i]);
    if (i < KLB_BPOST) {
      const int co = i / MAXZ, ci = i % MAXZ;
      if (co < Z && ci < Z && dw_post) dw_post[co * Z + ci] = v;
    } else if (i < KLB_WPRE) {
      const int co = i - KLB_BPOST;
      if (co < Z && db_post) db_post[co] = v;
    } else if (i < KLB_BPRE) {
      const int j = i - KLB_WPRE, co = j / MAXC, ci = j % MAXC;
      if (co < M && ci < M && dw_pre) dw_pre[co * M + ci] = v;
    } else {
      const int co = i - KLB_BPRE;
      if (co < M && db_pre) db_pre[co] = v;
    }
  }
}

}  // namespace

// one KL partial per pixel workgroup
extern "C" size_t sdmi_kl_workspace(long long pixels) {
  return pixels > 0 ? (size_t)pixel_blocks(pixels) * sizeof(float) : 0;
}

extern "C" size_t sdmi_kl_bwd_workspace(void) { return (size_t)KL_CAP * KLB_PART * sizeof(float); }

extern "C" int sdmi_kl_sample(const float* h, int ldh, const float* w_pre, const float* b_pre, const float* eps, int B,
                              int z, int HW, float* moments, float* sample, const float* w_post, const float* b_post,
                              void* zin, int ld, float* ws, float* kl, sdmi_stream_t stream) {
  if (!h || !w_pre || !moments || !sample || B <= 0 || z <= 0 || 2 * z > MAXC || HW <= 0 || ldh < 2 * z) return -1;
  const long long P = (long long)B * HW;
  if (P * 2 * z > 0x7fffffffLL) return -1;
  if (zin && (!w_post || ld < z)) return -1;
  if (kl && !ws) return -1;
  KlSampleArgs a;
  a.h = h; a.ldh = ldh; a.w_pre = w_pre; a.b_pre = b_pre; a.eps = eps; a.B = B; a.Z = z; a.HW = HW;
  a.moments = moments; a.sample = sample; a.w_post = w_post; a.b_post = b_post; a.zin = (bf16_t*)zin; a.ld = ld;
  a.partial = kl ? ws : nullptr;
  const int pb = pixel_blocks(P);
  sdmi_rt::launch(kl_sample_kernel, dim3(pb), dim3(KL_NT), 0, (hipStream_t)stream, a);
  SDMI_CHECK_LAUNCH();
  if (kl) {
    sdmi_rt::launch(kl_loss_kernel, dim3(1), dim3(KL_NT), 0, (hipStream_t)stream, (const float*)ws, pb, B, kl);
    SDMI_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int sdmi_kl_bwd(const void* dzin, int ld_dzin, const float* w_post, const float* sample,
                           const float* moments, const float* eps, const float* h, int ldh, const float* w_pre, int B,
                           int z, int HW, float kl_weight, const float* loss_w, const float* dsample_add,
                           const float* dmom_add, void* dh, int ld_out, float* dmom, float* ws, float* dw_post,
                           float* db_post, float* dw_pre, float* db_pre, sdmi_stream_t stream) {
  if (!moments || !ws || B <= 0 || z <= 0 || 2 * z > MAXC || HW <= 0) return -1;
  const long long P = (long long)B * HW;
  if (P * 2 * z > 0x7fffffffLL) return -1;
  if (dzin && (!w_post || !sample || ld_dzin < z)) return -1;
  if (!dzin && (dw_post || db_post)) return -1;
  if (dh && (!w_pre || ld_out < 2 * z)) return -1;
  if (dw_pre && (!h || ldh < 2 * z)) return -1;
  if (!dh && !dmom && !dw_pre && !db_pre && !dw_post && !db_post) return -1;
  KlBwdArgs a;
  a.dzin = (const bf16_t*)dzin; a.ld_dzin = ld_dzin; a.w_post = w_post; a.sample = sample; a.moments = moments;
  a.eps = eps; a.h = dw_pre ? h : nullptr; a.ldh = ldh; a.w_pre = w_pre; a.B = B; a.Z = z; a.HW = HW;
  a.kl_weight = kl_weight; a.loss_w = loss_w; a.dsample_add = dsample_add; a.dmom_add = dmom_add;
  a.dh = (bf16_t*)dh; a.ld_out = ld_out; a.dmom = dmom; a.partial = ws;
  const int pb = pixel_blocks(P);
  sdmi_rt::launch(kl_bwd_kernel, dim3(pb), dim3(KL_NT), 0, (hipStream_t)stream, a);
  SDMI_CHECK_LAUNCH();
  sdmi_rt::launch(kl_bwd_finish_kernel, dim3(1), dim3(KL_NT), 0, (hipStream_t)stream, (const float*)ws, pb, z, dw_post,
                  db_post, dw_pre, db_pre);
  SDMI_CHECK_LAUNCH();
  return 0;
}
