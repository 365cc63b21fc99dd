// Learned-step-size (LSQ) quantisers of the reference's quantise-and-noise layers for gfx950
// (cim_layers/quant_noise_utils.py:51-54, 66-69, 101-120; layers_utils_lsq.py:31-83):
//
//     se = (s - s*g).detach() + s*g            grad_scale: the step's forward value, g = fp32(1 / sqrt(Qp * numel))
//     v  = x / se,  c = clamp(v, -Qp, Qp),  q = round(c),  y = q * se
//
// and the backward autograd derives from it. Everything is fp32 with every operation rounded on its own (fl()):
//
//  se       = fl(fl(s - fl(s g)) + fl(s g)); a null step pointer (a quantiser that is switched off) is se = 1.
//  forward  : v = fl(x / se); c = v below -Qp ? -Qp : v above Qp ? Qp : v (a NaN passes); q = fl(fl(rint(c) - c) + c),
//             round_pass's expression: rint(c), ties to even, with a zero result always +0 (torch gives +0 for -0.3 and
//             for -0.0); y = fl(q se).
//  dx       = fl((inside ? fl(dy se) : 0) / se), inside = v >= -Qp && v <= Qp (both ends inclusive, a NaN v outside).
//  ds       = fl(S g), S = sum t_i, t_i = fl(dy_i fl(q_i - v_i)) inside (q - v is exact), fl(dy_i q_i) outside.
//  S        : a thread adds its terms in the order it meets them (below), then the butterfly over the wave, then the
//             four waves in order -> one partial per workgroup; the finisher (one workgroup) puts the partials through
//             one butterfly and the four waves in order. No atomics: a second call repeats every bit.
//  init     : range = max |x| (NaN if any), step = fl(1 / fl(fl(1 / range) Qp)); range == 0 leaves the step as it is.
//
// The steps are read from device memory by every kernel; no launch argument depends on a step's value.
//
// Host grid rules. Flat kernels (quant_fwd, quant_bwd, in_bwd, out_fwd, scale, absmax): 256 threads, a workgroup
// spans 1024 consecutive elements per trip -- thread t owns elements 4t .. 4t+3 of the span, one 16-byte access where
// the pointers are 16-byte aligned and the four lie inside, the same elements one by one otherwise (the same order of
// additions either way) -- min(256, ceil(n / 1024)) workgroups, grid-stride. Row kernels (in_fwd, out_bwd): one thread per
// (pixel, group of 8 channels), 16-byte bf16 stores, min(256, ceil(items / 256)) workgroups, grid-stride, item =
// group * pixels + pixel so neighbouring threads read neighbouring pixels of one NCHW channel.
#include "lsq_device.h"
#include "../../include/sdmi.h"

namespace {

__global__ __launch_bounds__(LQ_NT) void lsq_quant_fwd_kernel(const float* x, long long n, Step st, float qp, float* y,
                                                              float* codes, bool vec) {
  const float se = eff_step(st);
  LQ_FLAT_LOOP(n) {
    float xv[4], yv[4], cv[4];
    load4(x, i0, n, vec, xv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const Q e = quant(xv[k], se, qp);
      cv[k] = e.q;
      yv[k] = mul_ieee(e.q, se);
    }
    if (y) store4(y, i0, n, vec, yv);
    if (codes) store4(codes, i0, n, vec, cv);
  }
}

// dy is first scaled by the effective step `sc` of the other GEMM operand (se = 1 when sc.s is null)
__global__ __launch_bounds__(LQ_NT) void lsq_quant_bwd_kernel(const float* x, const float* dy, long long n, Step st,
                                                              float qp, Step sc, float* dx, float* partial, bool vec) {
  __shared__ float red[LQ_WAVES];
  const float se = eff_step(st), ssc = eff_step(sc);
  float acc = 0.f;
  LQ_FLAT_LOOP(n) {
    float xv[4], gv[4], dv[4];
    load4(x, i0, n, vec, xv);
    load4(dy, i0, n, vec, gv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float t = 0.f;
      const float g = sc.s ? mul_ieee(ssc, gv[k]) : gv[k];
      dv[k] = quant_bwd(quant(xv[k], se, qp), g, se, t);
      if (i0 + k < n) acc = add_ieee(acc, t);
    }
    store4(dx, i0, n, vec, dv);
  }
  block_partial(acc, red, partial);
}

// fp32 (B, C, P) -> NHWC bf16 codes [B*P][ld], columns >= C zero. item = group * BP + pixel.
__global__ __launch_bounds__(LQ_NT) void lsq_in_fwd_kernel(const float* x, int B, int C, int P, Step st, float qp,
                                                           bf16_t* out, int ld) {
  const float se = eff_step(st);
  const long long BP = (long long)B * P, items = BP * (ld / 8);
  for (long long it = (long long)blockIdx.x * LQ_NT + threadIdx.x; it < items; it += (long long)gridDim.x * LQ_NT) {
    const long long grp = it / BP, bp = it - grp * BP;
    const long long b = bp / P, p = bp - b * P;
    float f[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = (int)grp * 8 + k;
      f[k] = c < C ? quant(x[(b * C + c) * P + p], se, qp).q : 0.0f;
    }
    *(uint4*)(out + bp * ld + grp * 8) = pack8(f);
  }
}

// the input quantiser's backward on the data-gradient GEMM's result G (NHWC fp32 [B*P][ld]), written (B, C, P)
__global__ __launch_bounds__(LQ_NT) void lsq_in_bwd_kernel(const float* x, const float* G, int ld, int C, int P,
                                                           long long n, Step st, float qp, Step sc, float* dx,
                                                           float* partial, bool vec) {
  __shared__ float red[LQ_WAVES];
  const float se = eff_step(st), ssc = eff_step(sc);
  float acc = 0.f;
  LQ_FLAT_LOOP(n) {
    float xv[4], dv[4];
    load4(x, i0, n, vec, xv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long long i = i0 + k;
      dv[k] = 0.f;
      if (i < n) {
        const long long bc = i / P, p = i - bc * P, b = bc / C, c = bc - b * C;
        const float gr = G[(b * P + p) * ld + c];
        const float g = sc.s ? mul_ieee(ssc, gr) : gr;
        float t;
        dv[k] = quant_bwd(quant(xv[k], se, qp), g, se, t);
        acc = add_ieee(acc, t);
      }
    }
    store4(dx, i0, n, vec, dv);
  }
  block_partial(acc, red, partial);
}

// output stage over the GEMM's fp32 NHWC accumulator: pre = fl(fl(acc f) + bias[c]), f = fl(se_in se_w), kept in place
// of acc (have_pre: acc already holds pre); y (B, C, P) = the output quantiser of pre, or pre itself when qp == 0.
__global__ __launch_bounds__(LQ_NT) void lsq_out_fwd_kernel(float* acc, int ld, int C, int P, long long n, Step s_in,
                                                            Step s_w, const float* bias, Step s_out, float qp,
                                                            int have_pre, float* y, bool vec) {
  const float f = mul_ieee(eff_step(s_in), eff_step(s_w));
  const float se = eff_step(s_out);
  LQ_FLAT_LOOP(n) {
    float yv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long long i = i0 + k;
      yv[k] = 0.f;
      if (i < n) {
        const long long bc = i / P, p = i - bc * P, b = bc / C, c = bc - b * C;
        float* a = acc + (b * P + p) * ld + c;
        float pre = *a;
        if (!have_pre) {
          pre = mul_ieee(pre, f);
          if (bias) pre = add_ieee(pre, bias[c]);
          *a = pre;
        }
        yv[k] = qp > 0.f ? mul_ieee(quant(pre, se, qp).q, se) : pre;
      }
    }
    store4(y, i0, n, vec, yv);
  }
}

// output quantiser's backward: dy (B, C, P) fp32 and pre (NHWC fp32 [B*P][ld]) -> d_pre NHWC bf16 [B*P][ld_d]
// (columns >= C zero) and the partials of ds_out; a thread adds its items' terms in grid-stride order, channels ascending
__global__ __launch_bounds__(LQ_NT) void lsq_out_bwd_kernel(const float* pre, int ld, const float* dy, int B, int C,
                                                            int P, Step st, float qp, bf16_t* dpre, int ld_d,
                                                            float* partial) {
  __shared__ float red[LQ_WAVES];
  const float se = eff_step(st);
  const long long BP = (long long)B * P, items = BP * (ld_d / 8);
  float acc = 0.f;
  for (long long it = (long long)blockIdx.x * LQ_NT + threadIdx.x; it < items; it += (long long)gridDim.x * LQ_NT) {
    const long long grp = it / BP, bp = it - grp * BP;
    const long long b = bp / P, p = bp - b * P;
    float f[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = (int)grp * 8 + k;
      f[k] = 0.f;
      if (c < C) {
        float t;
        f[k] = quant_bwd(quant(pre[bp * ld + c], se, qp), dy[(b * C + c) * P + p], se, t);
        acc = add_ieee(acc, t);
      }
    }
    *(uint4*)(dpre + bp * ld_d + grp * 8) = pack8(f);
  }
  block_partial(acc, red, partial);
}

__global__ __launch_bounds__(LQ_NT) void lsq_scale_kernel(const float* x, long long n, Step st, int divide, float* out,
                                                          bool vec) {
  const float se = eff_step(st);
  LQ_FLAT_LOOP(n) {
    float xv[4];
    load4(x, i0, n, vec, xv);
#pragma unroll
    for (int k = 0; k < 4; ++k) xv[k] = divide ? div_ieee(xv[k], se) : mul_ieee(xv[k], se);
    store4(out, i0, n, vec, xv);
  }
}

__global__ __launch_bounds__(LQ_NT) void lsq_init_finish_kernel(const float* partial, int parts, float qp, float* step) {
  float m;
  int nan;
  absmax_finish(partial, parts, m, nan);
  if (threadIdx.x == 0) {
    if (nan) {
      step[0] = __int_as_float(0x7fc00000);
    } else if (m != 0.f) {
      step[0] = div_ieee(1.0f, mul_ieee(div_ieee(1.0f, m), qp));
    }
  }
}

}  // namespace

extern "C" size_t sdmi_lsq_workspace(void) { return (size_t)LQ_CAP * sizeof(float); }

extern "C" int sdmi_lsq_quant_fwd(const float* x, long long n, const float* step, float g, int qp, float* y,
                                  float* codes, sdmi_stream_t stream) {
  if (!x || !step || (!y && !codes) || n <= 0 || n > 0x7fffffffLL || !qp_ok(qp)) return -1;
  const bool vec = al16(x) && (!y || al16(y)) && (!codes || al16(codes));
  sdmi_rt::launch(lsq_quant_fwd_kernel, dim3(flat_blocks(n)), dim3(LQ_NT), 0, (hipStream_t)stream, x, n, Step{step, g},
                  (float)qp, y, codes, vec);
  SDMI_CHECK_LAUNCH();
  return 0;
}

extern "C" int sdmi_lsq_quant_bwd(const float* x, const float* dy, long long n, const float* step, float g, int qp,
                                  const float* scale_step, float scale_g, float* dx, float* ws, float* ds,
                                  sdmi_stream_t stream) {
  if (!x || !dy || !step || !dx || !ws || !ds || n <= 0 || n > 0x7fffffffLL || !qp_ok(qp)) return -1;
  const bool vec = al16(x) && al16(dy) && al16(dx);
  const int nb = flat_blocks(n);
  sdmi_rt::launch(lsq_quant_bwd_kernel, dim3(nb), dim3(LQ_NT), 0, (hipStream_t)stream, x, dy, n, Step{step, g},
                  (float)qp, Step{scale_step, scale_g}, dx, ws, vec);
  SDMI_CHECK_LAUNCH();
  sdmi_rt::launch(lsq_finish_kernel, dim3(1), dim3(LQ_NT), 0, (hipStream_t)stream, (const float*)ws, nb, g, ds);
  SDMI_CHECK_LAUNCH();
  return 0;
}

extern "C" int sdmi_lsq_in_fwd(const float* x, int B, int C, int P, const float* step, float g, int qp, void* codes,
                               int ld, sdmi_stream_t stream) {
  if (!x || !step || !codes || B <= 0 || C <= 0 || P <= 0 || ld < C || ld % 8 || !al16(codes) || !qp_ok(qp)) return -1;
  const long long BP = (long long)B * P;
  if (BP * ld > 0x7fffffffLL) return -1;
  sdmi_rt::launch(lsq_in_fwd_kernel, dim3(item_blocks(BP * (ld / 8))), dim3(LQ_NT), 0, (hipStream_t)stream, x, B, C, P,
                  Step{step, g}, (float)qp, (bf16_t*)codes, ld);
  SDMI_CHECK_LAUNCH();
  return 0;
}

extern "C" int sdmi_lsq_in_bwd(const float* x, const float* G, int ld, int B, int C, int P, const float* step, float g,
                               int qp, const float* scale_step, float scale_g, float* dx, float* ws, float* ds,
                               sdmi_stream_t stream) {
  if (!x || !G || !step || !dx || !ws || !ds || B <= 0 || C <= 0 || P <= 0 || ld < C || !qp_ok(qp)) return -1;
  const long long n = (long long)B * C * P;
  if ((long long)B * P * ld > 0x7fffffffLL) return -1;
  const bool vec = al16(x) && al16(dx);
  const int nb = flat_blocks(n);
  sdmi_rt::launch(lsq_in_bwd_kernel, dim3(nb), dim3(LQ_NT), 0, (hipStream_t)stream, x, G, ld, C, P, n, Step{step, g},
                  (float)qp, Step{scale_step, scale_g}, dx, ws, vec);
  SDMI_CHECK_LAUNCH();
  sdmi_rt::launch(lsq_finish_kernel, dim3(1), dim3(LQ_NT), 0, (hipStream_t)stream, (const float*)ws, nb, g, ds);
  SDMI_CHECK_LAUNCH();
  return 0;
}

extern "C" int sdmi_lsq_out_fwd(float* acc, int ld, int B, int C, int P, const float* step_in, float g_in,
                                const float* step_w, float g_w, const float* bias, const float* step_out, float g_out,
                                int qp, int have_pre, float* y, sdmi_stream_t stream) {
  if (!acc || !y || B <= 0 || C <= 0 || P <= 0 || ld < C) return -1;
  if (qp != 0 && (!qp_ok(qp) || !step_out)) return -1;
  const long long n = (long long)B * C * P;
  if ((long long)B * P * ld > 0x7fffffffLL) return -1;
  sdmi_rt::launch(lsq_out_fwd_kernel, dim3(flat_blocks(n)), dim3(LQ_NT), 0, (hipStream_t)stream, acc, ld, C, P, n,
                  Step{step_in, g_in}, Step{step_w, g_w}, bias, Step{qp ? step_out : nullptr, g_out}, (float)qp,
                  have_pre, y, al16(y));
  SDMI_CHECK_LAUNCH();
  return 0;
}

extern "C" int sdmi_lsq_out_bwd(const float* pre, int ld, const float* dy, int B, int C, int P, const float* step,
                                float g, int qp, void* dpre, int ld_d, float* ws, float* ds, sdmi_stream_t stream) {
  if (!pre || !dy || !step || !dpre || !ws || !ds || B <= 0 || C <= 0 || P <= 0 || ld < C || ld_d < C || ld_d % 8 ||
      !al16(dpre) || !qp_ok(qp))
    return -1;
  const long long BP = (long long)B * P;
  if (BP * ld > 0x7fffffffLL || BP * ld_d > 0x7fffffffLL) return -1;
  const int nb = item_blocks(BP * (ld_d / 8));
  sdmi_rt::launch(lsq_out_bwd_kernel, dim3(nb), dim3(LQ_NT), 0, (hipStream_t)stream, pre, ld, dy, B, C, P, Step{step, g},
                  (float)qp, (bf16_t*)dpre, ld_d, ws);
  SDMI_CHECK_LAUNCH();
  sdmi_rt::launch(lsq_finish_kernel, dim3(1), dim3(LQ_NT), 0, (hipStream_t)stream, (const float*)ws, nb, g, ds);
  SDMI_CHECK_LAUNCH();
  return 0;
}

extern "C" int sdmi_lsq_scale(const float* x, long long n, const float* step, float g, int divide, float* out,
                              sdmi_stream_t stream) {
  if (!x || !step || !out || n <= 0 || n > 0x7fffffffLL) return -1;
  sdmi_rt::launch(lsq_scale_kernel, dim3(flat_blocks(n)), dim3(LQ_NT), 0, (hipStream_t)stream, x, n, Step{step, g},
                  divide, out, al16(x) && al16(out));
  SDMI_CHECK_LAUNCH();
  return 0;
}

extern "C" int sdmi_lsq_init_step(const float* x, long long n, int qp, float* ws, float* step, sdmi_stream_t stream) {
  if (!x || !ws || !step || n <= 0 || n > 0x7fffffffLL || !qp_ok(qp)) return -1;
  const int nb = flat_blocks(n);
  sdmi_rt::launch(lsq_absmax_kernel, dim3(nb), dim3(LQ_NT), 0, (hipStream_t)stream, x, n, ws, al16(x));
  SDMI_CHECK_LAUNCH();
  sdmi_rt::launch(lsq_init_finish_kernel, dim3(1), dim3(LQ_NT), 0, (hipStream_t)stream, (const float*)ws, nb, (float)qp,
                  step);
  SDMI_CHECK_LAUNCH();
  return 0;
}
