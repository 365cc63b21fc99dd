// Device side of the LSQ quantiser shared by csrc/lsq.hip and csrc/adda.hip: the effective step, one element's forward
// and backward, the 4-element flat accesses, the per-workgroup partial and its one-workgroup finishers. The arithmetic
// and the host grid rules are stated at the top of lsq.hip. Everything sits in an anonymous namespace: each translation
// unit gets its own copy of the kernels.
#pragma once
#include "common.h"
#include <algorithm>

namespace {

constexpr int LQ_NT = 256, LQ_WAVES = LQ_NT / 64, LQ_SPAN = 4 * LQ_NT, LQ_CAP = 256;

inline int flat_blocks(long long n) { return (int)std::min<long long>(LQ_CAP, (n + LQ_SPAN - 1) / LQ_SPAN); }
inline int item_blocks(long long n) { return (int)std::min<long long>(LQ_CAP, (n + LQ_NT - 1) / LQ_NT); }
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct Step {
  const float* s;  // device scalar, or null: se = 1
  float g;
};

__device__ __forceinline__ float div_ieee(float a, float b) { return __fdiv_rn(a, b); }

__device__ __forceinline__ float eff_step(const Step st) {
  if (!st.s) return 1.0f;
  const float s = *st.s, sg = mul_ieee(s, st.g);
  return add_ieee(sub_ieee(s, sg), sg);
}

struct Q {
  float v, q;
  bool inside;
};

__device__ __forceinline__ Q quant(float x, float se, float qp) {
  Q r;
  r.v = div_ieee(x, se);
  const float c = r.v < -qp ? -qp : (r.v > qp ? qp : r.v);
  r.q = add_ieee(sub_ieee(rintf(c), c), c);  // round_pass: rint(c) with a zero result always +0
  r.inside = r.v >= -qp && r.v <= qp;
  return r;
}

// dx and the step-gradient term of one element with upstream gradient g
__device__ __forceinline__ float quant_bwd(const Q e, float g, float se, float& t) {
  t = mul_ieee(g, e.inside ? sub_ieee(e.q, e.v) : e.q);
  return div_ieee(e.inside ? mul_ieee(g, se) : 0.0f, se);
}

__device__ __forceinline__ void load4(const float* p, long long i0, long long n, bool vec, float* v) {
  if (vec && i0 + 3 < n) {
    const float4 t = *(const float4*)(p + i0);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i0 + k < n ? p[i0 + k] : 0.0f;
  }
}

__device__ __forceinline__ void store4(float* p, long long i0, long long n, bool vec, const float* v) {
  if (vec && i0 + 3 < n) {
    *(float4*)(p + i0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i0 + k < n) p[i0 + k] = v[k];
  }
}

// one partial per workgroup: the butterfly, then the four waves in order
__device__ __forceinline__ void block_partial(float acc, float* red, float* partial) {
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

#define LQ_FLAT_LOOP(n)                                                                                              \
  for (long long i0 = (long long)blockIdx.x * LQ_SPAN + 4 * threadIdx.x; i0 < (n); i0 += (long long)gridDim.x * LQ_SPAN)

__global__ __launch_bounds__(LQ_NT) void lsq_finish_kernel(const float* partial, int parts, float g, float* ds) {
  __shared__ float red[LQ_WAVES];
  float v = (int)threadIdx.x < parts ? partial[threadIdx.x] : 0.f;
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) ds[0] = mul_ieee(((red[0] + red[1]) + red[2]) + red[3], g);
}

// max |x| per workgroup (exact in any order); a NaN anywhere makes the partial NaN
__global__ __launch_bounds__(LQ_NT) void lsq_absmax_kernel(const float* x, long long n, float* partial, bool vec) {
  __shared__ float red[LQ_WAVES];
  __shared__ int rnan[LQ_WAVES];
  float m = 0.f;
  int nan = 0;
  LQ_FLAT_LOOP(n) {
    float xv[4];
    load4(x, i0, n, vec, xv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      nan |= (xv[k] != xv[k]);
      const float a = fabsf(xv[k]);
      m = a > m ? a : m;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float b = __shfl_xor(m, o, 64);
    m = b > m ? b : m;
    nan |= __shfl_xor(nan, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = m;
    rnan[threadIdx.x >> 6] = nan;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < LQ_WAVES; ++w) {
      m = red[w] > m ? red[w] : m;
      nan |= rnan[w];
    }
    partial[blockIdx.x] = nan ? __int_as_float(0x7fc00000) : m;
  }
}

// max over the workgroups' partials into *out_max / *out_nan of thread 0 (the other threads' values are unspecified)
__device__ __forceinline__ void absmax_finish(const float* partial, int parts, float& out_max, int& out_nan) {
  __shared__ float red[LQ_WAVES];
  __shared__ int rnan[LQ_WAVES];
  float m = (int)threadIdx.x < parts ? partial[threadIdx.x] : 0.f;
  int nan = m != m;
  m = nan ? 0.f : m;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float b = __shfl_xor(m, o, 64);
    m = b > m ? b : m;
    nan |= __shfl_xor(nan, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = m;
    rnan[threadIdx.x >> 6] = nan;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < LQ_WAVES; ++w) {
      m = red[w] > m ? red[w] : m;
      nan |= rnan[w];
    }
  }
  out_max = m;
  out_nan = nan;
}

inline bool qp_ok(int qp) { return qp >= 1 && qp <= 255; }  // bit widths 2 .. 9

}  // namespace
