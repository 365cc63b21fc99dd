// GroupNorm (+ fused SiLU) forward/backward and per-(batch, channel) pixel reductions on NHWC bf16.
//
// Replaces nn.GroupNorm(32, C) -> nn.SiLU() (models/blocks.py:45-47, 64-66 and the Mid/Up copies),
// the attention pre-norms on the (B, C, HW) view (blocks.py:124-126, 137-139: same statistics as
// 4-D) and unet_cond_base.py:179-180. Statistics: fp32 per-thread / per-channel sums, fp64 group merge,
// eps 1e-5.
//
// All kernels see an activation as x[b][p][c] = x[(b*P + p)*ld + c], P = H*W pixels. A workgroup owns a channel
// strip of one batch row (for GroupNorm a strip of whole groups), so per-(b, c) and per-(b, g) results come out of
// the workgroup directly. Sums over the batch (dgamma/dbeta, bias gradients) are finished by the last-arriving
// workgroup of each strip: rows are published with device-coherent (sc1) stores and a relaxed device-scope arrival
// counter, so no L2 write-back fence is needed.
//   sdmi_gn_fwd       : y = act(GroupNorm(x)) and the table {a = rstd*gamma, s = beta - mean*a, mean, rstd} per (b, c):
//                       one single-pass launch when a workgroup's slab fits its registers (pick_pass), else the
//                       statistics reduction (sdmi_gn_stats) and the elementwise pass (sdmi_gn_apply)
//   sdmi_gn_bwd       : dx = a*dz + q*x + o (+ addend) and dgamma/dbeta: one single-pass launch under the same rule,
//                       else the reduction (sum dz, sum dz*xhat) -> table2 {a, s, q, o} and the elementwise pass
//   sdmi_gn_bwd_part  : the same from the producing GEMM's segment statistics, one streaming launch
//   sdmi_gn_bwd_rows, sdmi_gn_bwd_part_rows, sdmi_gn_rows_sum(_grouped): dgamma/dbeta deferred to a later launch
//   sdmi_chan_sum     : per-(b, c) and per-c sums of dy (bias / time-embedding gradients)
// Top to bottom: shared device helpers, reduction, single-pass and streaming kernels, launch-shape selection, C ABI.
#include <atomic>
#include <cstdlib>

#include "common.h"
#include "../../include/sdmi.h"

namespace {

constexpr int NT = 256;
constexpr int NSLOTS = 2048;      // counter slots, one per launch, round-robin
constexpr int SLOT_CTRS = 2048;   // [0, 1024): per (strip, b) pixel-split counters, [1024, 2048): per strip
constexpr int BATCH_CTR = 1024;
constexpr int PS_MAX = 32;        // pixel splits per (strip, b) (small batches of large images: VQVAE B = 8 at 256^2)
__device__ unsigned g_norm_counters[NSLOTS * SLOT_CTRS];  // zero at load; the last arriver re-arms

struct StripArgs {
  const bf16_t* x; int ldx;   // GN input (modes 0, 1)
  const bf16_t* dy; int ldy;  // upstream gradient (modes 1, 2)
  const float4* tab;          // mode 1: forward table
  int B, P, C, G, CW, silu;
  float eps;
  const float* gamma; const float* beta;
  float4* out_tab;            // mode 0: table, mode 1: table2
  float* rows;                // [nb][C][2] per-row sums for the batch tail (sc1 stores)
  float* part;                // [nb][psplit][C][2] pixel-split partials (sc1 stores)
  unsigned* ctr;              // [nchunks] arrival counters
  float* sum1; float* sum2;   // batch tail outputs: mode 1 dbeta/dgamma, mode 2 per_c/per_c2
  bf16_t* per_bc; int ld_bc;  // mode 2
  int c_store;
  long long seg;              // mode 2: rows per (virtual) batch row; 0 = P
  int nb;                     // batch rows (virtual for mode 2)
  int rows_only;              // GroupNorm backward: publish the per-(b, c) sums to rows, no batch tail
};

// ---- Shared device helpers: each piece of GroupNorm arithmetic and each cross-workgroup hand-off is stated here once
__device__ __forceinline__ void st_coherent(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_coherent(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// true in every thread of the workgroup that arrives last among n at *ctr (which it re-arms)
__device__ __forceinline__ bool arrive_last(unsigned* ctr, int n) {
  __shared__ int flag;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this thread's coherent row stores are done
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned prev = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = prev == (unsigned)(n - 1);
    if (last) __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    flag = last;
  }
  __syncthreads();
  if (flag) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // acquire before reading the other arrivals' rows
  return flag != 0;
}

// Publish sums for another workgroup to read: dst[ch] = {v1, v2}; publish_sums: a strip's s1, s2 by NTH threads.
__device__ __forceinline__ void publish_pair(float* dst, int ch, float v1, float v2) {
  st_coherent(dst + 2 * ch, v1);
  st_coherent(dst + 2 * ch + 1, v2);
}
template <int NTH>
__device__ __forceinline__ void publish_sums(float* dst, const float* s1, const float* s2, int cw) {
  for (int ch = threadIdx.x; ch < cw; ch += NTH) publish_pair(dst, ch, s1[ch], s2[ch]);
}

// x1 += sum_i p[i*ld], x2 += sum_i p[i*ld + 1] over i = first, first + step, ... < n, in that order (deterministic).
// The coherent loads of N terms are issued together (from clamped, valid indices) before they are added: one
// cross-XCD round trip per N terms instead of a dependent chain of one per term.
template <int N>
__device__ __forceinline__ void ordered_sum(const float* p, int ld, int first, int step, int n, float& x1,
                                            float& x2) {
  for (int i0 = first; i0 < n; i0 += N * step) {
    float r1[N], r2[N];
#pragma unroll
    for (int u = 0; u < N; ++u) {
      const float* rp = p + (long long)min(i0 + u * step, n - 1) * ld;
      r1[u] = ld_coherent(rp);
      r2[u] = ld_coherent(rp + 1);
    }
#pragma unroll
    for (int u = 0; u < N; ++u) {
      if (i0 + u * step < n) {
        x1 += r1[u];
        x2 += r2[u];
      }
    }
  }
}

// pixels [p0, p1) of n for this workgroup's pixel split (blockIdx.z of gridDim.z)
template <typename T>
__device__ __forceinline__ void pixel_range(T n, T& p0, T& p1) {
  const T per = (n + gridDim.z - 1) / gridDim.z;
  p0 = blockIdx.z * per;
  p1 = min(n, p0 + per);
  if (p1 < p0) p1 = p0;
}

// {mean, rstd} of group gi from the strip's per-channel sums s1 = sum x, s2 = sum x^2 (fp64 merge)
__device__ __forceinline__ float2 group_mean_rstd(const float* s1, const float* s2, int gi, int Cg, int P, float eps) {
  double m1 = 0, m2 = 0;
  for (int c = gi * Cg; c < (gi + 1) * Cg; ++c) {
    m1 += s1[c];
    m2 += s2[c];
  }
  const double n = (double)P * Cg, mu = m1 / n;
  double var = m2 / n - mu * mu;
  if (var < 0) var = 0;
  return make_float2((float)mu, (float)(1.0 / sqrt(var + (double)eps)));
}

// forward table entry {a = rstd*gamma, s = beta - mean*a, mean, rstd} of one channel
__device__ __forceinline__ float4 fwd_entry(float2 mr, float gamma, float beta) {
  const float a = mr.y * gamma;
  return make_float4(a, beta - mr.x * a, mr.x, mr.y);
}

// y = act(x*a + s)
__device__ __forceinline__ float fwd_elem(float x, float a, float s, int silu) {
  const float z = fmaf(x, a, s);
  return silu ? silu_f(z) : z;
}

// dz = dy [* silu'(x*a + s)]
__device__ __forceinline__ float dz_elem(float dy, float x, float a, float s, int silu) {
  return silu ? dy * silu_grad_f(fmaf(x, a, s)) : dy;
}

// Backward coefficients {q, o} of group gi from the strip's sums s1 = sum dz, s2 = sum dz*xhat (gamma at the strip's
// first channel, t a forward table entry of the group):
// dx = rstd*(dz*gamma - A/n - xhat*Bc/n) = a*dz + q*x + o with q = -rstd^2 Bc/n, o = rstd^2 mean Bc/n - rstd A/n
__device__ __forceinline__ float2 bwd_group_coeffs(const float* gamma, const float* s1, const float* s2, int gi, int Cg,
                                                   float4 t, float inv_n) {
  float A = 0.f, Bc = 0.f;
  for (int ch = gi * Cg; ch < (gi + 1) * Cg; ++ch) {
    A += gamma[ch] * s1[ch];
    Bc += gamma[ch] * s2[ch];
  }
  const float rs = t.w, mu = t.z;
  return make_float2(-rs * rs * Bc * inv_n, rs * rs * mu * Bc * inv_n - rs * A * inv_n);
}

// dx = addend + a*dz + q*x + o
__device__ __forceinline__ float dx_elem(float add, float dz, float x, float a, float q, float o) {
  return add + fmaf(a, dz, fmaf(q, x, o));
}

// 8 channels of the addend at add + off, zeros without one
__device__ __forceinline__ void load_addend(const bf16_t* add, long long off, float* av) {
  if (add) {
    unpack8(*(const uint4*)(add + off), av);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) av[e] = 0.f;
  }
}

// The streaming backward of one thread: dx = addend + a*dz + q*x + o on 8 channels from cc of the pixel rows first,
// first + step, ... < p1 of the batch row at row rb -- one read of x, dy and the addend, one write of dx, UNROLL rows
// in flight. coef(e) = {a, s, q, o} of channel cc + e: the coefficients are built here and not handed in as an array,
// because a caller's register array that a helper sees by reference is split into scalars late in the compile, and
// the loop then held 8 (apply) / 24 (part) more VGPRs, one / two waves per SIMD fewer.
template <int UNROLL, class Coef>
__device__ __forceinline__ void bwd_stream(const bf16_t* x, int ldx, const bf16_t* dy, int lddy, const bf16_t* add,
                                           int ldadd, bf16_t* dx, int lddx, int silu, long long rb, int cc, int first,
                                           int p1, int step, Coef coef) {
  float4 tb[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) tb[e] = coef(e);
#pragma unroll UNROLL
  for (int p = first; p < p1; p += step) {
    const long long row = rb + p;
    float xv[8], gv[8], av[8], ov[8];
    unpack8(*(const uint4*)(x + row * ldx + cc), xv);
    unpack8(*(const uint4*)(dy + row * lddy + cc), gv);
    load_addend(add, row * ldadd + cc, av);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      ov[e] = dx_elem(av[e], dz_elem(gv[e], xv[e], tb[e].x, tb[e].y, silu), xv[e], tb[e].x, tb[e].z, tb[e].w);
    *(uint4*)(dx + row * lddx + cc) = pack8(ov);
  }
}

// ---- Reduction kernels: 256 threads reduce all pixels (or one pixel split) of a (batch row, channel strip)
// Per-channel sums over rows [row0, row0 + nrows) of the strip [c0, c0 + cw) -> s1[cw], s2[cw] in LDS.
// mode 0: (x, x^2); mode 1: (dz, dz*xhat) with dz = dy [* silu'(x*a + s)]; mode 2: (dy, 0).
template <int MODE>
__device__ __forceinline__ void strip_reduce(const StripArgs& a, int b, long long row0, long long nrows, int c0, int cw,
                                             float* s1, float* s2) {
  __shared__ float red[NT][17];
  const int L = cw >> 3;            // lanes per pixel row
  const int R = NT / L;             // pixel rows per iteration
  const int t = threadIdx.x;
  const int lane = t % L, r = t / L;
  const int cc = c0 + lane * 8;
  float u[8], v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { u[e] = 0.f; v[e] = 0.f; }
  float4 tb[8];
  if (MODE == 1) {
#pragma unroll
    for (int e = 0; e < 8; ++e) tb[e] = r < R ? a.tab[(long long)b * a.C + cc + e] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (r < R && nrows > 0) {
    // rows in batches of RB: the batch's loads are issued together from clamped (valid) rows and masked after, so
    // each thread keeps RB (x2 in mode 1) 16-byte loads in flight instead of one row per round trip
    constexpr int RB = MODE == 1 ? 4 : 8;
    for (long long p0 = r; p0 < nrows; p0 += (long long)RB * R) {
      uint4 rx[RB], rg[RB];
#pragma unroll
      for (int q = 0; q < RB; ++q) {
        const long long row = row0 + min(p0 + (long long)q * R, nrows - 1);
        if (MODE != 2) rx[q] = *(const uint4*)(a.x + row * a.ldx + cc);
        if (MODE != 0) rg[q] = *(const uint4*)(a.dy + row * a.ldy + cc);
      }
#pragma unroll
      for (int q = 0; q < RB; ++q) {
        if (p0 + (long long)q * R >= nrows) break;
        float xv[8], gv[8];
        if (MODE == 0) {
          unpack8(rx[q], xv);
#pragma unroll
          for (int e = 0; e < 8; ++e) { u[e] += xv[e]; v[e] = fmaf(xv[e], xv[e], v[e]); }
        } else if (MODE == 1) {
          unpack8(rx[q], xv);
          unpack8(rg[q], gv);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float dz = dz_elem(gv[e], xv[e], tb[e].x, tb[e].y, a.silu);
            u[e] += dz;
            v[e] = fmaf(dz, (xv[e] - tb[e].z) * tb[e].w, v[e]);
          }
        } else {
          unpack8(rg[q], gv);
#pragma unroll
          for (int e = 0; e < 8; ++e) u[e] += gv[e];
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) { red[t][e] = u[e]; red[t][8 + e] = v[e]; }
  __syncthreads();
  for (int ch = t; ch < cw; ch += NT) {
    const int l = ch >> 3, e = ch & 7;
    float x1 = 0.f, x2 = 0.f;
    for (int rr = 0; rr < R; ++rr) {
      x1 += red[rr * L + l][e];
      x2 += red[rr * L + l][8 + e];
    }
    s1[ch] = x1;
    s2[ch] = x2;
  }
  __syncthreads();
}

// Last strip of a batch column: out1[c] = sum_b rows[b][c][0], out2[c] = sum_b rows[b][c][1] for the strip.
__device__ __forceinline__ void batch_tail(const StripArgs& a, int c0, int cw, float* o1, float* o2, int c_store,
                                           bool dup = false) {
  __shared__ float acc[NT][2];
  const int t = threadIdx.x;
  const int nthr = min((int)blockDim.x, NT);  // the single-pass kernels run 64 .. 1024 threads
  const int ld = a.C * 2;
  const auto put = [&](int c, float x1, float x2) {
    if (c < c_store) {
      if (o1) o1[c] = x1;
      if (o2) o2[c] = dup ? x1 : x2;
    }
  };
  if (cw > nthr) {  // narrow workgroup, wide strip: one thread per channel, all batch rows in order
    for (int ch = t; ch < cw; ch += blockDim.x) {
      float x1 = 0.f, x2 = 0.f;
      ordered_sum<16>(a.rows + (long long)(c0 + ch) * 2, ld, 0, 1, a.nb, x1, x2);
      put(c0 + ch, x1, x2);
    }
    return;
  }
  // nbg threads per channel: thread bg sums batch rows bg, bg + nbg, ..., then the nbg partials are added in order
  const int nbg = max(1, nthr / cw);
  const int ch = t % cw, bg = t / cw;
  float x1 = 0.f, x2 = 0.f;
  if (t < nthr && bg < nbg && t < nbg * cw)
    ordered_sum<16>(a.rows + (long long)(c0 + ch) * 2, ld, bg, nbg, a.nb, x1, x2);
  if (t < nthr) {
    acc[t][0] = x1;
    acc[t][1] = x2;
  }
  __syncthreads();
  if (t < cw) {
    float y1 = 0.f, y2 = 0.f;
    for (int g = 0; g < nbg; ++g) {
      y1 += acc[g * cw + t][0];
      y2 += acc[g * cw + t][1];
    }
    put(c0 + t, y1, y2);
  }
}

// Pixel-split combine: with gridDim.z > 1 every workgroup publishes its strip sums and the last of the
// (strip, b) group continues with the complete sums (added in split order) in s1/s2; the others return false.
__device__ __forceinline__ bool combine_psplits(const StripArgs& a, int b, int c0, int cw, float* s1, float* s2) {
  const int nz = gridDim.z;
  if (nz == 1) return true;
  publish_sums<NT>(a.part + (((long long)b * nz + blockIdx.z) * a.C + c0) * 2, s1, s2, cw);
  if (!arrive_last(a.ctr + blockIdx.x * gridDim.y + b, nz)) return false;
  for (int ch = threadIdx.x; ch < cw; ch += NT) {
    float x1 = 0.f, x2 = 0.f;
    ordered_sum<8>(a.part + ((long long)b * nz * a.C + c0 + ch) * 2, a.C * 2, 0, 1, nz, x1, x2);
    s1[ch] = x1;
    s2[ch] = x2;
  }
  __syncthreads();
  return true;
}

// grid (nchunks, B, pixel splits): GroupNorm statistics of whole groups -> forward table
__global__ __launch_bounds__(NT) void gn_stats_kernel(StripArgs a) {
  __shared__ float s1[NT], s2[NT];
  __shared__ float2 grp[NT];
  const int b = blockIdx.y;
  const int c0 = blockIdx.x * a.CW;
  const int cw = min(a.CW, a.C - c0);
  const int Cg = a.C / a.G;
  long long p0, p1;
  pixel_range((long long)a.P, p0, p1);
  strip_reduce<0>(a, b, (long long)b * a.P + p0, p1 - p0, c0, cw, s1, s2);
  if (!combine_psplits(a, b, c0, cw, s1, s2)) return;
  const int ng = cw / Cg;
  if ((int)threadIdx.x < ng) grp[threadIdx.x] = group_mean_rstd(s1, s2, threadIdx.x, Cg, a.P, a.eps);
  __syncthreads();
  for (int ch = threadIdx.x; ch < cw; ch += NT) {
    const int c = c0 + ch;
    a.out_tab[(long long)b * a.C + c] = fwd_entry(grp[ch / Cg], a.gamma[c], a.beta[c]);
  }
}

// grid (nchunks, B, pixel splits): GroupNorm backward coefficients -> table2 {a, s, q, o} for gn_bwd_apply_kernel;
// dgamma/dbeta by the batch tail
__global__ __launch_bounds__(NT) void gn_bwd_reduce_kernel(StripArgs a) {
  __shared__ float s1[NT], s2[NT];
  __shared__ float2 grp[NT];
  const int b = blockIdx.y;
  const int c0 = blockIdx.x * a.CW;
  const int cw = min(a.CW, a.C - c0);
  const int Cg = a.C / a.G;
  long long p0, p1;
  pixel_range((long long)a.P, p0, p1);
  strip_reduce<1>(a, b, (long long)b * a.P + p0, p1 - p0, c0, cw, s1, s2);
  if (!combine_psplits(a, b, c0, cw, s1, s2)) return;
  const int ng = cw / Cg;
  const float inv_n = 1.0f / ((float)a.P * Cg);
  if ((int)threadIdx.x < ng)
    grp[threadIdx.x] = bwd_group_coeffs(a.gamma + c0, s1, s2, threadIdx.x, Cg,
                                        a.tab[(long long)b * a.C + c0 + threadIdx.x * Cg], inv_n);
  __syncthreads();
  for (int ch = threadIdx.x; ch < cw; ch += NT) {
    const int c = c0 + ch;
    const float4 t = a.tab[(long long)b * a.C + c];
    const float2 qo = grp[ch / Cg];
    a.out_tab[(long long)b * a.C + c] = make_float4(t.x, t.y, qo.x, qo.y);
  }
  if (a.sum1 || a.rows_only) publish_sums<NT>(a.rows + ((long long)b * a.C + c0) * 2, s1, s2, cw);
  if (!a.sum1) return;
  if (!arrive_last(a.ctr + BATCH_CTR + blockIdx.x, a.nb)) return;
  batch_tail(a, c0, cw, a.sum1, a.sum2, a.C);
}

// grid (nchunks, nb, pixel splits): per-(row, c) sums of dy -> per_bc (bf16), per-c sums by the batch tail
__global__ __launch_bounds__(NT) void chan_sum_kernel(StripArgs a) {
  __shared__ float s1[NT], s2[NT];
  const int b = blockIdx.y;
  const int c0 = blockIdx.x * a.CW;
  const int cw = min(a.CW, a.C - c0);
  const long long total = (long long)a.B * a.P;
  const long long row0 = (long long)b * a.seg;
  const long long nrows = max(0LL, min(a.seg, total - row0));
  long long p0, p1;
  pixel_range(nrows, p0, p1);
  strip_reduce<2>(a, b, row0 + p0, p1 - p0, c0, cw, s1, s2);
  if (!combine_psplits(a, b, c0, cw, s1, s2)) return;
  const bool tail = a.sum1 || a.sum2;
  for (int ch = threadIdx.x; ch < cw; ch += NT) {
    if (a.per_bc) a.per_bc[(long long)b * a.ld_bc + c0 + ch] = f2bf(s1[ch]);
    if (tail) publish_pair(a.rows + ((long long)b * a.C + c0) * 2, ch, s1[ch], 0.f);
  }
  if (!tail) return;
  if (!arrive_last(a.ctr + BATCH_CTR + blockIdx.x, a.nb)) return;
  batch_tail(a, c0, cw, a.sum1, a.sum2, a.c_store, /*dup=*/true);  // per_c2: a second bias with the same gradient
}

struct RowsGroup {
  sdmi_gn_rows_job j[SDMI_GN_ROWS_GROUP_MAX];
};

// grid (C/256, jobs): dgamma[c] = sum_b rows[b][c][1], dbeta[c] = sum_b rows[b][c][0] of job blockIdx.y, batch rows in
// order (deterministic)
__global__ __launch_bounds__(NT) void gn_rows_sum_grouped_kernel(const RowsGroup g) {
  const sdmi_gn_rows_job& J = g.j[blockIdx.y];
  const int c = blockIdx.x * NT + threadIdx.x;
  if (c >= J.C) return;
  const float2* rows = (const float2*)J.rows;
  float s1 = 0.f, s2 = 0.f;
#pragma unroll 8
  for (int b = 0; b < J.B; ++b) {
    const float2 v = rows[(long long)b * J.C + c];
    s1 += v.x;
    s2 += v.y;
  }
  J.dbeta[c] = s1;
  J.dgamma[c] = s2;
}

// ---- Single-pass GroupNorm: one workgroup of NTH threads owns a (batch row, channel strip of whole groups), keeps its
// P x strip slab in registers as packed bf16 (IT pixel rows per thread), reduces, and applies -- one launch and one
// read of x (and dy) instead of a statistics pass, a cross-workgroup combine and a second elementwise pass. The
// (NTH, IT) pairs that exist are the rows of PASS_SHAPES.
// per-channel sums of u (and v) over the workgroup's rows -> s1/s2[cw] in LDS (red: [NTH][17] scratch), in two
// fixed-order stages so no thread sums more than ~8 + NTH / cw partials: (1) thread j sums a contiguous segment of
// ~8 rows of channel j % cw (segment j / cw), (2) one thread per channel sums the segments
template <int NTH>
__device__ __forceinline__ void small_reduce(const float* u, const float* v, int cw, float (*red)[17], float* s1,
                                             float* s2) {
  __shared__ float seg[NTH][2];
  const int t = threadIdx.x, L = cw >> 3, R = NTH / L;
#pragma unroll
  for (int e = 0; e < 8; ++e) { red[t][e] = u[e]; red[t][8 + e] = v[e]; }
  __syncthreads();
  const int S = max(1, min(R, NTH / cw));  // segments per channel
  const int RS = (R + S - 1) / S;          // rows per segment
  for (int j = t; j < S * cw; j += NTH) {  // S * cw <= NTH unless the strip is wider than the workgroup (S = 1)
    const int ch = j % cw, sg = j / cw, l = ch >> 3, e = ch & 7;
    const int r1 = min(R, (sg + 1) * RS);
    float x1 = 0.f, x2 = 0.f;
    for (int rr = sg * RS; rr < r1; ++rr) {
      x1 += red[rr * L + l][e];
      x2 += red[rr * L + l][8 + e];
    }
    if (S > 1) {
      seg[j][0] = x1;
      seg[j][1] = x2;
    } else {
      s1[ch] = x1;
      s2[ch] = x2;
    }
  }
  __syncthreads();
  if (S == 1) return;
  for (int ch = t; ch < cw; ch += NTH) {
    float x1 = 0.f, x2 = 0.f;
    for (int sg = 0; sg < S; ++sg) {
      x1 += seg[sg * cw + ch][0];
      x2 += seg[sg * cw + ch][1];
    }
    s1[ch] = x1;
    s2[ch] = x2;
  }
  __syncthreads();
}

// (strip, batch row) of a single-pass workgroup on an (nchunks, B) grid, XCD-aware: workgroups are dispatched
// round-robin over the 8 XCDs (dispatch id d on XCD d % 8, one 4 MiB L2 each); the logical ids are re-numbered so
// every XCD owns a contiguous band, strips fastest -- the narrow strips that share the 128-B lines of one batch row's
// pixel rows then read them through ONE L2 instead of up to eight (bijective for any grid size)
__device__ __forceinline__ void strip_block(int& strip, int& b) {
  const int total = gridDim.x * gridDim.y;
  const int d = blockIdx.y * gridDim.x + blockIdx.x;
  const int xcd = d & 7, q = total >> 3, r = total & 7;
  const int l = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (d >> 3);
  b = l / gridDim.x;
  strip = l - b * gridDim.x;
}

// grid (nchunks, B): y = act(GroupNorm(x)), and the forward table for the backward pass. NTH threads, IT pixel rows
// per thread (P <= IT * (NTH / (strip / 8)))
template <int NTH, int IT>
__global__ __launch_bounds__(NTH) void gn_fwd_pass_kernel(StripArgs a, bf16_t* y, int ldy) {
  __shared__ float red[NTH][17];
  __shared__ float s1[NT], s2[NT];
  __shared__ float2 grp[NT];
  int strip, b;
  strip_block(strip, b);
  const int c0 = strip * a.CW, cw = min(a.CW, a.C - c0);
  const int L = cw >> 3, R = NTH / L, t = threadIdx.x, lane = t % L, r = t / L;
  const int cc = c0 + lane * 8, Cg = a.C / a.G;
  const bool act = r < R;
  float u[8], v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { u[e] = 0.f; v[e] = 0.f; }
  const bf16_t* X = a.x + (long long)b * a.P * a.ldx + cc;
  // every row load issued first from a clamped (valid) row, masked afterwards: a guarded load per row would make
  // the compiler wait for each one before the next
  uint4 rx[IT];
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int p = min(min(r, R - 1) + it * R, a.P - 1);
    rx[it] = *(const uint4*)(X + (long long)p * a.ldx);
  }
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    float xv[8];
    unpack8(rx[it], xv);
    if (act && r + it * R < a.P) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { u[e] += xv[e]; v[e] = fmaf(xv[e], xv[e], v[e]); }
    }
  }
  small_reduce<NTH>(u, v, cw, red, s1, s2);
  const int ng = cw / Cg;
  for (int gi = t; gi < ng; gi += NTH) grp[gi] = group_mean_rstd(s1, s2, gi, Cg, a.P, a.eps);
  __syncthreads();
  for (int ch = t; ch < cw; ch += NTH) {
    const int c = c0 + ch;
    a.out_tab[(long long)b * a.C + c] = fwd_entry(grp[ch / Cg], a.gamma[c], a.beta[c]);
  }
  if (!act) return;
  float ta[8], ts[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float4 te = fwd_entry(grp[(lane * 8 + e) / Cg], a.gamma[cc + e], a.beta[cc + e]);
    ta[e] = te.x;
    ts[e] = te.y;
  }
  bf16_t* Y = y + (long long)b * a.P * ldy + cc;
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int p = r + it * R;
    if (p < a.P) {
      float xv[8], o[8];
      unpack8(rx[it], xv);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = fwd_elem(xv[e], ta[e], ts[e], a.silu);
      *(uint4*)(Y + (long long)p * ldy) = pack8(o);
    }
  }
}

// grid (nchunks, B): GroupNorm (+SiLU) backward in one pass; dgamma/dbeta by the batch tail. x and dy stay packed in
// registers; the 8-row form re-reads dy in the apply pass (an L2 hit: the workgroup read it moments before) to stay
// within the 128 VGPRs a 16-wave workgroup allows, and dz = dy * SiLU'(...) is recomputed there.
template <int NTH, int IT>
__global__ __launch_bounds__(NTH) void gn_bwd_pass_kernel(StripArgs a, bf16_t* dx, int lddx, const bf16_t* add,
                                                          int ldadd) {
  __shared__ float red[NTH][17];
  __shared__ float s1[NT], s2[NT];
  __shared__ float2 grp[NT];
  __shared__ float4 stb[NT];  // forward table of the strip
  int strip, b;
  strip_block(strip, b);
  const int c0 = strip * a.CW, cw = min(a.CW, a.C - c0);
  const int L = cw >> 3, R = NTH / L, t = threadIdx.x, lane = t % L, r = t / L;
  const int cc = c0 + lane * 8, Cg = a.C / a.G;
  const bool act = r < R;
  const long long rb = (long long)b * a.P;
  constexpr bool KEEP_DY = IT <= 4 || NTH <= 256;  // else dy is re-read in the apply pass (VGPR budget)
  // IT <= 4: dz = dy * SiLU'(x a + s) of the reduction pass is kept (fp32) for the apply pass instead of being
  // recomputed there (the SiLU derivative is an exp + a reciprocal per element: ~1/3 of the kernel's VALU work)
  constexpr bool KEEP_DZ = KEEP_DY && IT <= 4;
  float dzk[KEEP_DZ ? IT * 8 : 1];
  uint4 rx[IT], rg[IT];  // all row loads in flight first
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int p = min(min(r, R - 1) + it * R, a.P - 1);
    rx[it] = *(const uint4*)(a.x + (rb + p) * a.ldx + cc);
    rg[it] = *(const uint4*)(a.dy + (rb + p) * a.ldy + cc);
  }
  for (int ch = t; ch < cw; ch += NTH) stb[ch] = a.tab[(long long)b * a.C + c0 + ch];
  __syncthreads();
  float u[8], v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { u[e] = 0.f; v[e] = 0.f; }
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    float xv[8], gv[8];
    unpack8(rx[it], xv);
    unpack8(rg[it], gv);
    if (act && r + it * R < a.P) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float4 tb = stb[lane * 8 + e];
        const float dz = dz_elem(gv[e], xv[e], tb.x, tb.y, a.silu);
        if constexpr (KEEP_DZ) dzk[it * 8 + e] = dz;
        u[e] += dz;
        v[e] = fmaf(dz, (xv[e] - tb.z) * tb.w, v[e]);
      }
    }
  }
  small_reduce<NTH>(u, v, cw, red, s1, s2);
  const int ng = cw / Cg;
  const float inv_n = 1.0f / ((float)a.P * Cg);
  for (int gi = t; gi < ng; gi += NTH) grp[gi] = bwd_group_coeffs(a.gamma + c0, s1, s2, gi, Cg, stb[gi * Cg], inv_n);
  if (a.sum1 || a.rows_only) publish_sums<NTH>(a.rows + ((long long)b * a.C + c0) * 2, s1, s2, cw);
  __syncthreads();
  if (act) {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int p = r + it * R;
      if (p < a.P) {
        float xv[8], gv[8], av[8], ov[8];
        unpack8(rx[it], xv);
        if constexpr (KEEP_DZ) {
#pragma unroll
          for (int e = 0; e < 8; ++e) gv[e] = dzk[it * 8 + e];
        } else if (KEEP_DY) {
          unpack8(rg[it], gv);
        } else {
          unpack8(*(const uint4*)(a.dy + (rb + p) * a.ldy + cc), gv);
        }
        load_addend(add, (rb + p) * ldadd + cc, av);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float4 tb = stb[lane * 8 + e];
          const float2 qo = grp[(lane * 8 + e) / Cg];
          const float dz = KEEP_DZ ? gv[e] : dz_elem(gv[e], xv[e], tb.x, tb.y, a.silu);
          ov[e] = dx_elem(av[e], dz, xv[e], tb.x, qo.x, qo.y);
        }
        *(uint4*)(dx + (rb + p) * lddx + cc) = pack8(ov);
      }
    }
  }
  if (!a.sum1) return;
  if (!arrive_last(a.ctr + BATCH_CTR + strip, a.nb)) return;
  batch_tail(a, c0, cw, a.sum1, a.sum2, a.C);
}

// ---- Streaming kernels: elementwise over pixels with per-(b, c) coefficients held in registers
struct ApplyArgs {
  const bf16_t* x; int ldx;
  bf16_t* y; int ldy;
  const bf16_t* dy; int lddy;
  bf16_t* dx; int lddx;
  const float4* tab;  // apply: {a, s, -, -}; backward: {a, s, q, o}
  const bf16_t* add; int ldadd;
  int B, P, C, silu;
};

// Elementwise passes: grid (C/64 strips, B, pixel splits); a thread owns 8 channels of one strip for
// all of its pixels, so its table entries are loaded once and stay in registers.
constexpr int APPLY_CW = 64;

// first channel cc, pixel row r (of 32 per iteration) and pixel range of a thread; false past the last channel
__device__ __forceinline__ bool apply_coords(const ApplyArgs& a, int& cc, int& r, int& p0, int& p1) {
  const int lane = threadIdx.x & 7;
  r = threadIdx.x >> 3;
  cc = blockIdx.x * APPLY_CW + lane * 8;
  pixel_range(a.P, p0, p1);
  return cc < a.C;
}

// y = act(x*a + s)
__global__ __launch_bounds__(NT) void gn_apply_kernel(ApplyArgs a) {
  int cc, r, p0, p1;
  if (!apply_coords(a, cc, r, p0, p1)) return;
  const int b = blockIdx.y;
  float ta[8], ts[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float4 t = a.tab[(long long)b * a.C + cc + e];
    ta[e] = t.x;
    ts[e] = t.y;
  }
  const bf16_t* X = a.x + (long long)b * a.P * a.ldx + cc;
  bf16_t* Y = a.y + (long long)b * a.P * a.ldy + cc;
#pragma unroll 4
  for (int p = p0 + r; p < p1; p += NT / 8) {
    float xv[8], yv[8];
    unpack8(*(const uint4*)(X + (long long)p * a.ldx), xv);
#pragma unroll
    for (int e = 0; e < 8; ++e) yv[e] = fwd_elem(xv[e], ta[e], ts[e], a.silu);
    *(uint4*)(Y + (long long)p * a.ldy) = pack8(yv);
  }
}

// dx = a*dz + q*x + o (+ addend), dz = dy [* silu'(x*a + s)], coefficients from gn_bwd_reduce_kernel's table2
__global__ __launch_bounds__(NT) void gn_bwd_apply_kernel(ApplyArgs a) {
  int cc, r, p0, p1;
  if (!apply_coords(a, cc, r, p0, p1)) return;
  const int b = blockIdx.y;
  bwd_stream<2>(a.x, a.ldx, a.dy, a.lddy, a.add, a.ldadd, a.dx, a.lddx, a.silu, (long long)b * a.P, cc, p0 + r, p1,
                NT / 8, [&](int e) { return a.tab[(long long)b * a.C + cc + e]; });
}

// s1[ch], s2[ch] (ch < cw <= NT) = the sums over the nseg segment partials {sum, sum2} of (batch row b, channel
// c0 + ch) for gn_bwd_part_kernel. Each thread loads two channels (16 B) of every SLN-th segment -- SLN = NT / (cw / 2)
// segment lanes (<= 4), all loads of a lane independent -- and the lanes are merged in lane order: a fixed summation
// order (deterministic) with nseg / SLN loads per thread instead of nseg.
__device__ __forceinline__ void part_sums(const float2* part, int b, int nseg, int C, int c0, int cw, float* s1,
                                          float* s2, float* p1, float* p2) {
  const int t = threadIdx.x, hc = cw >> 1, sln = min(NT / hc, 4), c2 = t % hc, sl = t / hc;
  if (sl < sln) {
    const float4* pp = (const float4*)(part + (long long)b * nseg * C + c0) + c2;
    const long long ld4 = C >> 1;
    float x1 = 0.f, x2 = 0.f, y1 = 0.f, y2 = 0.f;
#pragma unroll 8
    for (int j = sl; j < nseg; j += sln) {
      const float4 v = pp[(long long)j * ld4];
      x1 += v.x;
      x2 += v.y;
      y1 += v.z;
      y2 += v.w;
    }
    p1[sl * cw + 2 * c2] = x1;
    p2[sl * cw + 2 * c2] = x2;
    p1[sl * cw + 2 * c2 + 1] = y1;
    p2[sl * cw + 2 * c2 + 1] = y2;
  }
  __syncthreads();
  for (int c = t; c < cw; c += NT) {
    float a1 = 0.f, a2 = 0.f;
    for (int l = 0; l < sln; ++l) {
      a1 += p1[l * cw + c];
      a2 += p2[l * cw + c];
    }
    s1[c] = a1;
    s2[c] = a2;
  }
  __syncthreads();
}

// GroupNorm (+SiLU) backward from the producing GEMM's statistics (sdmi_gemm_desc::gn_part): grid (strips of whole
// groups, B, pixel splits). Every workgroup sums the P / rb segment partials of its (batch row, strip) in segment order
// (fp32, fixed order: deterministic), forms the group coefficients exactly as gn_bwd_pass_kernel does, and streams
// dx = a*dz + q*x + o (+ addend) over its pixel range -- one read of x, dy and the addend, one write of dx, no
// reduction phase. dgamma / dbeta: the pixel-split-0 workgroups publish their (b, c) sums and the last of the B
// arrivals per strip sums them (batch_tail).
__global__ __launch_bounds__(NT) void gn_bwd_part_kernel(StripArgs a, const float2* part, int rb, bf16_t* dx, int lddx,
                                                         const bf16_t* add, int ldadd) {
  __shared__ float s1[NT], s2[NT], q1[2 * NT], q2[2 * NT];
  __shared__ float2 grp[NT];
  __shared__ float4 stb[NT];
  const int strip = blockIdx.x, b = blockIdx.y;
  const int c0 = strip * a.CW, cw = min(a.CW, a.C - c0);
  const int t = threadIdx.x, Cg = a.C / a.G;
  for (int ch = t; ch < cw; ch += NT) stb[ch] = a.tab[(long long)b * a.C + c0 + ch];
  part_sums(part, b, a.P / rb, a.C, c0, cw, s1, s2, q1, q2);
  const int ng = cw / Cg;
  const float inv_n = 1.0f / ((float)a.P * Cg);
  for (int gi = t; gi < ng; gi += NT) grp[gi] = bwd_group_coeffs(a.gamma + c0, s1, s2, gi, Cg, stb[gi * Cg], inv_n);
  const bool publish = (a.sum1 || a.rows_only) && blockIdx.z == 0;
  if (publish) publish_sums<NT>(a.rows + ((long long)b * a.C + c0) * 2, s1, s2, cw);
  __syncthreads();
  const int L = cw >> 3, R = NT / L, lane = t % L, r = t / L;
  if (r < R) {
    int p0, p1;
    pixel_range(a.P, p0, p1);
    bwd_stream<4>(a.x, a.ldx, a.dy, a.ldy, add, ldadd, dx, lddx, a.silu, (long long)b * a.P, c0 + lane * 8, p0 + r, p1,
                  R, [&](int e) {
                    const float4 fe = stb[lane * 8 + e];
                    const float2 qo = grp[(lane * 8 + e) / Cg];
                    return make_float4(fe.x, fe.y, qo.x, qo.y);
                  });
  }
  if (!publish || !a.sum1) return;
  if (!arrive_last(a.ctr + BATCH_CTR + strip, a.nb)) return;
  batch_tail(a, c0, cw, a.sum1, a.sum2, a.C);
}

// ---- Launch-shape selection and launches (host)
// Strip width: a multiple of `unit` (whole groups) and of 8 channels, at least 64 channels when C allows
// (narrower strips measured slower: 16-byte row segments coalesce poorly).
int strip_width(int C, int unit) {
  int cw = unit;
  while (cw % 8 || (cw < 64 && cw * 2 <= C)) cw += unit;
  while ((C + cw - 1) / cw > SLOT_CTRS) cw += unit;
  return cw;
}

// Strip width of the streaming gn_bwd_part_kernel: whole groups AND a multiple of 64 channels (128-B row segments, so no
// cache line is shared by two strips' workgroups), else the whole row -- e.g. C = 384 in 32 groups: 192, not 72
int part_strip_width(int C, int unit) {
  int cw = unit;
  while (cw % 64 && cw < C) cw += unit;
  if (cw > C || cw > NT) cw = strip_width(C, unit);
  return cw;
}

// pixel splits per (strip, batch row): aim for >= 512 workgroups with >= 128 pixels each
int pick_psplit(int nch, int nb, long long rows_per_b) {
  int ps = 1;
  if ((long long)nch * nb > BATCH_CTR) return 1;
  while ((long long)nch * nb * ps < 512 && rows_per_b / (ps * 2) >= 128 && ps < PS_MAX) ps *= 2;
  return ps;
}

// grid of an elementwise pass: C/64 strips x B x pixel splits, >= ~2048 workgroups, >= 64 pixels each
dim3 apply_grid(int B, int P, int C) {
  const int strips = (C + APPLY_CW - 1) / APPLY_CW;
  int ps = 1;
  while ((long long)strips * B * ps < 2048 && P / (ps * 2) >= 64) ps *= 2;
  return dim3(strips, B, ps);
}

// The single-pass kernels that exist: threads per workgroup x pixel rows per thread, fewest threads first. These are
// all the pairs pick_pass can ask for with <= 32 lanes per pixel row (a wider workgroup with fewer rows is never
// needed once a narrower one manages <= 4). 8 rows only at 1024 threads: its x and dy slabs (64 VGPRs) stay within
// the 128 VGPRs a 16-wave workgroup allows (32x32 levels with 64-channel strips).
struct PassShape {
  int nth, it;
};
constexpr PassShape PASS_SHAPES[] = {{64, 1},  {64, 2},  {64, 4},   {256, 1},  {256, 2}, {256, 4},
                                     {512, 2}, {512, 4}, {1024, 2}, {1024, 4}, {1024, 8}};
constexpr int N_PASS_SHAPES = sizeof(PASS_SHAPES) / sizeof(PASS_SHAPES[0]);

// The row of PASS_SHAPES for P pixel rows at L lanes per row: the fewest threads with <= 4 pixel rows each (loads in
// flight per thread), else <= 8; -1 if none holds the slab.
int pass_shape(int P, int L) {
  for (int lim : {4, 8}) {
    for (int i = 0; i < N_PASS_SHAPES; ++i) {
      const PassShape& s = PASS_SHAPES[i];
      if (s.it <= lim && P <= (long long)s.it * (s.nth / L)) return i;
    }
  }
  return -1;
}

// Single-pass launch: strip width (whole groups, 8-channel lanes) and a row of PASS_SHAPES.
struct PassCfg {
  int cw, shape;
};

// Occupancy-first choice: the widest strip that still gives >= 512 workgroups (2 per CU, measured best of 512 / 1024 /
// 2048; narrow strips share 128-B lines with their neighbours, which strip_block() keeps on one XCD), else the
// narrowest strip; per strip the shape pass_shape gives.
bool pick_pass(int B, int P, int C, int G, PassCfg& pc) {
  const int Cg = C / G;
  // 32x32 and larger images (P >= 1024): 256 workgroups of wider strips measured better in isolation (32^2 C=384
  // fwd 19.7 -> 15.2 us, bwd 35.1 -> 33.7 us; C=128 bwd 18.2 -> 16.6 us; others equal), smaller images keep 512
  const int target = P >= 1024 ? 256 : 512;
  int u = Cg;
  while (u % 8) u += Cg;
  PassCfg good = {0, -1}, any = {0, -1};
  long long any_wg = 0;
  for (int cw = u; cw <= NT && cw - u < C; cw += u) {
    const PassCfg c = {cw, pass_shape(P, cw / 8)};
    if (c.shape < 0) continue;
    const long long wg = (long long)((C + cw - 1) / cw) * B;
    if (wg >= target) good = c;  // widest so far with enough workgroups (cw ascends)
    if (wg > any_wg) {
      any = c;
      any_wg = wg;
    }
  }
  const PassCfg best = good.shape >= 0 ? good : any;
  if (best.shape < 0 || (C + best.cw - 1) / best.cw > BATCH_CTR) return false;
  pc = best;
  return true;
}

// the forward (out = y) or backward (out = dx) single-pass kernel of row pc.shape of PASS_SHAPES, grid (strips, B)
template <int I = 0>
int launch_pass(bool bwd, const PassCfg& pc, hipStream_t s, const StripArgs& a, bf16_t* out, int ldo,
                const bf16_t* add = nullptr, int ldadd = 0) {
  if constexpr (I < N_PASS_SHAPES) {
    if (pc.shape != I) return launch_pass<I + 1>(bwd, pc, s, a, out, ldo, add, ldadd);
    constexpr int NTH = PASS_SHAPES[I].nth, IT = PASS_SHAPES[I].it;
    const dim3 grid((a.C + pc.cw - 1) / pc.cw, a.B);
    if (bwd) sdmi_rt::launch(gn_bwd_pass_kernel<NTH, IT>, grid, dim3(NTH), 0, s, a, out, ldo, add, ldadd);
    else sdmi_rt::launch(gn_fwd_pass_kernel<NTH, IT>, grid, dim3(NTH), 0, s, a, out, ldo);
    SDMI_CHECK_LAUNCH();
    return 0;
  }
  return -2;  // not a row of the table: pick_pass hands out none
}

unsigned* counter_slot() {
  static std::atomic<unsigned> next{0};
  static unsigned* base[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  if (!base[dev]) {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_norm_counters)) != hipSuccess) return nullptr;
    base[dev] = (unsigned*)p;
  }
  return base[dev] + (size_t)(next.fetch_add(1) % NSLOTS) * SLOT_CTRS;
}

float* part_base(float* ws, int nb, int C) { return ws + (size_t)(nb > 32 ? nb : 32) * C * 2; }

// The checks and StripArgs fields the GroupNorm entry points share; the forward ones stop at gamma. rows_out: the
// per-(batch row, channel) sums go there and dgamma / dbeta (which must be null) are left to sdmi_gn_rows_sum.
int gn_args(StripArgs& a, const void* x, int ldx, int B, int P, int C, int G, int silu, const float* gamma,
            const void* dy = nullptr, int lddy = 0, const float* table = nullptr, float* ws = nullptr,
            float* dgamma = nullptr, float* dbeta = nullptr, float* rows_out = nullptr) {
  if (C % 8 || G <= 0 || C % G) return -1;
  if ((dgamma == nullptr) != (dbeta == nullptr) || (rows_out && dgamma)) return -3;
  a = {};
  a.x = (const bf16_t*)x; a.ldx = ldx; a.dy = (const bf16_t*)dy; a.ldy = lddy; a.tab = (const float4*)table;
  a.B = B; a.P = P; a.C = C; a.G = G; a.silu = silu; a.gamma = gamma;
  a.rows = rows_out ? rows_out : ws; a.rows_only = rows_out != nullptr; a.nb = B; a.sum1 = dbeta; a.sum2 = dgamma;
  return 0;
}

// Forward: the single-pass kernel when pick_pass finds a shape, else gn_stats_kernel then the elementwise pass.
// y == nullptr: the table only (sdmi_gn_stats)
int gn_fwd_impl(const void* x, int ldx, void* y, int ldy, int B, int P, int C, int G, float eps, const float* gamma,
                const float* beta, int silu, float* ws, float* table, sdmi_stream_t stream) {
  StripArgs a;
  const int rc = gn_args(a, x, ldx, B, P, C, G, silu, gamma);
  if (rc) return rc;
  a.eps = eps; a.beta = beta; a.out_tab = (float4*)table;
  PassCfg pc;
  if (y && pick_pass(B, P, C, G, pc)) {
    a.CW = pc.cw;
    return launch_pass(false, pc, (hipStream_t)stream, a, (bf16_t*)y, ldy);
  }
  a.CW = strip_width(C, C / G);
  const int nch = (C + a.CW - 1) / a.CW;
  if (a.CW > NT || nch > BATCH_CTR) return -2;
  const int ps = pick_psplit(nch, B, P);
  if (ps > 1) {
    a.part = part_base(ws, B, C);
    if (!(a.ctr = counter_slot())) return -4;
  }
  sdmi_rt::launch(gn_stats_kernel, dim3(nch, B, ps), dim3(NT), 0, (hipStream_t)stream, a);
  SDMI_CHECK_LAUNCH();
  return y ? sdmi_gn_apply(x, ldx, y, ldy, table, B, P, C, silu, stream) : 0;
}

// Backward: the single-pass kernel when pick_pass finds a shape, else gn_bwd_reduce_kernel (-> table2_ws, float4
// [B][C]) then gn_bwd_apply_kernel. table: the forward table; ws: sdmi_chan_reduce_workspace
int gn_bwd_impl(const void* x, int ldx, const void* dy, int lddy, void* dx, int lddx, const float* table,
                const float* gamma, int B, int P, int C, int G, int silu, float* ws, float* table2_ws, float* dgamma,
                float* dbeta, float* rows_out, const void* addend, int ldadd, sdmi_stream_t stream) {
  StripArgs r;
  const int rc = gn_args(r, x, ldx, B, P, C, G, silu, gamma, dy, lddy, table, ws, dgamma, dbeta, rows_out);
  if (rc) return rc;
  r.out_tab = (float4*)table2_ws;
  hipStream_t s = (hipStream_t)stream;
  PassCfg pc;
  if (pick_pass(B, P, C, G, pc)) {
    r.CW = pc.cw;
    if (dgamma && !(r.ctr = counter_slot())) return -4;
    return launch_pass(true, pc, s, r, (bf16_t*)dx, lddx, (const bf16_t*)addend, ldadd);
  }
  r.CW = strip_width(C, C / G);
  const int nch = (C + r.CW - 1) / r.CW;
  if (r.CW > NT || nch > BATCH_CTR) return -2;
  const int ps = pick_psplit(nch, B, P);
  r.part = part_base(ws, B, C);
  if ((dgamma || ps > 1) && !(r.ctr = counter_slot())) return -4;
  sdmi_rt::launch(gn_bwd_reduce_kernel, dim3(nch, B, ps), dim3(NT), 0, s, r);
  SDMI_CHECK_LAUNCH();
  ApplyArgs a = {};
  a.x = (const bf16_t*)x; a.ldx = ldx; a.dy = (const bf16_t*)dy; a.lddy = lddy; a.dx = (bf16_t*)dx; a.lddx = lddx;
  a.tab = (const float4*)table2_ws; a.add = (const bf16_t*)addend; a.ldadd = ldadd;
  a.B = B; a.P = P; a.C = C; a.silu = silu;
  sdmi_rt::launch(gn_bwd_apply_kernel, apply_grid(B, P, C), dim3(NT), 0, s, a);
  SDMI_CHECK_LAUNCH();
  return 0;
}

// Backward from the dgrad GEMM's segment partials (sdmi_gemm_desc::gn_part, rb rows per segment)
int gn_bwd_part_impl(const void* x, int ldx, const void* dy, int lddy, void* dx, int lddx, const float* table,
                     const float* gamma, int B, int P, int C, int G, int silu, const float* part, int rb, float* ws,
                     float* dgamma, float* dbeta, float* rows_out, const void* addend, int ldadd, sdmi_stream_t stream) {
  if (B <= 0 || P <= 0 || rb <= 0 || P % rb || !part) return -1;
  StripArgs r;
  const int rc = gn_args(r, x, ldx, B, P, C, G, silu, gamma, dy, lddy, table, ws, dgamma, dbeta, rows_out);
  if (rc) return rc;
  if (ldx % 8 || lddy % 8 || lddx % 8 || (addend && ldadd % 8)) return -5;
  r.CW = part_strip_width(C, C / G);
  const int nch = (C + r.CW - 1) / r.CW;
  if (r.CW > NT || nch > BATCH_CTR) return -2;
  if (dgamma && !(r.ctr = counter_slot())) return -4;
  // pixel splits: >= 1024 workgroups while every split keeps >= 64 pixels
  int ps = 1;
  while ((long long)nch * B * ps < 1024 && P / (ps * 2) >= 64) ps *= 2;
  sdmi_rt::launch(gn_bwd_part_kernel, dim3(nch, B, ps), dim3(NT), 0, (hipStream_t)stream, r, (const float2*)part, rb,
                  (bf16_t*)dx, lddx, (const bf16_t*)addend, ldadd);
  SDMI_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// ---- C ABI (include/sdmi.h)
extern "C" size_t sdmi_chan_reduce_workspace(int B, int P, int C) {
  (void)P;
  const size_t nb = B > 32 ? B : 32;
  return (nb + nb * PS_MAX) * C * 2 * sizeof(float);
}

// stats -> per-(b,c) table {a = rstd*gamma, s = beta - mean*a, mean, rstd} (fp32 float4 [B][C])
extern "C" int sdmi_gn_stats(const void* x, int ldx, int B, int P, int C, int G, float eps, const float* gamma,
                             const float* beta, float* ws, float* table, sdmi_stream_t stream) {
  return gn_fwd_impl(x, ldx, nullptr, 0, B, P, C, G, eps, gamma, beta, 0, ws, table, stream);
}

// stats + apply in one call
extern "C" int sdmi_gn_fwd(const void* x, int ldx, void* y, int ldy, int B, int P, int C, int G, float eps,
                           const float* gamma, const float* beta, int silu, float* ws, float* table, sdmi_stream_t stream) {
  return gn_fwd_impl(x, ldx, y, ldy, B, P, C, G, eps, gamma, beta, silu, ws, table, stream);
}

extern "C" int sdmi_gn_apply(const void* x, int ldx, void* y, int ldy, const float* table, int B, int P, int C,
                             int silu, sdmi_stream_t stream) {
  if (C % 8) return -1;
  ApplyArgs a = {};
  a.x = (const bf16_t*)x; a.ldx = ldx; a.y = (bf16_t*)y; a.ldy = ldy;
  a.tab = (const float4*)table; a.B = B; a.P = P; a.C = C; a.silu = silu;
  sdmi_rt::launch(gn_apply_kernel, apply_grid(B, P, C), dim3(NT), 0, (hipStream_t)stream, a);
  SDMI_CHECK_LAUNCH();
  return 0;
}

extern "C" int sdmi_gn_bwd(const void* x, int ldx, const void* dy, int lddy, void* dx, int lddx, const float* table,
                           const float* gamma, int B, int P, int C, int G, int silu, float* ws, float* table2_ws,
                           float* dgamma, float* dbeta, const void* addend, int ldadd, sdmi_stream_t stream) {
  return gn_bwd_impl(x, ldx, dy, lddy, dx, lddx, table, gamma, B, P, C, G, silu, ws, table2_ws, dgamma, dbeta, nullptr,
                     addend, ldadd, stream);
}

extern "C" int sdmi_gn_bwd_rows(const void* x, int ldx, const void* dy, int lddy, void* dx, int lddx, const float* table,
                                const float* gamma, int B, int P, int C, int G, int silu, float* ws, float* table2_ws,
                                float* rows, const void* addend, int ldadd, sdmi_stream_t stream) {
  if (!rows) return -1;
  return gn_bwd_impl(x, ldx, dy, lddy, dx, lddx, table, gamma, B, P, C, G, silu, ws, table2_ws, nullptr, nullptr, rows,
                     addend, ldadd, stream);
}

extern "C" int sdmi_gn_bwd_part(const void* x, int ldx, const void* dy, int lddy, void* dx, int lddx, const float* table,
                                const float* gamma, int B, int P, int C, int G, int silu, const float* part, int rb,
                                float* ws, float* dgamma, float* dbeta, const void* addend, int ldadd,
                                sdmi_stream_t stream) {
  return gn_bwd_part_impl(x, ldx, dy, lddy, dx, lddx, table, gamma, B, P, C, G, silu, part, rb, ws, dgamma, dbeta,
                          nullptr, addend, ldadd, stream);
}

extern "C" int sdmi_gn_bwd_part_rows(const void* x, int ldx, const void* dy, int lddy, void* dx, int lddx,
                                     const float* table, const float* gamma, int B, int P, int C, int G, int silu,
                                     const float* part, int rb, float* ws, float* rows, const void* addend, int ldadd,
                                     sdmi_stream_t stream) {
  if (!rows) return -1;
  return gn_bwd_part_impl(x, ldx, dy, lddy, dx, lddx, table, gamma, B, P, C, G, silu, part, rb, ws, nullptr, nullptr,
                          rows, addend, ldadd, stream);
}

extern "C" int sdmi_gn_rows_sum_grouped(const sdmi_gn_rows_job* jobs, int njobs, sdmi_stream_t stream) {
  if (!jobs || njobs <= 0 || njobs > SDMI_GN_ROWS_GROUP_MAX) return -1;
  RowsGroup g = {};
  int cmax = 0;
  for (int i = 0; i < njobs; ++i) {
    const sdmi_gn_rows_job& J = jobs[i];
    if (!J.rows || !J.dgamma || !J.dbeta || J.B <= 0 || J.C <= 0 || ((uintptr_t)J.rows & 7)) return -1;
    g.j[i] = J;
    cmax = J.C > cmax ? J.C : cmax;
  }
  sdmi_rt::launch(gn_rows_sum_grouped_kernel, dim3((cmax + NT - 1) / NT, njobs), dim3(NT), 0, (hipStream_t)stream, g);
  SDMI_CHECK_LAUNCH();
  return 0;
}

// a group of one job
extern "C" int sdmi_gn_rows_sum(const float* rows, int B, int C, float* dgamma, float* dbeta, sdmi_stream_t stream) {
  const sdmi_gn_rows_job job = {rows, dgamma, dbeta, B, C};
  return sdmi_gn_rows_sum_grouped(&job, 1, stream);
}

// per-(b, c) and per-c sums of dy over pixels (bias and time-embedding-bias gradients)
extern "C" int sdmi_chan_sum(const void* dy, int lddy, int B, int P, int C, float* ws, void* per_bc, int ld_bc,
                             float* per_c, float* per_c2, int c_store, sdmi_stream_t stream) {
  if (c_store <= 0 || c_store > C) c_store = C;
  if (C % 8 || B <= 0 || P <= 0) return -1;
  StripArgs r = {};
  r.dy = (const bf16_t*)dy; r.ldy = lddy; r.B = B; r.P = P; r.C = C;
  r.per_bc = (bf16_t*)per_bc; r.ld_bc = ld_bc; r.c_store = c_store;
  r.sum1 = per_c; r.sum2 = per_c2; r.rows = ws;
  if (per_bc) {
    r.nb = B;
    r.seg = P;
  } else {  // only batch totals: cut the B*P rows into <= 32 contiguous segments of >= 64 rows
    const long long total = (long long)B * P;
    long long nb = total / 64;
    nb = nb < 1 ? 1 : (nb > 32 ? 32 : nb);
    r.seg = (total + nb - 1) / nb;
    r.nb = (int)((total + r.seg - 1) / r.seg);
  }
  r.CW = strip_width(C, 8);
  const int nch = (C + r.CW - 1) / r.CW;
  if (nch > BATCH_CTR || r.CW > NT) return -2;
  const int ps = pick_psplit(nch, r.nb, r.seg);
  r.part = part_base(ws, r.nb, C);
  if ((per_c || per_c2 || ps > 1) && !(r.ctr = counter_slot())) return -4;
  sdmi_rt::launch(chan_sum_kernel, dim3(nch, r.nb, ps), dim3(NT), 0, (hipStream_t)stream, r);
  SDMI_CHECK_LAUNCH();
  return 0;
}
