// The split-K reducers of sdmi_gemm: the GEMM kernels write fp32 slabs (EpiArgs::raw), these sum them in a fixed
// order and apply the same epilogue.
#include <algorithm>

#include "gemm_epilogue.h"

using namespace sdmi_gemm_impl;

namespace {

// Sum split-K slabs and apply the epilogue, N % 8 == 0 (16-B slab reads). A workgroup owns 256/SL consecutive
// 8-column items; its SL slab lanes sum disjoint slab subsets (a wave reads 64 consecutive items of ONE slab:
// contiguous 2 KiB) and are merged in LDS in a fixed order, so the result is deterministic. SL > 1 spreads the
// deep split-K of small weight gradients (a 128 x 128 dW = 2048 items) over enough workgroups to fill the chip.
template <int SL>
__global__ __launch_bounds__(256) void splitk_reduce_n8_kernel(const EpiArgs g0) {
  EpiArgs g = g0;  // grid.y = problem of a grouped launch
  if (blockIdx.y) group_epi(g, g0.Cg[blockIdx.y], g0.sum_g[blockIdx.y], blockIdx.y);
  constexpr int IPB = 256 / SL;
  __shared__ float4 part[SL > 1 ? SL : 1][IPB][2];
  const float* ws = g.ws;
  const unsigned N8 = g.N >> 3;
  const unsigned total = (unsigned)g.M * N8;
  const int zs = (int)g.split_stride;
  const int li = threadIdx.x % IPB, sl = threadIdx.x / IPB;
  for (unsigned i0 = blockIdx.x * IPB; i0 < total; i0 += gridDim.x * IPB) {  // uniform trip count per block
    const unsigned idx = i0 + li;
    // 32-bit index math (slabs are < 2^31 bytes) and a multiply-high row split: no 64-bit division per chunk
    const unsigned r = g.n8_magic ? __umulhi(idx, g.n8_magic) : (N8 == 1 ? idx : idx / N8);
    const int row = (int)r, col = (int)(idx - r * N8) * 8;
    const int base = row * g.N + col;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (idx < total) {
      for (int zz = sl; zz < g.nsplit; zz += SL) {
        const float* p = ws + zz * zs + base;
        const float4 x = *(const float4*)p, y = *(const float4*)(p + 4);
        a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w;
        b.x += y.x; b.y += y.y; b.z += y.z; b.w += y.w;
      }
    }
    if constexpr (SL > 1) {
      part[sl][li][0] = a;
      part[sl][li][1] = b;
      __syncthreads();
      if (sl == 0) {
#pragma unroll
        for (int q = 1; q < SL; ++q) {
          const float4 x = part[q][li][0], y = part[q][li][1];
          a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w;
          b.x += y.x; b.y += y.y; b.z += y.z; b.w += y.w;
        }
      }
      __syncthreads();
    }
    if (sl == 0 && idx < total) {
      float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
      if (g.n_x0 && col >= g.n_x0) {
        Epi::extra(g, row, col, v, 8);
      } else if (g.vec) {
        if (row < g.m_store && col < g.n_store) Epi::finish8(g, row, col, v);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) Epi::store_final(g, row, col + e, v[e]);
      }
    }
  }
}

// Sum split-K slabs, store bf16(alpha * sum) and the GroupNorm-backward statistics (EpiArgs::gn_part): grid
// (ceil(N / 256), M / gn_rb); 256 threads = 32 column chunks x 8 row lanes, the row lanes summed in LDS in a fixed
// order into the segment's column partials (same arithmetic as epi_gn_half).
__global__ __launch_bounds__(256) void splitk_reduce_gn_kernel(const EpiArgs e) {
  __shared__ float red[8][256][2];
  const int t = threadIdx.x, c8 = t & 31, rl0 = t >> 5;
  const int col = blockIdx.x * 256 + c8 * 8;
  const int r0 = blockIdx.y * e.gn_rb;
  const bool on = col < e.N;
  float u[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, w[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (on) {
    const int b = (int)e.gn_pd.div((unsigned)r0);
    float4 tb[8];
    const float4* tp = e.gn_tab + (long long)b * e.N + col;
#pragma unroll
    for (int q = 0; q < 8; ++q) tb[q] = tp[q];
    const int zs = (int)e.split_stride;
#pragma unroll 1
    for (int rl = rl0; rl < e.gn_rb; rl += 8) {
      const int row = r0 + rl;
      // the slab sum in splitk_reduce_n8_kernel<gn_sl>'s order: lane l sums slabs l, l + SL, ... in order, then the
      // lanes are added in lane order -- so the stored dy is bitwise the reducer's without the statistics
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), c = a;
      const float* p = e.ws + (long long)row * e.N + col;
#pragma unroll 1
      for (int l = 0; l < e.gn_sl; ++l) {
        float4 pa = make_float4(0.f, 0.f, 0.f, 0.f), pc = pa;
#pragma unroll 4
        for (int zz = l; zz < e.nsplit; zz += e.gn_sl) {
          const float4 x = *(const float4*)(p + (long long)zz * zs), y = *(const float4*)(p + (long long)zz * zs + 4);
          pa.x += x.x; pa.y += x.y; pa.z += x.z; pa.w += x.w;
          pc.x += y.x; pc.y += y.y; pc.z += y.z; pc.w += y.w;
        }
        if (l == 0) {
          a = pa;
          c = pc;
        } else {
          a.x += pa.x; a.y += pa.y; a.z += pa.z; a.w += pa.w;
          c.x += pc.x; c.y += pc.y; c.z += pc.z; c.w += pc.w;
        }
      }
      float v[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] *= e.alpha;
      const uint4 xr = *(const uint4*)(e.gn_x + (long long)row * e.gn_ldx + col);
      const uint4 pk = pack8(v);
      *(uint4*)((bf16_t*)e.C + (long long)row * e.ldc + col) = pk;
      unpack8(pk, v);
      gn_accum(e, v, xr, tb, u, w);
    }
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    red[rl0][c8 * 8 + q][0] = u[q];
    red[rl0][c8 * 8 + q][1] = w[q];
  }
  __syncthreads();
  const int j = blockIdx.x * 256 + t;
  if (j < e.N) {
    float a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      a1 += red[r][t][0];
      a2 += red[r][t][1];
    }
    *(float2*)(e.gn_part + ((long long)blockIdx.y * e.N + j) * 2) = make_float2(a1, a2);
  }
}

// Sum split-K slabs and apply the epilogue, general N (one element per thread).
__global__ void splitk_reduce_kernel(const EpiArgs g0) {
  EpiArgs g = g0;  // grid.y = problem of a grouped launch
  if (blockIdx.y) group_epi(g, g0.Cg[blockIdx.y], g0.sum_g[blockIdx.y], blockIdx.y);
  const float* ws = g.ws;
  long long stride = (long long)gridDim.x * blockDim.x;
  long long total = (long long)g.M * g.N;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
    float s = 0.f;
    for (int zz = 0; zz < g.nsplit; ++zz) s += ws[(long long)zz * g.split_stride + idx];
    int row = (int)(idx / g.N), col = (int)(idx - (long long)row * g.N);
    if (row < g.M && col < g.N) Epi::store_final(g, row, col, s);
  }
}

// slab lanes of the n8 reducer: aim for >= 1024 workgroups
int reduce_lanes(const EpiArgs& red) {
  const long long items = (long long)red.M * (red.N / 8);
  int sl = 1;
  while (sl < 32 && sl * 2 <= red.nsplit && items * sl / 256 < 1024) sl *= 2;
  return sl;
}

}  // namespace

hipError_t sdmi_gemm_impl::launch_reduce(const EpiArgs& red, hipStream_t s, int G) {
  if (red.gn_part) {
    EpiArgs r = red;
    r.gn_sl = reduce_lanes(red);
    return launched(sdmi_rt::launch(splitk_reduce_gn_kernel,
                                    dim3((unsigned)((red.N + 255) / 256), (unsigned)(red.M / red.gn_rb)), dim3(256), 0, s, r));
  }
  if (!red.n8) {
    const long long total = (long long)red.M * red.N;
    return launched(sdmi_rt::launch(splitk_reduce_kernel, dim3((unsigned)std::min<long long>((total + 255) / 256, 4096), G),
                                    dim3(256), 0, s, red));
  }
  const long long items = (long long)red.M * (red.N / 8);
  const int sl = reduce_lanes(red);
  const unsigned blocks = (unsigned)std::min<long long>((items * sl + 255) / 256, 8192);
  const dim3 grid(blocks, G);  // y: problem of a grouped launch
  switch (sl) {
    case 1: return launched(sdmi_rt::launch(splitk_reduce_n8_kernel<1>, grid, dim3(256), 0, s, red));
    case 2: return launched(sdmi_rt::launch(splitk_reduce_n8_kernel<2>, grid, dim3(256), 0, s, red));
    case 4: return launched(sdmi_rt::launch(splitk_reduce_n8_kernel<4>, grid, dim3(256), 0, s, red));
    case 8: return launched(sdmi_rt::launch(splitk_reduce_n8_kernel<8>, grid, dim3(256), 0, s, red));
    case 16: return launched(sdmi_rt::launch(splitk_reduce_n8_kernel<16>, grid, dim3(256), 0, s, red));
    default: return launched(sdmi_rt::launch(splitk_reduce_n8_kernel<32>, grid, dim3(256), 0, s, red));
  }
}

