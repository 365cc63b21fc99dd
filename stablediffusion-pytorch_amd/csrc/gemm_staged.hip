// The register-staged GEMM kernel (variant 0 of gemm.hip) and its launcher.
//
// Tile 128x128x64, 256 threads = 4 waves (2x2), each wave 64x64 = 4x4 MFMA 16x16x32 bf16 tiles.
// Operands are register-staged (so the conv gathers can zero-pad) into two LDS buffers:
//   "K-contiguous" tiles [128 rows][64 k] (A row-major / conv, B [n][k]) read with ds_read_b128,
//      16-B chunk c of row r stored at chunk (c ^ (r & 7))  -> conflict-free b128 fragment reads;
//   "MN-contiguous" tiles [64 k][128 cols] (A col-major, B [k][n]) read with ds_read_b64_tr_b16
//      (hardware transpose), chunk c of row r stored at c ^ (((r&3) | ((r>>1)&4)) << 1)
//      -> conflict-free transposed reads.
#include "gemm_device.h"
#include "gemm_epilogue.h"

using namespace sdmi_gemm_impl;

namespace {

constexpr int TILE_BYTES = 128 * 64 * 2;  // 16 KiB per operand tile (both layouts)

// RED (col-major A only): 0 plain GEMM, 1 + VALU row sums of A (bias gradient), 2 + synthesised reduction columns
// (bias and per-group sums) -- compile-time so the plain instantiations carry none of it
template <int AM, int BMODE, int RED = 0, bool GNE = false>
__global__ __launch_bounds__(NT, 2) void gemm_kernel(const Args g, const EpiArgs e) {
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE_BYTES];
  // buffer b: A tile at smem + 2*b*TILE_BYTES, B tile right after it
#define SA(b) (smem + (b) * 2 * TILE_BYTES)
#define SB(b) (smem + (b) * 2 * TILE_BYTES + TILE_BYTES)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const TileId tl = tile_id();
  const int m0 = tl.m0, n0 = tl.n0;
  const Slice sl = slice_of(g, tl.z);
  const int grp = sl.grp, z = sl.z, kt0 = sl.kt0, kt1 = sl.kt1;
  const bf16_t* const opA = sl.A;
  const bf16_t* const opB = sl.B;

  // ---------------- per-thread staging coordinates ----------------
  // K-contiguous staging: rows (tid>>3)+32i, chunk tid&7.   MN-contiguous: k-rows (tid>>4)+16i, chunk tid&15.
  int a_pb[4], a_iy[4], a_ix[4];
  bool a_ok[4];
  if (AM == SDMI_A_CONV) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int m = m0 + (tid >> 3) + 32 * i;
      a_ok[i] = m < g.M;
      int b, oy, ox;
      pixel_coords(g, m, b, oy, ox);
      a_pb[i] = b * g.ih;
      a_iy[i] = oy * g.sy + g.oy0;
      a_ix[i] = ox * g.sx + g.ox0;
    }
  }
  int b_ty = 0, b_tx = 0, b_ci = 0;
  bool b_nok = true;
  if (BMODE == SDMI_B_KN_CONV) {
    int n = n0 + (tid & 15) * 8;
    b_nok = n < g.N;
    int tap = n / g.cin;
    b_ci = n - tap * g.cin;
    b_ty = tap / g.kw;
    b_tx = tap - b_ty * g.kw;
  }

  uint4 ra[4], rb[4];
  // Buffer descriptors: out-of-range offsets return zeros in hardware, which is how padding taps,
  // ragged tiles and k >= K are zero-filled without a select on a pointer.
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)opA, (short)0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)opB, (short)0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsA2 =
      __builtin_amdgcn_make_buffer_rsrc((void*)(g.A2 ? g.A2 : opA), (short)0, 0x7fffffff, 0x00020000);
  constexpr int OOB = (int)0x80000000;
#define BUF_LD(rs, off) __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128((rs), (off), 0, 0))

  auto load_tiles = [&](int kt) __attribute__((always_inline)) {
    const int k0 = kt * BK;
    // ---- A ----
    if (AM == SDMI_A_ROWMAJOR) {
      int k = k0 + (tid & 7) * 8;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int m = m0 + (tid >> 3) + 32 * i;
        int off = (m < g.M && k < g.K) ? (m * g.lda + k) * 2 : OOB;
        ra[i] = BUF_LD(rsA, off);
      }
    } else if (AM == SDMI_A_CONV) {
      int k = k0 + (tid & 7) * 8;
      if (k >= g.k_split) {  // K-concatenated second source: plain row-major rows (fused 1x1 conv)
        int kk = k - g.k_split;
        bool kok = k < g.K;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          int m = m0 + (tid >> 3) + 32 * i;
          int off = (kok && a_ok[i]) ? (m * g.lda2 + kk) * 2 : OOB;
          ra[i] = BUF_LD(rsA2, off);
        }
      } else {
        int tap = k / g.cin;
        int ci = k - tap * g.cin;
        int ty = tap / g.kw;
        int tx = tap - ty * g.kw;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          int iy = a_iy[i] + ty, ix = a_ix[i] + tx;
          bool ok = a_ok[i] && (unsigned)iy < (unsigned)g.ih && (unsigned)ix < (unsigned)g.iw;
          int off = ok ? (((a_pb[i] + iy) * g.iw + ix) * g.ldx + ci) * 2 : OOB;
          ra[i] = BUF_LD(rsA, off);
        }
      }
    } else {  // col-major A: A[k*lda + m]
      int m = m0 + (tid & 15) * 8;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int k = k0 + (tid >> 4) + 16 * i;
        int off = (m < g.M && k < g.K) ? (k * g.lda + m) * 2 : OOB;
        ra[i] = BUF_LD(rsA, off);
      }
    }
    // ---- B ----
    if (BMODE == SDMI_B_NK) {
      int k = k0 + (tid & 7) * 8;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int n = n0 + (tid >> 3) + 32 * i;
        int off = (n < g.N && k < g.K) ? (n * g.ldb + k) * 2 : OOB;
        rb[i] = BUF_LD(rsB, off);
      }
    } else if (RED == 2 && n0 + (tid & 15) * 8 >= g.n_x0) {  // reduction columns (both MN-contiguous B modes)
      const int n = n0 + (tid & 15) * 8;
#pragma unroll
      for (int i = 0; i < 4; ++i) rb[i] = reduction_cols(g, n, k0 + (tid >> 4) + 16 * i);
    } else if (BMODE == SDMI_B_KN) {
      int n = n0 + (tid & 15) * 8;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int k = k0 + (tid >> 4) + 16 * i;
        int off = (n < g.N && k < g.K) ? (k * g.ldb + n) * 2 : OOB;
        rb[i] = BUF_LD(rsB, off);
      }
    } else {  // conv gather, k = pixel of the (oh x ow) grid
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int p = k0 + (tid >> 4) + 16 * i;
        int b, oy, ox;
        pixel_coords(g, p, b, oy, ox);
        int iy = oy * g.sy + g.oy0 + b_ty, ix = ox * g.sx + g.ox0 + b_tx;
        bool ok = b_nok && p < g.K && (unsigned)iy < (unsigned)g.ih && (unsigned)ix < (unsigned)g.iw;
        int off = ok ? (((b * g.ih + iy) * g.iw + ix) * g.ldx + b_ci) * 2 : OOB;
        rb[i] = BUF_LD(rsB, off);
      }
    }
  };

  auto store_tiles = [&](int buf) __attribute__((always_inline)) {
    if (AM == SDMI_A_COLMAJOR) {
#pragma unroll
      for (int i = 0; i < 4; ++i) *(uint4*)(SA(buf) + tr_off((tid >> 4) + 16 * i, tid & 15)) = ra[i];
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) *(uint4*)(SA(buf) + kc_off((tid >> 3) + 32 * i, tid & 7)) = ra[i];
    }
    if (BMODE == SDMI_B_NK) {
#pragma unroll
      for (int i = 0; i < 4; ++i) *(uint4*)(SB(buf) + kc_off((tid >> 3) + 32 * i, tid & 7)) = rb[i];
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) *(uint4*)(SB(buf) + tr_off((tid >> 4) + 16 * i, tid & 15)) = rb[i];
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // VALU row sums of col-major A (Args::rowsum) by the workgroups of n-tile 0: m = m0 + (tid & 15) * 8 + e
  const bool rowsum = RED == 1 && n0 == 0;
  float rs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  auto sum_rows = [&]() __attribute__((always_inline)) {
    if (rowsum) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float t[8];
        unpack8(ra[i], t);
#pragma unroll
        for (int q = 0; q < 8; ++q) rs[q] += t[q];
      }
    }
  };

  if (kt0 < kt1) {
    load_tiles(kt0);
    sum_rows();
    store_tiles(0);
    __syncthreads();
    int cur = 0;
    for (int kt = kt0; kt < kt1; ++kt) {
      const bool more = kt + 1 < kt1;
      if (more) load_tiles(kt + 1);
      const char* ta = SA(cur);
      const char* tb = SB(cur);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        s16x8 fa[4], fb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          fa[i] = (AM == SDMI_A_COLMAJOR) ? frag_tr(ta, wm + 16 * i, ks, lane) : frag_kc(ta, wm + 16 * i, ks, lane);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          fb[j] = (BMODE == SDMI_B_NK) ? frag_kc(tb, wn + 16 * j, ks, lane) : frag_tr(tb, wn + 16 * j, ks, lane);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
      }
      if (more) {
        sum_rows();
        store_tiles(cur ^ 1);
      }
      __syncthreads();
      cur ^= 1;
    }
  }
  // The epilogue arguments are read through a laundered pointer into the kernel-argument segment: the compiler
  // cannot hoist those scalar loads above this point, so ~50 EpiArgs fields are not held (and spilled) in SGPRs
  // across the main loop.
  const EpiArgs ev = epi_args_late(g, grp);
  const EpiArgs* ep = &ev;
  if (rowsum) {  // combine the 16 k-row lanes of each 8-column chunk in LDS (workgroup-uniform branch)
    float* red = (float*)smem;  // [16][128]
#pragma unroll
    for (int q = 0; q < 8; ++q) red[(tid >> 4) * 128 + (tid & 15) * 8 + q] = rs[q];
    __syncthreads();
    if (tid < BM) {
      float t = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) t += red[r * 128 + tid];
      const int m = m0 + tid;
      if (m < ep->M) {
        if (ep->raw) {  // slab column n_x0 of this split (the reducer routes it to sum_out / sum_out2)
          ((float*)ep->ws)[(long long)z * ep->split_stride + (long long)m * ep->N + ep->n_x0] = t;
        } else if (m < ep->m_store) {
          if (ep->sum_out) ep->sum_out[m] = t;
          if (ep->sum_out2) ep->sum_out2[m] = t;
        }
      }
    }
    __syncthreads();
  }

  gemm_epilogue<BN, RED == 2, BM, BN / 32, NT, GNE>(*ep, acc, smem, m0, n0, wm, wn, lane, z);
}

template <int AM, int BMODE>
hipError_t launch_ab(const Args& a, const EpiArgs& e, dim3 grid, hipStream_t s) {
  if constexpr (AM == SDMI_A_COLMAJOR) {
    if (a.rowsum) return launched(sdmi_rt::launch((gemm_kernel<AM, BMODE, 1>), grid, dim3(NT), 0, s, a, e));
    if (a.n_x0) return launched(sdmi_rt::launch((gemm_kernel<AM, BMODE, 2>), grid, dim3(NT), 0, s, a, e));
  }
  if constexpr (AM != SDMI_A_COLMAJOR && BMODE != SDMI_B_KN_CONV) {
    if (e.gn_part && !e.raw)
      return launched(sdmi_rt::launch((gemm_kernel<AM, BMODE, 0, true>), grid, dim3(NT), 0, s, a, e));
  }
  if (e.gn_part && !e.raw) return hipErrorInvalidValue;
  return launched(sdmi_rt::launch((gemm_kernel<AM, BMODE>), grid, dim3(NT), 0, s, a, e));
}

}  // namespace

hipError_t sdmi_gemm_impl::launch_staged(int a_mode, int b_mode, const Args& a, const EpiArgs& e, dim3 grid, hipStream_t s) {
  switch (a_mode * 3 + b_mode) {
    case SDMI_A_ROWMAJOR * 3 + SDMI_B_NK: return launch_ab<SDMI_A_ROWMAJOR, SDMI_B_NK>(a, e, grid, s);
    case SDMI_A_ROWMAJOR * 3 + SDMI_B_KN: return launch_ab<SDMI_A_ROWMAJOR, SDMI_B_KN>(a, e, grid, s);
    case SDMI_A_CONV * 3 + SDMI_B_NK: return launch_ab<SDMI_A_CONV, SDMI_B_NK>(a, e, grid, s);
    case SDMI_A_COLMAJOR * 3 + SDMI_B_KN: return launch_ab<SDMI_A_COLMAJOR, SDMI_B_KN>(a, e, grid, s);
    case SDMI_A_COLMAJOR * 3 + SDMI_B_KN_CONV: return launch_ab<SDMI_A_COLMAJOR, SDMI_B_KN_CONV>(a, e, grid, s);
  }
  return hipErrorInvalidValue;
}
