// ---------------------------------------------------------------------------------------------
// LDS-DMA pipelined variant: operands go global -> LDS with buffer_load ... lds (no VGPR staging, no
// ds_write), STAGES-deep ring, one barrier per 64-deep K tile. The LDS destination of a DMA
// wave-instruction is lane-linear (1 KiB per instruction), so the XOR swizzles of the LDS images are
// applied to the per-lane SOURCE addresses (logical chunk = physical slot ^ swizzle(row)); the
// fragment reads are unchanged. Out-of-range lanes (conv padding, ragged tiles) use an offset beyond
// the buffer record and the hardware writes zeros.
// ---------------------------------------------------------------------------------------------
// This header holds the kernel template and its launcher; gemm_dma_{rowmajor,conv,colmajor}.hip instantiate it for
// one A mode each, so the instantiations compile in parallel.
#pragma once
#include <algorithm>
#include <type_traits>

#include "gemm_device.h"
#include "gemm_epilogue.h"
#include "gemm_variants.h"

using namespace sdmi_gemm_impl;

namespace {

template <int N>
struct IC { static constexpr int value = N; };
struct RT { int value; };  // a runtime ring stage (K-contiguous-only kernels keep their plain loop)

// all LDS reads issued so far have landed; the fragments are re-defined after the wait so no consumer (an MFMA is
// register-only and would otherwise be hoisted above an asm wait) reads them earlier
template <int N>
__device__ __forceinline__ void lds_wait_frags(s16x8 (&f)[N]) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int i = 0; i < N; ++i) asm volatile("" : "+v"(f[i]));
}

__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rs, char* lds_wave_base, int off) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (SDMI_LDS void*)lds_wave_base, 16, off, 0, 0, 0);
}

// Tile shapes (TBM x TBN, NWN waves along N, TBM / 64 along M; every wave owns 64 x TBN/NWN):
//   128 x {64, 128, 192}, 4 waves (2 x 2): the default family -- 2 x <= 80 KiB of LDS fits two workgroups per CU;
//     N = 384 outputs split into 2 (not 3) 192-column tiles, so a 32768 x 384 conv is exactly 512 tiles = one round
//   256 x {128, 192}, 8 waves (4 x 2), B_NK: the large-M convolutions / linears -- 1.5x the MFMA work per byte staged
//   128 x {256, 384}, 8 waves (2 x 4), MN-contiguous B: weight gradients, whose N = 9 * cin is a multiple of 384
//   64 x {64, 128}, 4 waves (1 x 4), K-contiguous A and B: the latency-bound low-resolution GEMMs (M <= 8192, a grid
//     of <= 256 tiles, K of 8-40 k-tiles) with a 6-stage ring -- five 64-deep k-tiles in flight per workgroup, so the
//     DMA latency is paid about once per launch instead of once per k-tile
// The MN-contiguous (ds_read_b64_tr_b16) LDS images are kept as 128-column sub-tiles [64 k][128] (256-B rows).
// RED (col-major A only): reduction columns as extra MFMA tiles against synthesised B fragments (see reduce_frag).
template <int TBM, int NWN>
constexpr int dma_threads() { return 64 * (TBM / 64) * NWN; }

// KBK: k depth of one staged tile (64, or 32 for deeper rings in the same LDS: more bytes in flight per CU). Split-K
// slices stay in units of 64 (host k-tiles).
// KG (col-major A, the weight gradients): k-groups per workgroup. KG wave groups, each with its own LDS ring, compute
// the same output tile over interleaved k-tiles of the split's range (group g: tiles g, g + KG, ...); their fp32
// accumulators are summed through LDS in group order (deterministic) before the epilogue. A tile's k range then
// needs KG x fewer split-K slices for the same number of waves on the chip: fewer fp32 slabs written, read and reduced.
template <int TBM, int NWN, int KG>
constexpr int dma_min_waves(int ring_bytes) {
  return KG > 1 ? 2 : ((dma_threads<TBM, NWN>() == 256 && ring_bytes <= 80 * 1024) ? 2 : 1);
}

#ifdef SDMI_GEMM_TRACE
// Probe build only (scripts/gemm_phase_probe.py): per-workgroup phase timestamps of the LDS-DMA kernel, 100 MHz
// s_memrealtime -- entry, first k-tile landed, main loop done, epilogue done -- by thread 0, vector stores to Args::trace.
#define SDMI_TRACE_T(i) \
  do {                  \
    if (threadIdx.x == 0) tr_t[i] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#else
#define SDMI_TRACE_T(i) \
  do {                  \
  } while (0)
#endif

template <int AM, int BMODE, int STAGES, int TBN = BN, int TBM = BM, int NWN = 2, int RED = 0, int KBK = BK,
          bool GNE = false, int KG = 1>
__global__ __launch_bounds__((dma_threads<TBM, NWN>() * KG),
                             (dma_min_waves<TBM, NWN, KG>(STAGES * (TBM + TBN) * KBK * 2)))
void gemm_dma_kernel(const Args g, const EpiArgs e) {
  constexpr int NTH = dma_threads<TBM, NWN>() * KG;  // all threads; the DMA pieces are shared out per k-group
  constexpr int NW = NTH / 64 / KG;                    // waves per k-group
  constexpr int WTN = TBN / NWN;                     // columns per wave
  constexpr int NJ = WTN / 16;                       // 16-column MFMA tiles per wave
  constexpr bool A_MN = AM == SDMI_A_COLMAJOR, B_MN = BMODE != SDMI_B_NK;
  static_assert(KBK == 64 || KBK == 32, "staged k depth");
  constexpr int KS = KBK / 32;                        // MFMA k-steps per staged tile
  constexpr int RB = KBK * 2;                         // K-contiguous image row bytes
  constexpr int RPI = 1024 / RB, CPR = KBK / 8;       // rows per DMA wave-instruction, 16-B chunks per row
  constexpr int SUB = KBK * 256, IPS = KBK / 4;       // MN image: 128-column sub-tile bytes, DMA pieces per sub-tile
  constexpr int A_BYTES = TBM * KBK * 2, B_BYTES = TBN * KBK * 2;
  constexpr int STAGE_BYTES = A_BYTES + B_BYTES;     // A | B
  constexpr int A_PW = A_BYTES / 1024 / NW, B_PW = B_BYTES / 1024 / NW;  // DMA wave-instructions per tile
  static_assert(A_PW * NW * 1024 == A_BYTES && B_PW * NW * 1024 == B_BYTES, "DMA pieces per wave");
  static_assert(!A_MN || TBM % 128 == 0, "MN-contiguous A: 128-column sub-tiles");
  static_assert(!B_MN || TBN % 128 == 0, "MN-contiguous B: 128-column sub-tiles");
  static_assert(WTN % 16 == 0 && TBM % 64 == 0, "wave tile");
  static_assert(RED == 0 || A_MN, "reductions: col-major A only");
  static_assert(KG == 1 || TBM == 128, "k-groups: 128-row tiles");
  constexpr int RPW = RED == 0 ? 0 : (RED == 1 ? 1 : (3 + NWN - 1) / NWN);  // reduction tiles per wave (<= 3 total)
  extern __shared__ __attribute__((aligned(16))) char smem[];  // STAGES x (A | B)
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave_all = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably wave-uniform: scalar LDS bases / M0
  const int kg = wave_all / NW, wave = wave_all - kg * NW;            // k-group, wave within it
  char* const ring = smem + kg * STAGES * (TBM + TBN) * KBK * 2;       // this k-group's LDS ring
  const int wm = (wave / NWN) * 64, wn = (wave % NWN) * WTN;
#ifdef SDMI_GEMM_TRACE
  unsigned long long tr_t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
  SDMI_TRACE_T(0);
  const TileId tl = tile_id<TBN, TBM>();
  const int m0 = tl.m0, n0 = tl.n0;
  const Slice sl = slice_of<KBK>(g, tl.z);
  const int grp = sl.grp, z = sl.z, kt0 = sl.kt0, kt1 = sl.kt1;
  const bf16_t* const opA = sl.A;
  const bf16_t* const opB = sl.B;
  constexpr int OOB = (int)0x80000000;

  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)opA, (short)0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)opB, (short)0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsA2 =
      __builtin_amdgcn_make_buffer_rsrc((void*)(g.A2 ? g.A2 : opA), (short)0, 0x7fffffff, 0x00020000);

  // ---- per-lane, per-instruction coordinates, fixed over the K loop ----
  // instruction q = wave * PW + j writes 1 KiB at tile + q * 1024 (lane-linear):
  //   K-contiguous image: rows q*8 .. +8, lane -> row + lane>>3, physical slot lane&7
  //   MN-contiguous image: 128-column sub-tile q >> 4, k-rows (q & 15)*4 .. +4, lane -> k-row + lane>>4, slot lane&15
  int a_base[A_PW], b_base[B_PW];  // element offsets (without the k / pixel part)
  int a_kk[A_PW], b_kk[B_PW];      // k offset inside the tile (KC: chunk*8) or k-row (MN)
  bool a_ok[A_PW], b_ok[B_PW];
  int a_iy[A_PW], a_ix[A_PW], a_pb[A_PW], a_pix[A_PW];
  int b_ty[B_PW], b_tx[B_PW];
  const bool cin64 = AM == SDMI_A_CONV && g.cin % KBK == 0;  // k tile lies inside one tap
#pragma unroll
  for (int j = 0; j < A_PW; ++j) {
    const int q = wave * A_PW + j;
    if (A_MN) {
      int kr = (q % IPS) * 4 + (lane >> 4);
      int c = (lane & 15) ^ tr_swz(kr);
      int m = m0 + (q / IPS) * 128 + c * 8;
      a_ok[j] = m < g.M;
      a_base[j] = m;
      a_kk[j] = kr;
    } else {
      int r = q * RPI + lane / CPR;
      int c = (kc_off<KBK>(r, lane % CPR) - r * RB) >> 4;  // logical chunk of the lane's physical slot (involution)
      int m = m0 + r;
      a_ok[j] = m < g.M;
      a_kk[j] = c * 8;
      if (AM == SDMI_A_ROWMAJOR) {
        a_base[j] = m * g.lda;
      } else {
        int b, oy, ox;
        pixel_coords(g, m, b, oy, ox);
        a_pb[j] = b * g.ih;
        a_iy[j] = oy * g.sy + g.oy0;
        a_ix[j] = ox * g.sx + g.ox0;
        a_base[j] = m * g.lda2;  // second (K-concatenated) source row
        a_pix[j] = ((a_pb[j] + a_iy[j]) * g.iw + a_ix[j]) * g.ldx;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < B_PW; ++j) {
    const int q = wave * B_PW + j;
    if (!B_MN) {
      int r = q * RPI + lane / CPR;
      int c = (kc_off<KBK>(r, lane % CPR) - r * RB) >> 4;
      int n = n0 + r;
      b_ok[j] = n < g.N;
      b_base[j] = n * g.ldb;
      b_kk[j] = c * 8;
    } else {
      int kr = (q % IPS) * 4 + (lane >> 4);
      int c = (lane & 15) ^ tr_swz(kr);
      int n = n0 + (q / IPS) * 128 + c * 8;
      b_ok[j] = n < g.N;
      b_kk[j] = kr;
      b_base[j] = n;
      if (BMODE == SDMI_B_KN_CONV) {
        int tap = n / g.cin;
        int ci = n - tap * g.cin;
        b_ty[j] = tap / g.kw;
        b_tx[j] = tap - b_ty[j] * g.kw;
        b_base[j] = ci;
      }
    }
  }
  // implicit-im2col B, full k-tiles of a regular pixel grid (Args::bfast): the tile-invariant part of every lane's
  // gather offset, so issue_fast_b needs an add, a range check and a select per piece (no per-piece divisions)
  const int bform = BMODE == SDMI_B_KN_CONV ? ((g.bfast >> (KBK == 64 ? 0 : 2)) & 3) : 0;
  int bf_c[B_PW], bf_y[B_PW];
#pragma unroll
  for (int j = 0; j < B_PW; ++j) {
    bf_c[j] = OOB;
    bf_y[j] = -(1 << 29);
    if (BMODE == SDMI_B_KN_CONV && bform) {
      const int kr = b_kk[j];
      if (bform == 1) {  // lane row kr of the tile: row dy below the tile's first output row, column ox
        const int dy = (int)g.ow_d.div((unsigned)kr), ox = kr - dy * g.ow_d.d();
        const int ix = ox * g.sx + g.ox0 + b_tx[j];
        if (b_ok[j] && (unsigned)ix < (unsigned)g.iw) {
          bf_y[j] = dy * g.sy + g.oy0 + b_ty[j];
          bf_c[j] = (ix * g.ldx + b_base[j]) * 2;
        }
      } else {  // image db after the tile's first image, at (oy, ox)
        const int db = (int)g.ohw_d.div((unsigned)kr), r = kr - db * g.ohw_d.d();
        const int oy = (int)g.ow_d.div((unsigned)r), ox = r - oy * g.ow_d.d();
        const int iy = oy * g.sy + g.oy0 + b_ty[j], ix = ox * g.sx + g.ox0 + b_tx[j];
        if (b_ok[j] && (unsigned)iy < (unsigned)g.ih && (unsigned)ix < (unsigned)g.iw)
          bf_c[j] = (((db * g.ih + iy) * g.iw + ix) * g.ldx + b_base[j]) * 2;
      }
    }
  }

  // implicit-conv tap state (cin % 64 == 0): the (ty, tx, channel offset) of the next k-tile to issue, advanced
  // incrementally -- issue() is called for consecutive k-tiles -- instead of two runtime divisions per tile
  int c_ty = 0, c_tx = 0, c_ci = 0;
  // (k-groups: this group's first tile is kt0 + kg, and each issue advances KG tiles)
  if (AM == SDMI_A_CONV && cin64 && (kt0 + kg) * KBK < g.k_split) {
    const int tap = ((kt0 + kg) * KBK) / g.cin;
    c_ci = (kt0 + kg) * KBK - tap * g.cin;
    c_ty = tap / g.kw;
    c_tx = tap - c_ty * g.kw;
  }
  auto advance_tap = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < KG; ++q) {
      c_ci += KBK;
      if (c_ci >= g.cin) {
        c_ci = 0;
        if (++c_tx == g.kw) {
          c_tx = 0;
          ++c_ty;
        }
      }
    }
  };
  // Fast issue path for full k-tiles: every per-lane part of a DMA source offset is fixed over the K loop, the
  // per-tile part is wave-uniform (k0, or the conv tap shift), so a piece costs an add and a select instead of the
  // general path's coordinate math and bounds checks. Invalid lanes keep OOB (+ a uniform offset < 2^31: still out
  // of the 2^31 - 1 byte buffer record). Conv A (cin % KBK == 0): tap validity per lane is a precomputed bit mask.
  int a_v[A_PW], b_v[B_PW];
  unsigned a_tm[A_PW];
#pragma unroll
  for (int j = 0; j < A_PW; ++j) {
    a_tm[j] = 0u;
    if (AM == SDMI_A_ROWMAJOR) a_v[j] = a_ok[j] ? (a_base[j] + a_kk[j]) * 2 : OOB;
    else if (A_MN) a_v[j] = a_ok[j] ? (a_kk[j] * g.lda + a_base[j]) * 2 : OOB;
    else {
      a_v[j] = (a_pix[j] + a_kk[j]) * 2;
      if (cin64) {
        const int taps = g.k_split / g.cin;  // <= 16 (4x4 kernels)
        for (int tp = 0, ty = 0, tx = 0; tp < taps; ++tp) {
          const int iy = a_iy[j] + ty, ix = a_ix[j] + tx;
          if (a_ok[j] && (unsigned)iy < (unsigned)g.ih && (unsigned)ix < (unsigned)g.iw) a_tm[j] |= 1u << tp;
          if (++tx == g.kw) { tx = 0; ++ty; }
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < B_PW; ++j) {
    if (BMODE == SDMI_B_NK) b_v[j] = b_ok[j] ? (b_base[j] + b_kk[j]) * 2 : OOB;
    else if (BMODE == SDMI_B_KN) b_v[j] = b_ok[j] ? (b_kk[j] * g.ldb + b_base[j]) * 2 : OOB;
    else b_v[j] = 0;
  }

  // general issue path (ragged k-tiles, the fused second source, conv with cin % KBK != 0, the B im2col gather)
  auto issue_general_a = [&](int k0, char* sa) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < A_PW; ++j) {
      char* dst = sa + (wave * A_PW + j) * 1024;
      int off;
      if (AM == SDMI_A_ROWMAJOR) {
        int k = k0 + a_kk[j];
        off = (a_ok[j] && k < g.K) ? (a_base[j] + k) * 2 : OOB;
      } else if (A_MN) {
        int k = k0 + a_kk[j];
        off = (a_ok[j] && k < g.K) ? (k * g.lda + a_base[j]) * 2 : OOB;
      } else {
        int k = k0 + a_kk[j];
        if (k0 >= g.k_split) {  // fused 1x1 second source, tile-uniform (k_split % KBK == 0 on this path)
          off = (a_ok[j] && k < g.K) ? (a_base[j] + (k - g.k_split)) * 2 : OOB;
          dma16(rsA2, dst, off);
          continue;
        } else if (cin64) {
          // tap, and with it the (ty, tx) shift, is uniform over the tile (tracked incrementally)
          const int ty = c_ty, tx = c_tx;
          const int sh = (ty * g.iw + tx) * g.ldx + c_ci;
          int iy = a_iy[j] + ty, ix = a_ix[j] + tx;
          bool ok = a_ok[j] && (unsigned)iy < (unsigned)g.ih && (unsigned)ix < (unsigned)g.iw;
          off = ok ? (a_pix[j] + sh + a_kk[j]) * 2 : OOB;
        } else {
          int tap = k / g.cin;
          int ci = k - tap * g.cin;
          int ty = tap / g.kw, tx = tap - (tap / g.kw) * g.kw;
          int iy = a_iy[j] + ty, ix = a_ix[j] + tx;
          bool ok = a_ok[j] && k < g.k_split && (unsigned)iy < (unsigned)g.ih && (unsigned)ix < (unsigned)g.iw;
          off = ok ? (((a_pb[j] + iy) * g.iw + ix) * g.ldx + ci) * 2 : OOB;
        }
      }
      dma16(rsA, dst, off);
    }
    if (AM == SDMI_A_CONV && cin64 && k0 < g.k_split) advance_tap();
  };
  auto issue_general_b = [&](int k0, char* sb) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < B_PW; ++j) {
      char* dst = sb + (wave * B_PW + j) * 1024;
      int off;
      if (BMODE == SDMI_B_NK) {
        int k = k0 + b_kk[j];
        off = (b_ok[j] && k < g.K) ? (b_base[j] + k) * 2 : OOB;
      } else if (BMODE == SDMI_B_KN) {
        int k = k0 + b_kk[j];
        off = (b_ok[j] && k < g.K) ? (k * g.ldb + b_base[j]) * 2 : OOB;
      } else {
        int p = k0 + b_kk[j];
        int b, oy, ox;
        pixel_coords(g, p, b, oy, ox);
        int iy = oy * g.sy + g.oy0 + b_ty[j], ix = ox * g.sx + g.ox0 + b_tx[j];
        bool ok = b_ok[j] && p < g.K && (unsigned)iy < (unsigned)g.ih && (unsigned)ix < (unsigned)g.iw;
        off = ok ? (((b * g.ih + iy) * g.iw + ix) * g.ldx + b_base[j]) * 2 : OOB;
      }
      dma16(rsB, dst, off);
    }
  };

  // full k-tile of implicit-im2col B at pixel k0 (k0 % KBK == 0), bform != 0: the tile's image (and first output row)
  // are wave-uniform scalars
  auto issue_fast_b = [&](int k0, char* sb) __attribute__((always_inline)) {
    const int b = (int)g.ohw_d.div((unsigned)k0);
    const int sbase = b * g.ih * g.iw * g.ldx * 2;
    if (bform == 1) {
      const int soy = (int)g.ow_d.div((unsigned)(k0 - b * g.ohw_d.d())) * g.sy;
      const int rowb = g.iw * g.ldx * 2;
#pragma unroll
      for (int j = 0; j < B_PW; ++j) {
        const int iy = bf_y[j] + soy;
        dma16(rsB, sb + (wave * B_PW + j) * 1024, (unsigned)iy < (unsigned)g.ih ? sbase + iy * rowb + bf_c[j] : OOB);
      }
    } else {
#pragma unroll
      for (int j = 0; j < B_PW; ++j) dma16(rsB, sb + (wave * B_PW + j) * 1024, bf_c[j] + sbase);  // OOB stays OOB
    }
  };

  auto issue = [&](int kt, int stage) __attribute__((always_inline)) {
    char* sa = ring + stage * STAGE_BYTES;
    char* sb = sa + A_BYTES;
    const int k0 = kt * KBK;
    if (k0 + KBK <= g.K && (AM != SDMI_A_CONV || (cin64 && k0 + KBK <= g.k_split))) {
      const int tap = c_ty * g.kw + c_tx;
      const int ash = AM == SDMI_A_ROWMAJOR ? k0 * 2
                      : A_MN              ? k0 * g.lda * 2
                                          : ((c_ty * g.iw + c_tx) * g.ldx + c_ci) * 2;
#pragma unroll
      for (int j = 0; j < A_PW; ++j) {
        int off;
        if (AM == SDMI_A_CONV) off = ((a_tm[j] >> tap) & 1u) ? a_v[j] + ash : OOB;
        else off = a_v[j] + ash;
        dma16(rsA, sa + (wave * A_PW + j) * 1024, off);
      }
      if (AM == SDMI_A_CONV) advance_tap();
      if (BMODE != SDMI_B_KN_CONV) {
        const int bsh = BMODE == SDMI_B_NK ? k0 * 2 : k0 * g.ldb * 2;
#pragma unroll
        for (int j = 0; j < B_PW; ++j) dma16(rsB, sb + (wave * B_PW + j) * 1024, b_v[j] + bsh);
        return;
      }
      if (bform) {
        issue_fast_b(k0, sb);
        return;
      }
    } else {
      issue_general_a(k0, sa);
    }
    issue_general_b(k0, sb);
  };

  f32x4 acc[4][NJ];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // reduction tiles r = (wave % NWN) + rr * NWN of the tiles in column-tile 0 (workgroup-uniform)
  const bool red_tile = RED != 0 && n0 == 0;
  const int nred = RED == 0 ? 0 : (RED == 1 ? 1 : (8 + e.ngrp + 15) / 16);
  f32x4 accr[RPW > 0 ? RPW : 1][4];
#pragma unroll
  for (int rr = 0; rr < (RPW > 0 ? RPW : 1); ++rr)
#pragma unroll
    for (int i = 0; i < 4; ++i) accr[rr][i] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // this k-group's tiles of the split: local tile t is k-tile kt0 + t * KG + kg (KG == 1: all of them, in order)
  const int nt_all = kt1 - kt0;
  const int nt = nt_all > kg ? (nt_all - kg + KG - 1) / KG : 0;
  const int nt_loop = (nt_all + KG - 1) / KG;  // barrier count: every k-group runs the first group's trip count
  // Transposed (MN-contiguous) fragment reads: the lane's address at stage 0, k-step 0 is loop-invariant (one VGPR per
  // 16-row / 16-column fragment); stage, k-step and the +4-row half are immediates of ds_read_b64_tr_b16 when the ring
  // fits the 16-bit offset field, else the stage part is one add per fragment and stage. The loop body is unrolled
  // over the ring's stages so the stage index is a compile-time constant. (The round-4 loop recomputed every read
  // address from a runtime stage base: 44 VALU adds per 32 MFMAs in the weight-gradient kernel.)
  const unsigned ring_lds = (unsigned)(uintptr_t)(SDMI_LDS const char*)ring;
  unsigned fa_base[4], fb_base[NJ];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int mb = wm + 16 * i;
    fa_base[i] = ring_lds + (mb >> 7) * SUB + frag_tr_lane(mb & 127, lane);
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int nb = wn + 16 * j;
    fb_base[j] = ring_lds + A_BYTES + (nb >> 7) * SUB + frag_tr_lane(nb & 127, lane);
  }
  // largest immediate: last stage + last k-step + the +4-row half
  constexpr bool STAGE_IMM = (STAGES - 1) * STAGE_BYTES + (KS - 1) * 8192 + 1024 < 65536;
  static_assert(STAGES <= 6, "stage-unrolled loop");

  // one k-tile of this k-group at ring stage st_c (IC: compile time; RT: run time): wait, barrier, refill, MFMAs
  auto step = [&](int t, auto st_c) __attribute__((always_inline)) {
    using SC = decltype(st_c);
    constexpr bool CST = !std::is_same<SC, RT>::value;
    const int ST = st_c.value;
    // tile t landed for this thread: at most (tiles issued after t) x (A_PW + B_PW) DMA instructions outstanding
    // (in the last STAGES-2 tiles fewer are in flight: wait for all)
    if (STAGES > 2 && t + STAGES - 2 < nt)
      asm volatile("s_waitcnt vmcnt(%0)" ::"i"((STAGES > 2 ? STAGES - 2 : 0) * (A_PW + B_PW)) : "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every wave's DMA for tile t done; every wave done with tile t-1
    if (t == 0) SDMI_TRACE_T(1);
    if (KG > 1 && t >= nt) return;  // this k-group has no tile t (its last barriers only)
    if (t + STAGES - 1 < nt) issue(kt0 + (t + STAGES - 1) * KG + kg, (ST + STAGES - 1) % STAGES);
    const char* ta = ring + ST * STAGE_BYTES;
    const char* tb = ta + A_BYTES;
    (void)ta;
    (void)tb;
    constexpr int SOFF = [] {
      if constexpr (CST) return STAGE_IMM ? SC::value * STAGE_BYTES : 0;
      else return 0;
    }();
    unsigned fa_b[4], fb_b[NJ];
#pragma unroll
    for (int i = 0; i < 4; ++i) fa_b[i] = STAGE_IMM ? fa_base[i] : fa_base[i] + ST * STAGE_BYTES;
#pragma unroll
    for (int j = 0; j < NJ; ++j) fb_b[j] = STAGE_IMM ? fb_base[j] : fb_base[j] + ST * STAGE_BYTES;
    __builtin_amdgcn_s_setprio(1);
    auto kstep = [&](auto ks_c) __attribute__((always_inline)) {
      constexpr int ks = decltype(ks_c)::value;
      s16x8 fa[4], fb[NJ];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int mb = wm + 16 * i;
        if constexpr (A_MN) fa[i] = frag_tr_off<SOFF + ks * 8192>(fa_b[i]);
        else fa[i] = frag_kc<KBK>(ta, mb, ks, lane);
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int nb = wn + 16 * j;
        if constexpr (B_MN) fb[j] = frag_tr_off<SOFF + ks * 8192>(fb_b[j]);
        else fb[j] = frag_kc<KBK>(tb, nb, ks, lane);
      }
      if constexpr (A_MN) lds_wait_frags(fa);
      if constexpr (B_MN) lds_wait_frags(fb);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
      if (RED != 0 && red_tile) {
        const int kb = (kt0 + t * KG + kg) * KBK + ks * 32 + (lane >> 4) * 8;
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
          const int r = wave % NWN + rr * NWN;
          if (r < nred) {
            const s16x8 fr = reduce_frag<RED>(g, r, kb, lane);
#pragma unroll
            for (int i = 0; i < 4; ++i)
              accr[rr][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fr, accr[rr][i], 0, 0, 0);
          }
        }
      }
    };
    kstep(IC<0>{});
    if constexpr (KS > 1) kstep(IC<1>{});
    __builtin_amdgcn_s_setprio(0);
  };

  if (nt_loop > 0) {
    // prologue: STAGES-1 tiles in flight
#pragma unroll
    for (int s = 0; s < STAGES - 1; ++s)
      if (s < nt) issue(kt0 + s * KG + kg, s);
    // tile t sits in ring stage t % STAGES: with transposed reads the loop advances STAGES tiles per trip with the
    // stage as a constant; the K-contiguous-only kernels keep the plain loop (their reads fold the stage base
    // themselves, and the unrolled form measured slower for the 32^2 conv forward: 88 -> 93 us)
    if constexpr (!A_MN && !B_MN) {
      for (int t = 0; t < nt_loop; ++t) step(t, RT{t % STAGES});
    } else
    for (int t0 = 0; t0 < nt_loop; t0 += STAGES) {
      step(t0, IC<0>{});
      if constexpr (STAGES > 1) if (t0 + 1 < nt_loop) step(t0 + 1, IC<1 % STAGES>{});
      if constexpr (STAGES > 2) if (t0 + 2 < nt_loop) step(t0 + 2, IC<2 % STAGES>{});
      if constexpr (STAGES > 3) if (t0 + 3 < nt_loop) step(t0 + 3, IC<3 % STAGES>{});
      if constexpr (STAGES > 4) if (t0 + 4 < nt_loop) step(t0 + 4, IC<4 % STAGES>{});
      if constexpr (STAGES > 5) if (t0 + 5 < nt_loop) step(t0 + 5, IC<5 % STAGES>{});
    }
  }
  SDMI_TRACE_T(2);
  __syncthreads();
  SDMI_TRACE_T(4);
  if constexpr (KG > 1) {
    // k-group g > 0 hands its accumulators (and reduction-tile sums) to k-group 0 through LDS, one group after the
    // other in group order: a fixed summation order, so the result does not depend on timing. Lane-linear 16-B slots
    // (conflict-free ds_write_b128 / ds_read_b128); NE4 float4 per lane, one [NE4][64] block per wave.
    constexpr int NE4 = 4 * NJ + (RPW > 0 ? RPW : 1) * 4;
    float4* xs = (float4*)smem + (long long)wave * NE4 * 64 + lane;
#pragma unroll 1
    for (int src = 1; src < KG; ++src) {
      if (kg == src) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < NJ; ++j) xs[(i * NJ + j) * 64] = __builtin_bit_cast(float4, acc[i][j]);
        if constexpr (RED != 0) {
#pragma unroll
          for (int rr = 0; rr < RPW; ++rr)
#pragma unroll
            for (int i = 0; i < 4; ++i) xs[(4 * NJ + rr * 4 + i) * 64] = __builtin_bit_cast(float4, accr[rr][i]);
        }
      }
      __syncthreads();
      if (kg == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < NJ; ++j) acc[i][j] += __builtin_bit_cast(f32x4, xs[(i * NJ + j) * 64]);
        if constexpr (RED != 0) {
#pragma unroll
          for (int rr = 0; rr < RPW; ++rr)
#pragma unroll
            for (int i = 0; i < 4; ++i) accr[rr][i] += __builtin_bit_cast(f32x4, xs[(4 * NJ + rr * 4 + i) * 64]);
        }
      }
      __syncthreads();
    }
  }
  EpiArgs ev = epi_args_late(g, grp);  // epilogue arguments loaded only from here on
  // The column tiles of this kernel cover only the n GEMM columns; the reduction columns [n_x0, n_gemm) of a split-K
  // slab belong to the reduction tiles below. The last column tile's padding (n % TBN != 0) must not store its zero
  // accumulators there: it raced with the reduction tile's stores of the same slab entries (round-4 gsum probe).
  if (RED == 2) ev.n_gemm = ev.n_x0;
  const EpiArgs* ep = &ev;
  if (RED != 0 && red_tile && kg == 0) {
    // lane holds C[wm + 16i + 4(lane>>4) + q][r*16 + (lane & 15)]: column 0 = row sums, 8 + j = group j
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr) {
      const int col = (wave % NWN + rr * NWN) * 16 + (lane & 15);
      if (!(col == 0 || (RED == 2 && col >= 8 && col - 8 < ep->ngrp))) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = m0 + wm + 16 * i + 4 * (lane >> 4) + q;
          if (row >= ep->M) continue;
          const float v = accr[rr][i][q];
          if (ep->raw) ((float*)ep->ws)[(long long)z * ep->split_stride + (long long)row * ep->N + ep->n_x0 + col] = v;
          else Epi::extra(*ep, row, ep->n_x0 + col, &v, 1);
        }
    }
  }
  // only k-group 0 holds the tile (wm = -1: the other groups' waves stage nothing, but share the stores)
  SDMI_TRACE_T(5);
  gemm_epilogue<TBN, false, TBM, NJ, NTH, GNE>(*ep, acc, smem, m0, n0, kg == 0 ? wm : -1, wn, lane, z);
#ifdef SDMI_GEMM_TRACE
  SDMI_TRACE_T(3);
  if (threadIdx.x == 0) {
    const unsigned d = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if (d < (1u << 17)) {
#pragma unroll
      for (int i = 0; i < 8; ++i) g.trace[d * 8 + i] = tr_t[i];
    }
  }
#endif
}

template <int AM, int BMODE, int STAGES, int TBN, int TBM, int NWN, int RED, int KBK = BK, int KG = 1>
hipError_t launch_dma(const Args& a, const EpiArgs& e, dim3 grid, hipStream_t s) {
  constexpr int NTH = dma_threads<TBM, NWN>();
  constexpr size_t ring = (size_t)STAGES * (TBM + TBN) * KBK * 2 * KG, epi = (size_t)64 * (TBN + 4) * 4;
  if constexpr (RED == 0 && AM != SDMI_A_COLMAJOR && BMODE != SDMI_B_KN_CONV) {
    if (e.gn_part && !e.raw) {  // GroupNorm statistics: + the row-lane sums (NTH / (TBN / 8) x TBN x 2 floats)
      const size_t epi_gn = epi + (size_t)(NTH * KG / (TBN / 8)) * TBN * 2 * 4;
      size_t lds = std::max(ring, epi_gn);
      if constexpr (KG > 1) lds = std::max(lds, (size_t)(4 * (TBN / NWN / 16) + 4) * 16 * NTH);
      return launched(sdmi_rt::launch((gemm_dma_kernel<AM, BMODE, STAGES, TBN, TBM, NWN, 0, KBK, true, KG>), grid,
                                      dim3(NTH * KG), lds, s, a, e));
    }
  }
  if (e.gn_part && !e.raw) return hipErrorInvalidValue;
  if constexpr (KG > 1) {
    // + the k-group hand-off of the accumulators: (4 NJ + 4 RPW) float4 per lane, per wave of one group
    constexpr int NJ = TBN / NWN / 16, RPW = RED == 0 ? 1 : (RED == 1 ? 1 : (3 + NWN - 1) / NWN);
    constexpr size_t xs = (size_t)(4 * NJ + 4 * RPW) * 16 * NTH;
    static_assert(std::max(ring, std::max(epi, xs)) <= 160 * 1024, "LDS");
    return launched(sdmi_rt::launch((gemm_dma_kernel<AM, BMODE, STAGES, TBN, TBM, NWN, RED, KBK, false, KG>), grid,
                                    dim3(NTH * KG), std::max(ring, std::max(epi, xs)), s, a, e));
  }
  return launched(sdmi_rt::launch((gemm_dma_kernel<AM, BMODE, STAGES, TBN, TBM, NWN, RED, KBK>), grid, dim3(NTH),
                                  std::max(ring, epi), s, a, e));
}

// variant V of the table (gemm_variants.h) with its TI-th column tile, if that is tbn and the kernel exists for
// these modes; else the next tile
template <int AM, int BMODE, int RED, int V, int TI = 0>
hipError_t launch_variant(const Args& a, const EpiArgs& e, dim3 grid, hipStream_t s, int tbn) {
  if constexpr (TI < DMA_MAX_TILES) {
    constexpr DmaVariant d = DMA_VARIANTS[V];
    if constexpr (dma_instantiated(d, d.tbn[TI], AM, BMODE, RED)) {
      if (tbn == d.tbn[TI])
        return launch_dma<AM, BMODE, d.stages, d.tbn[TI], d.tbm, d.nwn, RED, d.kbk, d.kg>(a, e, grid, s);
    }
    return launch_variant<AM, BMODE, RED, V, TI + 1>(a, e, grid, s, tbn);
  }
  return hipErrorInvalidValue;
}

template <int AM, int BMODE, int RED>
hipError_t launch_dma_red(const Args& a, const EpiArgs& e, dim3 grid, hipStream_t s, int v, int tbn) {
  switch (v) {
#define SDMI_DMA_CASE(V) \
  case V: return launch_variant<AM, BMODE, RED, V>(a, e, grid, s, tbn);
    SDMI_DMA_CASE(2) SDMI_DMA_CASE(3) SDMI_DMA_CASE(4) SDMI_DMA_CASE(5) SDMI_DMA_CASE(6) SDMI_DMA_CASE(7)
    SDMI_DMA_CASE(8) SDMI_DMA_CASE(9) SDMI_DMA_CASE(10) SDMI_DMA_CASE(11)
#undef SDMI_DMA_CASE
  }
  return hipErrorInvalidValue;
}

// RED (col-major A, whose B is MN-contiguous): 2 reduction columns, 1 VALU row sums
template <int AM, int BMODE>
hipError_t launch_dma_ab(const Args& a, const EpiArgs& e, dim3 grid, hipStream_t s, int v, int tbn) {
  if constexpr (AM == SDMI_A_COLMAJOR) {
    if (a.n_x0) return launch_dma_red<AM, BMODE, 2>(a, e, grid, s, v, tbn);
    if (a.rowsum) return launch_dma_red<AM, BMODE, 1>(a, e, grid, s, v, tbn);
  }
  return launch_dma_red<AM, BMODE, 0>(a, e, grid, s, v, tbn);
}

}  // namespace

// the B modes A mode AM is paired with (col-major A with [n][k] B has no DMA kernel)
template <int AM>
hipError_t sdmi_gemm_impl::launch_dma_mode(int b_mode, const Args& a, const EpiArgs& e, dim3 grid, hipStream_t s, int v,
                                      int tbn) {
  if constexpr (AM != SDMI_A_COLMAJOR)
    if (b_mode == SDMI_B_NK) return launch_dma_ab<AM, SDMI_B_NK>(a, e, grid, s, v, tbn);
  if constexpr (AM != SDMI_A_CONV)
    if (b_mode == SDMI_B_KN) return launch_dma_ab<AM, SDMI_B_KN>(a, e, grid, s, v, tbn);
  if constexpr (AM == SDMI_A_COLMAJOR)
    if (b_mode == SDMI_B_KN_CONV) return launch_dma_ab<AM, SDMI_B_KN_CONV>(a, e, grid, s, v, tbn);
  return hipErrorInvalidValue;
}

