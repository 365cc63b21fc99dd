// Device helpers shared by the GEMM kernels (gemm_staged.hip, gemm_dma.h): gather coordinates, the synthesised
// reduction columns, the swizzled LDS images and their fragment readers, the tile order, and the per-workgroup
// prologue / late epilogue-argument load of a (possibly grouped) launch.
#pragma once
#include "gemm_args.h"

namespace sdmi_gemm_impl {

__device__ __forceinline__ void pixel_coords(const Args& g, int m, int& b, int& oy, int& ox) {
  b = (int)g.ohw_d.div((unsigned)m);
  const int r = m - b * g.ohw_d.d();
  oy = (int)g.ow_d.div((unsigned)r);
  ox = r - oy * g.ow_d.d();
}

// 8 synthesised B values (one 16-B chunk, columns [n, n + 8)) of the reduction columns at k (see Args::n_x0):
// bf16 1.0 where the column's indicator holds, 0 elsewhere and for k >= K
__device__ __forceinline__ uint4 reduction_cols(const Args& g, int n, int k) {
  uint4 r = make_uint4(0u, 0u, 0u, 0u);
  if (k >= g.K) return r;
  const int j = n - g.n_x0;
  const int d = j == 0 ? 0 : (int)g.grp_d.div((unsigned)k) - (j - 8);
  if (d < 0 || d >= 8) return r;
  const unsigned one = 0x3F80u << ((d & 1) * 16);  // bf16 1.0 in the low / high half of the 32-bit lane
  if ((d >> 1) == 0) r.x = one;
  else if ((d >> 1) == 1) r.y = one;
  else if ((d >> 1) == 2) r.z = one;
  else r.w = one;
  return r;
}

// B fragment (8 k-values of one column, lane layout of mfma_f32_16x16x32_bf16: k = kb .. kb+7, column = lane & 15)
// of reduction tile r: column 0 all ones (row sums: bias gradient), column 8 + j the indicator of group j = k / grp
// (per-sample sums: time-embedding gradient; needs grp % 8 == 0 so 8 consecutive k share one group)
template <int RED>
__device__ __forceinline__ s16x8 reduce_frag(const Args& g, int r, int kb, int lane) {
  const int col = r * 16 + (lane & 15);
  bool one = col == 0;
  if (RED == 2 && col >= 8) one = (int)g.grp_d.div((unsigned)kb) == col - 8;
  const short v = one ? (short)0x3F80 : (short)0;
  return (s16x8){v, v, v, v, v, v, v, v};
}

// K-contiguous LDS image with KBK-deep rows: 128-B rows (KBK 64), chunk c of row r at slot c ^ (r & 7); 64-B rows
// (KBK 32), chunk c at slot c ^ f((r >> 2) & 3) with f = {0, 2, 3, 1}: the four ds_read_b128 lane groups of a
// fragment read (rows 0-15 x chunks 0-3) then each hit 16 distinct 16-B slots of the 256-B bank row
template <int KBK = BK>
__device__ __forceinline__ int kc_off(int r, int c) {
  if constexpr (KBK == 64) return r * 128 + ((c ^ (r & 7)) << 4);
  return r * 64 + ((c ^ ((0x1320 >> (((r >> 2) & 3) * 4)) & 3)) << 4);
}
// MN-contiguous LDS image [64 k][128 cols] (256-B rows)
__device__ __forceinline__ int tr_swz(int r) { return ((r & 3) | ((r >> 1) & 4)) << 1; }
__device__ __forceinline__ int tr_off(int r, int c) { return r * 256 + ((c ^ tr_swz(r)) << 4); }

template <int KBK = BK>
__device__ __forceinline__ s16x8 frag_kc(const char* tile, int rbase, int ks, const int& lane) {
  int r = rbase + (lane & 15);
  int c = ks * 4 + (lane >> 4);
  return *(const s16x8*)(tile + kc_off<KBK>(r, c));
}

// transposed fragment read through the builtin (register-staged kernel)
__device__ __forceinline__ s16x8 frag_tr(const char* tile, int cbase, int ks, const int& lane) {
  int gq = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  int r1 = ks * 32 + gq * 8 + q;
  int c = (cbase >> 3) + (p >> 1);
  int o1 = tr_off(r1, c) + (p & 1) * 8;
  int o2 = tr_off(r1 + 4, c) + (p & 1) * 8;
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((SDMI_LDS s16x4*)(tile + o1));
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((SDMI_LDS s16x4*)(tile + o2));
  s16x8 r;
  r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
  r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  return r;
}

// Transposed fragment read for the LDS-DMA kernels, as inline asm. hipcc (ROCm 7.2) cannot prove a
// ds_read_b64_tr_b16 builtin disjoint from the LDS-DMA writes in flight and emits s_waitcnt vmcnt(0) before it --
// which drains the prefetch of the NEXT k-tile issued just before (measured: every DMA kernel with an MN-contiguous
// operand ran fully serialised). The asm reads are invisible to hipcc's lgkmcnt bookkeeping, so the caller waits
// for them explicitly (lds_wait_frags) before the MFMAs that consume them.
// The read is at LDS byte address a + OFF (OFF < 65536: the instruction's offset field), so the loop-invariant part of
// an address stays in one VGPR and the stage / k-step / row part is an immediate (no per-iteration VALU address adds)
template <int OFF>
__device__ __forceinline__ s16x4 ds_tr_off(unsigned a) {
  static_assert(OFF >= 0 && OFF < 65536, "ds offset field");
  s16x4 r;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(a), "i"(OFF) : "memory");
  return r;
}

template <int OFF>
__device__ __forceinline__ s16x8 frag_tr_off(unsigned a) {
  const s16x4 lo = ds_tr_off<OFF>(a), hi = ds_tr_off<OFF + 1024>(a);  // k-rows +4: same swizzle (tr_swz ignores bit 2)
  s16x8 r;
  r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
  r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  return r;
}

// lane part of frag_tr's address for column base cbase (% 128) at k-step 0 (k-step ks adds 32 rows = 8192 B: the
// swizzle ignores bit 5 of the row)
__device__ __forceinline__ int frag_tr_lane(int cbase, int lane) {
  const int gq = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  return tr_off(gq * 8 + q, (cbase >> 3) + (p >> 1)) + (p & 1) * 8;
}

// XCD-aware tile order. Workgroups are dispatched round-robin over the 8 XCDs (dispatch id d runs on XCD d % 8,
// each XCD has its own 4 MiB L2). The grid is (N tiles, M tiles, splits); re-number it so every XCD owns a
// CONTIGUOUS band of logical tiles (bijective for any grid size), with N tiles fastest: the N tiles of one
// 128-row A band -- and, for implicit-GEMM convs, the neighbouring bands whose halo rows it re-reads -- are
// then fetched into ONE L2 instead of up to eight.
struct TileId {
  int m0, n0, z, tile;  // tile = logical (m, n) index within the split slice
};

template <int TBN = BN, int TBM = BM>
__device__ __forceinline__ TileId tile_id() {
  const int gx = gridDim.x, per = gridDim.x * gridDim.y;
  const int total = per * gridDim.z;
  const int d = (blockIdx.z * gridDim.y + blockIdx.y) * gx + blockIdx.x;
  const int xcd = d & 7, q = total >> 3, r = total & 7;
  const int l = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (d >> 3);
  TileId t;
  t.z = l / per;
  t.tile = l - t.z * per;
  const int mt = t.tile / gx;
  t.m0 = mt * TBM;
  t.n0 = (t.tile - mt * gx) * TBN;
  return t;
}

// What grid slice z of a launch works on: problem grp of a grouped launch (0 otherwise) with its operands, split z
// within it, and that split's range [kt0, kt1) of KBK-deep k-tiles (split-K slices stay in units of BK)
struct Slice {
  int grp, z, kt0, kt1;
  const bf16_t *A, *B;
};

template <int KBK = BK>
__device__ __forceinline__ Slice slice_of(const Args& g, int tz) {
  Slice s;
  s.grp = g.ngroups > 1 ? tz / g.nsplit : 0;  // grouped launch: problem index, then the split within it
  s.z = tz - s.grp * g.nsplit;
  s.A = s.grp ? g.Ag[s.grp] : g.A;
  s.B = s.grp ? g.Bg[s.grp] : g.B;
  const int nkt_total = (g.K + KBK - 1) / KBK;
  s.kt0 = s.z * g.ktiles_per_split * (BK / KBK);
  s.kt1 = min(nkt_total, s.kt0 + g.ktiles_per_split * (BK / KBK));
  return s;
}

// The kernels take (const Args g, const EpiArgs e): e sits in the kernel-argument segment right after g. Reading it
// through a laundered segment pointer AFTER the main loop keeps the compiler from hoisting ~50 scalar loads of
// epilogue fields to the kernel entry, where they stayed live (and spilled) in SGPRs across the whole main loop.
// grp: the problem of a grouped launch whose outputs the copy addresses.
__device__ __forceinline__ EpiArgs epi_args_late(const Args& g, int grp) {
  EpiArgs r;
#if defined(__HIP_DEVICE_COMPILE__)  // the host compilation pass never runs device code
  typedef __attribute__((address_space(4))) const char* kptr_t;
  kptr_t ka = (kptr_t)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(ka));
  constexpr size_t off = (sizeof(Args) + alignof(EpiArgs) - 1) / alignof(EpiArgs) * alignof(EpiArgs);
  __builtin_memcpy(&r, ka + off, sizeof(EpiArgs));
#endif
  if (grp) group_epi(r, g.Cg[grp], g.sum_g[grp], grp);
  return r;
}

}  // namespace sdmi_gemm_impl
