// The pieces the weight-gradient kernels share, one copy each: the stage geometries (the ONE statement of a body's LDS layout, read
// by the body and by its launch), the staging task and row table, the window builder, the tile cursor, the DMA ring's helpers and the
// two epilogues.  Device code: included by
// conv_wgrad_bf16.hip and, for wg_atomic_tiles, by conv_wgrad_tiled.hip.
#pragma once
#include "blk_cell.h"
#include "limb_split.h"

// ---- stage geometries ----
constexpr int WG_CU_LDS = 160 * 1024;                 // LDS of a CU
constexpr int WG3_RED_BYTES = 4 * 8 * 288 * 4;        // WG3_REDUCE_TILES: 8 rows x 288 n per row group of waves

// wgrad3_bf16_body: BM dy rows x 64 pixels (TW x TH) + the 32-channel patch with halo, NPL limb planes, NBUF stages
template <int BM, int TW, int LIMBS>
struct W3Stage {
  static constexpr int TP = 64, TH = TP / TW, GPR = TW / 8, NG = TP / 8, KSTEPS = NG / 2;
  static constexpr int NPL = LIMBS ? 3 : 1, NBUF = LIMBS ? 1 : 2;         // limb planes of a stage; stages
  static constexpr int PH = TH + 2, XG = GPR + 2, PWP = XG * 8;           // patch: PH rows of XG 8-pixel groups (tile columns start at 8)
  static constexpr int ARS = (TP + 8) * 2;                                // bytes per dy row (16 B padding)
  static constexpr int CHSB = (PH * PWP * 2 + 31) / 32 * 32 + 16;         // bytes per patch channel: an odd number of 16-byte slots
  static constexpr int A_BYTES = BM * ARS, X_BYTES = 32 * CHSB, ST_BYTES = A_BYTES + X_BYTES;
  static constexpr int NTA = BM * NG / 256;                               // dy tasks per thread
  static constexpr int XT = 32 * PH * XG, NTX = (XT + 255) / 256;         // patch tasks (per thread)
  static constexpr int LDS_BYTES = NBUF * NPL * ST_BYTES > WG3_RED_BYTES ? NBUF * NPL * ST_BYTES : WG3_RED_BYTES;
  static constexpr int DYN_BYTES = LIMBS ? LDS_BYTES : 0;                 // the limb stages are larger than the 64 KB a kernel may declare
  static_assert((BM * NG) % 256 == 0 && LDS_BYTES <= WG_CU_LDS, "config; LDS of a CU");
};
// wgrad1_bf16_body: BM + BN rows x 64 pixels
template <int BM, int BN, int LIMBS>
struct W1Stage {
  static constexpr int TP = 64, NG = TP / 8, KSTEPS = NG / 2;
  static constexpr int NPL = LIMBS ? 3 : 1, NBUF = LIMBS ? 1 : 2, ARS = (TP + 8) * 2;
  static constexpr int A_BYTES = BM * ARS, B_BYTES = BN * ARS, ST_BYTES = A_BYTES + B_BYTES;
  static constexpr int NTA = BM * NG / 256, NTB = BN * NG / 256;
  static constexpr int LDS_BYTES = NBUF * NPL * ST_BYTES;
  static constexpr int DYN_BYTES = LIMBS ? LDS_BYTES : 0;
  static_assert((BM * NG) % 256 == 0 && (BN * NG) % 256 == 0 && LDS_BYTES <= WG_CU_LDS, "config; LDS of a CU");
};
// the DMA rings: NR stages of C_DMA 1 KB instructions per wave (short waves issue all-OOB fillers: one vmcnt rule)
template <int N_DMA, int NR>
struct WgRing {
  static constexpr int C_DMA = (N_DMA + 3) / 4;
  static constexpr int ST_BYTES = 4 * C_DMA * 1024;
  static_assert(NR >= 2 && NR <= 5 && (NR - 2) * C_DMA < 64 && NR * ST_BYTES <= WG_CU_LDS, "vmcnt is 6 bits; LDS of a CU");
};
// wgrad3_tr_body: the dy tile slab-major (16 pixels per instruction), then the input patch row-major with halo (PW pixels per row)
template <int BM, int TW, int TH, int NR>
struct W3Ring : WgRing<BM / 32 * (TW * TH / 16) + ((TH + 2) * (TW + 2) + 15) / 16, NR> {
  static constexpr int TP = TW * TH, NK = TP / 16;
  static constexpr int PW = TW + 2, PH = TH + 2, XPX = PH * PW;
  static constexpr int NA = BM / 32 * NK, NX = (XPX + 15) / 16;
  static constexpr int X_OFF = NA * 1024;
  static constexpr int LDS_BYTES = NR * W3Ring::ST_BYTES > WG3_RED_BYTES ? NR * W3Ring::ST_BYTES : WG3_RED_BYTES, DYN_BYTES = LDS_BYTES;
  static_assert(TW % 8 == 0 && 4 * W3Ring::C_DMA >= NA + NX && 4 * (W3Ring::C_DMA - 1) < NA + NX, "config; the base's count is NA + NX");
};
// wgrad1_tr_body: TP pixels of the BM / 32 + BN / 32 channel slabs of the two operands
template <int BM, int BN, int TP, int NR>
struct W1Ring : WgRing<(BM / 32 + BN / 32) * (TP / 16), NR> {
  static constexpr int NK = TP / 16, SA = BM / 32, SB = BN / 32, ND = (SA + SB) * NK;
  static constexpr int B_OFF = SA * NK * 1024;
  static constexpr int LDS_BYTES = NR * W1Ring::ST_BYTES, DYN_BYTES = LDS_BYTES;
  static_assert(NR <= 4 && 4 * W1Ring::C_DMA >= ND && 4 * (W1Ring::C_DMA - 1) < ND, "config; the base's count is ND");
};

// The stage of a body: static LDS, or the dynamic LDS of the launch (Geo::DYN_BYTES of wgb_launch).
template <int BYTES, bool DYN>
__device__ __forceinline__ char* wgb_stage_lds() {
  if constexpr (DYN) {
    extern __shared__ __attribute__((aligned(1024))) char wgb_dyn_lds[];
    return wgb_dyn_lds;
  } else {
    __shared__ __attribute__((aligned(16))) char wgb_static_lds[BYTES];
    return wgb_static_lds;
  }
}

// ---- staging of the register-staged bodies ----
// One staging task = 8 consecutive pixels of one row of one channel -> one 16-byte bf16 cell.
// V4: two dwordx4 loads (W % 4 == 0: each is entirely inside or outside the row); otherwise 8 dword loads + a validity mask.
template <bool V4>
struct Task8 {
  float v[8];
  __device__ __forceinline__ void load(const __amdgpu_buffer_rsrc_t r, int off_elems, bool ok_row, int gx, int W) {
    if constexpr (V4) {
      const unsigned o0 = (ok_row && gx >= 0 && gx + 3 < W) ? (unsigned)off_elems * 4u : RSIS_OOB;
      const unsigned o1 = (ok_row && gx + 4 >= 0 && gx + 7 < W) ? (unsigned)(off_elems + 4) * 4u : RSIS_OOB;
      const f32x4 a = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, o0, 0, 0));
      const f32x4 b = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, o1, 0, 0));
      v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const bool ok = ok_row && (unsigned)(gx + i) < (unsigned)W;
        v[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, ok ? (unsigned)(off_elems + i) * 4u : RSIS_OOB, 0, 0));
      }
    }
  }
  __device__ __forceinline__ u32x4 cell() const {
    u32x4 c;
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = blk_pack2(v[2 * k], v[2 * k + 1]);
    return c;
  }
  // LIMBS: the three exact bf16 limbs of the 8 values (limb_split.h) as three cells, one per limb plane of the stage.  (The stores of
  // the cells stay in the bodies' W3_STORE / W1_STORE: one store function, in three forms, changed the limb kernels' register counts.)
  // (rsis_limb_pack8_cells and wg_limb_pack8 of conv_wgrad_tiled.hip -- a permute in registers, for fragments that never see LDS --
  //  stay two functions on purpose.)
  __device__ __forceinline__ void limb_cells(u32x4 (&c)[3]) const {
    unsigned q[3][4];
    rsis_limb_pack8_cells(v, q[0], q[1], q[2]);
#pragma unroll
    for (int l = 0; l < 3; ++l) c[l] = u32x4{q[l][0], q[l][1], q[l][2], q[l][3]};
  }
};

// The loop-invariant part of the NT row tasks of thread t: rows of NG 8-pixel groups (GPR per tile row), task e = t + 256 i is group
// e % NG of row e / NG.  off: element offset inside the image slab of the tile's first pixel, -1 beyond the last channel; y, x: the
// tile-local pixel; lds: byte inside the operand's part of the stage.
template <int NT, int NG, int GPR, int ARS>
__device__ __forceinline__ void wg_row_tasks(const int t, const int c0, const int C, const int HW, const int W, int (&off)[NT],
                                             int (&y)[NT], int (&x)[NT], int (&lds)[NT]) {
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int e = t + i * 256;
    const int row = e / NG, G = e % NG;
    y[i] = G / GPR; x[i] = (G % GPR) * 8;
    off[i] = c0 + row < C ? row * HW + y[i] * W + x[i] : -1;
    lds[i] = row * ARS + G * 16;
  }
}

// The tile cursor of a split: spatial tile t of the job = (image tb, tile row ty, tile column tx), walked in that order.
// (The 1x1 DMA body runs it with tiles_y = 1, the flattened map.)
struct WgCursor {
  int tb, ty, tx;
  __device__ __forceinline__ WgCursor(const int t, const int tiles_x, const int tiles_y) {
    tb = t / (tiles_x * tiles_y);
    const int trem = t - tb * (tiles_x * tiles_y);
    ty = trem / tiles_x;
    tx = trem - ty * tiles_x;
  }
  __device__ __forceinline__ void next(const int tiles_x, const int tiles_y) {
    if (++tx == tiles_x) { tx = 0; if (++ty == tiles_y) { ty = 0; ++tb; } }
  }
};

// The three shifted windows of a patch row for the taps s = 0 / 1 / 2: the aligned 16-byte window at `row` plus one dword on either
// side, 4 v_alignbit_b32 each for s = 0 and s = 2.
__device__ __forceinline__ void wg3_windows(const char* row, bf16x8 (&w)[3]) {
  const unsigned d0 = *(const unsigned*)(row - 4);
  const u32x4 m = *(const u32x4*)row;
  const unsigned d5 = *(const unsigned*)(row + 16);
  const u32x4 w0 = {__builtin_amdgcn_alignbit(m[0], d0, 16), __builtin_amdgcn_alignbit(m[1], m[0], 16),
                    __builtin_amdgcn_alignbit(m[2], m[1], 16), __builtin_amdgcn_alignbit(m[3], m[2], 16)};
  const u32x4 w2 = {__builtin_amdgcn_alignbit(m[1], m[0], 16), __builtin_amdgcn_alignbit(m[2], m[1], 16),
                    __builtin_amdgcn_alignbit(m[3], m[2], 16), __builtin_amdgcn_alignbit(d5, m[3], 16)};
  w[0] = __builtin_bit_cast(bf16x8, w0); w[1] = __builtin_bit_cast(bf16x8, m); w[2] = __builtin_bit_cast(bf16x8, w2);
}

// ---- the DMA ring of the blk bodies ----
// one DMA instruction of a stage: 1 KB of blk cells (16 B per lane, at byte `off` of the dy or the x image) to sd + at
__device__ __forceinline__ void wg_dma(const bool from_a, const __amdgpu_buffer_rsrc_t ra, const __amdgpu_buffer_rsrc_t rx, char* sd,
                                       const int at, const unsigned off) {
  if (from_a) __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_vp_t)(sd + at), 16, off, 0, 0, 0);
  else __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_vp_t)(sd + at), 16, off, 0, 0, 0);
}
// tile t of ntl has landed once at most `ahead` younger tiles of this wave's DMA (C_DMA instructions each) are still in flight
template <int NR, int C_DMA>
__device__ __forceinline__ void wg_ring_wait(const int t, const int ntl) {
  const int ahead = min(NR - 2, ntl - 1 - t);
  if (NR >= 5 && ahead == 3) { RSIS_VMCNT(3 * C_DMA); }
  else if (NR >= 4 && ahead == 2) { RSIS_VMCNT(2 * C_DMA); }
  else if (NR >= 3 && ahead == 1) { RSIS_VMCNT(C_DMA); }
  else { RSIS_VMCNT(0); }
}

// ---- epilogues ----
// TM x TN accumulator tiles (32 x 32) of a wave -> dW with fp32 buffer atomics: a row of the tile is a per-lane base + a scalar
// multiple of ldo; the gate-interleaved rows 4 j + g of the ConvLSTM weights (ihid > 0) go to row g * ihid + j; rows >= Cout get an
// out-of-range offset and are dropped, columns >= n_valid are skipped.  row0_of_wave / n0_of_wave: the lane's first row (the wave's
// first row + 4 * (lane / 32): a multiple of 4) and column (the wave's first column + lane % 32) in tile (0, 0).
template <int TM, int TN>
__device__ __forceinline__ void wg_atomic_tiles(const f32x16 (&acc)[TM][TN], float* dw, const int Cout, const int ldo, const int n_off,
                                                const int ihid, const int row0_of_wave, const int n0_of_wave, const int n_valid) {
  const __amdgpu_buffer_rsrc_t rdw = __builtin_amdgcn_make_buffer_rsrc((void*)dw, 0, (unsigned)((size_t)Cout * ldo * 4), 0x00020000);
  const unsigned ldb = (unsigned)ldo * 4u;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n0_of_wave + j * 32;
    if (n >= n_valid) continue;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int row0 = row0_of_wave + i * 32;
      const int rows_left = Cout - row0;
      const unsigned vo = (unsigned)((ihid > 0 ? row0 >> 2 : row0) * ldo + n_off + n) * 4u;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = (r & 3) + 8 * (r >> 2);
        const unsigned ro = (unsigned)(ihid > 0 ? (r & 3) * ihid + 2 * (r >> 2) : k) * ldb;
        __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(acc[i][j][r], rdw, k < rows_left ? vo + ro : RSIS_OOB, 0, 0);
      }
    }
  }
}

// The nine 32 x 32 tap tiles of a 3x3 wave (acc[9]) -> dW[co][ci][r][s]: the KSPW wave copies (wk) of a row group (wm) first sum their
// partial tiles in LDS (fewer same-address atomics: they are serialised by the L2), 8 rows x 288 columns at a time; the rows are then
// split over the copies and added to dW with the lanes running along n (consecutive addresses).  All waves of the block run it, after
// a barrier behind their last read of the stage: `lds` is reused (WG3_RED_BYTES).
// A MACRO over the body's own names (p, lds, acc, lane, l31, hi, wm, wk, co0, ci0, Cs, Cout, KSPW): the same text as a __forceinline__
// function that takes the job by reference and reads its fields inside the row loop gave wgrad3_tr_group_kernel<64, 32, 4, 2> and
// <64, 8, 8, 3> 227 / 213 VGPRs for 229 / 215 (NOTES (86)).
#define WG3_REDUCE_TILES()                                                                                         \
  {                                                                                                                \
    float* red = (float*)lds + wm * (8 * 288);                                                                     \
    const int nvalid = min(32, Cs - ci0) * 9;                        /* valid columns of this block's 288 */       \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                                \
      _Pragma("unroll") for (int k = 0; k < KSPW; ++k) {                                                           \
        if (wk == k) {                                                                                             \
          _Pragma("unroll") for (int t = 0; t < 9; ++t)                                                            \
            _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                        \
              float* d = red + (r + 4 * hi) * 288 + l31 * 9 + t;                                                   \
              if (k == 0) *d = acc[t][4 * q + r];                                                                  \
              else *d += acc[t][4 * q + r];                                                                        \
            }                                                                                                      \
        }                                                                                                          \
        __syncthreads();                                                                                           \
      }                                                                                                            \
      _Pragma("unroll") for (int rr = wk; rr < 8; rr += KSPW) {                                                    \
        const int co = co0 + wm * 32 + 8 * q + rr;                                                                 \
        if (co >= Cout) continue;                                                                                  \
        const int orow = p.interleave_hid > 0 ? (co & 3) * p.interleave_hid + (co >> 2) : co;                      \
        float* dst = p.dw + (size_t)orow * p.ldo + p.n_off + ci0 * 9;                                              \
        _Pragma("unroll") for (int c = 0; c < 5; ++c) {                                                            \
          const int n = c * 64 + lane;                                                                             \
          if (n < nvalid) atomicAdd(dst + n, red[rr * 288 + n]);                                                   \
        }                                                                                                          \
      }                                                                                                            \
      __syncthreads();                                                                                             \
    }                                                                                                              \
  }
