// Shared by the two implicit-GEMM kernels (conv_gemm.hip: everything through LDS, any layout / precision;
// conv_gemm_ad.hip: the f16x3 fast path with activations loaded straight into MFMA fragments).
#pragma once
#include "common.h"

namespace mspi {

typedef float v16f __attribute__((ext_vector_type(16)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef _Float16 v4h __attribute__((ext_vector_type(4)));

// Precision modes.
//  PREC_F32   : v_mfma_f32_32x32x2_f32 on fp32 operands (exact fp32 fmaf chain).
//  PREC_F16X3 : fp32-accurate product on the 16x faster f16 matrix pipe.  Every operand is split
//               x = hi + lo with hi = f16(x), lo = f16(x - hi) (22 significand bits together) and
//               the product is accumulated in fp32 as hi*hi + hi*lo + lo*hi by three
//               v_mfma_f32_32x32x16_f16 (the dropped lo*lo term is 2^-22 relative; f16xf16
//               products are exact in fp32).  Weights are split once at pack time (pre-scaled by a
//               power of two so their lo part stays a normal f16); activations are split while they
//               are staged into LDS.
enum { PREC_F32 = 0, PREC_F16X3 = 1 };

struct ConvArgs {
  const float* x;
  const float* w;
  const float* bias;
  const float* res;
  const float* gate;
  float* y;
  int N, T, H, W, C;
  long sN, sT, sH, sW, sC;
  int kT, kH, kW, strT, strH, strW, padT, padH, padW;
  int To, Ho, Wo, Cout;
  long ldy, ldw, ldr;
  int act;
  int M, K;
  int rows_per_sample;
  int tiles_n, nblocks;
  float out_scale;  // F16X3: 1 / (power-of-two weight pre-scale), applied to the accumulator
  int* status;      // range guard (common.h): set to 1 when an output is not finite; may be NULL
  int dbg;          // ablation switches for tools/gemm_probe.py (MSPI_CONV_DBG); 0 in production
  int ksplit;       // split-K: gridDim.y workgroups share an output tile, each owns a contiguous range of K steps ...
  float* ws;        // ... and writes its partial sums to ws[z][M][Cout] (no bias / residual / activation); NULL: no split
  // pre-split activations (conv_gemm_dma_kernel<..., APRE>): A is two BLOCKED f16 planes (common.h plane_off; ldxs == K) (hi, then lo `xplane` elements
  // later), written by a producer's epilogue; the kernel then DMAs them like the weight planes and splits nothing
  int dense_rows;       // 1: 1x1x1 / stride 1 / no padding on an input whose (n,t,h,w) positions are equally spaced rows (offset = m * sW):
                        // the loaders skip the per-row integer divisions of the general gather
  const _Float16* wb;   // blocked f16 hi/lo weight planes (common.h plane_off; rows padded to 16), or NULL: the LDS-DMA kernels' weight source
  const _Float16* xs;
  long ldxs, xplane;
  // split-plane OUTPUT (any kernel's epilogue): when ys != NULL the result goes to two f16 planes instead of y
  _Float16* ys;
  long ldys, yplane;
};

constexpr int BK = 32;

// The tile codes of MspiConvDesc.tile (include/mspi_hip.h): the one place a tile is declared.  kind is the leading digit of
// the variant code (mspi_conv_variant; the pre-split entry point reports kind + 2); bm x bn is the output tile, wm x wn the
// wave grid (the LDS-DMA kernels give every wave a 32-row slab of all bn columns: wm = waves, wn = 1).  BN_ALL: one column
// tile holding every output channel (rounded up to 32, <= 256).  sp_bn: the column tile mspi_gemm_sp_fwd runs under this code,
// 0 = not offered there (code 11 is 128 x 32 on fp32 activations and 128 x 256 on pre-split planes).  slots / eff feed the
// register tiles' cost model in conv_select: resident workgroups and relative time per unit of work.
// Adding or removing a tile: its row here and its case in launch_conv_reg (conv_gemm.hip) or launch_conv_dma
// (conv_gemm_ad.hip), which turn the row's numbers into template arguments.
enum { TILE_REG4 = 1, TILE_REG8 = 2, TILE_DMA128 = 4, TILE_DMA256 = 5 };
constexpr int BN_ALL = 1;
enum { FORM_SP = 3 };   // launch_conv_dma's form for pre-split activation planes, after the forms 0..2 of mspi_conv_variant
struct Tile { int kind, bm, bn, wm, wn, sp_bn, slots; float eff; };
static const Tile kTiles[] = {
    {TILE_REG4, 128, 128, 2, 2, 0, 512, 1.00f},     //  0
    {TILE_REG4, 128, 64, 2, 2, 0, 512, 1.06f},      //  1
    {TILE_REG4, 128, 32, 4, 1, 0, 768, 1.30f},      //  2
    {TILE_REG4, 64, 64, 2, 2, 0, 1024, 1.25f},      //  3  (also the split-K tile)
    {TILE_REG8, 128, 128, 4, 2, 0, 512, 1.00f},     //  4  32 x 64 per wave
    {TILE_REG8, 256, 128, 4, 2, 0, 256, 1.10f},     //  5  64 x 64 per wave
    {TILE_DMA128, 128, 128, 4, 1, 128, 0, 0.f},     //  6
    {TILE_DMA128, 128, 64, 4, 1, 64, 0, 0.f},       //  7
    {TILE_DMA128, 128, BN_ALL, 4, 1, 0, 0, 0.f},    //  8  the only way to the 160- and 224-column kernels
    {TILE_DMA128, 128, 96, 4, 1, 96, 0, 0.f},       //  9
    {TILE_DMA128, 128, 192, 4, 1, 192, 0, 0.f},     // 10
    {TILE_DMA128, 128, 32, 4, 1, 256, 0, 0.f},      // 11
    {TILE_DMA256, 256, 256, 8, 1, 256, 0, 0.f},     // 12
    {TILE_DMA256, 256, 192, 8, 1, 192, 0, 0.f},     // 13
    {TILE_DMA256, 256, 128, 8, 1, 128, 0, 0.f},     // 14
};
constexpr int kNumTiles = sizeof(kTiles) / sizeof(kTiles[0]);
inline bool tile_is_dma(const Tile& t) { return t.kind >= TILE_DMA128; }
inline int variant_code(int kind, int bm, int bn, int form) { return kind * 10000000 + bm * 10000 + bn * 10 + form; }

// XCD-aware, bijective block remap: blocks dealt to one XCD (bid % 8) get consecutive logical ids, so the
// N-tiles that re-read one A row panel (and the M-tiles that re-read one weight panel) share that XCD's L2.
__device__ __forceinline__ int xcd_logical_block(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

}  // namespace mspi
