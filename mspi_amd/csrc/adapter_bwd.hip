// Weight gradient of the adapter's Inception (backbones/s3d.py upstream: eight conv -> BatchNorm3d -> ReLU layers whose widths
// 16, 48, 64, 96, 192, 208, 416 are multiples of 16 but not all of 32).  Entry point (include/mspi_adapter_train_hip.h), fp32:
//   mspi_conv_wgrad_t16   dW [Cout][taps C] and db [Cout] of a stride-1 "same" conv (1,1,1), (1,3,3) or (3,1,1)   one pass + the ordered add
// Sums that cross a workgroup go through the caller's workspace as one record per row slice, which a second launch adds in
// slice order (rt_sum_records, common.h): bitwise repeatable.  Nothing here allocates or synchronises.
#include "common.h"
#include "conv_common.h"
#include "../../include/mspi_adapter_train_hip.h"

namespace mspi {

typedef float v4f_t16 __attribute__((ext_vector_type(4)));

// The three kernel shapes are one problem over a grid of IMAGES j with two coordinates (a, b), a halo ha along a and hb along b:
//   (1,1,1)  one image, a trivial, b = the flat row index                          ha = hb = 0, 1 tap
//   (1,3,3)  image = frame (n, t), a = h, b = w                                     ha = hb = 1, 9 taps (da, db) = (kh, kw)
//   (3,1,1)  image = clip n,       a = t, b = h W + w                               ha = 1, hb = 0, 3 taps da = kt
// and output row (j, a, b) is row (j A + a) Bx + b of dy in all three.  A BOX is BA x BB positions of one image, at most
// T16_RC = 32 rows; its dy rows [32][Cout] and its x rows with the halo [(BA + 2 ha) (BB + 2 hb)][channels] are staged in LDS
// once, positions outside the image as zeros (the conv's zero padding: a tap never reads across an image), and every tap reads
// its operands from there.  Only the rows that exist are listed (a ragged box is shorter), padded to a multiple of four with
// rows whose dy is zero and whose x is a block of zero rows behind the box -- one for every tap offset, written once -- so that
// no padding row can multiply real data or what a previous workgroup left in LDS (0 x Inf, 0 x NaN).
// v_mfma_f32_16x16x4_f32: D[co][ci] += A[co][k] B[k][ci], k = four consecutive rows of the list; lane l feeds
// A = dy[4 i + (l >> 4)][co0 + (l & 15)] and B = x[row of 4 i + (l >> 4) moved by the tap][ci0 + (l & 15)].
// A workgroup owns a slice of the boxes, a group of ncb 16-wide input-channel tiles, every tap and all of Cout: nco x ncb x taps
// accumulator tiles, tile p to wave p % 4, at most T16_TPW = 30 each (13 x 9 = 117 tiles at 96 -> 208 (1,3,3)).  Consecutive
// tiles of a wave are independent accumulators, which covers the MFMA's 40-cycle dependent latency over its 32-cycle issue.
// db comes from the A operands of the tiles of tap 0, channel tile 0 (p < nco), in the workgroups of channel group 0.
constexpr int T16_T = 256;
constexpr int T16_RC = 32;               // rows per box
constexpr int T16_TPW = 30;              // accumulator tiles per wave
constexpr int T16_MAX_CO = 208;
constexpr int T16_MAX_C = 416;
constexpr int T16_XROWS = 104;           // staged x rows of a box with its halo: at most (32 + 2) (1 + 2)
constexpr int T16_XL = 8448;             // floats of the x stage
constexpr int T16_DL = T16_RC * T16_MAX_CO;
constexpr int T16_SLICE_SMALL = 64;      // rows per slice below T16_MID_ROWS rows
constexpr int T16_SLICE_MID = 128;       // from T16_MID_ROWS rows on (2 688 rows, two clips: 21 slices)
constexpr int T16_SLICE_BIG = 256;       // from T16_BIG_ROWS rows on (10 752 rows, eight clips: 42 slices)
constexpr int T16_MID_ROWS = 1024;
constexpr int T16_BIG_ROWS = 8192;

struct T16Geom {
  int kind;                              // 0: (1,1,1), 1: (1,3,3), 2: (3,1,1)
  int C, Cout, nco, taps;
  int T, H, W;
  long sN, sT, sH, sW, ldy;
  long R;                                // output rows
  int A, Bx, ha, hb;                     // image extent and halo
  int BA, BB, XB, nba, nbb;              // box extent, staged line length BB + 2 hb, boxes per image along a and b
  long NB;                               // boxes
  int L, bps, S;                         // rows per slice (nominal: 32 per box), boxes per slice, slices
  int ncb, groups;                       // channel tiles per group, groups
  int ldd, ldx;                          // LDS row strides
};

__host__ __device__ inline long t16_record_floats(int Cout, int K) { return (long)Cout * K + Cout; }
// a row stride of 16 (mod 32) floats puts the four rows of one MFMA step on different banks
__host__ __device__ inline int t16_ld(int c) { return c % 32 ? c : c + 16; }

__global__ __launch_bounds__(T16_T) void conv_wgrad_t16_kernel(T16Geom g, const float* __restrict__ x, const float* __restrict__ dy,
                                                               float* __restrict__ ws) {
  __shared__ float4 dL4[T16_DL / 4];
  __shared__ float4 xL4[T16_XL / 4];
  __shared__ long xoff[T16_XROWS];       // element offset of a staged x row, -1: outside the image
  __shared__ int xbase[T16_RC];          // staged x row of a listed row at tap (0, 0)
  float* dL = reinterpret_cast<float*>(dL4);
  float* xL = reinterpret_cast<float*>(xL4);
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // scalar: the branches around the MFMAs below are uniform
  const int nct = g.C >> 4;
  const int ct0 = blockIdx.y * g.ncb;
  const int ncw = nct - ct0 < g.ncb ? nct - ct0 : g.ncb;          // this workgroup's channel tiles
  const int cw = ncw * 16, c0 = ct0 * 16;
  const int tiles = g.nco * ncw * g.taps;
  const int XA = g.BA + 2 * g.ha;
  const int zrow = XA * g.XB;                                     // the first zero row of the x stage
  const int nz = 1 + 2 * g.ha * g.XB + 2 * g.hb;                  // zero rows: a padding row reads one at every tap offset
  const int tb = 2 * g.hb + 1;                                    // taps along b

  int aoff[T16_TPW], boff[T16_TPW];
  bool tok[T16_TPW];
#pragma unroll
  for (int j = 0; j < T16_TPW; ++j) {
    const int p = wave + 4 * j;                                   // tile p = (tap, channel tile ct, output tile cot), cot fastest
    tok[j] = p < tiles;
    const int q = tok[j] ? p : 0, cot = q % g.nco, q2 = q / g.nco, ct = q2 % ncw, tap = q2 / ncw;
    const int da = tap / tb, db = tap - da * tb;
    aoff[j] = cot * 16;
    boff[j] = (da * g.XB + db) * g.ldx + ct * 16;
  }
  v4f_t16 acc[T16_TPW];
#pragma unroll
  for (int j = 0; j < T16_TPW; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[j][r] = 0.f;
  float bs[4] = {0.f, 0.f, 0.f, 0.f};                             // db of output tiles wave, wave + 4, wave + 8, wave + 12
  bool bok[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) bok[j] = blockIdx.y == 0 && wave + 4 * j < g.nco;

  const int nqx = cw >> 2, nqy = g.Cout >> 2;
  for (int e = tid; e < nz * nqx; e += T16_T) {                   // never written again: the boxes stage rows below zrow only
    const int q = e / nqx, qd = e - q * nqx;
    *reinterpret_cast<float4*>(xL + (zrow + q) * g.ldx + qd * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const long bx0 = (long)blockIdx.x * g.bps;
  const long bx1 = bx0 + g.bps < g.NB ? bx0 + g.bps : g.NB;
  for (long bx = bx0; bx < bx1; ++bx) {
    const int per = g.nba * g.nbb;
    const long j = bx / per;
    const int rem = (int)(bx - j * per), ia = rem / g.nbb, ib = rem - ia * g.nbb;
    const int a0 = ia * g.BA, b0 = ib * g.BB;
    const int va = g.A - a0 < g.BA ? g.A - a0 : g.BA, vb = g.Bx - b0 < g.BB ? g.Bx - b0 : g.BB;
    const int nr = va * vb, nr4 = (nr + 3) & ~3;
    __syncthreads();                                              // the previous box has been read
    if (tid < T16_RC) {
      const int la = tid / vb, lb = tid - la * vb;
      xbase[tid] = tid < nr ? (la * g.XB + lb) : zrow;
    }
    for (int q = tid; q < zrow; q += T16_T) {
      const int xa = q / g.XB, xb = q - xa * g.XB;
      const int ga = a0 + xa - g.ha, gb = b0 + xb - g.hb;
      long off = -1;
      if (ga >= 0 && ga < g.A && gb >= 0 && gb < g.Bx) {
        long n;
        int t, h, w;
        if (g.kind == 0) {
          unsigned m = (unsigned)gb;                              // fewer than 2^31 rows (host-checked)
          w = (int)(m % (unsigned)g.W); m /= (unsigned)g.W;
          h = (int)(m % (unsigned)g.H); m /= (unsigned)g.H;
          t = (int)(m % (unsigned)g.T); n = (long)(m / (unsigned)g.T);
        } else if (g.kind == 1) {
          n = j / g.T; t = (int)(j - n * g.T); h = ga; w = gb;
        } else {
          n = j; t = ga; h = gb / g.W; w = gb - h * g.W;
        }
        off = n * g.sN + t * g.sT + h * g.sH + w * g.sW + c0;
      }
      xoff[q] = off;
    }
    __syncthreads();
    for (int e = tid; e < zrow * nqx; e += T16_T) {
      const int q = e / nqx, qd = e - q * nqx;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      const long off = xoff[q];
      if (off >= 0) v = *reinterpret_cast<const float4*>(x + off + qd * 4);
      *reinterpret_cast<float4*>(xL + q * g.ldx + qd * 4) = v;
    }
    for (int e = tid; e < nr4 * nqy; e += T16_T) {
      const int r = e / nqy, qd = e - r * nqy;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < nr) {
        const int la = r / vb, lb = r - la * vb;
        const long m = (j * g.A + a0 + la) * g.Bx + b0 + lb;
        v = *reinterpret_cast<const float4*>(dy + m * g.ldy + qd * 4);
      }
      *reinterpret_cast<float4*>(dL + r * g.ldd + qd * 4) = v;
    }
    __syncthreads();
    const int steps = nr4 >> 2;
    for (int i = 0; i < steps; ++i) {
      const int r = 4 * i + lk;
      const float* dr = dL + r * g.ldd + li;
      const float* xr = xL + xbase[r] * g.ldx + li;
#pragma unroll
      for (int jt = 0; jt < T16_TPW; ++jt)
        if (tok[jt]) {
          const float a = dr[aoff[jt]];
          acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xr[boff[jt]], acc[jt], 0, 0, 0);
          if (jt < 4 && bok[jt]) bs[jt] += a;
        }
    }
  }

  // accumulator (reg r, lane) -> D[co = 4 lk + r][ci = li] of its tile
  const int K = g.taps * g.C;
  float* rec = ws + (long)blockIdx.x * t16_record_floats(g.Cout, K);
#pragma unroll
  for (int jt = 0; jt < T16_TPW; ++jt)
    if (tok[jt]) {
      const int p = wave + 4 * jt, cot = p % g.nco, q2 = p / g.nco, ct = q2 % ncw, tap = q2 / ncw;
      const int col = tap * g.C + c0 + ct * 16 + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) rec[(long)(cot * 16 + 4 * lk + r) * K + col] = acc[jt][r];
    }
  float* rb = rec + (long)g.Cout * K;
#pragma unroll
  for (int jt = 0; jt < 4; ++jt)
    if (bok[jt]) {
      float s = bs[jt];
      s += __shfl_xor(s, 16, 64);                                 // the four rows of every step
      s += __shfl_xor(s, 32, 64);
      if (lane < 16) rb[(wave + 4 * jt) * 16 + lane] = s;
    }
}

// dW [Cout][K] then db [Cout] (n == nW without db), both in the records' own layout, slice by slice in order; grid ceil(n / 64).
__global__ __launch_bounds__(256) void conv_wgrad_t16_reduce_kernel(const float* __restrict__ ws, int S, long nW, long n, long stride,
                                                                    float* __restrict__ dW, float* __restrict__ db) {
  __shared__ float part[4][64];
  const long e = (long)blockIdx.x * 64 + (threadIdx.x & 63);
  const bool live = e < n;
  const float r = rt_sum_records(ws + (live ? e : 0), stride, S, live, part);
  if (threadIdx.x < 64 && live) {
    if (e < nW) dW[e] = r;
    else db[e - nW] = r;
  }
}

static const char* t16_refusal(const MspiConvDesc* d) {
  if (!d) return "null descriptor";
  if (d->N <= 0 || d->T <= 0 || d->H <= 0 || d->W <= 0 || d->To <= 0 || d->Ho <= 0 || d->Wo <= 0) return "empty extent";
  if (d->strT != 1 || d->strH != 1 || d->strW != 1) return "the stride must be 1";
  const bool k111 = d->kT == 1 && d->kH == 1 && d->kW == 1 && !d->padT && !d->padH && !d->padW;
  const bool k133 = d->kT == 1 && d->kH == 3 && d->kW == 3 && !d->padT && d->padH == 1 && d->padW == 1;
  const bool k311 = d->kT == 3 && d->kH == 1 && d->kW == 1 && d->padT == 1 && !d->padH && !d->padW;
  if (!k111 && !k133 && !k311) return "the kernel must be (1,1,1), (1,3,3) pad (0,1,1) or (3,1,1) pad (1,0,0)";
  if (d->To != d->T || d->Ho != d->H || d->Wo != d->W) return "output extent does not follow from the input extent";
  if (d->C < 16 || d->C % 16) return "stored Cin must be a multiple of 16 (C % 16 == 0)";
  if (d->C > T16_MAX_C) return "stored Cin must be at most 416 (C <= 416)";
  if (d->Cout < 16 || d->Cout % 16) return "stored Cout must be a multiple of 16 (Cout % 16 == 0)";
  if (d->Cout > T16_MAX_CO) return "stored Cout must be at most 208 (Cout <= 208)";
  if (d->sC != 1) return "the input must be channels-last (sC == 1)";
  if (d->sN % 4 || d->sT % 4 || d->sH % 4 || d->sW % 4) return "input strides must be multiples of 4";
  if (d->ldy < d->Cout || d->ldy % 4) return "ldy must be a multiple of 4, >= Cout";
  if ((long)d->N * d->T * d->H * d->W >= (1L << 31)) return "2^31 or more output rows";
  return nullptr;
}

static T16Geom t16_geom(const MspiConvDesc* d) {
  T16Geom g;
  g.kind = d->kH == 3 ? 1 : (d->kT == 3 ? 2 : 0);
  g.C = d->C; g.Cout = d->Cout; g.nco = g.Cout / 16;
  g.T = d->T; g.H = d->H; g.W = d->W;
  g.sN = d->sN; g.sT = d->sT; g.sH = d->sH; g.sW = d->sW; g.ldy = d->ldy;
  g.R = (long)d->N * d->T * d->H * d->W;
  long J;
  if (g.kind == 0) {
    J = 1; g.A = 1; g.Bx = (int)g.R; g.ha = g.hb = 0; g.BA = 1; g.BB = T16_RC;
  } else if (g.kind == 1) {
    J = (long)d->N * d->T; g.A = d->H; g.Bx = d->W; g.ha = g.hb = 1;
    g.BB = d->W < 8 ? d->W : 8;
    g.BA = d->H < T16_RC / g.BB ? d->H : T16_RC / g.BB;
  } else {
    J = d->N; g.A = d->T; g.Bx = d->H * d->W; g.ha = 1; g.hb = 0;   // H W < 2^31: the rows are
    g.BA = d->T < 4 ? d->T : 4;
    g.BB = g.Bx < T16_RC / g.BA ? g.Bx : T16_RC / g.BA;
  }
  g.taps = (2 * g.ha + 1) * (2 * g.hb + 1);
  g.XB = g.BB + 2 * g.hb;
  g.nba = (g.A + g.BA - 1) / g.BA;
  g.nbb = (g.Bx + g.BB - 1) / g.BB;
  g.NB = J * g.nba * g.nbb;
  g.L = g.R < T16_MID_ROWS ? T16_SLICE_SMALL : (g.R < T16_BIG_ROWS ? T16_SLICE_MID : T16_SLICE_BIG);
  g.bps = g.L / T16_RC;
  g.S = (int)((g.NB + g.bps - 1) / g.bps);
  // channel tiles per group: within the waves' accumulator budget and the x stage (the box's rows and the zero rows)
  const int nct = g.C / 16, xrows = (g.BA + 2 * g.ha) * g.XB + 1 + 2 * g.ha * g.XB + 2 * g.hb;
  int ncb = 4 * T16_TPW / (g.nco * g.taps);
  const int cap = g.taps == 1 ? 8 : 4;
  if (ncb > cap) ncb = cap;
  if (ncb > nct) ncb = nct;
  while (ncb > 1 && xrows * t16_ld(ncb * 16) > T16_XL) --ncb;
  g.groups = (nct + ncb - 1) / ncb;
  g.ncb = (nct + g.groups - 1) / g.groups;
  g.ldd = t16_ld(g.Cout);                                        // at most 208: 192 + 16, and 208 itself is 16 (mod 32)
  g.ldx = t16_ld(g.ncb * 16);
  return g;
}

}  // namespace mspi

using namespace mspi;

extern "C" int mspi_conv_wgrad_t16_supported(const MspiConvDesc* d) {
  const char* why = t16_refusal(d);
  if (why) set_error("mspi_conv_wgrad_t16: %s", why);
  return why ? 0 : 1;
}

extern "C" size_t mspi_conv_wgrad_t16_ws_bytes(const MspiConvDesc* d) {
  if (t16_refusal(d)) return 0;
  const T16Geom g = t16_geom(d);
  return (size_t)g.S * t16_record_floats(g.Cout, g.taps * g.C) * sizeof(float);
}

extern "C" int mspi_conv_wgrad_t16_variant(const MspiConvDesc* d, const void* x, const void* dy) {
  const char* why = t16_refusal(d);
  if (!why && !(x && dy && aligned16(x) && aligned16(dy))) why = "x and dy must be 16-byte aligned";
  if (why) {
    set_error("mspi_conv_wgrad_t16: %s", why);
    return -1;
  }
  return t16_geom(d).L;
}

extern "C" int mspi_conv_wgrad_t16(const MspiConvDesc* d, const float* x, const float* dy, float* dW, float* db, void* ws,
                                   mspi_stream_t stream) {
  MSPI_REQUIRE(x && dy && dW && ws, "mspi_conv_wgrad_t16: null argument");
  if (mspi_conv_wgrad_t16_variant(d, x, dy) < 0) return MSPI_EINVAL;
  MSPI_REQUIRE(aligned16(ws) && aligned16(dW), "mspi_conv_wgrad_t16: dW and ws must be 16-byte aligned");
  const T16Geom g = t16_geom(d);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(conv_wgrad_t16_kernel, dim3(g.S, g.groups), dim3(T16_T), 0, st, g, x, dy, (float*)ws);
  const long nW = (long)g.Cout * g.taps * g.C, n = nW + (db ? g.Cout : 0);
  hipLaunchKernelGGL(conv_wgrad_t16_reduce_kernel, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, st, (const float*)ws, g.S, nW, n,
                     t16_record_floats(g.Cout, g.taps * g.C), dW, db);
  return check_launch("mspi_conv_wgrad_t16");
}
