// Weight gradient of the laterals' entry convs (model/model_utils.py:440-470): the 1x1x1 conv C_k -> 192 and, composed with it,
// the (s,1,1) / stride (s,1,1) conv 192 -> 192 behind it.  Entry point (include/mspi_entry_train_hip.h), fp32:
//   mspi_conv_wgrad_entry   dW [Cout][s C] and db [Cout] for kernel == stride along T, 1x1 in space      one pass + the ordered add
// Sums that cross a workgroup go through the caller's workspace as one record per workgroup, which a second launch adds in a
// fixed order (rt_sum_records, common.h): bitwise repeatable.  Nothing here allocates or synchronises.
#include "common.h"
#include "conv_common.h"
#include "../../include/mspi_entry_train_hip.h"

namespace mspi {

// With kernel == stride and no padding every input frame below To s belongs to exactly one (output row, tap): the s C values
// (tap, ci) of output row r = (n, to, h, w) are s runs of C floats, sT apart -- one LINE of K = s C columns, and
//   dW [Cout][K] = dy^T [Cout][R] . lines [R][K],   db = the column sums of dy
// is one GEMM with the rows as the contraction.  v_mfma_f32_32x32x2_f32: D[co][col] += A[co][k] B[k][col], k = two consecutive
// rows, lane l feeding A = dy[2 i + (l >> 5)][co0 + (l & 31)] and B = line[2 i + (l >> 5)][col0 + (l & 31)].
// A workgroup owns a slice of the rows, EW_CW = 128 columns (four tiles of 32; the last may be ragged, and a tile may straddle
// two taps: a column finds its tap by division, once per thread) and all of Cout (nco = Cout / 32 tiles).  Its nco x nct
// accumulator tiles go round-robin to the four waves, tile p to wave p % 4, at most EW_TPW = 6 each: 18 tiles (K = 96, the
// narrow end) load the waves 5 5 4 4, 24 tiles 6 6 6 6.  Rows are staged EW_RC = 32 at a time: dL [32][Cout] and xL [32][128],
// each global float read once per workgroup; a bank is a column, so the one-float-per-lane operand reads are conflict free.
// db comes from the A operands of the tiles of column tile 0, in the workgroups of column group 0.
constexpr int EW_T = 256;
constexpr int EW_RC = 32;               // rows per staged chunk
constexpr int EW_CW = 128;              // columns per workgroup
constexpr int EW_TPW = 6;               // accumulator tiles per wave: 6 x 4 tiles / 4 waves
constexpr int EW_MAX_CO = 192;
constexpr int EW_MAX_C = 2560;
constexpr int EW_SLICE_SMALL = 64;      // rows per slice below EW_MID_ROWS rows
constexpr int EW_SLICE_MID = 256;       // from EW_MID_ROWS rows on
constexpr int EW_SLICE_BIG = 512;       // from EW_BIG_ROWS rows on
constexpr int EW_MID_ROWS = 1024;
constexpr int EW_BIG_ROWS = 32768;

struct EntryGeom {
  int s, C, K, Cout, nco;               // K = s C
  int To, H, W;                         // output positions per sample: To x H x W
  long sN, sT, sH, sW, ldy;
  long R;                               // output rows
  int L, S, groups;                     // rows per slice, slices, column groups
};

__host__ __device__ inline long ew_record_floats(int Cout, int K) { return (long)Cout * K + Cout; }

__global__ __launch_bounds__(EW_T) void conv_wgrad_entry_kernel(EntryGeom g, const float* __restrict__ x, const float* __restrict__ dy,
                                                                float* __restrict__ ws) {
  __shared__ float4 dL4[EW_RC * EW_MAX_CO / 4];
  __shared__ float4 xL4[EW_RC * EW_CW / 4];
  __shared__ long rowbase[EW_RC];
  float* dL = reinterpret_cast<float*>(dL4);
  float* xL = reinterpret_cast<float*>(xL4);
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // scalar: the branches around the MFMAs below are uniform
  const int col0 = blockIdx.y * EW_CW;
  const int Kp = (g.K + 31) & ~31;
  const int ncw = Kp - col0 < EW_CW ? Kp - col0 : EW_CW;          // this workgroup's columns, a multiple of 32
  const int tiles = g.nco * (ncw >> 5);

  int aoff[EW_TPW], boff[EW_TPW];
  bool tok[EW_TPW];
#pragma unroll
  for (int j = 0; j < EW_TPW; ++j) {
    const int p = wave + 4 * j;                                   // tile p = (column tile ct, channel tile cot), cot fastest
    tok[j] = p < tiles;
    const int q = tok[j] ? p : 0, ct = q / g.nco, cot = q - ct * g.nco;
    aoff[j] = cot * 32 + li;
    boff[j] = ct * 32 + li;
  }
  v16f acc[EW_TPW];
#pragma unroll
  for (int j = 0; j < EW_TPW; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  float bs0 = 0.f, bs1 = 0.f;                                     // db of channel tiles wave and wave + 4 (column tile 0: p < nco)
  const bool b0 = wave < g.nco, b1 = wave + 4 < g.nco;

  // staging roles.  x: thread (xr, xq) loads column quad xq of rows xr, xr + 8, ...; dy: thread (yr, yq) quad yq of rows yr, yr + 4, ...
  const int xq = tid & 31, xr = tid >> 5;
  const int xcol = col0 + xq * 4;
  const bool xlive = xq * 4 < ncw, xin = xcol < g.K;              // a quad never straddles K or a tap: C % 4 == 0
  const int xtap = xin ? xcol / g.C : 0;
  const long xoff = (long)xtap * g.sT + (xcol - xtap * g.C);
  const int yq = tid & 63, yr = tid >> 6;
  const bool ylive = yq * 4 < g.Cout;

  const long m0s = (long)blockIdx.x * g.L;
  const long m1s = m0s + g.L < g.R ? m0s + g.L : g.R;
  for (long m0 = m0s; m0 < m1s; m0 += EW_RC) {
    const int nr = m1s - m0 < EW_RC ? (int)(m1s - m0) : EW_RC;
    __syncthreads();                                              // the previous chunk has been read
    if (tid < nr) {
      unsigned q = (unsigned)(m0 + tid);                          // fewer than 2^31 rows (host-checked)
      const int w = (int)(q % (unsigned)g.W); q /= (unsigned)g.W;
      const int h = (int)(q % (unsigned)g.H); q /= (unsigned)g.H;
      const int to = (int)(q % (unsigned)g.To);
      const long n = (long)(q / (unsigned)g.To);
      rowbase[tid] = n * g.sN + (long)to * g.s * g.sT + h * g.sH + w * g.sW;
    }
    __syncthreads();
    if (xlive)
      for (int r = xr; r < EW_RC; r += EW_T / 32) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (xin && r < nr) v = *reinterpret_cast<const float4*>(x + rowbase[r] + xoff);
        *reinterpret_cast<float4*>(xL + r * EW_CW + xq * 4) = v;
      }
    if (ylive)
      for (int r = yr; r < EW_RC; r += EW_T / 64) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < nr) v = *reinterpret_cast<const float4*>(dy + (m0 + r) * g.ldy + yq * 4);
        *reinterpret_cast<float4*>(dL + r * g.Cout + yq * 4) = v;
      }
    __syncthreads();
    const int steps = (nr + 1) >> 1;                              // an odd last row pairs with a zero row
    for (int i = 0; i < steps; ++i) {
      const int r = 2 * i + lh;
      const float* dr = dL + r * g.Cout;
      const float* xr_ = xL + r * EW_CW;
#pragma unroll
      for (int j = 0; j < EW_TPW; ++j)
        if (tok[j]) {
          const float a = dr[aoff[j]];
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xr_[boff[j]], acc[j], 0, 0, 0);
          if (j == 0 && b0) bs0 += a;
          if (j == 1 && b1) bs1 += a;
        }
    }
  }

  // accumulator (reg r, lane) -> D[co = (r & 3) + 8 (r >> 2) + 4 lh][col = li] of its tile
  float* rec = ws + (long)blockIdx.x * ew_record_floats(g.Cout, g.K);
#pragma unroll
  for (int j = 0; j < EW_TPW; ++j)
    if (tok[j]) {
      const int p = wave + 4 * j, ct = p / g.nco, cot = p - ct * g.nco;
      const int col = col0 + ct * 32 + li;
      if (col < g.K) {
#pragma unroll
        for (int r = 0; r < 16; ++r) rec[(long)(cot * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * g.K + col] = acc[j][r];
      }
    }
  if (blockIdx.y == 0) {
    float* rb = rec + (long)g.Cout * g.K;
    if (b0) {
      bs0 += __shfl_xor(bs0, 32, 64);                             // the two rows of every pair
      if (lane < 32) rb[wave * 32 + lane] = bs0;
    }
    if (b1) {
      bs1 += __shfl_xor(bs1, 32, 64);
      if (lane < 32) rb[(wave + 4) * 32 + lane] = bs1;
    }
  }
}

// dW [Cout][K] then db [Cout], both in the records' own layout, slice by slice in order; grid ceil(n / 64).
__global__ __launch_bounds__(256) void conv_wgrad_entry_reduce_kernel(const float* __restrict__ ws, int S, long nW, long n,
                                                                      float* __restrict__ dW, float* __restrict__ db) {
  __shared__ float part[4][64];
  const long e = (long)blockIdx.x * 64 + (threadIdx.x & 63);
  const bool live = e < n;
  const float r = rt_sum_records(ws + (live ? e : 0), n, S, live, part);
  if (threadIdx.x < 64 && live) {
    if (e < nW) dW[e] = r;
    else db[e - nW] = r;
  }
}

static const char* entry_refusal(const MspiConvDesc* d) {
  if (!d) return "null descriptor";
  if (d->N <= 0 || d->T <= 0 || d->H <= 0 || d->W <= 0 || d->To <= 0 || d->Ho <= 0 || d->Wo <= 0) return "empty extent";
  if (d->kH != 1 || d->kW != 1) return "the kernel must be 1x1 in space (no spatial taps)";
  if (d->kT != 1 && d->kT != 2 && d->kT != 4) return "the kernel along T must be 1, 2 or 4";
  if (d->strT != d->kT || d->strH != 1 || d->strW != 1) return "the stride must equal the kernel: (s,1,1) / stride (s,1,1)";
  if (d->padT || d->padH || d->padW) return "padding must be 0";
  if (d->To != d->T / d->kT || d->Ho != d->H || d->Wo != d->W) return "output extent does not follow from the input extent";
  if (d->Cout < 32 || d->Cout > EW_MAX_CO || d->Cout % 32) return "stored Cout must be a multiple of 32, at most 192";
  if (d->C < 4 || d->C > EW_MAX_C || d->C % 4) return "stored Cin must be a multiple of 4 (C % 4 == 0), at most 2560";
  if (d->sC != 1) return "the input must be channels-last (sC == 1)";
  if (d->sN % 4 || d->sT % 4 || d->sH % 4 || d->sW % 4) return "input strides must be multiples of 4";
  if (d->ldy < d->Cout || d->ldy % 4) return "ldy must be a multiple of 4, >= Cout";
  if ((long)d->N * d->To * d->Ho * d->Wo >= (1L << 31)) return "2^31 or more output rows";
  return nullptr;
}

static EntryGeom entry_geom(const MspiConvDesc* d) {
  EntryGeom g;
  g.s = d->kT; g.C = d->C; g.K = g.s * g.C; g.Cout = d->Cout; g.nco = g.Cout / 32;
  g.To = d->To; g.H = d->H; g.W = d->W;
  g.sN = d->sN; g.sT = d->sT; g.sH = d->sH; g.sW = d->sW; g.ldy = d->ldy;
  g.R = (long)d->N * d->To * d->H * d->W;
  g.L = g.R < EW_MID_ROWS ? EW_SLICE_SMALL : (g.R < EW_BIG_ROWS ? EW_SLICE_MID : EW_SLICE_BIG);
  g.S = (int)((g.R + g.L - 1) / g.L);
  g.groups = (g.K + EW_CW - 1) / EW_CW;
  return g;
}

}  // namespace mspi

using namespace mspi;

extern "C" int mspi_conv_wgrad_entry_supported(const MspiConvDesc* d) {
  const char* why = entry_refusal(d);
  if (why) set_error("mspi_conv_wgrad_entry: %s", why);
  return why ? 0 : 1;
}

extern "C" size_t mspi_conv_wgrad_entry_ws_bytes(const MspiConvDesc* d) {
  if (entry_refusal(d)) return 0;
  const EntryGeom g = entry_geom(d);
  return (size_t)g.S * ew_record_floats(g.Cout, g.K) * sizeof(float);
}

extern "C" int mspi_conv_wgrad_entry_variant(const MspiConvDesc* d, const void* x, const void* dy) {
  const char* why = entry_refusal(d);
  if (!why && !(x && dy && aligned16(x) && aligned16(dy))) why = "x and dy must be 16-byte aligned";
  if (why) {
    set_error("mspi_conv_wgrad_entry: %s", why);
    return -1;
  }
  return entry_geom(d).L;
}

extern "C" int mspi_conv_wgrad_entry(const MspiConvDesc* d, const float* x, const float* dy, float* dW, float* db, void* ws,
                                     mspi_stream_t stream) {
  MSPI_REQUIRE(x && dy && dW && db && ws, "mspi_conv_wgrad_entry: null argument");
  if (mspi_conv_wgrad_entry_variant(d, x, dy) < 0) return MSPI_EINVAL;
  MSPI_REQUIRE(aligned16(ws) && aligned16(dW), "mspi_conv_wgrad_entry: dW and ws must be 16-byte aligned");
  const EntryGeom g = entry_geom(d);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(conv_wgrad_entry_kernel, dim3(g.S, g.groups), dim3(EW_T), 0, st, g, x, dy, (float*)ws);
  const long nW = (long)g.Cout * g.K, n = nW + g.Cout;
  hipLaunchKernelGGL(conv_wgrad_entry_reduce_kernel, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, st, (const float*)ws, g.S, nW, n,
                     dW, db);
  return check_launch("mspi_conv_wgrad_entry");
}
