// Backward of the SyncBlock's transformer Block (model/model_utils.py:84-152): the two pieces no other file has.  Entry points
// (include/mspi_sync_train_hip.h), all fp32:
//   mspi_attn_bwd             dq, dk, dv of o = softmax(scale q k^T) v             two launches
//   mspi_layernorm_bwd_wide   mspi_layernorm_bwd for rows of 256 < C <= 512        one pass + the ordered add
// Attention on v_mfma_f32_32x32x2_f32 with the layout trick of attn.hip: the tile that is computed is the TRANSPOSED one, so
// that the row a softmax statistic belongs to sits on the lane and the probabilities are, as they leave the accumulator, the B
// operand of the product that consumes them.  Nothing is added across workgroups: every dq row belongs to the workgroup that
// owns its 128 queries, every dk / dv row to the workgroup that owns its 128 keys, and each walks the other side in tile order,
// so two runs give equal bits.  The forward stores no statistics; the first launch computes them again.
//   attn_bwd_dq_kernel    workgroup = 128 queries of one (sequence, head), a wave 32 of them, the query on the lane.
//       phase 1: over the key tiles, S^T = K . Qs^T (Qs = scale q) and the online maximum / sum -> lse = m + log(l); then
//                Delta = sum_d dO o.  Both go to the workspace ([B Hh][Nq] each) for the second launch.
//       phase 2: over the key tiles again, P^T = exp(S^T - lse), dP^T = V . dO^T, dS^T = P^T (dP^T - Delta),
//                dq^T += K^T . dS^T; dq = scale dq^T.
//   attn_bwd_dkv_kernel   workgroup = 128 keys, a wave 32 of them, the key on the lane; over the query tiles
//                S = Qs . K^T, P = exp(S - lse), dP = dO . V^T, dS = P (dP - Delta), dv^T += dO^T . P, dk^T += Qs^T . dS.
// Tiles of 32 rows are staged in LDS with rows padded by 4 floats (attn.hip: the fragment reads are conflict-free).  Padded
// keys get probability exactly 0 and padded queries add exactly 0 (the probability is selected, not computed).
// Four waves a workgroup whatever the grid: with one wave a workgroup the short grids of 2 clips fill the chip (208 workgroups
// instead of 56 at 820 tokens) but nothing hides a tile's staging, and the launch pair takes 1.08 ms instead of 0.67.
#include "common.h"
#include "../../include/mspi_sync_train_hip.h"

#include <string>

namespace mspi {

typedef float v16f __attribute__((ext_vector_type(16)));

struct AttnBwdArgs {
  const float* q;
  const float* k;
  const float* v;
  const float* o;
  const float* dO;
  float* dq;
  float* dk;
  float* dv;
  float* lse;      // workspace [B * Hh][Nq]
  float* delta;    // workspace [B * Hh][Nq]
  int B, Hh, Nq, Nk;
  long q_sB, q_sH, q_sT, k_sB, k_sH, k_sT, v_sB, v_sH, v_sT, o_sB, o_sH, o_sT;
  float scale;
  int* status;
};

// The accumulator row that register r holds in lane half lh (32x32x2 MFMA): also the k index that lane half supplies when
// register r is fed back as the B operand.
__device__ __forceinline__ int acc_row(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// Rows row0 .. row0 + 31 of the matrix at src (row stride ld) times mul into a [32][D + 4] LDS tile; rows beyond n are zeros.
template <int D>
__device__ __forceinline__ void stage_rows(float* dst, const float* src, long ld, int row0, int n, float mul) {
  constexpr int LDD = D + 4;
  for (int idx = threadIdx.x; idx < 32 * (D / 4); idx += 256) {
    const int row = idx / (D / 4), c4 = idx - row * (D / 4);
    const bool ok = row0 + row < n;
    float4 t = *reinterpret_cast<const float4*>(src + (ok ? (long)(row0 + row) * ld + c4 * 4 : 0));
    t = ok ? make_float4(t.x * mul, t.y * mul, t.z * mul, t.w * mul) : make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(&dst[row * LDD + c4 * 4]) = t;
  }
}

// The lane's own row as the B operand: lane half lh keeps the columns 4 (2 j + lh) .. + 3 of chunk j, times mul; zeros if !ok.
template <int D>
__device__ __forceinline__ void load_row(const float* p, bool ok, int lh, float mul, float4 (&r)[D / 8]) {
#pragma unroll
  for (int j = 0; j < D / 8; ++j) {
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) t = *reinterpret_cast<const float4*>(p + 4 * (2 * j + lh));
    r[j] = make_float4(t.x * mul, t.y * mul, t.z * mul, t.w * mul);
  }
}

// acc[row][col] = sum_d T[row][d] R[col][d]: A = the rows of the LDS tile T (row on the lane), B = the lane's row R in registers.
template <int D>
__device__ __forceinline__ v16f tile_dot(const float* T, const float4 (&r)[D / 8], int li, int lh) {
  constexpr int LDD = D + 4;
  v16f s;
#pragma unroll
  for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
  for (int j = 0; j < D / 8; ++j) {
    const float4 a = *reinterpret_cast<const float4*>(&T[li * LDD + 4 * (2 * j + lh)]);
    s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, r[j].x, s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, r[j].y, s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, r[j].z, s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, r[j].w, s, 0, 0, 0);
  }
  return s;
}

// acc[t][d][col] += sum_row T[row][t * 32 + d] b[row][col]: A = T^T read from the LDS tile at the row my half supplies, B = the
// registers of b as they left the accumulator.
template <int D>
__device__ __forceinline__ void tile_tdot(const float* T, const v16f& b, int li, int lh, v16f (&acc)[D / 32]) {
  constexpr int LDD = D + 4;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = acc_row(r, lh);
#pragma unroll
    for (int t = 0; t < D / 32; ++t) {
      const float a = T[row * LDD + t * 32 + li];
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[r], acc[t], 0, 0, 0);
    }
  }
}

// One output row: accumulators times mul, range guard, 16-byte stores.  Lane half lh holds, in registers 4g .. 4g+3 of tile t,
// the 4 consecutive d = t * 32 + 8 g + 4 lh + (0..3).
template <int NT>
__device__ __forceinline__ void store_row(const v16f (&acc)[NT], float mul, int lh, float* dst, int* status) {
  bool bad = false;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 o4 = make_float4(acc[t][4 * g] * mul, acc[t][4 * g + 1] * mul, acc[t][4 * g + 2] * mul, acc[t][4 * g + 3] * mul);
      bad |= nonfinite(o4.x) || nonfinite(o4.y) || nonfinite(o4.z) || nonfinite(o4.w);
      *reinterpret_cast<float4*>(dst + t * 32 + 8 * g + 4 * lh) = o4;
    }
  report_nonfinite(status, bad);
}

template <int D, int DV>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const AttnBwdArgs p) {
  constexpr int LDD = D + 4, LDV = DV + 4;
  __shared__ __attribute__((aligned(16))) float smem[32 * LDD + 32 * LDV];
  float* Ks = smem;
  float* Vs = smem + 32 * LDD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int b = blockIdx.y / p.Hh, h = blockIdx.y % p.Hh;
  const int q = blockIdx.x * 128 + wave * 32 + li;
  const bool qok = q < p.Nq;
  const long qrow = qok ? q : 0;
  const float* kb = p.k + (long)b * p.k_sB + (long)h * p.k_sH;
  const float* vb = p.v + (long)b * p.v_sB + (long)h * p.v_sH;
  const long oo = (long)b * p.o_sB + (long)h * p.o_sH + qrow * p.o_sT;

  float4 qr[D / 8];
  load_row<D>(p.q + (long)b * p.q_sB + (long)h * p.q_sH + qrow * p.q_sT, qok, lh, p.scale, qr);

  // ---- phase 1: the statistics of my query
  float m_run = -INFINITY, l_run = 0.f;
  for (int k0 = 0; k0 < p.Nk; k0 += 32) {
    __syncthreads();
    stage_rows<D>(Ks, kb, p.k_sT, k0, p.Nk, 1.f);
    __syncthreads();
    v16f s = tile_dot<D>(Ks, qr, li, lh);
    float mt = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (k0 + acc_row(r, lh) >= p.Nk) s[r] = -INFINITY;
      mt = fmaxf(mt, s[r]);
    }
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const float m_new = fmaxf(m_run, mt);      // finite: every tile holds at least one valid key
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) ps += expf(s[r] - m_new);
    ps += __shfl_xor(ps, 32, 64);
    l_run = l_run * expf(m_run - m_new) + ps;
    m_run = m_new;
  }
  const float lse = m_run + logf(l_run);

  float4 dor[DV / 8];
  load_row<DV>(p.dO + oo, qok, lh, 1.f, dor);
  float delta = 0.f;
#pragma unroll
  for (int j = 0; j < DV / 8; ++j) {
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (qok) t = *reinterpret_cast<const float4*>(p.o + oo + 4 * (2 * j + lh));
    delta += (dor[j].x * t.x + dor[j].y * t.y) + (dor[j].z * t.z + dor[j].w * t.w);
  }
  delta += __shfl_xor(delta, 32, 64);
  if (qok && lh == 0) {
    p.lse[(long)blockIdx.y * p.Nq + q] = lse;
    p.delta[(long)blockIdx.y * p.Nq + q] = delta;
  }

  // ---- phase 2: dq
  v16f acc[D / 32];
#pragma unroll
  for (int t = 0; t < D / 32; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  for (int k0 = 0; k0 < p.Nk; k0 += 32) {
    __syncthreads();
    stage_rows<D>(Ks, kb, p.k_sT, k0, p.Nk, 1.f);
    stage_rows<DV>(Vs, vb, p.v_sT, k0, p.Nk, 1.f);
    __syncthreads();
    v16f s = tile_dot<D>(Ks, qr, li, lh);
    const v16f dp = tile_dot<DV>(Vs, dor, li, lh);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool kok = k0 + acc_row(r, lh) < p.Nk;
      const float pr = expf(s[r] - lse);
      s[r] = kok ? pr * (dp[r] - delta) : 0.f;
    }
    tile_tdot<D>(Ks, s, li, lh, acc);
  }
  if (qok) store_row<D / 32>(acc, p.scale, lh, p.dq + (long)b * p.q_sB + (long)h * p.q_sH + qrow * p.q_sT, p.status);
}

template <int D, int DV>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(const AttnBwdArgs p) {
  constexpr int LDD = D + 4, LDV = DV + 4;
  __shared__ __attribute__((aligned(16))) float smem[32 * LDD + 32 * LDV + 64];
  float* Qs = smem;
  float* Gs = smem + 32 * LDD;                 // dO
  float* Ls = smem + 32 * LDD + 32 * LDV;      // lse [32], Delta [32]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int b = blockIdx.y / p.Hh, h = blockIdx.y % p.Hh;
  const int key = blockIdx.x * 128 + wave * 32 + li;
  const bool kok = key < p.Nk;
  const long krow = kok ? key : 0;
  const float* qb = p.q + (long)b * p.q_sB + (long)h * p.q_sH;
  const float* gb = p.dO + (long)b * p.o_sB + (long)h * p.o_sH;
  const float* lseb = p.lse + (long)blockIdx.y * p.Nq;
  const float* delb = p.delta + (long)blockIdx.y * p.Nq;

  float4 kr[D / 8], vr[DV / 8];
  load_row<D>(p.k + (long)b * p.k_sB + (long)h * p.k_sH + krow * p.k_sT, kok, lh, 1.f, kr);
  load_row<DV>(p.v + (long)b * p.v_sB + (long)h * p.v_sH + krow * p.v_sT, kok, lh, 1.f, vr);

  v16f acck[D / 32], accv[DV / 32];
#pragma unroll
  for (int t = 0; t < D / 32; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acck[t][r] = 0.f;
#pragma unroll
  for (int t = 0; t < DV / 32; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) accv[t][r] = 0.f;

  for (int q0 = 0; q0 < p.Nq; q0 += 32) {
    __syncthreads();
    stage_rows<D>(Qs, qb, p.q_sT, q0, p.Nq, p.scale);
    stage_rows<DV>(Gs, gb, p.o_sT, q0, p.Nq, 1.f);
    if (tid < 64) {
      const int i = tid & 31;
      const bool ok = q0 + i < p.Nq;
      const float t = (tid < 32 ? lseb : delb)[ok ? q0 + i : 0];
      Ls[tid] = ok ? t : 0.f;
    }
    __syncthreads();
    v16f s = tile_dot<D>(Qs, kr, li, lh);
    v16f dp = tile_dot<DV>(Gs, vr, li, lh);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = acc_row(r, lh);
      const bool ok = kok && q0 + row < p.Nq;
      const float pr = expf(s[r] - Ls[row]);
      s[r] = ok ? pr : 0.f;
      dp[r] = ok ? pr * (dp[r] - Ls[32 + row]) : 0.f;
    }
    tile_tdot<DV>(Gs, s, li, lh, accv);
    tile_tdot<D>(Qs, dp, li, lh, acck);
  }
  if (kok) {
    store_row<D / 32>(acck, 1.f, lh, p.dk + (long)b * p.k_sB + (long)h * p.k_sH + krow * p.k_sT, p.status);
    store_row<DV / 32>(accv, 1.f, lh, p.dv + (long)b * p.v_sB + (long)h * p.v_sH + krow * p.v_sT, p.status);
  }
}

// ------------------------------------------------------------------------------------------------ LayerNorm, 256 < C <= 512
// The lanes of layernorm_kernel<32, 4> (rowops.hip, ln_select): 32 lanes own a row, lane `sub` its vectors sub, sub + 32, ...;
// mean and rstd by the same two passes and the same xor tree, so x^ has the forward's bits.  A workgroup walks LNW_ROWS rows, 8
// at a time, and keeps its lanes' shares of dgamma and dbeta in registers; they meet across the two row slots of a wave by one
// shuffle, across the four waves through LDS in wave order, and leave as one record [dbeta | dgamma].
constexpr int LNW_ROWS = 256;
constexpr int LNW_MINC = 260, LNW_MAXC = 512;
constexpr int LNW_VPT = 4;

__host__ __device__ inline int lnw_groups(long M) { return (int)((M + LNW_ROWS - 1) / LNW_ROWS); }

__device__ __forceinline__ float row32_sum(float s) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

__global__ __launch_bounds__(256) void layernorm_bwd_wide_kernel(const float* __restrict__ x, long ldx, const float* dy, long lddy,
                                                                 const float* __restrict__ gamma, float eps, float* dx, long lddx,
                                                                 float* __restrict__ ws, long M, int C) {
  constexpr int VPT = LNW_VPT;
  __shared__ float4 sh[4][2][32 * VPT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane & 31;
  const int nv = C >> 2;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 gam[VPT], sg[VPT], sb[VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int i = sub + 32 * j;
    gam[j] = *reinterpret_cast<const float4*>(gamma + (i < nv ? i : 0) * 4);
    sg[j] = zero;
    sb[j] = zero;
  }
  const long base = (long)blockIdx.x * LNW_ROWS;
  for (int pass = 0; pass < LNW_ROWS / 8; ++pass) {
    if (base + pass * 8 >= M) break;                  // uniform over the workgroup
    const long row = base + pass * 8 + wave * 2 + (lane >> 5);
    const bool rok = row < M;                         // dead rows stay in the shuffles on row 0's data and add nothing
    const long rr = rok ? row : 0;
    float4 v[VPT], d[VPT];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const int i = sub + 32 * j;
      const float4 t = *reinterpret_cast<const float4*>(x + rr * ldx + (i < nv ? i : 0) * 4);
      const float4 u = *reinterpret_cast<const float4*>(dy + rr * lddy + (i < nv ? i : 0) * 4);
      v[j] = i < nv ? t : zero;
      d[j] = i < nv ? u : zero;
      s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
    }
    const float mean = row32_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      if (sub + 32 * j < nv) {
        const float a = v[j].x - mean, b = v[j].y - mean, c = v[j].z - mean, e = v[j].w - mean;
        q += (a * a + b * b) + (c * c + e * e);
      }
    }
    const float rstd = rsqrtf(row32_sum(q) / (float)C + eps);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      if (sub + 32 * j < nv) {
        v[j] = make_float4((v[j].x - mean) * rstd, (v[j].y - mean) * rstd, (v[j].z - mean) * rstd, (v[j].w - mean) * rstd);   // x^
        const float4 a = make_float4(d[j].x * gam[j].x, d[j].y * gam[j].y, d[j].z * gam[j].z, d[j].w * gam[j].w);
        s1 += (a.x + a.y) + (a.z + a.w);
        s2 += (a.x * v[j].x + a.y * v[j].y) + (a.z * v[j].z + a.w * v[j].w);
      }
    }
    const float m1 = row32_sum(s1) / (float)C, m2 = row32_sum(s2) / (float)C;
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const int i = sub + 32 * j;
      if (rok && i < nv) {
        float4 o;
        o.x = rstd * (d[j].x * gam[j].x - m1 - v[j].x * m2);
        o.y = rstd * (d[j].y * gam[j].y - m1 - v[j].y * m2);
        o.z = rstd * (d[j].z * gam[j].z - m1 - v[j].z * m2);
        o.w = rstd * (d[j].w * gam[j].w - m1 - v[j].w * m2);
        *reinterpret_cast<float4*>(dx + row * lddx + i * 4) = o;
        sg[j].x = fmaf(d[j].x, v[j].x, sg[j].x); sg[j].y = fmaf(d[j].y, v[j].y, sg[j].y);
        sg[j].z = fmaf(d[j].z, v[j].z, sg[j].z); sg[j].w = fmaf(d[j].w, v[j].w, sg[j].w);
        sb[j].x += d[j].x; sb[j].y += d[j].y; sb[j].z += d[j].z; sb[j].w += d[j].w;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    sg[j].x += __shfl_xor(sg[j].x, 32, 64); sg[j].y += __shfl_xor(sg[j].y, 32, 64);
    sg[j].z += __shfl_xor(sg[j].z, 32, 64); sg[j].w += __shfl_xor(sg[j].w, 32, 64);
    sb[j].x += __shfl_xor(sb[j].x, 32, 64); sb[j].y += __shfl_xor(sb[j].y, 32, 64);
    sb[j].z += __shfl_xor(sb[j].z, 32, 64); sb[j].w += __shfl_xor(sb[j].w, 32, 64);
    if (lane < 32) {
      sh[wave][0][sub + 32 * j] = sb[j];
      sh[wave][1][sub + 32 * j] = sg[j];
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < 2 * nv) {
    const int which = (int)threadIdx.x / nv, i = (int)threadIdx.x - which * nv;
    const float4 a = sh[0][which][i], b = sh[1][which][i], c = sh[2][which][i], e = sh[3][which][i];
    float* rec = ws + (long)blockIdx.x * 2 * C + which * C + i * 4;
    *reinterpret_cast<float4*>(rec) = make_float4((a.x + b.x) + (c.x + e.x), (a.y + b.y) + (c.y + e.y), (a.z + b.z) + (c.z + e.z),
                                                  (a.w + b.w) + (c.w + e.w));
  }
}

// Sum of the S records [n] in ws, element e to a[e] (e < nA) or b[e - nA]; grid ceil(n / 64).
__global__ __launch_bounds__(256) void sync_reduce_kernel(const float* __restrict__ ws, int S, int n, int nA, float* __restrict__ a,
                                                          float* __restrict__ b) {
  __shared__ float part[4][64];
  const int e = blockIdx.x * 64 + (threadIdx.x & 63);
  const bool live = e < n;
  const float r = rt_sum_records(ws + (live ? e : 0), n, S, live, part);
  if (threadIdx.x < 64 && live) {
    if (e < nA) a[e] = r;
    else b[e - nA] = r;
  }
}

static const char* lnw_refusal(int64_t M, int32_t C) {
  if (M <= 0) return "no rows";
  if (M >= (1L << 31)) return "2^31 or more rows";
  if (C < LNW_MINC || C > LNW_MAXC || C % 4) return "C must be a multiple of 4 with 256 < C <= 512 (mspi_layernorm_bwd takes C <= 256)";
  return nullptr;
}

static bool lnw_rows_ok(const void* p, int64_t ld, int32_t C) { return p && aligned16(p) && ld >= C && ld % 4 == 0; }

// ------------------------------------------------------------------------------------------------ attention backward: host side
// The instantiated (D, Dv) pairs: here and in mspi_attn_bwd's switch.
struct AttnBwdPair { int D, Dv; };
static constexpr AttnBwdPair kAttnBwdPairs[] = {{128, 128}};

static bool attn_bwd_pair_ok(int D, int Dv) {
  for (const AttnBwdPair& p : kAttnBwdPairs)
    if (p.D == D && p.Dv == Dv) return true;
  return false;
}

static std::string attn_bwd_pairs() {
  std::string t;
  for (const AttnBwdPair& p : kAttnBwdPairs) t += (t.empty() ? "(" : ",(") + std::to_string(p.D) + "," + std::to_string(p.Dv) + ")";
  return t;
}

// What the launch refuses for the descriptor alone; nullptr = accepted.  `why` receives the text.
static bool attn_bwd_desc_ok(const MspiAttnDesc* d, std::string& why) {
  if (!d) { why = "null descriptor"; return false; }
  if (d->B <= 0 || d->Hh <= 0 || d->Nq <= 0 || d->Nk <= 0) { why = "empty extent"; return false; }
  if (d->prec != MSPI_PREC_F32) {
    why = "prec = " + std::to_string(d->prec) + ": only MSPI_PREC_F32 (the operands are gradients, the f16x3 split is not exact there)";
    return false;
  }
  if (!attn_bwd_pair_ok(d->D, d->Dv)) {
    why = "(D=" + std::to_string(d->D) + ", Dv=" + std::to_string(d->Dv) + ") not in {" + attn_bwd_pairs() + "}";
    return false;
  }
  if (d->nmask != 0 || d->nwin != 0) { why = "no mask and no token index (nmask and nwin must be 0)"; return false; }
  const int64_t st[12] = {d->q_sB, d->q_sH, d->q_sT, d->k_sB, d->k_sH, d->k_sT, d->v_sB, d->v_sH, d->v_sT, d->o_sB, d->o_sH, d->o_sT};
  for (int i = 0; i < 12; ++i)
    if (st[i] & 3) { why = "strides must be multiples of 4 floats"; return false; }
  if ((long)d->B * d->Hh >= 65536) { why = "B*H too large"; return false; }
  return true;
}

}  // namespace mspi

using namespace mspi;

extern "C" size_t mspi_attn_bwd_ws_bytes(const MspiAttnDesc* d) {
  std::string why;
  if (!attn_bwd_desc_ok(d, why)) return 0;
  return (size_t)d->B * d->Hh * d->Nq * 2 * sizeof(float);
}

extern "C" int mspi_attn_bwd_variant(const MspiAttnDesc* d) {
  std::string why;
  if (!attn_bwd_desc_ok(d, why)) {
    set_error("mspi_attn_bwd_variant: %s", why.c_str());
    return -1;
  }
  return 10000000 + d->D * 10000 + d->Dv * 10;
}

extern "C" int mspi_attn_bwd(const MspiAttnDesc* d, const float* q, const float* k, const float* v, const float* o, const float* dO,
                             float* dq, float* dk, float* dv, void* ws, mspi_stream_t stream) {
  MSPI_REQUIRE(d && q && k && v && o && dO && dq && dk && dv && ws, "mspi_attn_bwd: null argument");
  std::string why;
  MSPI_REQUIRE(attn_bwd_desc_ok(d, why), "mspi_attn_bwd: %s", why.c_str());
  MSPI_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(o) && aligned16(dO) && aligned16(dq) && aligned16(dk) &&
                   aligned16(dv) && aligned16(ws), "mspi_attn_bwd: pointers must be 16-B aligned");
  AttnBwdArgs a;
  a.q = q; a.k = k; a.v = v; a.o = o; a.dO = dO; a.dq = dq; a.dk = dk; a.dv = dv;
  a.lse = reinterpret_cast<float*>(ws);
  a.delta = a.lse + (long)d->B * d->Hh * d->Nq;
  a.B = d->B; a.Hh = d->Hh; a.Nq = d->Nq; a.Nk = d->Nk;
  a.q_sB = d->q_sB; a.q_sH = d->q_sH; a.q_sT = d->q_sT;
  a.k_sB = d->k_sB; a.k_sH = d->k_sH; a.k_sT = d->k_sT;
  a.v_sB = d->v_sB; a.v_sH = d->v_sH; a.v_sT = d->v_sT;
  a.o_sB = d->o_sB; a.o_sH = d->o_sH; a.o_sT = d->o_sT;
  a.scale = d->scale;
  a.status = g_status_word;
  hipStream_t s = (hipStream_t)stream;
  const dim3 gq((unsigned)((d->Nq + 127) / 128), (unsigned)(d->B * d->Hh)), gk((unsigned)((d->Nk + 127) / 128), (unsigned)(d->B * d->Hh));
  switch (d->D * 1000 + d->Dv) {      // one case per row of kAttnBwdPairs
    case 128128:
      hipLaunchKernelGGL((attn_bwd_dq_kernel<128, 128>), gq, dim3(256), 0, s, a);
      hipLaunchKernelGGL((attn_bwd_dkv_kernel<128, 128>), gk, dim3(256), 0, s, a);
      break;
    default: MSPI_REQUIRE(false, "mspi_attn_bwd: (D=%d, Dv=%d) not in {%s}", d->D, d->Dv, attn_bwd_pairs().c_str());
  }
  return check_launch("mspi_attn_bwd");
}

extern "C" size_t mspi_layernorm_bwd_wide_ws_bytes(int64_t M, int32_t C) {
  if (lnw_refusal(M, C)) return 0;
  return (size_t)lnw_groups(M) * 2 * C * sizeof(float);
}

extern "C" int mspi_layernorm_bwd_wide(const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* gamma, float eps,
                                       float* dx, int64_t lddx, float* dgamma, float* dbeta, void* ws, int64_t M, int32_t C,
                                       mspi_stream_t stream) {
  MSPI_REQUIRE(x && dy && gamma && dx && dgamma && dbeta && ws, "mspi_layernorm_bwd_wide: null argument");
  const char* why = lnw_refusal(M, C);
  MSPI_REQUIRE(!why, "mspi_layernorm_bwd_wide: C=%d: %s", C, why);
  MSPI_REQUIRE(eps >= 0.f, "mspi_layernorm_bwd_wide: negative eps");
  MSPI_REQUIRE(lnw_rows_ok(x, ldx, C) && lnw_rows_ok(dy, lddy, C) && lnw_rows_ok(dx, lddx, C),
               "mspi_layernorm_bwd_wide: x, dy and dx must be 16-byte aligned, their row strides multiples of 4, >= C");
  MSPI_REQUIRE(aligned16(gamma) && aligned16(ws), "mspi_layernorm_bwd_wide: gamma and ws must be 16-byte aligned");
  const int G = lnw_groups(M);
  hipStream_t st = (hipStream_t)stream;
  float* w = (float*)ws;
  hipLaunchKernelGGL(layernorm_bwd_wide_kernel, dim3(G), dim3(256), 0, st, x, (long)ldx, dy, (long)lddy, gamma, eps, dx, (long)lddx, w,
                     (long)M, C);
  hipLaunchKernelGGL(sync_reduce_kernel, dim3((2 * C + 63) / 64), dim3(256), 0, st, (const float*)w, G, 2 * C, C, dbeta, dgamma);
  return check_launch("mspi_layernorm_bwd_wide");
}
