// Baseline JPEG decoder for the input frames on the device -- Image.open(path).convert('RGB') of the reference's
// torch_transform (inference.py:154-165), i.e. libjpeg-turbo's default decode, pixel for pixel: Huffman decoding, the integer
// "islow" IDCT of jidctint.c, fancy (triangle) chroma up-sampling of jdsample.c and the fixed-point YCbCr -> RGB of jdcolor.c.
// Everything is integer arithmetic; launches are bitwise reproducible.
//
// A scan without restart markers has no entry points, so the entropy decoder synchronises itself: the unstuffed scan is cut
// into subsequences of S bits, every lane decodes its own from a guessed state, then again from the state its left neighbour
// ended in, until a pass changes no end state.  Lane 0 starts from the truth, so the fixed point is the sequential decode
// whatever the data; Huffman streams re-synchronise quickly, so natural frames settle in a few passes.
//
// Five launches and one memset per batch of B images of one geometry (tables and scan lengths are per image):
//   1. unstuff   one workgroup per image: FF 00 -> FF by flag / scan / compact, sixteen FF bytes behind the end
//   2. entropy   one workgroup of 1024 lanes per image: synchronise, count blocks, scan the counts, decode once more writing
//                int16 coefficients in natural order to ws[block][64] (DC terms as differences); status and pass count
//   3. dc        one workgroup per image: per-component prefix sum of the DC differences over the blocks in scan order
//   4. idct      eight lanes per block: dequantise, IDCT, clamp -> padded uint8 component planes
//   5. convert   one lane per pixel: up-sample the chroma planes, convert, store HWC through the caller's pitch
// Speculative lanes decode garbage by design and files can be corrupt: every position, block index and coefficient index
// is bounded, a missing code consumes 16 bits, and every store is guarded by the image's own block count and size.
#include "common.h"

namespace mspi {

namespace {

constexpr int kMaxLanes = 1024;
constexpr int kTailPad = 16;                    // FF bytes behind the unstuffed scan: a lane reads at most 12 bytes past its position

__constant__ const uint8_t c_natural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                  41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                  30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

size_t rup16(size_t v) { return (v + 15) / 16 * 16; }

// Geometry of one image and the layout of its workspace: scan bytes | meta | coefficients | component planes.
struct Geo {
  int H, W, ncomp, hs, vs;
  int mx, my, bpm, nblk;          // MCUs across / down, blocks per MCU, blocks per image
  int pw[3], ph[3];               // padded plane sizes
  size_t off_meta, off_coef, off_plane[3], ws_stride;
};

bool make_geo(const MspiJpegDecDesc* d, Geo& g) {
  g.H = d->H; g.W = d->W; g.ncomp = d->ncomp; g.hs = d->hs; g.vs = d->vs;
  const int mw = 8 * d->hs, mh = 8 * d->vs;
  g.mx = (d->W + mw - 1) / mw;
  g.my = (d->H + mh - 1) / mh;
  g.bpm = d->ncomp == 1 ? 1 : d->hs * d->vs + 2;
  const long nblk = (long)g.mx * g.my * g.bpm;
  if (nblk > 0x7fffffffL / 64) return false;
  g.nblk = (int)nblk;
  size_t off = rup16((size_t)d->scan_cap + kTailPad);
  g.off_meta = off;
  off += 16;
  g.off_coef = off;
  off += (size_t)nblk * 128;
  for (int c = 0; c < 3; ++c) {
    g.pw[c] = c < d->ncomp ? g.mx * 8 * (c == 0 ? d->hs : 1) : 0;
    g.ph[c] = c < d->ncomp ? g.my * 8 * (c == 0 ? d->vs : 1) : 0;
    g.off_plane[c] = off;
    off += rup16((size_t)g.pw[c] * g.ph[c]);
  }
  g.ws_stride = off;
  return true;
}

__device__ __forceinline__ int comp_of(const Geo& g, int r) {   // component of block r of an MCU
  const int ny = g.hs * g.vs;
  return g.ncomp == 1 || r < ny ? 0 : r - ny + 1;
}

__device__ __forceinline__ unsigned wave_scan_incl(unsigned v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// Exclusive scan over the workgroup (blockDim.x / 64 <= 16 waves); `total` is the sum.  Two barriers.
__device__ __forceinline__ int block_scan_excl(int v, int* s_part, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int inc = (int)wave_scan_incl((unsigned)v, lane);
  if (lane == 63) s_part[wave] = inc;
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < nw; ++w) {
    if (w < wave) before += s_part[w];
    all += s_part[w];
  }
  __syncthreads();
  total = all;
  return before + inc - v;
}

// ----------------------------------------------------------------------------------------------------------- 1. unstuff
__global__ __launch_bounds__(kMaxLanes) void jpegdec_unstuff_kernel(Geo g, const uint8_t* __restrict__ scans, long scan_stride, long scan_cap,
                                                               const MspiJpegDecTables* __restrict__ tabs, uint8_t* __restrict__ ws) {
  __shared__ int s_part[16];
  const int b = blockIdx.x, tid = threadIdx.x;
  const uint8_t* src = scans + (size_t)b * scan_stride;
  uint8_t* dst = ws + (size_t)b * g.ws_stride;
  long n = tabs[b].scan_len;
  n = n < 0 ? 0 : (n > scan_cap ? scan_cap : n);
  long carry = 0;
  for (long base = 0; base < n; base += kMaxLanes * 16) {
    const long i0 = base + (long)tid * 16;
    uint8_t v[16];
    unsigned keep = 0;
    uint8_t prev = i0 > 0 && i0 <= n ? src[i0 - 1] : 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      v[j] = i0 + j < n ? src[i0 + j] : 0;
      if (i0 + j < n && !(v[j] == 0 && prev == 0xFF)) keep |= 1u << j;
      prev = v[j];
    }
    int all;
    long pos = carry + block_scan_excl(__popc(keep), s_part, all);
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (keep & (1u << j)) dst[pos++] = v[j];           // pos < n <= scan_cap
    carry += all;
  }
  if (tid < kTailPad) dst[carry + tid] = 0xFF;           // the tail of 1-bits
  if (tid == 0) *reinterpret_cast<int*>(dst + g.off_meta) = (int)carry;
}

// ----------------------------------------------------------------------------------------------------------- 2. entropy
struct HuffLds {
  uint16_t lut[4][512];       // 9 leading bits -> length << 8 | symbol; 0: a longer code, or none
  int maxcode[4][17];         // largest code of length l, -1 where there is none
  int valoff[4][17];          // index of the first symbol of length l minus its code
  uint8_t vals[4][256];
};

struct State {
  int pos, bk;                // bit position; block within the MCU * 64 + coefficient index (0: a DC code is next)
};
__device__ __forceinline__ bool same(State a, State b) { return a.pos == b.pos && a.bk == b.bk; }

// Decode from `st` until the position reaches `limit` (a symbol that starts before it is finished).  Returns the blocks
// completed.  EMIT: also store the coefficients of blocks gblk... < expected, and the position behind block expected - 1.
template <bool EMIT>
__device__ __forceinline__ int decode_run(const HuffLds& h, const uint8_t* s_tdc, const uint8_t* s_tac, const uint8_t* s_nat, int bpm,
                                          const uint32_t* __restrict__ words, State& st, int limit, int16_t* __restrict__ coef,
                                          long gblk, long expected, int* endpos) {
  int pos = st.pos, blk = st.bk >> 6, k = st.bk & 63, done = 0;
  // hi : lo is the 64-bit window at word cw; nx, the word behind it, is loaded one refill early so that its latency is
  // not waited for by the wave every time one of its lanes crosses a word
  int cw = pos >> 5;
  uint32_t hi = 0, lo = 0, nx = 0;
  if (pos < limit) {
    hi = __builtin_bswap32(words[cw]);
    lo = __builtin_bswap32(words[cw + 1]);
    nx = words[cw + 2];
  }
  while (pos < limit) {
    const int w = pos >> 5;
    if (w != cw) {
      if (w == cw + 1) {
        hi = lo;
        lo = __builtin_bswap32(nx);
      } else {              // a symbol of up to 31 bits crosses at most one word; 16 skipped bits none more: not reached
        hi = __builtin_bswap32(words[w]);
        lo = __builtin_bswap32(words[w + 1]);
      }
      nx = words[w + 2];
      cw = w;
    }
    const int sh = pos & 31;
    const uint32_t bits = sh ? (hi << sh) | (lo >> (32 - sh)) : hi;
    const int t = k == 0 ? s_tdc[blk] : s_tac[blk];
    const unsigned e = h.lut[t][bits >> 23];
    int len = (int)(e >> 8), sym = (int)(e & 255u);
    if (len == 0) {
      for (int l = 10; l <= 16; ++l) {
        const int c = (int)(bits >> (32 - l));
        if (c <= h.maxcode[t][l]) {
          len = l;
          sym = h.vals[t][(h.valoff[t][l] + c) & 255];
          break;
        }
      }
      if (len == 0) {         // no such code: step over 16 bits, the state stays
        pos += 16;
        continue;
      }
    }
    const int s = sym & 15;
    int v = 0;
    if (s) {                  // len + s <= 31
      const int ext = (int)((bits << len) >> (32 - s));
      v = ext < (1 << (s - 1)) ? ext - (1 << s) + 1 : ext;
    }
    pos += len + s;
    if (k == 0) {
      if (EMIT && gblk < expected) coef[gblk * 64] = (int16_t)v;
      k = 1;
    } else if (s == 0) {
      k = (sym >> 4) == 15 ? k + 16 : 64;              // ZRL / EOB
    } else {
      k += sym >> 4;
      if (EMIT && k < 64 && gblk < expected) coef[gblk * 64 + s_nat[k]] = (int16_t)v;
      ++k;
    }
    if (k >= 64) {
      k = 0;
      blk = blk + 1 == bpm ? 0 : blk + 1;
      ++done;
      if (EMIT) {
        ++gblk;
        if (gblk == expected) *endpos = pos;
      }
    }
  }
  st.pos = pos;
  st.bk = blk * 64 + k;
  return done;
}

__global__ __launch_bounds__(kMaxLanes) void jpegdec_entropy_kernel(Geo g, int S, const MspiJpegDecTables* __restrict__ tabs,
                                                                     uint8_t* __restrict__ ws, int32_t* __restrict__ status,
                                                                     int32_t* __restrict__ passes) {
  __shared__ HuffLds h;
  __shared__ State s_end[2][kMaxLanes];
  __shared__ uint8_t s_tdc[8], s_tac[8], s_nat[64];
  __shared__ int s_part[16];
  __shared__ int s_endpos;
  const int b = blockIdx.x, i = threadIdx.x;
  const MspiJpegDecTables& tb = tabs[b];
  uint8_t* wsb = ws + (size_t)b * g.ws_stride;
  const uint32_t* words = reinterpret_cast<const uint32_t*>(wsb);
  int16_t* coef = reinterpret_cast<int16_t*>(wsb + g.off_coef);
  const int nbits = 8 * *reinterpret_cast<const int*>(wsb + g.off_meta);
  int n = (int)(((long)nbits + S - 1) / S);
  n = n > kMaxLanes ? kMaxLanes : n;                    // the host refused descriptors that could give more

  for (int j = i; j < 4 * 512; j += kMaxLanes) (&h.lut[0][0])[j] = 0;
  (&h.vals[0][0])[i] = (&tb.vals[0][0])[i];
  if (i < 8) {
    const int c = comp_of(g, i < g.bpm ? i : 0);
    s_tdc[i] = tb.comp_dc[c] & 1;
    s_tac[i] = 2 + (tb.comp_ac[c] & 1);
  }
  if (i == 0) s_endpos = -1;
  if (i < 64) s_nat[i] = c_natural[i];
  __syncthreads();
  if (i < 4) {   // canonical codes of Annex C; tables that claim more code space than there is are cut at the LUT's end
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
      const int cnt = tb.counts[i][l - 1];
      h.valoff[i][l] = k - code;
      for (int c = 0; c < cnt; ++c, ++code, ++k) {
        if (l <= 9) {
          const int base = code << (9 - l);
          for (int f = 0; f < (1 << (9 - l)); ++f)
            if (base + f < 512) h.lut[i][base + f] = (uint16_t)(l << 8 | h.vals[i][k & 255]);
        }
      }
      h.maxcode[i][l] = cnt ? code - 1 : -1;
      code <<= 1;
    }
  }
  __syncthreads();

  const bool active = i < n;
  const int limit = active ? min((i + 1) * S, nbits) : 0;
  State start = {active ? i * S : 0, 0}, end = start;
  int cnt = 0;
  if (active) cnt = decode_run<false>(h, s_tdc, s_tac, s_nat, g.bpm, words, end, limit, nullptr, 0, 0, nullptr);
  s_end[0][i] = end;
  int npass = 1;
  for (;; ++npass) {      // pass `npass` (pass 0 was the guess): one barrier, inside __syncthreads_or, per pass; the last one confirms
    __syncthreads();
    bool changed = false;
    if (active && i > 0) {
      const State from = s_end[(npass - 1) & 1][i - 1];
      if (!same(from, start)) {
        start = from;
        State e = from;
        cnt = decode_run<false>(h, s_tdc, s_tac, s_nat, g.bpm, words, e, limit, nullptr, 0, 0, nullptr);
        changed = !same(e, end);
        end = e;
      }
    }
    s_end[npass & 1][i] = end;
    if (!__syncthreads_or(changed)) break;
  }

  int total;
  const int base = block_scan_excl(cnt, s_part, total);
  if (active) {
    State e = start;
    decode_run<true>(h, s_tdc, s_tac, s_nat, g.bpm, words, e, limit, coef, base, g.nblk, &s_endpos);
  }
  __syncthreads();
  if (i == 0) {
    const int ep = s_endpos;
    status[b] = total < g.nblk ? 1 : (total > g.nblk ? 2 : (ep > nbits - 8 && ep <= nbits ? 0 : 3));
    passes[b] = npass;
  }
}

// ----------------------------------------------------------------------------------------------------------- 3. dc
__global__ __launch_bounds__(kMaxLanes) void jpegdec_dc_kernel(Geo g, uint8_t* __restrict__ ws) {
  __shared__ int s_part[16];
  const int b = blockIdx.x, i = threadIdx.x;
  int16_t* coef = reinterpret_cast<int16_t*>(ws + (size_t)b * g.ws_stride + g.off_coef);
  const long nmcu = (long)g.mx * g.my, per = (nmcu + kMaxLanes - 1) / kMaxLanes;
  const long m0 = min((long)i * per, nmcu), m1 = min(m0 + per, nmcu);
  int sum[3] = {0, 0, 0};
  for (long m = m0; m < m1; ++m)
    for (int r = 0; r < g.bpm; ++r) sum[comp_of(g, r)] += coef[(m * g.bpm + r) * 64];
  int pred[3], all;
  for (int c = 0; c < 3; ++c) pred[c] = block_scan_excl(sum[c], s_part, all);
  for (long m = m0; m < m1; ++m)
    for (int r = 0; r < g.bpm; ++r) {
      const int c = comp_of(g, r);
      pred[c] += coef[(m * g.bpm + r) * 64];
      coef[(m * g.bpm + r) * 64] = (int16_t)pred[c];
    }
}

// ----------------------------------------------------------------------------------------------------------- 4. idct
#define DESCALE(x, n) (((x) + (1 << ((n) - 1))) >> (n))
// One pass of jidctint.c (CONST_BITS 13, PASS1_BITS 2) over eight values.  ROW: the second pass, + 128 and clamp.
template <bool ROW>
__device__ __forceinline__ void idct8(const int* in, int* out) {
  constexpr int N = ROW ? 18 : 11;
  int z2 = in[2], z3 = in[6];
  int z1 = (z2 + z3) * 4433;
  int tmp2 = z1 + z3 * -15137, tmp3 = z1 + z2 * 6270;
  int tmp0 = (in[0] + in[4]) << 13, tmp1 = (in[0] - in[4]) << 13;
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
  z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
  int z4 = tmp1 + tmp3;
  const int z5 = (z3 + z4) * 9633;
  tmp0 *= 2446; tmp1 *= 16819; tmp2 *= 25172; tmp3 *= 12299;
  z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
  z3 += z5; z4 += z5;
  tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
  out[0] = DESCALE(tmp10 + tmp3, N); out[7] = DESCALE(tmp10 - tmp3, N);
  out[1] = DESCALE(tmp11 + tmp2, N); out[6] = DESCALE(tmp11 - tmp2, N);
  out[2] = DESCALE(tmp12 + tmp1, N); out[5] = DESCALE(tmp12 - tmp1, N);
  out[3] = DESCALE(tmp13 + tmp0, N); out[4] = DESCALE(tmp13 - tmp0, N);
  if (ROW) {
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = min(max(out[j] + 128, 0), 255);
  }
}
#undef DESCALE

// 32 blocks per workgroup, eight lanes per block: lane j takes column j, then row j.
__global__ __launch_bounds__(256) void jpegdec_idct_kernel(Geo g, const MspiJpegDecTables* __restrict__ tabs, uint8_t* __restrict__ ws) {
  __shared__ int s_w[32][65];
  const int b = blockIdx.y, bl = threadIdx.x >> 3, j = threadIdx.x & 7;
  const long gb = (long)blockIdx.x * 32 + bl;
  const bool valid = gb < g.nblk;
  uint8_t* wsb = ws + (size_t)b * g.ws_stride;
  int comp = 0, by = 0, bx = 0;
  if (valid) {
    const long m = gb / g.bpm;
    const int r = (int)(gb - m * g.bpm), my = (int)(m / g.mx), mx = (int)(m - (long)my * g.mx);
    comp = comp_of(g, r);
    if (comp == 0 && g.ncomp == 3) {
      by = my * g.vs + r / g.hs;
      bx = mx * g.hs + r % g.hs;
    } else {
      by = my;
      bx = mx;
    }
    const int16_t* coef = reinterpret_cast<const int16_t*>(wsb + g.off_coef) + gb * 64;
    const uint16_t* q = tabs[b].quant[comp];
    int in[8], out[8];
#pragma unroll
    for (int r8 = 0; r8 < 8; ++r8) in[r8] = (int)coef[8 * r8 + j] * (int)q[8 * r8 + j];
    idct8<false>(in, out);
#pragma unroll
    for (int r8 = 0; r8 < 8; ++r8) s_w[bl][8 * r8 + j] = out[r8];
  }
  __syncthreads();
  if (valid) {
    int in[8], out[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) in[c] = s_w[bl][8 * j + c];
    idct8<true>(in, out);
    uint8_t* row = wsb + g.off_plane[comp] + (size_t)(by * 8 + j) * g.pw[comp] + bx * 8;      // 8-byte aligned
    uint2 v;
    v.x = (unsigned)out[0] | (unsigned)out[1] << 8 | (unsigned)out[2] << 16 | (unsigned)out[3] << 24;
    v.y = (unsigned)out[4] | (unsigned)out[5] << 8 | (unsigned)out[6] << 16 | (unsigned)out[7] << 24;
    *reinterpret_cast<uint2*>(row) = v;
  }
}

// ----------------------------------------------------------------------------------------------------------- 5. convert
// Chroma sample (x, y) of the full-size image from a plane of cw x ch real samples: jdsample.c's fancy up-sampling with the
// edge row / column replicated (h2v1: (3 near + far + 1 or 2) >> 2; h2v2: row sums 3 near + far, then (3 near + far + 8 or 7) >> 4).
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ p, int pw, int cw, int ch, int hs, int vs, int x, int y) {
  if (hs == 1) return p[(size_t)y * pw + x];
  const int i = x >> 1, io = (x & 1) ? min(i + 1, cw - 1) : max(i - 1, 0);
  if (vs == 1) {
    const uint8_t* row = p + (size_t)y * pw;
    return (3 * row[i] + row[io] + ((x & 1) ? 2 : 1)) >> 2;
  }
  const int yn = y >> 1, yf = (y & 1) ? min(yn + 1, ch - 1) : max(yn - 1, 0);
  const uint8_t* near = p + (size_t)yn * pw;
  const uint8_t* far = p + (size_t)yf * pw;
  const int ri = 3 * near[i] + far[i], ro = 3 * near[io] + far[io];
  return (3 * ri + ro + ((x & 1) ? 7 : 8)) >> 4;
}

__global__ __launch_bounds__(256) void jpegdec_convert_kernel(Geo g, const uint8_t* __restrict__ ws, uint8_t* __restrict__ rgb,
                                                               long pitch, long img_stride) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  if (x >= g.W) return;
  const uint8_t* wsb = ws + (size_t)b * g.ws_stride;
  const int Y = wsb[g.off_plane[0] + (size_t)y * g.pw[0] + x];
  int R = Y, G = Y, B = Y;
  if (g.ncomp == 3) {
    const int cw = (g.W + g.hs - 1) / g.hs, ch = (g.H + g.vs - 1) / g.vs;
    const int cb = chroma_at(wsb + g.off_plane[1], g.pw[1], cw, ch, g.hs, g.vs, x, y) - 128;
    const int cr = chroma_at(wsb + g.off_plane[2], g.pw[2], cw, ch, g.hs, g.vs, x, y) - 128;
    R = min(max(Y + ((91881 * cr + 32768) >> 16), 0), 255);
    G = min(max(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0), 255);
    B = min(max(Y + ((116130 * cb + 32768) >> 16), 0), 255);
  }
  uint8_t* o = rgb + (size_t)b * img_stride + (size_t)y * pitch + 3 * (size_t)x;
  o[0] = (uint8_t)R;
  o[1] = (uint8_t)G;
  o[2] = (uint8_t)B;
}

// ----------------------------------------------------------------------------------------------------------- host
bool dims_ok(int H, int W) { return H >= 1 && H <= 65535 && W >= 1 && W <= 65535; }

int check_desc(const MspiJpegDecDesc* d, const char* who) {
  MSPI_REQUIRE(d, "%s: null descriptor", who);
  MSPI_REQUIRE(dims_ok(d->H, d->W), "%s: %d x %d is outside 1...65535", who, d->H, d->W);
  MSPI_REQUIRE(d->B >= 1 && d->B <= 65535, "%s: batch %d is outside 1...65535", who, d->B);
  MSPI_REQUIRE(d->ncomp == 1 || d->ncomp == 3, "%s: %d components (1 or 3)", who, d->ncomp);
  MSPI_REQUIRE((d->hs == 1 && d->vs == 1) || (d->ncomp == 3 && d->hs == 2 && (d->vs == 1 || d->vs == 2)),
               "%s: sampling %d x %d of %d components (1x1, 2x1 or 2x2)", who, d->hs, d->vs, d->ncomp);
  MSPI_REQUIRE(d->hs == 1 || d->W >= 3, "%s: chroma width of a %d-pixel row is below 2", who, d->W);
  MSPI_REQUIRE(d->S >= 128 && d->S % 32 == 0 && d->S <= (1 << 24), "%s: S = %d is not a multiple of 32 in 128...2^24", who, d->S);
  MSPI_REQUIRE(d->scan_cap >= 1 && d->scan_cap <= (1 << 27), "%s: scan_cap %lld is outside 1...2^27", who, (long long)d->scan_cap);
  MSPI_REQUIRE((8 * d->scan_cap + d->S - 1) / d->S <= kMaxLanes, "%s: S = %d cuts %lld scan bytes into more than %d subsequences",
               who, d->S, (long long)d->scan_cap, kMaxLanes);
  Geo g;
  MSPI_REQUIRE(make_geo(d, g), "%s: a %d x %d image has too many blocks", who, d->H, d->W);
  return MSPI_OK;
}

int be16(const unsigned char* p) { return p[0] << 8 | p[1]; }

}  // namespace

}  // namespace mspi

using namespace mspi;

extern "C" int mspi_jpeg_dec_parse(const unsigned char* file, int64_t n, MspiJpegDecInfo* info) {
  MSPI_REQUIRE(info, "mspi_jpeg_dec_parse: null info");
  MSPI_REQUIRE(file && n > 0, "mspi_jpeg_dec_parse: empty input");
  MSPI_REQUIRE(n >= 4 && file[0] == 0xFF && file[1] == 0xD8, "mspi_jpeg_dec_parse: not a JPEG file (no SOI)");
  MSPI_REQUIRE(n <= 0x7fffffff, "mspi_jpeg_dec_parse: a file of %lld bytes", (long long)n);
  memset(info, 0, sizeof(*info));
  uint16_t qt[4][64];
  bool have_q[4] = {false, false, false, false}, have_h[4] = {false, false, false, false};
  bool sof = false, jfif = false, adobe = false;
  int adobe_transform = -1, comp_id[3] = {0, 0, 0}, comp_tq[3] = {0, 0, 0};
  int64_t p = 2;
  for (;;) {
    MSPI_REQUIRE(p + 4 <= n, "mspi_jpeg_dec_parse: truncated header (the file ends at byte %lld before SOS)", (long long)n);
    MSPI_REQUIRE(file[p] == 0xFF, "mspi_jpeg_dec_parse: no marker at byte %lld", (long long)p);
    const int m = file[p + 1];
    if (m == 0xFF) { ++p; continue; }                                           // fill byte
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD8)) { p += 2; continue; }            // stand-alone markers
    MSPI_REQUIRE(m != 0xD9, "mspi_jpeg_dec_parse: EOI before any scan");
    const int len = be16(file + p + 2);
    MSPI_REQUIRE(len >= 2 && p + 2 + len <= n, "mspi_jpeg_dec_parse: truncated header (segment %02X at byte %lld runs past the file)",
                 m, (long long)p);
    const unsigned char* seg = file + p + 4;
    const int sl = len - 2;
    if (m == 0xDB) {
      for (int o = 0; o < sl;) {
        const int pq = seg[o] >> 4, tq = seg[o] & 15;
        MSPI_REQUIRE(pq == 0, "mspi_jpeg_dec_parse: unsupported: 16-bit DQT");
        MSPI_REQUIRE(tq < 4 && o + 65 <= sl, "mspi_jpeg_dec_parse: bad DQT segment");
        for (int k = 0; k < 64; ++k) qt[tq][kNatural[k]] = seg[o + 1 + k];
        have_q[tq] = true;
        o += 65;
      }
    } else if (m == 0xC4) {
      for (int o = 0; o < sl;) {
        MSPI_REQUIRE(o + 17 <= sl, "mspi_jpeg_dec_parse: bad DHT segment");
        const int tc = seg[o] >> 4, th = seg[o] & 15;
        MSPI_REQUIRE(tc < 2 && th < 2, "mspi_jpeg_dec_parse: unsupported: Huffman table class %d id %d (baseline has 0 / 1)", tc, th);
        int total = 0, code = 0;
        for (int l = 0; l < 16; ++l) {
          total += seg[o + 1 + l];
          code = (code + seg[o + 1 + l]) << 1;
          MSPI_REQUIRE(code <= (2 << (l + 1)), "mspi_jpeg_dec_parse: DHT claims more codes of length %d than exist", l + 1);
        }
        MSPI_REQUIRE(total <= 256 && o + 17 + total <= sl, "mspi_jpeg_dec_parse: bad DHT segment");
        const int t = tc * 2 + th;
        memset(info->tables.vals[t], 0, 256);
        memcpy(info->tables.counts[t], seg + o + 1, 16);
        memcpy(info->tables.vals[t], seg + o + 17, total);
        have_h[t] = true;
        o += 17 + total;
      }
    } else if (m == 0xC0) {
      MSPI_REQUIRE(!sof, "mspi_jpeg_dec_parse: two SOF segments");
      MSPI_REQUIRE(sl >= 6, "mspi_jpeg_dec_parse: bad SOF segment");
      MSPI_REQUIRE(seg[0] == 8, "mspi_jpeg_dec_parse: unsupported: %d-bit samples", seg[0]);
      info->H = be16(seg + 1);
      info->W = be16(seg + 3);
      info->ncomp = seg[5];
      MSPI_REQUIRE(info->H >= 1 && info->W >= 1, "mspi_jpeg_dec_parse: unsupported: %d x %d image (DNL)", info->H, info->W);
      MSPI_REQUIRE(info->ncomp == 1 || info->ncomp == 3, "mspi_jpeg_dec_parse: unsupported: %d components (CMYK / YCCK)", info->ncomp);
      MSPI_REQUIRE(sl >= 6 + 3 * info->ncomp, "mspi_jpeg_dec_parse: bad SOF segment");
      for (int c = 0; c < info->ncomp; ++c) {
        const int hv = seg[7 + 3 * c], h = hv >> 4, v = hv & 15;
        comp_id[c] = seg[6 + 3 * c];
        comp_tq[c] = seg[8 + 3 * c];
        MSPI_REQUIRE(comp_tq[c] < 4, "mspi_jpeg_dec_parse: bad SOF segment");
        if (c == 0) {
          info->hs = h;
          info->vs = v;
        } else {
          MSPI_REQUIRE(h == 1 && v == 1, "mspi_jpeg_dec_parse: unsupported: chroma sampling %d x %d", h, v);
        }
      }
      if (info->ncomp == 1) info->hs = info->vs = 1;         // a one-component scan is not interleaved: its factors do not matter
      MSPI_REQUIRE((info->hs == 1 && info->vs == 1) || (info->hs == 2 && (info->vs == 1 || info->vs == 2)),
                   "mspi_jpeg_dec_parse: unsupported: luma sampling %d x %d", info->hs, info->vs);
      MSPI_REQUIRE(info->hs == 1 || info->W >= 3, "mspi_jpeg_dec_parse: unsupported: chroma width below 2");
      sof = true;
    } else if (m == 0xC2 || m == 0xC6 || m == 0xCA || m == 0xCE) {
      MSPI_REQUIRE(false, "mspi_jpeg_dec_parse: unsupported: progressive JPEG (SOF%d)", m - 0xC0);
    } else if (m == 0xCC || (m >= 0xC9 && m <= 0xCF)) {
      MSPI_REQUIRE(false, "mspi_jpeg_dec_parse: unsupported: arithmetic coding (marker %02X)", m);
    } else if (m >= 0xC1 && m <= 0xC7) {
      MSPI_REQUIRE(false, "mspi_jpeg_dec_parse: unsupported: SOF%d (only baseline SOF0)", m - 0xC0);
    } else if (m == 0xDD) {
      MSPI_REQUIRE(sl >= 2, "mspi_jpeg_dec_parse: bad DRI segment");
      MSPI_REQUIRE(be16(seg) == 0, "mspi_jpeg_dec_parse: unsupported: restart interval %d", be16(seg));
    } else if (m == 0xE0) {
      jfif = jfif || (sl >= 5 && memcmp(seg, "JFIF", 5) == 0);
    } else if (m == 0xEE) {
      if (sl >= 12 && memcmp(seg, "Adobe", 5) == 0) {
        adobe = true;
        adobe_transform = seg[11];
      }
    } else if (m == 0xDA) {
      MSPI_REQUIRE(sof, "mspi_jpeg_dec_parse: SOS before SOF0");
      MSPI_REQUIRE(sl >= 1 && sl >= 4 + 2 * seg[0], "mspi_jpeg_dec_parse: bad SOS segment");
      MSPI_REQUIRE(seg[0] == info->ncomp, "mspi_jpeg_dec_parse: unsupported: a scan of %d of %d components (several scans)", seg[0],
                   info->ncomp);
      for (int c = 0; c < info->ncomp; ++c) {
        MSPI_REQUIRE(seg[1 + 2 * c] == comp_id[c], "mspi_jpeg_dec_parse: unsupported: scan components out of frame order");
        const int td = seg[2 + 2 * c] >> 4, ta = seg[2 + 2 * c] & 15;
        MSPI_REQUIRE(td < 2 && ta < 2 && have_h[td] && have_h[2 + ta], "mspi_jpeg_dec_parse: component %d uses a Huffman table the file does not define", c);
        MSPI_REQUIRE(have_q[comp_tq[c]], "mspi_jpeg_dec_parse: component %d uses a quantiser table the file does not define", c);
        info->tables.comp_dc[c] = (uint8_t)td;
        info->tables.comp_ac[c] = (uint8_t)ta;
        memcpy(info->tables.quant[c], qt[comp_tq[c]], sizeof(qt[0]));
      }
      const unsigned char* t = seg + 1 + 2 * info->ncomp;
      MSPI_REQUIRE(t[0] == 0 && t[1] == 63 && t[2] == 0, "mspi_jpeg_dec_parse: unsupported: spectral selection %d...%d / approximation %02X",
                   t[0], t[1], t[2]);
      if (info->ncomp == 3) {
        MSPI_REQUIRE(!adobe || adobe_transform == 1, "mspi_jpeg_dec_parse: unsupported: Adobe transform %d", adobe_transform);
        MSPI_REQUIRE(jfif || adobe || !(comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B'),
                     "mspi_jpeg_dec_parse: unsupported: RGB components");
      }
      p += 2 + len;
      break;
    }
    p += 2 + len;
  }
  int64_t e = p;
  while (e < n && !(file[e] == 0xFF && e + 1 < n && file[e + 1] != 0x00 && !(file[e + 1] >= 0xD0 && file[e + 1] <= 0xD7))) ++e;
  if (e == n && n > p && file[n - 1] == 0xFF) --e;      // a lone FF at the end of a cut file is no data
  MSPI_REQUIRE(e > p, "mspi_jpeg_dec_parse: truncated: no entropy-coded data behind SOS");
  MSPI_REQUIRE(e + 1 >= n || file[e + 1] == 0xD9, "mspi_jpeg_dec_parse: unsupported: marker %02X behind the scan (several scans)",
               file[e + 1]);
  info->scan_off = (int32_t)p;
  info->scan_len = (int32_t)(e - p);
  info->tables.scan_len = info->scan_len;
  return MSPI_OK;
}

extern "C" size_t mspi_jpeg_dec_ws_bytes(const MspiJpegDecDesc* d) {
  if (check_desc(d, "mspi_jpeg_dec_ws_bytes") != MSPI_OK) return 0;
  Geo g;
  make_geo(d, g);
  return g.ws_stride * (size_t)d->B;
}

extern "C" int mspi_jpeg_dec_fwd(const MspiJpegDecDesc* d, const unsigned char* scans, const MspiJpegDecTables* tables,
                                 unsigned char* rgb, int32_t* status, int32_t* passes, void* ws, mspi_stream_t stream) {
  MSPI_REQUIRE(d && scans && tables && rgb && status && passes && ws, "mspi_jpeg_dec_fwd: null pointer");
  if (check_desc(d, "mspi_jpeg_dec_fwd") != MSPI_OK) return MSPI_EINVAL;
  MSPI_REQUIRE(d->pitch >= 3 * (int64_t)d->W, "mspi_jpeg_dec_fwd: pitch %lld is below 3 * W = %d", (long long)d->pitch, 3 * d->W);
  MSPI_REQUIRE(d->B == 1 || d->img_stride >= d->pitch * (int64_t)(d->H - 1) + 3 * (int64_t)d->W,
               "mspi_jpeg_dec_fwd: image stride %lld does not hold a %d x %d image of pitch %lld", (long long)d->img_stride, d->H, d->W,
               (long long)d->pitch);
  MSPI_REQUIRE(d->B == 1 || d->scan_stride >= d->scan_cap, "mspi_jpeg_dec_fwd: scan stride %lld is below scan_cap %lld",
               (long long)d->scan_stride, (long long)d->scan_cap);
  MSPI_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15u) == 0 && (reinterpret_cast<uintptr_t>(tables) & 7u) == 0,
               "mspi_jpeg_dec_fwd: the workspace must be 16-byte and the tables 8-byte aligned");
  Geo g;
  make_geo(d, g);
  hipStream_t s = (hipStream_t)stream;
  uint8_t* w = reinterpret_cast<uint8_t*>(ws);
  if (hipMemsetAsync(w, 0, g.ws_stride * (size_t)d->B, s) != hipSuccess)      // coefficients the scan does not code are zero
    return check_launch("mspi_jpeg_dec_fwd");
  hipLaunchKernelGGL(jpegdec_unstuff_kernel, dim3(d->B), dim3(kMaxLanes), 0, s, g, scans, (long)d->scan_stride, (long)d->scan_cap, tables, w);
  hipLaunchKernelGGL(jpegdec_entropy_kernel, dim3(d->B), dim3(kMaxLanes), 0, s, g, d->S, tables, w, status, passes);
  hipLaunchKernelGGL(jpegdec_dc_kernel, dim3(d->B), dim3(kMaxLanes), 0, s, g, w);
  hipLaunchKernelGGL(jpegdec_idct_kernel, dim3((unsigned)((g.nblk + 31) / 32), d->B), dim3(256), 0, s, g, tables, w);
  hipLaunchKernelGGL(jpegdec_convert_kernel, dim3((unsigned)((d->W + 255) / 256), d->H, d->B), dim3(256), 0, s, g, w, rgb,
                     (long)d->pitch, (long)d->img_stride);
  return check_launch("mspi_jpeg_dec_fwd");
}
