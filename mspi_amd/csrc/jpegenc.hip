// Baseline JPEG encoder for uint8 grey maps on the device -- the last step of the reference's process()
// (inference.py:89-91, cv2.imwrite; PIL's Image.save(quality=95) in mspi_amd/inference.py).  One 8-bit component, 8x8 blocks
// in raster order, no restart markers, the Annex K luminance Huffman tables: the file libjpeg writes, byte for byte
// (integer "islow" FDCT of jfdctint.c, its quantiser rounding, jpeg_quality_scaling), so turning device encoding on changes no
// byte of a written map.  Everything is integer arithmetic; launches are bitwise reproducible.
//
// Four launches per batch:
//   1. count   one wave64 per block: FDCT, quantise, code lengths -> bits per block
//   2. scan    one workgroup per map: exclusive scan of the bit counts, zeroes the words of the scan the map needs and sets
//              the 1-bits that pad the last byte
//   3. emit    the same per-block code again, now with the codes: a block's bit string is put together in LDS and stored at
//              its bit offset; only the first and last word of a block, shared with its neighbours, are OR-ed atomically
//   4. stuff   one workgroup per map: header, FF -> FF 00 by count / scan / scatter over the scan bytes, EOI, file length
// Steps 1 and 3 recompute the block rather than keep 64 coefficients per block in the workspace: the arithmetic is a few
// hundred integer operations per block and the kernels are bound by launch latency.
#include "common.h"

namespace mspi {

namespace {

constexpr int kHeaderLen = 328;
constexpr int kMaxBlockBits = 20 + 63 * 26;     // DC: 9-bit code + 11 bits; each AC: 16-bit code + 10 bits, no EOB
constexpr int kLdsWords = 56;                   // (31 + kMaxBlockBits + 31) / 32 = 53 words, + the zero spill of a 3-word OR

constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr uint8_t kBaseLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                   14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                   18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kDcBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr uint8_t kAcVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// Symbol -> code and length by the canonical assignment of Annex C, worked out by the compiler.
struct HuffTable {
  uint16_t code[256];
  uint8_t len[256];
};
template <int NV>
constexpr HuffTable make_huff(const uint8_t (&bits)[16], const uint8_t (&vals)[NV]) {
  HuffTable t{};
  unsigned code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code) {
      t.code[vals[k]] = (uint16_t)code;
      t.len[vals[k]] = (uint8_t)l;
    }
    code <<= 1;
  }
  return t;
}

__constant__ const HuffTable c_dc = make_huff(kDcBits, kDcVals);
__constant__ const HuffTable c_ac = make_huff(kAcBits, kAcVals);
__constant__ const uint8_t c_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                           41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                           30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

void quality_table(int quality, uint8_t* q /* natural order */) {   // jpeg_quality_scaling + jpeg_add_quant_table(force_baseline)
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int i = 0; i < 64; ++i) {
    int v = (kBaseLuma[i] * scale + 50) / 100;
    q[i] = (uint8_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
  }
}

size_t blocks_of(int H, int W) { return (size_t)((H + 7) / 8) * (size_t)((W + 7) / 8); }
size_t scan_words_of(size_t nblk) { return (nblk * kMaxBlockBits + 31) / 32 + 2; }

struct JpegArgs {
  const uint8_t* maps;
  long pitch, map_stride;
  int H, W, bw, nblk;
  uint16_t div[64];      // zigzag order
};

#define DESCALE(x, n) (((x) + (1 << ((n) - 1))) >> (n))

// One pass of jfdctint.c over 8 values spaced `st` apart.  FIRST: the row pass (results scaled up by 2^PASS1_BITS = 4).
template <bool FIRST>
__device__ __forceinline__ void fdct8(int* d, int st) {
  constexpr int N = FIRST ? 11 : 15;      // CONST_BITS -/+ PASS1_BITS
  const int d0 = d[0], d1 = d[st], d2 = d[2 * st], d3 = d[3 * st], d4 = d[4 * st], d5 = d[5 * st], d6 = d[6 * st], d7 = d[7 * st];
  int tmp0 = d0 + d7, tmp7 = d0 - d7, tmp1 = d1 + d6, tmp6 = d1 - d6, tmp2 = d2 + d5, tmp5 = d2 - d5, tmp3 = d3 + d4, tmp4 = d3 - d4;
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  d[0] = FIRST ? (tmp10 + tmp11) << 2 : DESCALE(tmp10 + tmp11, 2);
  d[4 * st] = FIRST ? (tmp10 - tmp11) << 2 : DESCALE(tmp10 - tmp11, 2);
  int z1 = (tmp12 + tmp13) * 4433;
  d[2 * st] = DESCALE(z1 + tmp13 * 6270, N);
  d[6 * st] = DESCALE(z1 - tmp12 * 15137, N);
  z1 = tmp4 + tmp7;
  int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int z5 = (z3 + z4) * 9633;
  tmp4 *= 2446; tmp5 *= 16819; tmp6 *= 25172; tmp7 *= 12299;
  z1 *= -7373; z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d[7 * st] = DESCALE(tmp4 + z1 + z3, N);
  d[5 * st] = DESCALE(tmp5 + z2 + z4, N);
  d[3 * st] = DESCALE(tmp6 + z2 + z3, N);
  d[st] = DESCALE(tmp7 + z1 + z4, N);
}
#undef DESCALE

// libjpeg's quantiser: round half away from zero of c / div.  `/` on unsigned ints is exact.
__device__ __forceinline__ int quantise(int c, int div) {
  const unsigned t = ((unsigned)(c < 0 ? -c : c) + ((unsigned)div >> 1)) / (unsigned)div;
  return c < 0 ? -(int)t : (int)t;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned wave_scan_u(unsigned v, int lane) {   // inclusive
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

__device__ __forceinline__ void append(unsigned long long& acc, int& n, unsigned code, int len) {
  acc = (acc << len) | code;
  n += len;
}
// Size category of v and the bits libjpeg appends for it (v itself, or v - 1 in `nb` bits when negative).
__device__ __forceinline__ void magnitude(int v, int& nb, unsigned& vb) {
  const unsigned a = (unsigned)(v < 0 ? -v : v);
  nb = a ? 32 - __clz((int)a) : 0;
  vb = (unsigned)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u);
}

// One wave64 = one 8x8 block, four blocks per workgroup.  Lane l holds sample (l / 8, l % 8), later zigzag coefficient l.
template <bool EMIT>
__global__ __launch_bounds__(256) void jpeg_block_kernel(JpegArgs a, uint32_t* __restrict__ bits,
                                                          const unsigned long long* __restrict__ offs,
                                                          uint32_t* __restrict__ scan, long scan_words) {
  __shared__ int s_c[4][64];
  __shared__ uint32_t s_w[4][kLdsWords];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.y;
  int blk = blockIdx.x * 4 + wave;
  const bool valid = blk < a.nblk;
  if (!valid) blk = a.nblk - 1;           // keeps the barriers below uniform; nothing is stored for it
  const uint8_t* m = a.maps + (long)b * a.map_stride;
  const int by = blk / a.bw, bx = blk - by * a.bw;
  {   // the right and bottom edges replicate the last column and row
    const int y = min(by * 8 + (lane >> 3), a.H - 1), x = min(bx * 8 + (lane & 7), a.W - 1);
    s_c[wave][lane] = (int)m[(long)y * a.pitch + x] - 128;
  }
  // The DC term of the scaled FDCT is exactly the sum of the 64 centred samples ((4 S + 2) >> 2 = S), so the previous block's
  // DC -- the predictor -- is a wave sum over its samples rather than a value handed from block to block.
  int prev_sum = 0;
  if (blk > 0) {
    const int py = (blk - 1) / a.bw, px = (blk - 1) - py * a.bw;
    const int y = min(py * 8 + (lane >> 3), a.H - 1), x = min(px * 8 + (lane & 7), a.W - 1);
    prev_sum = wave_sum_i((int)m[(long)y * a.pitch + x] - 128);
  }
  if (EMIT && lane < kLdsWords) s_w[wave][lane] = 0;
  __syncthreads();
  if (lane < 8) fdct8<true>(&s_c[wave][lane * 8], 1);
  __syncthreads();
  if (lane < 8) fdct8<false>(&s_c[wave][lane], 8);
  __syncthreads();
  const int q = quantise(s_c[wave][c_zigzag[lane]], a.div[lane]);

  const bool nz = lane > 0 && q != 0;
  const unsigned long long mask = __ballot(nz);
  unsigned long long acc = 0;
  int n = 0, nb;
  unsigned vb;
  if (lane == 0) {
    magnitude(q - quantise(prev_sum, a.div[0]), nb, vb);
    append(acc, n, c_dc.code[nb], c_dc.len[nb]);
    append(acc, n, vb, nb);
  } else if (nz) {
    const unsigned long long below = mask & ((1ull << lane) - 1ull);
    const int prev = below ? 63 - __clzll((long long)below) : 0;
    const int run = lane - prev - 1;
    for (int z = run >> 4; z > 0; --z) append(acc, n, c_ac.code[0xF0], c_ac.len[0xF0]);     // ZRL: 16 zeros
    magnitude(q, nb, vb);
    const int sym = ((run & 15) << 4) | nb;
    append(acc, n, c_ac.code[sym], c_ac.len[sym]);
    append(acc, n, vb, nb);
  } else if (lane == 63) {
    append(acc, n, c_ac.code[0], c_ac.len[0]);                                               // EOB
  }
  const unsigned inc = wave_scan_u((unsigned)n, lane);
  const unsigned total = __shfl(inc, 63, 64);
  if (!EMIT) {
    if (valid && lane == 0) bits[(size_t)b * a.nblk + blk] = total;
    return;
  }
  const unsigned long long goff = offs[(size_t)b * a.nblk + blk];
  const unsigned sh = (unsigned)(goff & 31u);
  if (n > 0) {   // n <= 59 bits at bit p of the block's LDS words, most significant bit first: at most three words
    const unsigned p = sh + (inc - (unsigned)n), s = p & 31u;
    const unsigned long long v = acc << (64 - n);
    const unsigned long long hi = v >> s;
    const unsigned lo = s ? (unsigned)((v << (64 - s)) >> 32) : 0u;
    uint32_t* w = &s_w[wave][p >> 5];
    atomicOr(w, (unsigned)(hi >> 32));
    if ((unsigned)hi) atomicOr(w + 1, (unsigned)hi);
    if (lo) atomicOr(w + 2, lo);
  }
  __syncthreads();
  const int nw = (int)((sh + total + 31u) >> 5);
  if (valid && lane < nw) {
    uint32_t* g = scan + (size_t)b * scan_words + (size_t)(goff >> 5) + lane;
    const uint32_t val = s_w[wave][lane];
    if (lane == 0 || lane == nw - 1) atomicOr(g, val);      // shared with the neighbouring blocks (and the pad bits)
    else *g = val;
  }
}

// Exclusive scan of a map's per-block bit counts; one workgroup per map, 256 blocks per step.  Then the words of the scan that
// the map's bits reach are cleared for the emit kernel, the one holding the end of the stream with the 1-bits that pad it.
__global__ __launch_bounds__(256) void jpeg_scan_kernel(const uint32_t* __restrict__ bits, unsigned long long* __restrict__ offs,
                                                         unsigned long long* __restrict__ totals, uint32_t* __restrict__ scan,
                                                         long scan_words, int nblk) {
  __shared__ unsigned s_part[4];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  bits += (size_t)b * nblk;
  offs += (size_t)b * nblk;
  unsigned long long carry = 0;
  for (int base = 0; base < nblk; base += 256) {
    const int i = base + tid;
    const unsigned v = i < nblk ? bits[i] : 0u;
    const unsigned inc = wave_scan_u(v, lane);
    if (lane == 63) s_part[wave] = inc;
    __syncthreads();
    unsigned before = 0, all = 0;
    for (int w = 0; w < 4; ++w) {
      if (w < wave) before += s_part[w];
      all += s_part[w];
    }
    if (i < nblk) offs[i] = carry + before + (inc - v);
    carry += all;
    __syncthreads();
  }
  const unsigned long long T = carry;
  if (tid == 0) totals[b] = T;
  uint32_t* sw = scan + (size_t)b * scan_words;
  const unsigned long long nwords = (T + 31) >> 5;
  for (unsigned long long i = tid; i < nwords; i += 256) {
    uint32_t val = 0;
    if ((T & 7u) && i == (T >> 5)) {
      const unsigned s = (unsigned)(T & 31u), npad = 8u - (unsigned)(T & 7u);
      val = ((1u << npad) - 1u) << (32u - s - npad);
    }
    sw[i] = val;
  }
}

// The file of one map: header template, the scan with a zero byte behind every FF, EOI.  One workgroup per map; a thread takes
// 16 scan bytes per step, the FFs before them come from a scan over the workgroup.
__global__ __launch_bounds__(256) void jpeg_stuff_kernel(const uint32_t* __restrict__ scan, long scan_words,
                                                          const unsigned long long* __restrict__ totals,
                                                          const uint8_t* __restrict__ header, int hlen, uint8_t* __restrict__ files,
                                                          long file_stride, long cap, int32_t* __restrict__ lengths) {
  __shared__ unsigned s_part[4];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint32_t* sw = scan + (size_t)b * scan_words;
  uint8_t* out = files + (size_t)b * file_stride;
  const long n = (long)((totals[b] + 7) >> 3);
  for (int i = tid; i < hlen; i += 256)
    if (i < cap) out[i] = header[i];
  long carry = 0;
  for (long base = 0; base < n; base += 256 * 16) {
    const long i0 = base + (long)tid * 16;
    uint32_t w[4];
    unsigned cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      w[j] = i0 + 4 * j < n ? sw[(i0 >> 2) + j] : 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) cnt += (i0 + 4 * j + k < n && ((w[j] >> (24 - 8 * k)) & 255u) == 255u) ? 1u : 0u;
    }
    const unsigned inc = wave_scan_u(cnt, lane);
    if (lane == 63) s_part[wave] = inc;
    __syncthreads();
    unsigned before = 0, all = 0;
    for (int k = 0; k < 4; ++k) {
      if (k < wave) before += s_part[k];
      all += s_part[k];
    }
    long pos = hlen + i0 + carry + before + (inc - cnt);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (i0 + 4 * j + k < n) {
          const uint8_t v = (uint8_t)(w[j] >> (24 - 8 * k));
          if (pos < cap) out[pos] = v;
          ++pos;
          if (v == 255u) {
            if (pos < cap) out[pos] = 0;
            ++pos;
          }
        }
    carry += all;
    __syncthreads();
  }
  if (tid == 0) {
    const long pos = hlen + n + carry;
    if (pos < cap) out[pos] = 0xFF;
    if (pos + 1 < cap) out[pos + 1] = 0xD9;
    lengths[b] = (int32_t)(pos + 2);
  }
}

bool dims_ok(int H, int W) { return H >= 1 && H <= 65535 && W >= 1 && W <= 65535; }

}  // namespace

}  // namespace mspi

using namespace mspi;

extern "C" int mspi_jpeg_gray_header(int32_t H, int32_t W, int32_t quality, unsigned char* dst, int64_t cap) {
  MSPI_REQUIRE(dst, "mspi_jpeg_gray_header: null destination");
  MSPI_REQUIRE(dims_ok(H, W), "mspi_jpeg_gray_header: %d x %d is outside 1...65535", H, W);
  MSPI_REQUIRE(quality >= 1 && quality <= 100, "mspi_jpeg_gray_header: quality %d is outside 1...100", quality);
  MSPI_REQUIRE(cap >= kHeaderLen, "mspi_jpeg_gray_header: cap %lld is below the %d header bytes", (long long)cap, kHeaderLen);
  uint8_t q[64];
  quality_table(quality, q);
  unsigned char* p = dst;
  auto put = [&p](std::initializer_list<int> bytes) { for (int v : bytes) *p++ = (unsigned char)v; };
  put({0xFF, 0xD8});                                                                               // SOI
  put({0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});                      // APP0: JFIF 1.01, 1x1
  put({0xFF, 0xDB, 0, 67, 0});                                                                     // DQT, 8-bit, table 0
  for (int k = 0; k < 64; ++k) *p++ = q[kZigzag[k]];
  put({0xFF, 0xC0, 0, 11, 8, H >> 8, H & 255, W >> 8, W & 255, 1, 1, 0x11, 0});                    // SOF0
  put({0xFF, 0xC4, 0, 31, 0x00});                                                                  // DHT: DC table 0
  for (int i = 0; i < 16; ++i) *p++ = kDcBits[i];
  for (int i = 0; i < 12; ++i) *p++ = kDcVals[i];
  put({0xFF, 0xC4, 0, 181, 0x10});                                                                 // DHT: AC table 0
  for (int i = 0; i < 16; ++i) *p++ = kAcBits[i];
  for (int i = 0; i < 162; ++i) *p++ = kAcVals[i];
  put({0xFF, 0xDA, 0, 8, 1, 1, 0x00, 0, 63, 0});                                                   // SOS
  return (int)(p - dst);
}

extern "C" size_t mspi_jpeg_gray_bound(int32_t H, int32_t W) {
  if (!dims_ok(H, W)) return 0;
  return (size_t)kHeaderLen + 2 * ((blocks_of(H, W) * kMaxBlockBits + 7) / 8) + 2;
}

// workspace: bits u32 [B * nblk] | offs u64 [B * nblk] | totals u64 [B] | scan u32 [B * scan_words]
extern "C" size_t mspi_jpeg_gray_ws_bytes(int32_t B, int32_t H, int32_t W) {
  if (!dims_ok(H, W) || B < 1) return 0;
  const size_t nblk = blocks_of(H, W), cells = (size_t)B * nblk;
  return (cells + 1) / 2 * 8 + cells * 8 + (size_t)B * 8 + (size_t)B * scan_words_of(nblk) * 4;
}

extern "C" int mspi_jpeg_gray_fwd(const MspiJpegDesc* d, const unsigned char* maps, unsigned char* files, int32_t* lengths,
                                  void* ws, mspi_stream_t stream) {
  MSPI_REQUIRE(d && maps && files && lengths && ws, "mspi_jpeg_gray_fwd: null pointer");
  MSPI_REQUIRE(d->header, "mspi_jpeg_gray_fwd: null header template");
  MSPI_REQUIRE(dims_ok(d->H, d->W), "mspi_jpeg_gray_fwd: %d x %d is outside 1...65535", d->H, d->W);
  MSPI_REQUIRE(d->B >= 1 && d->B <= 65535, "mspi_jpeg_gray_fwd: batch %d is outside 1...65535", d->B);
  MSPI_REQUIRE(d->quality >= 1 && d->quality <= 100, "mspi_jpeg_gray_fwd: quality %d is outside 1...100", d->quality);
  const size_t bound = mspi_jpeg_gray_bound(d->H, d->W);
  MSPI_REQUIRE(bound <= 0x7fffffffu, "mspi_jpeg_gray_fwd: a %d x %d map can exceed the int32 file length", d->H, d->W);
  MSPI_REQUIRE(d->cap >= (int64_t)bound, "mspi_jpeg_gray_fwd: cap %lld is below mspi_jpeg_gray_bound = %zu", (long long)d->cap, bound);
  MSPI_REQUIRE(d->file_stride >= d->cap, "mspi_jpeg_gray_fwd: file stride %lld is below cap", (long long)d->file_stride);
  MSPI_REQUIRE(d->pitch >= d->W && (d->B == 1 || d->map_stride >= d->pitch * (int64_t)(d->H - 1) + d->W),
               "mspi_jpeg_gray_fwd: pitch %lld / map stride %lld do not hold a %d x %d map", (long long)d->pitch,
               (long long)d->map_stride, d->H, d->W);
  MSPI_REQUIRE(d->header_len == kHeaderLen, "mspi_jpeg_gray_fwd: header template of %d bytes, mspi_jpeg_gray_header writes %d",
               d->header_len, kHeaderLen);
  uint8_t q[64];
  quality_table(d->quality, q);
  JpegArgs a;
  for (int k = 0; k < 64; ++k) {
    MSPI_REQUIRE(d->div[k] == 8 * q[kZigzag[k]], "mspi_jpeg_gray_fwd: divisor %d is %d, quality %d gives 8 * %d", k, d->div[k],
                 d->quality, q[kZigzag[k]]);
    a.div[k] = d->div[k];
  }
  MSPI_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0, "mspi_jpeg_gray_fwd: workspace must be 8-byte aligned");
  a.maps = maps;
  a.pitch = d->pitch;
  a.map_stride = d->map_stride;
  a.H = d->H;
  a.W = d->W;
  a.bw = (d->W + 7) / 8;
  const size_t nblk = blocks_of(d->H, d->W), cells = (size_t)d->B * nblk;
  a.nblk = (int)nblk;
  const long sw = (long)scan_words_of(nblk);
  uint32_t* bits = reinterpret_cast<uint32_t*>(ws);
  unsigned long long* offs = reinterpret_cast<unsigned long long*>(bits + (cells + 1) / 2 * 2);
  unsigned long long* totals = offs + cells;
  uint32_t* scan = reinterpret_cast<uint32_t*>(totals + d->B);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((nblk + 3) / 4), d->B);
  hipLaunchKernelGGL(jpeg_block_kernel<false>, grid, dim3(256), 0, s, a, bits, offs, scan, sw);
  hipLaunchKernelGGL(jpeg_scan_kernel, dim3(d->B), dim3(256), 0, s, bits, offs, totals, scan, sw, a.nblk);
  hipLaunchKernelGGL(jpeg_block_kernel<true>, grid, dim3(256), 0, s, a, bits, offs, scan, sw);
  hipLaunchKernelGGL(jpeg_stuff_kernel, dim3(d->B), dim3(256), 0, s, scan, sw, totals, (const uint8_t*)d->header, d->header_len,
                     files, (long)d->file_stride, (long)d->cap, lengths);
  return check_launch("mspi_jpeg_gray_fwd");
}
