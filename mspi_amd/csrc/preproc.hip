// Clip-loop pre-processing on the GPU (inference.py:24-63 and :154-165 upstream, where they
// are torchaudio / torchvision-on-PIL calls made once per sliding window on the host).
//
//  * log-spectrogram windows: the 16 kHz mono wave of a video sits in HBM once; every window of a batch is one grid row.
//    Spectrogram(n_fft=512, hop=160): Hann window, centre + reflect padding, power 2 -> log(p + 1e-6) -> per time column
//    standardisation over the 257 bins (unbiased std) -> crop / pad with 0.02 to Wa columns.  One workgroup per
//    (window, column); the 512-point DFT is evaluated directly against an LDS twiddle table with fp64 accumulation
//    (263 k FMA per column -- noise next to one conv), so there is no FFT plan and no intermediate in memory.
//  * frame resize + normalise: PIL's 8-bit bilinear resampling (antialiased: support scales with the shrink factor),
//    horizontal pass then vertical pass in its 22-bit fixed point with a uint8 intermediate -- integer arithmetic, so
//    the result is PIL's bit for bit -- followed by /255, -mean, /std into the NCHW fp32 frame the model takes.
#include "common.h"

namespace mspi {

constexpr int NFFT = 512, NBIN = 257;

__global__ __launch_bounds__(256) void logspec_kernel(const float* __restrict__ wave, long n_wave,
                                                      const int* __restrict__ seg,   // [B][3] = start, length, reversed
                                                      const float* __restrict__ win, float* __restrict__ out, int Wa, int hop,
                                                      float pad_value) {
  __shared__ double2 tw[NFFT];
  __shared__ float xs[NFFT];
  __shared__ float red[8];
  const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int start = seg[b * 3], len = seg[b * 3 + 1], rev = seg[b * 3 + 2];
  const int nframes = len > 0 ? 1 + len / hop : 0;
  float* o = out + (long)b * NBIN * Wa + f;
  if (f >= nframes) {        // uniform per block
    o[(long)tid * Wa] = pad_value;
    if (tid == 0) o[256L * Wa] = pad_value;
    return;
  }
  for (int j = tid; j < NFFT; j += 256) {
    double s, c;
    sincospi(2.0 * j / NFFT, &s, &c);
    tw[j] = make_double2(c, -s);
    int i = f * hop - NFFT / 2 + j;           // centre=True: the frame is centred on sample f*hop of the segment
    if (i < 0) i = -i;                        // reflect padding (requires len > NFFT/2, checked on the host)
    if (i >= len) i = 2 * (len - 1) - i;
    const long src = rev ? (long)start + len - 1 - i : (long)start + i;
    xs[j] = wave[src] * win[j];
  }
  __syncthreads();
  float lp[2];
  const int nb = tid == 0 ? 2 : 1;
  for (int q = 0; q < nb; ++q) {
    const int k = q == 0 ? tid : 256;
    double re = 0.0, im = 0.0;
#pragma unroll 8
    for (int n = 0; n < NFFT; ++n) {
      const double2 t = tw[(k * n) & (NFFT - 1)];
      const double x = (double)xs[n];
      re = fma(x, t.x, re);
      im = fma(x, t.y, im);
    }
    const float p = (float)(re * re + im * im);
    lp[q] = logf(p + 1e-6f);
  }
  // mean / unbiased std over the 257 bins of this column.  This summation order is load-bearing: on digital silence all 257
  // values are logf(1e-6f), and wave_sum's butterfly, the four partial sums in this order and / 257 give that value back
  // exactly, so the column is exactly 0 (tests/test_logspec_kernel.py pins it).  That holds for this value and its 1-ulp
  // neighbours, not for every float: whoever reorders the sum should centre the values on lp[0] of thread 0 first.
  float s = lp[0] + (tid == 0 ? lp[1] : 0.f);
  s = wave_sum(s);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  const float mean = (red[0] + red[1] + red[2] + red[3]) / (float)NBIN;
  float d0 = lp[0] - mean, d1 = tid == 0 ? lp[1] - mean : 0.f;
  float v = wave_sum(d0 * d0 + d1 * d1);
  if ((tid & 63) == 0) red[4 + (tid >> 6)] = v;
  __syncthreads();
  const float sd = sqrtf((red[4] + red[5] + red[6] + red[7]) / (float)(NBIN - 1));
  const float inv = 1.f / (sd + 1e-6f);
  o[(long)tid * Wa] = d0 * inv;
  if (tid == 0) o[256L * Wa] = d1 * inv;
}

// PIL ImagingResample, 8 bits per channel: out = clip8((2^21 + sum_i in[xmin+i] * kk[i]) >> 22).
// Horizontal pass: src u8 [H][Win][3] (interleaved RGB) -> tmp u8 [H][Wout][3].
__global__ __launch_bounds__(256) void resample_h_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                         const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                         int H, int Win, int Wout) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)H * Wout) return;
  const int x = (int)(idx % Wout), y = (int)(idx / Wout);
  const int xmin = bounds[2 * x], n = bounds[2 * x + 1];
  const int* k = kk + (long)x * ksize;
  const unsigned char* row = src + ((long)y * Win + xmin) * 3;
  int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
  for (int i = 0; i < n; ++i) {
    const int w = k[i];
    s0 += row[3 * i] * w; s1 += row[3 * i + 1] * w; s2 += row[3 * i + 2] * w;
  }
  unsigned char* o = dst + idx * 3;
  o[0] = (unsigned char)min(255, max(0, s0 >> 22));
  o[1] = (unsigned char)min(255, max(0, s1 >> 22));
  o[2] = (unsigned char)min(255, max(0, s2 >> 22));
}

// Vertical pass + ToTensor + Normalize: tmp u8 [Hin][W][3] -> out fp32 [3][Hout][W] (plane stride out_sC floats).
__global__ __launch_bounds__(256) void resample_v_norm_kernel(const unsigned char* __restrict__ src, float* __restrict__ out,
                                                              long out_sC, const int* __restrict__ bounds,
                                                              const int* __restrict__ kk, int ksize, int Hin, int Hout, int W,
                                                              float m0, float m1, float m2, float d0, float d1, float d2) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)Hout * W) return;
  const int x = (int)(idx % W), y = (int)(idx / W);
  const int ymin = bounds[2 * y], n = bounds[2 * y + 1];
  const int* k = kk + (long)y * ksize;
  int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
  for (int i = 0; i < n; ++i) {
    const unsigned char* p = src + ((long)(ymin + i) * W + x) * 3;
    const int w = k[i];
    s0 += p[0] * w; s1 += p[1] * w; s2 += p[2] * w;
  }
  const float v0 = (float)min(255, max(0, s0 >> 22)), v1 = (float)min(255, max(0, s1 >> 22)), v2 = (float)min(255, max(0, s2 >> 22));
  out[idx] = (v0 / 255.f - m0) / d0;                 // ToTensor then Normalize, in that order and with true divisions
  out[out_sC + idx] = (v1 / 255.f - m1) / d1;
  out[2 * out_sC + idx] = (v2 / 255.f - m2) / d2;
}

}  // namespace mspi

using namespace mspi;

extern "C" int mspi_logspec_fwd(const float* wave, int64_t n_wave, const int32_t* seg, const int32_t* seg_host, int32_t B,
                                const float* window, float* out, int32_t Wa, mspi_stream_t stream) {
  MSPI_REQUIRE(wave && seg && seg_host && window && out && B > 0 && B < 65536 && Wa > 0 && n_wave > 0,
               "mspi_logspec_fwd: bad argument");
  for (int b = 0; b < B; ++b) {     // the host copy of the segment table is what makes the bounds checkable before launch
    const long st = seg_host[3 * b], len = seg_host[3 * b + 1];
    MSPI_REQUIRE(st >= 0 && len >= 0 && st + len <= n_wave, "mspi_logspec_fwd: window %d = [%ld, %ld) outside the %ld-sample wave",
                 b, st, st + len, (long)n_wave);
    MSPI_REQUIRE(len == 0 || len > NFFT / 2, "mspi_logspec_fwd: window %d has %ld samples; reflect padding needs more than %d",
                 b, len, NFFT / 2);
  }
  hipLaunchKernelGGL(logspec_kernel, dim3(Wa, B), dim3(256), 0, (hipStream_t)stream, wave, (long)n_wave, seg, window, out, Wa,
                     160, 0.02f);
  return check_launch("mspi_logspec_fwd");
}

extern "C" int mspi_resize_norm_fwd(const unsigned char* rgb, int32_t Hin, int32_t Win, unsigned char* tmp, float* out,
                                    int64_t out_plane_stride, int32_t Hout, int32_t Wout, const int32_t* hb,
                                    const int32_t* hk, int32_t hks, const int32_t* vb, const int32_t* vk, int32_t vks,
                                    const float* mean3_host, const float* std3_host, mspi_stream_t stream) {
  MSPI_REQUIRE(rgb && tmp && out && hb && hk && vb && vk && mean3_host && std3_host, "mspi_resize_norm_fwd: null argument");
  MSPI_REQUIRE(Hin > 0 && Win > 0 && Hout > 0 && Wout > 0 && hks > 0 && vks > 0 && out_plane_stride >= (int64_t)Hout * Wout,
               "mspi_resize_norm_fwd: bad extent");
  hipStream_t s = (hipStream_t)stream;
  const long n1 = (long)Hin * Wout, n2 = (long)Hout * Wout;
  hipLaunchKernelGGL(resample_h_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, s, rgb, tmp, hb, hk, hks, Hin, Win, Wout);
  hipLaunchKernelGGL(resample_v_norm_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, s, tmp, out, (long)out_plane_stride,
                     vb, vk, vks, Hin, Hout, Wout, mean3_host[0], mean3_host[1], mean3_host[2], std3_host[0], std3_host[1],
                     std3_host[2]);
  return check_launch("mspi_resize_norm_fwd");
}

// ------------------------------------------------------------------------------------------------ clip assembly
// N decoded frames of one source size -> their (b, t) slots of a fp32 [B][3][T][Hout][Wout] clip tensor, in ONE launch and
// with PIL's arithmetic (the two kernels above, fused).  A workgroup owns `TH` output rows of one frame at full width.  The
// input rows those output rows tap are one contiguous byte range of the frame: it is copied to LDS in batches of `RB` rows
// with aligned dword loads (a lane never issues a byte load to HBM, the thing resample_h_kernel spends its time on), the
// horizontal pass runs from that LDS copy into a second LDS image of uint8 rows, planar ([row][channel][WP]) so that the
// vertical pass reads ONE dword per tap for four neighbouring outputs and stores 16 bytes.  No intermediate leaves the CU.
namespace mspi {

constexpr long CLIP_RAW_BYTES = 8 * 1024;    // LDS for one batch of input rows
constexpr long CLIP_HBUF_BYTES = 32 * 1024;  // LDS for the horizontally resampled rows of a tile (40 KB in all: 4 workgroups / CU)
constexpr int CLIP_MAX_TH = 32, CLIP_MAX_RB = 8;

struct ClipPlan { int TH, R, RB, WP; long raw_bytes, lds_bytes; };

// Tile height from the vertical bounds table: the largest TH <= 32 whose tiles all need at most floor(32 KB / (3 * WP))
// staged rows.  False where not even one output row fits (extreme shrink factors, very wide frames).  vb must have passed
// check_bounds (monotonic, inside [0, Hin)).
static bool plan_clip(const int32_t* vb, long /*Hin*/, long Win, long Hout, long Wout, ClipPlan* p) {
  const long WP = (Wout + 3) & ~3L, rowbytes = Win * 3;
  if (rowbytes + 8 > CLIP_RAW_BYTES || 3 * WP > CLIP_HBUF_BYTES) return false;
  const long maxR = CLIP_HBUF_BYTES / (3 * WP);
  for (long th = Hout < CLIP_MAX_TH ? Hout : CLIP_MAX_TH; th >= 1; --th) {
    long need = 0;
    for (long y0 = 0; y0 < Hout; y0 += th) {
      const long y1 = (y0 + th < Hout ? y0 + th : Hout) - 1;
      const long r = (long)vb[2 * y1] + vb[2 * y1 + 1] - vb[2 * y0];
      if (r > need) need = r;
    }
    if (need <= maxR) {
      long rb = (CLIP_RAW_BYTES - 8) / rowbytes;
      if (rb > CLIP_MAX_RB) rb = CLIP_MAX_RB;
      if (rb > need) rb = need;
      p->TH = (int)th; p->R = (int)need; p->RB = (int)rb; p->WP = (int)WP;
      p->raw_bytes = (rb * rowbytes + 8 + 3) & ~3L;      // + the up to 3 bytes in front of an unaligned start, rounded to dwords
      p->lds_bytes = p->raw_bytes + need * 3 * WP;
      return true;
    }
  }
  return false;
}

// A PIL bounds table as the kernels index with it: taps inside [0, in_size), at least one and at most ksize per output,
// first index and end non-decreasing (what makes a tile's input rows one range).
static bool check_bounds(const int32_t* b, long out_size, long in_size, long ksize) {
  long prev0 = 0, prev1 = 0;
  for (long i = 0; i < out_size; ++i) {
    const long lo = b[2 * i], n = b[2 * i + 1];
    if (lo < 0 || n < 1 || n > ksize || lo + n > in_size || lo < prev0 || lo + n < prev1) return false;
    prev0 = lo; prev1 = lo + n;
  }
  return true;
}

// dword at byte offset a (a multiple of 4) of a 4-byte-aligned buffer of `total` bytes; the last, partial dword is put
// together from the bytes that exist.
__device__ __forceinline__ unsigned load_dword_in(const unsigned char* __restrict__ base, long a, long total) {
  if (a + 4 <= total) return *reinterpret_cast<const unsigned*>(base + a);
  unsigned v = 0;
  for (int j = 0; j < 4; ++j)
    if (a + j < total) v |= (unsigned)base[a + j] << (8 * j);
  return v;
}

__device__ __forceinline__ int clip8(int s) { return min(255, max(0, s >> 22)); }

template <bool VEC>
__global__ __launch_bounds__(256) void clip_resize_norm_kernel(
    const unsigned char* __restrict__ frames, long total_bytes, const int* __restrict__ slots, float* __restrict__ out, int T,
    long sB, long sC, long sT, long sH, int Hin, int Win, int Hout, int Wout, const int* __restrict__ hb,
    const int* __restrict__ hk, int hks, const int* __restrict__ vb, const int* __restrict__ vk, int vks, int TH, int RB,
    int WP, int raw_bytes, int tiles, float m0, float m1, float m2, float d0, float d1, float d2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* raw = smem;
  unsigned char* hbuf = smem + raw_bytes;
  const int tid = threadIdx.x;
  const int frame = blockIdx.x / tiles, tile = blockIdx.x - frame * tiles;
  const int y0 = tile * TH, y1 = min(Hout, y0 + TH);
  const int r0 = vb[2 * y0], r1 = vb[2 * (y1 - 1)] + vb[2 * (y1 - 1) + 1];      // input rows [r0, r1) feed this tile
  const long rowbytes = (long)Win * 3;
  const long fbase = (long)frame * Hin * rowbytes;

  for (int rb = r0; rb < r1; rb += RB) {
    const int nb = min(RB, r1 - rb);
    const long g0 = fbase + (long)rb * rowbytes;
    const int mis = (int)(g0 & 3);
    const long a0 = g0 - mis;
    const int ndw = (int)((mis + nb * rowbytes + 3) >> 2);
    for (int i = tid; i < ndw; i += 256) reinterpret_cast<unsigned*>(raw)[i] = load_dword_in(frames, a0 + 4L * i, total_bytes);
    __syncthreads();
    for (int it = tid; it < nb * Wout; it += 256) {
      const int row = it / Wout, x = it - row * Wout;
      const int xmin = hb[2 * x], n = hb[2 * x + 1];
      const int* k = hk + (long)x * hks;
      const unsigned char* p = raw + mis + row * rowbytes + xmin * 3;
      int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
      for (int i = 0; i < n; ++i) {
        const int w = k[i];
        s0 += p[3 * i] * w; s1 += p[3 * i + 1] * w; s2 += p[3 * i + 2] * w;
      }
      unsigned char* o = hbuf + (long)(rb - r0 + row) * 3 * WP + x;
      o[0] = (unsigned char)clip8(s0);
      o[WP] = (unsigned char)clip8(s1);
      o[2 * WP] = (unsigned char)clip8(s2);
    }
    __syncthreads();
  }

  const int slot = slots[frame];
  const int b = slot / T, t = slot - b * T;
  float* obase = out + b * sB + t * sT;
  const int ng = WP >> 2;
  const unsigned* h32 = reinterpret_cast<const unsigned*>(hbuf);
  for (int it = tid; it < (y1 - y0) * 3 * ng; it += 256) {
    const int g = it % ng, yc = it / ng;
    const int c = yc % 3, y = y0 + yc / 3;
    const int ymin = vb[2 * y], n = vb[2 * y + 1];
    const int* k = vk + (long)y * vks;
    const unsigned* p = h32 + ((long)(ymin - r0) * 3 + c) * ng + g;
    int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21, s3 = 1 << 21;
    for (int i = 0; i < n; ++i) {
      const int w = k[i];
      const unsigned d = p[(long)i * 3 * ng];
      s0 += (int)(d & 255u) * w; s1 += (int)((d >> 8) & 255u) * w; s2 += (int)((d >> 16) & 255u) * w; s3 += (int)(d >> 24) * w;
    }
    const float m = c == 0 ? m0 : (c == 1 ? m1 : m2), dd = c == 0 ? d0 : (c == 1 ? d1 : d2);
    float4 v;                                        // ToTensor then Normalize, in that order and with true divisions
    v.x = ((float)clip8(s0) / 255.f - m) / dd;
    v.y = ((float)clip8(s1) / 255.f - m) / dd;
    v.z = ((float)clip8(s2) / 255.f - m) / dd;
    v.w = ((float)clip8(s3) / 255.f - m) / dd;
    float* o = obase + c * sC + y * sH + 4 * g;
    if (VEC) {
      *reinterpret_cast<float4*>(o) = v;
    } else {
      const int x = 4 * g;
      if (x < Wout) o[0] = v.x;
      if (x + 1 < Wout) o[1] = v.y;
      if (x + 2 < Wout) o[2] = v.z;
      if (x + 3 < Wout) o[3] = v.w;
    }
  }
}

}  // namespace mspi

extern "C" int mspi_clip_resize_plan(const int32_t* vb_host, int32_t Hin, int32_t Win, int32_t Hout, int32_t Wout, int32_t vks,
                                     int32_t* plan4) {
  MSPI_REQUIRE(vb_host && plan4, "mspi_clip_resize_plan: null argument");
  MSPI_REQUIRE(Hin > 0 && Win > 0 && Hout > 0 && Wout > 0 && vks > 0, "mspi_clip_resize_plan: bad extent");
  MSPI_REQUIRE(check_bounds(vb_host, Hout, Hin, vks), "mspi_clip_resize_plan: the vertical bounds table does not lie inside %d rows", Hin);
  ClipPlan p;
  MSPI_REQUIRE(plan_clip(vb_host, Hin, Win, Hout, Wout, &p),
               "mspi_clip_resize_plan: no tile of %d x %d -> %d x %d fits the LDS budget (use mspi_resize_norm_fwd per frame)", Hin, Win,
               Hout, Wout);
  plan4[0] = p.TH; plan4[1] = p.R; plan4[2] = p.RB; plan4[3] = (int32_t)p.lds_bytes;
  return MSPI_OK;
}

extern "C" int mspi_clip_resize_norm_fwd(const unsigned char* frames, int32_t N, int32_t Hin, int32_t Win, const int32_t* slots,
                                         const int32_t* slots_host, float* out, int32_t B, int32_t T, int64_t sB, int64_t sC,
                                         int64_t sT, int64_t sH, int32_t Hout, int32_t Wout, const int32_t* hb,
                                         const int32_t* hb_host, const int32_t* hk, int32_t hks, const int32_t* vb,
                                         const int32_t* vb_host, const int32_t* vk, int32_t vks, const float* mean3_host,
                                         const float* std3_host, mspi_stream_t stream) {
  MSPI_REQUIRE(frames && slots && slots_host && out && hb && hb_host && hk && vb && vb_host && vk && mean3_host && std3_host,
               "mspi_clip_resize_norm_fwd: null argument");
  MSPI_REQUIRE(N > 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0 && B > 0 && T > 0 && hks > 0 && vks > 0,
               "mspi_clip_resize_norm_fwd: bad extent");
  MSPI_REQUIRE((int64_t)B * T < (1LL << 31) && N <= (int64_t)B * T, "mspi_clip_resize_norm_fwd: %d frames for %d x %d slots", N, B, T);
  MSPI_REQUIRE(sH >= Wout && sT >= (int64_t)Hout * sH && sC >= (int64_t)T * sT && sB >= 3 * sC,
               "mspi_clip_resize_norm_fwd: strides (%ld, %ld, %ld, %ld) are smaller than the planes they step over", (long)sB, (long)sC,
               (long)sT, (long)sH);
  MSPI_REQUIRE((reinterpret_cast<uintptr_t>(frames) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0,
               "mspi_clip_resize_norm_fwd: frames and out must be 4-byte aligned");
  MSPI_REQUIRE(check_bounds(hb_host, Wout, Win, hks), "mspi_clip_resize_norm_fwd: the horizontal bounds table does not lie inside %d columns", Win);
  MSPI_REQUIRE(check_bounds(vb_host, Hout, Hin, vks), "mspi_clip_resize_norm_fwd: the vertical bounds table does not lie inside %d rows", Hin);
  {                               // the host copy of the slot table is what makes the destinations checkable before launch
    const int64_t ns = (int64_t)B * T;
    uint8_t* seen = (uint8_t*)calloc((size_t)ns, 1);
    MSPI_REQUIRE(seen, "mspi_clip_resize_norm_fwd: out of host memory");
    int bad = -1, dup = -1;
    for (int i = 0; i < N && bad < 0 && dup < 0; ++i) {
      const int64_t s = slots_host[i];
      if (s < 0 || s >= ns) bad = i;
      else if (seen[s]) dup = i;
      else seen[s] = 1;
    }
    free(seen);
    MSPI_REQUIRE(bad < 0, "mspi_clip_resize_norm_fwd: frame %d goes to slot %d outside the %d x %d clip tensor", bad, slots_host[bad], B, T);
    MSPI_REQUIRE(dup < 0, "mspi_clip_resize_norm_fwd: slot %d is written twice (frame %d)", slots_host[dup], dup);
  }
  ClipPlan p;
  MSPI_REQUIRE(plan_clip(vb_host, Hin, Win, Hout, Wout, &p),
               "mspi_clip_resize_norm_fwd: no tile of %d x %d -> %d x %d fits the LDS budget (use mspi_resize_norm_fwd per frame)", Hin,
               Win, Hout, Wout);
  const long tiles = ((long)Hout + p.TH - 1) / p.TH;
  MSPI_REQUIRE(tiles * N < (1L << 31), "mspi_clip_resize_norm_fwd: %d frames x %ld tiles exceed the grid", N, tiles);
  const long total = (long)N * Hin * Win * 3;
  const bool vec = Wout % 4 == 0 && sH % 4 == 0 && sT % 4 == 0 && sC % 4 == 0 && sB % 4 == 0 && aligned16(out);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(tiles * N)), block(256);
#define MSPI_CLIP_LAUNCH(V)                                                                                                       \
  hipLaunchKernelGGL(clip_resize_norm_kernel<V>, grid, block, (size_t)p.lds_bytes, s, frames, total, slots, out, T, (long)sB,    \
                     (long)sC, (long)sT, (long)sH, Hin, Win, Hout, Wout, hb, hk, hks, vb, vk, vks, p.TH, p.RB, p.WP,             \
                     (int)p.raw_bytes, (int)tiles, mean3_host[0], mean3_host[1], mean3_host[2], std3_host[0], std3_host[1],      \
                     std3_host[2])
  if (vec) MSPI_CLIP_LAUNCH(true); else MSPI_CLIP_LAUNCH(false);
#undef MSPI_CLIP_LAUNCH
  return check_launch("mspi_clip_resize_norm_fwd");
}
