// FID's feature extractor: the FID variant of Inception-v3 up to pool3 (torch-fidelity's
// FeatureExtractorInceptionV3 / pytorch-fid's pt_inception-2015-12-05), and the fp64 feature statistics behind it.
//
//   front end   uint8 (or fp32 in [0, 1], quantised) NCHW images -> TF1-legacy bilinear resize to 299 x 299 in fp32 with exactly
//               the written roundings, (v - 128) / 128 -> bf16 NHWC of FID_IN_C channels (three real ones, the others zero)
//   tower       94 convolutions (BatchNorm folded on the host) as ONE implicit-GEMM kernel, conv_relu_slice_kernel: any of the
//               network's (kh, kw, stride, pad) forms, reads a channel slice, writes max(acc + bias, 0) into a channel slice of a
//               wider NHWC buffer -- the concatenation at the end of every block is never a copy.  3x3 pools write slices too.
//   pool3       Mixed_7c is written in fp32; the mean over its 8 x 8 pixels in pixel order -> [images][2048] fp32
//   statistics  sum[d] += sum_i f_i, cov_sum[d][d] += sum_i f_i f_i^T in fp64 on v_mfma_f64_16x16x4_f64, the images as K
//
// The convolution keeps no operand in LDS: with A = weights and B = pixels, a lane's MFMA fragment is eight consecutive K
// elements of ONE weight row / ONE pixel, i.e. one 16-byte load of the packed weights / of the NHWC map, and the accumulator
// holds four consecutive output channels of one pixel (one 8- or 16-byte store).  K runs taps-major, channels inside, always in
// the same order and never split, and a pixel's sum reads only that pixel's window: an image's features do not depend on the
// batch it sits in.  The layer table is NOT here: mvd_amd/packing.py INCEPTION_FID_LAYERS is compiled into the program of
// mvd_fid_create, which this file interprets.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "host_util.h"

typedef __attribute__((ext_vector_type(4))) double f64x4;

namespace {

constexpr int FID_SIZE = 299;      // the tower's input
constexpr int FID_IN_C = 16;       // channels of the resized map: r, g, b and 13 zeros (the convolution reads multiples of 16)

// ---------------------------------------------------------------- implicit-GEMM convolution + bias + ReLU into a channel slice
// Workgroup: 64 output pixels x 64 output channels, wave v the pixels 16 v ... 16 v + 15 against four 16-channel tiles (fewer at
// the end of cout: a multiple of 16).  Packed weights [cout][kh kw][cin_pad], cin_pad = cin rounded up to 32, the padding zeros;
// a lane's 16-byte chunk of a 32-wide K step lies inside the real channels or is not loaded at all (cin is a multiple of 16).
struct ConvArgs {
  const bf16_t* x; const bf16_t* w; const float* bias; void* out;
  int h, wd, ld_in, cin_off, cin, cin_pad;
  int oh, ow, kh, kw, stride, ph, pw;
  int cout, c_off, ld_out, out_f32;
  long M;
};

__global__ __launch_bounds__(256) void conv_relu_slice_kernel(ConvArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const long row = (long)blockIdx.x * 64 + wave * 16 + r;
  const int n0 = blockIdx.y * 64;
  const int left = (a.cout - n0) >> 4, nt = left < 4 ? left : 4;      // the same for the whole workgroup
  const bool live = row < a.M;
  const long pix = live ? row : 0;
  const int ox = (int)(pix % a.ow);
  const long t0 = pix / a.ow;
  const int oy = (int)(t0 % a.oh);
  const long b = t0 / a.oh;
  const int taps = a.kh * a.kw;
  const size_t Kp = (size_t)taps * a.cin_pad;
  const bf16_t* wrow = a.w + (size_t)(n0 + r) * Kp + 8 * q;
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int ky = 0; ky < a.kh; ++ky) {
    const int iy = oy * a.stride - a.ph + ky;
    for (int kx = 0; kx < a.kw; ++kx) {
      const int ix = ox * a.stride - a.pw + kx;
      const bool ok = live && (unsigned)iy < (unsigned)a.h && (unsigned)ix < (unsigned)a.wd;
      const bf16_t* xp = a.x + (ok ? ((size_t)(b * a.h + iy) * a.wd + ix) * a.ld_in + a.cin_off + 8 * q : 0);
      const bf16_t* wp = wrow + (size_t)(ky * a.kw + kx) * a.cin_pad;
      for (int c = 0; c < a.cin_pad; c += 32) {
        u32x4 xv = {0u, 0u, 0u, 0u};      // a tap outside the image, a row beyond M, the tail of a 32-wide step: exact zeros
        if (ok && c + 8 * q < a.cin) xv = *reinterpret_cast<const u32x4*>(xp + c);
        const bf16x8 xf = __builtin_bit_cast(bf16x8, xv);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (t < nt) {
            const bf16x8 wf = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(wp + (size_t)t * 16 * Kp + c));
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf, acc[t], 0, 0, 0);
          }
        }
      }
    }
  }
  // D[channel 4 q + i of the tile][pixel r]: four consecutive channels of this lane's own pixel
  if (!live) return;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t < nt) {
      const int n = n0 + 16 * t + 4 * q;
      const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bias + n);
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = fmaxf(acc[t][i] + bv[i], 0.f);
      const size_t o = (size_t)row * a.ld_out + a.c_off + n;
      if (a.out_f32) *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.out) + o) = f32x4{v[0], v[1], v[2], v[3]};
      else *reinterpret_cast<u32x2*>(reinterpret_cast<bf16_t*>(a.out) + o) = u32x2{pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
    }
  }
}

int cin_pad_of(int cin) { return (cin + 31) & ~31; }

bool kernel_form_ok(int kh, int kw) {
  return (kh == 1 && kw == 1) || (kh == 3 && kw == 3) || (kh == 5 && kw == 5) || (kh == 1 && kw == 7) || (kh == 7 && kw == 1) || (kh == 1 && kw == 3) ||
         (kh == 3 && kw == 1);
}

int launch_conv(const bf16_t* x, int batch, int h, int w, int ld_in, int cin_off, int cin, const bf16_t* wt, const float* bias, int kh, int kw, int stride,
                int ph, int pw, int cout, void* out, int ld_out, int c_off, int out_f32, hipStream_t s) {
  if (!x || !wt || !bias || !out || batch <= 0 || h <= 0 || w <= 0) { mvd_set_error("conv_relu_slice: null pointer or empty map"); return -1; }
  if (!kernel_form_ok(kh, kw) || (stride != 1 && stride != 2) || ph < 0 || pw < 0 || ph >= kh || pw >= kw) {
    mvd_set_error("conv_relu_slice: kernel %d x %d stride %d pad (%d, %d): 1x1, 3x3, 5x5, 1x7, 7x1, 1x3 or 3x1, stride 1 or 2, pad below the kernel size", kh, kw, stride, ph, pw);
    return -1;
  }
  if (cin <= 0 || cout <= 0 || (cin | cout | c_off | cin_off | ld_in | ld_out) % 16 || cin_off < 0 || c_off < 0 || cin_off + cin > ld_in || c_off + cout > ld_out) {
    mvd_set_error("conv_relu_slice: channels [%d, %d + %d) of %d -> [%d, %d + %d) of %d: all multiples of 16, the slices inside their rows", cin_off, cin_off, cin, ld_in,
                  c_off, c_off, cout, ld_out);
    return -1;
  }
  if (((uintptr_t)x | (uintptr_t)wt | (uintptr_t)bias | (uintptr_t)out) & 15) { mvd_set_error("conv_relu_slice: 16-byte aligned buffers"); return -1; }
  const int oh = (h + 2 * ph - kh) / stride + 1, ow = (w + 2 * pw - kw) / stride + 1;
  if (h + 2 * ph < kh || w + 2 * pw < kw) { mvd_set_error("conv_relu_slice: a %d x %d map has no %d x %d window", h, w, kh, kw); return -1; }
  const long M = (long)batch * oh * ow;
  if (M >= (1L << 31) - 64 || (long)batch * h * w >= (1L << 31)) { mvd_set_error("conv_relu_slice: 2^31 rows or more: split the batch"); return -1; }
  if ((cout + 63) / 64 > 65535) { mvd_set_error("conv_relu_slice: too many output channels"); return -1; }
  ConvArgs a{x, wt, bias, out, h, w, ld_in, cin_off, cin, cin_pad_of(cin), oh, ow, kh, kw, stride, ph, pw, cout, c_off, ld_out, out_f32, M};
  hipLaunchKernelGGL(conv_relu_slice_kernel, dim3((unsigned)((M + 63) / 64), (unsigned)((cout + 63) / 64)), dim3(256), 0, s, a);
  return launch_check("conv_relu_slice");
}

// ---------------------------------------------------------------- 3x3 pools into a channel slice
// mode 0: average, stride 1, pad 1, over the in-image taps only (count_include_pad=False): fp32 sum in tap order, a true division
//         by the count, one rounding; 1: maximum, stride 1, pad 1 (the pad never wins: only in-image taps are read);
//      2: maximum, stride 2, no padding, floor.  One thread per 16-byte chunk (8 channels) of the output.
__global__ __launch_bounds__(256) void pool3x3_slice_kernel(const bf16_t* __restrict__ x, int h, int w, int ld_in, int cin_off, int oh, int ow, int c8, int mode,
                                                            int ld_out, int c_off, long total, bf16_t* __restrict__ y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ch = (int)(i % c8);
  const long pix = i / c8;
  const int ox = (int)(pix % ow);
  const long t = pix / ow;
  const int oy = (int)(t % oh);
  const long b = t / oh;
  const int stride = mode == 2 ? 2 : 1, pad = mode == 2 ? 0 : 1;
  float s[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = mode == 0 ? 0.f : -INFINITY;
  int count = 0;
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = oy * stride - pad + ky;
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = ox * stride - pad + kx;
      if ((unsigned)iy >= (unsigned)h || (unsigned)ix >= (unsigned)w) continue;
      const u32x4 p = *reinterpret_cast<const u32x4*>(x + ((size_t)(b * h + iy) * w + ix) * ld_in + cin_off + 8 * ch);
      ++count;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float lo = bflo(p[j]), hi = bfhi(p[j]);
        if (mode == 0) { s[2 * j] += lo; s[2 * j + 1] += hi; }
        else { s[2 * j] = fmaxf(s[2 * j], lo); s[2 * j + 1] = fmaxf(s[2 * j + 1], hi); }
      }
    }
  }
  if (mode == 0) {
    const float n = (float)count;
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = s[j] / n;
  }
  *reinterpret_cast<u32x4*>(y + (size_t)pix * ld_out + c_off + 8 * ch) = u32x4{pack2bf(s[0], s[1]), pack2bf(s[2], s[3]), pack2bf(s[4], s[5]), pack2bf(s[6], s[7])};
}

int launch_pool(const bf16_t* x, int batch, int h, int w, int ld_in, int cin_off, int c, int mode, bf16_t* y, int ld_out, int c_off, hipStream_t s) {
  if (!x || !y || batch <= 0 || h <= 0 || w <= 0 || mode < 0 || mode > 2) { mvd_set_error("pool3x3_slice: bad argument (mode 0 avg, 1 max, 2 max stride 2)"); return -1; }
  if (c <= 0 || (c | cin_off | c_off | ld_in | ld_out) % 8 || cin_off < 0 || c_off < 0 || cin_off + c > ld_in || c_off + c > ld_out) {
    mvd_set_error("pool3x3_slice: channels [%d, %d + %d) of %d -> [%d, ...) of %d: multiples of 8, the slices inside their rows", cin_off, cin_off, c, ld_in, c_off, ld_out);
    return -1;
  }
  if (((uintptr_t)x | (uintptr_t)y) & 15) { mvd_set_error("pool3x3_slice: 16-byte aligned buffers"); return -1; }
  if (mode == 2 && (h < 3 || w < 3)) { mvd_set_error("pool3x3_slice: a %d x %d map has no 3 x 3 window", h, w); return -1; }
  const int oh = mode == 2 ? (h - 3) / 2 + 1 : h, ow = mode == 2 ? (w - 3) / 2 + 1 : w;
  const long total = (long)batch * oh * ow * (c / 8);
  if (blocks_of(total) >= (1L << 31) || (long)batch * h * w >= (1L << 31)) { mvd_set_error("pool3x3_slice: too many elements for one launch"); return -1; }
  hipLaunchKernelGGL(pool3x3_slice_kernel, dim3((unsigned)blocks_of(total)), dim3(256), 0, s, x, h, w, ld_in, cin_off, oh, ow, c / 8, mode, ld_out, c_off, total, y);
  return launch_check("pool3x3_slice");
}

// ---------------------------------------------------------------- front end: quantise, TF1-legacy bilinear resize, (v - 128) / 128
// One thread per output pixel.  src = dst * scale with scale = float32(in / out) from the host, i0 = floor(src),
// i1 = min(i0 + 1, in - 1); top = tl + (tr - tl) wx, bot likewise, out = top + (bot - top) wy: compiled without contraction, so
// every product and sum is rounded as written.  fp32 input: trunc(clamp(x, 0, 1) * 255), torchmetrics' normalize=True.
template <bool F32>
__global__ __launch_bounds__(256) void resize_tf1_kernel(const void* __restrict__ src, int h, int w, float scale_h, float scale_w, long total,
                                                         bf16_t* __restrict__ out) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ox = (int)(i % FID_SIZE);
  const long t = i / FID_SIZE;
  const int oy = (int)(t % FID_SIZE);
  const long b = t / FID_SIZE;
  const float sy = (float)oy * scale_h, sx = (float)ox * scale_w;
  const float fy = floorf(sy), fx = floorf(sx);
  const float wy = sy - fy, wx = sx - fx;
  int y0 = (int)fy, x0 = (int)fx;
  y0 = y0 < h - 1 ? y0 : h - 1; x0 = x0 < w - 1 ? x0 : w - 1;
  const int y1 = y0 + 1 < h ? y0 + 1 : h - 1, x1 = x0 + 1 < w ? x0 + 1 : w - 1;
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const size_t plane = ((size_t)b * 3 + c) * h;
    float p[4];
    const size_t idx[4] = {(plane + y0) * w + x0, (plane + y0) * w + x1, (plane + y1) * w + x0, (plane + y1) * w + x1};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (F32) {
        float f = reinterpret_cast<const float*>(src)[idx[k]];
        f = fminf(fmaxf(f, 0.f), 1.f);
        p[k] = truncf(f * 255.f);
      } else {
        p[k] = (float)reinterpret_cast<const unsigned char*>(src)[idx[k]];
      }
    }
    const float top = p[0] + (p[1] - p[0]) * wx;
    const float bot = p[2] + (p[3] - p[2]) * wx;
    const float val = top + (bot - top) * wy;
    v[c] = (val - 128.f) * 0.0078125f;
  }
  u32x4* o = reinterpret_cast<u32x4*>(out + (size_t)i * FID_IN_C);
  o[0] = u32x4{pack2bf(v[0], v[1]), pack2bf(v[2], 0.f), 0u, 0u};
  o[1] = u32x4{0u, 0u, 0u, 0u};
}

int launch_resize(const void* src, int dtype, int batch, int h, int w, bf16_t* out, hipStream_t s) {
  if (!src || !out || batch <= 0 || h <= 0 || w <= 0 || h > 32768 || w > 32768 || (dtype != 0 && dtype != 1)) {
    mvd_set_error("resize_tf1: bad argument (dtype 0: uint8, 1: fp32 in [0, 1]; h, w in [1, 32768])"); return -1;
  }
  if (((uintptr_t)out & 15) || (dtype == 1 && ((uintptr_t)src & 3))) { mvd_set_error("resize_tf1: output 16-byte aligned, fp32 input 4-byte aligned"); return -1; }
  const long total = (long)batch * FID_SIZE * FID_SIZE;
  if (total >= (1L << 31) || (long)batch * 3 * h * w >= (1L << 40)) { mvd_set_error("resize_tf1: too many images for one launch"); return -1; }
  const float sh = (float)((double)h / (double)FID_SIZE), sw = (float)((double)w / (double)FID_SIZE);
  if (dtype == 1) hipLaunchKernelGGL(resize_tf1_kernel<true>, dim3((unsigned)blocks_of(total)), dim3(256), 0, s, src, h, w, sh, sw, total, out);
  else hipLaunchKernelGGL(resize_tf1_kernel<false>, dim3((unsigned)blocks_of(total)), dim3(256), 0, s, src, h, w, sh, sw, total, out);
  return launch_check("resize_tf1");
}

// ---------------------------------------------------------------- the mean over the pixels of an fp32 NHWC map, in pixel order
__global__ __launch_bounds__(256) void global_mean_kernel(const float* __restrict__ x, int pixels, int c, long total, float* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long b = i / c;
  const int ch = (int)(i % c);
  const float* p = x + (size_t)b * pixels * c + ch;
  float s = 0.f;
  for (int k = 0; k < pixels; ++k) s += p[(size_t)k * c];
  out[i] = s / (float)pixels;
}

int launch_global_mean(const float* x, int batch, int pixels, int c, float* out, hipStream_t s) {
  if (!x || !out || batch <= 0 || pixels <= 0 || c <= 0) { mvd_set_error("global_mean: bad argument"); return -1; }
  const long total = (long)batch * c;
  if (blocks_of(total) >= (1L << 31)) { mvd_set_error("global_mean: too many elements for one launch"); return -1; }
  hipLaunchKernelGGL(global_mean_kernel, dim3((unsigned)blocks_of(total)), dim3(256), 0, s, x, pixels, c, total, out);
  return launch_check("global_mean");
}

// ---------------------------------------------------------------- feature statistics in fp64
// cov_sum[a][b] += sum_i f[i][a] f[i][b]: workgroup = a 64 x 64 tile, wave = a 32 x 32 quadrant = 2 x 2 tiles of
// v_mfma_f64_16x16x4_f64 with four images per instruction (K), the last step zero padded.  A: lane l holds f[k = l >> 4]
// [a = l & 15], B the same with b; D: col = l & 15, row = (l >> 4) + 4 reg (the f64 form's own map).  The images run in order and
// one lane owns an element: no atomics.  sum[d] += sum_i f[i][d] is a kernel of its own, one thread per column.
__global__ __launch_bounds__(256) void feature_cov_kernel(const float* __restrict__ f, int n, int d, double* __restrict__ cov) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int a0 = blockIdx.y * 64 + (wave >> 1) * 32, b0 = blockIdx.x * 64 + (wave & 1) * 32;
  f64x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < n; k0 += 4) {
    const int img = k0 + q;
    const bool live = img < n;
    const float* row = f + (size_t)(live ? img : 0) * d;
    double av[2], bv[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      av[t] = live ? (double)row[a0 + 16 * t + r] : 0.0;
      bv[t] = live ? (double)row[b0 + 16 * t + r] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], bv[j], acc[i][j], 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const size_t o = (size_t)(a0 + 16 * i + q + 4 * g) * d + b0 + 16 * j + r;
        cov[o] += acc[i][j][g];
      }
}

__global__ __launch_bounds__(256) void feature_sum_kernel(const float* __restrict__ f, int n, int d, double* __restrict__ sum) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= d) return;
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += (double)f[(size_t)i * d + c];
  sum[c] += s;
}

int launch_feature_stats(const float* f, int n, int d, double* sum, double* cov, hipStream_t s) {
  if (!f || !sum || !cov || n <= 0 || d <= 0 || d % 64 || d > 64 * 65535) { mvd_set_error("feature_stats: bad argument (n >= 1, d a multiple of 64)"); return -1; }
  if (((uintptr_t)f & 3) || (((uintptr_t)sum | (uintptr_t)cov) & 7)) { mvd_set_error("feature_stats: misaligned buffer"); return -1; }
  hipLaunchKernelGGL(feature_sum_kernel, dim3((unsigned)blocks_of(d)), dim3(256), 0, s, f, n, d, sum);
  CHECK(launch_check("feature_stats (sum)"));
  hipLaunchKernelGGL(feature_cov_kernel, dim3(d / 64, d / 64), dim3(256), 0, s, f, n, d, cov);
  return launch_check("feature_stats (cov_sum)");
}

// ---------------------------------------------------------------- the program of mvd_fid_create
constexpr int OP_INTS = 13;
enum { OP_CONV = 0, OP_POOL = 1 };
struct Op { int kind, src, dst, c_off, cin, cout, kh, kw, stride, ph, pw, conv, mode; };
struct Buf { int channels, f32; };

}  // namespace

struct mvd_fid : ModuleBase {
  std::vector<Op> ops;
  std::vector<Buf> bufs;
  std::vector<std::string> names;      // of the convolutions: weight slots "<name>.weight" / "<name>.bias"
  int final_buf = 0, max_pass = 8;
};

namespace {

int out_size(const Op& o, int in, bool height) {
  if (o.kind == OP_POOL) return o.mode == 2 ? (in - 3) / 2 + 1 : in;
  const int k = height ? o.kh : o.kw, p = height ? o.ph : o.pw;
  return (in + 2 * p - k) / o.stride + 1;
}

// sizes of every buffer for a FID_SIZE x FID_SIZE input; < 0 when the program is inconsistent
int geometry(const mvd_fid* v, std::vector<int>& hs, std::vector<int>& ws) {
  hs.assign(v->bufs.size(), 0); ws.assign(v->bufs.size(), 0);
  hs[0] = ws[0] = FID_SIZE;
  for (size_t i = 0; i < v->ops.size(); ++i) {
    const Op& o = v->ops[i];
    if (!hs[o.src]) { mvd_set_error("fid: op %zu reads buffer %d before anything wrote it", i, o.src); return -1; }
    const int oh = out_size(o, hs[o.src], true), ow = out_size(o, ws[o.src], false);
    if (oh < 1 || ow < 1) { mvd_set_error("fid: op %zu has no output", i); return -1; }
    if (hs[o.dst] && (hs[o.dst] != oh || ws[o.dst] != ow)) { mvd_set_error("fid: op %zu writes %d x %d into buffer %d of %d x %d", i, oh, ow, o.dst, hs[o.dst], ws[o.dst]); return -1; }
    hs[o.dst] = oh; ws[o.dst] = ow;
  }
  if (!hs[v->final_buf]) { mvd_set_error("fid: the feature buffer is never written"); return -1; }
  return 0;
}

int check_weights(mvd_fid* v, std::vector<const bf16_t*>* wt, std::vector<const float*>* bias) {
  int err = 0;
  for (const Op& o : v->ops) {
    if (o.kind != OP_CONV) continue;
    const std::string& n = v->names[o.conv];
    const void* pw = v->w.find(n + ".weight", 1, (int64_t)o.cout * o.kh * o.kw * cin_pad_of(o.cin), &err, "fid: ");
    if (err) return err;
    const void* pb = v->w.find(n + ".bias", 0, o.cout, &err, "fid: ");
    if (err) return err;
    if (wt) { (*wt)[o.conv] = (const bf16_t*)pw; (*bias)[o.conv] = (const float*)pb; }
  }
  return 0;
}

// one pass over `np` images: every buffer of the program lives in the arena for the whole pass (about 25 MiB an image), so the
// bytes of a pass grow with every image added.  dry: sizes only.
int run_pass(mvd_fid* v, bool dry, const void* images, int dtype, int np, int h, int w, float* feat_out, hipStream_t s) {
  std::vector<int> hs, ws;
  CHECK(geometry(v, hs, ws));
  Arena& ar = v->ar;
  std::vector<void*> p(v->bufs.size());
  for (size_t i = 0; i < v->bufs.size(); ++i) p[i] = ar.alloc((size_t)np * hs[i] * ws[i] * v->bufs[i].channels * (v->bufs[i].f32 ? 4 : 2));
  if (ar.overflow()) { mvd_set_error("fid: workspace too small for a pass of %d images", np); return -4; }
  if (dry) return 0;
  std::vector<const bf16_t*> wt(v->names.size()); std::vector<const float*> bias(v->names.size());
  CHECK(check_weights(v, &wt, &bias));
  CHECK(launch_resize(images, dtype, np, h, w, (bf16_t*)p[0], s));
  for (const Op& o : v->ops) {
    const Buf& src = v->bufs[o.src]; const Buf& dst = v->bufs[o.dst];
    if (o.kind == OP_CONV)
      CHECK(launch_conv((const bf16_t*)p[o.src], np, hs[o.src], ws[o.src], src.channels, 0, o.cin, wt[o.conv], bias[o.conv], o.kh, o.kw, o.stride, o.ph, o.pw, o.cout,
                        p[o.dst], dst.channels, o.c_off, dst.f32, s));
    else
      CHECK(launch_pool((const bf16_t*)p[o.src], np, hs[o.src], ws[o.src], src.channels, 0, o.cin, o.mode, (bf16_t*)p[o.dst], dst.channels, o.c_off, s));
  }
  const int fb = v->final_buf;
  return launch_global_mean((const float*)p[fb], np, hs[fb] * ws[fb], v->bufs[fb].channels, feat_out, s);
}

int pass_bytes(mvd_fid* v, int np, size_t* out) {
  v->ar.reset(true);
  CHECK(run_pass(v, true, nullptr, 0, np, 0, 0, nullptr, nullptr));
  *out = align256(v->ar.high);
  return 0;
}

int feature_dim(const mvd_fid* v) { return v->bufs[v->final_buf].channels; }
size_t feat_region(const mvd_fid* v, int images) { return align256((size_t)images * feature_dim(v) * sizeof(float)); }

int check_call(const char* who, mvd_fid* v, const void* images, int dtype, int n, int h, int w) {
  if (!v || !images) { mvd_set_error("%s: null argument", who); return -1; }
  if ((dtype != 0 && dtype != 1) || n <= 0 || n > (1 << 24) || h <= 0 || w <= 0 || h > 32768 || w > 32768) {
    mvd_set_error("%s: bad argument (dtype 0 uint8 / 1 fp32, %d images of %d x %d: h, w in [1, 32768])", who, n, h, w); return -1;
  }
  return 0;
}

// the passes of a call: every size that will run is sized first, and nothing is launched unless all of them fit behind `head` bytes
int run_features(const char* who, mvd_fid* v, size_t head, const void* images, int dtype, int n, int h, int w, float* feat_out, hipStream_t s) {
  CHECK(check_weights(v, nullptr, nullptr));
  if (!v->ws_ptr) { mvd_set_error("%s: workspace not bound", who); return -1; }
  const int P = v->max_pass;
  size_t need = 0, tail = 0;
  CHECK(pass_bytes(v, n < P ? n : P, &need));
  if (n > P && n % P) CHECK(pass_bytes(v, n % P, &tail));
  if (tail > need) need = tail;
  if (head + need > (size_t)v->ws_bytes) { mvd_set_error("%s: workspace too small: need %zu bytes, bound %lld", who, head + need, (long long)v->ws_bytes); return -4; }
  const size_t img = (size_t)3 * h * w * (dtype ? 4 : 1);
  const int D = feature_dim(v);
  for (int p0 = 0; p0 < n; p0 += P) {
    const int np = n - p0 < P ? n - p0 : P;
    module_bind_arena(*v, head);
    CHECK(run_pass(v, false, reinterpret_cast<const char*>(images) + p0 * img, dtype, np, h, w, feat_out + (size_t)p0 * D, s));
  }
  return 0;
}

}  // namespace

extern "C" {

int mvd_fid_create(const int* program, int n_ops, const int* buffers, int n_buffers, const char* const* conv_names, int n_convs, int final_buffer,
                   int max_images_per_pass, mvd_fid_t** out) {
  if (!program || !buffers || !conv_names || !out || n_ops <= 0 || n_ops > 4096 || n_buffers < 2 || n_buffers > 4096 || n_convs <= 0 || n_convs > n_ops ||
      final_buffer <= 0 || final_buffer >= n_buffers || max_images_per_pass < 0 || max_images_per_pass > 4096) {
    mvd_set_error("fid_create: bad argument"); return -1;
  }
  mvd_fid* v = new mvd_fid();
  v->max_pass = max_images_per_pass ? max_images_per_pass : 8;
  v->final_buf = final_buffer;
  for (int i = 0; i < n_buffers; ++i) v->bufs.push_back(Buf{buffers[2 * i], buffers[2 * i + 1]});
  for (int i = 0; i < n_convs; ++i) v->names.push_back(conv_names[i] ? conv_names[i] : "");
  int bad = -1, convs = 0;
  for (int i = 0; i < n_ops && bad < 0; ++i) {
    const int* r = program + (size_t)i * OP_INTS;
    const Op o{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10], r[11], r[12]};
    if ((o.kind != OP_CONV && o.kind != OP_POOL) || o.src < 0 || o.src >= n_buffers || o.dst <= 0 || o.dst >= n_buffers || o.src == o.dst) { bad = i; break; }
    const Buf& s = v->bufs[o.src]; const Buf& d = v->bufs[o.dst];
    if (s.f32 || o.cin != s.channels || o.cin <= 0 || o.cin % 16 || o.c_off < 0 || o.c_off % 16 || d.channels % 16) bad = i;
    if (o.kind == OP_CONV) {
      if (o.conv != convs++ || o.conv >= n_convs || o.cout <= 0 || o.cout % 16 || o.c_off + o.cout > d.channels || !kernel_form_ok(o.kh, o.kw) ||
          (o.stride != 1 && o.stride != 2) || o.ph < 0 || o.pw < 0 || o.ph >= o.kh || o.pw >= o.kw) bad = i;
    } else {
      if (o.mode < 0 || o.mode > 2 || d.f32 || o.c_off + o.cin > d.channels) bad = i;
    }
    v->ops.push_back(o);
  }
  if (bad < 0 && (convs != n_convs || v->bufs[0].channels != FID_IN_C || v->bufs[0].f32 || !v->bufs[final_buffer].f32 || v->bufs[final_buffer].channels % 64)) bad = n_ops;
  if (bad >= 0) { mvd_set_error("fid_create: op %d of the program is not one this schedule runs (or the buffers / names do not fit it)", bad); delete v; return -1; }
  std::vector<int> hs, ws;
  if (int r = geometry(v, hs, ws)) { delete v; return r; }
  *out = v;
  return 0;
}
int mvd_fid_destroy(mvd_fid_t* v) { delete v; return 0; }

int mvd_fid_set_weight(mvd_fid_t* v, const char* slot, const void* ptr, int64_t numel, int dtype) {
  return module_set_weight(v, "fid", slot, ptr, numel, dtype);
}

int mvd_fid_feature_dim(mvd_fid_t* v) {
  if (!v) { mvd_set_error("fid_feature_dim: null handle"); return -1; }
  return feature_dim(v);
}

int64_t mvd_fid_workspace_bytes(mvd_fid_t* v, int images) {
  if (!v || images <= 0 || images > (1 << 24)) { mvd_set_error("fid_workspace_bytes: bad argument"); return -1; }
  size_t need = 0;
  if (int r = pass_bytes(v, images < v->max_pass ? images : v->max_pass, &need)) return r;
  return (int64_t)(feat_region(v, images) + need);
}

int mvd_fid_bind_workspace(mvd_fid_t* v, void* ws, int64_t bytes) {
  return module_bind_workspace(v, "fid", ws, bytes, 0);
}

int mvd_fid_features(mvd_fid_t* v, const void* images, int dtype, int n, int h, int w, float* feat_out, void* stream) {
  CHECK(check_call("fid_features", v, images, dtype, n, h, w));
  if (!feat_out || ((uintptr_t)feat_out & 3)) { mvd_set_error("fid_features: null or misaligned output"); return -1; }
  return run_features("fid_features", v, 0, images, dtype, n, h, w, feat_out, (hipStream_t)stream);
}

int mvd_fid_update(mvd_fid_t* v, const void* images, int dtype, int n, int h, int w, double* sum, double* cov_sum, void* stream) {
  CHECK(check_call("fid_update", v, images, dtype, n, h, w));
  if (!sum || !cov_sum || (((uintptr_t)sum | (uintptr_t)cov_sum) & 7)) { mvd_set_error("fid_update: null or misaligned state"); return -1; }
  if (!v->ws_ptr) { mvd_set_error("fid_update: workspace not bound"); return -1; }
  const size_t head = feat_region(v, n);
  if (head >= (size_t)v->ws_bytes) { mvd_set_error("fid_update: workspace too small for the features of %d images", n); return -4; }
  float* feats = reinterpret_cast<float*>(v->ws_ptr);
  CHECK(run_features("fid_update", v, head, images, dtype, n, h, w, feats, (hipStream_t)stream));
  return launch_feature_stats(feats, n, feature_dim(v), sum, cov_sum, (hipStream_t)stream);
}

int mvd_op_conv_relu_slice(const void* x, int batch, int h, int w, int ld_in, int cin_off, int cin, const void* w_packed, const float* bias, int kh, int kw,
                           int stride, int pad_h, int pad_w, int cout, void* out, int ld_out, int c_off, int out_f32, void* stream) {
  return launch_conv((const bf16_t*)x, batch, h, w, ld_in, cin_off, cin, (const bf16_t*)w_packed, bias, kh, kw, stride, pad_h, pad_w, cout, out, ld_out, c_off,
                     out_f32 ? 1 : 0, (hipStream_t)stream);
}

int mvd_op_pool3x3_slice(const void* x, int batch, int h, int w, int ld_in, int cin_off, int c, int mode, void* out, int ld_out, int c_off, void* stream) {
  return launch_pool((const bf16_t*)x, batch, h, w, ld_in, cin_off, c, mode, (bf16_t*)out, ld_out, c_off, (hipStream_t)stream);
}

int mvd_op_resize_tf1(const void* src, int dtype, int batch, int h, int w, void* out, void* stream) {
  return launch_resize(src, dtype, batch, h, w, (bf16_t*)out, (hipStream_t)stream);
}

int mvd_op_global_mean(const float* x, int batch, int pixels, int c, float* out, void* stream) {
  return launch_global_mean(x, batch, pixels, c, out, (hipStream_t)stream);
}

int mvd_op_feature_stats(const float* f, int n, int d, double* sum, double* cov_sum, void* stream) {
  return launch_feature_stats(f, n, d, sum, cov_sum, (hipStream_t)stream);
}

}  // extern "C"
