// LPIPS v0.1 with the AlexNet and VGG-16 backbones: what the reference's val.py:87 builds as
// lpips.LPIPS(net="alex"), on this project's kernels.
//
//   front end   fp32 NCHW images in [-1, 1] -> (x - shift) / scale as ONE affine map per channel, applied by
//               im2col_patch_image_kernel while it writes the K = 363 -> 384 rows of the 11x11 stride-4 pad-2 convolution (taps
//               outside the image are zeros, not the shift: a padded convolution of the SCALED image) -> conv1 as a K = 384 dense
//               GEMM with ReLU
//   tower       3x3 stride-2 max-pool, the 5x5 pad-2 convolution as im2col rows of K = 1600 and a dense GEMM with ReLU, the
//               pool again, three 3x3 pad-1 convolutions on the implicit-GEMM tiles with the ReLU epilogue; bf16 NHWC maps
//   head        ONE launch over all five taps: per pixel both channel norms, then sum_c w_c (a_c / na - b_c / nb)^2 in fp32;
//               per-(layer, chunk, pair) sums in fp64, fixed order; a one-workgroup finish: mean over pixels per layer, sum
//               over layers, mean over pairs
//
// Launches per pass: 2 im2col + 5 GEMMs (+ a reduce pass where K is split) + 2 pools + 2 for the head.  x and y of a pair are
// rows of the same launches, so identical inputs give identical taps and a distance of exactly 0.  No float atomics.
// The VGG variant is a composition on the host side of mvd_amd/lpips.py: mvd_vgg_features with its taps, then mvd_op_lpips_head.
#include <stdio.h>
#include <string.h>

#include <string>

#include "host_util.h"

namespace {

// ---------------------------------------------------------------- im2col, from the fp32 NCHW image: 11x11, stride 4, pad 2, 3 channels
// One thread per 16-byte chunk (8 columns) of a row; column (ky * 11 + kx) * 3 + c, zero padded 363 -> 384.  Images b < nx come
// from x, the others from y: both halves of a pair in one launch.  The affine map touches in-image taps only.
constexpr int P1_K = 11, P1_STRIDE = 4, P1_PAD = 2, P1_COLS = 384, P1_REAL = P1_K * P1_K * 3;
__global__ __launch_bounds__(256) void im2col_patch_image_kernel(const float* __restrict__ x, int nx, const float* __restrict__ y, int h, int w, int oh,
                                                                 int ow, float sc0, float sc1, float sc2, float sh0, float sh1, float sh2, long total,
                                                                 bf16_t* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int q = (int)(i % (P1_COLS / 8));
  const long row = i / (P1_COLS / 8);
  const int ox = (int)(row % ow);
  const long t = row / ow;
  const int oy = (int)(t % oh);
  const int b = (int)(t / oh);
  const float* img = b < nx ? x + (size_t)b * 3 * h * w : y + (size_t)(b - nx) * 3 * h * w;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int col = q * 8 + j;
    const int tap = col / 3, c = col - 3 * tap;
    const int ky = tap / P1_K, kx = tap - P1_K * ky;
    const int iy = oy * P1_STRIDE - P1_PAD + ky, ix = ox * P1_STRIDE - P1_PAD + kx;
    v[j] = 0.f;
    if (col < P1_REAL && (unsigned)iy < (unsigned)h && (unsigned)ix < (unsigned)w) {
      const float sc = c == 0 ? sc0 : c == 1 ? sc1 : sc2, sh = c == 0 ? sh0 : c == 1 ? sh1 : sh2;
      v[j] = fmaf(img[((size_t)c * h + iy) * w + ix], sc, sh);
    }
  }
  reinterpret_cast<u32x4*>(out)[i] = u32x4{pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])};
}

// ---------------------------------------------------------------- im2col, from a bf16 NHWC map of 64 channels: 5x5, stride 1, pad 2
// One thread per 16-byte chunk: chunk q of a row is channels 8 (q % 8) ... of tap q / 8, so the copy keeps (ky, kx, c) order.
constexpr int P2_K = 5, P2_PAD = 2, P2_C = 64, P2_COLS = P2_K * P2_K * P2_C;
__global__ __launch_bounds__(256) void im2col_patch_map_kernel(const bf16_t* __restrict__ x, int h, int w, long total, bf16_t* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int q = (int)(i % (P2_COLS / 8));
  const long row = i / (P2_COLS / 8);
  const int ox = (int)(row % w);
  const long t = row / w;
  const int oy = (int)(t % h);
  const long b = t / h;
  const int tap = q >> 3, c8 = q & 7;
  const int ky = tap / P2_K, kx = tap - P2_K * ky;
  const int iy = oy + ky - P2_PAD, ix = ox + kx - P2_PAD;
  u32x4 v = {0u, 0u, 0u, 0u};
  if ((unsigned)iy < (unsigned)h && (unsigned)ix < (unsigned)w) v = reinterpret_cast<const u32x4*>(x)[((b * h + iy) * w + ix) * (P2_C / 8) + c8];
  reinterpret_cast<u32x4*>(out)[i] = v;
}

// ---------------------------------------------------------------- 3x3 max-pool, stride 2, no padding, floor
// One thread per 16-byte chunk (8 channels) of the output: nine 16-byte loads, one store.  The maximum of bf16 values is one of
// them, so nothing is rounded.  The last window ends at row 2 (oh - 1) + 2 <= h - 1.
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(const bf16_t* __restrict__ x, int h, int w, int oh, int ow, int c8, long total,
                                                           bf16_t* __restrict__ y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ch = (int)(i % c8);
  const long pix = i / c8;
  const int ox = (int)(pix % ow);
  const long t = pix / ow;
  const int oy = (int)(t % oh);
  const long b = t / oh;
  const u32x4* src = reinterpret_cast<const u32x4*>(x) + ((b * h + 2 * oy) * w + 2 * ox) * c8 + ch;
  u32x4 o = src[0];
#pragma unroll
  for (int k = 1; k < 9; ++k) {
    const u32x4 p = src[((long)(k / 3) * w + k % 3) * c8];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = max2bf(o[j], p[j]);
  }
  reinterpret_cast<u32x4*>(y)[i] = o;
}

// ---------------------------------------------------------------- the LPIPS head
// Layer l: maps x, y [pairs][pixels][C] (bf16, or fp32 with an optional ReLU on the way in), linear weights w [C] >= 0.
// Workgroup (chunk, pair): `chunk` counts HEAD_PIX-pixel chunks over all layers (HeadLayer::chunk0 is a layer's first).  Eight
// lanes share a pixel and read its channels in 16-byte chunks, twice: the two sums of squares (reduced over the eight lanes, so
// all of them hold the same norms), then w_c (a_c / na - b_c / nb)^2 with 1 / na = 1 / (sqrt(sum) + 1e-10).  A pixel of zeros
// has 1 / na = 1e10 and a_c / na = 0: no NaN.  a == b gives equal norms and a difference of exactly 0 -- which is why this
// function is compiled without contraction: fma(a, ra, -(b * rb)) would leave the rounding error of one product.  A lane adds
// its pixels' fp32 sums in fp64 in pixel order; then the shuffle tree and the four waves in wave order.
constexpr int HEAD_PIX = 256;      // pixels per workgroup: 8 rounds of 32 pixels
constexpr int HEAD_MAX_LAYERS = 8;
struct HeadLayer { const void* x; const void* y; const float* w; int pixels, c, bf16, relu, chunk0, nchunks; };
struct HeadTable { HeadLayer L[HEAD_MAX_LAYERS]; int n, chunks; };

MVD_DEVINL float sum8(float v) {      // over the eight lanes of a pixel
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  return v;
}

__global__ __launch_bounds__(256) void lpips_head_kernel(HeadTable T, double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  const int chunk = blockIdx.x, pair = blockIdx.y;
  int l = 0;
  for (int k = 1; k < T.n; ++k) l = chunk >= T.L[k].chunk0 ? k : l;
  const int C = T.L[l].c, pixels = T.L[l].pixels, is_bf = T.L[l].bf16, relu = T.L[l].relu;
  const float* __restrict__ wl = T.L[l].w;
  const int p0 = (chunk - T.L[l].chunk0) * HEAD_PIX;
  const int sub = threadIdx.x & 7, slot = threadIdx.x >> 3;
  const size_t pair_off = (size_t)pair * pixels;
  double acc = 0.0;
  for (int r = 0; r < HEAD_PIX / 32; ++r) {
    const int pix = p0 + r * 32 + slot;
    const bool live = pix < pixels;      // (the same for the eight lanes of a pixel; a dead slot re-reads the last pixel and adds nothing)
    const size_t base = (pair_off + (live ? pix : pixels - 1)) * C;
    float sa = 0.f, sb = 0.f, s = 0.f;
    if (is_bf) {
      const u32x4* a = reinterpret_cast<const u32x4*>(reinterpret_cast<const bf16_t*>(T.L[l].x) + base);
      const u32x4* b = reinterpret_cast<const u32x4*>(reinterpret_cast<const bf16_t*>(T.L[l].y) + base);
      for (int q = sub; q < (C >> 3); q += 8) {
        const u32x4 va = a[q], vb = b[q];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float a0 = bflo(va[k]), a1 = bfhi(va[k]), b0 = bflo(vb[k]), b1 = bfhi(vb[k]);
          sa += a0 * a0; sa += a1 * a1; sb += b0 * b0; sb += b1 * b1;
        }
      }
      sa = sum8(sa); sb = sum8(sb);
      const float ra = 1.0f / (sqrtf(sa) + 1e-10f), rb = 1.0f / (sqrtf(sb) + 1e-10f);
      for (int q = sub; q < (C >> 3); q += 8) {
        const u32x4 va = a[q], vb = b[q];
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(wl + 8 * q), w1 = *reinterpret_cast<const f32x4*>(wl + 8 * q + 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float d0 = bflo(va[k]) * ra - bflo(vb[k]) * rb, d1 = bfhi(va[k]) * ra - bfhi(vb[k]) * rb;
          const float u0 = k < 2 ? w0[2 * k] : w1[2 * k - 4], u1 = k < 2 ? w0[2 * k + 1] : w1[2 * k - 3];
          s += u0 * (d0 * d0); s += u1 * (d1 * d1);
        }
      }
    } else {
      const f32x4* a = reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(T.L[l].x) + base);
      const f32x4* b = reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(T.L[l].y) + base);
      for (int q = sub; q < (C >> 2); q += 8) {
        f32x4 va = a[q], vb = b[q];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (relu) { va[k] = fmaxf(va[k], 0.f); vb[k] = fmaxf(vb[k], 0.f); }
          sa += va[k] * va[k]; sb += vb[k] * vb[k];
        }
      }
      sa = sum8(sa); sb = sum8(sb);
      const float ra = 1.0f / (sqrtf(sa) + 1e-10f), rb = 1.0f / (sqrtf(sb) + 1e-10f);
      for (int q = sub; q < (C >> 2); q += 8) {
        f32x4 va = a[q], vb = b[q];
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wl + 4 * q);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (relu) { va[k] = fmaxf(va[k], 0.f); vb[k] = fmaxf(vb[k], 0.f); }
          const float d = va[k] * ra - vb[k] * rb;
          s += wv[k] * (d * d);
        }
      }
    }
    if (live) acc += (double)s;
  }
  acc = block_sum_f64(acc, red);
  if (threadIdx.x == 0) part[(size_t)pair * T.chunks + chunk] = acc;
}

// One workgroup: per pair and layer the chunk sums in a fixed strided order and the same tree, / pixels; the layers in layer
// order; thread 0 adds the pairs in pair order to a running total that lives in the workspace head (a distance over several
// passes), and the last pass writes total / all pairs.
__global__ __launch_bounds__(256) void lpips_finish_kernel(HeadTable T, const double* __restrict__ part, int pairs, double* __restrict__ total, int first,
                                                           int last, long all_pairs, float* __restrict__ per_pair, float* __restrict__ per_layer,
                                                           float* __restrict__ mean) {
  __shared__ double red[4];
  double run = first ? 0.0 : *total;      // (thread 0's copy is the one that counts)
  for (int p = 0; p < pairs; ++p) {
    double d = 0.0;
    for (int l = 0; l < T.n; ++l) {
      const double* src = part + (size_t)p * T.chunks + T.L[l].chunk0;
      double acc = 0.0;
      for (int c = threadIdx.x; c < T.L[l].nchunks; c += 256) acc += src[c];
      acc = block_sum_f64(acc, red);
      const double dl = acc / (double)T.L[l].pixels;
      if (threadIdx.x == 0 && per_layer) per_layer[(size_t)p * T.n + l] = (float)dl;
      d += dl;
    }
    if (threadIdx.x == 0 && per_pair) per_pair[p] = (float)d;
    run += d;
  }
  if (threadIdx.x == 0) {
    *total = run;
    if (last && mean) *mean = (float)(run / (double)all_pairs);
  }
}

constexpr int HEAD_BYTES = 256;      // the running total of a distance over several passes

int head_chunks(int pixels) { return (pixels + HEAD_PIX - 1) / HEAD_PIX; }

// fills chunk0 / nchunks / chunks from the pixels of the n layers already in T
int finish_table(HeadTable& T, const char* who) {
  long chunks = 0;
  for (int l = 0; l < T.n; ++l) {
    const HeadLayer& L = T.L[l];
    if (L.pixels <= 0 || L.c <= 0 || L.c % 64 || L.c > 4096) { mvd_set_error("%s: layer %d has %d pixels of %d channels (channels: a multiple of 64, at most 4096)", who, l, L.pixels, L.c); return -1; }
    T.L[l].chunk0 = (int)chunks; T.L[l].nchunks = head_chunks(L.pixels);
    chunks += T.L[l].nchunks;
  }
  if (chunks >= (1L << 31) - 1) { mvd_set_error("%s: too many pixels for one launch", who); return -1; }
  T.chunks = (int)chunks;
  return 0;
}

// part: pairs * T.chunks doubles; total: one double
int launch_head(const HeadTable& T, int pairs, double* part, double* total, int first, int last, long all_pairs, float* per_pair, float* per_layer,
                float* mean, hipStream_t s) {
  hipLaunchKernelGGL(lpips_head_kernel, dim3(T.chunks, pairs), dim3(256), 0, s, T, part);
  CHECK(launch_check("lpips head"));
  hipLaunchKernelGGL(lpips_finish_kernel, dim3(1), dim3(256), 0, s, T, part, pairs, total, first, last, all_pairs, per_pair, per_layer, mean);
  return launch_check("lpips finish");
}

int launch_im2col_image(const float* x, int nx, const float* y, int ny, int h, int w, const float* scale, const float* shift, bf16_t* out, hipStream_t s) {
  const int oh = (h + 2 * P1_PAD - P1_K) / P1_STRIDE + 1, ow = (w + 2 * P1_PAD - P1_K) / P1_STRIDE + 1;
  const long total = (long)(nx + ny) * oh * ow * (P1_COLS / 8);
  if (blocks_of(total) >= (1L << 31)) { mvd_set_error("im2col_patch: too many rows for one launch"); return -1; }
  hipLaunchKernelGGL(im2col_patch_image_kernel, dim3((unsigned)blocks_of(total)), dim3(256), 0, s, x, nx, y ? y : x, h, w, oh, ow, scale[0], scale[1], scale[2],
                     shift[0], shift[1], shift[2], total, out);
  return launch_check("im2col_patch (image)");
}
int launch_im2col_map(const bf16_t* x, int batch, int h, int w, bf16_t* out, hipStream_t s) {
  const long total = (long)batch * h * w * (P2_COLS / 8);
  if (blocks_of(total) >= (1L << 31)) { mvd_set_error("im2col_patch: too many rows for one launch"); return -1; }
  hipLaunchKernelGGL(im2col_patch_map_kernel, dim3((unsigned)blocks_of(total)), dim3(256), 0, s, x, h, w, total, out);
  return launch_check("im2col_patch (map)");
}
int launch_maxpool3(const bf16_t* x, int batch, int h, int w, int c, bf16_t* y, hipStream_t s) {
  if (!x || !y || batch <= 0 || h < 3 || w < 3 || c <= 0 || c % 8) { mvd_set_error("maxpool3x3s2: bad arguments (batch %d, %d x %d, c=%d: c %% 8 == 0, h, w >= 3)", batch, h, w, c); return -1; }
  if (((uintptr_t)x | (uintptr_t)y) & 15) { mvd_set_error("maxpool3x3s2: 16-byte aligned buffers"); return -1; }
  const int oh = (h - 3) / 2 + 1, ow = (w - 3) / 2 + 1;
  const long total = (long)batch * oh * ow * (c / 8);
  if (blocks_of(total) >= (1L << 31)) { mvd_set_error("maxpool3x3s2: too many elements for one launch"); return -1; }
  hipLaunchKernelGGL(maxpool3x3s2_kernel, dim3((unsigned)blocks_of(total)), dim3(256), 0, s, x, h, w, oh, ow, c / 8, total, y);
  return launch_check("maxpool3x3s2");
}

// ---------------------------------------------------------------- the layer table of torchvision's alexnet().features[:12]
struct AlexConv { int idx, cin, cout, k; };
const AlexConv kConvs[5] = {{0, 3, 64, 11}, {3, 64, 192, 5}, {6, 192, 384, 3}, {8, 384, 256, 3}, {10, 256, 256, 3}};
int64_t packed_k(const AlexConv& L) { return L.k == 11 ? P1_COLS : (int64_t)L.k * L.k * L.cin; }
// the scaling layer: (x - shift) / scale = x * (1 / scale) + (-shift / scale)
const float kShift[3] = {-.030f, -.088f, -.188f}, kScale[3] = {.458f, .448f, .450f};

struct Geo { int h[5], w[5]; int ph1, pw1, ph2, pw2; };      // h[k] x w[k]: tap k
Geo geo_of(int h, int w) {
  Geo g;
  g.h[0] = (h - 7) / 4 + 1; g.w[0] = (w - 7) / 4 + 1;
  g.ph1 = (g.h[0] - 3) / 2 + 1; g.pw1 = (g.w[0] - 3) / 2 + 1;
  g.h[1] = g.ph1; g.w[1] = g.pw1;
  g.ph2 = (g.ph1 - 3) / 2 + 1; g.pw2 = (g.pw1 - 3) / 2 + 1;
  for (int k = 2; k < 5; ++k) { g.h[k] = g.ph2; g.w[k] = g.pw2; }
  return g;
}

}  // namespace

struct mvd_lpips : ModuleBase {};

namespace {

constexpr size_t kSplitReserve = (size_t)512 * 128 * 128;      // floats: see tower_gemm

// The lock-step tiles with the split-K the tile heuristic asks for, as the VGG tower does -- but NOT TowerCtx::gemm: the split
// factor is not monotone in M (a smaller batch can ask for a split that a larger one does not), so the sizing run reserves a bound
// on the partials that is: S <= 16, and S <= 512 / tiles with tiles >= M N / (128 x 128) on the ReLU tiles, so
// S M N <= min(16 M N, 512 x 128 x 128).  Then the bytes of a pass never shrink when images are added, and a workspace sized for a
// full pass holds every shorter one.
int tower_gemm(TowerCtx& c, MvdGemmArgs& g) {
  if (c.err) return c.err;
  Arena& ar = c.m->ar;
  const int S = mvd_gemm_pick_splitk(g);
  const size_t mark = ar.off;
  const size_t mn = (size_t)g.M * g.N, reserve = 16 * mn < kSplitReserve ? 16 * mn : kSplitReserve;
  if (S > 1) {
    g.splitk = S;
    if (!c.dry && S * mn > reserve) { mvd_set_error("lpips: split-K %d of a %d x %d GEMM exceeds the partials the workspace was sized for", S, g.M, g.N); return c.err = -4; }
    g.part = ar.alloc_n<float>(c.dry ? reserve : S * mn);
  } else if (c.dry) {
    ar.alloc_n<float>(reserve);
  }
  if (ar.overflow()) { mvd_set_error("lpips: workspace too small for this pass"); return c.err = -4; }
  const int r = c.dry ? 0 : launch_tiled(g, c.s);
  ar.off = mark;
  return r;
}

int check_geometry(const char* who, int images, int h, int w) {
  // below 31 the second pool has no output: (h - 7) / 4 + 1 = 6 -> 2 -> nothing
  if (images <= 0 || h < 31 || w < 31 || h > 32768 || w > 32768) { mvd_set_error("%s: bad shape (%d images of %d x %d: h, w in [31, 32768])", who, images, h, w); return -1; }
  const Geo g = geo_of(h, w);
  if ((long)images * g.h[0] * g.w[0] >= (1L << 31) - 256) { mvd_set_error("%s: %d images of %d x %d is 2^31 rows or more: split the batch", who, images, h, w); return -1; }
  return 0;
}

// x / y: two fp32 NCHW arrays of nx / ny images that form ONE batch of nx + ny (y may be null).  taps: null, or five nullable
// buffers; tap_out receives where the five maps are (the caller's buffers, or the arena's).
int tower(TowerCtx& c, const float* x, int nx, const float* y, int ny, int h, int w, void* const* taps, bf16_t** tap_out) {
  Arena& ar = c.m->ar;
  const int B = nx + ny;
  const Geo G = geo_of(h, w);
  bf16_t* tap[5];
  for (int k = 0; k < 5; ++k) {
    tap[k] = (taps && taps[k]) ? (bf16_t*)taps[k] : ar.alloc_n<bf16_t>((size_t)B * G.h[k] * G.w[k] * kConvs[k].cout);
    tap_out[k] = tap[k];
  }
  const bf16_t* wt[5]; const float* bias[5];
  for (int k = 0; k < 5; ++k) {
    const std::string name = "features." + std::to_string(kConvs[k].idx);
    wt[k] = (const bf16_t*)c.W(name + ".weight", 1, kConvs[k].cout * packed_k(kConvs[k]));
    bias[k] = (const float*)c.W(name + ".bias", 0, kConvs[k].cout);
    if (c.err) return c.err;
  }
  const size_t mark = ar.off;
  // conv1: im2col rows of both halves, then a dense GEMM
  {
    const int M = B * G.h[0] * G.w[0];
    bf16_t* cols = ar.alloc_n<bf16_t>((size_t)M * P1_COLS);
    if (ar.overflow()) { mvd_set_error("lpips: workspace too small for this pass"); return -4; }
    if (!c.dry) {
      float sc[3], sh[3];
      for (int k = 0; k < 3; ++k) { sc[k] = 1.0f / kScale[k]; sh[k] = -kShift[k] / kScale[k]; }
      CHECK(launch_im2col_image(x, nx, y, ny, h, w, sc, sh, cols, c.s));
    }
    MvdGemmArgs g = gemm_dense(cols, nullptr, P1_COLS, 0, M, wt[0], 0, bias[0], 64, tap[0], 64);
    g.relu = 1;
    CHECK(tower_gemm(c, g));
    ar.off = mark;
  }
  // pool, conv2: im2col rows, then a dense GEMM (the buffers below reuse the rows of conv1: everything is in stream order)
  {
    const int M = B * G.ph1 * G.pw1;
    bf16_t* pooled = ar.alloc_n<bf16_t>((size_t)M * 64);
    bf16_t* cols = ar.alloc_n<bf16_t>((size_t)M * P2_COLS);
    if (ar.overflow()) { mvd_set_error("lpips: workspace too small for this pass"); return -4; }
    if (!c.dry) {
      CHECK(launch_maxpool3(tap[0], B, G.h[0], G.w[0], 64, pooled, c.s));
      CHECK(launch_im2col_map(pooled, B, G.ph1, G.pw1, cols, c.s));
    }
    MvdGemmArgs g = gemm_dense(cols, nullptr, P2_COLS, 0, M, wt[1], 0, bias[1], 192, tap[1], 192);
    g.relu = 1;
    CHECK(tower_gemm(c, g));
    ar.off = mark;
  }
  // pool, conv3 - conv5 on the implicit-GEMM tiles
  bf16_t* pooled = ar.alloc_n<bf16_t>((size_t)B * G.ph2 * G.pw2 * 192);
  if (ar.overflow()) { mvd_set_error("lpips: workspace too small for this pass"); return -4; }
  if (!c.dry) CHECK(launch_maxpool3(tap[1], B, G.ph1, G.pw1, 192, pooled, c.s));
  const bf16_t* in = pooled;
  for (int k = 2; k < 5; ++k) {
    MvdGemmArgs g = gemm_conv3(in, G.ph2, G.pw2, kConvs[k].cin, 1, 0, 0, nullptr, nullptr, 0, 0, wt[k], bias[k], B, G.ph2, G.pw2, kConvs[k].cout, tap[k]);
    g.relu = 1;
    CHECK(tower_gemm(c, g));
    in = tap[k];
  }
  ar.off = mark;
  return c.err;
}

// the head's table over the taps of `np` pairs stacked as [x of the pass; y of the pass]
int pair_table(TowerCtx& c, bf16_t* const* tap, int np, const Geo& G, HeadTable& T) {
  memset(&T, 0, sizeof(T));
  T.n = 5;
  for (int k = 0; k < 5; ++k) {
    const int pixels = G.h[k] * G.w[k], C = kConvs[k].cout;
    const float* lw = (const float*)c.W("lin" + std::to_string(k) + ".weight", 0, C);
    if (c.err) return c.err;
    T.L[k] = HeadLayer{tap[k], tap[k] + (size_t)np * pixels * C, lw, pixels, C, 1, 0, 0, 0};
  }
  return finish_table(T, "lpips_distance");
}

// arena bytes of one pass over `images` images, the head's partial sums of images / 2 pairs included
int pass_bytes(mvd_lpips* v, int images, int h, int w, size_t* out) {
  v->ar.reset(true);
  TowerCtx c{v, nullptr, true, false, "lpips: "};
  bf16_t* tap[5];
  CHECK(tower(c, nullptr, images, nullptr, 0, h, w, nullptr, tap));
  HeadTable T;
  CHECK(pair_table(c, tap, (images + 1) / 2, geo_of(h, w), T));
  v->ar.alloc_n<double>((size_t)((images + 1) / 2) * T.chunks);
  *out = HEAD_BYTES + align256(v->ar.high);
  return 0;
}

int check_weights(mvd_lpips* v, bool head) {
  TowerCtx c{v, nullptr, true, true, "lpips: "};
  for (int k = 0; k < 5; ++k) {
    const std::string name = "features." + std::to_string(kConvs[k].idx);
    c.W(name + ".weight", 1, kConvs[k].cout * packed_k(kConvs[k]));
    c.W(name + ".bias", 0, kConvs[k].cout);
    if (head) c.W("lin" + std::to_string(k) + ".weight", 0, kConvs[k].cout);
    if (c.err) return c.err;
  }
  return 0;
}

}  // namespace

extern "C" {

int mvd_lpips_create(mvd_lpips_t** out) {
  if (!out) { mvd_set_error("lpips_create: null argument"); return -1; }
  *out = new mvd_lpips();
  return 0;
}
int mvd_lpips_destroy(mvd_lpips_t* v) { delete v; return 0; }

int mvd_lpips_set_weight(mvd_lpips_t* v, const char* slot, const void* ptr, int64_t numel, int dtype) {
  return module_set_weight(v, "lpips", slot, ptr, numel, dtype);
}

int64_t mvd_lpips_workspace_bytes(mvd_lpips_t* v, int images, int h, int w) {
  if (!v) { mvd_set_error("lpips_workspace_bytes: null handle"); return -1; }
  if (int r = check_geometry("lpips_workspace_bytes", images, h, w)) return r;
  size_t need = 0;
  if (int r = pass_bytes(v, images, h, w, &need)) return r;
  return (int64_t)need;
}

int mvd_lpips_bind_workspace(mvd_lpips_t* v, void* ws, int64_t bytes) {
  return module_bind_workspace(v, "lpips", ws, bytes, HEAD_BYTES);
}

int mvd_lpips_features(mvd_lpips_t* v, const float* images_nchw, int images, int h, int w, void* const* taps, void* stream) {
  if (!v || !images_nchw || !taps) { mvd_set_error("lpips_features: null argument"); return -1; }
  for (int k = 0; k < 5; ++k)
    if ((uintptr_t)taps[k] & 15) { mvd_set_error("lpips_features: tap %d must be 16-byte aligned", k); return -1; }
  if (int r = check_geometry("lpips_features", images, h, w)) return r;
  if (int r = check_weights(v, false)) return r;      // weights and sizes first: nothing is launched on a failure
  size_t need = 0;
  if (int r = pass_bytes(v, images, h, w, &need)) return r;
  if (!v->ws_ptr) { mvd_set_error("lpips_features: workspace not bound"); return -1; }
  if (need > (size_t)v->ws_bytes) { mvd_set_error("lpips_features: workspace too small: need %zu bytes, bound %lld", need, (long long)v->ws_bytes); return -4; }
  module_bind_arena(*v, HEAD_BYTES);
  TowerCtx c{v, (hipStream_t)stream, false, true, "lpips: "};
  bf16_t* tap[5];
  return tower(c, images_nchw, images, nullptr, 0, h, w, taps, tap);
}

int mvd_lpips_distance(mvd_lpips_t* v, const float* x, const float* y, int pairs, int h, int w, int max_pairs_per_pass, float* per_pair_out,
                       float* per_layer_out, float* mean_out, void* stream) {
  if (!v || !x || !y || (!per_pair_out && !mean_out)) { mvd_set_error("lpips_distance: null argument"); return -1; }
  if (pairs <= 0 || pairs > (1 << 20)) { mvd_set_error("lpips_distance: bad number of pairs %d", pairs); return -1; }
  if (int r = check_geometry("lpips_distance", 2, h, w)) return r;
  if (int r = check_weights(v, true)) return r;
  if (!v->ws_ptr) { mvd_set_error("lpips_distance: workspace not bound"); return -1; }
  const Geo G = geo_of(h, w);
  // pairs per pass: as many as the bound workspace holds
  int pp = pairs > 32768 ? 32768 : pairs;      // (the head's grid: one row of workgroups per pair)
  if (max_pairs_per_pass > 0 && pp > max_pairs_per_pass) pp = max_pairs_per_pass;
  CHECK(pairs_per_pass("lpips_distance", h, w, v->ws_bytes, [&](int n, size_t* need) {
    if ((long)2 * n * G.h[0] * G.w[0] >= (1L << 31) - 256) { *need = ~size_t(0); return 0; }
    CHECK(pass_bytes(v, 2 * n, h, w, need));
    // the shorter last pass is sized too: nothing is launched unless every pass that will run fits
    size_t tail = 0;
    if (pairs % n) CHECK(pass_bytes(v, 2 * (pairs % n), h, w, &tail));
    if (tail > *need) *need = tail;
    return 0;
  }, &pp));
  const size_t img = (size_t)3 * h * w;
  double* total = reinterpret_cast<double*>(v->ws_ptr);
  for (int p0 = 0; p0 < pairs; p0 += pp) {
    const int np = pairs - p0 < pp ? pairs - p0 : pp;
    module_bind_arena(*v, HEAD_BYTES);
    TowerCtx c{v, (hipStream_t)stream, false, true, "lpips: "};
    bf16_t* tap[5];
    CHECK(tower(c, x + p0 * img, np, y + p0 * img, np, h, w, nullptr, tap));
    HeadTable T;
    CHECK(pair_table(c, tap, np, G, T));
    double* part = v->ar.alloc_n<double>((size_t)np * T.chunks);
    if (v->ar.overflow()) { mvd_set_error("lpips_distance: workspace too small for a pass of %d pairs", np); return -4; }
    CHECK(launch_head(T, np, part, total, p0 == 0, p0 + np == pairs, pairs, per_pair_out ? per_pair_out + p0 : nullptr,
                      per_layer_out ? per_layer_out + (size_t)p0 * 5 : nullptr, mean_out, (hipStream_t)stream));
  }
  return 0;
}

int mvd_op_im2col_patch(const void* src, int form, int batch, int h, int w, const float* scale, const float* shift, void* rows_out, void* stream) {
  if (!src || !rows_out || batch <= 0 || h <= 0 || w <= 0 || (form != 0 && form != 1) || ((scale == nullptr) != (shift == nullptr))) { mvd_set_error("im2col_patch: bad argument (form 0: fp32 NCHW image, 1: bf16 NHWC map of 64 channels)"); return -1; }
  if (((uintptr_t)rows_out & 15) || (form == 1 && ((uintptr_t)src & 15))) { mvd_set_error("im2col_patch: 16-byte aligned buffers"); return -1; }
  if (form == 1) {
    if (scale) { mvd_set_error("im2col_patch: the map form has no affine map"); return -1; }
    return launch_im2col_map((const bf16_t*)src, batch, h, w, (bf16_t*)rows_out, (hipStream_t)stream);
  }
  if (h < P1_K - 2 * P1_PAD || w < P1_K - 2 * P1_PAD) { mvd_set_error("im2col_patch: a %d x %d image has no 11 x 11 window", h, w); return -1; }
  static const float one[3] = {1.f, 1.f, 1.f}, zero[3] = {0.f, 0.f, 0.f};
  return launch_im2col_image((const float*)src, batch, nullptr, 0, h, w, scale ? scale : one, shift ? shift : zero, (bf16_t*)rows_out, (hipStream_t)stream);
}

int mvd_op_maxpool3x3s2(const void* x, int batch, int h, int w, int c, void* y, void* stream) {
  return launch_maxpool3((const bf16_t*)x, batch, h, w, c, (bf16_t*)y, (hipStream_t)stream);
}

int64_t mvd_op_lpips_head_ws_bytes(int layers, const int* pixels, int pairs) {
  if (layers <= 0 || layers > HEAD_MAX_LAYERS || !pixels || pairs <= 0) { mvd_set_error("lpips_head_ws_bytes: bad argument (1 - 8 layers)"); return -1; }
  size_t chunks = 0;
  for (int l = 0; l < layers; ++l) {
    if (pixels[l] <= 0) { mvd_set_error("lpips_head_ws_bytes: layer %d has %d pixels", l, pixels[l]); return -1; }
    chunks += head_chunks(pixels[l]);
  }
  return (int64_t)(HEAD_BYTES + align256((size_t)pairs * chunks * sizeof(double)));
}

int mvd_op_lpips_head(int layers, const void* const* x, const void* const* y, const int* dtype, const int* relu_in, const int* pixels, const int* channels,
                      const float* const* lin_w, int pairs, float* per_pair_out, float* per_layer_out, float* mean_out, void* ws, int64_t ws_bytes,
                      void* stream) {
  if (layers <= 0 || layers > HEAD_MAX_LAYERS || !x || !y || !dtype || !relu_in || !pixels || !channels || !lin_w || !ws || (!per_pair_out && !mean_out) ||
      pairs <= 0 || pairs > 65535) { mvd_set_error("lpips_head: bad argument (1 - 8 layers, pairs <= 65535)"); return -1; }
  HeadTable T; memset(&T, 0, sizeof(T));
  T.n = layers;
  for (int l = 0; l < layers; ++l) {
    if (!x[l] || !y[l] || !lin_w[l] || (dtype[l] != 0 && dtype[l] != 1) || (relu_in[l] != 0 && relu_in[l] != 1) || (dtype[l] == 1 && relu_in[l])) {
      mvd_set_error("lpips_head: layer %d: null pointer, dtype not 0 (fp32) / 1 (bf16), or relu_in on a bf16 map", l); return -1;
    }
    if (((uintptr_t)x[l] | (uintptr_t)y[l] | (uintptr_t)lin_w[l]) & 15) { mvd_set_error("lpips_head: layer %d: 16-byte aligned buffers", l); return -1; }
    T.L[l] = HeadLayer{x[l], y[l], lin_w[l], pixels[l], channels[l], dtype[l], relu_in[l], 0, 0};
  }
  CHECK(finish_table(T, "lpips_head"));
  if ((uintptr_t)ws & 255) { mvd_set_error("lpips_head: ws 256-byte aligned"); return -1; }
  if (ws_bytes < (int64_t)(HEAD_BYTES + align256((size_t)pairs * T.chunks * sizeof(double)))) { mvd_set_error("lpips_head: workspace too small"); return -4; }
  double* total = reinterpret_cast<double*>(ws);
  double* part = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + HEAD_BYTES);
  return launch_head(T, pairs, part, total, 1, 1, pairs, per_pair_out, per_layer_out, mean_out, (hipStream_t)stream);
}

}  // extern "C"
