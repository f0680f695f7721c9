// VGG-16 feature tower and perceptual loss: what the reference's PerceptualLoss takes from torchvision's
// vgg16(...).features[:29] (src/training/losses.py:21-56), on this project's kernels.
//
//   front end   fp32 NCHW images in [-1, 1] -> ((x + 1) / 2 - mean) / std as ONE affine map per channel, applied by
//               im2col_in_kernel while it writes the K = 27 -> 64 im2col rows (taps outside the image are zeros, not the shift:
//               a padded convolution of the NORMALISED image) -> conv1_1 as a K = 64 dense GEMM with ReLU
//   tower       twelve more 3x3 pad-1 convolutions on the lock-step implicit-GEMM tiles of gemm.hip with the ReLU epilogue
//               (MvdGemmArgs::relu), bf16 NHWC maps, a 2x2 max-pool behind relu1_2 / 2_2 / 3_3 / 4_3; the last convolution
//               (features.28) has no ReLU and writes fp32
//   loss        sum of squared differences of the two halves of the fp32 feature buffer per pair (fp64, fixed order), then a
//               one-workgroup finish in pair order
//
// Launches per pass: 2 (im2col of x and y) + 13 GEMMs (+ a reduce pass where K is split) + 4 pools + 2 for the loss.  x and y of
// a pair are rows of the same launches, so identical inputs give identical features and a loss of exactly 0.  No float atomics.
#include <stdio.h>
#include <string.h>

#include <string>

#include "host_util.h"

namespace {

// ---------------------------------------------------------------- 2x2 max-pool, stride 2 (floor: an odd trailing row / column is dropped)
// One thread per 16-byte chunk (8 channels) of the output: four 16-byte loads, one store; consecutive threads take consecutive
// chunks of a pixel, so a wave reads and writes whole 128-byte lines.  The values are post-ReLU bf16 (no NaN handling needed
// beyond what v_max gives); the maximum of bf16 values is one of them, so nothing is rounded.
__global__ __launch_bounds__(256) void maxpool2x2_kernel(const bf16_t* __restrict__ x, int h, int w, int c8, long total, bf16_t* __restrict__ y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int oh = h >> 1, ow = w >> 1;
  const int ch = (int)(i % c8);
  const long pix = i / c8;
  const int ox = (int)(pix % ow);
  const long t = pix / ow;
  const int oy = (int)(t % oh);
  const long b = t / oh;
  const u32x4* src = reinterpret_cast<const u32x4*>(x) + ((b * h + 2 * oy) * w + 2 * ox) * c8 + ch;
  const u32x4 p00 = src[0], p01 = src[c8], p10 = src[(long)w * c8], p11 = src[(long)w * c8 + c8];
  u32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = max2bf(max2bf(p00[k], p01[k]), max2bf(p10[k], p11[k]));
  reinterpret_cast<u32x4*>(y)[i] = o;
}

// ---------------------------------------------------------------- squared differences of two fp32 arrays, per pair
// Stage 1: workgroup (chunk, pair) sums (a - b)^2 over elements [chunk * SQ_CHUNK, ...) of the pair in fp64: a lane adds its
// float4s in index order, the shuffle tree, the four waves in wave order.  Stage 2, one workgroup: per pair the chunk sums in a
// fixed strided order and the same tree; thread 0 adds the pairs in pair order to a running total that lives in the workspace
// (a loss over several passes), and the last pass writes total / (all pairs * n).  The chunking depends on n alone: two
// launches give the same bits.  Against an fp64 evaluation of the same fp32 features the error is the fp64 round-off of
// ~n additions plus ONE rounding of the result to fp32: below 1e-7 relative.
constexpr int SQ_CHUNK = 4096;      // elements per workgroup: 256 lanes x 4 float4
__global__ __launch_bounds__(256) void sqdiff_kernel(const float* __restrict__ a, const float* __restrict__ b, long n, int nchunks, double* __restrict__ part) {
  __shared__ double red[4];
  const int chunk = blockIdx.x, pair = blockIdx.y;
  const float* ap = a + (size_t)pair * n;
  const float* bp = b + (size_t)pair * n;
  const long e0 = (long)chunk * SQ_CHUNK;
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long e = e0 + ((long)k * 256 + threadIdx.x) * 4;
    if (e < n) {      // (n % 4 == 0: a float4 is inside or outside as a whole)
      const f32x4 va = *reinterpret_cast<const f32x4*>(ap + e), vb = *reinterpret_cast<const f32x4*>(bp + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) { const double d = (double)va[j] - (double)vb[j]; acc += d * d; }
    }
  }
  acc = block_sum_f64(acc, red);
  if (threadIdx.x == 0) part[(size_t)pair * nchunks + chunk] = acc;
}
__global__ __launch_bounds__(256) void sqdiff_finish_kernel(const double* __restrict__ part, int pairs, int nchunks, long n, double* __restrict__ total,
                                                            int first, int last, long all_pairs, float* __restrict__ per_pair, float* __restrict__ mean) {
  __shared__ double red[4];
  double run = first ? 0.0 : *total;      // (thread 0's copy is the one that counts)
  for (int p = 0; p < pairs; ++p) {
    double acc = 0.0;
    for (int c = threadIdx.x; c < nchunks; c += 256) acc += part[(size_t)p * nchunks + c];
    acc = block_sum_f64(acc, red);
    if (threadIdx.x == 0 && per_pair) per_pair[p] = (float)(acc / (double)n);
    run += acc;
  }
  if (threadIdx.x == 0) {
    *total = run;
    if (last && mean) *mean = (float)(run / ((double)all_pairs * (double)n));
  }
}

// scale | shift of the front end, written on the device (no upload: nothing here touches the host's memory)
struct Affine { float v[8]; };
__global__ void vgg_affine_kernel(Affine a, float* __restrict__ out) {
  if (threadIdx.x < 8) out[threadIdx.x] = a.v[threadIdx.x];
}

int sq_chunks(long n) { return (int)((n + SQ_CHUNK - 1) / SQ_CHUNK); }

// part: pairs * sq_chunks(n) doubles; total: one double
int launch_sqdiff(const float* a, const float* b, int pairs, long n, double* part, double* total, int first, int last, long all_pairs, float* per_pair,
                  float* mean, hipStream_t s) {
  const int nc = sq_chunks(n);
  hipLaunchKernelGGL(sqdiff_kernel, dim3(nc, pairs), dim3(256), 0, s, a, b, n, nc, part);
  CHECK(launch_check("sqdiff"));
  hipLaunchKernelGGL(sqdiff_finish_kernel, dim3(1), dim3(256), 0, s, part, pairs, nc, n, total, first, last, all_pairs, per_pair, mean);
  return launch_check("sqdiff finish");
}

// ---------------------------------------------------------------- the layer table of torchvision's vgg16().features[:29]
struct VggConv { int idx, cin, cout; };
const VggConv kConvs[13] = {{0, 3, 64},    {2, 64, 64},   {5, 64, 128},   {7, 128, 128},  {10, 128, 256}, {12, 256, 256}, {14, 256, 256},
                            {17, 256, 512}, {19, 512, 512}, {21, 512, 512}, {24, 512, 512}, {26, 512, 512}, {28, 512, 512}};
// a pool follows convs 1, 3, 6, 9 (features.4, .9, .16, .23); taps[i] is the map in front of pool i
bool pool_after(int k) { return k == 1 || k == 3 || k == 6 || k == 9; }
constexpr int HEAD_BYTES = 256;      // the running total of a loss over several passes

}  // namespace

int mvd_launch_maxpool2x2(const bf16_t* x, int batch, int h, int w, int c, bf16_t* y, hipStream_t s) {
  if (!x || !y || batch <= 0 || h < 2 || w < 2 || c <= 0 || c % 8) { mvd_set_error("maxpool2x2: bad arguments (batch %d, %d x %d, c=%d: c %% 8 == 0, h, w >= 2)", batch, h, w, c); return -1; }
  if (((uintptr_t)x | (uintptr_t)y) & 15) { mvd_set_error("maxpool2x2: 16-byte aligned buffers"); return -1; }
  const long total = (long)batch * (h / 2) * (w / 2) * (c / 8);
  if (blocks_of(total) >= (1L << 31)) { mvd_set_error("maxpool2x2: too many elements for one launch"); return -1; }
  hipLaunchKernelGGL(maxpool2x2_kernel, dim3((unsigned)blocks_of(total)), dim3(256), 0, s, x, h, w, c / 8, total, y);
  return launch_check("maxpool2x2");
}

struct mvd_vgg : ModuleBase {};

namespace {

// (the tower runs on a TowerCtx; its gemm() splits K where the tile heuristic asks for it: deep layers of small images, M = images * h * w / 256)

int check_geometry(const char* who, int images, int h, int w) {
  if (images <= 0 || h < 16 || w < 16 || h > 32768 || w > 32768) { mvd_set_error("%s: bad shape (%d images of %d x %d: h, w in [16, 32768])", who, images, h, w); return -1; }
  // the lock-step tiles form 64-bit byte offsets; rows (images x h x w) and the tile count must stay below 2^31
  if ((long)images * h * w >= (1L << 31) - 256) { mvd_set_error("%s: %d images of %d x %d is 2^31 rows or more: split the batch", who, images, h, w); return -1; }
  return 0;
}

// x / y: two fp32 NCHW arrays of nx / ny images that form ONE batch of nx + ny (y may be null).  feat [nx + ny][h/16][w/16][512] fp32.
int tower(TowerCtx& c, const float* x, int nx, const float* y, int ny, int h, int w, float* feat, void* const* taps) {
  Arena& ar = c.m->ar;
  const int B = nx + ny;
  const size_t rows = (size_t)B * h * w;
  bf16_t* buf[2] = {ar.alloc_n<bf16_t>(rows * 64), ar.alloc_n<bf16_t>(rows * 64)};
  static const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  // scale | shift of the front end: 3 + 3 floats (at 0 and 4) that im2col_in_kernel reads with ld_ss = 0 (one pair set for the whole batch)
  float* ss = ar.alloc_n<float>(8);
  if (!c.dry) {
    Affine af; memset(&af, 0, sizeof(af));
    for (int k = 0; k < 3; ++k) { af.v[k] = 0.5f / stdv[k]; af.v[4 + k] = (0.5f - mean[k]) / stdv[k]; }
    hipLaunchKernelGGL(vgg_affine_kernel, dim3(1), dim3(64), 0, c.s, af, ss);
    CHECK(launch_check("vgg front-end constants"));
    CHECK(mvd_launch_im2col_in(x, nx, 3, h, w, ss, ss + 4, 0, buf[0], c.s));
    if (ny) CHECK(mvd_launch_im2col_in(y, ny, 3, h, w, ss, ss + 4, 0, buf[0] + (size_t)nx * h * w * 64, c.s));
  }
  int cur = 0, H = h, W_ = w, tap = 0;
  for (int k = 0; k < 13; ++k) {
    const VggConv& L = kConvs[k];
    const std::string name = "features." + std::to_string(L.idx);
    const int kk = k == 0 ? 64 : 9 * L.cin;
    const bf16_t* wt = (const bf16_t*)c.W(name + ".weight", 1, (int64_t)L.cout * kk);
    const float* bias = (const float*)c.W(name + ".bias", 0, L.cout);
    if (c.err) return c.err;
    const bool last = k == 12, pooled = pool_after(k);
    void* out = last ? (void*)feat : (pooled && taps && taps[tap]) ? taps[tap] : (void*)buf[cur ^ 1];
    const int M = B * H * W_;
    MvdGemmArgs g = k == 0 ? gemm_dense(buf[cur], nullptr, 64, 0, M, wt, 0, bias, 64, out, 64)
                           : gemm_conv3(buf[cur], H, W_, L.cin, 1, 0, 0, nullptr, nullptr, 0, 0, wt, bias, B, H, W_, L.cout, out);
    g.relu = last ? 0 : 1;
    g.out_f32 = last ? 1 : 0;      // the loss is a difference of two nearby maps: not rounded to bf16 first
    CHECK(c.gemm(g));
    if (last) break;
    if (pooled) {
      if (!c.dry) CHECK(mvd_launch_maxpool2x2((const bf16_t*)out, B, H, W_, L.cout, out == (void*)buf[cur ^ 1] ? buf[cur] : buf[cur ^ 1], c.s));
      if (out != (void*)buf[cur ^ 1]) cur ^= 1;      // (pooled from the tap buffer into the other ping-pong half)
      H /= 2; W_ /= 2; ++tap;
    } else {
      cur ^= 1;
    }
  }
  return c.err;
}

// arena bytes of one pass over `images` images, the internal fp32 feature buffer and the loss partials included
int pass_bytes(mvd_vgg* v, int images, int h, int w, size_t* out) {
  v->ar.reset(true);
  TowerCtx c{v, nullptr, true, false, "vgg: "};
  const long n = (long)(h / 16) * (w / 16) * 512;
  float* feat = v->ar.alloc_n<float>((size_t)images * n);
  v->ar.alloc_n<double>((size_t)((images + 1) / 2) * sq_chunks(n));
  CHECK(tower(c, nullptr, images, nullptr, 0, h, w, feat, nullptr));
  *out = HEAD_BYTES + align256(v->ar.high);
  return 0;
}

int check_weights(mvd_vgg* v) {
  TowerCtx c{v, nullptr, true, true, "vgg: "};
  for (const VggConv& L : kConvs) {
    const std::string name = "features." + std::to_string(L.idx);
    c.W(name + ".weight", 1, (int64_t)L.cout * (L.idx == 0 ? 64 : 9 * L.cin));
    c.W(name + ".bias", 0, L.cout);
    if (c.err) return c.err;
  }
  return 0;
}

}  // namespace

extern "C" {

int mvd_vgg_create(mvd_vgg_t** out) {
  if (!out) { mvd_set_error("vgg_create: null argument"); return -1; }
  *out = new mvd_vgg();
  return 0;
}
int mvd_vgg_destroy(mvd_vgg_t* v) { delete v; return 0; }

int mvd_vgg_set_weight(mvd_vgg_t* v, const char* slot, const void* ptr, int64_t numel, int dtype) {
  return module_set_weight(v, "vgg", slot, ptr, numel, dtype);
}

int64_t mvd_vgg_workspace_bytes(mvd_vgg_t* v, int images, int h, int w) {
  if (!v) { mvd_set_error("vgg_workspace_bytes: null handle"); return -1; }
  if (int r = check_geometry("vgg_workspace_bytes", images, h, w)) return r;
  size_t need = 0;
  if (int r = pass_bytes(v, images, h, w, &need)) return r;
  return (int64_t)need;
}

int mvd_vgg_bind_workspace(mvd_vgg_t* v, void* ws, int64_t bytes) {
  return module_bind_workspace(v, "vgg", ws, bytes, HEAD_BYTES);
}

int mvd_vgg_features(mvd_vgg_t* v, const float* images_nchw, int images, int h, int w, float* feat_out, void* const* taps, void* stream) {
  if (!v || !images_nchw || !feat_out) { mvd_set_error("vgg_features: null argument"); return -1; }
  if (int r = check_geometry("vgg_features", images, h, w)) return r;
  if (int r = check_weights(v)) return r;      // weights and sizes first: nothing is launched on a failure
  size_t need = 0;
  if (int r = pass_bytes(v, images, h, w, &need)) return r;
  if (!v->ws_ptr) { mvd_set_error("vgg_features: workspace not bound"); return -1; }
  if (need > (size_t)v->ws_bytes) { mvd_set_error("vgg_features: workspace too small: need %zu bytes, bound %lld", need, (long long)v->ws_bytes); return -4; }
  module_bind_arena(*v, HEAD_BYTES);
  TowerCtx c{v, (hipStream_t)stream, false, true, "vgg: "};
  return tower(c, images_nchw, images, nullptr, 0, h, w, feat_out, taps);
}

int mvd_vgg_perceptual(mvd_vgg_t* v, const float* x, const float* y, int pairs, int h, int w, float* loss_out, float* per_pair_out, void* stream) {
  if (!v || !x || !y || (!loss_out && !per_pair_out)) { mvd_set_error("vgg_perceptual: null argument"); return -1; }
  if (pairs <= 0 || pairs > (1 << 20)) { mvd_set_error("vgg_perceptual: bad number of pairs %d", pairs); return -1; }
  if (int r = check_geometry("vgg_perceptual", 2, h, w)) return r;
  if (int r = check_weights(v)) return r;
  if (!v->ws_ptr) { mvd_set_error("vgg_perceptual: workspace not bound"); return -1; }
  // pairs per pass: as many as the bound workspace holds
  int pp = pairs > 32768 ? 32768 : pairs;      // (the loss kernel's grid: one row of workgroups per pair)
  CHECK(pairs_per_pass("vgg_perceptual", h, w, v->ws_bytes, [&](int n, size_t* need) {
    if ((long)2 * n * h * w >= (1L << 31) - 256) { *need = ~size_t(0); return 0; }
    return pass_bytes(v, 2 * n, h, w, need);
  }, &pp));
  const long n = (long)(h / 16) * (w / 16) * 512;
  const size_t img = (size_t)3 * h * w;
  double* total = reinterpret_cast<double*>(v->ws_ptr);
  for (int p0 = 0; p0 < pairs; p0 += pp) {
    const int np = pairs - p0 < pp ? pairs - p0 : pp;
    module_bind_arena(*v, HEAD_BYTES);
    TowerCtx c{v, (hipStream_t)stream, false, true, "vgg: "};
    float* feat = v->ar.alloc_n<float>((size_t)2 * np * n);
    double* part = v->ar.alloc_n<double>((size_t)np * sq_chunks(n));
    CHECK(tower(c, x + p0 * img, np, y + p0 * img, np, h, w, feat, nullptr));
    CHECK(launch_sqdiff(feat, feat + (size_t)np * n, np, n, part, total, p0 == 0, p0 + np == pairs, pairs, per_pair_out ? per_pair_out + p0 : nullptr,
                        loss_out, (hipStream_t)stream));
  }
  return 0;
}

int mvd_op_conv3x3_relu(const void* x, int batch, int in_h, int in_w, int cin, const void* w, const float* bias, void* out, int cout, int relu,
                        int out_f32, int force_cfg, int splitk, float* splitk_ws, void* stream) {
  if (!x || !w || !out || batch <= 0 || in_h <= 0 || in_w <= 0 || cin <= 0 || cout <= 0 || (relu != 0 && relu != 1)) { mvd_set_error("mvd_op_conv3x3_relu: bad argument"); return -1; }
  if (force_cfg >= 100) { mvd_set_error("mvd_op_conv3x3_relu: the lock-step tiles only (force_cfg < 100)"); return -1; }
  if (splitk > 1 && !splitk_ws) { mvd_set_error("mvd_op_conv3x3_relu: split-K needs a workspace"); return -1; }
  MvdGemmArgs g = gemm_conv3((const bf16_t*)x, in_h, in_w, cin, 1, 0, 0, nullptr, nullptr, 0, 0, (const bf16_t*)w, bias, batch, in_h, in_w, cout, out);
  g.relu = relu; g.out_f32 = out_f32; g.part = splitk_ws; g.splitk = splitk > 1 ? splitk : 1;
  return launch_tiled(g, (hipStream_t)stream, force_cfg);
}

int mvd_op_linear_relu(const void* a, int k, const void* w, const float* bias, void* out, int m, int n, int relu, int out_f32, int force_cfg, int splitk,
                       float* splitk_ws, void* stream) {
  if (!a || !w || !out || m <= 0 || n <= 0 || k <= 0 || (relu != 0 && relu != 1)) { mvd_set_error("mvd_op_linear_relu: bad argument"); return -1; }
  if (force_cfg >= 100) { mvd_set_error("mvd_op_linear_relu: the lock-step tiles only (force_cfg < 100)"); return -1; }
  if (splitk > 1 && !splitk_ws) { mvd_set_error("mvd_op_linear_relu: split-K needs a workspace"); return -1; }
  MvdGemmArgs g = gemm_dense((const bf16_t*)a, nullptr, k, 0, m, (const bf16_t*)w, 0, bias, n, out, n);
  g.relu = relu; g.out_f32 = out_f32; g.part = splitk_ws; g.splitk = splitk > 1 ? splitk : 1;
  return launch_tiled(g, (hipStream_t)stream, force_cfg);
}

int mvd_op_maxpool2x2(const void* x, int batch, int h, int w, int c, void* y, void* stream) {
  return mvd_launch_maxpool2x2((const bf16_t*)x, batch, h, w, c, (bf16_t*)y, (hipStream_t)stream);
}

int64_t mvd_op_sqdiff_mean_ws_bytes(int pairs, int64_t n) {
  if (pairs <= 0 || n <= 0) { mvd_set_error("sqdiff_mean_ws_bytes: bad argument"); return -1; }
  return (int64_t)(HEAD_BYTES + align256((size_t)pairs * sq_chunks(n) * sizeof(double)));
}

int mvd_op_sqdiff_mean(const float* a, const float* b, int pairs, int64_t n, float* mean_out, float* per_pair_out, void* ws, int64_t ws_bytes,
                       void* stream) {
  if (!a || !b || !ws || (!mean_out && !per_pair_out) || pairs <= 0 || pairs > 65535 || n <= 0 || (n & 3)) { mvd_set_error("sqdiff_mean: bad argument (n %% 4 == 0, pairs <= 65535)"); return -1; }
  if ((((uintptr_t)a | (uintptr_t)b) & 15) || ((uintptr_t)ws & 255)) { mvd_set_error("sqdiff_mean: a, b 16-byte aligned, ws 256-byte aligned"); return -1; }
  if (ws_bytes < mvd_op_sqdiff_mean_ws_bytes(pairs, n)) { mvd_set_error("sqdiff_mean: workspace too small"); return -4; }
  double* total = reinterpret_cast<double*>(ws);
  double* part = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + HEAD_BYTES);
  return launch_sqdiff(a, b, pairs, n, part, total, 1, 1, pairs, per_pair_out, mean_out, (hipStream_t)stream);
}

}  // extern "C"
