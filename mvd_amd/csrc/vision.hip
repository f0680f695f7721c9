// CLIP image tower and CLIP score: what the reference's validation takes from torchmetrics'
// CLIPScore / transformers' CLIPModel (val.py:60-196, src/training/losses.py:59-98), on this project's kernels.
//
//   preprocess  fp32 NCHW images -> uint8 (losses.py:11-13) -> PIL's 8-bit bicubic resize (horizontal pass, uint8, vertical pass,
//               uint8: integer arithmetic, bit for bit) -> centre crop -> (u8 / 255 - mean) / std -> bf16 patch rows and / or
//               fp32 pixel_values
//   encode      patch rows . Wpatch^T (the GEMM kernels, fp32 out) -> [class | patches] + position, pre_layrnorm -> the layers
//               of clip_layer.h with the bidirectional flash attention of attention.hip (prescaled q, nq = nk = 1 + patches)
//               -> post_layernorm of token 0 -> visual_projection -> L2 normalisation
//   score       per-row dot products of two normalised embedding arrays and their mean in a fixed order
//
// Launches per image batch: 2 (resize passes) + GEMM + embed/LN + 8 per layer + [fold] + pool/project + L2 norm; + 1 for a cosine.
// No float atomics anywhere: two launches on the same input give the same bits.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "clip_layer.h"

namespace {

// ---------------------------------------------------------------- PIL's resampling coefficients (Resample.c), on the host
// One pass in -> out: out rows of `ksize` int32 weights (2^22 fixed point) + the first tap of every output position + its
// tap count.  Equal sizes: the pass is skipped (n == 0).
constexpr int PRECISION_BITS = 32 - 8 - 2;
struct PassTable {
  int in = 0, out = 0, ksize = 0;
  std::vector<int> kk, xmin, xcnt;
  bool skipped() const { return in == out; }
};
double bicubic_filter(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
int build_pass(int in, int out, PassTable* t) {
  t->in = in; t->out = out; t->ksize = 0;
  t->kk.clear(); t->xmin.clear(); t->xcnt.clear();
  if (in == out) return 0;
  const double scale = (double)in / out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * fs;
  const int ksize = (int)ceil(support) * 2 + 1;
  t->ksize = ksize;
  t->kk.assign((size_t)out * ksize, 0);
  t->xmin.resize(out); t->xcnt.resize(out);
  std::vector<double> k(ksize);
  const double ss = 1.0 / fs;
  for (int xx = 0; xx < out; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) { const double w = bicubic_filter((x + xmin - center + 0.5) * ss); k[x] = w; ww += w; }
    long worst = 0;
    for (int x = 0; x < xmax; ++x) {
      if (ww != 0.0) k[x] /= ww;
      const int q = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << PRECISION_BITS)) : (int)(0.5 + k[x] * (1 << PRECISION_BITS));
      t->kk[(size_t)xx * ksize + x] = q;
      worst += q < 0 ? -(long)q : (long)q;
    }
    // the accumulator is a 32-bit integer: 2^21 + 255 * sum |kk| must stay below 2^31
    if (255 * worst + (1L << (PRECISION_BITS - 1)) >= (1L << 31)) { mvd_set_error("vision_preprocess: resampling weights overflow 32 bits (%d -> %d)", in, out); return -1; }
    t->xmin[xx] = xmin; t->xcnt[xx] = xmax;
  }
  return 0;
}
// both passes of one geometry as one int32 blob: [kk_h | xmin_h | xcnt_h | kk_v | xmin_v | xcnt_v]
struct Geometry {
  PassTable hp, vp;
  std::vector<int> blob;
  size_t off_h = 0, off_v = 0;
};
void resized_size(int h, int w, int resize_to, int* oh, int* ow) {     // transformers' shortest-edge rule
  if (h <= w) { *oh = resize_to; *ow = (int)((long)resize_to * w / h); }
  else { *ow = resize_to; *oh = (int)((long)resize_to * h / w); }
}
size_t pass_ints(int in, int out) {
  if (in == out) return 0;
  const double scale = (double)in / out;
  const int ksize = (int)ceil(2.0 * (scale < 1.0 ? 1.0 : scale)) * 2 + 1;
  return (size_t)out * (ksize + 2);
}
size_t table_bytes(int h, int w, int resize_to) {
  if (h <= 0 || w <= 0 || resize_to <= 0) return 0;
  int oh, ow;
  resized_size(h, w, resize_to, &oh, &ow);
  return align256((pass_ints(w, ow) + pass_ints(h, oh)) * 4 + 16);
}

// ---------------------------------------------------------------- preprocess kernels
// losses.py:11-13 ((x.clamp(-1, 1) + 1) / 2 * 255).to(uint8): the same fp32 operations one by one (no contraction), truncated
MVD_DEVINL int to_u8(float x, int quantize) {
  float t = x;
  if (quantize) {
    t = fminf(fmaxf(x, -1.0f), 1.0f);
    t = __fmul_rn(__fmul_rn(__fadd_rn(t, 1.0f), 0.5f), 255.0f);
  }
  const int v = (int)t;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}
MVD_DEVINL int clip8(int acc) {
  const int v = acc >> PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}
// horizontal pass (or, with kk == null, the quantisation alone): x [planes][h][w] fp32 -> y [planes][h][ow] uint8
__global__ __launch_bounds__(256) void clip_resize_h_kernel(const float* __restrict__ x, long total, int w, int ow, int quantize, const int* __restrict__ kk,
                                                            const int* __restrict__ xmin, const int* __restrict__ xcnt, int ksize,
                                                            unsigned char* __restrict__ y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long row = i / ow;
  const int xo = (int)(i - row * ow);
  const float* xr = x + row * w;
  int v;
  if (!kk) v = to_u8(xr[xo], quantize);
  else {
    const int x0 = xmin[xo], n = xcnt[xo];
    const int* k = kk + (size_t)xo * ksize;
    int acc = 1 << (PRECISION_BITS - 1);
    for (int t = 0; t < n; ++t) acc += to_u8(xr[x0 + t], quantize) * k[t];
    v = clip8(acc);
  }
  y[i] = (unsigned char)v;
}
// vertical pass (kk == null: none) of the cropped window, then (u8 / 255 - mean) / std.  P > 0: the index space is the patch
// rows [B * (crop / P)^2][Kp], element (c, py, px) of patch (pr, pc), pad columns zero; pixel_values (nullable) gets the same
// values as fp32 NCHW.  P == 0: the index space is pixel_values alone.
struct NormArgs { float mean[3], std[3]; };
__global__ __launch_bounds__(256) void clip_resize_v_kernel(const unsigned char* __restrict__ u, long total, int h, int ow, int crop, int top, int left,
                                                            const int* __restrict__ kk, const int* __restrict__ ymin, const int* __restrict__ ycnt,
                                                            int ksize, NormArgs na, int P, int Kp, bf16_t* __restrict__ patches,
                                                            float* __restrict__ pixel_values) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  int b, c, cy, cx;
  if (P > 0) {
    const long row = i / Kp;
    const int col = (int)(i - row * Kp);
    if (col >= 3 * P * P) { patches[i] = 0; return; }
    const int g = crop / P, per = g * g;
    b = (int)(row / per);
    const int pi = (int)(row - (long)b * per), pr = pi / g, pc = pi - pr * g;
    c = col / (P * P);
    const int r = col - c * P * P, py = r / P, px = r - py * P;
    cy = pr * P + py; cx = pc * P + px;
  } else {
    const int cc = crop * crop;
    const long plane = i / cc;
    const int r = (int)(i - plane * cc);
    b = (int)(plane / 3); c = (int)(plane - (long)b * 3);
    cy = r / crop; cx = r - cy * crop;
  }
  const unsigned char* up = u + ((size_t)b * 3 + c) * h * ow + (left + cx);
  const int yo = top + cy;
  int v;
  if (!kk) v = up[(size_t)yo * ow];
  else {
    const int y0 = ymin[yo], n = ycnt[yo];
    const int* k = kk + (size_t)yo * ksize;
    int acc = 1 << (PRECISION_BITS - 1);
    for (int t = 0; t < n; ++t) acc += (int)up[(size_t)(y0 + t) * ow] * k[t];
    v = clip8(acc);
  }
  // transformers' order: the 1 / 255 product in double rounded to fp32, then (x - mean) / std in fp32
  const float f = __fdiv_rn(__fsub_rn((float)((double)v * (1.0 / 255.0)), na.mean[c]), na.std[c]);
  if (P > 0) patches[i] = f2bf(f);
  if (pixel_values) pixel_values[(((size_t)b * 3 + c) * crop + cy) * crop + cx] = f;
}
// fp32 pixel_values [B][3][S][S] -> bf16 patch rows (the encode entry that is handed pixel_values)
__global__ __launch_bounds__(256) void vit_patchify_kernel(const float* __restrict__ pv, long total, int S, int P, int Kp, bf16_t* __restrict__ patches) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long row = i / Kp;
  const int col = (int)(i - row * Kp);
  if (col >= 3 * P * P) { patches[i] = 0; return; }
  const int g = S / P, per = g * g;
  const int b = (int)(row / per), pi = (int)(row - (long)b * per), pr = pi / g, pc = pi - pr * g;
  const int c = col / (P * P), r = col - c * P * P, py = r / P, px = r - py * P;
  patches[i] = f2bf(pv[(((size_t)b * 3 + c) * S + pr * P + py) * S + pc * P + px]);
}

// ---------------------------------------------------------------- [class | patches] + position, then pre_layrnorm
// x[b][0] = class + pos[0], x[b][1 + i] = patch_out[b][i] + pos[1 + i]; x = LN(x) (fp32, the residual stream).  One wave per
// row, the row in registers, two-pass variance (as text_add_ln_kernel).
__global__ __launch_bounds__(256) void vit_embed_ln_kernel(const float* __restrict__ patch_out, const float* __restrict__ cls, const float* __restrict__ pos,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, int rows, int T, int H,
                                                           float eps, float* __restrict__ x) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int b = row / T, tok = row - b * T;
  const int nch = H / 4;
  const f32x4* src = reinterpret_cast<const f32x4*>(tok ? patch_out + ((size_t)b * (T - 1) + tok - 1) * H : cls);
  const f32x4* pp = reinterpret_cast<const f32x4*>(pos + (size_t)tok * H);
  f32x4 v[LN_MAXCH];
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < LN_MAXCH; ++c) {
    const int ch = c * 64 + lane;
    v[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (ch < nch) {
      v[c] = src[ch] + pp[ch];
      sum += (v[c][0] + v[c][1]) + (v[c][2] + v[c][3]);
    }
  }
  const float mean = wave_sum(sum) / (float)H;
  float sq = 0.f;
#pragma unroll
  for (int c = 0; c < LN_MAXCH; ++c) {
    if (c * 64 + lane < nch) {
      const f32x4 d = v[c] - mean;
      sq += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
    }
  }
  const float rstd = rsqrtf(wave_sum(sq) / (float)H + eps);
#pragma unroll
  for (int c = 0; c < LN_MAXCH; ++c) {
    const int ch = c * 64 + lane;
    if (ch < nch) {
      const f32x4 g = reinterpret_cast<const f32x4*>(gamma)[ch], bb = reinterpret_cast<const f32x4*>(beta)[ch];
      reinterpret_cast<f32x4*>(x + (size_t)row * H)[ch] = (v[c] - mean) * rstd * g + bb;
    }
  }
}
// out = x + delta (the encoder's last hidden state, only when the caller asks for it)
__global__ __launch_bounds__(256) void vit_fold_kernel(const float* __restrict__ x, const float* __restrict__ delta, long n4, float* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  reinterpret_cast<f32x4*>(out)[i] = reinterpret_cast<const f32x4*>(x)[i] + reinterpret_cast<const f32x4*>(delta)[i];
}

// ---------------------------------------------------------------- pooled row -> [LayerNorm] -> projection; L2 normalisation
// One workgroup per (batch row, slice of 64 output features): 32 x 12 workgroups for a ViT-L/14 batch of 32 instead of 32 (one
// workgroup per image measured 321 us, a seventh of a batch-1 encode).  Every slice rebuilds the pooled
// row -- at most 2048 floats -- itself.  The pooled token: 0 without ids (image tower); with ids, transformers' two rules -- the
// argmax of the ids when eos_id == 2 (its legacy branch), else the first position equal to eos_id (0 when there is none).
// row = hidden[b][tok] (+ delta[b][tok]); gamma != null: LayerNorm (two-pass) first.  The projection is fp32 weights
// [proj][H], fp32 accumulation: a wave takes 16 features of the slice four at a time, lane-strided partial sums, the shuffle
// tree.  The results go to raw and, still unnormalised, to nrm; clip_l2norm_kernel then divides nrm's rows by their norm.  All
// sums run in a fixed order.
constexpr int PP_MAXH = 2048, PP_SLICE = 64;
MVD_DEVINL float block_sum(float v, float* red) {      // 256 threads; every thread gets the sum (waves added in order)
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void clip_pool_project_kernel(const float* __restrict__ hidden, const float* __restrict__ delta, const int* __restrict__ ids,
                                                                int T, int H, int eos_id, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                float eps, const float* __restrict__ wp, int proj, float* __restrict__ raw,
                                                                float* __restrict__ nrm) {
  __shared__ __attribute__((aligned(16))) float row[PP_MAXH];
  __shared__ float red[4];
  __shared__ int s_tok;
  const int b = blockIdx.x, n0 = blockIdx.y * PP_SLICE, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) {
    int tok = 0;
    if (ids) {
      const int* r = ids + (size_t)b * T;
      if (eos_id == 2) { int best = r[0]; for (int t = 1; t < T; ++t) if (r[t] > best) { best = r[t]; tok = t; } }
      else { for (int t = 0; t < T; ++t) if (r[t] == eos_id) { tok = t; break; } }
    }
    s_tok = tok;
  }
  __syncthreads();
  const size_t base = ((size_t)b * T + s_tok) * H;
  float part = 0.f;
  for (int c = tid; c < H; c += 256) {
    const float v = hidden[base + c] + (delta ? delta[base + c] : 0.f);
    row[c] = v; part += v;
  }
  if (gamma) {
    const float mean = block_sum(part, red) / (float)H;
    float sq = 0.f;
    for (int c = tid; c < H; c += 256) { const float d = row[c] - mean; sq += d * d; }
    const float rstd = rsqrtf(block_sum(sq, red) / (float)H + eps);
    for (int c = tid; c < H; c += 256) row[c] = (row[c] - mean) * rstd * gamma[c] + beta[c];
  }
  __syncthreads();
#pragma unroll 1
  for (int g = 0; g < 4; ++g) {
    const int n = n0 + wave * 16 + g * 4;          // features n .. n + 3 (wave-uniform)
    if (n >= proj) break;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = lane; c < H / 4; c += 64) {
      const f32x4 r4 = *reinterpret_cast<const f32x4*>(row + 4 * c);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (n + j < proj) {
          const f32x4 w4 = reinterpret_cast<const f32x4*>(wp + (size_t)(n + j) * H)[c];
          acc[j] += (w4[0] * r4[0] + w4[1] * r4[1]) + (w4[2] * r4[2] + w4[3] * r4[3]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float v = wave_sum(acc[j]);
      if (lane == 0 && n + j < proj) {
        if (raw) raw[(size_t)b * proj + n + j] = v;
        if (nrm) nrm[(size_t)b * proj + n + j] = v;
      }
    }
  }
}
// x[b][:] /= ||x[b]||_2, in place; one workgroup per row, dim <= PP_MAXH
__global__ __launch_bounds__(256) void clip_l2norm_kernel(float* __restrict__ x, int dim) {
  __shared__ float red[4];
  float* r = x + (size_t)blockIdx.x * dim;
  float sq = 0.f;
  for (int n = threadIdx.x; n < dim; n += 256) sq += r[n] * r[n];
  const float norm = sqrtf(block_sum(sq, red));
  for (int n = threadIdx.x; n < dim; n += 256) r[n] = r[n] / norm;
}
int launch_pool_project(const float* hidden, const float* delta, const int* ids, int batch, int T, int H, int eos_id, const float* gamma, const float* beta,
                        float eps, const float* wp, int proj, float* raw, float* nrm, hipStream_t s) {
  hipLaunchKernelGGL(clip_pool_project_kernel, dim3(batch, (proj + PP_SLICE - 1) / PP_SLICE), dim3(256), 0, s, hidden, delta, ids, T, H, eos_id, gamma, beta, eps,
                     wp, proj, raw, nrm);
  CHECK(launch_check("clip pool + projection"));
  if (nrm) {
    hipLaunchKernelGGL(clip_l2norm_kernel, dim3(batch), dim3(256), 0, s, nrm, proj);
    CHECK(launch_check("clip L2 normalisation"));
  }
  return 0;
}

// ---------------------------------------------------------------- cosine of normalised rows and their mean
// One workgroup.  Wave w takes rows w, w + 4, ...: lane-strided products, the shuffle tree; it adds its rows in row order in
// fp64, the four wave sums are added in wave order through LDS and the mean is finished in fp64: two launches, same bits.
__global__ __launch_bounds__(256) void clip_cosine_kernel(const float* __restrict__ a, const float* __restrict__ b, int batch, int dim,
                                                          float* __restrict__ per_row, float* __restrict__ mean) {
  __shared__ double part[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc = 0.0;
  for (int r = wave; r < batch; r += 4) {
    const float *ar = a + (size_t)r * dim, *br = b + (size_t)r * dim;
    float d = 0.f;
    for (int c = lane; c < dim; c += 64) d += ar[c] * br[c];
    d = wave_sum(d);
    if (lane == 0 && per_row) per_row[r] = d;
    acc += (double)d;
  }
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0 && mean) *mean = (float)((((part[0] + part[1]) + part[2]) + part[3]) / (double)batch);
}

}  // namespace

struct mvd_vision : ModuleBase {      // (ar unused: the arena of a run lives in its ClipCtx, behind the split-K tile counters)
  mvd_vision_config_t cfg;
  std::map<std::tuple<int, int, int>, Geometry> geo;        // (h, w, resize_to) -> host tables, built once
  std::tuple<int, int, int> resident{0, 0, 0};              // the geometry whose tables sit at the head of the workspace
  size_t head_bytes = 0;                                    // bytes of that table region (the patch rows start behind it)
  int pre_batch = 0;                                        // batch of the patch rows the last preprocess left there
  int tokens() const { const int g = cfg.image_size / cfg.patch_size; return 1 + g * g; }
  int kp() const { return (3 * cfg.patch_size * cfg.patch_size + 63) / 64 * 64; }
  size_t patch_bytes(int B) const { return align256((size_t)B * (tokens() - 1) * kp() * 2); }
};

namespace {

// the tower's attention: bidirectional over the fused [B * T][3H] q | k | v rows (q prescaled at pack time) -> at [B * T][H]
int vit_attention(const bf16_t* qkv, bf16_t* at, int B, int heads, int T, hipStream_t s) {
  const int H = heads * 64;
  MvdAttnArgs a; memset(&a, 0, sizeof(a));
  a.nprob = 1; a.batch = B; a.heads = heads; a.prescaled = 1;
  a.p[0] = {qkv, qkv + H, qkv + 2 * H, at, 3 * H, 3 * H, 3 * H, H, (int64_t)T * 3 * H, (int64_t)T * 3 * H, (int64_t)T * 3 * H, (int64_t)T * H, T, T};
  return mvd_launch_attention(a, s);
}

// dry: sizes only; otherwise `cnt` = the counter words the dry run asked for.  Workspace behind the patch rows:
// [split-K tile counters | activations].
int vencode_impl(mvd_vision* v, const float* pixel_values, int B, float* last_hidden, float* embeds, float* embeds_norm, hipStream_t s,
                 bool dry, int cnt, size_t* high_out, int* cnt_out, bool check_w = true) {
  const mvd_vision_config_t& c = v->cfg;
  const int H = c.hidden_size, I = c.intermediate_size, T = v->tokens(), np = T - 1, M = B * T, Kp = v->kp();
  ClipCtx x{&v->w, "vision: ", c.layer_norm_eps, s, dry};
  x.check_w = check_w; x.ar.dry = dry;
  bf16_t* patches = nullptr;
  if (!dry) {
    char* p = reinterpret_cast<char*>(v->ws_ptr) + v->head_bytes;
    patches = reinterpret_cast<bf16_t*>(p);
    p += v->patch_bytes(B);
    x.cnt_base = reinterpret_cast<unsigned int*>(p);
    x.ar.base = p + cnt_bytes(cnt);
    if (cnt > 0 && hipMemsetAsync(x.cnt_base, 0, (size_t)cnt * 4, s) != hipSuccess) { mvd_set_error("vision_encode: hipMemsetAsync failed"); return -3; }
  }
  ClipBufs b;
  b.alloc(x, M, H, I);
  float* po = x.alloc<float>((size_t)B * np * H);       // patch embedding, fp32
  const bf16_t* wpatch = x.WB("patch.w", (int64_t)H * Kp);
  const float *cls = x.WF("cls", H), *pos = x.WF("pos", (int64_t)T * H), *gp = x.WF("pre_ln.g", H), *bp = x.WF("pre_ln.b", H);
  const float *go = x.WF("post_ln.g", H), *bo = x.WF("post_ln.b", H), *wproj = x.WF("proj.w", (int64_t)c.projection_dim * H);
  if (x.err) return x.err;
  if (!dry && pixel_values) {
    const long total = (long)B * np * Kp;
    hipLaunchKernelGGL(vit_patchify_kernel, dim3((unsigned)blocks_of(total)), dim3(256), 0, s, pixel_values, total, c.image_size, c.patch_size, Kp, patches);
    CHECK(launch_check("vision patchify"));
  }
  CHECK(x.linear(patches, Kp, B * np, wpatch, nullptr, H, po, true));
  if (!dry) {
    hipLaunchKernelGGL(vit_embed_ln_kernel, dim3((M + 3) / 4), dim3(256), 0, s, po, cls, pos, gp, bp, M, T, H, c.layer_norm_eps, b.xs);
    CHECK(launch_check("vision embedding"));
  }
  CHECK(clip_layers(x, b, c.num_layers, H, I, M, c.act, [&](const bf16_t* qkv, bf16_t* at) { return vit_attention(qkv, at, B, c.num_heads, T, s); }));
  if (!dry) {
    const float* dl = c.num_layers ? b.dl : nullptr;
    if (last_hidden) {
      if (dl) {
        const long n4 = (long)M * H / 4;
        hipLaunchKernelGGL(vit_fold_kernel, dim3((unsigned)blocks_of(n4)), dim3(256), 0, s, b.xs, dl, n4, last_hidden);
        CHECK(launch_check("vision last hidden state"));
      } else if (hipMemcpyAsync(last_hidden, b.xs, (size_t)M * H * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) { mvd_set_error("vision_encode: hipMemcpyAsync failed"); return -3; }
    }
    CHECK(launch_pool_project(b.xs, dl, nullptr, B, T, H, 0, go, bo, c.layer_norm_eps, wproj, c.projection_dim, embeds, embeds_norm, s));
  }
  if (high_out) *high_out = x.ar.high;
  if (cnt_out) *cnt_out = x.cnt_used;
  return x.err;
}

int vcheck_batch(int batch, int tokens, const char* who) {
  if (batch <= 0) { mvd_set_error("%s: bad batch %d", who, batch); return -1; }
  if ((long)batch * tokens > (1L << 20)) { mvd_set_error("%s: batch %d x %d tokens is beyond what one call takes", who, batch, tokens); return -1; }
  return 0;
}
// bytes behind the table region and the patch rows that one preprocess needs: the uint8 intermediate
size_t pre_rest_bytes(int B, int h, int w, int resize_to) {
  int oh, ow;
  resized_size(h, w, resize_to, &oh, &ow);
  return align256((size_t)B * 3 * h * ow);
}

}  // namespace

extern "C" {

int mvd_vision_create(const mvd_vision_config_t* cfg, mvd_vision_t** out) {
  if (!cfg || !out) { mvd_set_error("vision_create: null argument"); return -1; }
  if (cfg->num_heads <= 0 || cfg->hidden_size != cfg->num_heads * 64) { mvd_set_error("vision_create: hidden_size %d / num_heads %d: the head dimension must be 64", cfg->hidden_size, cfg->num_heads); return -1; }
  if (cfg->hidden_size % 64 || cfg->hidden_size > LN_MAXCH * 256) { mvd_set_error("vision_create: hidden_size %d must be a multiple of 64, at most %d", cfg->hidden_size, LN_MAXCH * 256); return -1; }
  if (cfg->intermediate_size <= 0 || cfg->intermediate_size % 64) { mvd_set_error("vision_create: intermediate_size %d must be a multiple of 64", cfg->intermediate_size); return -1; }
  if (cfg->projection_dim <= 0 || cfg->projection_dim % 64 || cfg->projection_dim > PP_MAXH) { mvd_set_error("vision_create: projection_dim %d must be a multiple of 64, at most %d", cfg->projection_dim, PP_MAXH); return -1; }
  if (cfg->patch_size <= 0 || cfg->patch_size > 64 || cfg->image_size <= 0 || cfg->image_size > 4096 || cfg->image_size % cfg->patch_size) { mvd_set_error("vision_create: image_size %d must be a multiple of patch_size %d", cfg->image_size, cfg->patch_size); return -1; }
  if (cfg->act != 0 && cfg->act != 1) { mvd_set_error("vision_create: act %d (0 gelu, 1 quick_gelu)", cfg->act); return -1; }
  if (cfg->num_layers < 0 || !(cfg->layer_norm_eps > 0.f)) { mvd_set_error("vision_create: bad num_layers / layer_norm_eps"); return -1; }
  mvd_vision* v = new mvd_vision();
  v->cfg = *cfg;
  *out = v;
  return 0;
}
int mvd_vision_destroy(mvd_vision_t* v) { delete v; return 0; }

int mvd_vision_set_weight(mvd_vision_t* v, const char* slot, const void* ptr, int64_t numel, int dtype) {
  return module_set_weight(v, "vision", slot, ptr, numel, dtype);
}

int64_t mvd_vision_workspace_bytes(mvd_vision_t* v, int batch, int h, int w, int resize_to) {
  if (!v) { mvd_set_error("vision_workspace_bytes: null handle"); return -1; }
  if (int r = vcheck_batch(batch, v->tokens(), "vision_workspace_bytes")) return r;
  if (h < 0 || w < 0 || h > 16384 || w > 16384 || ((h > 0 || w > 0) && (h < 1 || w < 1 || resize_to < 1 || resize_to > 4096))) { mvd_set_error("vision_workspace_bytes: bad image size %d x %d (resize_to %d)", h, w, resize_to); return -1; }
  size_t high = 0; int cnt = 0;
  if (int r = vencode_impl(v, nullptr, batch, nullptr, nullptr, nullptr, nullptr, true, 0, &high, &cnt, false)) return r;   // (sizes do not depend on the weights)
  size_t rest = cnt_bytes(cnt) + high;
  if (h > 0) { const size_t pr = pre_rest_bytes(batch, h, w, resize_to); rest = pr > rest ? pr : rest; }
  return (int64_t)(table_bytes(h, w, resize_to) + v->patch_bytes(batch) + rest + 4096);
}

int mvd_vision_bind_workspace(mvd_vision_t* v, void* ws, int64_t bytes) {
  CHECK(module_bind_workspace(v, "vision", ws, bytes, 0));
  v->resident = std::make_tuple(0, 0, 0); v->head_bytes = 0; v->pre_batch = 0;
  return 0;
}

int mvd_vision_preprocess(mvd_vision_t* v, const float* images, int batch, int h, int w, int quantize, int resize_to, int crop, const float* mean,
                          const float* std_, int want_patches, float* pixel_values, void* stream) {
  if (!v || !images || !mean || !std_) { mvd_set_error("vision_preprocess: null argument"); return -1; }
  if (int r = vcheck_batch(batch, v->tokens(), "vision_preprocess")) return r;
  if (h < 1 || w < 1 || h > 16384 || w > 16384) { mvd_set_error("vision_preprocess: bad image size %d x %d", h, w); return -1; }
  if (resize_to < 1 || resize_to > 4096 || crop < 1) { mvd_set_error("vision_preprocess: bad resize_to %d / crop %d", resize_to, crop); return -1; }
  if (!want_patches && !pixel_values) { mvd_set_error("vision_preprocess: nothing to write (no patch rows, no pixel_values)"); return -1; }
  if (want_patches && crop != v->cfg.image_size) { mvd_set_error("vision_preprocess: crop %d is not the model's image_size %d", crop, v->cfg.image_size); return -1; }
  for (int c = 0; c < 3; ++c) if (!(std_[c] > 0.f)) { mvd_set_error("vision_preprocess: image_std must be positive"); return -1; }
  int oh, ow;
  resized_size(h, w, resize_to, &oh, &ow);
  if (oh < crop || ow < crop) { mvd_set_error("vision_preprocess: the %d x %d resized image is smaller than the %d crop (padding is not implemented)", oh, ow, crop); return -1; }
  if ((long)batch * 3 * h * ow >= (1L << 31) || (long)batch * 3 * crop * crop >= (1L << 31)) { mvd_set_error("vision_preprocess: batch too large for one call"); return -1; }
  const auto key = std::make_tuple(h, w, resize_to);
  auto it = v->geo.find(key);
  if (it == v->geo.end()) {
    Geometry g;
    if (build_pass(w, ow, &g.hp) || build_pass(h, oh, &g.vp)) return -1;
    for (PassTable* t : {&g.hp, &g.vp}) {
      (t == &g.hp ? g.off_h : g.off_v) = g.blob.size();
      g.blob.insert(g.blob.end(), t->kk.begin(), t->kk.end());
      g.blob.insert(g.blob.end(), t->xmin.begin(), t->xmin.end());
      g.blob.insert(g.blob.end(), t->xcnt.begin(), t->xcnt.end());
    }
    it = v->geo.emplace(key, std::move(g)).first;
  }
  const Geometry& g = it->second;
  const size_t head = table_bytes(h, w, resize_to), pb = v->patch_bytes(batch), rest = pre_rest_bytes(batch, h, w, resize_to);
  if (g.blob.size() * 4 > head) { mvd_set_error("vision_preprocess: internal: table region too small"); return -1; }
  if (!v->ws_ptr) { mvd_set_error("vision_preprocess: workspace not bound"); return -1; }
  if (head + pb + rest > (size_t)v->ws_bytes) { mvd_set_error("vision_preprocess: workspace too small: need %zu bytes, bound %lld", head + pb + rest, (long long)v->ws_bytes); return -4; }
  hipStream_t s = (hipStream_t)stream;
  char* base = reinterpret_cast<char*>(v->ws_ptr);
  if (v->resident != key) {       // the first call of a geometry on this workspace uploads its tables; later ones nothing
    if (!g.blob.empty() && hipMemcpyAsync(base, g.blob.data(), g.blob.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess) { mvd_set_error("vision_preprocess: hipMemcpyAsync failed"); return -3; }
    v->resident = key; v->head_bytes = head;
  }
  v->pre_batch = 0;
  const int* tab = reinterpret_cast<const int*>(base);
  bf16_t* patches = reinterpret_cast<bf16_t*>(base + head);
  unsigned char* inter = reinterpret_cast<unsigned char*>(base + head + pb);
  const int *kh = nullptr, *xh = nullptr, *ch = nullptr, *kv = nullptr, *xv = nullptr, *cv = nullptr;
  if (!g.hp.skipped()) { kh = tab + g.off_h; xh = kh + (size_t)ow * g.hp.ksize; ch = xh + ow; }
  if (!g.vp.skipped()) { kv = tab + g.off_v; xv = kv + (size_t)oh * g.vp.ksize; cv = xv + oh; }
  const long th = (long)batch * 3 * h * ow;
  hipLaunchKernelGGL(clip_resize_h_kernel, dim3((unsigned)blocks_of(th)), dim3(256), 0, s, images, th, w, ow, quantize, kh, xh, ch, g.hp.ksize, inter);
  CHECK(launch_check("vision resize (horizontal)"));
  NormArgs na;
  for (int c = 0; c < 3; ++c) { na.mean[c] = mean[c]; na.std[c] = std_[c]; }
  const int top = (oh - crop) / 2, left = (ow - crop) / 2;
  const int P = want_patches ? v->cfg.patch_size : 0, Kp = v->kp();
  const long tv = want_patches ? (long)batch * (v->tokens() - 1) * Kp : (long)batch * 3 * crop * crop;
  hipLaunchKernelGGL(clip_resize_v_kernel, dim3((unsigned)blocks_of(tv)), dim3(256), 0, s, inter, tv, h, ow, crop, top, left, kv, xv, cv, g.vp.ksize, na, P, Kp,
                     want_patches ? patches : nullptr, pixel_values);
  CHECK(launch_check("vision resize (vertical)"));
  if (want_patches) v->pre_batch = batch;
  return 0;
}

int64_t mvd_vision_patch_rows_offset(mvd_vision_t* v) {
  if (!v) { mvd_set_error("vision_patch_rows_offset: null handle"); return -1; }
  if (!v->ws_ptr || v->pre_batch <= 0) { mvd_set_error("vision_patch_rows_offset: the workspace holds no patch rows"); return -1; }
  return (int64_t)v->head_bytes;
}

int mvd_vision_encode(mvd_vision_t* v, const float* pixel_values, int batch, float* last_hidden_out, float* embeds_out, float* embeds_norm_out,
                      void* stream) {
  if (!v || (!embeds_out && !embeds_norm_out && !last_hidden_out)) { mvd_set_error("vision_encode: null argument"); return -1; }
  if (int r = vcheck_batch(batch, v->tokens(), "vision_encode")) return r;
  size_t high = 0; int cnt = 0;
  if (int r = vencode_impl(v, nullptr, batch, nullptr, nullptr, nullptr, nullptr, true, 0, &high, &cnt)) return r;   // weights and sizes first: nothing is launched on a failure
  if (!v->ws_ptr) { mvd_set_error("vision_encode: workspace not bound"); return -1; }
  if (!pixel_values && v->pre_batch != batch) { mvd_set_error("vision_encode: no pixel_values and the workspace holds the patch rows of %d images, not %d", v->pre_batch, batch); return -1; }
  const size_t need = v->head_bytes + v->patch_bytes(batch) + cnt_bytes(cnt) + high;
  if (need > (size_t)v->ws_bytes) { mvd_set_error("vision_encode: workspace too small: need %zu bytes, bound %lld", need, (long long)v->ws_bytes); return -4; }
  if (pixel_values) v->pre_batch = 0;        // the patch rows are about to be overwritten
  return vencode_impl(v, pixel_values, batch, last_hidden_out, embeds_out, embeds_norm_out, (hipStream_t)stream, false, cnt, nullptr, nullptr);
}

int mvd_op_clip_pool_project(const float* hidden, const float* delta, const int32_t* ids, int batch, int tokens, int hidden_size, int eos_token_id,
                             const float* ln_gamma, const float* ln_beta, float eps, const float* proj_w, int proj_dim, float* embeds,
                             float* embeds_norm, void* stream) {
  if (!hidden || !proj_w || (!embeds && !embeds_norm)) { mvd_set_error("clip_pool_project: null argument"); return -1; }
  if (batch <= 0 || tokens <= 0 || hidden_size <= 0 || hidden_size % 4 || hidden_size > PP_MAXH || proj_dim <= 0 || proj_dim > PP_MAXH) { mvd_set_error("clip_pool_project: bad shape (batch %d, tokens %d, hidden %d, proj %d)", batch, tokens, hidden_size, proj_dim); return -1; }
  if ((ln_gamma == nullptr) != (ln_beta == nullptr)) { mvd_set_error("clip_pool_project: LayerNorm gain and bias go together"); return -1; }
  if (((uintptr_t)proj_w) & 15) { mvd_set_error("clip_pool_project: proj_w must be 16-byte aligned"); return -1; }
  return launch_pool_project(hidden, delta, ids, batch, tokens, hidden_size, eos_token_id, ln_gamma, ln_beta, eps, proj_w, proj_dim, embeds, embeds_norm,
                             (hipStream_t)stream);
}

int mvd_op_clip_cosine(const float* a, const float* b, int batch, int dim, float* per_row_out, float* mean_out, void* stream) {
  if (!a || !b || (!per_row_out && !mean_out) || batch <= 0 || dim <= 0) { mvd_set_error("clip_cosine: bad argument"); return -1; }
  hipLaunchKernelGGL(clip_cosine_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a, b, batch, dim, per_row_out, mean_out);
  return launch_check("clip_cosine");
}

int mvd_op_vision_add_ln(float* x, const float* delta, const float* gamma, const float* beta, int rows, int H, float eps, void* y_bf16, float* y_f32,
                         void* stream) {
  return op_add_ln("vision_add_ln", x, delta, gamma, beta, rows, H, eps, y_bf16, y_f32, (hipStream_t)stream);
}

int mvd_op_vision_act(const float* x, int64_t n, int act, void* y_bf16, void* stream) { return op_act("vision_act", x, n, act, y_bf16, (hipStream_t)stream); }

int mvd_op_vit_patchify(const float* pixel_values, int batch, int image_size, int patch_size, void* patches_bf16, void* stream) {
  if (!pixel_values || !patches_bf16) { mvd_set_error("vit_patchify: null argument"); return -1; }
  if (batch <= 0 || patch_size <= 0 || patch_size > 64 || image_size <= 0 || image_size > 4096 || image_size % patch_size) { mvd_set_error("vit_patchify: bad shape (batch %d, image_size %d, patch_size %d)", batch, image_size, patch_size); return -1; }
  const int g = image_size / patch_size, Kp = (3 * patch_size * patch_size + 63) / 64 * 64;
  const long total = (long)batch * g * g * Kp;
  if (total >= (1L << 31) || (long)batch * 3 * image_size * image_size >= (1L << 31)) { mvd_set_error("vit_patchify: batch too large for one call"); return -1; }
  hipLaunchKernelGGL(vit_patchify_kernel, dim3((unsigned)blocks_of(total)), dim3(256), 0, (hipStream_t)stream, pixel_values, total, image_size, patch_size, Kp,
                     (bf16_t*)patches_bf16);
  return launch_check("vision patchify");
}

int mvd_op_vit_embed_ln(const float* patch_out, const float* cls, const float* pos, const float* gamma, const float* beta, int batch, int tokens, int H,
                        float eps, float* x, void* stream) {
  if (!cls || !pos || !gamma || !beta || !x || (tokens > 1 && !patch_out)) { mvd_set_error("vit_embed_ln: null argument"); return -1; }
  if (batch <= 0 || tokens <= 0 || (long)batch * tokens > (1L << 20) || !(eps > 0.f)) { mvd_set_error("vit_embed_ln: bad batch %d / tokens %d / eps", batch, tokens); return -1; }
  if (H < 4 || H % 4 || H > LN_MAXCH * 256) { mvd_set_error("vit_embed_ln: H = %d must be a multiple of 4 in 4..%d", H, LN_MAXCH * 256); return -1; }
  if (((uintptr_t)patch_out | (uintptr_t)cls | (uintptr_t)pos | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)x) & 15) { mvd_set_error("vit_embed_ln: every pointer must be 16-byte aligned"); return -1; }
  const int M = batch * tokens;
  hipLaunchKernelGGL(vit_embed_ln_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, patch_out, cls, pos, gamma, beta, M, tokens, H, eps, x);
  return launch_check("vision embedding");
}

int mvd_op_vit_fold(const float* x, const float* delta, int64_t n, float* out, void* stream) {
  if (!x || !delta || !out) { mvd_set_error("vit_fold: null argument"); return -1; }
  if (n <= 0 || n % 4 || n > ((int64_t)1 << 38)) { mvd_set_error("vit_fold: n = %lld must be a positive multiple of 4 (at most 2^38)", (long long)n); return -1; }
  if (((uintptr_t)x | (uintptr_t)delta | (uintptr_t)out) & 15) { mvd_set_error("vit_fold: x, delta and out must be 16-byte aligned"); return -1; }
  const long n4 = (long)(n / 4);
  hipLaunchKernelGGL(vit_fold_kernel, dim3((unsigned)blocks_of(n4)), dim3(256), 0, (hipStream_t)stream, x, delta, n4, out);
  return launch_check("vision last hidden state");
}

int mvd_op_clip_l2norm(float* x, int rows, int dim, void* stream) {
  if (!x || rows <= 0 || dim <= 0 || dim > PP_MAXH) { mvd_set_error("clip_l2norm: bad argument (rows %d, dim %d: at most %d)", rows, dim, PP_MAXH); return -1; }
  hipLaunchKernelGGL(clip_l2norm_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, x, dim);
  return launch_check("clip L2 normalisation");
}

int mvd_debug_clip_attention(const void* qkv, void* out, int batch, int heads, int tokens, void* stream) {
  if (!qkv || !out || batch <= 0 || heads <= 0 || tokens <= 0) { mvd_set_error("clip_attention: bad argument"); return -1; }
  return vit_attention((const bf16_t*)qkv, (bf16_t*)out, batch, heads, tokens, (hipStream_t)stream);
}

}  // extern "C"
