// AutoencoderKL (the SD-2.1 VAE) encode / decode on the hot path's kernels -- SURVEY.md 8f row N3: the step either side
// of the denoising loop (/root/reference/src/models/pipeline.py:115-116 `vae.encode(x).latent_dist.sample()`,
// :171-176 `vae.decode(z).sample`).  diffusers-0.32.2 semantics restated (the reference reaches the VAE only through
// diffusers' StableDiffusionPipeline; parity unpinned like the UNet, oracle/vae.py):
//
//   Encoder  conv_in 3->C0 | per level: R x ResnetBlock2D (no time embedding), Downsample2D(padding=0) = zero pad
//            bottom/right + 3x3 stride-2 conv | mid: resnet, attention (1 head of C channels, GroupNorm, residual),
//            resnet | GroupNorm + SiLU | conv_out C->2*latent | quant_conv 1x1
//   Decoder  post_quant_conv 1x1 | conv_in latent->C | mid | per level (reversed): (R+1) resnets, nearest-2x + 3x3 conv |
//            GroupNorm + SiLU | conv_out C0->3
//
// Everything above 8 channels is NHWC bf16 through the implicit-GEMM conv / MFMA GEMM kernels (gemm.hip, gemm_pp.hip);
// the mid-block attention has head_dim = C (512), outside the 64-wide flash kernel, and runs as GEMMs per image:
// S = q.k^T / sqrt(C) (fp32) -> row softmax -> P.V with V^T produced directly by a GEMM with swapped roles (W_v . x^T),
// the value bias added after the product (softmax rows sum to one).
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "host_util.h"

namespace {

// fp32 row softmax -> bf16 probabilities; one workgroup per row
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ s, int n, bf16_t* __restrict__ p) {
  __shared__ float red[4];
  const float* row = s + (size_t)blockIdx.x * n;
  bf16_t* out = p + (size_t)blockIdx.x * n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float mx = -3.0e38f;
  for (int i = threadIdx.x; i < n; i += 256) mx = fmaxf(mx, row[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float sum = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) sum += __expf(row[i] - mx);
  sum = wave_sum(sum);
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  const float inv = 1.0f / (red[0] + red[1] + red[2] + red[3]);
  for (int i = threadIdx.x; i < n; i += 256) out[i] = f2bf(__expf(row[i] - mx) * inv);
}

// 1x1 convolution on a tiny channel count (<= 8 in and out), NCHW fp32 -> NCHW fp32 (quant_conv / post_quant_conv)
__global__ void pointwise_small_kernel(const float* __restrict__ x, int cin, int cout, int hw, const float* __restrict__ w,
                                       const float* __restrict__ bias, float* __restrict__ y, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;     // over (b, p)
  if (i >= total) return;
  const int p = i % hw;
  const long b = i / hw;
  float v[8];
  for (int c = 0; c < cin; ++c) v[c] = x[((size_t)b * cin + c) * hw + p];
  for (int o = 0; o < cout; ++o) {
    float a = bias[o];
    for (int c = 0; c < cin; ++c) a = fmaf(w[o * cin + c], v[c], a);
    y[((size_t)b * cout + o) * hw + p] = a;
  }
}

// DiagonalGaussianDistribution.sample(): mean + exp(0.5 * clamp(logvar, -30, 20)) * noise, times `scale`
__global__ void gaussian_sample_kernel(const float* __restrict__ mom, const float* __restrict__ noise, int c, int hw, float scale,
                                       float* __restrict__ out, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;     // over (b, c, p)
  if (i >= total) return;
  const long chw = (long)c * hw;
  const long b = i / chw, r = i - b * chw;
  const float mean = mom[b * 2 * chw + r];
  const float lv = fminf(fmaxf(mom[b * 2 * chw + chw + r], -30.f), 20.f);
  out[i] = (mean + __expf(0.5f * lv) * noise[i]) * scale;
}

// the kernel keeps one pixel's input channels in float v[8]: more is refused before the launch
int pointwise_shape(int B, int cin, int cout, int hw) {
  if (B <= 0 || hw <= 0 || cin <= 0 || cout <= 0) { mvd_set_error("vae pointwise: bad shape (batch %d, cin %d, cout %d, hw %d)", B, cin, cout, hw); return -1; }
  if (cin > 8 || cout > 8) { mvd_set_error("vae pointwise: cin %d / cout %d: at most 8 channels in and out", cin, cout); return -1; }
  return 0;
}
int launch_pointwise(const float* x, int B, int cin, int cout, int hw, const float* w, const float* b, float* y, hipStream_t s) {
  const long total = (long)B * hw;
  hipLaunchKernelGGL(pointwise_small_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, cin, cout, hw, w, b, y, total);
  return launch_check("vae pointwise");
}

}  // namespace

struct mvd_vae : ModuleBase {
  mvd_vae_config_t cfg;
};

namespace {

struct VCtx {
  mvd_vae* v;
  hipStream_t s;
  bool dry;
  int err = 0;

  const void* W(const std::string& name, int dtype, int64_t numel) { return dry ? nullptr : v->w.find(name, dtype, numel, &err, "vae: "); }
  const bf16_t* WB(const std::string& n, int64_t numel) { return (const bf16_t*)W(n, 1, numel); }
  const float* WF(const std::string& n, int64_t numel) { return (const float*)W(n, 0, numel); }
  template <class T> T* alloc(size_t n) { return v->ar.alloc_n<T>(n); }
  Act act(int B, int H, int W_, int C) { return arena_act(v->ar, B, H, W_, C); }

  // the tiled kernels only (never the small-M kernels); an unsplit launch leaves splitk = 0, "undecided"
  int gemm(MvdGemmArgs& g) { return err ? err : arena_gemm(v->ar, g, s, dry); }
  int linear(const bf16_t* a, int k, int M, const bf16_t* w, const float* bias, int N, const bf16_t* res, void* out, float alpha = 1.f,
             bool out_f32 = false) {
    MvdGemmArgs g = gemm_dense(a, nullptr, k, 0, M, w, 0, bias, N, out, N);
    g.res = res; g.ldres = N; g.alpha = alpha; g.out_f32 = out_f32;
    return gemm(g);
  }
  // 3x3 conv (pad 1; stride 2 = the VAE's bottom/right-padded downsampler; ups = nearest 2x in front), optional residual
  // or fused 1x1 shortcut on `sc`
  int conv3(const Act& x, int stride, int ups, const bf16_t* w, const float* bias, const bf16_t* res, const bf16_t* sc, int scc, Act& out) {
    MvdGemmArgs g = gemm_conv3(x.p, x.H, x.W, x.C, stride, ups, stride == 2 ? 1 : 0, sc, nullptr, scc, 0, w, bias, out.B, out.H, out.W, out.C, out.p);
    g.res = res;
    return gemm(g);
  }
  int groupnorm(const Act& x, const float* g, const float* b, int silu, bf16_t* y) {
    if (err) return err;
    float* ws = alloc<float>((size_t)x.B * MVD_GN_MAXCHUNK * v->cfg.norm_num_groups * 2);
    if (dry) return 0;
    return mvd_launch_groupnorm(x.p, nullptr, x.C, 0, x.B, x.hw(), v->cfg.norm_num_groups, v->cfg.norm_eps, g, b, silu, y, ws, s);
  }

  // ResnetBlock2D without a time embedding: GN+SiLU -> conv1 -> GN+SiLU -> conv2 (+ x, or || 1x1 conv_shortcut(x))
  int resnet(const std::string& key, const Act& x, int cout, Act& out) {
    const int cin = x.C;
    const size_t mark = v->ar.off;
    Act t1 = act(x.B, x.H, x.W, cin);
    CHECK(groupnorm(x, WF(key + ".norm1.g", cin), WF(key + ".norm1.b", cin), 1, t1.p));
    Act h1 = act(x.B, x.H, x.W, cout);
    CHECK(conv3(t1, 1, 0, WB(key + ".conv1.w", (int64_t)cout * 9 * cin), WF(key + ".conv1.b", cout), nullptr, nullptr, 0, h1));
    Act t2 = act(x.B, x.H, x.W, cout);
    CHECK(groupnorm(h1, WF(key + ".norm2.g", cout), WF(key + ".norm2.b", cout), 1, t2.p));
    if (cin != cout) {
      CHECK(conv3(t2, 1, 0, WB(key + ".conv2.w", (int64_t)cout * (9 * cout + cin)), WF(key + ".conv2.b", cout), nullptr, x.p, cin, out));
    } else {
      CHECK(conv3(t2, 1, 0, WB(key + ".conv2.w", (int64_t)cout * 9 * cout), WF(key + ".conv2.b", cout), x.p, nullptr, 0, out));
    }
    v->ar.off = mark;
    return err;
  }

  // mid-block attention: one head of C channels over the H*W positions of each image
  int attention(const std::string& key, const Act& x, Act& out) {
    const int C = x.C, hw = x.hw(), M = x.rows();
    if (hw % 64 || C % 64) { mvd_set_error("vae attention: %d positions x %d channels must be multiples of 64", hw, C); return -1; }
    const size_t mark = v->ar.off;
    bf16_t* xn = alloc<bf16_t>((size_t)M * C);
    CHECK(groupnorm(x, WF(key + ".norm.g", C), WF(key + ".norm.b", C), 0, xn));
    bf16_t* q = alloc<bf16_t>((size_t)M * C);
    bf16_t* k = alloc<bf16_t>((size_t)M * C);
    bf16_t* o = alloc<bf16_t>((size_t)M * C);
    CHECK(linear(xn, C, M, WB(key + ".q.w", (int64_t)C * C), WF(key + ".q.b", C), C, nullptr, q));
    CHECK(linear(xn, C, M, WB(key + ".k.w", (int64_t)C * C), WF(key + ".k.b", C), C, nullptr, k));
    bf16_t* vt = alloc<bf16_t>((size_t)C * hw);
    float* sc = alloc<float>((size_t)hw * hw);
    bf16_t* pr = alloc<bf16_t>((size_t)hw * hw);
    const bf16_t* wv = WB(key + ".v.w", (int64_t)C * C);
    const float* bv = WF(key + ".v.b", C);
    const float scale = 1.0f / sqrtf((float)C);
    for (int b = 0; b < x.B && !err; ++b) {
      const size_t o0 = (size_t)b * hw * C;
      CHECK(linear(wv, C, C, xn + o0, nullptr, hw, nullptr, vt));                          // V^T = W_v . x^T   [C][hw]
      CHECK(linear(q + o0, C, hw, k + o0, nullptr, hw, nullptr, sc, scale, true));          // S = q.k^T / sqrt(C)  fp32
      if (!dry) { hipLaunchKernelGGL(softmax_rows_kernel, dim3(hw), dim3(256), 0, s, sc, hw, pr); CHECK(launch_check("vae softmax")); }
      CHECK(linear(pr, hw, hw, vt, bv, C, nullptr, o + o0));                                // P.V + b_v
    }
    CHECK(linear(o, C, M, WB(key + ".out.w", (int64_t)C * C), WF(key + ".out.b", C), C, x.p, out.p));   // to_out + residual
    v->ar.off = mark;
    return err;
  }

  int mid(const std::string& p, const Act& x, Act& out) {
    const int C = x.C;
    Act r0 = act(x.B, x.H, x.W, C), a0 = act(x.B, x.H, x.W, C);
    CHECK(resnet(p + ".resnets.0", x, C, r0));
    CHECK(attention(p + ".attn", r0, a0));
    CHECK(resnet(p + ".resnets.1", a0, C, out));
    return err;
  }
  // conv_in: NCHW fp32 -> im2col rows (K padded to 64) -> GEMM
  int conv_in(const std::string& key, const float* x_nchw, int B, int cin, int H, int W_, int cout, Act& out) {
    bf16_t* col = alloc<bf16_t>((size_t)B * H * W_ * 64);
    if (!dry && !err) CHECK(mvd_launch_im2col_in(x_nchw, B, cin, H, W_, nullptr, nullptr, 0, col, s));
    return linear(col, 64, B * H * W_, WB(key + ".w", (int64_t)cout * 64), WF(key + ".b", cout), cout, nullptr, out.p);
  }
  int norm_conv_out(const std::string& pfx, const Act& x, int cout, float* y_nchw) {
    bf16_t* t = alloc<bf16_t>((size_t)x.rows() * x.C);
    CHECK(groupnorm(x, WF(pfx + ".norm_out.g", x.C), WF(pfx + ".norm_out.b", x.C), 1, t));
    const bf16_t* w = WB(pfx + ".conv_out.w", (int64_t)cout * 9 * x.C);
    const float* b = WF(pfx + ".conv_out.b", cout);
    if (!dry && !err) CHECK(mvd_launch_conv_out(t, x.B, x.H, x.W, x.C, w, b, cout, y_nchw, s));
    return err;
  }
  int pointwise(const std::string& key, const float* x, int B, int cin, int cout, int hw, float* y) {
    CHECK(pointwise_shape(B, cin, cout, hw));
    const float* w = WF(key + ".w", (int64_t)cout * cin);
    const float* b = WF(key + ".b", cout);
    if (dry || err) return err;
    return launch_pointwise(x, B, cin, cout, hw, w, b, y, s);
  }
};

int encode_impl(mvd_vae* v, const float* image, int B, int H, int W_, float* moments, hipStream_t s, bool dry) {
  const mvd_vae_config_t& c = v->cfg;
  const int n = c.num_levels, div = 1 << (n - 1);
  if (B <= 0 || H <= 0 || W_ <= 0 || H % div || W_ % div) { mvd_set_error("vae encode: image %dx%d must be divisible by %d", H, W_, div); return -1; }
  v->ar.reset(dry);
  VCtx x{v, s, dry};
  Act h = x.act(B, H, W_, c.block_out_channels[0]);
  CHECK(x.conv_in("encoder.conv_in", image, B, c.in_channels, H, W_, c.block_out_channels[0], h));
  for (int i = 0; i < n; ++i) {
    const int co = c.block_out_channels[i];
    const std::string bk = "encoder.down_blocks." + std::to_string(i);
    for (int j = 0; j < c.layers_per_block; ++j) {
      Act r = x.act(B, h.H, h.W, co);
      CHECK(x.resnet(bk + ".resnets." + std::to_string(j), h, co, r));
      h = r;
    }
    if (i + 1 < n) {
      Act d = x.act(B, h.H / 2, h.W / 2, co);
      CHECK(x.conv3(h, 2, 0, x.WB(bk + ".down.w", (int64_t)co * 9 * co), x.WF(bk + ".down.b", co), nullptr, nullptr, 0, d));
      h = d;
    }
  }
  Act m = x.act(B, h.H, h.W, h.C);
  CHECK(x.mid("encoder.mid_block", h, m));
  const int L2 = 2 * c.latent_channels, hw = m.hw();
  float* pre = x.alloc<float>((size_t)B * L2 * hw);
  CHECK(x.norm_conv_out("encoder", m, L2, pre));
  CHECK(x.pointwise("quant_conv", pre, B, L2, L2, hw, moments));
  if (x.err) return x.err;
  if (!dry && v->ar.high > (size_t)v->ws_bytes) { mvd_set_error("vae encode: workspace too small"); return -4; }
  return 0;
}

// one mid-block attention (the encoder's or the decoder's weights) on caller buffers: the same VCtx::attention that
// encode_impl / decode_impl run inside mid(), for the operator-level tests
int mid_attention_impl(mvd_vae* v, int decoder, const bf16_t* x_nhwc, int B, int H, int W_, bf16_t* out_nhwc, hipStream_t s, bool dry) {
  if (B <= 0 || H <= 0 || W_ <= 0 || (decoder != 0 && decoder != 1)) { mvd_set_error("vae mid_attention: bad shape or coder"); return -1; }
  v->ar.reset(dry);
  VCtx x{v, s, dry};
  Act in;
  in.p = const_cast<bf16_t*>(x_nhwc); in.B = B; in.H = H; in.W = W_; in.C = v->cfg.block_out_channels[v->cfg.num_levels - 1];
  Act out = in;
  out.p = out_nhwc;
  CHECK(x.attention(decoder ? "decoder.mid_block.attn" : "encoder.mid_block.attn", in, out));
  return x.err;
}

int decode_impl(mvd_vae* v, const float* latents, int B, int h_, int w_, float* image, hipStream_t s, bool dry) {
  const mvd_vae_config_t& c = v->cfg;
  const int n = c.num_levels;
  if (B <= 0 || h_ <= 0 || w_ <= 0) { mvd_set_error("vae decode: bad shape"); return -1; }
  v->ar.reset(dry);
  VCtx x{v, s, dry};
  const int L = c.latent_channels, cm = c.block_out_channels[n - 1];
  float* z = x.alloc<float>((size_t)B * L * h_ * w_);
  CHECK(x.pointwise("post_quant_conv", latents, B, L, L, h_ * w_, z));
  Act h = x.act(B, h_, w_, cm);
  CHECK(x.conv_in("decoder.conv_in", z, B, L, h_, w_, cm, h));
  Act m = x.act(B, h_, w_, cm);
  CHECK(x.mid("decoder.mid_block", h, m));
  h = m;
  for (int i = 0; i < n; ++i) {
    const int co = c.block_out_channels[n - 1 - i];
    const std::string bk = "decoder.up_blocks." + std::to_string(i);
    for (int j = 0; j <= c.layers_per_block; ++j) {
      Act r = x.act(B, h.H, h.W, co);
      CHECK(x.resnet(bk + ".resnets." + std::to_string(j), h, co, r));
      h = r;
    }
    if (i + 1 < n) {
      Act u = x.act(B, h.H * 2, h.W * 2, co);
      CHECK(x.conv3(h, 1, 1, x.WB(bk + ".up.w", (int64_t)co * 9 * co), x.WF(bk + ".up.b", co), nullptr, nullptr, 0, u));
      h = u;
    }
  }
  CHECK(x.norm_conv_out("decoder", h, c.in_channels, image));
  if (x.err) return x.err;
  if (!dry && v->ar.high > (size_t)v->ws_bytes) { mvd_set_error("vae decode: workspace too small"); return -4; }
  return 0;
}

}  // namespace

extern "C" {

int mvd_vae_create(const mvd_vae_config_t* cfg, mvd_vae_t** out) {
  if (!cfg || !out) { mvd_set_error("vae_create: null argument"); return -1; }
  if (cfg->num_levels < 2 || cfg->num_levels > MVD_MAX_LEVELS || cfg->layers_per_block < 1 || cfg->in_channels > 7 || cfg->latent_channels > 4 ||
      cfg->in_channels < 1 || cfg->latent_channels < 1) { mvd_set_error("vae_create: unsupported topology"); return -1; }
  for (int i = 0; i < cfg->num_levels; ++i)
    if (cfg->block_out_channels[i] % 64 || cfg->block_out_channels[i] % cfg->norm_num_groups) { mvd_set_error("vae_create: level %d: channels must be a multiple of 64 and of the group count", i); return -1; }
  mvd_vae* v = new mvd_vae();
  v->cfg = *cfg;
  *out = v;
  return 0;
}
int mvd_vae_destroy(mvd_vae_t* v) { delete v; return 0; }

int mvd_vae_set_weight(mvd_vae_t* v, const char* slot, const void* ptr, int64_t numel, int dtype) {
  return module_set_weight(v, "vae", slot, ptr, numel, dtype);
}

int64_t mvd_vae_workspace_bytes(mvd_vae_t* v, int batch, int height, int width, int decode) {
  if (!v) { mvd_set_error("vae_workspace_bytes: null handle"); return -1; }
  const int r = decode ? decode_impl(v, nullptr, batch, height, width, nullptr, nullptr, true)
                       : encode_impl(v, nullptr, batch, height, width, nullptr, nullptr, true);
  if (r) return r;
  return (int64_t)v->ar.high + 4096;
}

int mvd_vae_bind_workspace(mvd_vae_t* v, void* ws, int64_t ws_bytes) {
  CHECK(module_bind_workspace(v, "vae", ws, ws_bytes, 0));
  v->ar.base = (char*)ws; v->ar.cap = (size_t)ws_bytes;
  return 0;
}

int mvd_vae_encode(mvd_vae_t* v, const float* image_nchw, int batch, int height, int width, float* moments, void* stream) {
  if (!v || !image_nchw || !moments) { mvd_set_error("vae_encode: null argument"); return -1; }
  if (!v->ws_ptr) { mvd_set_error("vae_encode: workspace not bound"); return -1; }
  if (int r = encode_impl(v, nullptr, batch, height, width, nullptr, nullptr, true)) return r;       // size first: nothing is launched into a short buffer
  if (v->ar.high > (size_t)v->ws_bytes) { mvd_set_error("vae_encode: workspace too small: need %zu bytes, bound %lld", v->ar.high, (long long)v->ws_bytes); return -4; }
  return encode_impl(v, image_nchw, batch, height, width, moments, (hipStream_t)stream, false);
}

int mvd_vae_decode(mvd_vae_t* v, const float* latents_nchw, int batch, int height, int width, float* image, void* stream) {
  if (!v || !latents_nchw || !image) { mvd_set_error("vae_decode: null argument"); return -1; }
  if (!v->ws_ptr) { mvd_set_error("vae_decode: workspace not bound"); return -1; }
  if (int r = decode_impl(v, nullptr, batch, height, width, nullptr, nullptr, true)) return r;
  if (v->ar.high > (size_t)v->ws_bytes) { mvd_set_error("vae_decode: workspace too small: need %zu bytes, bound %lld", v->ar.high, (long long)v->ws_bytes); return -4; }
  return decode_impl(v, latents_nchw, batch, height, width, image, (hipStream_t)stream, false);
}

int64_t mvd_vae_mid_attention_workspace_bytes(mvd_vae_t* v, int decoder, int batch, int height, int width) {
  if (!v) { mvd_set_error("vae_mid_attention_workspace_bytes: null handle"); return -1; }
  if (int r = mid_attention_impl(v, decoder, nullptr, batch, height, width, nullptr, nullptr, true)) return r;
  return (int64_t)v->ar.high + 4096;
}

int mvd_vae_mid_attention(mvd_vae_t* v, int decoder, const void* x_nhwc, int batch, int height, int width, void* out_nhwc, void* stream) {
  if (!v || !x_nhwc || !out_nhwc) { mvd_set_error("vae_mid_attention: null argument"); return -1; }
  if (!v->ws_ptr) { mvd_set_error("vae_mid_attention: workspace not bound"); return -1; }
  if (int r = mid_attention_impl(v, decoder, nullptr, batch, height, width, nullptr, nullptr, true)) return r;   // size first
  if (v->ar.high > (size_t)v->ws_bytes) { mvd_set_error("vae_mid_attention: workspace too small: need %zu bytes, bound %lld", v->ar.high, (long long)v->ws_bytes); return -4; }
  return mid_attention_impl(v, decoder, (const bf16_t*)x_nhwc, batch, height, width, (bf16_t*)out_nhwc, (hipStream_t)stream, false);
}

int mvd_op_softmax_rows(const float* s, int rows, int n, void* p_bf16, void* stream) {
  if (!s || !p_bf16 || rows <= 0 || n <= 0) { mvd_set_error("softmax_rows: bad argument"); return -1; }
  hipLaunchKernelGGL(softmax_rows_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, s, n, (bf16_t*)p_bf16);
  return launch_check("softmax_rows");
}

int mvd_op_gaussian_sample(const float* moments, const float* noise, int batch, int channels, int hw, float scale, float* out, void* stream) {
  if (!moments || !noise || !out || batch <= 0 || channels <= 0 || hw <= 0) { mvd_set_error("gaussian_sample: bad argument"); return -1; }
  const long total = (long)batch * channels * hw;
  hipLaunchKernelGGL(gaussian_sample_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, moments, noise, channels, hw,
                     scale, out, total);
  return launch_check("gaussian_sample");
}

int mvd_op_vae_pointwise(const float* x, int batch, int cin, int cout, int hw, const float* w, const float* bias, float* y, void* stream) {
  if (!x || !w || !bias || !y) { mvd_set_error("vae_pointwise: null argument"); return -1; }
  CHECK(pointwise_shape(batch, cin, cout, hw));
  return launch_pointwise(x, batch, cin, cout, hw, w, bias, y, (hipStream_t)stream);
}

}  // extern "C"
