// The pre-LN transformer layer both CLIP towers run (text.hip: causal, vision.hip: bidirectional), lifted out of text.hip:
// residual add + LayerNorm, the activation pass, the GEMM routing and the per-layer schedule.  The two towers differ in
// the attention launch only, which the schedule takes as a callable.  Everything here sits in an unnamed namespace: each
// of the two translation units carries its own copy of the two kernels.
//
//   per layer:  h = LN1(x); q,k,v = h.Wqkv^T + b;  a = attention(q, k, v)  per head of 64 channels
//               x = x + a.Wo^T + bo;  h = LN2(x); h = act(h.W1^T + b1); x = x + h.W2^T + b2
//
// The residual stream x stays in fp32; GEMM operands are bf16 with fp32 accumulation.  A projection that feeds the residual
// writes its fp32 result (`out_f32`) to a delta buffer, and the NEXT add + LayerNorm folds it into x, so after the last
// layer the caller still owes x += delta (its final LayerNorm does it).  Per layer: add+LN, QKV GEMM, attention,
// out-projection, add+LN, fc1, activation, fc2 = 8 launches (plus in-kernel split-K where the small-M planner asks for it).
#pragma once
#include <string>

#include "host_util.h"

namespace {

// ---------------------------------------------------------------- residual add + LayerNorm
// x[row] += delta[row] (fp32, in place; delta may be null), then y = LN(x) as bf16 (y_bf) or fp32 (y_f32).  One wave per
// row, the row in registers (H <= 2048), two-pass variance.
constexpr int LN_MAXCH = 8;     // float4 chunks per lane
__global__ __launch_bounds__(256) void text_add_ln_kernel(float* __restrict__ x, const float* __restrict__ delta, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, int rows, int H, float eps, bf16_t* __restrict__ y_bf,
                                                          float* __restrict__ y_f32) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int nch = H / 4;
  f32x4* xp = reinterpret_cast<f32x4*>(x + (size_t)row * H);
  const f32x4* dp = delta ? reinterpret_cast<const f32x4*>(delta + (size_t)row * H) : nullptr;
  f32x4 v[LN_MAXCH];
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < LN_MAXCH; ++c) {
    const int ch = c * 64 + lane;
    v[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (ch < nch) {
      v[c] = xp[ch];
      if (dp) { v[c] += dp[ch]; xp[ch] = v[c]; }
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
      const f32x4 g = reinterpret_cast<const f32x4*>(gamma)[ch], b = reinterpret_cast<const f32x4*>(beta)[ch];
      const f32x4 r = (v[c] - mean) * rstd * g + b;
      if (y_f32) reinterpret_cast<f32x4*>(y_f32 + (size_t)row * H)[ch] = r;
      else {
        const u32x2 o = {pack2bf(r[0], r[1]), pack2bf(r[2], r[3])};
        reinterpret_cast<u32x2*>(y_bf + (size_t)row * H)[ch] = o;
      }
    }
  }
}

// ---------------------------------------------------------------- activation pass: fp32 pre-activations -> bf16
// act 0: gelu (erf form), 1: quick_gelu = x * sigmoid(1.702 x).  8 elements per thread (2 x 16-byte loads, one 16-byte store).
// gelu as 0.5 x erfc(-x / sqrt 2): the same function as 0.5 x (1 + erf(x / sqrt 2)) without its cancellation -- 1 + erf loses every
// digit below x = -3 (10 % off at -5, flushed to 0 from -5.7 on, where the value is still a normal bf16 number).
MVD_DEVINL float text_act(float x, int act) {
  return act ? x / (1.0f + __expf(-1.702f * x)) : 0.5f * x * erfcf(x * -0.70710678118654752f);
}
__global__ __launch_bounds__(256) void text_act_kernel(const float* __restrict__ x, long n8, int act, bf16_t* __restrict__ y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const f32x4 a = reinterpret_cast<const f32x4*>(x)[2 * i], b = reinterpret_cast<const f32x4*>(x)[2 * i + 1];
  const u32x4 o = {pack2bf(text_act(a[0], act), text_act(a[1], act)), pack2bf(text_act(a[2], act), text_act(a[3], act)),
                   pack2bf(text_act(b[0], act), text_act(b[1], act)), pack2bf(text_act(b[2], act), text_act(b[3], act))};
  reinterpret_cast<u32x4*>(y)[i] = o;
}

// ---------------------------------------------------------------- the two launches, shared by the schedule and the operator entries
int launch_add_ln(float* x, const float* delta, const float* g, const float* b, int rows, int H, float eps, bf16_t* y_bf, float* y_f32,
                  hipStream_t s) {
  hipLaunchKernelGGL(text_add_ln_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, delta, g, b, rows, H, eps, y_bf, y_f32);
  return launch_check("add+layernorm");
}
int launch_act(const float* x, long n8, int act, bf16_t* y, hipStream_t s) {
  hipLaunchKernelGGL(text_act_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, x, n8, act, y);
  return launch_check("activation");
}
// the operator entries of a translation unit (mvd_op_text_* / mvd_op_vision_*): what the kernels cannot take is refused here
int op_add_ln(const char* who, float* x, const float* delta, const float* g, const float* b, int rows, int H, float eps, void* y_bf,
              float* y_f32, hipStream_t s) {
  if (!x || !g || !b) { mvd_set_error("%s: null argument", who); return -1; }
  if ((y_bf == nullptr) == (y_f32 == nullptr)) { mvd_set_error("%s: exactly one of y_bf16 and y_f32 must be given", who); return -1; }
  if (rows <= 0 || rows > (1 << 24) || !(eps > 0.f)) { mvd_set_error("%s: bad rows %d / eps", who, rows); return -1; }
  if (H < 4 || H % 4 || H > LN_MAXCH * 256) { mvd_set_error("%s: H = %d must be a multiple of 4 in 4..%d", who, H, LN_MAXCH * 256); return -1; }
  if ((((uintptr_t)x | (uintptr_t)delta | (uintptr_t)g | (uintptr_t)b | (uintptr_t)y_f32) & 15) || ((uintptr_t)y_bf & 7)) {
    mvd_set_error("%s: x, delta, gamma, beta and y_f32 must be 16-byte aligned, y_bf16 8-byte aligned", who); return -1;
  }
  return launch_add_ln(x, delta, g, b, rows, H, eps, (bf16_t*)y_bf, y_f32, s);
}
int op_act(const char* who, const float* x, int64_t n, int act, void* y, hipStream_t s) {
  if (!x || !y) { mvd_set_error("%s: null argument", who); return -1; }
  if (n <= 0 || n % 8 || n > ((int64_t)1 << 40)) { mvd_set_error("%s: n = %lld must be a positive multiple of 8 (at most 2^40)", who, (long long)n); return -1; }
  if (act != 0 && act != 1) { mvd_set_error("%s: act %d (0 gelu, 1 quick_gelu)", who, act); return -1; }
  if (((uintptr_t)x | (uintptr_t)y) & 15) { mvd_set_error("%s: x and y must be 16-byte aligned", who); return -1; }
  return launch_act(x, (long)(n / 8), act, (bf16_t*)y, s);
}

// ---------------------------------------------------------------- host side of one tower's schedule
struct ClipCtx {
  const WeightTable* w;
  const char* prefix;         // of the error messages ("text: ", "vision: ")
  float eps;
  hipStream_t s;
  bool dry;
  bool check_w = true;        // false (sizing only): weight slots are not looked at
  Arena ar;                   // activations (ar.base: behind the split-K tile counters)
  unsigned int* cnt_base = nullptr;
  int cnt_used = 0;
  int err = 0;
  int last_tile = -1, last_splitk = 1;   // route of the last linear(): small-M tile (-1: the tiled kernels) and split-K factor

  template <class T> T* alloc(size_t n) { return ar.alloc_n<T>(n); }
  const void* W(const std::string& name, int dtype, int64_t numel) { return check_w ? w->find(name, dtype, numel, &err, prefix) : nullptr; }
  const bf16_t* WB(const std::string& n, int64_t numel) { return (const bf16_t*)W(n, 1, numel); }
  const float* WF(const std::string& n, int64_t numel) { return (const float*)W(n, 0, numel); }

  // out[M][N] = a[M][K] . w[N][K]^T + bias: the small-M kernels (split-K combined in the kernel) where their planner takes
  // the shape, else the tiled kernels (+ split-K reduce) -- the same routing as the UNet engine's
  int linear(const bf16_t* a, int K, int M, const bf16_t* wt, const float* bias, int N, void* out, bool out_f32) {
    if (err) return err;
    MvdGemmArgs g = gemm_dense(a, nullptr, K, 0, M, wt, 0, bias, N, out, N);
    g.ldres = N; g.out_f32 = out_f32 ? 1 : 0;
    const size_t mark = ar.off;
    int r = 0;
    int tile = 0, ns = 0, S = 1;
    if (mvd_gemm_sm_plan(g, &tile, &ns, &S)) {
      if (S > 1) {
        g.splitk = S; g.part = alloc<float>((size_t)S * M * N);
        g.tile_cnt = cnt_base + cnt_used;
        cnt_used += ((M + 63) / 64) * (N / 64);       // (an upper bound for every tile shape)
      }
      if (!dry) r = mvd_launch_gemm_sm(g, s, tile, ns);
    } else {
      S = mvd_gemm_pick_splitk(g);
      if (S > 1) { g.splitk = S; g.part = alloc<float>((size_t)S * M * N); } else g.splitk = 1;
      if (!dry) r = launch_tiled(g, s);
      tile = -1;
    }
    last_tile = tile; last_splitk = S;
    ar.off = mark;
    return r;
  }
  int add_ln(float* x, const float* delta, const float* g, const float* b, int rows, int H, bf16_t* y_bf, float* y_f32) {
    if (err) return err;
    if (dry) return 0;
    return launch_add_ln(x, delta, g, b, rows, H, eps, y_bf, y_f32, s);
  }
};

size_t cnt_bytes(int cnt) { return align256((size_t)cnt * 4); }

// the activations of the layer schedule, allocated in this order
struct ClipBufs {
  float* xs;       // residual stream [M][H]
  float* dl;       // fp32 result of the projection that feeds it
  bf16_t *h, *qkv, *at;
  float* f1;
  bf16_t* g1;
  void alloc(ClipCtx& x, int M, int H, int I) {
    xs = x.alloc<float>((size_t)M * H);
    dl = x.alloc<float>((size_t)M * H);
    h = x.alloc<bf16_t>((size_t)M * H);
    qkv = x.alloc<bf16_t>((size_t)M * 3 * H);
    at = x.alloc<bf16_t>((size_t)M * H);
    f1 = x.alloc<float>((size_t)M * I);
    g1 = x.alloc<bf16_t>((size_t)M * I);
  }
};

// `layers` layers over b.xs (complete on entry); on return b.dl holds the last fc2 result, not yet added (layers > 0).
// attn(qkv, at): the tower's attention over the fused [M][3H] q | k | v rows (q prescaled at pack time) -> at [M][H];
// called on real runs only.  Slots: layers.N.{ln1,ln2}.{g,b}, layers.N.{qkv,out,fc1,fc2}.{w,b}.
template <class Attn>
int clip_layers(ClipCtx& x, const ClipBufs& b, int layers, int H, int I, int M, int act, Attn&& attn) {
  for (int l = 0; l < layers; ++l) {
    const std::string p = "layers." + std::to_string(l);
    const float *g1w = x.WF(p + ".ln1.g", H), *b1w = x.WF(p + ".ln1.b", H), *g2w = x.WF(p + ".ln2.g", H), *b2w = x.WF(p + ".ln2.b", H);
    const bf16_t *wqkv = x.WB(p + ".qkv.w", (int64_t)3 * H * H), *wo = x.WB(p + ".out.w", (int64_t)H * H);
    const bf16_t *w1 = x.WB(p + ".fc1.w", (int64_t)I * H), *w2 = x.WB(p + ".fc2.w", (int64_t)H * I);
    const float *bqkv = x.WF(p + ".qkv.b", 3 * H), *bo = x.WF(p + ".out.b", H), *bf1 = x.WF(p + ".fc1.b", I), *bf2 = x.WF(p + ".fc2.b", H);
    if (x.err) return x.err;
    CHECK(x.add_ln(b.xs, l ? b.dl : nullptr, g1w, b1w, M, H, b.h, nullptr));
    CHECK(x.linear(b.h, H, M, wqkv, bqkv, 3 * H, b.qkv, false));
    if (!x.dry) CHECK(attn(b.qkv, b.at));
    CHECK(x.linear(b.at, H, M, wo, bo, H, b.dl, true));
    CHECK(x.add_ln(b.xs, b.dl, g2w, b2w, M, H, b.h, nullptr));
    CHECK(x.linear(b.h, H, M, w1, bf1, I, b.f1, true));
    if (!x.dry) CHECK(launch_act(b.f1, (long)M * I / 8, act, b.g1, x.s));
    CHECK(x.linear(b.g1, I, M, w2, bf2, H, b.dl, true));
  }
  return x.err;
}

}  // namespace
