// CLIP text transformer (the `last_hidden_state` of transformers' CLIPTextModel) on the hot path's kernels -- SURVEY.md 8f
// row N5: the first stage of MVDPipeline.__call__ (/root/reference/src/models/pipeline.py:52-75, tokenise + text-encode).
//
//   x   = token_embedding[ids] + position_embedding[0:T]
//   per layer:  h = LN1(x); q,k,v = h.Wqkv^T + b;  a = softmax(q.k^T / sqrt(64) + causal).v  per head of 64 channels
//               x = x + a.Wo^T + bo;  h = LN2(x); h = act(h.W1^T + b1); x = x + h.W2^T + b2
//   out = final_layer_norm(x)
//
// The residual stream x stays in fp32 (23 pre-LN layers add into it); GEMM operands are bf16 with fp32 accumulation.  The
// GEMMs are the existing kernels, untouched: a projection that feeds the residual writes its fp32 result (`out_f32`) to a
// delta buffer, and the NEXT kernel -- residual add + LayerNorm in one pass -- folds it into x, so the fp32 residual costs no
// launch of its own and no epilogue mode of the GEMM kernels changes.  fc1 writes fp32 pre-activations, one pass applies
// GELU (erf) / quick-GELU and rounds to the bf16 operand of fc2.  Per layer: add+LN, QKV GEMM, causal attention,
// out-projection, add+LN, fc1, activation, fc2 = 8 launches (plus in-kernel split-K where the small-M planner asks for it).
// The layer schedule and its two elementwise kernels live in clip_layer.h, shared with the image tower (vision.hip).
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <unordered_map>

#include "clip_layer.h"     // add + LayerNorm, the activation pass and the layer schedule, shared with vision.hip

namespace {

// ---------------------------------------------------------------- embedding gather + position add
// one wave per row, 16-byte loads; the id is clamped for address safety only (range validation is the caller's, host side)
__global__ __launch_bounds__(256) void text_embed_kernel(const int* __restrict__ ids, const float* __restrict__ tok, const float* __restrict__ pos,
                                                         int rows, int T, int H, int vocab, float* __restrict__ x) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  int id = ids[row];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const f32x4* tp = reinterpret_cast<const f32x4*>(tok + (size_t)id * H);
  const f32x4* pp = reinterpret_cast<const f32x4*>(pos + (size_t)(row % T) * H);
  f32x4* xp = reinterpret_cast<f32x4*>(x + (size_t)row * H);
  for (int c = lane; c < H / 4; c += 64) xp[c] = tp[c] + pp[c];
}

// ---------------------------------------------------------------- causal attention, n <= 96 keys, d = 64
// One workgroup (4 waves) per (batch, head): q, k and v^T of the whole problem sit in LDS (61 KB with the probability tile),
// zero filled up to the MFMA tile.  Wave w owns the 16-query row tiles w and w + 4: scores of the tiles at or left of the
// diagonal by v_mfma_f32_16x16x32_bf16 (A = q rows, B = k rows: D[query][key], a lane holds 4 queries x 1 key per tile), the
// causal mask on the diagonal tile, fp32 softmax in the exp2 domain with the row reductions across the 16 lanes that share
// a query, P as bf16 through LDS (A operand of P.V wants keys along k), P.V against v^T rows, 1 / denominator applied to
// the fp32 result.  Keys beyond the query never reach a result: masked scores become exactly 0 and v is zero beyond n, so
// 0 * v adds nothing (padded keys j >= n are > every live query and fall under the same mask); padded query rows are
// computed and never stored.
constexpr int CA_NP = 96, CA_LDQ = 72, CA_LDP = 104;     // row strides (bf16) padded off the 128-byte bank period, 16-byte multiples
__global__ __launch_bounds__(256) void text_attn_causal_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                                                               bf16_t* __restrict__ o, int heads, int n, int ldq, int ldk, int ldv, int ldo,
                                                               float scale_log2) {
  __shared__ __attribute__((aligned(16))) bf16_t sQ[CA_NP * CA_LDQ];
  __shared__ __attribute__((aligned(16))) bf16_t sK[CA_NP * CA_LDQ];
  __shared__ __attribute__((aligned(16))) bf16_t sVt[64 * CA_LDP];
  __shared__ __attribute__((aligned(16))) bf16_t sP[CA_NP * CA_LDP];
  const int b = blockIdx.x / heads, hd = blockIdx.x - b * heads;
  const size_t row0 = (size_t)b * n;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = (n + 15) >> 4;                 // live 16-row tiles (<= 6)
  const int np32 = ((nt + 1) >> 1) * 32;        // rows staged: P.V walks the keys 32 at a time (<= 96)
  for (int c = tid; c < np32 * 8; c += 256) {
    const int r = c >> 3, c8 = (c & 7) * 8;
    u32x4 qv = {0u, 0u, 0u, 0u}, kv = qv, vv = qv;
    if (r < n) {
      qv = *reinterpret_cast<const u32x4*>(q + (row0 + r) * ldq + hd * 64 + c8);
      kv = *reinterpret_cast<const u32x4*>(k + (row0 + r) * ldk + hd * 64 + c8);
      vv = *reinterpret_cast<const u32x4*>(v + (row0 + r) * ldv + hd * 64 + c8);
    }
    *reinterpret_cast<u32x4*>(sQ + r * CA_LDQ + c8) = qv;
    *reinterpret_cast<u32x4*>(sK + r * CA_LDQ + c8) = kv;
#pragma unroll
    for (int e = 0; e < 8; ++e) sVt[(c8 + e) * CA_LDP + r] = (bf16_t)(vv[e >> 1] >> ((e & 1) * 16));
  }
  __syncthreads();
  const int fr = lane & 15, fq = lane >> 4;
#pragma unroll 1
  for (int it = 0; it < 2; ++it) {
    const int i = wave + 4 * it;                // this wave's row tile (wave-uniform)
    const bool live = i < nt;
    float inv[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) {
      bf16x8 qa[2];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) qa[kk] = *reinterpret_cast<const bf16x8*>(sQ + (i * 16 + fr) * CA_LDQ + kk * 32 + fq * 8);
      f32x4 s[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (j <= i) {
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            const bf16x8 kb = *reinterpret_cast<const bf16x8*>(sK + (j * 16 + fr) * CA_LDQ + kk * 32 + fq * 8);
            s[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[kk], kb, s[j], 0, 0, 0);
          }
        }
      }
      // s[j][r]: query i*16 + fq*4 + r, key j*16 + fr
      float mx[4] = {-3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f};
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        if (j <= i) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float t = s[j][r] * scale_log2;
            if (j == i && fr > fq * 4 + r) t = -3.0e38f;
            s[j][r] = t;
            mx[r] = fmaxf(mx[r], t);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) mx[r] = fmaxf(mx[r], __shfl_xor(mx[r], d, 64));
      }
      float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        if (j <= i) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float p = exp2f(s[j][r] - mx[r]);
            sum[r] += p;
            sP[(i * 16 + fq * 4 + r) * CA_LDP + j * 16 + fr] = f2bf(p);
          }
        }
      }
      if (!(i & 1)) {                           // an odd number of key tiles: the second half of the last 32-key step is zero
#pragma unroll
        for (int r = 0; r < 4; ++r) sP[(i * 16 + fq * 4 + r) * CA_LDP + (i + 1) * 16 + fr] = 0;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) sum[r] += __shfl_xor(sum[r], d, 64);
        inv[r] = 1.0f / sum[r];
      }
    }
    __syncthreads();
    if (live) {
      const int nks = (i + 2) >> 1;             // 32-key steps covering keys 0 .. 16 (i + 1) - 1
      f32x4 acc[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 3; ++ks) {
        if (ks < nks) {
          const bf16x8 pa = *reinterpret_cast<const bf16x8*>(sP + (i * 16 + fr) * CA_LDP + ks * 32 + fq * 8);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const bf16x8 vb = *reinterpret_cast<const bf16x8*>(sVt + (c * 16 + fr) * CA_LDP + ks * 32 + fq * 8);
            acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, vb, acc[c], 0, 0, 0);
          }
        }
      }
      // acc[c][r]: query i*16 + fq*4 + r, channel c*16 + fr
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = i * 16 + fq * 4 + r;
        if (row < n) {
          bf16_t* op = o + (row0 + row) * ldo + hd * 64 + fr;
#pragma unroll
          for (int c = 0; c < 4; ++c) op[c * 16] = f2bf(acc[c][r] * inv[r]);
        }
      }
    }
  }
}

int launch_attn_causal(const bf16_t* q, const bf16_t* k, const bf16_t* v, bf16_t* o, int batch, int heads, int n, int ldq, int ldk, int ldv,
                       int ldo, float scale, hipStream_t s) {
  if (!q || !k || !v || !o || batch <= 0 || heads <= 0 || n <= 0) { mvd_set_error("attention_causal: bad argument"); return -1; }
  if (n > CA_NP) { mvd_set_error("attention_causal: n = %d exceeds %d keys", n, CA_NP); return -1; }
  if ((ldq | ldk | ldv) % 8 || ldq < heads * 64 || ldk < heads * 64 || ldv < heads * 64 || ldo < heads * 64) {
    mvd_set_error("attention_causal: row strides must cover heads * 64 channels (q / k / v: multiples of 8)"); return -1;
  }
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) { mvd_set_error("attention_causal: q / k / v must be 16-byte aligned"); return -1; }
  if ((long)batch * heads > 0x7fffffffL) { mvd_set_error("attention_causal: grid too large"); return -1; }
  // scale == 0: q already carries softmax_scale * log2(e) (the packed q rows, as for mvd_op_attention)
  const float sl = scale == 0.f ? 1.0f : scale * 1.4426950408889634f;
  hipLaunchKernelGGL(text_attn_causal_kernel, dim3(batch * heads), dim3(256), 0, s, q, k, v, o, heads, n, ldq, ldk, ldv, ldo, sl);
  return launch_check("attention_causal");
}

}  // namespace

struct mvd_text : ModuleBase {      // (ar unused: the arena of a run lives in its ClipCtx, behind the split-K tile counters)
  mvd_text_config_t cfg;
};

namespace {

// dry: sizes only (x.ar.high, x.cnt_used); otherwise `cnt` = the counter words the dry run asked for
int encode_impl(mvd_text* t, const int* ids, int B, int T, float* out, hipStream_t s, bool dry, int cnt, size_t* high_out, int* cnt_out,
                bool check_w = true) {
  const mvd_text_config_t& c = t->cfg;
  const int H = c.hidden_size, I = c.intermediate_size, M = B * T;
  ClipCtx x{&t->w, "text: ", c.layer_norm_eps, s, dry};
  x.check_w = check_w; x.ar.dry = dry;
  if (!dry) {
    x.cnt_base = reinterpret_cast<unsigned int*>(t->ws_ptr);
    x.ar.base = reinterpret_cast<char*>(t->ws_ptr) + cnt_bytes(cnt);
    if (cnt > 0 && hipMemsetAsync(x.cnt_base, 0, (size_t)cnt * 4, s) != hipSuccess) { mvd_set_error("text_encode: hipMemsetAsync failed"); return -3; }
  }
  ClipBufs b;
  b.alloc(x, M, H, I);
  const float* tok = x.WF("tok", (int64_t)c.vocab_size * H);
  const float* pos = x.WF("pos", (int64_t)c.max_positions * H);
  if (x.err) return x.err;
  if (!dry) {
    hipLaunchKernelGGL(text_embed_kernel, dim3((M + 3) / 4), dim3(256), 0, s, ids, tok, pos, M, T, H, c.vocab_size, b.xs);
    CHECK(launch_check("text embedding"));
  }
  CHECK(clip_layers(x, b, c.num_layers, H, I, M, c.act, [&](const bf16_t* qkv, bf16_t* at) {
    return launch_attn_causal(qkv, qkv + H, qkv + 2 * H, at, B, c.num_heads, T, 3 * H, 3 * H, 3 * H, H, 0.f, s);   // q rows prescaled at pack time
  }));
  const float *gf = x.WF("final_ln.g", H), *bf = x.WF("final_ln.b", H);
  if (x.err) return x.err;
  CHECK(x.add_ln(b.xs, c.num_layers ? b.dl : nullptr, gf, bf, M, H, nullptr, out));
  if (high_out) *high_out = x.ar.high;
  if (cnt_out) *cnt_out = x.cnt_used;
  return x.err;
}

int check_shape(mvd_text* t, int batch, int seq_len, const char* who) {
  if (batch <= 0 || seq_len <= 0) { mvd_set_error("%s: bad shape (batch %d, seq_len %d)", who, batch, seq_len); return -1; }
  if (seq_len > t->cfg.max_positions) { mvd_set_error("%s: seq_len %d exceeds max_positions %d", who, seq_len, t->cfg.max_positions); return -1; }
  if ((long)batch * seq_len > (1L << 20)) { mvd_set_error("%s: batch %d x seq_len %d rows is beyond what one call takes", who, batch, seq_len); return -1; }
  return 0;
}

// ClipCtx::linear on caller buffers: ws = [split-K tile counters | partials], the counters zeroed as encode_impl zeroes them
int debug_linear(const bf16_t* a, int K, int M, const bf16_t* w, const float* bias, int N, void* out, bool out_f32, void* ws, hipStream_t s,
                        bool dry, int cnt, size_t* bytes_out, int* cnt_out, int* route_out = nullptr) {
  ClipCtx x{nullptr, "clip_linear: ", 1e-5f, s, dry};
  x.check_w = false; x.ar.dry = dry;
  if (!dry) {
    x.cnt_base = reinterpret_cast<unsigned int*>(ws);
    x.ar.base = reinterpret_cast<char*>(ws) + cnt_bytes(cnt);
    if (cnt > 0 && hipMemsetAsync(x.cnt_base, 0, (size_t)cnt * 4, s) != hipSuccess) { mvd_set_error("clip_linear: hipMemsetAsync failed"); return -3; }
  }
  CHECK(x.linear(a, K, M, w, bias, N, out, out_f32));
  if (bytes_out) *bytes_out = cnt_bytes(x.cnt_used) + x.ar.high;
  if (cnt_out) *cnt_out = x.cnt_used;
  if (route_out) { route_out[0] = x.last_tile; route_out[1] = x.last_splitk; }
  return 0;
}
int debug_linear_shape(int M, int N, int K) {
  if (M <= 0 || M > (1 << 20) || N <= 0 || N % 64 || K <= 0 || K % 64) { mvd_set_error("clip_linear: bad shape (M %d, N %d, K %d): N and K must be multiples of 64", M, N, K); return -1; }
  return 0;
}

}  // namespace

extern "C" {

int mvd_text_create(const mvd_text_config_t* cfg, mvd_text_t** out) {
  if (!cfg || !out) { mvd_set_error("text_create: null argument"); return -1; }
  if (cfg->num_heads <= 0 || cfg->hidden_size != cfg->num_heads * 64) { mvd_set_error("text_create: hidden_size %d / num_heads %d: the head dimension must be 64", cfg->hidden_size, cfg->num_heads); return -1; }
  if (cfg->hidden_size % 64 || cfg->hidden_size > LN_MAXCH * 256) { mvd_set_error("text_create: hidden_size %d must be a multiple of 64, at most %d", cfg->hidden_size, LN_MAXCH * 256); return -1; }
  if (cfg->intermediate_size <= 0 || cfg->intermediate_size % 64) { mvd_set_error("text_create: intermediate_size %d must be a multiple of 64", cfg->intermediate_size); return -1; }
  if (cfg->max_positions <= 0 || cfg->max_positions > CA_NP) { mvd_set_error("text_create: max_positions %d must be in 1..%d", cfg->max_positions, CA_NP); return -1; }
  if (cfg->act != 0 && cfg->act != 1) { mvd_set_error("text_create: act %d (0 gelu, 1 quick_gelu)", cfg->act); return -1; }
  if (cfg->vocab_size <= 0 || cfg->num_layers < 0 || !(cfg->layer_norm_eps > 0.f)) { mvd_set_error("text_create: bad vocab_size / num_layers / layer_norm_eps"); return -1; }
  mvd_text* t = new mvd_text();
  t->cfg = *cfg;
  *out = t;
  return 0;
}
int mvd_text_destroy(mvd_text_t* t) { delete t; return 0; }

int mvd_text_set_weight(mvd_text_t* t, const char* slot, const void* ptr, int64_t numel, int dtype) {
  return module_set_weight(t, "text", slot, ptr, numel, dtype);
}

int64_t mvd_text_workspace_bytes(mvd_text_t* t, int batch, int seq_len) {
  if (!t) { mvd_set_error("text_workspace_bytes: null handle"); return -1; }
  if (int r = check_shape(t, batch, seq_len, "text_workspace_bytes")) return r;
  size_t high = 0; int cnt = 0;
  if (int r = encode_impl(t, nullptr, batch, seq_len, nullptr, nullptr, true, 0, &high, &cnt, false)) return r;   // (sizes do not depend on the weights)
  return (int64_t)(cnt_bytes(cnt) + high + 4096);
}

int mvd_text_bind_workspace(mvd_text_t* t, void* ws, int64_t bytes) {
  return module_bind_workspace(t, "text", ws, bytes, 0);
}

int mvd_text_encode(mvd_text_t* t, const int32_t* ids, int batch, int seq_len, float* out, void* stream) {
  if (!t || !ids || !out) { mvd_set_error("text_encode: null argument"); return -1; }
  if (int r = check_shape(t, batch, seq_len, "text_encode")) return r;
  size_t high = 0; int cnt = 0;
  if (int r = encode_impl(t, nullptr, batch, seq_len, nullptr, nullptr, true, 0, &high, &cnt)) return r;   // weights and sizes first: nothing is launched on a failure
  if (!t->ws_ptr) { mvd_set_error("text_encode: workspace not bound"); return -1; }
  if (cnt_bytes(cnt) + high > (size_t)t->ws_bytes) { mvd_set_error("text_encode: workspace too small: need %zu bytes, bound %lld", cnt_bytes(cnt) + high, (long long)t->ws_bytes); return -4; }
  return encode_impl(t, ids, batch, seq_len, out, (hipStream_t)stream, false, cnt, nullptr, nullptr);
}

int mvd_op_attention_causal(const void* q, const void* k, const void* v, void* o, int batch, int heads, int n, int ldq, int ldk, int ldv,
                            int ldo, float scale, void* stream) {
  return launch_attn_causal((const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o, batch, heads, n, ldq, ldk, ldv, ldo, scale,
                            (hipStream_t)stream);
}

int mvd_op_text_add_ln(float* x, const float* delta, const float* gamma, const float* beta, int rows, int H, float eps, void* y_bf16, float* y_f32,
                       void* stream) {
  return op_add_ln("text_add_ln", x, delta, gamma, beta, rows, H, eps, y_bf16, y_f32, (hipStream_t)stream);
}

int mvd_op_text_act(const float* x, int64_t n, int act, void* y_bf16, void* stream) { return op_act("text_act", x, n, act, y_bf16, (hipStream_t)stream); }

int mvd_op_text_embed(const int32_t* ids, const float* tok, const float* pos, int rows, int T, int H, int vocab, float* x, void* stream) {
  if (!ids || !tok || !pos || !x) { mvd_set_error("text_embed: null argument"); return -1; }
  if (rows <= 0 || rows > (1 << 24) || T <= 0 || vocab <= 0 || H < 4 || H % 4) { mvd_set_error("text_embed: bad shape (rows %d, T %d, H %d, vocab %d): H must be a multiple of 4", rows, T, H, vocab); return -1; }
  if (((uintptr_t)tok | (uintptr_t)pos | (uintptr_t)x) & 15) { mvd_set_error("text_embed: tok, pos and x must be 16-byte aligned"); return -1; }
  hipLaunchKernelGGL(text_embed_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, ids, tok, pos, rows, T, H, vocab, x);
  return launch_check("text embedding");
}

int64_t mvd_debug_clip_linear_ws_bytes(int M, int N, int K, int out_f32) {
  CHECK(debug_linear_shape(M, N, K));
  size_t bytes = 0;
  CHECK(debug_linear((const bf16_t*)0x1000, K, M, (const bf16_t*)0x1000, nullptr, N, (void*)0x1000, out_f32 != 0, nullptr, nullptr, true, 0, &bytes, nullptr));
  return (int64_t)bytes + 256;
}

int mvd_debug_clip_linear(const void* a, int K, int M, const void* w, const float* bias, int N, void* out, int out_f32, void* ws, int64_t ws_bytes,
                          int* route_out, void* stream) {
  if (!a || !w || !out) { mvd_set_error("clip_linear: null argument"); return -1; }
  CHECK(debug_linear_shape(M, N, K));
  if (((uintptr_t)a | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)out) & 15) { mvd_set_error("clip_linear: a, w, bias and out must be 16-byte aligned"); return -1; }
  size_t bytes = 0; int cnt = 0;
  CHECK(debug_linear((const bf16_t*)a, K, M, (const bf16_t*)w, bias, N, out, out_f32 != 0, nullptr, nullptr, true, 0, &bytes, &cnt));
  if (bytes > 0 && (!ws || ((uintptr_t)ws & 255) || (size_t)ws_bytes < bytes)) { mvd_set_error("clip_linear: workspace: need %zu bytes, 256-byte aligned (given %lld)", bytes, (long long)ws_bytes); return -4; }
  return debug_linear((const bf16_t*)a, K, M, (const bf16_t*)w, bias, N, out, out_f32 != 0, ws, (hipStream_t)stream, false, cnt, nullptr, nullptr, route_out);
}

}  // extern "C"
