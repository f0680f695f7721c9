// Small / elementwise kernels of the MVD hot path: layout conversion, FiLM, conv_in,
// conv_out, timestep + camera embeddings and the skinny fp32 linears of the camera MLPs.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include "host_util.h"

static thread_local char g_err[512] = "";
void mvd_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* mvd_last_error(void) { return g_err; }

namespace {

__global__ void nchw_to_nhwc_kernel(const float* __restrict__ x, int c, int hw, const float* __restrict__ scale,
                                    const float* __restrict__ shift, int ld_ss, bf16_t* __restrict__ y, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // over (b, p, ch)
  if (i >= total) return;
  const int ch = i % c;
  const long bp = i / c;
  const int p = bp % hw;
  const int b = bp / hw;
  float v = x[((size_t)b * c + ch) * hw + p];
  if (scale) v = v * scale[(size_t)b * ld_ss + ch] + shift[(size_t)b * ld_ss + ch];
  y[i] = f2bf(v);
}

__global__ void nhwc_to_nchw_f32_kernel(const bf16_t* __restrict__ x, int hw, int c, float* __restrict__ y, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // over (b, ch, p) output order
  if (i >= total) return;
  const int p = i % hw;
  const long bc = i / hw;
  const int ch = bc % c;
  const int b = bc / c;
  y[i] = bf2f(x[((size_t)b * hw + p) * c + ch]);
}

__global__ void film_kernel(const bf16_t* __restrict__ x, int hw, int c, const float* __restrict__ scale,
                            const float* __restrict__ shift, int ld_ss, bf16_t* __restrict__ y, long nvec) {
  const int vec = c >> 3;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < nvec; e += (long)gridDim.x * blockDim.x) {
    const int v = e % vec;
    const long bp = e / vec;
    const int b = bp / hw;
    const u32x4 in = *reinterpret_cast<const u32x4*>(x + e * 8);
    const float* sc = scale + (size_t)b * ld_ss + v * 8;
    const float* sf = shift + (size_t)b * ld_ss + v * 8;
    u32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      o[j] = pack2bf(fmaf(bflo(in[j]), sc[2 * j], sf[2 * j]), fmaf(bfhi(in[j]), sc[2 * j + 1], sf[2 * j + 1]));
    *reinterpret_cast<u32x4*>(y + e * 8) = o;
  }
}

// conv_in: thread = (pixel, 8 output channels)
__global__ void conv_in_kernel(const bf16_t* __restrict__ x, int h, int w, int cin, const float* __restrict__ wt,
                               const float* __restrict__ bias, int cout, bf16_t* __restrict__ y, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int ng = cout >> 3;
  const int g = i % ng;
  const long bp = i / ng;
  const int hw = h * w;
  const int p = bp % hw;
  const int b = bp / hw;
  const int oy = p / w, ox = p % w;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = bias[g * 8 + j];
  for (int tap = 0; tap < 9; ++tap) {
    const int iy = oy + tap / 3 - 1, ix = ox + tap % 3 - 1;
    if ((unsigned)iy >= (unsigned)h || (unsigned)ix >= (unsigned)w) continue;
    const bf16_t* xp = x + ((size_t)b * hw + iy * w + ix) * cin;
    for (int ci = 0; ci < cin; ++ci) {
      const float xv = bf2f(xp[ci]);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = fmaf(xv, wt[((size_t)(g * 8 + j) * 9 + tap) * cin + ci], acc[j]);
    }
  }
  u32x4 o = {pack2bf(acc[0], acc[1]), pack2bf(acc[2], acc[3]), pack2bf(acc[4], acc[5]), pack2bf(acc[6], acc[7])};
  *reinterpret_cast<u32x4*>(y + bp * cout + g * 8) = o;
}

// (Round 3 tried four adjacent pixels per wave -- 2-3x fewer loads -- and went back: correct in every single-process test,
//  but with a second process on the same GPU (the two-rank bench rehearsal) 2-15 isolated output elements, always the third
//  pixel of a quad, differed between two forwards of the same inputs in 9 of 17 runs; this form: 0 of 5.  Not understood;
//  conv_out is 0.3 % of a 32-pair step.)
// conv_out: one wave per output pixel, lanes split K = 9*C in 16-byte chunks
__global__ __launch_bounds__(256) void conv_out_kernel(const bf16_t* __restrict__ x, int batch, int h, int w, int c,
                                                        const bf16_t* __restrict__ wt, const float* __restrict__ bias,
                                                        int cout, float* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const long pix = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int hw = h * w;
  if (pix >= (long)batch * hw) return;
  const int b = pix / hw, p = pix % hw;
  const int oy = p / w, ox = p % w;
  const int vec = c >> 3;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (int q = lane; q < 9 * vec; q += 64) {
    const int tap = q / vec, v = q % vec;
    const int iy = oy + tap / 3 - 1, ix = ox + tap % 3 - 1;
    if ((unsigned)iy >= (unsigned)h || (unsigned)ix >= (unsigned)w) continue;
    const u32x4 xv = *reinterpret_cast<const u32x4*>(x + ((size_t)b * hw + iy * w + ix) * c + v * 8);
#pragma unroll
    for (int co = 0; co < 8; ++co) {
      if (co < cout) {
        const u32x4 wv = *reinterpret_cast<const u32x4*>(wt + ((size_t)co * 9 + tap) * c + v * 8);
        float a = acc[co];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          a = fmaf(bflo(xv[j]), bflo(wv[j]), a);
          a = fmaf(bfhi(xv[j]), bfhi(wv[j]), a);
        }
        acc[co] = a;
      }
    }
  }
#pragma unroll
  for (int co = 0; co < 8; ++co) {
    if (co < cout) {
      const float t = wave_sum(acc[co]);
      if (lane == 0) y[((size_t)b * cout + co) * hw + p] = t + bias[co];
    }
  }
}

__global__ void f32_to_bf16_kernel(const float* __restrict__ x, long n, bf16_t* __restrict__ y) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) y[i] = f2bf(x[i]);
}

// skinny linear (camera / time MLPs, fp32 activations): one wave per output feature, the weight row is read
// ONCE per 32 batch rows (it was the dominant cost at batch 32), 16-byte loads when K % 4 == 0
template <bool WBF16>
__global__ __launch_bounds__(256) void skinny_linear_kernel(const float* __restrict__ x, int ldx, int batch, int k,
                                                             const void* __restrict__ wv, const float* __restrict__ bias,
                                                             int n, int act_in, float* __restrict__ y, int ldy) {
  constexpr int BC = 32;
  const int lane = threadIdx.x & 63;
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (o >= n) return;
  const bool vec = !WBF16 && (k & 3) == 0 && (ldx & 3) == 0;
  for (int b0 = 0; b0 < batch; b0 += BC) {
    float acc[BC];
#pragma unroll
    for (int j = 0; j < BC; ++j) acc[j] = 0.f;
    if (vec) {
      const float* wr = reinterpret_cast<const float*>(wv) + (size_t)o * k;
      for (int kk = lane * 4; kk < k; kk += 256) {
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(wr + kk);
#pragma unroll
        for (int j = 0; j < BC; ++j) {
          if (b0 + j < batch) {
            f32x4 x4 = *reinterpret_cast<const f32x4*>(x + (size_t)(b0 + j) * ldx + kk);
            if (act_in == 1) { x4[0] = silu_f(x4[0]); x4[1] = silu_f(x4[1]); x4[2] = silu_f(x4[2]); x4[3] = silu_f(x4[3]); }
            acc[j] = fmaf(x4[0], w4[0], fmaf(x4[1], w4[1], fmaf(x4[2], w4[2], fmaf(x4[3], w4[3], acc[j]))));
          }
        }
      }
    } else {
      for (int kk = lane; kk < k; kk += 64) {
        float wgt;
        if (WBF16) wgt = bf2f(reinterpret_cast<const bf16_t*>(wv)[(size_t)o * k + kk]);
        else wgt = reinterpret_cast<const float*>(wv)[(size_t)o * k + kk];
#pragma unroll
        for (int j = 0; j < BC; ++j) {
          if (b0 + j < batch) {
            float xv = x[(size_t)(b0 + j) * ldx + kk];
            if (act_in == 1) xv = silu_f(xv);
            acc[j] = fmaf(xv, wgt, acc[j]);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < BC; ++j) {
      if (b0 + j < batch) {
        const float t = wave_sum(acc[j]);
        if (lane == 0) y[(size_t)(b0 + j) * ldy + o] = t + (bias ? bias[o] : 0.f);
      }
    }
  }
}

// Vectorised form: one wave computes F output features for up to 32 batch rows, so every x element fetched serves F
// weight rows (the x re-reads from L2 dominated the one-feature kernel); 16-byte loads of both operands.
// GROUPED: output feature o reads the input segment x + g * xseg, g = the first segment with o < seg.end[g] (segment ends are
// multiples of F, so a wave's F features share a segment).
template <bool WBF16, int F, bool GROUPED = false>
__global__ __launch_bounds__(256) void skinny_linear_vec_kernel(const float* __restrict__ x, int ldx, int batch, int k,
                                                                 const void* __restrict__ wv, const float* __restrict__ bias,
                                                                 int n, int act_in, float* __restrict__ y, int ldy,
                                                                 const MvdSegTable seg = MvdSegTable{}, int xseg = 0) {
  constexpr int BC = 32;
  constexpr int KV = WBF16 ? 8 : 4;          // k elements per lane per iteration (16 bytes of weight)
  const int lane = threadIdx.x & 63;
  const int o0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * F;
  if (o0 >= n) return;
  if constexpr (GROUPED) {
    int g = 0;
    while (g + 1 < seg.n && o0 >= seg.end[g]) ++g;
    x += (size_t)g * xseg;
  }
  for (int b0 = 0; b0 < batch; b0 += BC) {
    float acc[BC][F];
#pragma unroll
    for (int j = 0; j < BC; ++j)
#pragma unroll
      for (int f = 0; f < F; ++f) acc[j][f] = 0.f;
    for (int kk = lane * KV; kk < k; kk += 64 * KV) {
      float w[F][KV];
#pragma unroll
      for (int f = 0; f < F; ++f) {
        const int o = o0 + f < n ? o0 + f : n - 1;
        if (WBF16) {
          const u32x4 r = *reinterpret_cast<const u32x4*>(reinterpret_cast<const bf16_t*>(wv) + (size_t)o * k + kk);
#pragma unroll
          for (int e = 0; e < 4; ++e) { w[f][2 * e] = bflo(r[e]); w[f][2 * e + 1] = bfhi(r[e]); }
        } else {
          const f32x4 r = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(wv) + (size_t)o * k + kk);
#pragma unroll
          for (int e = 0; e < 4; ++e) w[f][e] = r[e];
        }
      }
#pragma unroll
      for (int j = 0; j < BC; ++j) {
        const int jr = b0 + j < batch ? b0 + j : batch - 1;      // rows past the batch repeat the last one (never stored):
        float xv[KV];                                            // no branch in the loop, the 32 row loads issue back to back
#pragma unroll
        for (int q = 0; q < KV / 4; ++q) {
          const f32x4 x4 = *reinterpret_cast<const f32x4*>(x + (size_t)jr * ldx + kk + 4 * q);
#pragma unroll
          for (int e = 0; e < 4; ++e) xv[4 * q + e] = act_in == 1 ? silu_f(x4[e]) : x4[e];
        }
#pragma unroll
        for (int f = 0; f < F; ++f)
#pragma unroll
          for (int e = 0; e < KV; ++e) acc[j][f] = fmaf(xv[e], w[f][e], acc[j][f]);
      }
    }
#pragma unroll
    for (int j = 0; j < BC; ++j) {
      if (b0 + j < batch) {
#pragma unroll
        for (int f = 0; f < F; ++f) {
          const float t = wave_sum(acc[j][f]);
          if (lane == 0 && o0 + f < n) y[(size_t)(b0 + j) * ldy + o0 + f] = t + (bias ? bias[o0 + f] : 0.f);
        }
      }
    }
  }
}

// Matrix-pipe form (round 5): y[b][o] = sum_k act(x[b][k]) * W[o][k] + bias[o] in FULL fp32 (v_mfma_f32_32x32x2_f32: the camera
// path stays fp32, Q9) for the camera / time MLPs of the front matter -- ~30 launches in front of the main pass, on the step's
// critical path.  The vector form above gives a wave 2 features x 32 rows (it works on 32 rows whatever the batch is), reloads
// every x element per feature pair and ends in 64 six-step wave reductions: 150 us alone for the grouped modulator layer
// (14088 x 512 weights, 32 rows), 390 us beside the encoder pass's persistent kernels.
// Here a workgroup owns 32 output features x 32 batch rows; its four waves split K (wave w takes the 8-float chunks c = w mod 4;
// 16 bf16 for WBF16) and are summed through LDS in wave order (bit-deterministic).  MFMA operands: A = W (row = feature),
// B = x^T (column = batch row): lane l supplies W[o0 + (l & 31)][k] and x[b0 + (l & 31)][k] for k = chunk + 4 (l >> 5) + t,
// t = 0..3, i.e. ONE 16-byte load per operand and lane feeds four MFMAs (any pairing of k values is a valid contraction as long
// as A and B agree).  D: lane (j = l & 31, h = l >> 5) holds features o0 + 8 q + 4 h + (r & 3), q = r >> 2, of batch row b0 + j.
// GROUPED as above (a tile's 32 features must share a segment: the launcher checks that segment ends are multiples of 32).
template <bool WBF16, bool GROUPED>
__global__ __launch_bounds__(256) void skinny_mfma_kernel(const float* __restrict__ x, int ldx, int batch, int k,
                                                           const void* __restrict__ wv, const float* __restrict__ bias, int n, int act_in,
                                                           float* __restrict__ y, int ldy, const MvdSegTable seg, int xseg) {
  typedef __attribute__((ext_vector_type(16))) float f32x16;
  __shared__ f32x16 red[3][64];
  constexpr int KS = WBF16 ? 16 : 8;                 // k elements a wave consumes per iteration (both lane halves together)
  constexpr int KL = KS / 2;                         // per lane
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 31, h = lane >> 5;
  const int o0 = blockIdx.x * 32;
  if constexpr (GROUPED) {
    int g = 0;
    while (g + 1 < seg.n && o0 >= seg.end[g]) ++g;
    x += (size_t)g * xseg;
  }
  const int o = o0 + li < n ? o0 + li : n - 1;       // features past n repeat the last one (never stored)
  for (int b0 = 0; b0 < batch; b0 += 32) {
    const int jr = b0 + li < batch ? b0 + li : batch - 1;
    const float* xr = x + (size_t)jr * ldx;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // (the trip count is WAVE-UNIFORM: an MFMA must not sit in a branch only half of the lanes take.  At K = 1020 the upper lane half
    //  has no last half chunk: such lanes re-load the lower half's chunk and multiply it by zero weights.)
#pragma unroll 4
    for (int kc = wave * KS; kc < k; kc += 4 * KS) {
      const bool live = kc + h * KL < k;
      const int kk = live ? kc + h * KL : kc;
      float wf[KL], xf[KL];
      if constexpr (WBF16) {
        const u32x4 r = *reinterpret_cast<const u32x4*>(reinterpret_cast<const bf16_t*>(wv) + (size_t)o * k + kk);
#pragma unroll
        for (int e = 0; e < 4; ++e) { wf[2 * e] = live ? bflo(r[e]) : 0.f; wf[2 * e + 1] = live ? bfhi(r[e]) : 0.f; }
      } else {
        const f32x4 r = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(wv) + (size_t)o * k + kk);
#pragma unroll
        for (int e = 0; e < 4; ++e) wf[e] = live ? r[e] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < KL / 4; ++q) {
        const f32x4 x4 = *reinterpret_cast<const f32x4*>(xr + kk + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) xf[4 * q + e] = act_in == 1 ? silu_f(x4[e]) : x4[e];
      }
#pragma unroll
      for (int e = 0; e < KL; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[e], xf[e], acc, 0, 0, 0);
    }
    if (wave) red[wave - 1][lane] = acc;
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int w = 0; w < 3; ++w) {
        const f32x16 t = red[w][lane];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] += t[r];
      }
      if (b0 + li < batch) {
        float* yr = y + (size_t)(b0 + li) * ldy;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int oo = o0 + 8 * (r >> 2) + 4 * h + (r & 3);
          if (oo < n) yr[oo] = acc[r] + (bias ? bias[oo] : 0.f);
        }
      }
    }
    __syncthreads();
  }
}

__global__ void timestep_embedding_kernel(const float* __restrict__ t, int dim, float* __restrict__ y) {
  const int b = blockIdx.x;
  const int half = dim >> 1;
  for (int i = threadIdx.x; i < half; i += blockDim.x) {
    const float f = expf(-9.210340371976184f * (float)i / (float)half);
    const float ang = t[b] * f;
    y[(size_t)b * dim + i] = cosf(ang);
    y[(size_t)b * dim + half + i] = sinf(ang);
  }
}

// relative pose + Fourier features (camera_encoder.py:107-151 of the reference)
__global__ void camera_features_kernel(const float* __restrict__ src, const float* __restrict__ tgt, int cam_rows,
                                       int nfreq, float log_max_freq, float* __restrict__ rflat,
                                       float* __restrict__ enc) {
  const int b = blockIdx.x;
  __shared__ float R[9], T[3];
  const float* s = src + (size_t)b * cam_rows * 4;
  const float* g = tgt + (size_t)b * cam_rows * 4;
  if (threadIdx.x < 9) {
    const int i = threadIdx.x / 3, j = threadIdx.x % 3;
    float a = 0.f;
    for (int kk = 0; kk < 3; ++kk) a += g[i * 4 + kk] * s[j * 4 + kk];  // tR . sR^T
    R[threadIdx.x] = a;
    rflat[(size_t)b * 9 + threadIdx.x] = a;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int i = threadIdx.x;
    float a = g[i * 4 + 3];
    for (int kk = 0; kk < 3; ++kk) a -= R[i * 3 + kk] * s[kk * 4 + 3];
    T[i] = a;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 3 * nfreq; e += blockDim.x) {
    const int ax = e / nfreq, i = e % nfreq;
    const float f = expf(log_max_freq * (float)i / (float)(nfreq - 1));
    const float ang = T[ax] * f;
    enc[(size_t)b * 6 * nfreq + ax * 2 * nfreq + i] = sinf(ang);
    enc[(size_t)b * 6 * nfreq + ax * 2 * nfreq + nfreq + i] = cosf(ang);
  }
}

__global__ void film_params_kernel(const float* __restrict__ raw, int batch, int dim, float strength, float* __restrict__ scale,
                                   float* __restrict__ shift, int total) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int b = (i / dim) % batch, ch = i % dim;   // output rows beyond `batch` repeat the inputs cyclically
  const float s = raw[(size_t)b * 2 * dim + ch], t = raw[(size_t)b * 2 * dim + dim + ch];
  scale[i] = 2.0f * strength / (1.0f + expf(-s));
  shift[i] = t * strength;
}

// conv_in front end: NCHW fp32 latent (+ optional camera FiLM) -> im2col rows [pixel][64] bf16 with
// k = tap*C + ch (tap-major, like the packed conv weights), zero padded to 64, so conv_in runs as a K=64
// MFMA GEMM instead of a scalar convolution.
template <int CIN>
__global__ void im2col_in_kernel(const float* __restrict__ x, int h, int w, const float* __restrict__ scale,
                                 const float* __restrict__ shift, int ld_ss, bf16_t* __restrict__ y, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // pixel index over (b, y, x)
  if (i >= total) return;
  const int hw = h * w;
  const int p = i % hw;
  const int b = i / hw;
  const int oy = p / w, ox = p % w;
  float v[64];
#pragma unroll
  for (int k = 0; k < 64; ++k) v[k] = 0.f;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int iy = oy + tap / 3 - 1, ix = ox + tap % 3 - 1;
    const bool ok = (unsigned)iy < (unsigned)h && (unsigned)ix < (unsigned)w;
#pragma unroll
    for (int ch = 0; ch < CIN; ++ch) {
      if (ok) {
        float t = x[((size_t)b * CIN + ch) * hw + iy * w + ix];
        if (scale) t = t * scale[(size_t)b * ld_ss + ch] + shift[(size_t)b * ld_ss + ch];
        v[tap * CIN + ch] = t;
      }
    }
  }
  u32x4* out = reinterpret_cast<u32x4*>(y + i * 64);
#pragma unroll
  for (int q = 0; q < 8; ++q)
    out[q] = u32x4{pack2bf(v[8 * q], v[8 * q + 1]), pack2bf(v[8 * q + 2], v[8 * q + 3]), pack2bf(v[8 * q + 4], v[8 * q + 5]),
                   pack2bf(v[8 * q + 6], v[8 * q + 7])};
}

__global__ void film_nchw_f32_kernel(const float* __restrict__ x, int c, int hw, const float* __restrict__ scale,
                                     const float* __restrict__ shift, float* __restrict__ y, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long bc = i / hw;   // b*c + ch
  y[i] = fmaf(x[i], scale[bc], shift[bc]);
}

inline int nblk(long n, int t) { return (int)((n + t - 1) / t); }

}  // namespace

int mvd_launch_nchw_to_nhwc(const float* x, int batch, int c, int hw, const float* scale, const float* shift, int ld_ss,
                            bf16_t* y, hipStream_t s) {
  if (!x || !y || batch <= 0 || c <= 0 || hw <= 0 || ((scale == nullptr) != (shift == nullptr))) { mvd_set_error("nchw_to_nhwc: bad arguments"); return -1; }
  const long total = (long)batch * c * hw;
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, x, c, hw, scale, shift, ld_ss, y, total);
  return launch_check("nchw_to_nhwc");
}

int mvd_launch_nhwc_to_nchw_f32(const bf16_t* x, int batch, int hw, int c, float* y, hipStream_t s) {
  if (!x || !y || batch <= 0 || c <= 0 || hw <= 0) { mvd_set_error("nhwc_to_nchw: bad arguments"); return -1; }
  const long total = (long)batch * c * hw;
  hipLaunchKernelGGL(nhwc_to_nchw_f32_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, x, hw, c, y, total);
  return launch_check("nhwc_to_nchw");
}

int mvd_launch_film(const bf16_t* x, int batch, int hw, int c, const float* scale, const float* shift, int ld_ss,
                    bf16_t* y, hipStream_t s) {
  if (!x || !y || !scale || !shift || batch <= 0 || hw <= 0 || c <= 0 || (c % 8)) { mvd_set_error("film: bad arguments"); return -1; }
  const long nvec = (long)batch * hw * (c / 8);
  int grid = nblk(nvec, 256);
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(film_kernel, dim3(grid), dim3(256), 0, s, x, hw, c, scale, shift, ld_ss, y, nvec);
  return launch_check("film");
}

int mvd_launch_conv_in(const bf16_t* x, int batch, int h, int w, int cin, const float* wt, const float* bias, int cout,
                       bf16_t* y, hipStream_t s) {
  if (!x || !y || !wt || !bias || batch <= 0 || h <= 0 || w <= 0 || cin <= 0 || cin > 16 || (cout % 8)) { mvd_set_error("conv_in: bad arguments"); return -1; }
  const long total = (long)batch * h * w * (cout / 8);
  hipLaunchKernelGGL(conv_in_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, x, h, w, cin, wt, bias, cout, y, total);
  return launch_check("conv_in");
}

#ifdef MVD_PROBE
#include <stdio.h>
#include <unistd.h>
#include "probe/conv_out4.inc"
__global__ void word_sum_kernel(const unsigned* __restrict__ p, long n, unsigned long long* out) {
  unsigned long long s = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) s += (unsigned long long)p[i] * (unsigned long long)((i & 1023) + 1);
  atomicAdd(out, s);
}
// MVD_CONV_OUT_CMP: a = four-pixel kernel, b = the SAME kernel launched again behind it, r = the one-pixel kernel, all on the same
// input and with NO host synchronisation; cnt[0] += #(a != b bitwise), cnt[1] += #(|a - r| > tol), cnt[2] += #(|b - r| > tol),
// cnt[3] = index of the last a/b mismatch.  cnt lives in pinned host memory and is read without a synchronise (cumulative).
__global__ void conv_out_cmp_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ r, long n,
                                    float tol, unsigned long long* cnt) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float va = a[i], vb = b[i], vr = r[i];
    if (__float_as_uint(va) != __float_as_uint(vb)) { __hip_atomic_fetch_add(cnt, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); __hip_atomic_store(cnt + 3, (unsigned long long)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
    if (!(fabsf(va - vr) <= tol)) __hip_atomic_fetch_add(cnt + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (!(fabsf(vb - vr) <= tol)) __hip_atomic_fetch_add(cnt + 2, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
#endif

int mvd_launch_conv_out(const bf16_t* x, int batch, int h, int w, int c, const bf16_t* wt, const float* bias, int cout,
                        float* y, hipStream_t s) {
  if (!x || !y || !wt || !bias || batch <= 0 || h <= 0 || w <= 0 || (c % 8) || cout <= 0 || cout > 8) { mvd_set_error("conv_out: bad arguments"); return -1; }
#ifdef MVD_PROBE
  if (MVD_ENV_INT("MVD_CONV_OUT4", 0)) {          // diagnosis of the reverted four-pixel form (probe builds only)
    const long quads = (long)batch * h * ((w + 3) / 4);
    hipLaunchKernelGGL(conv_out4_kernel, dim3(nblk(quads, 4)), dim3(256), 0, s, x, batch, h, w, c, wt, bias, cout, y);
    if (MVD_ENV_INT("MVD_CONV_OUT_HASH", 0)) {
      // word sums of the INPUT, of the four-pixel kernel's output, and of the one-pixel kernel's output on the same input
      // (to a scratch buffer): which of them differs between two forwards of the same arguments?
      static unsigned long long* dsum = nullptr; static float* y1 = nullptr; static size_t y1n = 0;
      const size_t on = (size_t)batch * cout * h * w;
      if (!dsum) (void)hipMalloc(&dsum, 3 * sizeof(unsigned long long));
      if (y1n < on) { if (y1) (void)hipFree(y1); (void)hipMalloc(&y1, on * sizeof(float)); y1n = on; }
      (void)hipMemsetAsync(dsum, 0, 3 * sizeof(unsigned long long), s);
      const long pix1 = (long)batch * h * w;
      hipLaunchKernelGGL(conv_out_kernel, dim3(nblk(pix1, 4)), dim3(256), 0, s, x, batch, h, w, c, wt, bias, cout, y1);
      hipLaunchKernelGGL(word_sum_kernel, dim3(1024), dim3(256), 0, s, reinterpret_cast<const unsigned*>(x), (long)((size_t)batch * h * w * c / 2), dsum);
      hipLaunchKernelGGL(word_sum_kernel, dim3(1024), dim3(256), 0, s, reinterpret_cast<const unsigned*>(y), (long)on, dsum + 1);
      hipLaunchKernelGGL(word_sum_kernel, dim3(1024), dim3(256), 0, s, reinterpret_cast<const unsigned*>(y1), (long)on, dsum + 2);
      unsigned long long hs[3] = {0, 0, 0};
      (void)hipMemcpyAsync(hs, dsum, sizeof(hs), hipMemcpyDeviceToHost, s);
      (void)hipStreamSynchronize(s);
      fprintf(stderr, "conv_out hash pid %d: input %016llx  out(4-pixel) %016llx  out(1-pixel, same input) %016llx\n", (int)getpid(), hs[0], hs[1], hs[2]);
    }
    if (MVD_ENV_INT("MVD_CONV_OUT_CMP", 0)) {
      static unsigned long long* cnt = nullptr; static float* yb = nullptr; static float* yr = nullptr; static size_t yn = 0;
      static unsigned long long seen[3] = {0, 0, 0}; static int calls = 0;
      const size_t on = (size_t)batch * cout * h * w;
      if (!cnt) { (void)hipHostMalloc(&cnt, 4 * sizeof(unsigned long long), hipHostMallocMapped); cnt[0] = cnt[1] = cnt[2] = cnt[3] = 0; }
      if (yn < on) { if (yb) { (void)hipFree(yb); (void)hipFree(yr); } (void)hipMalloc(&yb, on * sizeof(float)); (void)hipMalloc(&yr, on * sizeof(float)); yn = on; }
      hipLaunchKernelGGL(conv_out4_kernel, dim3(nblk(quads, 4)), dim3(256), 0, s, x, batch, h, w, c, wt, bias, cout, yb);
      hipLaunchKernelGGL(conv_out_kernel, dim3(nblk((long)batch * h * w, 4)), dim3(256), 0, s, x, batch, h, w, c, wt, bias, cout, yr);
      hipLaunchKernelGGL(conv_out_cmp_kernel, dim3(256), dim3(256), 0, s, y, yb, yr, (long)on, 1e-3f, cnt);
      ++calls;
      volatile unsigned long long* vc = cnt;
      const unsigned long long c0 = vc[0], c1 = vc[1], c2 = vc[2];
      if (c0 != seen[0] || c1 != seen[1] || c2 != seen[2] || calls == 2 || calls == 20) {
        seen[0] = c0; seen[1] = c1; seen[2] = c2;
        fprintf(stderr, "conv_out cmp pid %d after ~%d calls: first!=second %llu  |first-ref|>1e-3 %llu  |second-ref|>1e-3 %llu  last idx %llu (x mod 4 = %llu)\n",
                (int)getpid(), calls - 1, c0, c1, c2, (unsigned long long)vc[3], (unsigned long long)vc[3] % 4);
      }
    }
    return launch_check("conv_out4");
  }
#endif
  const long pix = (long)batch * h * w;
  hipLaunchKernelGGL(conv_out_kernel, dim3(nblk(pix, 4)), dim3(256), 0, s, x, batch, h, w, c, wt, bias, cout, y);
  return launch_check("conv_out");
}

int mvd_launch_f32_to_bf16(const float* x, int64_t n, bf16_t* y, hipStream_t s) {
  if (!x || !y || n <= 0) { mvd_set_error("f32_to_bf16: bad arguments"); return -1; }
  int grid = nblk(n, 256);
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(grid), dim3(256), 0, s, x, (long)n, y);
  return launch_check("f32_to_bf16");
}

int mvd_launch_skinny_linear(const float* x, int ldx, int batch, int k, const void* w, int wbf16, const float* bias, int n,
                             int act_in, float* y, int ldy, hipStream_t s) {
  if (!x || !w || !y || batch <= 0 || batch > 4096 || k <= 0 || n <= 0 || ldx < k || ldy < n) { mvd_set_error("skinny_linear: bad arguments"); return -1; }
  // vector path: 16-byte aligned rows of both operands (every MLP of the camera / time path except the 9-wide
  // rotation input and misaligned views); two features per wave
  const int kv = wbf16 ? 8 : 4;
  const bool vec = (k % kv) == 0 && (ldx % 4) == 0 && (((uintptr_t)x | (uintptr_t)w) & 15) == 0;
  static const int use_vec = MVD_ENV_INT("MVD_SKINNY_VEC", 1);
  // the matrix-pipe form from 8 rows up (debug flag 8388608: the vector form everywhere, A/B).  Measured, same box: alone (one
  // stream) the 32-row front matter of a forward drops from ~0.75 to ~0.35 ms; beside the encoder pass a launch's time is the wait
  // for a CU whose register file a persistent kernel has filled (grouped layer 389 -> 81 us, time MLPs 145 -> 70 us in situ) and the
  // two-stream step gains nothing measurable (60.85 -> 60.72 ms, noise); at one row the vector form is 0.6 % of a cfg3 step faster
  if (vec && batch >= 8 && !(mvd_debug_flags() & MVD_DBG_SKINNY_VECTOR)) {
    const MvdSegTable none{};
    if (wbf16) hipLaunchKernelGGL((skinny_mfma_kernel<true, false>), dim3(nblk(n, 32)), dim3(256), 0, s, x, ldx, batch, k, w, bias, n, act_in, y, ldy, none, 0);
    else hipLaunchKernelGGL((skinny_mfma_kernel<false, false>), dim3(nblk(n, 32)), dim3(256), 0, s, x, ldx, batch, k, w, bias, n, act_in, y, ldy, none, 0);
    return launch_check("skinny_mfma");
  }
  if (vec && use_vec) {
    constexpr int F = 2;
    const dim3 g(nblk(n, 4 * F));
    if (wbf16) hipLaunchKernelGGL((skinny_linear_vec_kernel<true, F>), g, dim3(256), 0, s, x, ldx, batch, k, w, bias, n, act_in, y, ldy);
    else hipLaunchKernelGGL((skinny_linear_vec_kernel<false, F>), g, dim3(256), 0, s, x, ldx, batch, k, w, bias, n, act_in, y, ldy);
    return launch_check("skinny_linear");
  }
  if (wbf16) hipLaunchKernelGGL(skinny_linear_kernel<true>, dim3(nblk(n, 4)), dim3(256), 0, s, x, ldx, batch, k, w, bias, n, act_in, y, ldy);
  else hipLaunchKernelGGL(skinny_linear_kernel<false>, dim3(nblk(n, 4)), dim3(256), 0, s, x, ldx, batch, k, w, bias, n, act_in, y, ldy);
  return launch_check("skinny_linear");
}

int mvd_launch_skinny_linear_grouped(const float* x, int ldx, int xseg, int batch, int k, const float* w, const float* bias, int n,
                                     const MvdSegTable& seg, float* y, int ldy, hipStream_t s) {
  if (!x || !w || !y || batch <= 0 || batch > 4096 || k <= 0 || (k % 4) || (ldx % 4) || n <= 0 || ldy < n || seg.n < 1 || seg.n > 16 ||
      seg.end[seg.n - 1] != n || (((uintptr_t)x | (uintptr_t)w) & 15) || (xseg % 4)) { mvd_set_error("skinny_linear_grouped: bad arguments"); return -1; }
  for (int g = 0; g < seg.n; ++g) if (seg.end[g] % 2) { mvd_set_error("skinny_linear_grouped: segment ends must be even"); return -1; }
  bool tiles_ok = batch >= 8 && !(mvd_debug_flags() & MVD_DBG_SKINNY_VECTOR);    // a 32-feature tile must not straddle two segments
  for (int g = 0; g + 1 < seg.n; ++g) tiles_ok = tiles_ok && seg.end[g] % 32 == 0;
  if (tiles_ok) {
    hipLaunchKernelGGL((skinny_mfma_kernel<false, true>), dim3(nblk(n, 32)), dim3(256), 0, s, x, ldx, batch, k, (const void*)w, bias, n, 0, y, ldy, seg, xseg);
    return launch_check("skinny_mfma_grouped");
  }
  hipLaunchKernelGGL((skinny_linear_vec_kernel<false, 2, true>), dim3(nblk(n, 8)), dim3(256), 0, s, x, ldx, batch, k, (const void*)w, bias, n, 0, y, ldy, seg, xseg);
  return launch_check("skinny_linear_grouped");
}

__global__ void film_params_grouped_kernel(const float* __restrict__ raw, int batch, int ldraw, const MvdSegTable seg, float strength,
                                           float* __restrict__ out, int out_rows, int total) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;     // over out_rows * (sum of dims)
  if (i >= total) return;
  // segment g holds 2 dim_g raw features at raw column seg.end[g-1]; its outputs start at out + out_rows * seg.end[g-1]
  const int half = seg.end[seg.n - 1] / 2;                 // sum of dims
  const int r = i / half, cc = i - r * half;               // output row, channel index over all segments
  int g = 0, c0 = 0;
  while (g + 1 < seg.n && cc >= seg.end[g] / 2) ++g;
  c0 = g ? seg.end[g - 1] / 2 : 0;
  const int dim = seg.end[g] / 2 - c0, ch = cc - c0;
  const int b = r % batch;                                 // output rows beyond `batch` repeat the inputs cyclically
  const float* rw = raw + (size_t)b * ldraw + 2 * c0;
  const float sv = rw[ch], tv = rw[dim + ch];
  float* o = out + (size_t)out_rows * 2 * c0;
  o[(size_t)r * dim + ch] = 2.0f * strength / (1.0f + expf(-sv));
  o[(size_t)out_rows * dim + (size_t)r * dim + ch] = tv * strength;
}

int mvd_launch_film_params_grouped(const float* raw, int batch, const MvdSegTable& seg, float strength, float* out, int out_rows,
                                   hipStream_t s) {
  if (!raw || !out || batch <= 0 || out_rows < batch || seg.n < 1 || seg.n > 16) { mvd_set_error("film_params_grouped: bad arguments"); return -1; }
  const int total = out_rows * (seg.end[seg.n - 1] / 2);
  hipLaunchKernelGGL(film_params_grouped_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, raw, batch, seg.end[seg.n - 1], seg, strength, out, out_rows, total);
  return launch_check("film_params_grouped");
}

int mvd_launch_timestep_embedding(const float* t, int batch, int dim, float* y, hipStream_t s) {
  if (!t || !y || batch <= 0 || dim <= 0 || (dim & 1)) { mvd_set_error("timestep_embedding: bad arguments"); return -1; }
  hipLaunchKernelGGL(timestep_embedding_kernel, dim3(batch), dim3(128), 0, s, t, dim, y);
  return launch_check("timestep_embedding");
}

int mvd_launch_camera_features(const float* src, const float* tgt, int batch, int cam_rows, int nfreq, float max_freq,
                               float* rflat, float* enc, hipStream_t s) {
  if (!src || !tgt || !rflat || !enc || batch <= 0 || (cam_rows != 3 && cam_rows != 4) || nfreq < 2) { mvd_set_error("camera_features: bad arguments"); return -1; }
  hipLaunchKernelGGL(camera_features_kernel, dim3(batch), dim3(256), 0, s, src, tgt, cam_rows, nfreq, logf(max_freq), rflat, enc);
  return launch_check("camera_features");
}

int mvd_launch_film_params(const float* raw, int batch, int dim, float strength, float* scale, float* shift, int out_rows,
                           hipStream_t s) {
  if (!raw || !scale || !shift || batch <= 0 || dim <= 0 || out_rows < batch) { mvd_set_error("film_params: bad arguments"); return -1; }
  const int total = out_rows * dim;
  hipLaunchKernelGGL(film_params_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, raw, batch, dim, strength, scale, shift, total);
  return launch_check("film_params");
}

int mvd_launch_film_nchw_f32(const float* x, int batch, int c, int hw, const float* scale, const float* shift, float* y,
                             hipStream_t s) {
  if (!x || !y || !scale || !shift || batch <= 0 || c <= 0 || hw <= 0) { mvd_set_error("film_nchw: bad arguments"); return -1; }
  const long total = (long)batch * c * hw;
  hipLaunchKernelGGL(film_nchw_f32_kernel, dim3(nblk(total, 256)), dim3(256), 0, s, x, c, hw, scale, shift, y, total);
  return launch_check("film_nchw");
}

int mvd_launch_im2col_in(const float* x, int batch, int c, int h, int w, const float* scale, const float* shift, int ld_ss,
                         bf16_t* y, hipStream_t s) {
  if (!x || !y || batch <= 0 || c <= 0 || c > 7 || h <= 0 || w <= 0 || ((scale == nullptr) != (shift == nullptr))) { mvd_set_error("im2col_in: bad arguments (c=%d must be <= 7)", c); return -1; }
  const long total = (long)batch * h * w;
  const dim3 g(nblk(total, 128)), t(128);
  switch (c) {
    case 1: hipLaunchKernelGGL(im2col_in_kernel<1>, g, t, 0, s, x, h, w, scale, shift, ld_ss, y, total); break;
    case 2: hipLaunchKernelGGL(im2col_in_kernel<2>, g, t, 0, s, x, h, w, scale, shift, ld_ss, y, total); break;
    case 3: hipLaunchKernelGGL(im2col_in_kernel<3>, g, t, 0, s, x, h, w, scale, shift, ld_ss, y, total); break;
    case 4: hipLaunchKernelGGL(im2col_in_kernel<4>, g, t, 0, s, x, h, w, scale, shift, ld_ss, y, total); break;
    case 5: hipLaunchKernelGGL(im2col_in_kernel<5>, g, t, 0, s, x, h, w, scale, shift, ld_ss, y, total); break;
    case 6: hipLaunchKernelGGL(im2col_in_kernel<6>, g, t, 0, s, x, h, w, scale, shift, ld_ss, y, total); break;
    default: hipLaunchKernelGGL(im2col_in_kernel<7>, g, t, 0, s, x, h, w, scale, shift, ld_ss, y, total); break;
  }
  return launch_check("im2col_in");
}
