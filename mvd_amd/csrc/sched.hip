// Denoising-loop helpers around the UNet: the DDPM ancestral step, the
// classifier-free-guidance combine and the guided DDIM / DPM-Solver++ step as single fused elementwise kernels
// (fp32 latents, 16-byte vectors), and the guided step with guidance rescale (row N17), which needs two statistics per batch
// row and is one workgroup per row.
// Follows /root/reference/src/models/pipeline.py:156-161 and the diffusers-0.32.2 DDPMScheduler.step algebra;
// the per-step scalar coefficients are computed on the host (mvd_amd/scheduler.py) so the loop never syncs.
#include "kernels.h"

namespace {

// x0 = c0*model_out + c1*sample ; prev = c2*x0 + c3*sample + sigma*noise
__global__ void ddpm_step_kernel(const float* __restrict__ mo, const float* __restrict__ x, const float* __restrict__ nz,
                                 float c0, float c1, float c2, float c3, float sigma, float* __restrict__ y, long n4) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const f32x4 m = reinterpret_cast<const f32x4*>(mo)[i], s = reinterpret_cast<const f32x4*>(x)[i];
    f32x4 x0 = m * c0 + s * c1;
    f32x4 p = x0 * c2 + s * c3;
    if (nz) p += reinterpret_cast<const f32x4*>(nz)[i] * sigma;
    reinterpret_cast<f32x4*>(y)[i] = p;
  }
}

// noise_pred = uncond + g*(cond - uncond) with [uncond | cond] stacked on the batch dim
__global__ void cfg_combine_kernel(const float* __restrict__ both, float g, float* __restrict__ y, long n4) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const f32x4 u = reinterpret_cast<const f32x4*>(both)[i], c = reinterpret_cast<const f32x4*>(both)[i + n4];
    reinterpret_cast<f32x4*>(y)[i] = u + (c - u) * g;
  }
}

// The DDIM / DPM-Solver++ step (mvd_amd/scheduler.py), affine in (model output, sample, previous x0, noise):
//   m = guided ? u + g*(c - u) : model_out ; x0 = a0*m + a1*x ; y = p*x + q*x0 + r*d + sigma*z ; x0o = x0.
// x / y and d / x0o may alias (each element is read, then written, by the same thread): no __restrict__ on them.
__global__ void sampler_step_kernel(const float* __restrict__ mo, int guided, float g, const float* x, const float* d,
                                    const float* __restrict__ nz, float a0, float a1, float p, float q, float r, float sigma,
                                    float* y, float* x0o, long n4) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    f32x4 m = reinterpret_cast<const f32x4*>(mo)[i];
    if (guided) m = m + (reinterpret_cast<const f32x4*>(mo)[i + n4] - m) * g;
    const f32x4 s = reinterpret_cast<const f32x4*>(x)[i];
    const f32x4 x0 = m * a0 + s * a1;
    f32x4 o = s * p + x0 * q;
    if (d) o += reinterpret_cast<const f32x4*>(d)[i] * r;
    if (nz) o += reinterpret_cast<const f32x4*>(nz)[i] * sigma;
    reinterpret_cast<f32x4*>(y)[i] = o;
    if (x0o) reinterpret_cast<f32x4*>(x0o)[i] = x0;
  }
}

int grid_for(long n4) { long g = (n4 + 255) / 256; return (int)(g > 2048 ? 2048 : (g < 1 ? 1 : g)); }

// ---- the guided step with guidance rescale ----------------------------------------------------------
// One workgroup of RS_THREADS per row.  Thread t owns the 16-byte vectors t, t + RS_THREADS, ... of the row: a pure function
// of n_row.  The statistics are fp64 sums of x and x^2 of c and of m = u + g*(c - u) (m rounded to fp32 first, as the update
// uses it): per thread in vector order, across the wave by a xor butterfly, across the waves in wave order -- a fixed tree.
// KEEP > 0: the row's u and c stay in KEEP vectors per thread between the sums and the update (one HBM read); KEEP == 0: the
// row is streamed twice (the second read comes from L2 while a row fits there).
constexpr int RS_THREADS = 1024, RS_WAVE = 64, RS_WAVES = RS_THREADS / RS_WAVE;
constexpr int RS_KEEP_SMALL = 4, RS_KEEP_LARGE = 9;       // 16384 (512^2) and 36864 (768^2) floats per row

int rescale_keep(long n4) { return n4 <= (long)RS_KEEP_SMALL * RS_THREADS ? RS_KEEP_SMALL : n4 <= (long)RS_KEEP_LARGE * RS_THREADS ? RS_KEEP_LARGE : 0; }

__device__ __forceinline__ f32x4 guided4(f32x4 u, f32x4 c, float g) {
  f32x4 m;
#pragma unroll
  for (int j = 0; j < 4; ++j) m[j] = __fmaf_rn(c[j] - u[j], g, u[j]);
  return m;
}

__device__ __forceinline__ void rescale_sums(f32x4 c, f32x4 m, double (&s)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double cv = (double)c[j], mv = (double)m[j];
    s[0] += cv; s[1] = fma(cv, cv, s[1]); s[2] += mv; s[3] = fma(mv, mv, s[3]);
  }
}

// x / y and d / x0o may alias (each element is read, then written, by the same thread); x == nullptr reads as zeros
// (mvd_op_cfg_rescale).  mo overlaps no output (checked by the callers).
template <int KEEP>
__global__ __launch_bounds__(RS_THREADS) void sampler_step_rescaled_kernel(
    const float* __restrict__ mo, float g, float phi, const float* x, const float* d, const float* __restrict__ nz, float a0,
    float a1, float p, float q, float r, float sigma, float* y, float* x0o, long rows, long n4) {
  __shared__ double part[RS_WAVES][4];
  const long base = (long)blockIdx.x * n4;
  const f32x4* u4 = reinterpret_cast<const f32x4*>(mo) + base;
  const f32x4* c4 = u4 + rows * n4;
  const int tid = threadIdx.x;
  f32x4 ur[KEEP > 0 ? KEEP : 1], cr[KEEP > 0 ? KEEP : 1];
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (KEEP > 0) {
#pragma unroll
    for (int k = 0; k < KEEP; ++k) {
      const long i = tid + (long)k * RS_THREADS;
      if (i < n4) { ur[k] = u4[i]; cr[k] = c4[i]; }
    }
#pragma unroll
    for (int k = 0; k < KEEP; ++k)
      if (tid + (long)k * RS_THREADS < n4) rescale_sums(cr[k], guided4(ur[k], cr[k], g), s);
  } else {
    for (long i = tid; i < n4; i += RS_THREADS) {
      const f32x4 u = u4[i], c = c4[i];
      rescale_sums(c, guided4(u, c, g), s);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int mask = RS_WAVE / 2; mask > 0; mask >>= 1) s[j] += __shfl_xor(s[j], mask, RS_WAVE);
  if ((tid & (RS_WAVE - 1)) == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) part[tid / RS_WAVE][j] = s[j];
  }
  __syncthreads();
  double t[4] = {0.0, 0.0, 0.0, 0.0};
  for (int w = 0; w < RS_WAVES; ++w) {
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] += part[w][j];
  }
  // unbiased variances; the common divisor n - 1 cancels in the ratio.  No epsilon: var_m == 0 gives inf or NaN.
  const double n = 4.0 * (double)n4;
  const double var_c = fmax(t[1] - t[0] * (t[0] / n), 0.0), var_m = fmax(t[3] - t[2] * (t[2] / n), 0.0);
  const float f = (float)((double)phi * sqrt(var_c / var_m) + (1.0 - (double)phi));

  auto update = [&](long i, f32x4 u, f32x4 c) {
    const f32x4 m = guided4(u, c, g) * f;
    f32x4 sx = {0.f, 0.f, 0.f, 0.f};
    if (x) sx = reinterpret_cast<const f32x4*>(x)[base + i];
    const f32x4 x0 = m * a0 + sx * a1;
    f32x4 o = sx * p + x0 * q;
    if (d) o += reinterpret_cast<const f32x4*>(d)[base + i] * r;
    if (nz) o += reinterpret_cast<const f32x4*>(nz)[base + i] * sigma;
    reinterpret_cast<f32x4*>(y)[base + i] = o;
    if (x0o) reinterpret_cast<f32x4*>(x0o)[base + i] = x0;
  };
  if (KEEP > 0) {
#pragma unroll
    for (int k = 0; k < KEEP; ++k) {
      const long i = tid + (long)k * RS_THREADS;
      if (i < n4) update(i, ur[k], cr[k]);
    }
  } else {
    for (long i = tid; i < n4; i += RS_THREADS) update(i, u4[i], c4[i]);
  }
}

bool overlaps(const float* a, int64_t na, const float* b, int64_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a && b && a0 < b0 + (uintptr_t)nb * sizeof(float) && b0 < a0 + (uintptr_t)na * sizeof(float);
}

int launch_rescaled(const char* who, const float* mo, float g, float phi, const float* x, const float* d, const float* nz, float a0,
                    float a1, float p, float q, float r, float sigma, float* y, float* x0o, int64_t rows, int64_t n_row,
                    hipStream_t stream) {
  if (!(phi >= 0.f && phi <= 1.f)) { mvd_set_error("%s: guidance_rescale must lie in [0, 1], got %g", who, (double)phi); return -1; }
  if (rows > 0x7fffffffLL) { mvd_set_error("%s: too many rows", who); return -1; }
  if (overlaps(mo, 2 * rows * n_row, y, rows * n_row) || overlaps(mo, 2 * rows * n_row, x0o, rows * n_row)) {
    mvd_set_error("%s: an output overlaps the model output (every element of a row is read before any output is final)", who);
    return -1;
  }
  const long n4 = (long)(n_row / 4);
  const dim3 grid((unsigned)rows), block(RS_THREADS);
  switch (rescale_keep(n4)) {
    case RS_KEEP_SMALL:
      hipLaunchKernelGGL(sampler_step_rescaled_kernel<RS_KEEP_SMALL>, grid, block, 0, stream, mo, g, phi, x, d, nz, a0, a1, p, q, r,
                         sigma, y, x0o, (long)rows, n4);
      break;
    case RS_KEEP_LARGE:
      hipLaunchKernelGGL(sampler_step_rescaled_kernel<RS_KEEP_LARGE>, grid, block, 0, stream, mo, g, phi, x, d, nz, a0, a1, p, q, r,
                         sigma, y, x0o, (long)rows, n4);
      break;
    default:
      hipLaunchKernelGGL(sampler_step_rescaled_kernel<0>, grid, block, 0, stream, mo, g, phi, x, d, nz, a0, a1, p, q, r, sigma, y,
                         x0o, (long)rows, n4);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { mvd_set_error("%s launch: %s", who, hipGetErrorString(e)); return -3; }
  return 0;
}

}  // namespace

extern "C" int mvd_op_ddpm_step(const float* model_out, const float* sample, const float* noise, float c0, float c1, float c2,
                                float c3, float sigma, float* out, int64_t n, void* stream) {
  if (!model_out || !sample || !out || n <= 0 || (n & 3)) { mvd_set_error("ddpm_step: bad arguments (n must be a multiple of 4)"); return -1; }
  if (!noise && sigma != 0.f) { mvd_set_error("ddpm_step: noise required when sigma != 0"); return -1; }
  hipLaunchKernelGGL(ddpm_step_kernel, dim3(grid_for(n / 4)), dim3(256), 0, (hipStream_t)stream, model_out, sample, noise, c0, c1, c2,
                     c3, sigma, out, (long)(n / 4));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { mvd_set_error("ddpm_step launch: %s", hipGetErrorString(e)); return -3; }
  return 0;
}

extern "C" int mvd_op_cfg_combine(const float* uncond_cond, float guidance_scale, float* out, int64_t n_half, void* stream) {
  if (!uncond_cond || !out || n_half <= 0 || (n_half & 3)) { mvd_set_error("cfg_combine: bad arguments"); return -1; }
  hipLaunchKernelGGL(cfg_combine_kernel, dim3(grid_for(n_half / 4)), dim3(256), 0, (hipStream_t)stream, uncond_cond, guidance_scale, out,
                     (long)(n_half / 4));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { mvd_set_error("cfg_combine launch: %s", hipGetErrorString(e)); return -3; }
  return 0;
}

extern "C" int mvd_op_sampler_step(const float* model_out, int guided, float guidance_scale, const float* sample,
                                   const float* x0_prev, const float* noise, float a0, float a1, float p, float q, float r,
                                   float sigma, float* out, float* x0_out, int64_t n, void* stream) {
  if (!model_out || !sample || !out || n <= 0 || (n & 3)) { mvd_set_error("sampler_step: bad arguments (n must be a multiple of 4)"); return -1; }
  if (!x0_prev && r != 0.f) { mvd_set_error("sampler_step: x0_prev required when r != 0"); return -1; }
  if (!noise && sigma != 0.f) { mvd_set_error("sampler_step: noise required when sigma != 0"); return -1; }
  hipLaunchKernelGGL(sampler_step_kernel, dim3(grid_for(n / 4)), dim3(256), 0, (hipStream_t)stream, model_out, guided ? 1 : 0,
                     guidance_scale, sample, r != 0.f ? x0_prev : nullptr, sigma != 0.f ? noise : nullptr, a0, a1, p, q, r, sigma,
                     out, x0_out, (long)(n / 4));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { mvd_set_error("sampler_step launch: %s", hipGetErrorString(e)); return -3; }
  return 0;
}

extern "C" int mvd_op_cfg_rescale(const float* uncond_cond, float guidance_scale, float guidance_rescale, float* out, int64_t rows,
                                  int64_t n_row, void* stream) {
  if (!uncond_cond || !out || rows <= 0 || n_row <= 0 || (n_row & 3)) { mvd_set_error("cfg_rescale: bad arguments (n_row must be a multiple of 4)"); return -1; }
  return launch_rescaled("cfg_rescale", uncond_cond, guidance_scale, guidance_rescale, nullptr, nullptr, nullptr, 1.f, 0.f, 0.f, 1.f, 0.f,
                         0.f, out, nullptr, rows, n_row, (hipStream_t)stream);
}

extern "C" int mvd_op_sampler_step_rescaled(const float* model_out, float guidance_scale, float guidance_rescale, const float* sample,
                                            const float* x0_prev, const float* noise, float a0, float a1, float p, float q, float r,
                                            float sigma, float* out, float* x0_out, int64_t rows, int64_t n_row, void* stream) {
  if (!model_out || !sample || !out || rows <= 0 || n_row <= 0 || (n_row & 3)) {
    mvd_set_error("sampler_step_rescaled: bad arguments (n_row must be a multiple of 4)");
    return -1;
  }
  if (!x0_prev && r != 0.f) { mvd_set_error("sampler_step_rescaled: x0_prev required when r != 0"); return -1; }
  if (!noise && sigma != 0.f) { mvd_set_error("sampler_step_rescaled: noise required when sigma != 0"); return -1; }
  return launch_rescaled("sampler_step_rescaled", model_out, guidance_scale, guidance_rescale, sample, r != 0.f ? x0_prev : nullptr,
                         sigma != 0.f ? noise : nullptr, a0, a1, p, q, r, sigma, out, x0_out, rows, n_row, (hipStream_t)stream);
}

extern "C" int mvd_debug_cfg_rescale_plan(int64_t n_row, int* out) {
  if (!out || n_row <= 0 || (n_row & 3)) { mvd_set_error("cfg_rescale_plan: bad arguments (n_row must be a multiple of 4)"); return -1; }
  out[0] = RS_THREADS; out[1] = 4; out[2] = RS_WAVE; out[3] = rescale_keep((long)(n_row / 4));
  return 0;
}
