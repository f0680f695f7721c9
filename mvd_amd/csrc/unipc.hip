// The UniPC step (Zhao et al., NeurIPS 2023, "UniPC: A Unified Predictor-Corrector Framework for Fast
// Sampling of Diffusion Models"; diffusers-0.32.2 UniPCMultistepScheduler with predict_x0, restated): the corrector of the previous
// step and the predictor of this one as ONE fused elementwise kernel, the sibling of sampler_step_kernel (sched.hip) and in its
// style -- fp32 latents, 16-byte vectors, grid-stride.  Both updates are affine in (model output, sample, last sample, x0 history);
// the per-step scalar coefficients come from the host (mvd_amd/scheduler.py), so the loop never syncs.  Per element:
//   m  = guided ? u + g*(c - u) : model_out
//   x0 = a0*m + a1*x
//   xc = corr ? cx*xl + c0*h0 + c1*h1 + c2*h2 + ct*x0 : x
//   y  = px*xc + p0*x0 + p1*h0 + p2*h1 ;  xc_out = xc ;  x0_out = x0
// Evaluation order (every operation one fp32 rounding; a term whose coefficient is 0 is skipped, its pointer never read):
//   m  = fma(c - u, g, u)                                                         2 operations
//   x0 = fma(a0, m, a1*x)                                                         2
//   xc = cx*xl, then fma(c0, h0, .), fma(c1, h1, .), fma(c2, h2, .), fma(ct, x0, .)   5, in this order
//   y  = px*xc, then fma(p0, x0, .), fma(p1, h0, .), fma(p2, h1, .)                   4, in this order
#include "kernels.h"

namespace {

__device__ __forceinline__ f32x4 mul4(float a, f32x4 b) {
  f32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = __fmul_rn(a, b[j]);
  return o;
}

__device__ __forceinline__ f32x4 fma4(float a, f32x4 b, f32x4 c) {
  f32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = __fmaf_rn(a, b[j], c[j]);
  return o;
}

__device__ __forceinline__ f32x4 guided4(f32x4 u, f32x4 c, float g) {
  f32x4 m;
#pragma unroll
  for (int j = 0; j < 4; ++j) m[j] = __fmaf_rn(__fsub_rn(c[j], u[j]), g, u[j]);
  return m;
}

struct UniPCCoeffs {
  float a0, a1;                 // x0 = a0*m + a1*x
  float cx, c0, c1, c2, ct;     // the corrector (all 0 when corr == 0)
  float px, p0, p1, p2;         // the predictor
};

// y / x, xco / xl and x0o / one of h0..h2 may alias (each element is read, then written, by the same thread): no __restrict__ on
// them.  mo overlaps no output (checked by the caller).  A null h0 / h1 / h2 / xl goes with zero coefficients and is never read.
__global__ void unipc_step_kernel(const float* __restrict__ mo, int guided, float g, const float* x, const float* xl, const float* h0,
                                  const float* h1, const float* h2, int corr, UniPCCoeffs k, float* y, float* xco, float* x0o,
                                  long n4) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    f32x4 m = reinterpret_cast<const f32x4*>(mo)[i];
    if (guided) m = guided4(m, reinterpret_cast<const f32x4*>(mo)[i + n4], g);
    const f32x4 s = reinterpret_cast<const f32x4*>(x)[i];
    f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0, v2 = v0;
    if (h0) v0 = reinterpret_cast<const f32x4*>(h0)[i];
    if (h1) v1 = reinterpret_cast<const f32x4*>(h1)[i];
    if (h2) v2 = reinterpret_cast<const f32x4*>(h2)[i];
    const f32x4 x0 = fma4(k.a0, m, mul4(k.a1, s));
    f32x4 xc = s;
    if (corr) {
      xc = mul4(k.cx, reinterpret_cast<const f32x4*>(xl)[i]);
      if (k.c0 != 0.f) xc = fma4(k.c0, v0, xc);
      if (k.c1 != 0.f) xc = fma4(k.c1, v1, xc);
      if (k.c2 != 0.f) xc = fma4(k.c2, v2, xc);
      if (k.ct != 0.f) xc = fma4(k.ct, x0, xc);
    }
    f32x4 o = mul4(k.px, xc);
    if (k.p0 != 0.f) o = fma4(k.p0, x0, o);
    if (k.p1 != 0.f) o = fma4(k.p1, v0, o);
    if (k.p2 != 0.f) o = fma4(k.p2, v1, o);
    reinterpret_cast<f32x4*>(y)[i] = o;
    if (xco) reinterpret_cast<f32x4*>(xco)[i] = xc;
    if (x0o) reinterpret_cast<f32x4*>(x0o)[i] = x0;
  }
}

// sampler_step_kernel's grid: one vector per thread up to 2048 blocks of 256, the stride loop beyond
int grid_for(long n4) { long g = (n4 + 255) / 256; return (int)(g > 2048 ? 2048 : (g < 1 ? 1 : g)); }

bool overlaps(const float* a, int64_t na, const float* b, int64_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a && b && a0 < b0 + (uintptr_t)nb * sizeof(float) && b0 < a0 + (uintptr_t)na * sizeof(float);
}

}  // namespace

extern "C" int mvd_op_unipc_step(const float* model_out, int guided, float guidance_scale, const float* sample, const float* last_sample,
                                 const float* h0, const float* h1, const float* h2, float a0, float a1, int corr, float cx, float c0,
                                 float c1, float c2, float ct, float px, float p0, float p1, float p2, float* out, float* xc_out,
                                 float* x0_out, int64_t n, void* stream) {
  if (!model_out || !sample || !out || n <= 0 || (n & 3)) { mvd_set_error("unipc_step: bad arguments (n must be a multiple of 4)"); return -1; }
  if (!corr) cx = c0 = c1 = c2 = ct = 0.f;          // without the corrector its coefficients do not exist
  if (corr && !last_sample) { mvd_set_error("unipc_step: last_sample required with the corrector"); return -1; }
  if (!h0 && (c0 != 0.f || p1 != 0.f)) { mvd_set_error("unipc_step: h0 required when c0 != 0 or p1 != 0"); return -1; }
  if (!h1 && (c1 != 0.f || p2 != 0.f)) { mvd_set_error("unipc_step: h1 required when c1 != 0 or p2 != 0"); return -1; }
  if (!h2 && c2 != 0.f) { mvd_set_error("unipc_step: h2 required when c2 != 0"); return -1; }
  const int64_t n_mo = guided ? 2 * n : n;
  if (overlaps(model_out, n_mo, out, n) || overlaps(model_out, n_mo, xc_out, n) || overlaps(model_out, n_mo, x0_out, n)) {
    mvd_set_error("unipc_step: an output overlaps the model output (the guided halves are read by different threads)");
    return -1;
  }
  if (overlaps(out, n, xc_out, n) || overlaps(out, n, x0_out, n) || overlaps(xc_out, n, x0_out, n)) {
    mvd_set_error("unipc_step: out, xc_out and x0_out overlap one another");
    return -1;
  }
  const UniPCCoeffs k = {a0, a1, cx, c0, c1, c2, ct, px, p0, p1, p2};
  hipLaunchKernelGGL(unipc_step_kernel, dim3(grid_for(n / 4)), dim3(256), 0, (hipStream_t)stream, model_out, guided ? 1 : 0,
                     guidance_scale, sample, corr ? last_sample : nullptr, (c0 != 0.f || p1 != 0.f) ? h0 : nullptr,
                     (c1 != 0.f || p2 != 0.f) ? h1 : nullptr, c2 != 0.f ? h2 : nullptr, corr ? 1 : 0, k, out, xc_out, x0_out,
                     (long)(n / 4));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { mvd_set_error("unipc_step launch: %s", hipGetErrorString(e)); return -3; }
  return 0;
}
