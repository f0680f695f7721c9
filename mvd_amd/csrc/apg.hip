// Adaptive projected guidance fused into the guided step (Sadat, Hilliges and Weber, ICLR 2025,
// "Eliminating Oversaturation and Artifacts of High Guidance Scales in Diffusion Models"; diffusers' normalized_guidance with
// use_original_formulation=True, restated).  The sibling of sampler_step_rescaled_kernel (sched.hip, row N17) and laid out like
// it: one workgroup of AP_THREADS per batch row, thread t owns the 16-byte vectors t, t + AP_THREADS, ... of the row, five
// statistics per row as fixed-order fp64 sums (per thread in vector order, a xor butterfly inside the wave, the waves in wave
// order through LDS; no atomics), then an elementwise update and the affine sampler step.  Per row:
//   d = (c - u) + beta*M ; M <- d                      (space "x0": c <- a0*c + a1*x, d <- a0*(c - u) + beta*M first)
//   s = tau > 0 ? min(1, tau / sqrt(sum d^2)) : 1 ; alpha = s * sum(d c) / sum(c^2)
//   m = A*c + B*d ,  A = 1 - (g - 1)(1 - eta) alpha ,  B = (g - 1) s ;  phi > 0: A, B times phi*std(c)/std(m) + 1 - phi
// with the moments of m from the five sums (sum m = A sum c + B sum d, sum m^2 = A^2 sum c^2 + 2AB sum cd + B^2 sum d^2), so
// the row is read once.  The per-step scalar coefficients come from the host (mvd_amd/scheduler.py); the loop never syncs.
#include "kernels.h"

namespace {

constexpr int AP_THREADS = 1024, AP_WAVE = 64, AP_WAVES = AP_THREADS / AP_WAVE;
constexpr int AP_KEEP_SMALL = 4, AP_KEEP_LARGE = 9;       // 16384 (512^2) and 36864 (768^2) floats per row: N17's KEEP rule
constexpr int AP_SUMS = 5;                                // sum c, sum d, sum c^2, sum d^2, sum c d

int apg_keep(long n4) { return n4 <= (long)AP_KEEP_SMALL * AP_THREADS ? AP_KEEP_SMALL : n4 <= (long)AP_KEEP_LARGE * AP_THREADS ? AP_KEEP_LARGE : 0; }

struct ApgArgs {             // the launcher's arguments (host side)
  const float* mo;          // [uncond | cond], 2 * rows * n_row floats: read only
  float* mom;               // the momentum buffer M (rows * n_row), read and written in place; nullptr when beta == 0
  const float* x;           // the sample; nullptr reads as zeros (mvd_op_apg)
  const float* hist;        // the previous step's x0 (r != 0) or nullptr
  const float* nz;          // the step's noise (sigma != 0) or nullptr
  float* y;                 // the step's output; may be x
  float* x0o;               // this step's x0, or nullptr; may be hist
  float g, eta, tau, beta, phi;
  int x0_space;             // 1: the projection runs on the denoised prediction, m is the step's x0
  float a0, a1, p, q, r, sigma;
};

__device__ __forceinline__ f32x4 fma4(float a, f32x4 b, f32x4 c) {
  f32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = __fmaf_rn(a, b[j], c[j]);
  return o;
}

__device__ __forceinline__ void apg_sums(f32x4 c, f32x4 d, double (&s)[AP_SUMS]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double cv = (double)c[j], dv = (double)d[j];
    s[0] += cv; s[1] += dv; s[2] = fma(cv, cv, s[2]); s[3] = fma(dv, dv, s[3]); s[4] = fma(cv, dv, s[4]);
  }
}

// MOM: beta != 0, M is read and written.  X0: space "x0".  x / y and hist / x0o may alias, and M is updated in place: each element
// is read, then written, by the same thread.  mo overlaps no output and M overlaps no other argument (checked by the launcher).
// c and d are formed by the same fp32 operations wherever they are formed, so a streamed row's second pass has the first's bits.
template <int KEEP, bool MOM, bool X0>
__global__ __launch_bounds__(AP_THREADS) void sampler_step_apg_kernel(
    const float* __restrict__ mo, float* mom, const float* x, const float* hist, const float* __restrict__ nz, float* y, float* x0o,
    float g, float eta, float tau, float beta, float phi, float a0, float a1, float p, float q, float r, float sigma, long rows,
    long n4) {
  __shared__ double part[AP_WAVES][AP_SUMS];
  const long base = (long)blockIdx.x * n4;
  const f32x4* u4 = reinterpret_cast<const f32x4*>(mo) + base;
  const f32x4* c4 = u4 + rows * n4;
  const f32x4* x4 = reinterpret_cast<const f32x4*>(x) + base;            // dereferenced only where x is set
  f32x4* m4 = reinterpret_cast<f32x4*>(mom) + base;                      // dereferenced only under MOM
  const int tid = threadIdx.x;
  f32x4 cr[KEEP > 0 ? KEEP : 1], dr[KEEP > 0 ? KEEP : 1];
  double s[AP_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};

  // first pass: c and d of every vector of the thread, M <- d, the five sums in vector order
#define APG_FIRST(i, c, d)                                \
  f32x4 c = c4[i], d = c - u4[i];                         \
  if (X0) { d = d * a0; c = fma4(a0, c, x4[i] * a1); }    \
  if (MOM) { d = fma4(beta, m4[i], d); m4[i] = d; }
  if (KEEP > 0) {
#pragma unroll
    for (int k = 0; k < KEEP; ++k) {
      const long i = tid + (long)k * AP_THREADS;
      if (i < n4) {
        APG_FIRST(i, c, d)
        cr[k] = c; dr[k] = d;
      }
    }
#pragma unroll
    for (int k = 0; k < KEEP; ++k)
      if (tid + (long)k * AP_THREADS < n4) apg_sums(cr[k], dr[k], s);
  } else {
    for (long i = tid; i < n4; i += AP_THREADS) {
      APG_FIRST(i, c, d)
      apg_sums(c, d, s);
    }
  }
#pragma unroll
  for (int j = 0; j < AP_SUMS; ++j)
#pragma unroll
    for (int mask = AP_WAVE / 2; mask > 0; mask >>= 1) s[j] += __shfl_xor(s[j], mask, AP_WAVE);
  if ((tid & (AP_WAVE - 1)) == 0) {
#pragma unroll
    for (int j = 0; j < AP_SUMS; ++j) part[tid / AP_WAVE][j] = s[j];
  }
  __syncthreads();
  double t[AP_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
  // (four waves' partials in flight: all sixteen at once are 160 registers beside the kept row)
#pragma unroll 4
  for (int w = 0; w < AP_WAVES; ++w) {
#pragma unroll
    for (int j = 0; j < AP_SUMS; ++j) t[j] += part[w][j];
  }
  const double sc = t[0], sd = t[1], scc = t[2], sdd = t[3], scd = t[4];
  const double gm1 = (double)g - 1.0;
  const double cap = (tau > 0.f && sdd > 0.0) ? fmin(1.0, (double)tau / sqrt(sdd)) : 1.0;
  const double alpha = scc > 0.0 ? cap * scd / scc : 0.0;
  double A = 1.0 - gm1 * (1.0 - (double)eta) * alpha, B = gm1 * cap;
  if (phi > 0.f) {
    // N17's rescale on the moments of m = A c + B d: unbiased variances, the common divisor n - 1 cancels.  No epsilon.
    const double n = 4.0 * (double)n4;
    const double sm = A * sc + B * sd, smm = A * A * scc + 2.0 * A * B * scd + B * B * sdd;
    const double var_c = fmax(scc - sc * (sc / n), 0.0), var_m = fmax(smm - sm * (sm / n), 0.0);
    const double f = (double)phi * sqrt(var_c / var_m) + (1.0 - (double)phi);
    A *= f;
    B *= f;
  }
  const float Af = (float)A, Bf = (float)B;

  auto update = [&](long i, f32x4 c, f32x4 d) {
    const f32x4 m = fma4(Af, c, d * Bf);
    f32x4 sx = {0.f, 0.f, 0.f, 0.f};
    if (x) sx = x4[i];
    const f32x4 x0 = X0 ? m : m * a0 + sx * a1;
    f32x4 o = sx * p + x0 * q;
    if (hist) o += reinterpret_cast<const f32x4*>(hist)[base + i] * r;
    if (nz) o += reinterpret_cast<const f32x4*>(nz)[base + i] * sigma;
    reinterpret_cast<f32x4*>(y)[base + i] = o;
    if (x0o) reinterpret_cast<f32x4*>(x0o)[base + i] = x0;
  };
  if (KEEP > 0) {
#pragma unroll
    for (int k = 0; k < KEEP; ++k) {
      const long i = tid + (long)k * AP_THREADS;
      if (i < n4) update(i, cr[k], dr[k]);
    }
  } else {
    // streamed twice: d comes back from M (this thread wrote it) when there is one, else it is recomputed
    for (long i = tid; i < n4; i += AP_THREADS) {
      f32x4 c = c4[i], d;
      if (MOM) d = m4[i];
      else { d = c - u4[i]; if (X0) d = d * a0; }
      if (X0) c = fma4(a0, c, x4[i] * a1);
      update(i, c, d);
    }
  }
#undef APG_FIRST
}

bool overlaps(const float* a, int64_t na, const float* b, int64_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a && b && a0 < b0 + (uintptr_t)nb * sizeof(float) && b0 < a0 + (uintptr_t)na * sizeof(float);
}

// the checks both entry points share, then the launch
int launch_apg(const char* who, ApgArgs a, int64_t rows, int64_t n_row, hipStream_t stream) {
  if (!(a.eta >= 0.f && a.eta <= 1.f)) { mvd_set_error("%s: eta must lie in [0, 1], got %g", who, (double)a.eta); return -1; }
  if (!(a.tau >= 0.f) || a.tau > 3.0e38f) { mvd_set_error("%s: norm_threshold must be finite and >= 0 (0: off), got %g", who, (double)a.tau); return -1; }
  if (!(a.beta > -1.f && a.beta < 1.f)) { mvd_set_error("%s: momentum must lie in (-1, 1), got %g", who, (double)a.beta); return -1; }
  if (!(a.phi >= 0.f && a.phi <= 1.f)) { mvd_set_error("%s: guidance_rescale must lie in [0, 1], got %g", who, (double)a.phi); return -1; }
  if (a.x0_space != 0 && a.x0_space != 1) { mvd_set_error("%s: space must be 0 (output) or 1 (x0), got %d", who, a.x0_space); return -1; }
  if (a.x0_space && a.phi > 0.f) {
    mvd_set_error("%s: space=\"x0\" with guidance_rescale > 0 is not defined (the rescale is defined on the model output)", who);
    return -1;
  }
  if (a.beta != 0.f && !a.mom) { mvd_set_error("%s: momentum buffer required when momentum != 0", who); return -1; }
  if (a.beta == 0.f) a.mom = nullptr;                     // untouched
  if (rows > 0x7fffffffLL) { mvd_set_error("%s: too many rows", who); return -1; }
  const int64_t n = rows * n_row;
  if (overlaps(a.mo, 2 * n, a.y, n) || overlaps(a.mo, 2 * n, a.x0o, n) || overlaps(a.mo, 2 * n, a.mom, n)) {
    mvd_set_error("%s: an output overlaps the model output (every element of a row is read before any output is final)", who);
    return -1;
  }
  if (overlaps(a.mom, n, a.y, n) || overlaps(a.mom, n, a.x0o, n) || overlaps(a.mom, n, a.x, n) || overlaps(a.mom, n, a.hist, n) ||
      overlaps(a.mom, n, a.nz, n)) {
    mvd_set_error("%s: the momentum buffer overlaps another argument (it is written before the step reads its inputs)", who);
    return -1;
  }
  const long n4 = (long)(n_row / 4);
  const dim3 grid((unsigned)rows), block(AP_THREADS);
  const bool mom = a.mom != nullptr, x0 = a.x0_space != 0;
#define APG_LAUNCH_AS(KEEP, MOM, X0)                                                                                              \
  hipLaunchKernelGGL((sampler_step_apg_kernel<KEEP, MOM, X0>), grid, block, 0, stream, a.mo, a.mom, a.x, a.hist, a.nz, a.y, a.x0o, \
                     a.g, a.eta, a.tau, a.beta, a.phi, a.a0, a.a1, a.p, a.q, a.r, a.sigma, (long)rows, n4)
#define APG_LAUNCH(KEEP)                              \
  do {                                                \
    if (mom && x0) APG_LAUNCH_AS(KEEP, true, true);   \
    else if (mom) APG_LAUNCH_AS(KEEP, true, false);   \
    else if (x0) APG_LAUNCH_AS(KEEP, false, true);    \
    else APG_LAUNCH_AS(KEEP, false, false);           \
  } while (0)
  switch (apg_keep(n4)) {
    case AP_KEEP_SMALL: APG_LAUNCH(AP_KEEP_SMALL); break;
    case AP_KEEP_LARGE: APG_LAUNCH(AP_KEEP_LARGE); break;
    default: APG_LAUNCH(0);
  }
#undef APG_LAUNCH
#undef APG_LAUNCH_AS
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { mvd_set_error("%s launch: %s", who, hipGetErrorString(e)); return -3; }
  return 0;
}

}  // namespace

extern "C" int mvd_op_apg(const float* uncond_cond, float guidance_scale, float eta, float norm_threshold, float momentum,
                          float guidance_rescale, float* momentum_buffer, float* out, int64_t rows, int64_t n_row, void* stream) {
  if (!uncond_cond || !out || rows <= 0 || n_row <= 0 || (n_row & 3)) { mvd_set_error("apg: bad arguments (n_row must be a multiple of 4)"); return -1; }
  ApgArgs a = {};
  a.mo = uncond_cond; a.mom = momentum_buffer; a.y = out;
  a.g = guidance_scale; a.eta = eta; a.tau = norm_threshold; a.beta = momentum; a.phi = guidance_rescale;
  a.a0 = 1.f; a.a1 = 0.f; a.p = 0.f; a.q = 1.f; a.r = 0.f; a.sigma = 0.f;     // x0 = m, out = x0
  return launch_apg("apg", a, rows, n_row, (hipStream_t)stream);
}

extern "C" int mvd_op_sampler_step_apg(const float* model_out, float guidance_scale, float eta, float norm_threshold, float momentum,
                                       float guidance_rescale, int space, float* momentum_buffer, const float* sample,
                                       const float* x0_prev, const float* noise, float a0, float a1, float p, float q, float r,
                                       float sigma, float* out, float* x0_out, int64_t rows, int64_t n_row, void* stream) {
  if (!model_out || !sample || !out || rows <= 0 || n_row <= 0 || (n_row & 3)) {
    mvd_set_error("sampler_step_apg: bad arguments (n_row must be a multiple of 4)");
    return -1;
  }
  if (!x0_prev && r != 0.f) { mvd_set_error("sampler_step_apg: x0_prev required when r != 0"); return -1; }
  if (!noise && sigma != 0.f) { mvd_set_error("sampler_step_apg: noise required when sigma != 0"); return -1; }
  ApgArgs a = {};
  a.mo = model_out; a.mom = momentum_buffer; a.x = sample; a.hist = r != 0.f ? x0_prev : nullptr; a.nz = sigma != 0.f ? noise : nullptr;
  a.y = out; a.x0o = x0_out;
  a.g = guidance_scale; a.eta = eta; a.tau = norm_threshold; a.beta = momentum; a.phi = guidance_rescale; a.x0_space = space;
  a.a0 = a0; a.a1 = a1; a.p = p; a.q = q; a.r = r; a.sigma = sigma;
  return launch_apg("sampler_step_apg", a, rows, n_row, (hipStream_t)stream);
}

extern "C" int mvd_debug_apg_plan(int64_t n_row, int* out) {
  if (!out || n_row <= 0 || (n_row & 3)) { mvd_set_error("apg_plan: bad arguments (n_row must be a multiple of 4)"); return -1; }
  out[0] = AP_THREADS; out[1] = 4; out[2] = AP_WAVE; out[3] = apg_keep((long)(n_row / 4));
  return 0;
}
