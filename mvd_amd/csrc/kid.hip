// KID and the Inception score on the FID tower's pool3 features: the arithmetic behind torchmetrics'
// KernelInceptionDistance and InceptionScore(feature="logits_unbiased"), everything after the network.
//
//   kid_mmd_kernel    the polynomial-kernel MMD of many subsets in ONE launch: per subset the three Gram families xx, yy, xy of the
//                     m gathered rows, (dot gamma + coef)^degree summed per 64 x 64 tile on v_mfma_f64_16x16x4_f64; no m x m matrix
//                     ever exists.  One partial per tile; kid_finish_kernel adds them in tile order and forms the estimate.
//   fc_logits_kernel  logits = f . W^T in fp32 (torch-fidelity's logits_unbiased: no bias), one wave per class and row, an order
//                     that does not depend on the batch
//   is_*_kernel       the Inception-score head in fp64 from the fp32 logits: log-sum-exp per row, the mean probability per
//                     (chunk, class), the KL sum per row and exp(mean) per chunk
//
// No floating-point atomics: every sum has one owner and a written order, so two calls give the same bits.
#include <stdio.h>
#include <string.h>

#include "host_util.h"

typedef __attribute__((ext_vector_type(4))) double f64x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

namespace {

// ---------------------------------------------------------------- polynomial-kernel MMD
// Tiles of one subset, T = ceil(m / 64): xx and yy keep the T (T + 1) / 2 tiles with tj >= ti, row-major over (ti, tj), and count a
// tile off the diagonal twice (a multiplication by 2: exact); xy keeps all T T.  Tile order: xx, yy, xy.
constexpr int KID_KC = 32;            // K elements staged per step
constexpr int KID_LD = KID_KC + 4;    // LDS row stride in floats: 16-byte rows, lane (q, r) reads bank 4 r + q of 64
__host__ __device__ inline long kid_tri(long T) { return T * (T + 1) / 2; }
__host__ __device__ inline long kid_tiles(long T) { return 2 * kid_tri(T) + T * T; }

// Workgroup = one 64 x 64 tile; wave = a 32 x 32 quadrant = 2 x 2 MFMA tiles.  The 64 + 64 gathered rows are staged through LDS
// in fp32, KID_KC columns at a time, with coalesced 16-byte loads along a row (the next step's loads are in flight while this
// step's MFMAs run); a lane converts its operand to fp64 when it reads it: A lane l holds X[row l & 15][k + (l >> 4)], B the same
// for Y; D: col = l & 15, row = (l >> 4) + 4 reg.  K runs 0 .. d - 1 in order, four to an instruction, never split.
__global__ __launch_bounds__(256) void kid_mmd_kernel(const float* __restrict__ f_real, int n_real, const float* __restrict__ f_fake, int n_fake, int d,
                                                      const int* __restrict__ idx, int m, int degree, double gamma, double coef, long tiles,
                                                      double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ float stage[128 * KID_LD];
  __shared__ double wave_sum[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const long subset = blockIdx.x / tiles;
  long t = blockIdx.x - subset * tiles;
  const int T = (m + 63) >> 6;
  const long tri = kid_tri(T);
  int family = 0, ti, tj;
  if (t >= 2 * tri) {
    family = 2; t -= 2 * tri;
    ti = (int)(t / T); tj = (int)(t - (long)ti * T);
  } else {
    if (t >= tri) { family = 1; t -= tri; }
    ti = 0;
    while (t >= T - ti) { t -= T - ti; ++ti; }
    tj = ti + (int)t;
  }
  // slot 0 of idx indexes f_real, slot 1 f_fake; rows 0 .. 63 of the stage are the tile's rows (X), 64 .. 127 its columns (Y)
  const int* idx_x = idx + (subset * 2 + (family == 1 ? 1 : 0)) * (long)m;
  const int* idx_y = idx + (subset * 2 + (family == 0 ? 0 : 1)) * (long)m;
  const float* fx = family == 1 ? f_fake : f_real;
  const float* fy = family == 0 ? f_real : f_fake;
  const int nx = family == 1 ? n_fake : n_real, ny = family == 0 ? n_real : n_fake;
  const float* src[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int e = tid + 256 * p, row = e >> 3;
    const bool is_y = row >= 64;
    int pos = (is_y ? tj : ti) * 64 + (row & 63);
    pos = pos < m ? pos : m - 1;                       // beyond the subset: any valid row, masked in the epilogue
    int g = (is_y ? idx_y : idx_x)[pos];
    const int n = is_y ? ny : nx;
    g = g < 0 ? 0 : (g >= n ? n - 1 : g);              // never out of bounds (the host validates: no clamp in a correct call)
    src[p] = (is_y ? fy : fx) + (size_t)g * d + 4 * (e & 7);
  }
  f64x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
  f32x4 nxt[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) nxt[p] = *(const f32x4*)(src[p]);
  const float* arow = stage + ((wave >> 1) * 32 + r) * KID_LD + q;
  const float* brow = stage + (64 + (wave & 1) * 32 + r) * KID_LD + q;
  for (int k0 = 0; k0 < d; k0 += KID_KC) {
    __syncthreads();                                   // the previous step's reads are done
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int e = tid + 256 * p;
      *(f32x4*)(stage + (e >> 3) * KID_LD + 4 * (e & 7)) = nxt[p];
    }
    __syncthreads();
    const int kn = k0 + KID_KC < d ? k0 + KID_KC : k0;      // the last step loads its own columns again: in bounds, unused
#pragma unroll
    for (int p = 0; p < 4; ++p) nxt[p] = *(const f32x4*)(src[p] + kn);
#pragma unroll
    for (int kk = 0; kk < KID_KC; kk += 4) {
      double av[2], bv[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        av[u] = (double)arow[16 * u * KID_LD + kk];
        bv[u] = (double)brow[16 * u * KID_LD + kk];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
  }
  // epilogue in registers: (dot gamma + coef)^degree by repeated multiplication; outside the subset and, for xx / yy, on the
  // diagonal of POSITIONS (not of gathered row ids) an exact zero.  Sum: lane (i, j, reg order), wave (butterfly), workgroup.
  const bool diag = family != 2;
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int row = ti * 64 + (wave >> 1) * 32 + 16 * i + q + 4 * g;
        const int col = tj * 64 + (wave & 1) * 32 + 16 * j + r;
        const double base = acc[i][j][g] * gamma + coef;
        double v = base;
        for (int e = 1; e < degree; ++e) v = v * base;
        const bool live = row < m && col < m && !(diag && row == col);
        s = s + (live ? v : 0.0);
      }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s = s + __shfl_xor(s, o, 64);
  if (lane == 0) wave_sum[wave] = s;
  __syncthreads();
  if (tid == 0) {
    double w = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
    if (diag && tj != ti) w = w * 2.0;
    partial[blockIdx.x] = w;
  }
}

// one thread per subset: the tile partials in tile order, then (S_xx + S_yy) / (m (m - 1)) - 2 S_xy / m^2 as written
__global__ __launch_bounds__(256) void kid_finish_kernel(const double* __restrict__ partial, int subsets, int m, long tiles, double* __restrict__ sums,
                                                         double* __restrict__ out) {
#pragma clang fp contract(off)
  const int sub = blockIdx.x * 256 + threadIdx.x;
  if (sub >= subsets) return;
  const long T = (m + 63) >> 6, tri = kid_tri(T);
  const double* p = partial + (long)sub * tiles;
  double sxx = 0.0, syy = 0.0, sxy = 0.0;
  for (long t = 0; t < tri; ++t) sxx = sxx + p[t];
  for (long t = tri; t < 2 * tri; ++t) syy = syy + p[t];
  for (long t = 2 * tri; t < tiles; ++t) sxy = sxy + p[t];
  if (sums) { sums[3 * sub] = sxx; sums[3 * sub + 1] = syy; sums[3 * sub + 2] = sxy; }
  const double dm = (double)m;
  const double first = (sxx + syy) / (dm * (dm - 1.0));
  const double second = (2.0 * sxy) / (dm * dm);
  out[sub] = first - second;
}

// ---------------------------------------------------------------- logits = f . W^T, fp32
// Workgroup: four classes (one per wave) against up to eight rows.  A lane multiplies the 16-byte chunks k = 4 lane, 4 lane + 256,
// ... of its row and class in that order into ONE fp32 accumulator per row (fma), then the wave adds its 64 lanes in a butterfly:
// the order is a function of d alone, so a row's logits are the same bits alone and inside any batch.
constexpr int FC_ROWS = 8;
__global__ __launch_bounds__(256) void fc_logits_kernel(const float* __restrict__ f, int n, int d, const float* __restrict__ w, int classes,
                                                        float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 4 + wave;
  if (c >= classes) return;
  const int row0 = blockIdx.y * FC_ROWS;
  const int rows = n - row0 < FC_ROWS ? n - row0 : FC_ROWS;
  float acc[FC_ROWS];
#pragma unroll
  for (int i = 0; i < FC_ROWS; ++i) acc[i] = 0.f;
  const float* wr = w + (size_t)c * d;
  for (int k = 4 * lane; k < d; k += 256) {
    const f32x4 wv = *(const f32x4*)(wr + k);
#pragma unroll
    for (int i = 0; i < FC_ROWS; ++i) {
      if (i < rows) {
        const f32x4 x = *(const f32x4*)(f + (size_t)(row0 + i) * d + k);
        acc[i] = fmaf(x.x, wv.x, acc[i]);
        acc[i] = fmaf(x.y, wv.y, acc[i]);
        acc[i] = fmaf(x.z, wv.z, acc[i]);
        acc[i] = fmaf(x.w, wv.w, acc[i]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < FC_ROWS; ++i) {
    float s = acc[i];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0 && i < rows) out[(size_t)(row0 + i) * classes + c] = s;
  }
}

// ---------------------------------------------------------------- the Inception-score head, fp64 from the fp32 logits
// (a) one wave per row: the maximum, then lse = max + log(sum exp(x - max)): a lane adds the classes lane, lane + 64, ... in order,
//     the wave its lanes in a butterfly
__global__ __launch_bounds__(256) void is_lse_kernel(const float* __restrict__ logits, int n, int classes, double* __restrict__ lse) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const float* x = logits + (size_t)row * classes;
  float mx = -INFINITY;
  for (int c = lane; c < classes; c += 64) mx = fmaxf(mx, x[c]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  const double dmx = (double)mx;
  double s = 0.0;
  for (int c = lane; c < classes; c += 64) s = s + exp((double)x[c] - dmx);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s = s + __shfl_xor(s, o, 64);
  if (lane == 0) lse[row] = dmx + log(s);
}

// (b) one thread per (chunk, class): log(mean_p) with mean_p = (sum over the chunk's rows, in row order, of exp(x - lse)) / rows;
//     row j of the permuted order is row perm[j] of the logits
__global__ __launch_bounds__(256) void is_mean_kernel(const float* __restrict__ logits, int n, int classes, const int* __restrict__ perm, int chunk,
                                                      int n_chunks, const double* __restrict__ lse, double* __restrict__ log_mean) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)n_chunks * classes) return;
  const int k = (int)(i / classes), c = (int)(i - (long)k * classes);
  const int j0 = k * chunk, j1 = j0 + chunk < n ? j0 + chunk : n;
  double s = 0.0;
  for (int j = j0; j < j1; ++j) {
    int row = perm[j];
    row = row < 0 ? 0 : (row >= n ? n - 1 : row);
    s = s + exp((double)logits[(size_t)row * classes + c] - lse[row]);
  }
  log_mean[i] = log(s / (double)(j1 - j0));
}

// (c) one workgroup per chunk; a thread owns rows: kl = sum over the classes, in class order, of p ((x - lse) - log mean_p) with
//     p = exp(x - lse); then thread 0 adds the chunk's kl in row order and writes exp(mean)
__global__ __launch_bounds__(256) void is_kl_kernel(const float* __restrict__ logits, int n, int classes, const int* __restrict__ perm, int chunk,
                                                    const double* __restrict__ lse, const double* __restrict__ log_mean, double* __restrict__ kl,
                                                    double* __restrict__ out) {
#pragma clang fp contract(off)
  const int k = blockIdx.x;
  const int j0 = k * chunk, j1 = j0 + chunk < n ? j0 + chunk : n;
  const double* lm = log_mean + (size_t)k * classes;
  for (int j = j0 + threadIdx.x; j < j1; j += 256) {
    int row = perm[j];
    row = row < 0 ? 0 : (row >= n ? n - 1 : row);
    const float* x = logits + (size_t)row * classes;
    const double l = lse[row];
    double s = 0.0;
    for (int c = 0; c < classes; ++c) {
      const double lp = (double)x[c] - l;
      s = s + exp(lp) * (lp - lm[c]);
    }
    kl[j] = s;
  }
  __syncthreads();      // the workgroup's own global writes are visible to it behind the barrier
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int j = j0; j < j1; ++j) s = s + kl[j];
    out[k] = exp(s / (double)(j1 - j0));
  }
}

int64_t kid_ws_bytes(int subsets, int m) {
  if (subsets < 1 || m < 2) return -1;
  const long T = (m + 63) / 64;
  return (int64_t)align256((size_t)subsets * kid_tiles(T) * sizeof(double));
}

struct IsLayout { int chunk, n_chunks; size_t lse, log_mean, kl, total; };
bool is_layout(int n, int classes, int splits, IsLayout* L) {
  if (n < 1 || classes < 1 || splits < 1) return false;
  L->chunk = (int)(((long)n + splits - 1) / splits);
  L->n_chunks = (n + L->chunk - 1) / L->chunk;
  L->lse = 0;
  L->log_mean = align256((size_t)n * sizeof(double));
  L->kl = L->log_mean + align256((size_t)L->n_chunks * classes * sizeof(double));
  L->total = L->kl + align256((size_t)n * sizeof(double));
  return true;
}

}  // namespace

extern "C" {

int64_t mvd_op_kid_workspace_bytes(int subsets, int m) {
  const int64_t b = kid_ws_bytes(subsets, m);
  if (b < 0) mvd_set_error("kid_workspace_bytes: subsets >= 1 and m >= 2 required (got %d, %d)", subsets, m);
  return b;
}

int mvd_op_kid_mmd(const float* f_real, int n_real, const float* f_fake, int n_fake, int d, const int* idx, int subsets, int m, int degree, double gamma,
                   double coef, void* ws, int64_t ws_bytes, double* sums, double* out, void* stream) {
  if (!f_real || !f_fake || !idx || !out || !ws) { mvd_set_error("kid_mmd: null pointer"); return -1; }
  if (subsets < 1 || m < 2 || n_real < 1 || n_fake < 1 || m > n_real || m > n_fake) {
    mvd_set_error("kid_mmd: subsets >= 1 and 2 <= m <= min(n_real, n_fake) required (subsets %d, m %d, n_real %d, n_fake %d)", subsets, m, n_real, n_fake);
    return -1;
  }
  if (d < 64 || d % 64) { mvd_set_error("kid_mmd: d = %d must be a positive multiple of 64", d); return -1; }
  if (degree < 1) { mvd_set_error("kid_mmd: degree = %d must be at least 1", degree); return -1; }
  if ((((uintptr_t)f_real | (uintptr_t)f_fake) & 15) || ((uintptr_t)idx & 3) || (((uintptr_t)ws | (uintptr_t)out | (uintptr_t)sums) & 7)) {
    mvd_set_error("kid_mmd: misaligned buffer (features 16 bytes, idx 4, workspace / sums / out 8)");
    return -1;
  }
  const long tiles = kid_tiles((m + 63) / 64);
  const long blocks = tiles * subsets;
  if (blocks >= (1L << 31)) { mvd_set_error("kid_mmd: %ld tiles are too many for one launch", blocks); return -1; }
  const int64_t need = kid_ws_bytes(subsets, m);
  if (ws_bytes < need) { mvd_set_error("kid_mmd: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need); return -4; }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(kid_mmd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, f_real, n_real, f_fake, n_fake, d, idx, m, degree, gamma, coef, tiles,
                     (double*)ws);
  CHECK(launch_check("kid_mmd"));
  hipLaunchKernelGGL(kid_finish_kernel, dim3((unsigned)((subsets + 255) / 256)), dim3(256), 0, s, (const double*)ws, subsets, m, tiles, sums, out);
  return launch_check("kid_mmd (finish)");
}

int mvd_op_fc_logits(const float* f, int n, int d, const float* w, int classes, float* out, void* stream) {
  if (!f || !w || !out || n < 1 || classes < 1 || d < 4 || d % 4) { mvd_set_error("fc_logits: bad argument (n, classes >= 1, d a multiple of 4)"); return -1; }
  if ((((uintptr_t)f | (uintptr_t)w) & 15) || ((uintptr_t)out & 3)) { mvd_set_error("fc_logits: misaligned buffer"); return -1; }
  const long by = ((long)n + FC_ROWS - 1) / FC_ROWS;
  if (by > 65535) { mvd_set_error("fc_logits: n = %d is too many rows for one launch (at most %d)", n, 65535 * FC_ROWS); return -1; }
  hipLaunchKernelGGL(fc_logits_kernel, dim3((unsigned)((classes + 3) / 4), (unsigned)by), dim3(256), 0, (hipStream_t)stream, f, n, d, w, classes, out);
  return launch_check("fc_logits");
}

int64_t mvd_op_inception_score_workspace_bytes(int n, int classes, int splits) {
  IsLayout L;
  if (!is_layout(n, classes, splits, &L)) { mvd_set_error("inception_score_workspace_bytes: n, classes, splits >= 1 required"); return -1; }
  return (int64_t)L.total;
}

int mvd_op_inception_score(const float* logits, int n, int classes, const int* perm, int splits, void* ws, int64_t ws_bytes, double* out, int* n_chunks_out,
                           void* stream) {
  IsLayout L;
  if (!logits || !perm || !ws || !out || !is_layout(n, classes, splits, &L)) {
    mvd_set_error("inception_score: bad argument (n, classes, splits >= 1, no null pointer)");
    return -1;
  }
  if (((uintptr_t)logits & 3) || ((uintptr_t)perm & 3) || (((uintptr_t)ws | (uintptr_t)out) & 7)) { mvd_set_error("inception_score: misaligned buffer"); return -1; }
  if (ws_bytes < (int64_t)L.total) { mvd_set_error("inception_score: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)L.total); return -4; }
  const long mean_blocks = ((long)L.n_chunks * classes + 255) / 256;
  if (mean_blocks >= (1L << 31)) { mvd_set_error("inception_score: too many (chunk, class) pairs for one launch"); return -1; }
  if (n_chunks_out) *n_chunks_out = L.n_chunks;
  hipStream_t s = (hipStream_t)stream;
  double* lse = (double*)((char*)ws + L.lse);
  double* log_mean = (double*)((char*)ws + L.log_mean);
  double* kl = (double*)((char*)ws + L.kl);
  hipLaunchKernelGGL(is_lse_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, logits, n, classes, lse);
  CHECK(launch_check("inception_score (lse)"));
  hipLaunchKernelGGL(is_mean_kernel, dim3((unsigned)mean_blocks), dim3(256), 0, s, logits, n, classes, perm, L.chunk, L.n_chunks, (const double*)lse, log_mean);
  CHECK(launch_check("inception_score (mean)"));
  hipLaunchKernelGGL(is_kl_kernel, dim3((unsigned)L.n_chunks), dim3(256), 0, s, logits, n, classes, perm, L.chunk, (const double*)lse,
                     (const double*)log_mean, kl, out);
  return launch_check("inception_score (kl)");
}

}  // extern "C"
