// Improved precision / recall (Kynkaanniemi et al. 2019, torch-fidelity's `prc`) and density / coverage (Naeem et al. 2020, the
// `prdc` package) on the FID tower's pool3 features: everything after the network.
//
//   D2(a, b) = max(0, (|a|^2 + |b|^2) - 2 a.b) in fp64 from the fp32 rows: the dot product on v_mfma_f64_16x16x4_f64 over d in
//   order, never split; a norm is the fma chain of a row's squares in the order written at gram_tile.  Every comparison is on
//   SQUARED distances (exact for integer inputs, equivalent to comparing Euclidean distances).
//
//   knn_radii_kernel        a workgroup owns a 64-row strip of F and walks the 64-column tiles of its column part; per row the k + 1
//                           smallest D2 seen so far (the row's own diagonal entry counts), one owner thread per row, in LDS;
//                           only candidates below the row's current (k + 1)-th smallest are queued for the owner
//   knn_merge_kernel        per row the k + 1 smallest of the parts' lists -> radii_sq[i] = the (k + 1)-th smallest of row i of
//                           D2(F, F) = kthvalue(k + 1), and optionally the whole sorted list
//   manifold_counts_kernel  one 64 x 64 tile of queries x references: P[j][i] = D2(q_j, r_i) (<= or <) radii_sq[i] in registers,
//                           the tile's row sums added into hits_per_query and its column sums into hits_per_ref (int32 atomics:
//                           integer sums are exact in any order)
//
// No n x n matrix is written anywhere and there is no floating-point atomic: the k + 1 smallest values of a multiset do not
// depend on the order they are met in, so two calls give the same bits.
#include <stdio.h>
#include <string.h>

#include "host_util.h"

typedef __attribute__((ext_vector_type(4))) double f64x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

namespace {

constexpr int PR_KC = 32;             // K elements staged per step
constexpr int PR_LD = PR_KC + 4;      // LDS row stride in floats: 16-byte rows, lane (q, r) reads bank 4 r + q of 64 (kid_mmd_kernel's stage)
constexpr int PR_STAGE_BYTES = 128 * PR_LD * 4;
constexpr int PR_CAND_LD = 65;        // doubles: the owner of row l reads word 130 l + 2 c: 32 lanes cover the 64 banks
constexpr int PR_CAND_BYTES = 64 * PR_CAND_LD * 8;
constexpr int PR_KMAX = 15;
constexpr int PR_LIST_LD = PR_KMAX + 2;   // doubles, odd: the owners' lists start in different banks

// The 64 x 64 Gram tile X[x0 ..][:] . Y[y0 ..][:]^T of kid_mmd_kernel: wave = a 32 x 32 quadrant = 2 x 2 MFMA tiles; the 64 + 64
// rows staged through LDS in fp32, PR_KC columns at a time, coalesced 16-byte loads with the next step's in flight, converted to
// fp64 on read; A lane l holds X[row l & 15][k + (l >> 4)], B the same for Y; D: col = l & 15, row = (l >> 4) + 4 reg.  A row
// beyond its matrix reads the last row instead (never out of bounds; the callers mask it).
// Norms: the eight threads that stage a row each run ONE fma chain over their four columns of every step, in column order; the
// eight chains are added in a three-stage butterfly (xor 1, 2, 4).  norms[0 .. 63] the X rows, [64 .. 127] the Y rows.
// Ends behind a barrier: the norms are visible and nobody reads the stage any more.
__device__ __forceinline__ void gram_tile(const float* __restrict__ fx, int nx, int x0, const float* __restrict__ fy, int ny, int y0, int d,
                                          float* stage, double* norms, f64x4 (&acc)[2][2]) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const float* src[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int e = tid + 256 * p, row = e >> 3;
    const bool is_y = row >= 64;
    int g = (is_y ? y0 : x0) + (row & 63);
    const int n = is_y ? ny : nx;
    g = g < n ? g : n - 1;
    src[p] = (is_y ? fy : fx) + (size_t)g * d + 4 * (e & 7);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
  double nacc[4] = {0.0, 0.0, 0.0, 0.0};
  f32x4 nxt[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) nxt[p] = *(const f32x4*)(src[p]);
  const float* arow = stage + ((wave >> 1) * 32 + r) * PR_LD + q;
  const float* brow = stage + (64 + (wave & 1) * 32 + r) * PR_LD + q;
  for (int k0 = 0; k0 < d; k0 += PR_KC) {
    __syncthreads();                                   // the previous step's reads are done
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int e = tid + 256 * p;
      *(f32x4*)(stage + (e >> 3) * PR_LD + 4 * (e & 7)) = nxt[p];
      const double a = (double)nxt[p].x, b = (double)nxt[p].y, c = (double)nxt[p].z, w = (double)nxt[p].w;
      nacc[p] = fma(a, a, nacc[p]);
      nacc[p] = fma(b, b, nacc[p]);
      nacc[p] = fma(c, c, nacc[p]);
      nacc[p] = fma(w, w, nacc[p]);
    }
    __syncthreads();
    const int kn = k0 + PR_KC < d ? k0 + PR_KC : k0;      // the last step loads its own columns again: in bounds, unused
#pragma unroll
    for (int p = 0; p < 4; ++p) nxt[p] = *(const f32x4*)(src[p] + kn);
#pragma unroll
    for (int kk = 0; kk < PR_KC; kk += 4) {
      double av[2], bv[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        av[u] = (double)arow[16 * u * PR_LD + kk];
        bv[u] = (double)brow[16 * u * PR_LD + kk];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    double s = nacc[p];
    s = s + __shfl_xor(s, 1, 64);
    s = s + __shfl_xor(s, 2, 64);
    s = s + __shfl_xor(s, 4, 64);
    if ((tid & 7) == 0) norms[(tid >> 3) + 32 * p] = s;
  }
  __syncthreads();
}

__device__ __forceinline__ double dist2(double na, double nb, double dot) {
#pragma clang fp contract(off)
  const double t = (na + nb) - 2.0 * dot;
  return t < 0.0 ? 0.0 : t;
}

// l[0 .. k] ascending, v < l[k]: v goes to its place and l[k] drops out -> the new l[k].  Equal values are interchangeable, so
// where v lands among them does not matter.
__device__ __forceinline__ double list_insert(double* l, int k, double v) {
  int j = k;
  while (j > 0) {
    const double p = l[j - 1];
    if (!(p > v)) break;
    l[j] = p;
    --j;
  }
  l[j] = v;
  return l[k];
}

// grid (strips, parts); part p walks the column tiles [p tiles / parts, (p + 1) tiles / parts).  After a tile's K loop every lane
// compares its 16 D2 values with the row's current (k + 1)-th smallest and queues the survivors -- columns < n that are smaller,
// nothing else -- in the row's LDS queue (aliasing the operand stage; the slot comes from an integer LDS counter, so the queue's
// order varies, which the k + 1 smallest of a multiset do not depend on); thread l < 64 then offers row l's queue to the row's
// list.  A part's first tile queues all 64 columns, later tiles a few.  part_lists[part][row][k + 1], +inf where the part had
// fewer than k + 1 columns.
__global__ __launch_bounds__(256) void knn_radii_kernel(const float* __restrict__ f, int n, int d, int k, int tiles, int parts,
                                                        double* __restrict__ part_lists) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) char buf[PR_CAND_BYTES > PR_STAGE_BYTES ? PR_CAND_BYTES : PR_STAGE_BYTES];
  __shared__ double norms[128];
  __shared__ double lists[64 * PR_LIST_LD];
  __shared__ int queued[64];
  float* stage = (float*)buf;
  double* cand = (double*)buf;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int row0 = blockIdx.x * 64, part = blockIdx.y;
  const int t0 = (int)((long)part * tiles / parts), t1 = (int)((long)(part + 1) * tiles / parts);
  double* my = lists + tid * PR_LIST_LD;      // used by tid < 64 only
  if (tid < 64)
    for (int j = 0; j <= k; ++j) my[j] = INFINITY;
  double worst = INFINITY;
  for (int t = t0; t < t1; ++t) {
    const int col0 = t * 64;
    if (tid < 64) queued[tid] = 0;      // the barriers of gram_tile lie between this and the first increment
    f64x4 acc[2][2];
    gram_tile(f, n, row0, f, n, col0, d, stage, norms, acc);
    // (every wave is behind the first barrier of this tile's gram_tile only after the owners finished the previous tile: the
    // lists are at rest here)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int row = (wave >> 1) * 32 + 16 * i + q + 4 * g;
        const double nrow = norms[row], limit = lists[row * PR_LIST_LD + k];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int col = (wave & 1) * 32 + 16 * j + r;
          const double v = dist2(nrow, norms[64 + col], acc[i][j][g]);
          if (col0 + col < n && v < limit) {      // columns >= n never become candidates
            const int slot = atomicAdd(&queued[row], 1);      // < 64: one per column of the tile at most
            cand[row * PR_CAND_LD + slot] = v;
          }
        }
      }
    __syncthreads();
    if (tid < 64) {
      const int m = queued[tid];
      const double* c = cand + tid * PR_CAND_LD;
      for (int s = 0; s < m; ++s) {
        const double v = c[s];
        if (v < worst) worst = list_insert(my, k, v);
      }
    }
    // the next tile's first barrier (gram_tile) comes before anything is written to the stage: the owners' reads are done then
  }
  if (tid < 64 && row0 + tid < n) {
    double* out = part_lists + ((size_t)part * n + row0 + tid) * (k + 1);
    for (int j = 0; j <= k; ++j) out[j] = my[j];
  }
}

// one thread per row: the k + 1 smallest of the parts' (k + 1)-lists, with the same list code
__global__ __launch_bounds__(64) void knn_merge_kernel(const double* __restrict__ part_lists, int n, int k, int parts, double* __restrict__ radii_sq,
                                                       double* __restrict__ knn_sq) {
  __shared__ double lists[64 * PR_LIST_LD];
  const int row = blockIdx.x * 64 + threadIdx.x;
  if (row >= n) return;
  double* my = lists + threadIdx.x * PR_LIST_LD;
  for (int j = 0; j <= k; ++j) my[j] = INFINITY;
  double worst = INFINITY;
  for (int p = 0; p < parts; ++p) {
    const double* in = part_lists + ((size_t)p * n + row) * (k + 1);
    for (int j = 0; j <= k; ++j) {
      const double v = in[j];
      if (v < worst) worst = list_insert(my, k, v);
    }
  }
  radii_sq[row] = my[k];
  if (knn_sq)
    for (int j = 0; j <= k; ++j) knn_sq[(size_t)row * (k + 1) + j] = my[j];
}

// grid (reference tiles, query tiles).  Epilogue in registers; a lane's 16 predicate bits: rows q + 4 g + 16 i, columns r + 16 j.
// Row sums: a lane's two columns, then the 16 lanes of equal q; column sums: a lane's eight rows, then the 4 lanes of equal r.
__global__ __launch_bounds__(256) void manifold_counts_kernel(const float* __restrict__ fq, int nq, const float* __restrict__ fr, int nr, int d,
                                                              const double* __restrict__ radii_sq, int closed, int* __restrict__ hits_per_query,
                                                              int* __restrict__ hits_per_ref) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float stage[128 * PR_LD];
  __shared__ double norms[128];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int row0 = blockIdx.y * 64, col0 = blockIdx.x * 64;
  f64x4 acc[2][2];
  gram_tile(fq, nq, row0, fr, nr, col0, d, stage, norms, acc);
  int row_hits[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, col_hits[2] = {0, 0};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int lcol = (wave & 1) * 32 + 16 * j + r, col = col0 + lcol;
    const bool col_live = col < nr;
    const double rad = col_live ? radii_sq[col] : 0.0;
    const double ncol = norms[64 + lcol];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int lrow = (wave >> 1) * 32 + 16 * i + q + 4 * g;
        const double d2 = dist2(norms[lrow], ncol, acc[i][j][g]);
        const bool hit = col_live && row0 + lrow < nq && (closed ? d2 <= rad : d2 < rad);
        row_hits[i][g] += hit ? 1 : 0;
        col_hits[j] += hit ? 1 : 0;
      }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      int s = row_hits[i][g];
#pragma unroll
      for (int o = 1; o <= 8; o <<= 1) s += __shfl_xor(s, o, 64);
      const int row = row0 + (wave >> 1) * 32 + 16 * i + q + 4 * g;
      if (hits_per_query && r == 0 && s > 0 && row < nq) atomicAdd(hits_per_query + row, s);
    }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int s = col_hits[j];
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    const int col = col0 + (wave & 1) * 32 + 16 * j + r;
    if (hits_per_ref && q == 0 && s > 0 && col < nr) atomicAdd(hits_per_ref + col, s);
  }
}

// column parts of the k-NN pass, never more than tiles.  0 = automatic: about 2048 workgroups -- eight per compute unit of a 256-CU
// chip, of which three are resident, so that the last round of equally long workgroups leaves few units idle (at 10000 rows,
// 628 workgroups of 39 tiles cost 1.27 x the time of the same tiles as single-tile workgroups) -- but at least two tiles a part,
// because a part's first tile queues every column
int knn_parts(int n, int force_parts) {
  const int tiles = (n + 63) / 64;
  if (force_parts > 0) return force_parts < tiles ? force_parts : tiles;
  const int by_fill = (2048 + tiles - 1) / tiles, by_tiles = tiles / 2 > 1 ? tiles / 2 : 1;
  return by_fill < by_tiles ? by_fill : by_tiles;
}
bool knn_args_ok(int n, int k, int force_parts) { return k >= 1 && k <= PR_KMAX && n >= k + 1 && force_parts >= 0 && force_parts <= 65535; }
int64_t knn_ws_bytes(int n, int k, int force_parts) { return (int64_t)align256((size_t)knn_parts(n, force_parts) * n * (k + 1) * sizeof(double)); }

}  // namespace

extern "C" {

int64_t mvd_op_knn_radii_workspace_bytes(int n, int k, int force_parts) {
  if (!knn_args_ok(n, k, force_parts)) {
    mvd_set_error("knn_radii_workspace_bytes: 1 <= k <= %d, n >= k + 1 and 0 <= force_parts <= 65535 required (n %d, k %d, force_parts %d)", PR_KMAX, n, k,
                  force_parts);
    return -1;
  }
  return knn_ws_bytes(n, k, force_parts);
}

int mvd_op_knn_radii(const float* f, int n, int d, int k, int force_parts, double* radii_sq, double* knn_sq, void* ws, int64_t ws_bytes, void* stream) {
  if (!f || !radii_sq || !ws) { mvd_set_error("knn_radii: null pointer"); return -1; }
  if (!knn_args_ok(n, k, force_parts)) {
    mvd_set_error("knn_radii: 1 <= k <= %d, n >= k + 1 and 0 <= force_parts <= 65535 required (n %d, k %d, force_parts %d)", PR_KMAX, n, k, force_parts);
    return -1;
  }
  if (d < 64 || d % 64) { mvd_set_error("knn_radii: d = %d must be a positive multiple of 64", d); return -1; }
  if (((uintptr_t)f & 15) || (((uintptr_t)radii_sq | (uintptr_t)knn_sq | (uintptr_t)ws) & 7)) {
    mvd_set_error("knn_radii: misaligned buffer (features 16 bytes, radii_sq / knn_sq / workspace 8)");
    return -1;
  }
  const int64_t need = knn_ws_bytes(n, k, force_parts);
  if (ws_bytes < need) { mvd_set_error("knn_radii: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need); return -4; }
  const int tiles = (n + 63) / 64, parts = knn_parts(n, force_parts);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(knn_radii_kernel, dim3((unsigned)tiles, (unsigned)parts), dim3(256), 0, s, f, n, d, k, tiles, parts, (double*)ws);
  CHECK(launch_check("knn_radii"));
  hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)tiles), dim3(64), 0, s, (const double*)ws, n, k, parts, radii_sq, knn_sq);
  return launch_check("knn_radii (merge)");
}

int mvd_op_manifold_counts(const float* q, int nq, const float* r, int nr, int d, const double* r_radii_sq, int closed, int32_t* hits_per_query,
                           int32_t* hits_per_ref, void* stream) {
  if (!q || !r || !r_radii_sq) { mvd_set_error("manifold_counts: null pointer"); return -1; }
  if (nq < 1 || nr < 1) { mvd_set_error("manifold_counts: nq >= 1 and nr >= 1 required (got %d, %d)", nq, nr); return -1; }
  if (d < 64 || d % 64) { mvd_set_error("manifold_counts: d = %d must be a positive multiple of 64", d); return -1; }
  if (closed != 0 && closed != 1) { mvd_set_error("manifold_counts: closed = %d must be 0 (<) or 1 (<=)", closed); return -1; }
  if ((((uintptr_t)q | (uintptr_t)r) & 15) || ((uintptr_t)r_radii_sq & 7) || (((uintptr_t)hits_per_query | (uintptr_t)hits_per_ref) & 3)) {
    mvd_set_error("manifold_counts: misaligned buffer (features 16 bytes, radii 8, counts 4)");
    return -1;
  }
  const long qt = ((long)nq + 63) / 64, rt = ((long)nr + 63) / 64;
  if (qt > 65535) { mvd_set_error("manifold_counts: nq = %d is too many queries for one launch (at most %d)", nq, 65535 * 64); return -1; }
  hipStream_t s = (hipStream_t)stream;
  if ((hits_per_query && hipMemsetAsync(hits_per_query, 0, (size_t)nq * sizeof(int32_t), s) != hipSuccess) ||
      (hits_per_ref && hipMemsetAsync(hits_per_ref, 0, (size_t)nr * sizeof(int32_t), s) != hipSuccess)) {
    mvd_set_error("manifold_counts: zeroing the outputs failed: %s", hipGetErrorString(hipGetLastError()));
    return -3;
  }
  if (!hits_per_query && !hits_per_ref) return 0;
  hipLaunchKernelGGL(manifold_counts_kernel, dim3((unsigned)rt, (unsigned)qt), dim3(256), 0, s, q, nq, r, nr, d, r_radii_sq, closed, (int*)hits_per_query,
                     (int*)hits_per_ref);
  return launch_check("manifold_counts");
}

}  // extern "C"
