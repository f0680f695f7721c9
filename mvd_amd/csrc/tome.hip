// Token merging in front of self-attention (Bolya & Hoffman 2023; tomesd 0.1.x with use_rand = False, sx = sy = 2, restated;
// DESIGN.md section 9 N21).  x is one transformer block's LayerNorm1 output, [B][H*W][C] bf16, token-major.  Per image:
//   dst tokens   the top-left token of every complete 2 x 2 cell, nd = (H / 2)(W / 2) of them, in raster order of the cells
//   src tokens   every other token (a last odd row / column included), ns = H W - nd of them, in ascending token order
//   score(s, d)  x_s . x_d / (|x_s| |x_d|);  best(s) = argmax over d, a tie to the lowest d
//   the r src with the largest score(s, best(s)) (ties: the lower src index, which is the lower token index) are merged
//   merged sequence, N' = H W - r rows: row d < nd is the mean over dst d and the src merged into it, row nd + p the p-th kept src
// Four kernels, no float atomics, an image's bits never depend on the batch around it:
//   match    one wave per 32 src rows, every dst tile of 32 against them on v_mfma_f32_32x32x16_bf16.  Both operands are the RAW
//            bf16 rows, fragments loaded 16 bytes per lane straight from global memory (the map is L2-resident), so every product
//            is exact and the sum is fp32.  The squared norms are accumulated from the same fragments (fp32 FMA) and the division
//            by |x_s| |x_d| happens on the accumulator.  Running (max, argmax) per src row live in registers across the dst tiles;
//            the 32 lanes of a row are combined by a butterfly at the end.  The ns x nd matrix exists nowhere.
//   select   one workgroup of 1024 lanes per image, everything in LDS: a bitonic sort of the 64-bit keys (score descending, src
//            index ascending) ranks the src, the first r are marked, a block prefix sum gives the kept src their rows, and a
//            second bitonic sort of 32-bit keys (row, token) over the dst and the merged src lists every row's members in
//            ascending token order (CSR: starts [N' + 1], members [H W]).  slot [H W]: the merged row of every token.
//   merge    out[j] = bf16(fp32 sum of the members in that order / count); eight channels per lane.
//   unmerge  h[i] = bf16(float(h[i]) + float(t[slot[i]])); eight channels per lane, in place.
// Limits: H W <= MVD_TOME_MAX_TOKENS (the two sorts are 8192 x 8 and 16384 x 4 bytes of LDS), H, W >= 2, C a multiple of 64.
#include <math.h>
#include <stdint.h>

#include <mutex>

#include "host_util.h"

namespace {

constexpr int TM_MAX_TOKENS = MVD_TOME_MAX_TOKENS;      // 9216, 96 x 96 latents at the first level: 6912 src -> 8192 sort keys
constexpr int TM_SELECT_THREADS = 1024;
constexpr int TM_TOKEN_BITS = 14;          // (row, token) member keys: token < 2^14
constexpr int TM_MAX_DEVICES = 64;         // devices whose "asked for the large LDS" state is remembered
constexpr int TM_MATCH_WAVES = 4;          // waves per match workgroup, 32 src rows each

struct TomeGeo { int H, W, Hh, Wh, nd, ns, per; };     // per: src per complete row pair, 2 W - Wh

TomeGeo tome_geo(int H, int W) {
  TomeGeo g;
  g.H = H; g.W = W; g.Hh = H / 2; g.Wh = W / 2; g.nd = g.Hh * g.Wh; g.ns = H * W - g.nd; g.per = 2 * W - g.Wh;
  return g;
}
int pow2_at_least(int n) { int p = 1; while (p < n) p <<= 1; return p; }

MVD_DEVINL int tome_src_token(const TomeGeo& g, int s) {
  const int p = s / g.per;
  if (p >= g.Hh) return 2 * g.Hh * g.W + (s - g.Hh * g.per);          // the odd last row: all of it
  const int rem = s - p * g.per, e = g.W - g.Wh;
  if (rem < e) return 2 * p * g.W + (rem < g.Wh ? 2 * rem + 1 : g.Wh + rem);     // even row: odd columns, then an odd last column
  return (2 * p + 1) * g.W + (rem - e);                                   // odd row: all of it
}
MVD_DEVINL int tome_dst_token(const TomeGeo& g, int d) { return 2 * (d / g.Wh) * g.W + 2 * (d % g.Wh); }

MVD_DEVINL float sumsq8(const u32x4& v, float acc) {
  float f;
  f = bflo(v.x); acc = fmaf(f, f, acc); f = bfhi(v.x); acc = fmaf(f, f, acc);
  f = bflo(v.y); acc = fmaf(f, f, acc); f = bfhi(v.y); acc = fmaf(f, f, acc);
  f = bflo(v.z); acc = fmaf(f, f, acc); f = bfhi(v.z); acc = fmaf(f, f, acc);
  f = bflo(v.w); acc = fmaf(f, f, acc); f = bfhi(v.w); acc = fmaf(f, f, acc);
  return acc;
}
MVD_DEVINL void unpack8(const u32x4& v, float* f) {
  f[0] = bflo(v.x); f[1] = bfhi(v.x); f[2] = bflo(v.y); f[3] = bfhi(v.y);
  f[4] = bflo(v.z); f[5] = bfhi(v.z); f[6] = bflo(v.w); f[7] = bfhi(v.w);
}

// ------------------------------------------------------------------------------------------------------------------ match
struct TomeMatchArgs { const bf16_t* x; float* score; int* best; TomeGeo g; int C; };

__global__ __launch_bounds__(TM_MATCH_WAVES * 64) void tome_match_kernel(const TomeMatchArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const TomeGeo g = a.g;
  const int b = blockIdx.y, C = a.C;
  const int s0 = ((int)blockIdx.x * TM_MATCH_WAVES + wave) * 32;
  if (s0 >= g.ns) return;                                      // (wave-uniform; the kernel has no barrier)
  const bf16_t* xb = a.x + (long)b * g.H * g.W * C;
  // fragment of lane (r, h): elements k + 8 h .. k + 8 h + 7 of row r -- the A and the B lane map of the 32x32x16 MFMA alike
  const int s_mine = s0 + r < g.ns ? s0 + r : g.ns - 1;        // (rows past the end repeat the last one; they are not written)
  const bf16_t* arow = xb + (long)tome_src_token(g, s_mine) * C + 8 * h;
  float na = 0.f;
  for (int k = 0; k < C; k += 16) na = sumsq8(*reinterpret_cast<const u32x4*>(arow + k), na);
  na += __shfl_xor(na, 32, 64);
  na = sqrtf(na);
  float ra[16], bs[16]; int bi[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {                               // accumulator register q of this lane: row (q & 3) + 8 (q >> 2) + 4 h
    ra[q] = __shfl(na, (q & 3) + 8 * (q >> 2) + 4 * h, 64);
    bs[q] = -INFINITY; bi[q] = 0;
  }
  for (int d0 = 0; d0 < g.nd; d0 += 32) {
    const int d = d0 + r;
    const bf16_t* brow = xb + (long)tome_dst_token(g, d < g.nd ? d : g.nd - 1) * C + 8 * h;
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    float nb = 0.f;
    for (int k = 0; k < C; k += 16) {
      const u32x4 av = *reinterpret_cast<const u32x4*>(arow + k), bv = *reinterpret_cast<const u32x4*>(brow + k);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, bv), acc, 0, 0, 0);
      nb = sumsq8(bv, nb);
    }
    nb += __shfl_xor(nb, 32, 64);
    nb = sqrtf(nb);
    if (d < g.nd) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const float sc = acc[q] / (ra[q] * nb);
        if (sc > bs[q]) { bs[q] = sc; bi[q] = d; }               // (strict: within a lane d ascends, the lowest index stays)
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) {
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
      const float os = __shfl_xor(bs[q], o, 64); const int oi = __shfl_xor(bi[q], o, 64);
      if (os > bs[q] || (os == bs[q] && oi < bi[q])) { bs[q] = os; bi[q] = oi; }
    }
  }
  if (r == 0) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int s = s0 + (q & 3) + 8 * (q >> 2) + 4 * h;
      if (s < g.ns) { a.score[(long)b * g.ns + s] = bs[q]; a.best[(long)b * g.ns + s] = bi[q]; }
    }
  }
}

// ----------------------------------------------------------------------------------------------------------------- select
template <class K> MVD_DEVINL void bitonic_sort(K* key, int n, int tid) {        // ascending; n a power of two; ends on a barrier
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < (n >> 1); i += TM_SELECT_THREADS) {
        const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
        const K x = key[lo], y = key[hi];
        if ((x > y) == ((lo & k) == 0)) { key[lo] = y; key[hi] = x; }
      }
      __syncthreads();
    }
}

struct TomeSelectArgs { const float* score; const int* best; int* slot; int* members; int* starts; TomeGeo g; int r, n2, m2, sort_bytes; };

__global__ __launch_bounds__(TM_SELECT_THREADS) void tome_select_kernel(const TomeSelectArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tm_lds[];
  unsigned long long* k64 = reinterpret_cast<unsigned long long*>(tm_lds);     // [n2]: the score keys ...
  unsigned int* k32 = reinterpret_cast<unsigned int*>(tm_lds);                 // [m2]: ... and after them the member keys
  int* flag = reinterpret_cast<int*>(tm_lds + a.sort_bytes);                   // [ns]: 1 = merged
  int* wsum = flag + a.g.ns;                                                   // [16]: kept src per wave
  const TomeGeo g = a.g;
  const int tid = threadIdx.x, b = blockIdx.x, HW = g.H * g.W, r = a.r;
  const float* score = a.score + (long)b * g.ns;
  const int* best = a.best + (long)b * g.ns;
  int* slot = a.slot + (long)b * HW;
  int* members = a.members + (long)b * HW;
  int* starts = a.starts + (long)b * (HW - r + 1);
  // ---- rank the src: key = (descending score, ascending index); padding sorts last
  for (int i = tid; i < a.n2; i += TM_SELECT_THREADS) {
    unsigned long long key = ~0ull;
    if (i < g.ns) {
      unsigned int u = __float_as_uint(score[i]);
      u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);                           // unsigned order = float order
      key = ((unsigned long long)(~u) << 32) | (unsigned int)i;
    }
    k64[i] = key;
  }
  __syncthreads();
  bitonic_sort(k64, a.n2, tid);
  for (int i = tid; i < g.ns; i += TM_SELECT_THREADS) flag[(int)(k64[i] & 0xffffffffu)] = i < r ? 1 : 0;
  __syncthreads();
  // ---- rows of the kept src: exclusive prefix sum in src order (a contiguous chunk per lane, waves combined in order)
  const int chunk = (g.ns + TM_SELECT_THREADS - 1) / TM_SELECT_THREADS;
  const int c0 = tid * chunk < g.ns ? tid * chunk : g.ns, c1 = c0 + chunk < g.ns ? c0 + chunk : g.ns;
  int mine = 0;
  for (int s = c0; s < c1; ++s) mine += 1 - flag[s];
  int incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o, 64); if ((tid & 63) >= o) incl += v; }
  if ((tid & 63) == 63) wsum[tid >> 6] = incl;
  __syncthreads();
  int p = incl - mine;
  for (int w = 0; w < (tid >> 6); ++w) p += wsum[w];
  for (int s = c0; s < c1; ++s) {
    const int tok = tome_src_token(g, s);
    if (flag[s]) slot[tok] = best[s];
    else { slot[tok] = g.nd + p; members[g.nd + r + p] = tok; starts[g.nd + p] = g.nd + r + p; ++p; }
  }
  if (tid == 0) starts[HW - r] = HW;
  for (int d = tid; d < g.nd; d += TM_SELECT_THREADS) slot[tome_dst_token(g, d)] = d;
  // ---- members of the dst rows: (row, token) keys of the dst and the merged src, sorted (the score keys are dead: every lane has
  //      passed the barrier behind the flag loop)
  for (int i = tid; i < a.m2; i += TM_SELECT_THREADS) {
    unsigned int key = ~0u;
    if (i < g.nd) key = ((unsigned int)i << TM_TOKEN_BITS) | (unsigned int)tome_dst_token(g, i);
    else if (i - g.nd < g.ns && flag[i - g.nd]) key = ((unsigned int)best[i - g.nd] << TM_TOKEN_BITS) | (unsigned int)tome_src_token(g, i - g.nd);
    k32[i] = key;
  }
  __syncthreads();
  bitonic_sort(k32, a.m2, tid);
  for (int i = tid; i < g.nd + r; i += TM_SELECT_THREADS) {
    const unsigned int key = k32[i];
    members[i] = (int)(key & ((1u << TM_TOKEN_BITS) - 1));
    if (i == 0 || (k32[i - 1] >> TM_TOKEN_BITS) != (key >> TM_TOKEN_BITS)) starts[key >> TM_TOKEN_BITS] = i;
  }
}

// ------------------------------------------------------------------------------------------------------- merge / un-merge
__global__ __launch_bounds__(256) void tome_merge_kernel(const bf16_t* __restrict__ x, const int* __restrict__ members, const int* __restrict__ starts,
                                                         bf16_t* __restrict__ out, long total, int HW, int C, int Nm) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v >= total) return;
  const int cv = C >> 3;
  const int oc = (int)(v % cv); const long row = v / cv;
  const int b = (int)(row / Nm), j = (int)(row % Nm);
  const int i0 = starts[(long)b * (Nm + 1) + j], i1 = starts[(long)b * (Nm + 1) + j + 1];
  const int* mem = members + (long)b * HW;
  const bf16_t* xb = x + (long)b * HW * C + oc * 8;
  const u32x4 first = *reinterpret_cast<const u32x4*>(xb + (long)mem[i0] * C);
  u32x4 y = first;                                               // one member: the row as it is
  if (i1 - i0 > 1) {
    float acc[8], f[8];
    unpack8(first, acc);
    for (int i = i0 + 1; i < i1; ++i) {
      unpack8(*reinterpret_cast<const u32x4*>(xb + (long)mem[i] * C), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += f[e];
    }
    const float n = (float)(i1 - i0);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = acc[e] / n;
    y = u32x4{pack2bf(acc[0], acc[1]), pack2bf(acc[2], acc[3]), pack2bf(acc[4], acc[5]), pack2bf(acc[6], acc[7])};
  }
  *reinterpret_cast<u32x4*>(out + row * C + oc * 8) = y;
}

__global__ __launch_bounds__(256) void tome_unmerge_add_kernel(bf16_t* __restrict__ h, const bf16_t* __restrict__ t, const int* __restrict__ slot,
                                                               long total, int HW, int C, int Nm) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v >= total) return;
  const int cv = C >> 3;
  const int oc = (int)(v % cv); const long row = v / cv;
  const int b = (int)(row / HW);
  const int j = slot[row];
  float x[8], y[8];
  unpack8(*reinterpret_cast<const u32x4*>(h + row * C + oc * 8), x);
  unpack8(*reinterpret_cast<const u32x4*>(t + ((long)b * Nm + j) * C + oc * 8), y);
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] += y[e];
  *reinterpret_cast<u32x4*>(h + row * C + oc * 8) = u32x4{pack2bf(x[0], x[1]), pack2bf(x[2], x[3]), pack2bf(x[4], x[5]), pack2bf(x[6], x[7])};
}

// the checks every entry shares; -1 and a message for a problem the kernels do not take
int tome_check(const char* who, int B, int H, int W, int C, int r) {
  if (B <= 0 || H < 2 || W < 2) { mvd_set_error("%s: needs batch >= 1 and a map of at least 2 x 2 (one complete cell), got batch %d, %d x %d", who, B, H, W); return -1; }
  if ((long)H * W > TM_MAX_TOKENS) { mvd_set_error("%s: map %d x %d has %ld tokens, the select kernel takes at most %d (its two sorts live in LDS)", who, H, W, (long)H * W, TM_MAX_TOKENS); return -1; }
  if (C <= 0 || (C & 63)) { mvd_set_error("%s: channels must be a positive multiple of 64, got %d", who, C); return -1; }
  const TomeGeo g = tome_geo(H, W);
  if (r < 0 || r > g.ns) { mvd_set_error("%s: r = %d outside [0, %d] (the src tokens of a %d x %d map)", who, r, g.ns, H, W); return -1; }
  if ((long)B * H * W * (C / 8) > 0x7fffffffL * 256) { mvd_set_error("%s: batch %d is too large", who, B); return -1; }
  return 0;
}
size_t tome_select_lds(const TomeGeo& g, int* n2, int* m2, int* sort_bytes) {
  *n2 = pow2_at_least(g.ns); *m2 = pow2_at_least(g.H * g.W);
  const size_t a = (size_t)*n2 * 8, b = (size_t)*m2 * 4;
  *sort_bytes = (int)(a > b ? a : b);
  return (size_t)*sort_bytes + (size_t)g.ns * 4 + 16 * 4;
}

}  // namespace

int64_t mvd_tome_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H < 2 || W < 2) return 0;
  const TomeGeo g = tome_geo(H, W);
  return (int64_t)(2 * align256((size_t)B * g.ns * 4));
}

// match + select: slot [B][H W], members [B][H W], starts [B][H W - r + 1]; score / best [B][ns] go to the caller's arrays or, when
// those are null, live in `ws` (mvd_tome_workspace_bytes).  Every check before the first launch.
int mvd_launch_tome_match(const bf16_t* x, int B, int H, int W, int C, int r, int* slot, int* members, int* starts, float* score, int* best,
                          void* ws, int64_t ws_bytes, hipStream_t stream) {
  CHECK(tome_check("tome_match", B, H, W, C, r));
  if (!x || !slot || !members || !starts) { mvd_set_error("tome_match: null tensor"); return -1; }
  if (((uintptr_t)x & 15) || ((uintptr_t)slot & 3) || ((uintptr_t)members & 3) || ((uintptr_t)starts & 3)) { mvd_set_error("tome_match: x must be 16-byte aligned, slot / members / starts 4-byte aligned"); return -1; }
  const TomeGeo g = tome_geo(H, W);
  if (!score || !best) {
    if (!ws || ws_bytes < mvd_tome_workspace_bytes(B, H, W) || ((uintptr_t)ws & 255)) { mvd_set_error("tome_match: workspace missing, unaligned or too small (%lld bytes, %lld needed)", (long long)ws_bytes, (long long)mvd_tome_workspace_bytes(B, H, W)); return -1; }
    if (!score) score = (float*)ws;
    if (!best) best = (int*)((char*)ws + align256((size_t)B * g.ns * 4));
  }
  int n2, m2, sort_bytes;
  const size_t lds = tome_select_lds(g, &n2, &m2, &sort_bytes);
  if (lds > 64 * 1024) {              // dynamic LDS above 64 KB has to be asked for, once per DEVICE: the most any map within the limit needs
    static std::mutex mu;
    static bool asked[TM_MAX_DEVICES] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) { (void)hipGetLastError(); mvd_set_error("tome_match: hipGetDevice failed"); return -3; }
    std::lock_guard<std::mutex> lock(mu);
    if (dev >= TM_MAX_DEVICES || !asked[dev]) {       // (a device beyond the table is asked every time)
      const size_t ask = 64 * 1024 + 8192 * 4 + 16 * 4;
      if (lds > ask || hipFuncSetAttribute(reinterpret_cast<const void*>(tome_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ask) != hipSuccess) {
        (void)hipGetLastError(); mvd_set_error("tome_match: the select kernel's %zu bytes of LDS were refused", lds); return -3;
      }
      if (dev < TM_MAX_DEVICES) asked[dev] = true;
    }
  }
  TomeMatchArgs ma; ma.x = x; ma.score = score; ma.best = best; ma.g = g; ma.C = C;
  const int wgs = (g.ns + 32 * TM_MATCH_WAVES - 1) / (32 * TM_MATCH_WAVES);
  hipLaunchKernelGGL(tome_match_kernel, dim3((unsigned)wgs, (unsigned)B), dim3(TM_MATCH_WAVES * 64), 0, stream, ma);
  CHECK(launch_check("tome_match"));
  TomeSelectArgs sa; sa.score = score; sa.best = best; sa.slot = slot; sa.members = members; sa.starts = starts; sa.g = g; sa.r = r;
  sa.n2 = n2; sa.m2 = m2; sa.sort_bytes = sort_bytes;
  hipLaunchKernelGGL(tome_select_kernel, dim3((unsigned)B), dim3(TM_SELECT_THREADS), lds, stream, sa);
  return launch_check("tome_select");
}

int mvd_launch_tome_merge(const bf16_t* x, int B, int H, int W, int C, int r, const int* members, const int* starts, bf16_t* out, hipStream_t stream) {
  CHECK(tome_check("tome_merge", B, H, W, C, r));
  if (!x || !members || !starts || !out) { mvd_set_error("tome_merge: null tensor"); return -1; }
  if (((uintptr_t)x | (uintptr_t)out) & 15) { mvd_set_error("tome_merge: tensors must be 16-byte aligned"); return -1; }
  const int Nm = H * W - r;
  const long total = (long)B * Nm * (C / 8);
  hipLaunchKernelGGL(tome_merge_kernel, dim3((unsigned)blocks_of(total)), dim3(256), 0, stream, x, members, starts, out, total, H * W, C, Nm);
  return launch_check("tome_merge");
}

int mvd_launch_tome_unmerge_add(bf16_t* h, const bf16_t* t, int B, int H, int W, int C, int r, const int* slot, hipStream_t stream) {
  CHECK(tome_check("tome_unmerge_add", B, H, W, C, r));
  if (!h || !t || !slot) { mvd_set_error("tome_unmerge_add: null tensor"); return -1; }
  if (((uintptr_t)h | (uintptr_t)t) & 15) { mvd_set_error("tome_unmerge_add: tensors must be 16-byte aligned"); return -1; }
  const long total = (long)B * H * W * (C / 8);
  hipLaunchKernelGGL(tome_unmerge_add_kernel, dim3((unsigned)blocks_of(total)), dim3(256), 0, stream, h, t, slot, total, H * W, C, H * W - r);
  return launch_check("tome_unmerge_add");
}

extern "C" int64_t mvd_op_tome_workspace_bytes(int B, int H, int W) { return mvd_tome_workspace_bytes(B, H, W); }
extern "C" int mvd_op_tome_match(const void* x, int B, int H, int W, int C, int r, int* slot, int* members, int* starts, float* score, int* best,
                                 void* ws, int64_t ws_bytes, void* stream) {
  return mvd_launch_tome_match((const bf16_t*)x, B, H, W, C, r, slot, members, starts, score, best, ws, ws_bytes, (hipStream_t)stream);
}
extern "C" int mvd_op_tome_merge(const void* x, int B, int H, int W, int C, int r, const int* members, const int* starts, void* out, void* stream) {
  return mvd_launch_tome_merge((const bf16_t*)x, B, H, W, C, r, members, starts, (bf16_t*)out, (hipStream_t)stream);
}
extern "C" int mvd_op_tome_unmerge_add(void* h, const void* t, int B, int H, int W, int C, int r, const int* slot, void* stream) {
  return mvd_launch_tome_unmerge_add((bf16_t*)h, (const bf16_t*)t, B, H, W, C, r, slot, (hipStream_t)stream);
}
// out[8]: nd, ns, N' = H W - r, score sort keys, member sort keys, match workgroups per image, select LDS bytes, the token limit
extern "C" int mvd_debug_tome_plan(int H, int W, int C, int r, int64_t* out) {
  if (!out) { mvd_set_error("tome_plan: null output"); return -1; }
  out[7] = TM_MAX_TOKENS;
  CHECK(tome_check("tome_plan", 1, H, W, C, r));
  const TomeGeo g = tome_geo(H, W);
  int n2, m2, sort_bytes;
  const size_t lds = tome_select_lds(g, &n2, &m2, &sort_bytes);
  out[0] = g.nd; out[1] = g.ns; out[2] = (int64_t)H * W - r; out[3] = n2; out[4] = m2;
  out[5] = (g.ns + 32 * TM_MATCH_WAVES - 1) / (32 * TM_MATCH_WAVES); out[6] = (int64_t)lds;
  return 0;
}
