// Token downsampling of the self-attention keys (ToDo: Smith, Saxena and Saha, IJCAI 2024, restated).
// k and v are the K and V columns of one transformer block's fused q/k/v rows, [B][H*W] rows of C channels each with the shared row
// stride ld (3C or 4C elements) and the batch stride H*W*ld.  With a factor f the key map is Hk x Wk = (H / f) x (W / f):
//   nearest  key (i, j) is the row of token (i f, j f), copied bit for bit
//   area     key (i, j) is the mean over the f x f cell: the f*f bf16 values summed in fp32 in row-major order inside the cell, the
//            sum divided by float(f*f) (correctly rounded), one rounding to bf16 (RNE)
// Tokens of an incomplete last row or column of cells are in no key.  Output: compact [B][Nk][2C] bf16, K in columns [0, C) and V
// in [C, 2C), so the attention launch reads it with ldk = ldv = 2C and bsk = bsv = Nk 2C.
// One launch for K and V: a lane owns eight channels of one output row (16-byte loads and stores), lanes run along the 2C columns
// so a wave reads and writes whole rows.  No LDS, no atomics; a row's bits depend on its f*f input rows alone, not on the batch or
// on the grid.
#include <stdint.h>

#include "host_util.h"

namespace {

MVD_DEVINL void unpack8(const u32x4& v, float* f) {
  f[0] = bflo(v.x); f[1] = bfhi(v.x); f[2] = bflo(v.y); f[3] = bfhi(v.y);
  f[4] = bflo(v.z); f[5] = bfhi(v.z); f[6] = bflo(v.w); f[7] = bfhi(v.w);
}

struct TodoArgs {
  const bf16_t* k; const bf16_t* v; bf16_t* out;
  long total;            // lanes with work: B * Nk * (2C / 8)
  long bs;               // input batch stride, H * W * ld elements
  int ld, W, C, Wk, Nk;
};

template <int F, bool AREA>
__global__ __launch_bounds__(256) void todo_downsample_kernel(const TodoArgs a) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.total) return;
  const int cv = a.C >> 3;                                       // 16-byte chunks per K (or V) row
  const int oc = (int)(t % (2 * cv)); const long row = t / (2 * cv);
  const int b = (int)(row / a.Nk), j = (int)(row % a.Nk);
  const int ci = j / a.Wk, cj = j % a.Wk;
  const bool isv = oc >= cv;
  const bf16_t* src = (isv ? a.v : a.k) + (long)b * a.bs + ((long)(ci * F) * a.W + cj * F) * a.ld + (isv ? oc - cv : oc) * 8;
  u32x4 y = *reinterpret_cast<const u32x4*>(src);                // nearest: the cell's top-left token
  if constexpr (AREA) {
    float acc[8], f[8];
    unpack8(y, acc);
#pragma unroll
    for (int p = 1; p < F * F; ++p) {                            // row-major inside the cell
      unpack8(*reinterpret_cast<const u32x4*>(src + ((long)(p / F) * a.W + p % F) * a.ld), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += f[e];
    }
    const float n = (float)(F * F);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = acc[e] / n;
    y = u32x4{pack2bf(acc[0], acc[1]), pack2bf(acc[2], acc[3]), pack2bf(acc[4], acc[5]), pack2bf(acc[6], acc[7])};
  }
  *reinterpret_cast<u32x4*>(a.out + row * (2L * a.C) + oc * 8) = y;
}

template <int F> void todo_launch(const TodoArgs& a, int method, hipStream_t stream) {
  const dim3 grid((unsigned)blocks_of(a.total));
  if (method) hipLaunchKernelGGL((todo_downsample_kernel<F, true>), grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((todo_downsample_kernel<F, false>), grid, dim3(256), 0, stream, a);
}

}  // namespace

// Every argument is checked before the launch: -1 and a message, nothing written
int mvd_launch_todo_downsample(const bf16_t* k, const bf16_t* v, int ld, int B, int H, int W, int C, int f, int method, bf16_t* out,
                               hipStream_t stream) {
  if (f < 2 || f > 4) { mvd_set_error("todo_downsample: the factor must be 2, 3 or 4, got %d", f); return -1; }
  if (method != 0 && method != 1) { mvd_set_error("todo_downsample: the method is 0 (nearest) or 1 (area), got %d", method); return -1; }
  if (B <= 0 || H <= 0 || W <= 0) { mvd_set_error("todo_downsample: needs batch >= 1 and a map of at least 1 x 1, got batch %d, %d x %d", B, H, W); return -1; }
  if (C <= 0 || (C & 7)) { mvd_set_error("todo_downsample: channels must be a positive multiple of 8, got %d", C); return -1; }
  if ((ld & 7) || ld < C) { mvd_set_error("todo_downsample: the row stride must be a multiple of 8 and at least the %d channels, got %d", C, ld); return -1; }
  if (!k || !v || !out) { mvd_set_error("todo_downsample: null tensor"); return -1; }
  if (((uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) { mvd_set_error("todo_downsample: k, v and out must be 16-byte aligned"); return -1; }
  const int Hk = H / f, Wk = W / f;
  if (Hk < 1 || Wk < 1) { mvd_set_error("todo_downsample: a %d x %d map has no complete %d x %d cell", H, W, f, f); return -1; }
  const long Nk = (long)Hk * Wk;
  const long in_elems = ((long)B * H * W - 1) * ld + C;            // from a base pointer to the end of its last row
  const long out_elems = (long)B * Nk * 2 * C;
  if (Nk > 0x7fffffffL || in_elems > (1L << 40) || out_elems / 8 > 0x7fffffffL * 256) { mvd_set_error("todo_downsample: batch %d of %d x %d is too large", B, H, W); return -1; }
  const uintptr_t i0 = (uintptr_t)(k < v ? k : v), i1 = (uintptr_t)(k < v ? v : k) + (uintptr_t)in_elems * sizeof(bf16_t);
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)out_elems * sizeof(bf16_t);
  if (o0 < i1 && i0 < o1) { mvd_set_error("todo_downsample: out overlaps the input rows"); return -1; }
  TodoArgs a; a.k = k; a.v = v; a.out = out; a.total = out_elems / 8; a.bs = (long)H * W * ld; a.ld = ld; a.W = W; a.C = C; a.Wk = Wk; a.Nk = (int)Nk;
  if (f == 2) todo_launch<2>(a, method, stream);
  else if (f == 3) todo_launch<3>(a, method, stream);
  else todo_launch<4>(a, method, stream);
  return launch_check("todo_downsample");
}

extern "C" int mvd_op_todo_downsample(const void* k, const void* v, int ld, int B, int H, int W, int C, int f, int method, void* out, void* stream) {
  return mvd_launch_todo_downsample((const bf16_t*)k, (const bf16_t*)v, ld, B, H, W, C, f, method, (bf16_t*)out, (hipStream_t)stream);
}
