// ReLU forms of the lock-step GEMM / implicit 3x3 convolution (MvdGemmArgs::relu; the VGG tower of vgg.hip):
//
//   out[M][N] = max( alpha * ( A . W^T + bias + rowvec ) + res, 0 ), rounded once
//
// New instantiations of gemm_tile.h's kernel for the tiles an N = 64 / 128 / 256 / 512 problem selects -- 3 (128x128), 4 (128x64),
// 5 (64x64) -- over a dense A or one conv segment, with register or LDS-DMA staging, and the reduce pass of a split-K launch
// (whose GEMM writes raw partials, so it takes the plain kernel of gemm.hip).  A translation unit of its own: see gemm_tile.h.
#include "gemm_tile.h"

namespace {

// splitk_reduce_kernel of gemm.hip with the ReLU in front of the one rounding (that kernel is left as it is: a shared body
// changed its instruction stream)
__global__ __launch_bounds__(256) void splitk_reduce_relu_kernel(const MvdGemmArgs a) {
  const long nvec = (long)a.M * (a.N >> 2);
  const int nv = a.N >> 2;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < nvec; e += (long)gridDim.x * blockDim.x) {
    const int m = (int)(e / nv), n = (int)(e - (long)m * nv) * 4;
    f32x4 v = *reinterpret_cast<const f32x4*>(a.part + (size_t)m * a.N + n);
    for (int s = 1; s < a.splitk; ++s) v += *reinterpret_cast<const f32x4*>(a.part + ((size_t)s * a.M + m) * a.N + n);
    if (a.bias) v += *reinterpret_cast<const f32x4*>(a.bias + n);
    if (a.rowvec) v += *reinterpret_cast<const f32x4*>(a.rowvec + (size_t)(m / a.rows_per_batch) * a.ld_rowvec + n);
    v *= a.alpha;
    if (a.res) {
      const u32x2 r = *reinterpret_cast<const u32x2*>(a.res + (size_t)m * a.ldres + n);
      v[0] += bflo(r[0]); v[1] += bfhi(r[0]); v[2] += bflo(r[1]); v[3] += bfhi(r[1]);
    }
    v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f);
    if (a.out_f32) {
      *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.out) + (size_t)m * a.ldo + n) = v;
    } else {
      u32x2 o = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
      *reinterpret_cast<u32x2*>(reinterpret_cast<bf16_t*>(a.out) + (size_t)m * a.ldo + n) = o;
    }
  }
}

template <class C>
int launch_cfg_relu(const MvdGemmArgs& a, hipStream_t s, bool glds) {
  using R = WithRelu<C>;
  const bool dense = a.seg[0].mode == MVD_A_DENSE;
  if (glds) return dense ? launch_mode2<R, 0, true, false>(a, s) : launch_mode2<R, 1, true, false>(a, s);
  return dense ? launch_mode2<R, 0, false, false>(a, s) : launch_mode2<R, 1, false, false>(a, s);
}

}  // namespace

// arguments validated by mvd_launch_gemm; unsplit (a split-K launch goes to the plain kernels and the reduce pass below)
int mvd_launch_gemm_relu(const MvdGemmArgs& a, hipStream_t s, int cfg, bool glds) {
  if (a.splitk > 1 || !a.relu) { mvd_set_error("gemm_relu: internal: unsplit ReLU launches only"); return -1; }
  switch (cfg) {
    case 3: return launch_cfg_relu<Cfg<128, 128, 2, 2>>(a, s, glds);
    case 4: return launch_cfg_relu<Cfg<128, 64, 2, 2>>(a, s, glds);
    case 5: return launch_cfg_relu<Cfg<64, 64, 2, 2>>(a, s, glds);
    default: mvd_set_error("gemm: the ReLU epilogue exists for tile configs 3, 4, 5 (128x128, 128x64, 64x64), not %d", cfg); return -1;
  }
}

int mvd_launch_splitk_reduce_relu(const MvdGemmArgs& a, hipStream_t s, int grid) {
  hipLaunchKernelGGL(splitk_reduce_relu_kernel, dim3(grid), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { mvd_set_error("splitk_reduce launch: %s", hipGetErrorString(e)); return -3; }
  return 0;
}
