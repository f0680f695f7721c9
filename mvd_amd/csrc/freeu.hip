// FreeU (Si et al., CVPR 2024; diffusers 0.32.2 apply_freeu / fourier_filter with threshold = 1, restated) on the two inputs of
// an up-block resnet, one launch:
//   hidden' = hidden with channels [0, C / 2) multiplied by b                                   (one bf16 rounding)
//   skip'   = skip with the spatial frequencies {0, -1} x {0, -1} multiplied by s, per (image, channel), in fp32
// With threshold 1 the masked block of the shifted spectrum is those four frequencies for every H, W >= 2, so the
// fftn / fftshift / mask / ifftn chain is a rank-4 projection: with phi_kl(h, w) = 2 pi (k h / H + l w / W), k, l in {0, 1},
//   a_kl = sum x cos phi_kl,  b_kl = sum x sin phi_kl            (seven sums: b_00 = 0)
//   skip'[h, w] = x[h, w] + (s - 1) / (H W) * sum_kl (a_kl cos phi_kl(h, w) + b_kl sin phi_kl(h, w))
// (the real part of the inverse transform: frequency -1 and frequency +1 on BOTH axes give the same real part).
//
// Partition.  Tensors are [image][pixel][channel] bf16.  A lane owns eight channels (one 16-byte load / store).  A workgroup of
// 256 lanes owns 64 channels of one image's skip map: 8 channel octets x 32 pixel lanes, pixel lane q walks pixels q, q + 32, ..
// (a pixel's 64 channels are 128 contiguous bytes).  Each lane keeps 7 x 8 fp32 partial sums; the 8 pixel lanes of a wave are
// combined by a butterfly of lane exchanges, the 4 waves through LDS in wave order -- a fixed order, no atomics: the same bits
// every run.  The map is then read a second time (an L2 hit: one workgroup's slice of the largest map of a 64 x 64 latent is
// 32 KB) and the correction applied in fp32, one rounding to bf16.  The twiddles come from a per-workgroup LDS table of H + W
// (cos, sin) pairs built with the argument in half turns (sincospif), so that quarter turns are exactly 0 / +-1.
// Workgroups behind the skip map's take the backbone scale, eight channels per lane, grid-stride.
#include <math.h>
#include <stdint.h>

#include "host_util.h"

namespace {

constexpr int FU_THREADS = 256;
constexpr int FU_OCTETS = 8;                         // channel octets per workgroup (64 channels)
constexpr int FU_PLANES = FU_THREADS / FU_OCTETS;    // pixel lanes per workgroup (32: 8 per wave)
constexpr int FU_SUMS = 7;                           // a00, a10, b10, a01, b01, a11, b11
constexpr int FU_RED = FU_SUMS * FU_OCTETS * 8;      // floats of one wave's combined sums (448)
constexpr int FU_HIDDEN_WGS_MAX = 2048;

struct FreeuArgs {
  const bf16_t* hidden; const bf16_t* skip; bf16_t* hidden_out; bf16_t* skip_out;
  int B, H, W, C, Cs;
  float b;            // backbone scale of channels [0, C / 2)
  float k;            // (s - 1) / (H W); 0: the skip map is copied bit for bit
  int skip_chunks;    // workgroups per image over the skip channels: ceil(Cs / 64)
  int skip_wgs;       // B * skip_chunks; the workgroups behind them scale the backbone
  long hidden_vecs;   // B * H * W * C / 8
};

MVD_DEVINL void unpack8(const u32x4& v, float* f) {
  f[0] = bflo(v.x); f[1] = bfhi(v.x); f[2] = bflo(v.y); f[3] = bfhi(v.y);
  f[4] = bflo(v.z); f[5] = bfhi(v.z); f[6] = bflo(v.w); f[7] = bfhi(v.w);
}

__global__ __launch_bounds__(FU_THREADS) void freeu_kernel(const FreeuArgs a) {
  extern __shared__ __attribute__((aligned(16))) float fu_lds[];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= a.skip_wgs) {
    // ---- backbone scale: channels below C / 2 times b, the rest copied
    const int cv = a.C >> 3, half = a.C >> 1;
    const long stride = (long)(gridDim.x - a.skip_wgs) * FU_THREADS;
    for (long v = (long)((int)blockIdx.x - a.skip_wgs) * FU_THREADS + tid; v < a.hidden_vecs; v += stride) {
      const int c0 = (int)(v % cv) * 8;
      u32x4 x = *reinterpret_cast<const u32x4*>(a.hidden + v * 8);
      if (c0 < half) {
        float f[8];
        unpack8(x, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) if (c0 + j < half) f[j] *= a.b;
        u32x4 y = {pack2bf(f[0], f[1]), pack2bf(f[2], f[3]), pack2bf(f[4], f[5]), pack2bf(f[6], f[7])};
        if (c0 + 8 > half) {          // (C / 2 inside the octet: the upper elements keep their bits)
          const unsigned keep[4] = {x.x, x.y, x.z, x.w};
          unsigned out[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (c0 + j >= half) out[j >> 1] = (j & 1) ? ((out[j >> 1] & 0x0000ffffu) | (keep[j >> 1] & 0xffff0000u)) : ((out[j >> 1] & 0xffff0000u) | (keep[j >> 1] & 0x0000ffffu));
          y = u32x4{out[0], out[1], out[2], out[3]};
        }
        x = y;
      }
      *reinterpret_cast<u32x4*>(a.hidden_out + v * 8) = x;
    }
    return;
  }
  // ---- skip filter: image `img`, channels [c0, c0 + 8) of this lane, pixels q, q + 32, ..
  const int img = (int)blockIdx.x / a.skip_chunks, chunk = (int)blockIdx.x % a.skip_chunks;
  const int oct = tid & (FU_OCTETS - 1), q = tid >> 3;
  const int c0 = (chunk * FU_OCTETS + oct) * 8;
  const bool live = c0 < a.Cs;
  const int HW = a.H * a.W;
  const bf16_t* src = a.skip + ((long)img * HW) * a.Cs + c0;
  bf16_t* dst = a.skip_out + ((long)img * HW) * a.Cs + c0;
  if (a.k == 0.f) {                                                      // s == 1: every bit as it was (-0 and NaN included)
    if (live) for (int p = q; p < HW; p += FU_PLANES) *reinterpret_cast<u32x4*>(dst + (long)p * a.Cs) = *reinterpret_cast<const u32x4*>(src + (long)p * a.Cs);
    return;
  }
  float* red = fu_lds;                          // [4 waves][7][8 octets][8]
  float* tab = fu_lds + 4 * FU_RED;             // [H + W][2]: (cos, sin) of 2 pi h / H, then of 2 pi w / W
  for (int i = tid; i < a.H + a.W; i += FU_THREADS) {
    const float turns2 = i < a.H ? 2.f * (float)i / (float)a.H : 2.f * (float)(i - a.H) / (float)a.W;    // angle / pi, in [0, 2)
    float sn, cs;
    sincospif(turns2, &sn, &cs);
    tab[2 * i] = cs; tab[2 * i + 1] = sn;
  }
  __syncthreads();
  float acc[FU_SUMS][8];
#pragma unroll
  for (int m = 0; m < FU_SUMS; ++m)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[m][j] = 0.f;
  if (live)
    for (int p = q; p < HW; p += FU_PLANES) {
      const int h = p / a.W, w = p - h * a.W;
      const float ch = tab[2 * h], sh = tab[2 * h + 1], cw = tab[2 * (a.H + w)], sw = tab[2 * (a.H + w) + 1];
      const float c11 = ch * cw - sh * sw, s11 = sh * cw + ch * sw;
      float f[8];
      unpack8(*reinterpret_cast<const u32x4*>(src + (long)p * a.Cs), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        acc[0][j] += f[j];
        acc[1][j] = fmaf(f[j], ch, acc[1][j]); acc[2][j] = fmaf(f[j], sh, acc[2][j]);
        acc[3][j] = fmaf(f[j], cw, acc[3][j]); acc[4][j] = fmaf(f[j], sw, acc[4][j]);
        acc[5][j] = fmaf(f[j], c11, acc[5][j]); acc[6][j] = fmaf(f[j], s11, acc[6][j]);
      }
    }
  // the 8 pixel lanes of a wave (lane bits 3..5): a butterfly, every lane ends with the same sum
#pragma unroll
  for (int m = 0; m < FU_SUMS; ++m)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = acc[m][j];
      v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
      acc[m][j] = v;
    }
  const int wave = tid >> 6;
  if ((tid & 63) < FU_OCTETS) {
#pragma unroll
    for (int m = 0; m < FU_SUMS; ++m) {
      float* r = red + wave * FU_RED + (m * FU_OCTETS + oct) * 8;
      *reinterpret_cast<f32x4*>(r) = f32x4{acc[m][0], acc[m][1], acc[m][2], acc[m][3]};
      *reinterpret_cast<f32x4*>(r + 4) = f32x4{acc[m][4], acc[m][5], acc[m][6], acc[m][7]};
    }
  }
  __syncthreads();
  if (!live) return;
#pragma unroll
  for (int m = 0; m < FU_SUMS; ++m)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int o = (m * FU_OCTETS + oct) * 8 + j;
      acc[m][j] = ((red[o] + red[FU_RED + o]) + red[2 * FU_RED + o]) + red[3 * FU_RED + o];      // waves in order
    }
  for (int p = q; p < HW; p += FU_PLANES) {
    const int h = p / a.W, w = p - h * a.W;
    const float ch = tab[2 * h], sh = tab[2 * h + 1], cw = tab[2 * (a.H + w)], sw = tab[2 * (a.H + w) + 1];
    const float c11 = ch * cw - sh * sw, s11 = sh * cw + ch * sw;
    float f[8];
    unpack8(*reinterpret_cast<const u32x4*>(src + (long)p * a.Cs), f);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float t = acc[0][j];
      t = fmaf(acc[1][j], ch, t); t = fmaf(acc[2][j], sh, t);
      t = fmaf(acc[3][j], cw, t); t = fmaf(acc[4][j], sw, t);
      t = fmaf(acc[5][j], c11, t); t = fmaf(acc[6][j], s11, t);
      f[j] = fmaf(a.k, t, f[j]);
    }
    *reinterpret_cast<u32x4*>(dst + (long)p * a.Cs) = u32x4{pack2bf(f[0], f[1]), pack2bf(f[2], f[3]), pack2bf(f[4], f[5]), pack2bf(f[6], f[7])};
  }
}

bool overlaps(const void* p, size_t np, const void* q, size_t nq) {
  const char* a = (const char*)p; const char* b = (const char*)q;
  return a < b + nq && b < a + np;
}

}  // namespace

// Every check before the launch; -1 and a message for a problem the kernel does not take.
int mvd_launch_freeu(const bf16_t* hidden, int C, const bf16_t* skip, int Cs, int B, int H, int W, float b, float s, bf16_t* hidden_out,
                     bf16_t* skip_out, hipStream_t stream) {
  if (!hidden || !skip || !hidden_out || !skip_out) { mvd_set_error("freeu: null tensor"); return -1; }
  if (B <= 0 || H < 2 || W < 2) { mvd_set_error("freeu: needs batch >= 1 and a map of at least 2 x 2, got batch %d, %d x %d (one row or column has no frequency -1)", B, H, W); return -1; }
  if (C <= 0 || Cs <= 0 || (C & 7) || (Cs & 7)) { mvd_set_error("freeu: channels must be positive multiples of 8 (16-byte vectors), got hidden %d, skip %d", C, Cs); return -1; }
  if (!(b > 0.f) || !(s > 0.f) || !(b < INFINITY) || !(s < INFINITY)) { mvd_set_error("freeu: b and s must be positive and finite, got b = %g, s = %g", (double)b, (double)s); return -1; }
  if (((uintptr_t)hidden | (uintptr_t)skip | (uintptr_t)hidden_out | (uintptr_t)skip_out) & 15) { mvd_set_error("freeu: tensors must be 16-byte aligned"); return -1; }
  const size_t lds = (size_t)(4 * FU_RED + 2 * (H + W)) * sizeof(float);
  if ((long)H * W > (1 << 24) || lds > 64 * 1024) { mvd_set_error("freeu: map %d x %d is too large (the twiddle table of H + W pairs lives in LDS)", H, W); return -1; }
  const size_t nh = (size_t)B * H * W * C * sizeof(bf16_t), ns = (size_t)B * H * W * Cs * sizeof(bf16_t);
  if (overlaps(hidden_out, nh, hidden, nh) || overlaps(hidden_out, nh, skip, ns) || overlaps(skip_out, ns, hidden, nh) ||
      overlaps(skip_out, ns, skip, ns) || overlaps(hidden_out, nh, skip_out, ns)) {
    mvd_set_error("freeu: an output overlaps an input or the other output (the skip map is read twice)"); return -1;
  }
  FreeuArgs a;
  a.hidden = hidden; a.skip = skip; a.hidden_out = hidden_out; a.skip_out = skip_out;
  a.B = B; a.H = H; a.W = W; a.C = C; a.Cs = Cs; a.b = b;
  a.k = (s - 1.f) / (float)((long)H * W);
  a.skip_chunks = (Cs + FU_OCTETS * 8 - 1) / (FU_OCTETS * 8);
  const long skip_wgs = (long)B * a.skip_chunks;
  a.hidden_vecs = (long)B * H * W * (C / 8);
  long hidden_wgs = (a.hidden_vecs + FU_THREADS - 1) / FU_THREADS;
  if (hidden_wgs > FU_HIDDEN_WGS_MAX) hidden_wgs = FU_HIDDEN_WGS_MAX;
  if (skip_wgs + hidden_wgs > 0x7fffffffL) { mvd_set_error("freeu: batch %d x %d channels needs too many workgroups", B, Cs); return -1; }
  a.skip_wgs = (int)skip_wgs;
  hipLaunchKernelGGL(freeu_kernel, dim3((unsigned)(skip_wgs + hidden_wgs)), dim3(FU_THREADS), lds, stream, a);
  return launch_check("freeu");
}

extern "C" int mvd_op_freeu(const void* hidden, int C, const void* skip, int Cs, int B, int H, int W, float b, float s, void* hidden_out,
                            void* skip_out, void* stream) {
  return mvd_launch_freeu((const bf16_t*)hidden, C, (const bf16_t*)skip, Cs, B, H, W, b, s, (bf16_t*)hidden_out, (bf16_t*)skip_out,
                          (hipStream_t)stream);
}
