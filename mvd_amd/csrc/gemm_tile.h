// The lock-step tile kernel of gemm.hip (its head comment describes the design) and the launch of one instantiation, shared by
// the two translation units that instantiate it: gemm.hip (every tile the product ships) and gemm_relu.hip (the ReLU forms
// of tiles 3, 4, 5).  The ReLU forms live in a translation unit of their own so that gemm.hip's code object -- kernels, their
// order, and the distance from each kernel to g_zero16 -- is what it was without them (tools/isa_diff.py).  Everything
// sits in an unnamed namespace: each translation unit has its own g_zero16.
#pragma once
#include <stdlib.h>
#include <string.h>
#include "kernels.h"

namespace {

template <int BM_, int BN_, int WM_, int WN_>
struct Cfg {
  static constexpr int BM = BM_, BN = BN_, WM = WM_, WN = WN_;
  static constexpr int NT = 64 * WM * WN;
  static constexpr int WTM = BM / WM, WTN = BN / WN;
  static constexpr int TM = WTM / 16, TN = WTN / 16;
  static constexpr int A_CHUNKS = BM * 8, B_CHUNKS = BN * 8;
  static constexpr int A_IT = (A_CHUNKS + NT - 1) / NT;
  static constexpr int B_IT = (B_CHUNKS + NT - 1) / NT;
  static constexpr int ROWS_PER_IT = NT / 8;
  static constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128;
  static constexpr int STAGE_BYTES = A_BYTES + B_BYTES;
  static constexpr int LDS_BYTES = 2 * STAGE_BYTES;
  // register budget: keep as many workgroups co-resident per CU as LDS allows (2nd __launch_bounds__ argument
  // = waves per SIMD); without it hipcc spends up to 512 registers per lane and halves the residency
  static constexpr int WG_PER_CU = (160 * 1024 / LDS_BYTES) > 4 ? 4 : (160 * 1024 / LDS_BYTES);
  static constexpr int MIN_WAVES = (WG_PER_CU * NT / 256) < 1 ? 1 : (WG_PER_CU * NT / 256 > 4 ? 4 : WG_PER_CU * NT / 256);
  static_assert(WTM % 16 == 0 && WTN % 16 == 0, "wave tile must be a multiple of the MFMA tile");
  static_assert(A_CHUNKS % NT == 0, "A slab must divide evenly over the threads");
  static constexpr bool RELU = false;
};
// The same tile with max(., 0) in front of the one rounding of the epilogue (MvdGemmArgs::relu).  A type of its own, so the
// ReLU kernels are NEW instantiations beside the plain ones, whose symbols and instruction streams stay what they were.
template <class B>
struct WithRelu : B { static constexpr bool RELU = true; };

MVD_DEVINL int swz_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

// AMODE: 0 = dense A (one segment), 1 = implicit 3x3 conv, 2 = conv followed by a dense (1x1 shortcut) segment.
// The slab cursor (tap / channel offset) lives in scalar registers: it depends on kernel arguments only.
// GLDS: stage slabs with global_load_lds_dwordx4 (LDS-DMA: no VGPR round trip, no ds_write).  The LDS
// image is identical to the register-staged one: the DMA writes lane-linear, so the XOR swizzle is applied
// to the per-lane SOURCE column instead of the LDS address.  Out-of-image conv taps read a 16-byte zero buffer.
__device__ __attribute__((aligned(16))) unsigned int g_zero16[4] = {0u, 0u, 0u, 0u};

MVD_DEVINL void glds16(const void* gsrc, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// The kernel is PERSISTENT: gridDim.x workgroups walk the tile list (XCD-contiguous chunks) and the K-slab
// pipeline runs straight across tile boundaries -- the first slab of the next tile is already in flight while
// the last slab of the current tile is multiplied and its epilogue runs, so short-K GEMMs (K = 320: five slabs)
// do not pay a load-latency prologue per tile.
// DBG: measurement instantiations (probe builds only, -DMVD_PROBE) honour a.dbg; product instantiations carry no such branches.
template <class C, int AMODE, bool GLDS, bool SPLITK, bool DBG>
__global__ __launch_bounds__(C::NT, C::MIN_WAVES) void gemm_kernel(const MvdGemmArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / C::WN, wn = wave % C::WN;
  const int ntn = a.N / C::BN;
  const int ntm = (a.M + C::BM - 1) / C::BM;
  const int lrow = tid >> 3;
  // 16-byte K chunk this thread fetches: register staging swizzles the LDS address, LDS-DMA the source column
  const int kc = GLDS ? ((tid & 7) ^ ((lrow >> 1) & 7)) : (tid & 7);
  const int wave_chunk0 = tid & ~63;   // first chunk id of this wave (LDS-DMA destination is wave-uniform)

  // ---- tile walk: XCD x (= blockIdx & 7) owns tiles [tstart, tstart + tcnt); its workgroups stride through them
  const int S = SPLITK ? a.splitk : 1;            // split-K: each tile is S work items over disjoint slab ranges
  const int ntiles = ntn * ntm * S;               // (work items)
  const int xcd = blockIdx.x & 7, xj = blockIdx.x >> 3;
  const int gx = (gridDim.x >> 3) + ((int)(gridDim.x & 7) > xcd ? 1 : 0);   // workgroups on this XCD
  const int tq = ntiles >> 3, tr = ntiles & 7;
  const int tstart = xcd < tr ? xcd * (tq + 1) : tr * (tq + 1) + (xcd - tr) * tq;
  const int tend = tstart + tq + (xcd < tr ? 1 : 0);
  int tile = tstart + xj;
  if (tile >= tend) return;

  constexpr bool HAS_CONV = AMODE != 0;
  const MvdASeg& cs = a.seg[0];                       // conv segment (AMODE 1, 2)
  const MvdASeg& ds = a.seg[AMODE == 2 ? 1 : 0];      // dense segment (AMODE 0, 2)
  const int conv_c = cs.c0, conv_inW = cs.inW, conv_ups = cs.ups;
  const int limH = conv_ups ? 2 * cs.inH : cs.inH, limW = conv_ups ? 2 * cs.inW : cs.inW;
  const bf16_t* conv_p = cs.p0;
  const bf16_t* dp0 = ds.p0;
  const bf16_t* dp1 = ds.p1;
  const int dc0 = ds.c0, dc1 = ds.c1;
  const int nkt_conv = HAS_CONV ? (9 * conv_c) / 64 : 0;
  const int nkt = a.Ktot / 64;

  // ---- loader state (belongs to the tile whose slabs are being fetched -- may run one tile ahead)
  int a_m[C::A_IT], a_pb[C::A_IT], a_yx[C::A_IT];   // a_yx = (oy*stride) | (ox*stride) << 16
  int ld_n0 = 0;
  auto setup_loader = [&](int work) {
    const int t = S == 1 ? work : work / S;
    const int m0 = (t / ntn) * C::BM;
    ld_n0 = (t % ntn) * C::BN;
#pragma unroll
    for (int i = 0; i < C::A_IT; ++i) {
      int m = m0 + lrow + i * C::ROWS_PER_IT;
      m = m < a.M ? m : a.M - 1;
      a_m[i] = m;
      a_pb[i] = 0; a_yx[i] = 0;
      if (HAS_CONV) {
        const int b = m / a.rows_per_batch;
        const int rem = m - b * a.rows_per_batch;
        const int oy = rem / a.outW, ox = rem - oy * a.outW;
        a_pb[i] = b * cs.inH * cs.inW;
        a_yx[i] = (oy * cs.stride + cs.asym) | ((ox * cs.stride + cs.asym) << 16);   // asym: the window starts AT (2oy, 2ox)
      }
    }
  };

  u32x4 ra[C::A_IT], rb[C::B_IT];
  // fetch slab lk of the loader's tile into stage st (or into registers); the slab position (tap, channel
  // offset) is derived from lk alone so that it stays in scalar registers
  auto load_slab = [&](int st, int lk) {
    unsigned char* sa = smem + st * C::STAGE_BYTES;
    unsigned char* sb = sa + C::A_BYTES;
    if (HAS_CONV && (AMODE == 1 || lk < nkt_conv)) {
      // conv K order is [channel slice][tap][64 channels]: the nine taps of one 64-channel slice are consecutive
      // slabs, so a workgroup re-reads the same ~50 KB of the feature map nine times from L2 instead of cycling
      // through the whole 3-row x C window (~250 KB per workgroup, > L2 per XCD with 64 resident workgroups)
      const int ld_cs = lk / 9;
      const int ld_tap = lk - ld_cs * 9;
      const int ld_cc = ld_cs << 6;
      const int dy = ld_tap / 3, dx = ld_tap - dy * 3;
      const int col = ld_cc + kc * 8;
#pragma unroll
      for (int i = 0; i < C::A_IT; ++i) {
        const int iy = (a_yx[i] & 0xffff) - 1 + dy, ix = (a_yx[i] >> 16) - 1 + dx;
        const bool ok = (unsigned)iy < (unsigned)limH && (unsigned)ix < (unsigned)limW;
        const int sy = conv_ups ? (iy >> 1) : iy, sx = conv_ups ? (ix >> 1) : ix;
        const bf16_t* p = conv_p + (size_t)(a_pb[i] + sy * conv_inW + sx) * conv_c + col;
        if (GLDS) {
          glds16(ok ? (const void*)p : (const void*)g_zero16, sa + (wave_chunk0 + i * C::NT) * 16);
        } else {
          u32x4 v = {0u, 0u, 0u, 0u};
          if (ok) v = *reinterpret_cast<const u32x4*>(p);
          ra[i] = v;
        }
      }
    } else {
      const int ld_cc = (lk - nkt_conv) << 6;
      const bool first = ld_cc < dc0;
      const bf16_t* base = first ? dp0 : dp1;
      const int ld = first ? dc0 : dc1;
      const int col = (first ? ld_cc : ld_cc - dc0) + kc * 8;
#pragma unroll
      for (int i = 0; i < C::A_IT; ++i) {
        const bf16_t* p = base + (size_t)a_m[i] * ld + col;
        if (DBG && GLDS && (a.dbg & 4)) continue;   // measurement aid: no A traffic
        if (GLDS) glds16(p, sa + (wave_chunk0 + i * C::NT) * 16);
        else ra[i] = *reinterpret_cast<const u32x4*>(p);
      }
    }
#pragma unroll
    for (int i = 0; i < C::B_IT; ++i) {
      const int row = lrow + i * C::ROWS_PER_IT;
      if (C::B_CHUNKS % C::NT == 0 || row < C::BN) {
        const bf16_t* p = a.W + (size_t)(ld_n0 + row) * a.ldw + lk * 64 + kc * 8;
        if (DBG && GLDS && (a.dbg & 8)) continue;   // measurement aid: no W traffic
        if (GLDS) glds16(p, sb + (wave_chunk0 + i * C::NT) * 16);
        else rb[i] = *reinterpret_cast<const u32x4*>(p);
      }
    }
  };
  auto commit_slab = [&](int st) {   // make the fetched slab visible in LDS stage st (before the barrier)
    if (GLDS) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); return; }
    unsigned char* sa = smem + st * C::STAGE_BYTES;
    unsigned char* sb = sa + C::A_BYTES;
    const int kcr = tid & 7;
#pragma unroll
    for (int i = 0; i < C::A_IT; ++i)
      *reinterpret_cast<u32x4*>(sa + swz_off(lrow + i * C::ROWS_PER_IT, kcr)) = ra[i];
#pragma unroll
    for (int i = 0; i < C::B_IT; ++i) {
      const int row = lrow + i * C::ROWS_PER_IT;
      if (C::B_CHUNKS % C::NT == 0 || row < C::BN) *reinterpret_cast<u32x4*>(sb + swz_off(row, kcr)) = rb[i];
    }
  };

  f32x4 acc[C::TM][C::TN];
  const int fr = lane & 15, fq = lane >> 4;
  const float alpha = a.alpha;

  // The accumulators of a tile START at bias + per-batch row vector (out = alpha*(A.W^T + bias + rowvec) + res),
  // so the epilogue needs no operand registers for them.  lane holds out[m][n..n+3]: m = tile row (lane&15),
  // n = 4*(lane>>4) + reg.
  auto init_acc = [&](int m0, int n0) {
    asm volatile("" : "+s"(m0), "+s"(n0));   // keep the address arithmetic here (not hoisted into live registers)
    const int nb = n0 + wn * C::WTN + fq * 4;
#pragma unroll
    for (int i = 0; i < C::TM; ++i) {
#pragma unroll
      for (int j = 0; j < C::TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (SPLITK) return;
    if (a.bias) {
#pragma unroll
      for (int j = 0; j < C::TN; ++j) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bias + nb + j * 16);
#pragma unroll
        for (int i = 0; i < C::TM; ++i) acc[i][j] = bv;
      }
    }
    if (C::TN <= 5 && a.rowvec && a.rows_per_batch % C::BM == 0) {
      // the whole tile lies in one batch element (every level but the 8x8 one): one vector for all rows, one load batch
      const float* rv = a.rowvec + (size_t)(m0 / a.rows_per_batch) * a.ld_rowvec + nb;
#pragma unroll
      for (int j = 0; j < C::TN; ++j) {
        const f32x4 r = *reinterpret_cast<const f32x4*>(rv + j * 16);
#pragma unroll
        for (int i = 0; i < C::TM; ++i) acc[i][j] += r;
      }
    } else if (C::TN <= 5 && a.rowvec) {   // (GEGLU-only configs never carry a row vector)
#pragma unroll
      for (int i = 0; i < C::TM; ++i) {
        int m = m0 + wm * C::WTM + i * 16 + fr;
        m = m < a.M ? m : a.M - 1;
        const float* rv = a.rowvec + (size_t)(m / a.rows_per_batch) * a.ld_rowvec + nb;
#pragma unroll
        for (int j = 0; j < C::TN; ++j) acc[i][j] += *reinterpret_cast<const f32x4*>(rv + j * 16);
      }
    }
  };

  // Residual loads are issued as one batch per row tile: while an LDS-DMA is in flight hipcc waits vmcnt(0) for
  // every ordinary load, so load-use-load-use would serialise the epilogue into dozens of memory round trips.
  auto epilogue = [&](int m0, int n0, int ks) {
    asm volatile("" : "+s"(m0), "+s"(n0));   // keep the address arithmetic here (not hoisted into live registers)
    const int nb = n0 + wn * C::WTN + fq * 4;
    if (SPLITK) {   // raw fp32 partial tile; bias / residual / activation are applied by the reduce kernel
      float* pp = a.part + (size_t)ks * a.M * a.N;
#pragma unroll
      for (int i = 0; i < C::TM; ++i) {
        const int m = m0 + wm * C::WTM + i * 16 + fr;
#pragma unroll
        for (int j = 0; j < C::TN; ++j)
          if (m < a.M) *reinterpret_cast<f32x4*>(pp + (size_t)m * a.N + nb + j * 16) = acc[i][j];
      }
      return;
    }
    // Residual rows are fetched for RG row tiles at a time: hipcc waits vmcnt(0) for them (an LDS-DMA is in flight),
    // which also drains the stores issued so far, so every load batch costs a full memory round trip -- 2 (dense) or
    // 4 (conv: fewer spare registers) per tile instead of one per row tile.
    constexpr int RG = (C::TM % 4 == 0 && AMODE == 0) ? 4 : (C::TM % 2 == 0 ? 2 : 1);
#pragma unroll
    for (int i0 = 0; i0 < C::TM; i0 += RG) {
      u32x2 res_r[RG][C::TN > 5 ? 1 : C::TN];
      if (!(C::TN > 5 || a.geglu) && a.res) {
#pragma unroll
        for (int g = 0; g < RG; ++g) {
          int mr = m0 + wm * C::WTM + (i0 + g) * 16 + fr;
          mr = mr < a.M ? mr : a.M - 1;
          const bf16_t* rp = a.res + (size_t)mr * a.ldres + nb;
#pragma unroll
          for (int j = 0; j < (C::TN > 5 ? 1 : C::TN); ++j) res_r[g][j] = *reinterpret_cast<const u32x2*>(rp + j * 16);
        }
      }
#pragma unroll
      for (int g = 0; g < RG; ++g) {
      const int i = i0 + g;
      const int m = m0 + wm * C::WTM + i * 16 + fr;
      const bool live = m < a.M;
      if (!(C::TN > 5 || a.geglu)) {       // configs with TN > 5 exist for GEGLU only
#pragma unroll
        for (int j = 0; j < (C::TN > 5 ? 1 : C::TN); ++j) {
          const int n = nb + j * 16;
          f32x4 v = acc[i][j] * alpha;
          if (a.res) {
            v[0] += bflo(res_r[g][j][0]); v[1] += bfhi(res_r[g][j][0]); v[2] += bflo(res_r[g][j][1]); v[3] += bfhi(res_r[g][j][1]);
          }
          if constexpr (C::RELU) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
          if (!live || (DBG && (a.dbg & 1))) continue;
          if (a.out_f32) {
            *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.out) + (size_t)m * a.ldo + n) = v;
          } else {
            u32x2 o = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
            *reinterpret_cast<u32x2*>(reinterpret_cast<bf16_t*>(a.out) + (size_t)m * a.ldo + n) = o;
          }
        }
      } else {
        if constexpr (C::TN % 2 == 0) {
#pragma unroll
          for (int j = 0; j < C::TN; j += 2) {
            const f32x4 v = acc[i][j], g = acc[i][j + 1];    // packed rows: 16 value | 16 gate (bias already in)
            if (!live || (DBG && (a.dbg & 1))) continue;
            const int no = (n0 + wn * C::WTN) / 2 + (j / 2) * 16 + fq * 4;
            u32x2 o = {pack2bf(v[0] * gelu_erf_f(g[0]), v[1] * gelu_erf_f(g[1])),
                       pack2bf(v[2] * gelu_erf_f(g[2]), v[3] * gelu_erf_f(g[3]))};
            *reinterpret_cast<u32x2*>(reinterpret_cast<bf16_t*>(a.out) + (size_t)m * a.ldo + no) = o;
          }
        }
      }
      }
    }
  };

  // slab range of a work item (all of K unless split-K); kept out of the slab loop: the integer divisions by
  // the runtime split factor are ~40 instructions each
  auto slab_range = [&](int work, int& k0, int& k1) {
    if (S == 1) { k0 = 0; k1 = nkt; return; }
    const int ks = work % S;
    k0 = (ks * nkt) / S;
    k1 = ((ks + 1) * nkt) / S;
  };
  int kt0, kt1;
  slab_range(tile, kt0, kt1);
  setup_loader(tile);
  load_slab(0, kt0);
  {
    const int tl0 = S == 1 ? tile : tile / S;
    init_acc((tl0 / ntn) * C::BM, (tl0 % ntn) * C::BN);
  }
  commit_slab(0);
  __syncthreads();
  int cur = 0;
  for (;;) {
    const int tl = S == 1 ? tile : tile / S;
    const int ks = S == 1 ? 0 : tile - tl * S;
    const int m0 = (tl / ntn) * C::BM, n0 = (tl % ntn) * C::BN;
    const int next_tile = tile + gx;
    const bool have_next = next_tile < tend;
    int nkt0 = 0, nkt1 = 0;
    if (have_next) slab_range(next_tile, nkt0, nkt1);
    for (int kt = kt0; kt < kt1; ++kt) {
      const bool last_k = kt + 1 == kt1;
      const bool more = !last_k || have_next;
      if (more) {
        if (last_k) setup_loader(next_tile);   // the loader runs ahead into the next work item
        load_slab(cur ^ 1, last_k ? nkt0 : kt + 1);
      }
      const unsigned char* sa = smem + cur * C::STAGE_BYTES;
      const unsigned char* sb = sa + C::A_BYTES;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        if constexpr (C::TM > 4) {
          // tall wave tile (128 rows): 160 accumulator registers, so the A fragments are streamed two at a time
          // (sched_barrier keeps hipcc from hoisting all eight reads and spilling)
          bf16x8 wf[C::TN];
#pragma unroll
          for (int j = 0; j < C::TN; ++j)
            wf[j] = *reinterpret_cast<const bf16x8*>(sb + swz_off(wn * C::WTN + j * 16 + fr, s2 * 4 + fq));
#ifdef MVD_GEMM_NO_SWP
#pragma unroll
          for (int i = 0; i < C::TM; i += 2) {
            const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(sa + swz_off(wm * C::WTM + i * 16 + fr, s2 * 4 + fq));
            const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(sa + swz_off(wm * C::WTM + (i + 1) * 16 + fr, s2 * 4 + fq));
#pragma unroll
            for (int j = 0; j < C::TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], a0, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < C::TN; ++j) acc[i + 1][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], a1, acc[i + 1][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
          }
#else
          // software pipeline over BOTH 32-wide halves of the slab (8 steps of two row tiles): the next pair of A
          // fragments is read while the MFMAs of the current pair run, and during the last pair of the first half each
          // W fragment is replaced in place by its second-half successor as soon as its last MFMA has issued -- the
          // second half starts without waiting for LDS
          if (s2 == 1) continue;
          auto a_at = [&](int q) __attribute__((always_inline)) -> bf16x8 {   // q = half * TM + row tile
            return *reinterpret_cast<const bf16x8*>(sa + swz_off(wm * C::WTM + (q % C::TM) * 16 + fr, (q / C::TM) * 4 + fq));
          };
          bf16x8 a0 = a_at(0), a1 = a_at(1);
#pragma unroll
          for (int q = 0; q < 2 * C::TM; q += 2) {
            const int i = q % C::TM;
            bf16x8 n0 = a0, n1 = a1;
            if (q + 2 < 2 * C::TM) { n0 = a_at(q + 2); n1 = a_at(q + 3); }
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int j = 0; j < C::TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], a0, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < C::TN; ++j) {
              acc[i + 1][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], a1, acc[i + 1][j], 0, 0, 0);
              if (q == C::TM - 2)   // last pair of the first half
                wf[j] = *reinterpret_cast<const bf16x8*>(sb + swz_off(wn * C::WTN + j * 16 + fr, 4 + fq));
            }
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            a0 = n0; a1 = n1;
          }
#endif
          continue;
        } else if constexpr (C::TN > 5) {
          // wide wave tile (160 columns, used for GEGLU where value/gate tiles must pair up): the W fragments are
          // streamed in pairs through ONE software pipeline over both 32-wide halves of the slab (the next pair is read
          // while the 2 x TM MFMAs of the current pair run; the A fragments of the second half replace those of the
          // first in place during its last pair)
          if (s2 == 1) continue;
          constexpr int NP = C::TN / 2;                        // W pairs per half
          auto w_at = [&](int q, int which) __attribute__((always_inline)) -> bf16x8 {   // q = half * NP + pair
            return *reinterpret_cast<const bf16x8*>(sb + swz_off(wn * C::WTN + (2 * (q % NP) + which) * 16 + fr, (q / NP) * 4 + fq));
          };
          bf16x8 af[C::TM];
#pragma unroll
          for (int i = 0; i < C::TM; ++i)
            af[i] = *reinterpret_cast<const bf16x8*>(sa + swz_off(wm * C::WTM + i * 16 + fr, fq));
          bf16x8 w0 = w_at(0, 0), w1 = w_at(0, 1);
#pragma unroll
          for (int q = 0; q < 2 * NP; ++q) {
            const int j = 2 * (q % NP);
            bf16x8 n0 = w0, n1 = w1;
            if (q + 1 < 2 * NP) { n0 = w_at(q + 1, 0); n1 = w_at(q + 1, 1); }
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int i = 0; i < C::TM; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, af[i], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < C::TM; ++i) {
              acc[i][j + 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, af[i], acc[i][j + 1], 0, 0, 0);
              if (q == NP - 1)   // last pair of the first half: this A fragment is done, fetch its second-half successor
                af[i] = *reinterpret_cast<const bf16x8*>(sa + swz_off(wm * C::WTM + i * 16 + fr, 4 + fq));
            }
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            w0 = n0; w1 = n1;
          }
          continue;
        }
        bf16x8 af[C::TM], wf[C::TN];
#pragma unroll
        for (int i = 0; i < C::TM; ++i)
          af[i] = *reinterpret_cast<const bf16x8*>(sa + swz_off(wm * C::WTM + i * 16 + fr, s2 * 4 + fq));
#pragma unroll
        for (int j = 0; j < C::TN; ++j)
          wf[j] = *reinterpret_cast<const bf16x8*>(sb + swz_off(wn * C::WTN + j * 16 + fr, s2 * 4 + fq));
        if (!(DBG && (a.dbg & 2))) {
#pragma unroll
          for (int i = 0; i < C::TM; ++i)
#pragma unroll
            for (int j = 0; j < C::TN; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
        } else {
#pragma unroll
          for (int i = 0; i < C::TM; ++i) asm volatile("" :: "v"(af[i]));
#pragma unroll
          for (int j = 0; j < C::TN; ++j) asm volatile("" :: "v"(wf[j]));
        }
      }
      if (last_k) {                            // next work item's first slab is in flight meanwhile
        epilogue(m0, n0, ks);
        if (have_next) {
          const int tn = S == 1 ? next_tile : next_tile / S;
          init_acc((tn / ntn) * C::BM, (tn % ntn) * C::BN);
        }
      }
      if (more) commit_slab(cur ^ 1);
      __syncthreads();
      cur ^= 1;
    }
    if (!have_next) break;
    tile = next_tile; kt0 = nkt0; kt1 = nkt1;
  }
}

template <class C, int AMODE, bool GLDS, bool SPLITK, bool DBG>
int launch_mode3(const MvdGemmArgs& a, hipStream_t s) {
  static int per_cu = 0;   // resident workgroups per CU for this instantiation (LDS- and VGPR-limited)
  if (!per_cu) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_kernel<C, AMODE, GLDS, SPLITK, DBG>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES);
    if (e != hipSuccess) { mvd_set_error("gemm: hipFuncSetAttribute: %s", hipGetErrorString(e)); return -2; }
    int nb = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, gemm_kernel<C, AMODE, GLDS, SPLITK, DBG>, C::NT, C::LDS_BYTES);
    if (e != hipSuccess || nb < 1) nb = 1;
    per_cu = nb > 4 ? 4 : nb;
  }
  const int ntm = (a.M + C::BM - 1) / C::BM, ntn = a.N / C::BN;
  // persistent grid: as many workgroups as fit on the chip at once (LDS-limited), a multiple of the 8 XCDs
  int grid = 256 * per_cu;
  const int ntiles = ntm * ntn * (a.splitk > 1 ? a.splitk : 1);
  if (ntiles < grid) grid = ((ntiles + 7) / 8) * 8;
  g_mvd_last_gemm.tiles = ntiles; g_mvd_last_gemm.grid = grid; g_mvd_last_gemm.per_cu = per_cu;
  hipLaunchKernelGGL((gemm_kernel<C, AMODE, GLDS, SPLITK, DBG>), dim3(grid), dim3(C::NT), C::LDS_BYTES, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { mvd_set_error("gemm launch: %s", hipGetErrorString(e)); return -3; }
  return 0;
}

template <class C, int AMODE, bool GLDS, bool SPLITK>
int launch_mode2(const MvdGemmArgs& a, hipStream_t s) {
#ifdef MVD_PROBE
  if (a.dbg) return launch_mode3<C, AMODE, GLDS, SPLITK, true>(a, s);
#endif
  return launch_mode3<C, AMODE, GLDS, SPLITK, false>(a, s);
}

}  // namespace
