// bf16 MFMA GEMM / implicit-GEMM 3x3 convolution for gfx950 (MI355X).
//
//   out[M][N] = alpha * ( A[M][K] . W[N][K]^T + bias[N] + rowvec[batch(m)][N] ) + res[M][N]
//
// * A is either a dense token-major matrix (optionally the channel concat of two
//   sources) or the *virtual* im2col matrix of an NHWC feature map (3x3, pad 1, stride
//   1/2, optional fused nearest-2x upsample).  Up to two K segments are accumulated into
//   the same tile, which fuses a ResnetBlock2D's conv2 with its 1x1 conv_shortcut and an
//   attention out-projection with the adapter's to_out_ref.
// * W is [N][K] with K contiguous (the nn.Linear layout; conv weights are packed
//   [Cout][ky][kx][Cin] by the host).
// * v_mfma_f32_16x16x32_bf16 with the roles swapped (W rows feed the MFMA "A" operand) so
//   each lane ends up with 4 consecutive output channels of one row -> 8-byte stores.
// * Tiles are staged through LDS in 64-wide K slabs, XOR-swizzled at 16-byte granularity
//   ((row>>1)&7) so both the staging ds_write_b128 and the fragment ds_read_b128 are
//   bank-conflict free; double-buffered, global loads for slab t+1 are issued before the
//   MFMAs of slab t and written to LDS after them (one barrier per slab).
// * blockIdx -> tile mapping is XCD-aware: consecutive tiles (same A rows, different N
//   tile) land on the same XCD so the A slab is fetched from HBM once per XCD L2.
#include <stdlib.h>
#include <string.h>
#include "kernels.h"
#include "gemm_tile.h"

thread_local MvdLaunchPlan g_mvd_last_gemm = {-1, 1, 0, 0, 0, 0};

namespace {

// ---------------------------------------------------------------- split-K reduction + epilogue
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const MvdGemmArgs a) {
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
    if (a.out_f32) {
      *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.out) + (size_t)m * a.ldo + n) = v;
    } else {
      u32x2 o = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
      *reinterpret_cast<u32x2*>(reinterpret_cast<bf16_t*>(a.out) + (size_t)m * a.ldo + n) = o;
    }
  }
}

struct CfgInfo { int bm, bn, tn_even; };

template <class C, int AMODE, bool GLDS>
int launch_mode(const MvdGemmArgs& a, hipStream_t s) {
  if constexpr (GLDS) { if (a.splitk > 1) return launch_mode2<C, AMODE, true, true>(a, s); }
  return launch_mode2<C, AMODE, GLDS, false>(a, s);
}

// DMA_ONLY: the tile exists with LDS-DMA staging only (the 256x320 tile: its register-staged form spills 37-43 VGPRs to scratch
// memory and was never reachable in the product -- tools/lint_device_isa.py fails the build on any shipped kernel with scratch)
template <class C, bool DMA_ONLY = false>
int launch_cfg(const MvdGemmArgs& a, hipStream_t s, bool glds) {
  if (a.splitk > 1) glds = true;   // split-K exists for the LDS-DMA variants only
  if (glds || DMA_ONLY) {
    if (a.seg[0].mode == MVD_A_DENSE) return launch_mode<C, 0, true>(a, s);
    return a.nseg == 1 ? launch_mode<C, 1, true>(a, s) : launch_mode<C, 2, true>(a, s);
  }
  if constexpr (!DMA_ONLY) {
    if (a.seg[0].mode == MVD_A_DENSE) return launch_mode<C, 0, false>(a, s);
    return a.nseg == 1 ? launch_mode<C, 1, false>(a, s) : launch_mode<C, 2, false>(a, s);
  }
  return -1;
}

using C0 = Cfg<256, 160, 4, 2>;
using C1 = Cfg<256, 128, 4, 2>;
using C2 = Cfg<128, 160, 2, 2>;
using C3 = Cfg<128, 128, 2, 2>;
using C4 = Cfg<128, 64, 2, 2>;
using C5 = Cfg<64, 64, 2, 2>;
using C7 = Cfg<256, 320, 2, 4>;   // wave tile 128x80: 49 FLOP per LDS-read byte instead of 36
using C6 = Cfg<256, 320, 4, 2>;   // wave tile 64x160 (even number of 16-column tiles: GEGLU value/gate pairs)
// (a three-stage 256x160 experiment gave no gain: the kernel is LDS-read bound, not load-latency bound)
using C8 = Cfg<128, 320, 2, 4>;   // wave tile 64x80: twice the tiles of C7 for M = 8192 (deep levels) -> no split-K
const CfgInfo kCfgs[] = {{256, 160, 0}, {256, 128, 1}, {128, 160, 0}, {128, 128, 1}, {128, 64, 1}, {64, 64, 1}, {256, 320, 1}, {256, 320, 0},
                         {128, 320, 0}};
constexpr int kNumCfgs = 9;

}  // namespace

extern "C" int mvd_gemm_num_configs(void) { return kNumCfgs; }

// out[5] = {tile config, split-K factor, work items (tiles x split), workgroups launched, workgroups per CU} of the
// calling thread's last GEMM / conv launch
extern "C" int mvd_debug_last_gemm_plan(int* out) {
  if (!out) { mvd_set_error("last_gemm_plan: null argument"); return -1; }
  out[0] = g_mvd_last_gemm.cfg; out[1] = g_mvd_last_gemm.splitk; out[2] = g_mvd_last_gemm.tiles;
  out[3] = g_mvd_last_gemm.grid; out[4] = g_mvd_last_gemm.per_cu;
  return 0;
}

// launches of the 2x2 sub-pixel upsampling convolution (gemm_pp.hip, AMODE 4) by this process so far: tests and A/B runs read
// the difference across a forward to see which route the upsamplers took
std::atomic<long> g_mvd_up4_launches{0};
extern "C" long mvd_debug_up4_launches(void) { return g_mvd_up4_launches.load(); }

// 1 when the calling thread's last small-M split-K launch took the no-wait combine (asked for by the caller, or because its
// grid exceeded what the chip holds at once: gemm_sm.hip launch_sm3), else 0
extern "C" int mvd_debug_last_gemm_nowait(void) { return g_mvd_last_gemm.nowait; }

// Tile choice (tools/tune_gemm.py sweep on MI355X, profiles/r01_tune_gemm_B32_v2.log): the 256x320 tile wins wherever
// its grid (times a split-K of at most 2) can occupy the 256 CUs; below that, fall through 128x160 -> 128x128 ->
// 128x64 -> 64x64 until the grid has >= ~300 workgroups, else take the config with the most workgroups.
// split factor of the rule above (1: the rule does not apply)
static int deep_conv_split(const MvdGemmArgs& a, long t7) {
  static const int on = MVD_ENV_INT("MVD_GEMM_DEEP_CONV_SPLIT", 1);
  // (a.splitk: 0 = undecided, the engine asks mvd_gemm_pick_splitk first; a caller that fixed a shallow split -- the operator entry
  //  points with their default splitk = 1 -- keeps the tile that suits it: 32 unsplit 256x320 tiles would leave 224 CUs idle)
  if (!on || (mvd_debug_flags() & MVD_DBG_NO_DEEP_CONV_SPLIT) || a.seg[0].mode == MVD_A_DENSE || a.geglu || a.out_f32 || t7 < 24 || t7 > 64 || a.Ktot < 8192 || (a.splitk > 0 && a.splitk < 4)) return 1;
  int s = (int)(256 / t7);
  while (s > 1 && a.Ktot / 64 / s < 16) --s;
  return s > 16 ? 16 : s;
}

int mvd_gemm_pick_config(const MvdGemmArgs& a) {
  // 256x320 tile with 128x80 wave tiles (49 FLOP per LDS-read byte): the kernel is LDS-bandwidth bound, so this
  // is the fastest shape whenever its tile grid -- times a split-K of up to 8 -- can occupy the 256 CUs
  static const int use7 = MVD_ENV_INT("MVD_GEMM_BIG", 1);
  // (128x320 tiles instead of a two-way split-K at M = 8192: measured 1 % SLOWER end to end -- the W slab is
  //  re-fetched per 128 rows and the 64x80 wave tile reads more LDS per FLOP -- so it is an opt-in switch)
  static const int split_min_slabs = MVD_ENV_INT("MVD_GEMM_SPLIT_MINK", 4096) / 64;
  static const int use8 = MVD_ENV_INT("MVD_GEMM_C8", 0);
  if (use7 && !a.relu && a.N % 320 == 0 && a.M >= 1024) {
    const long t7 = (long)((a.M + 255) / 256) * (a.N / 320);
    if (a.geglu) { if (t7 >= 200) return 6; }
    // (a split of 2 at most: the fp32 partials of deeper splits cost more than the bigger tile gains)
    else if (t7 >= 200) return 7;
    else if (use8 && t7 * 2 >= 200) return 8;       // 128x320 tiles fill the chip without a split
    // too few 256x320 tiles (M = 8192 at the deep levels): a two-way split-K of the big tile only pays for long K
    // (K >= 4096: convolutions, ff2); shorter K goes to 128x160 tiles without a split -- and without the reduce pass
    // (measured at M 8192 x N 1280: K 1280 36 us vs 41 + 15 us, K 2560 67 vs 63 + 15 us, K 5120 a tie; end to end the
    //  rule is worth 0.2-0.5 %)
    else if (a.Ktot / 64 >= split_min_slabs && t7 * 2 >= 200) return 7;
    // the 3x3 convolutions of the 8x8 level at 32 images (M = 2048: 32 tiles, K = 11520 ... 23040): the big tile cut EIGHT ways
    // along K (256 workgroups, each slice >= 22 slabs) beats 512 work items of the 128x160 tile at split 4 by 7 / 16 / 3 %
    // (tools/tune_worst_shapes.py, profiles/r04_tune_worst_shapes.log) -- half the operand bytes per FLOP, same partial traffic
    else if (deep_conv_split(a, t7) > 1) return 7;
  }
  static const int order[] = {2, 3, 4, 5};
  int cfg = -1, first_valid = -1;
  long best_blocks = -1;
  for (int c : order) {
    if (a.N % kCfgs[c].bn) continue;
    if (a.geglu && !kCfgs[c].tn_even) continue;
    if (a.relu && c == 2) continue;      // (the ReLU epilogue exists for the N % 64 tiles 3, 4, 5)
    const long blocks = (long)((a.M + kCfgs[c].bm - 1) / kCfgs[c].bm) * (a.N / kCfgs[c].bn);
    if (first_valid < 0) {
      first_valid = c;
      // long K but too few tiles of the efficient shape: keep that tile, split-K supplies the parallelism
      if (blocks < 300 && !a.geglu && a.Ktot / 64 >= 16 && c <= 3 && a.M >= 512) return c;
    }
    if (blocks >= 300) return c;
    if (blocks > best_blocks) { best_blocks = blocks; cfg = c; }
  }
  return cfg;
}

int mvd_launch_gemm(const MvdGemmArgs& a, hipStream_t s, int force_cfg) {
  // ---- host-side shape validation: a wrong shape must never reach the kernel
  if (a.M <= 0 || a.N <= 0 || a.Ktot <= 0 || a.nseg < 1 || a.nseg > 2) { mvd_set_error("gemm: bad dims M=%d N=%d K=%d nseg=%d", a.M, a.N, a.Ktot, a.nseg); return -1; }
  int ksum = 0;
  for (int i = 0; i < a.nseg; ++i) {
    const MvdASeg& g = a.seg[i];
    if (g.mode == MVD_A_DENSE) {
      if (g.c0 % 64 || g.c1 % 64 || g.ksize != g.c0 + g.c1 || !g.p0 || (g.c1 && !g.p1)) { mvd_set_error("gemm: bad dense segment %d (c0=%d c1=%d ksize=%d)", i, g.c0, g.c1, g.ksize); return -1; }
    } else if (g.mode == MVD_A_CONV3) {
      if (g.ups != 0 && g.ups != 1 && g.ups != 2) { mvd_set_error("gemm: bad conv segment %d (ups=%d)", i, g.ups); return -1; }
      if (g.c0 % 64 || g.c1 != 0 || g.ksize != (g.ups == 2 ? 4 : 9) * g.c0 || !g.p0 || (g.stride != 1 && g.stride != 2) || (g.ups && g.stride != 1)) { mvd_set_error("gemm: bad conv segment %d", i); return -1; }
      if (g.asym && (g.asym != 1 || g.stride != 2 || (g.inH & 1) || (g.inW & 1))) { mvd_set_error("gemm: bottom/right-only padding needs stride 2 and an even input size"); return -1; }
      const int eh = g.ups ? 2 * g.inH : (g.stride == 2 ? (g.inH + 1) / 2 : g.inH);
      const int ew = g.ups ? 2 * g.inW : (g.stride == 2 ? (g.inW + 1) / 2 : g.inW);
      if (eh != a.outH || ew != a.outW || a.rows_per_batch != a.outH * a.outW || a.M % a.rows_per_batch) { mvd_set_error("gemm: conv geometry mismatch (in %dx%d out %dx%d rpb %d M %d)", g.inH, g.inW, a.outH, a.outW, a.rows_per_batch, a.M); return -1; }
    } else { mvd_set_error("gemm: bad mode"); return -1; }
    ksum += g.ksize;
  }
  if (a.nseg == 2 && !(a.seg[0].mode == MVD_A_CONV3 && a.seg[1].mode == MVD_A_DENSE)) { mvd_set_error("gemm: a second segment must be a dense segment after a conv segment"); return -1; }
  if (ksum != a.Ktot) { mvd_set_error("gemm: segment K sum %d != Ktot %d", ksum, a.Ktot); return -1; }
  if (a.ldw < a.Ktot || (a.ldw % 8) || !a.W) { mvd_set_error("gemm: bad weight stride ldw=%d (K=%d)", a.ldw, a.Ktot); return -1; }
  if (a.rows_per_batch <= 0) { mvd_set_error("gemm: rows_per_batch must be > 0"); return -1; }
  if (a.N % 64) { mvd_set_error("gemm: N=%d must be a multiple of 64", a.N); return -1; }
  if (a.splitk > 1 && (!a.part || a.geglu || a.splitk > (force_cfg >= 100 ? 64 : 16) || a.splitk > a.Ktot / 64)) { mvd_set_error("gemm: bad split-K request (splitk=%d)", a.splitk); return -1; }
  if (a.geglu && (a.out_f32 || a.res || a.rowvec)) { mvd_set_error("gemm: unsupported GEGLU epilogue combination"); return -1; }
  if (a.relu && (a.relu != 1 || a.geglu || a.ln_c1 || a.nseg != 1 || a.w_blocked || (a.seg[0].mode == MVD_A_CONV3 && a.seg[0].ups == 2))) {
    mvd_set_error("gemm: the ReLU epilogue takes one dense or one 3x3 segment (no GEGLU, LayerNorm fold, fused shortcut, sub-pixel upsampler, blocked weights)");
    return -1;
  }
  const int on = a.geglu ? a.N / 2 : a.N;
  if (a.ldo < on || (a.ldo % 4) || (a.res && (a.ldres % 4))) { mvd_set_error("gemm: bad leading dims"); return -1; }
  if (!mvd_gemm_rowvec_aligned(a)) { mvd_set_error("gemm: the row vector is read 16 bytes at a time: ld_rowvec=%d must be a multiple of 4 and the base 16-byte aligned", a.ld_rowvec); return -1; }

  // force_cfg: -1 = heuristic; 0..5 = tile config with register staging; 8..13 = same tiles with LDS-DMA staging
  static const int default_glds = MVD_ENV_INT("MVD_GEMM_GLDS", 1);
  bool glds = default_glds != 0;
#ifdef MVD_PROBE
  static const int dbg = MVD_ENV_INT("MVD_GEMM_DEBUG", 0);
  if (dbg) const_cast<MvdGemmArgs&>(a).dbg = dbg;
#endif
  // the 2x2 sub-pixel form of an upsampling convolution exists in the ping-pong kernel only: no other kernel may see ups == 2
  if (a.seg[0].mode == MVD_A_CONV3 && a.seg[0].ups == 2) {
    if ((force_cfg >= 0 && force_cfg != 7) || (a.dbg & ~32) || !mvd_gemm_pp_up4_applicable(a)) {
      mvd_set_error("gemm: the 2x2 sub-pixel upsampling convolution does not take this problem (in %dx%d C=%d N=%d cfg=%d): source width a multiple of 16 or 8 (even height), N %% 320 == 0, bias only, unsplit",
                    a.seg[0].inH, a.seg[0].inW, a.seg[0].c0, a.N, force_cfg);
      return -1;
    }
    g_mvd_last_gemm.cfg = 7; g_mvd_last_gemm.splitk = 1;
    return mvd_launch_gemm_pp(a, s);
  }
  int cfg = force_cfg;
  // force_cfg >= 100: the small-M kernels of gemm_sm.hip, 100 + 10 * tile + ring depth (0: default 4)
  if (cfg >= 1000) { const_cast<MvdGemmArgs&>(a).w_blocked = 1; cfg -= 1000; }    // (+1000: W in the blocked LDS-image layout)
  if (a.w_blocked && cfg < 100) { mvd_set_error("gemm: the blocked weight layout is read by the small-M kernels only"); return -1; }
  if (cfg >= 100) {
    const int tile = (cfg - 100) / 10, ns = (cfg - 100) % 10;
    if (a.splitk > 1 && !a.tile_cnt) { mvd_set_error("gemm: the small-M kernels combine split-K in the kernel and need tile counters"); return -1; }
    g_mvd_last_gemm.cfg = cfg; g_mvd_last_gemm.splitk = a.splitk > 1 ? a.splitk : 1;
    return mvd_launch_gemm_sm(a, s, tile, ns ? ns : 4);
  }
#ifdef MVD_PROBE
  // probe builds only: force_cfg 15 = the ring-pipelined 256x320 experiment (gemm_ring.hip, not part of the product
  // library); MVD_GEMM_RING=1 routes every plain 256x320 launch to it
  static const int use_ring = MVD_ENV_INT("MVD_GEMM_RING", 0);
  if (cfg == 15) {
    if (a.N % 320 || a.geglu || a.out_f32) { mvd_set_error("gemm: the ring kernel needs N %% 320 == 0, bf16 output, no GEGLU"); return -1; }
    return mvd_launch_gemm_ring(a, s);
  }
#endif
  // force_cfg 16 / 17 = the lock-step (round-1) form of tile configs 6 / 7; 6 / 7 and the heuristic take the ping-pong kernels
  bool legacy = MVD_ENV_INT("MVD_GEMM_LEGACY", 0) != 0;
  if (cfg == 16 || cfg == 17) { legacy = true; cfg -= 10; }
  if (cfg == 14) { glds = true; cfg = 8; }       // force_cfg 14 = the 128x320 tile (LDS-DMA only)
  else if (cfg >= 8 && cfg < 14) { glds = true; cfg -= 8; } else if (cfg >= 0 && cfg < 6) { glds = false; }
  if (cfg < 0) cfg = mvd_gemm_pick_config(a);
  if (a.ln_c1) {   // LayerNorm fold: exists in the ping-pong kernels only (callers ask mvd_gemm_ln_fold_ok first)
    if ((cfg != 6 && cfg != 7) || legacy || a.dbg || !mvd_gemm_ln_fold_ok(a)) { mvd_set_error("gemm: LayerNorm fold not available for M=%d N=%d K=%d cfg=%d", a.M, a.N, a.Ktot, cfg); return -1; }
  }
  if (cfg < 0 || cfg >= kNumCfgs || a.N % kCfgs[cfg].bn || (a.geglu && !kCfgs[cfg].tn_even)) { mvd_set_error("gemm: no tile config for N=%d geglu=%d cfg=%d", a.N, a.geglu, cfg); return -1; }
  g_mvd_last_gemm.cfg = cfg; g_mvd_last_gemm.splitk = a.splitk > 1 ? a.splitk : 1;
#ifndef MVD_PROBE
  // tile configs the heuristic never picks (256x160, 256x128, 128x320) and the lock-step forms of 6 / 7 as a forced choice
  // exist in probe builds only (tools/build_variant.py <tag> -DMVD_PROBE)
  if (cfg == 0 || cfg == 1 || cfg == 8 || force_cfg == 16 || force_cfg == 17) { mvd_set_error("gemm: tile config %d exists in probe builds only", force_cfg >= 0 ? force_cfg : cfg); return -1; }
#endif
  // lock-step tiles 3, 4, 5 only (gemm_relu.hip); the other kernel families refuse relu in their applicability checks
  // (a split-K launch writes raw partials: it takes the plain kernel of the same tile, and the reduce pass applies the ReLU)
  if (a.relu) {
    if (cfg < 3 || cfg > 5) { mvd_set_error("gemm: the ReLU epilogue exists for tile configs 3, 4, 5 (128x128, 128x64, 64x64), not %d", force_cfg >= 0 ? force_cfg : cfg); return -1; }
    if (a.splitk <= 1) return mvd_launch_gemm_relu(a, s, cfg, glds);
  }
  switch (cfg) {
#ifdef MVD_PROBE
    case 0: return launch_cfg<C0>(a, s, glds);
    case 1: return launch_cfg<C1>(a, s, glds);
    case 8: return launch_cfg<C8>(a, s, true);
#endif
    case 2: return launch_cfg<C2>(a, s, glds);
    case 3: return launch_cfg<C3>(a, s, glds);
    case 4: return launch_cfg<C4>(a, s, glds);
    case 6:
      if (!a.geglu || a.seg[0].mode != MVD_A_DENSE || a.splitk > 1) { mvd_set_error("gemm: tile config 6 is GEGLU-only"); return -1; }
      if (!legacy && !(a.dbg & ~32) && mvd_gemm_pp_applicable(a)) return mvd_launch_gemm_pp(a, s);
      return launch_mode2<C6, 0, true, false>(a, s);
    case 7:
      if (!legacy && !(a.dbg & ~32) && !a.geglu && mvd_gemm_pp_applicable(a)) return mvd_launch_gemm_pp(a, s);
#ifdef MVD_PROBE
      if (use_ring && !a.out_f32 && !a.dbg) return mvd_launch_gemm_ring(a, s);
#endif
      return launch_cfg<C7, true>(a, s, true);
    default: return launch_cfg<C5>(a, s, glds);
  }
}

// Split-K heuristic: GEMMs whose tile grid cannot fill the chip (deep levels: M = batch * 64 pixels) but whose K
// is long are cut along K so that ~512 work items exist; the partials are summed by splitk_reduce_kernel.
int mvd_gemm_pick_splitk(const MvdGemmArgs& a) {
  if (a.geglu) return 1;
  const int cfg = mvd_gemm_pick_config(a);
  if (cfg < 0) return 1;
  const long tiles = (long)((a.M + kCfgs[cfg].bm - 1) / kCfgs[cfg].bm) * (a.N / kCfgs[cfg].bn);
  const int nkt = a.Ktot / 64;
  if (cfg == 7 && deep_conv_split(a, tiles) > 1) return deep_conv_split(a, tiles);
  if (cfg == 7 || cfg == 8) return (tiles >= 200 || nkt < 16) ? 1 : 2;   // one 115-147 KB workgroup per CU
  if (tiles >= 256 || nkt < 16) return 1;
  long s = 512 / tiles;                                       // two workgroups per CU
  if (s > nkt / 8) s = nkt / 8;
  // the fp32 partials (written and read back: 8 S M N bytes) against the weight bytes the split spreads over more CUs
  // (2 N K): up to 4 always, deeper while the partials stay below the weights -- the 8x8 / 16x16 levels at small batch
  // are pure weight streaming (M = 64, K = 11520: 29 MB of weights, 20 tiles), which a 4-way split leaves on 80 CUs
  long cap = (long)a.Ktot / (4L * a.M);
  cap = cap < 4 ? 4 : (cap > 16 ? 16 : cap);
  if (s > cap) s = cap;
  return s < 2 ? 1 : (int)s;
}

// the split factor the engine's schedule would use for a GEMM / conv of this size (tests drive mvd_op_* with it)
extern "C" int mvd_debug_pick_splitk(int m, int n, int k, int geglu) {
  MvdGemmArgs a; memset(&a, 0, sizeof(a));
  a.M = m; a.N = n; a.Ktot = k; a.geglu = geglu;
  return mvd_gemm_pick_splitk(a);
}
// the same for a 3x3 convolution (implicit GEMM: K = 9 * Cin + shortcut channels) -- the 8x8-level rule is for convolutions only
extern "C" int mvd_debug_pick_splitk_conv(int m, int n, int k) {
  MvdGemmArgs a; memset(&a, 0, sizeof(a));
  a.M = m; a.N = n; a.Ktot = k; a.seg[0].mode = MVD_A_CONV3;
  return mvd_gemm_pick_splitk(a);
}

// The route the engine's single-stream schedule gives a dense GEMM [a | a2][m][k1 + k2] . W[n][k1 + k2]^T with a residual (pure host
// arithmetic): out[5] = {family: 1 small-M kernels (gemm_sm.hip) / 0 tiled kernels, small-M tile / tile config, split-K factor,
// small-M ring depth (0: tiled), column tiles per group of the ping-pong kernel's walk (0: row-major)}.  -1 for a shape no dense
// launch takes (a source width that is no multiple of the 64-deep slab, N % 64).
extern "C" int mvd_debug_dense_route(int m, int n, int k1, int k2, int* out) {
  if (!out || m <= 0 || n <= 0 || k1 <= 0 || k2 < 0 || k1 % 64 || k2 % 64 || n % 64) { mvd_set_error("dense_route: bad shape M=%d N=%d K=%d+%d", m, n, k1, k2); return -1; }
  static const float dummy[4] = {};
  const bf16_t* p = reinterpret_cast<const bf16_t*>(dummy);      // (the planners look at shapes and at WHICH operands exist, never through them)
  MvdGemmArgs g; memset(&g, 0, sizeof(g));
  g.seg[0].p0 = p; g.seg[0].p1 = k2 ? p : nullptr; g.seg[0].c0 = k1; g.seg[0].c1 = k2; g.seg[0].mode = MVD_A_DENSE; g.seg[0].ksize = k1 + k2;
  g.nseg = 1; g.W = p; g.ldw = g.Ktot = k1 + k2; g.M = m; g.N = n; g.rows_per_batch = m; g.outH = 1; g.outW = m;
  g.bias = dummy; g.alpha = 1.f; g.out = const_cast<float*>(dummy); g.ldo = n; g.res = p; g.ldres = n;
  int tile = 0, ns = 0, S = 1;
  if (mvd_gemm_sm_plan(g, &tile, &ns, &S)) { out[0] = 1; out[1] = tile; out[2] = S; out[3] = ns; out[4] = 0; return 0; }
  const int cfg = mvd_gemm_pick_config(g);
  if (cfg < 0) { mvd_set_error("dense_route: no tile config for N=%d", n); return -1; }
  S = mvd_gemm_pick_splitk(g);
  g.splitk = S;
  out[0] = 0; out[1] = cfg; out[2] = S; out[3] = 0; out[4] = (cfg == 7 && mvd_gemm_pp_applicable(g)) ? mvd_gemm_pp_walk(g) : 0;
  return 0;
}

// Whether the ping-pong kernel takes a dense bf16 launch [m][k] . W[n][ldw]^T + res[m][ldres] -> out[m][ldo] (pure host arithmetic:
// mvd_gemm_pp_applicable); a forced tile config 7 that it does not take runs on the lock-step 256x320 tile.  ldres 0: no residual.
extern "C" int mvd_debug_gemm_pp_takes(int m, int n, int k, int ldw, int ldres, int ldo) {
  if (m <= 0 || n <= 0 || k <= 0 || ldw < k || ldo < n || ldres < 0) { mvd_set_error("gemm_pp_takes: bad shape M=%d N=%d K=%d ldw=%d ldres=%d ldo=%d", m, n, k, ldw, ldres, ldo); return -1; }
  alignas(16) static const float dummy[4] = {};
  const bf16_t* p = reinterpret_cast<const bf16_t*>(dummy);
  MvdGemmArgs g; memset(&g, 0, sizeof(g));
  g.seg[0].p0 = p; g.seg[0].c0 = k; g.seg[0].mode = MVD_A_DENSE; g.seg[0].ksize = k;
  g.nseg = 1; g.W = p; g.ldw = ldw; g.Ktot = k; g.M = m; g.N = n; g.rows_per_batch = m; g.outH = 1; g.outW = m;
  g.bias = dummy; g.alpha = 1.f; g.out = const_cast<float*>(dummy); g.ldo = ldo; g.res = ldres ? p : nullptr; g.ldres = ldres; g.splitk = 1;
  return mvd_gemm_pp_applicable(g) ? 1 : 0;
}

int mvd_launch_splitk_reduce(const MvdGemmArgs& a, hipStream_t s) {
  if (a.splitk < 2 || !a.part || (a.N & 3)) { mvd_set_error("splitk_reduce: bad arguments"); return -1; }
  const long nvec = (long)a.M * (a.N >> 2);
  int grid = (int)((nvec + 255) / 256);
  if (grid > 2048) grid = 2048;
  if (a.relu) return mvd_launch_splitk_reduce_relu(a, s, grid);
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(grid), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { mvd_set_error("splitk_reduce launch: %s", hipGetErrorString(e)); return -3; }
  return 0;
}
