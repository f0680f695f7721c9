// Host-side plumbing shared by the schedules (engine.hip, vae.hip, text.hip / vision.hip) and the operator-level entry points:
// weight slots, the bump arena, activations, the two shapes of MvdGemmArgs and the tiled launch with its reduce pass.
// What is NOT here is routing: which kernel family a problem goes to differs per schedule on purpose (the VAE never takes
// the small-M kernels, the CLIP towers (clip_layer.h) ask mvd_gemm_sm_plan first, the engine adds the xs / ws / up4 / two-stream policy).
#pragma once
#include <stdio.h>
#include <string.h>

#include <string>
#include <unordered_map>

#include "kernels.h"

#define CHECK(x) do { int _r = (x); if (_r) return _r; } while (0)

struct Weight { const void* p; int64_t numel; int dtype; };   // dtype: 0 fp32, 1 bf16

// registered weight slots of one model (one set of the engine)
struct WeightTable {
  std::unordered_map<std::string, Weight> m;
  bool has(const std::string& name) const { return m.count(name) != 0; }
  // the slot's pointer, or null with *err = -10 (missing) / -11 (dtype or numel).  Messages: "<prefix>missing weight slot
  // '<name>'[ in set <set>]" and "<prefix>weight slot '<name>'[ (set <set>)]: expected ..." (set < 0: no set in the message)
  const void* find(const std::string& name, int dtype, int64_t numel, int* err, const char* prefix = "", int set = -1) const {
    char in_set[24] = "", of_set[24] = "";
    if (set >= 0) { snprintf(in_set, sizeof(in_set), " in set %d", set); snprintf(of_set, sizeof(of_set), " (set %d)", set); }
    auto it = m.find(name);
    if (it == m.end()) { mvd_set_error("%smissing weight slot '%s'%s", prefix, name.c_str(), in_set); *err = -10; return nullptr; }
    if (it->second.dtype != dtype || it->second.numel != numel) {
      mvd_set_error("%sweight slot '%s'%s: expected dtype %d numel %lld, got dtype %d numel %lld", prefix, name.c_str(), of_set, dtype,
                    (long long)numel, it->second.dtype, (long long)it->second.numel);
      *err = -11; return nullptr;
    }
    return it->second.p;
  }
};

// bump allocator over a bound buffer; a dry run (sizing) hands out fake pointers and only moves the high-water mark
struct Arena {
  char* base = nullptr;
  size_t cap = 0, off = 0, high = 0;
  bool dry = false;
  void* alloc(size_t bytes) {
    off = (off + 255) & ~size_t(255);
    void* p = dry ? (void*)(uintptr_t)(0x1000 + off) : (void*)(base + off);
    off += bytes;
    if (off > high) high = off;
    return p;
  }
  template <class T> T* alloc_n(size_t n) { return (T*)alloc(n * sizeof(T)); }
  void reset(bool dry_) { dry = dry_; off = high = 0; }
  bool overflow() const { return !dry && high > cap; }
};

struct Act {  // NHWC bf16 activation
  bf16_t* p = nullptr;
  int B = 0, H = 0, W = 0, C = 0;
  int hw() const { return H * W; }
  int rows() const { return B * H * W; }
};
inline Act arena_act(Arena& ar, int B, int H, int W, int C) { return Act{ar.alloc_n<bf16_t>((size_t)B * H * W * C), B, H, W, C}; }

// ---------------------------------------------------------------- the two shapes of MvdGemmArgs
// Everything a builder does not name stays zero (splitk = 0: undecided); callers set what is theirs: res / ldres, rowvec,
// geglu, ln_c1, out_f32, alpha, splitk.
// dense: out[M][N] = [a | a2][M][k1 + k2] . w[N][ldw]^T + bias     (ldw 0: k1 + k2)
inline MvdGemmArgs gemm_dense(const bf16_t* a, const bf16_t* a2, int k1, int k2, int M, const bf16_t* w, int ldw, const float* bias, int N,
                              void* out, int ldo) {
  MvdGemmArgs g; memset(&g, 0, sizeof(g));
  g.seg[0].p0 = a; g.seg[0].p1 = a2; g.seg[0].c0 = k1; g.seg[0].c1 = k2; g.seg[0].mode = MVD_A_DENSE; g.seg[0].ksize = k1 + k2;
  g.nseg = 1; g.W = w; g.ldw = ldw ? ldw : k1 + k2; g.M = M; g.N = N; g.Ktot = k1 + k2; g.rows_per_batch = M; g.outH = 1; g.outW = M;
  g.bias = bias; g.alpha = 1.f; g.out = out; g.ldo = ldo;
  return g;
}
// 3x3 convolution of x[batch][inH][inW][cin] as an implicit GEMM (K = 9 cin), optionally with a dense segment
// [sc0 | sc1][M][scc0 + scc1] behind it along K (the fused 1x1 shortcut); out[batch][outH][outW][cout] bf16, ldres = cout
inline MvdGemmArgs gemm_conv3(const bf16_t* x, int inH, int inW, int cin, int stride, int ups, int asym, const bf16_t* sc0,
                              const bf16_t* sc1, int scc0, int scc1, const bf16_t* w, const float* bias, int batch, int outH, int outW,
                              int cout, void* out) {
  MvdGemmArgs g; memset(&g, 0, sizeof(g));
  g.seg[0].p0 = x; g.seg[0].c0 = cin; g.seg[0].mode = MVD_A_CONV3; g.seg[0].ksize = 9 * cin;
  g.seg[0].inH = inH; g.seg[0].inW = inW; g.seg[0].stride = stride; g.seg[0].ups = ups; g.seg[0].asym = asym;
  g.nseg = 1; g.Ktot = 9 * cin;
  if (sc0) {
    g.seg[1].p0 = sc0; g.seg[1].p1 = sc1; g.seg[1].c0 = scc0; g.seg[1].c1 = scc1; g.seg[1].mode = MVD_A_DENSE;
    g.seg[1].ksize = scc0 + scc1; g.nseg = 2; g.Ktot += scc0 + scc1;
  }
  g.W = w; g.ldw = g.Ktot; g.M = batch * outH * outW; g.N = cout; g.rows_per_batch = outH * outW; g.outH = outH; g.outW = outW;
  g.bias = bias; g.ldres = cout; g.alpha = 1.f; g.out = out; g.ldo = cout;
  return g;
}
// the same convolution behind a nearest-2x upsample as four 2x2 sub-pixel convolutions (seg[0].ups = 2, K = 4 cin; the
// caller sets W = packing.pack_up4)
inline void gemm_conv3_to_up4(MvdGemmArgs& g) {
  g.seg[0].ups = 2; g.seg[0].ksize = 4 * g.seg[0].c0; g.Ktot = g.seg[0].ksize; g.ldw = g.Ktot;
}

// launch of the tiled kernels, then the reduce pass when K was split (g.splitk > 1).  `wrap` brackets the GEMM launch alone
// (the engine's per-class profiling).
template <class Wrap> int launch_tiled(const MvdGemmArgs& g, hipStream_t s, int force_cfg, Wrap&& wrap) {
  const int r = wrap([&] { return mvd_launch_gemm(g, s, force_cfg); });
  return !r && g.splitk > 1 ? mvd_launch_splitk_reduce(g, s) : r;
}
inline int launch_tiled(const MvdGemmArgs& g, hipStream_t s, int force_cfg = -1) {
  return launch_tiled(g, s, force_cfg, [](auto&& launch) { return launch(); });
}
