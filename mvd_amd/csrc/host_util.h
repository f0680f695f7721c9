// Host-side plumbing shared by the schedules (engine.hip, vae.hip, text.hip / vision.hip, the metric towers) and the operator-level
// entry points: the launch check, weight slots, the bump arena, activations, the two shapes of MvdGemmArgs, the tiled launch with its
// reduce pass, and the scaffold of a handle module (ModuleBase, TowerCtx, pairs_per_pass).
// What is NOT here is routing: which kernel family a problem goes to differs per schedule on purpose (the VAE never takes
// the small-M kernels, the CLIP towers (clip_layer.h) ask mvd_gemm_sm_plan first, the engine adds the xs / ws / up4 / two-stream policy).
#pragma once
#include <stdio.h>
#include <string.h>

#include <string>
#include <unordered_map>

#include "kernels.h"

#define CHECK(x) do { int _r = (x); if (_r) return _r; } while (0)

// after a kernel launch: -3 and "<what> launch: <error>" when it did not go out
inline int launch_check(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { mvd_set_error("%s launch: %s", what, hipGetErrorString(e)); return -3; }
  return 0;
}
inline long blocks_of(long n) { return (n + 255) / 256; }      // workgroups of 256 threads over n items
inline size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

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
    off = align256(off);
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

// the tiled kernels with the split-K the tile heuristic asks for; the partials live in the arena for the launch alone
inline int arena_gemm(Arena& ar, MvdGemmArgs& g, hipStream_t s, bool dry) {
  const int S = mvd_gemm_pick_splitk(g);
  const size_t mark = ar.off;
  if (S > 1) { g.splitk = S; g.part = ar.alloc_n<float>((size_t)S * g.M * g.N); }
  const int r = dry ? 0 : launch_tiled(g, s);
  ar.off = mark;
  return r;
}

// ---------------------------------------------------------------- the scaffold of a handle module (mvd_vae, mvd_text, mvd_vision, mvd_vgg, ...)
// What every handle owns: its weight slots, the bound workspace and the arena over it.  `who` is the module's name in its
// messages ("vgg" -> "vgg_set_weight: ...").
struct ModuleBase {
  WeightTable w;
  void* ws_ptr = nullptr; int64_t ws_bytes = 0;
  Arena ar;
};
inline int module_set_weight(ModuleBase* m, const char* who, const char* slot, const void* ptr, int64_t numel, int dtype) {
  if (!m || !slot || !ptr || numel <= 0 || dtype < 0 || dtype > 1) { mvd_set_error("%s_set_weight: bad argument", who); return -1; }
  if ((uintptr_t)ptr & 15) { mvd_set_error("%s_set_weight: '%s' must be 16-byte aligned", who, slot); return -1; }
  m->w.m[slot] = Weight{ptr, numel, dtype};
  return 0;
}
// min_bytes: what the module keeps at the head of its workspace (a buffer of that size or less holds nothing)
inline int module_bind_workspace(ModuleBase* m, const char* who, void* ws, int64_t bytes, int64_t min_bytes) {
  if (!m || !ws || bytes <= min_bytes || ((uintptr_t)ws & 255)) { mvd_set_error("%s_bind_workspace: bad argument (256-byte aligned buffer)", who); return -1; }
  m->ws_ptr = ws; m->ws_bytes = bytes;
  return 0;
}
// a real run's arena: the bound workspace behind its first `head` bytes
inline void module_bind_arena(ModuleBase& m, size_t head) {
  m.ar.reset(false);
  m.ar.base = reinterpret_cast<char*>(m.ws_ptr) + head;
  m.ar.cap = (size_t)m.ws_bytes - head;
}

// One run of a tower's schedule over m->ar.  dry: sizes only; check_w false (sizing): weight slots are not looked at.  The first
// failed lookup stays in err, and W() answers null from then on.
struct TowerCtx {
  ModuleBase* m; hipStream_t s; bool dry, check_w;
  const char* prefix;      // of the weight-slot messages ("vgg: ", "lpips: ")
  int err = 0;
  const void* W(const std::string& n, int dtype, int64_t numel) {
    if (!check_w) return (const void*)(uintptr_t)0x1000;
    if (err) return nullptr;
    return m->w.find(n, dtype, numel, &err, prefix);
  }
  // the partials are exactly what this launch needs (a tower whose pass sizes must be monotone in the batch reserves its own bound)
  int gemm(MvdGemmArgs& g) { return err ? err : arena_gemm(m->ar, g, s, dry); }
};

// Pairs per pass of a loss that runs in several passes: *pp shrinks (by the ratio of bound to need) until its passes fit `bound` bytes.
// need_of(pp, &need) sizes them: an error, or 0 with need = the bytes, ~size_t(0) when a pass of pp pairs has 2^31 rows or more.
// -4 and "<who>: workspace too small for one pair ..." when not even one pair fits.
template <class NeedOf> int pairs_per_pass(const char* who, int h, int w, int64_t bound, NeedOf&& need_of, int* pp) {
  for (;;) {
    size_t need = 0;
    CHECK(need_of(*pp, &need));
    if (need <= (size_t)bound) return 0;
    if (*pp == 1) { mvd_set_error("%s: workspace too small for one pair of %d x %d: need %zu bytes, bound %lld", who, h, w, need, (long long)bound); return -4; }
    const int guess = need == ~size_t(0) ? *pp / 2 : (int)((double)*pp * (double)bound / (double)need);
    *pp = guess < 1 ? 1 : (guess >= *pp ? *pp - 1 : guess);
  }
}
