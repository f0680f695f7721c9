// Host-side schedule of one MultiViewUNet.forward on one MI355X: the whole forward
// (camera encoder -> reference-image encoder UNet -> adapter K/V -> main UNet) is issued
// from C++ behind a single C-ABI call; Python only hands over device pointers.
//
// Follows /root/reference/src/models/mvd_unet.py:179-338 (orchestration),
// image_encoder.py:97-112 (encoder pass at t=0, 16 captured maps),
// attention.py:48-188 (adapter branch), camera_encoder.py:160-255 (embedding + FiLM) and
// the diffusers-0.32.2 UNet2DConditionModel layer order.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "host_util.h"
#include "ragged.h"

int mvd_launch_silu_to_bf16(const float* x, int64_t n, bf16_t* y, hipStream_t s);

// measurement / bisection switches (bench.py --debug-flags, tools/): mvd_debug_flag_t of include/mvd_hip.h
static int g_debug_flags = 0;
extern "C" int mvd_debug_set_flags(int flags) { g_debug_flags = flags; return 0; }
int mvd_debug_flags() { return g_debug_flags; }

namespace {

struct FeatureInfo { std::string name; int level; int C; int heads; std::string key; /* weight-slot prefix of the block */ };
constexpr int MVD_REF_ONLY_INTERNAL = 1 << 30;   // set by mvd_engine_reference_encode only (rejected on the public entry)

// The main-pass options (include/mvd_hip.h "main-pass options"): what the setters set, as one value.  mvd_engine::opt is assigned by
// apply_main_opts alone; the main pass reads it through PassOpts::main, the encoder pass never sees it.
struct MainOpts {
  bool freeu_on = false; float freeu_s[2] = {1.f, 1.f}, freeu_b[2] = {1.f, 1.f};   // FreeU: up blocks 0 and 1 read re-weighted hidden / skip inputs
  double tome_ratio = 0.0; int tome_maxds = 1; bool tome_keep = false;              // token merging: attn1 of the eligible blocks on the merged sequence
  int todo_f[2] = {1, 1}, todo_method = 0;    // token downsampling: the K/V factor at the latent's own level / one level below (1: off)
  bool dc_on = false; int dc_branch = 0;      // DeepCache
  bool taps_on = false;                       // main-pass taps
  bool merges() const { return tome_ratio > 0.0; }
  bool downsamples() const { return todo_f[0] > 1 || todo_f[1] > 1; }
};
enum MainOptField { OPT_FREEU, OPT_TOME, OPT_TODO, OPT_DEEPCACHE, OPT_TAPS };

}  // namespace

struct mvd_engine {
  mvd_config_t cfg;
  WeightTable w[2];
  Arena tmp, act, persist;
  void* ws_ptr = nullptr; int64_t ws_bytes = 0;
  void* rc_ptr = nullptr; int64_t rc_bytes = 0;
  std::vector<FeatureInfo> feats;
  // reference cache state (valid after a forward with MVD_USE_IMAGE)
  std::vector<bf16_t*> refkv;       // per feature: [ref_batch*hw][4C]
  std::vector<bf16_t*> feat_keep;   // per feature: [ref_batch][hw][C] when kept
  int rc_batch = 0, rc_h = 0, rc_w = 0; bool rc_valid = false; bool rc_keep = false;
  std::vector<int> rc_layout;       // ViewLayout::key() of the forward that filled the cache (ragged.h)
  // global Q2 statistics (mvd_engine_reference_encode / _finish): the encoder pass stops before the normalisation
  float* ref_stats_out = nullptr;   // set only while mvd_engine_reference_encode runs
  bool rc_pending = false;          // raw features are in feat_keep, waiting for the merged statistics
  int64_t ref_pixels(int h, int w) const { int64_t n = 0; for (auto& f : feats) n += (int64_t)(h >> f.level) * (w >> f.level); return n; }
  int64_t feat_pixel_off(int idx) const { int64_t n = 0; for (int i = 0; i < idx; ++i) n += (int64_t)(rc_h >> feats[i].level) * (rc_w >> feats[i].level); return n; }
  float* cam_emb = nullptr; int cam_batch = 0;
  // arrival counters of the in-kernel split-K combine (gemm_sm.hip): one zeroed block per entry call, carved from the
  // workspace, every split-K launch of the call takes its own slice (no counter is ever re-used inside a call)
  unsigned int* cnt_base = nullptr; int cnt_used = 0, cnt_cap = 0;
  // The reference-image encoder pass and the main pass are two chains of kernels of which the second needs the first only at
  // its adapter attentions (feature by feature) -- so the encoder pass is issued on a SIDE STREAM and the main pass waits per
  // feature on an event.  At batch 1 (infer.py) each chain alone leaves most of the chip idle.
  hipStream_t side = nullptr;
  std::vector<hipEvent_t> feat_ev;          // one per feature: its adapter K/V are complete
  hipEvent_t fork_ev = nullptr, join_ev = nullptr;
  bool dual_now = false;                    // this forward runs the encoder pass on the side stream
  int ensure_side_stream() {
    if (side) return 0;
    {
      // the side stream gets the HIGHEST priority: the encoder pass is the producer of every adapter attention's K/V, and with it
      // ahead the main pass fills the gaps (cfg4 cold, same box: default priority 63.06 / 62.83 ms, lowest 62.92 / 62.78, highest
      // 62.69 / 62.58; batch 1 indifferent; MVD_DBG_SIDE_DEFAULT_PRIORITY, for A/B)
      int lo = 0, hi = 0;
      (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
      const int pr = (g_debug_flags & MVD_DBG_SIDE_DEFAULT_PRIORITY) ? 0 : hi;
      if (hipStreamCreateWithPriority(&side, hipStreamNonBlocking, pr) != hipSuccess) { mvd_set_error("engine: hipStreamCreate failed"); return -3; }
    }
    feat_ev.resize(feats.size());
    for (auto& ev : feat_ev) if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { mvd_set_error("engine: hipEventCreate failed"); return -3; }
    if (hipEventCreateWithFlags(&fork_ev, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&join_ev, hipEventDisableTiming) != hipSuccess) { mvd_set_error("engine: hipEventCreate failed"); return -3; }
    return 0;
  }
  bool share_encoder = false;       // N4: the encoder pass reads weight set 0 (base UNet == image-encoder UNet)
  MainOpts opt;                     // FreeU, token merging, token downsampling, DeepCache, taps: see MainOpts and apply_main_opts
  // Records and buffers of the last issued forward (not options).  tome_tab: with opt.tome_keep, the slot table of every feature's
  // block (workspace memory; rows 0: the block did not merge); todo_nk: the keys of every feature's block (0: full)
  struct TomeTable { int* p = nullptr; int64_t n = 0; };
  std::vector<TomeTable> tome_tab;
  std::vector<int> todo_nk;
  // DeepCache (include/mvd_hip.h): the stored deep feature lives in a buffer of its own (the reference cache's allocator is reset by
  // every cold forward) and carries the record of the refresh forward that wrote it.  The record is NOT part of HostState: it is
  // written by unet_forward once a refresh forward has been issued (launched, captured or replayed), so replaying some other
  // forward's graph cannot roll it back.
  void* dc_ptr = nullptr; int64_t dc_bytes = 0;
  // Main-pass taps (include/mvd_hip.h): with opt.taps_on, the record of every block output of the last issued forward's main pass,
  // in execution order.  The tensors are the pass's own activations (workspace memory, like tome_tab: nothing of the main pass is
  // freed before the forward ends); only a FiLM hook that runs in place gets an output of its own.
  struct Tap { std::string name; const bf16_t* p; int B, H, W, C; };
  std::vector<Tap> taps;
  uint64_t weight_gen = 0;          // bumped by mvd_engine_set_weight / mvd_engine_clear_weights
  struct DeepRecord { bool valid = false; int batch = 0, h = 0, w = 0, cam = 0, img = 0, branch = 0; uint64_t wgen = 0; std::vector<int> layout; } dc_rec;
  bool dc_sizing = false;           // a sizing entry's dry run of a shallow forward: no stored feature is needed to size one
  int dc_hidden_channels() const { return cfg.layers_per_block - 1 - opt.dc_branch >= 1 ? cfg.block_out_channels[0] : cfg.block_out_channels[1]; }
  // hipGraph replay of whole forwards (mvd_engine_set_graph): one instantiated graph per distinct (arguments, cache state)
  struct HostState {                  // what a forward leaves behind on the host side
    std::vector<bf16_t*> refkv, feat_keep;
    int rc_batch, rc_h, rc_w; bool rc_valid, rc_keep;
    float* cam_emb; int cam_batch;
    std::vector<int> rc_layout;
    std::vector<Tap> taps;
    std::vector<int> todo_nk;
  };
  HostState host_state() const { return {refkv, feat_keep, rc_batch, rc_h, rc_w, rc_valid, rc_keep, cam_emb, cam_batch, rc_layout, taps, todo_nk}; }
  void set_host_state(const HostState& h) {
    refkv = h.refkv; feat_keep = h.feat_keep; rc_batch = h.rc_batch; rc_h = h.rc_h; rc_w = h.rc_w; rc_valid = h.rc_valid;
    rc_keep = h.rc_keep; cam_emb = h.cam_emb; cam_batch = h.cam_batch; rc_layout = h.rc_layout; taps = h.taps; todo_nk = h.todo_nk;
  }
  struct GraphEntry { std::string key; hipGraph_t g; hipGraphExec_t x; HostState after; };
  bool dual_late = false;                   // set by the main pass once it runs (mostly) alone again: single-stream launch policy
  bool graph_on = false;
  std::vector<GraphEntry> graphs;
  std::vector<std::string> graph_seen;      // keys that ran once un-captured (first-use initialisation happens there)
  void drop_graphs() {
    for (auto& ge : graphs) { (void)hipGraphExecDestroy(ge.x); (void)hipGraphDestroy(ge.g); }
    graphs.clear(); graph_seen.clear();
  }
  // K/V tables of the ragged forwards (mvd_unet_forward_ragged): one device slot per layout (view counts, g), holding the adapter
  // table and the text table, g * R entries each.  A slot is written ONCE, by a stream-ordered upload on the first forward of its
  // layout (never inside a capture), and is not rewritten while a captured graph can point at it: the set is bounded, and making
  // room for a new layout drops every captured graph first (they are re-captured on their next use).
  struct KvSlot { std::vector<int> layout /* counts..., g */, host /* [adapter | text] */; int* dev = nullptr; uint64_t used = 0; };
  static constexpr size_t KV_SLOTS = 8;
  std::vector<KvSlot> kv_slots; uint64_t kv_tick = 0;
  ~mvd_engine() {
    drop_graphs();
    for (auto& sl : kv_slots) if (sl.dev) (void)hipFree(sl.dev);
    for (hipEvent_t ev : ev_pool) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : feat_ev) if (ev) (void)hipEventDestroy(ev);
    if (fork_ev) (void)hipEventDestroy(fork_ev);
    if (join_ev) (void)hipEventDestroy(join_ev);
    if (side) (void)hipStreamDestroy(side);
  }
  std::vector<int> temb_off;        // per resnet offset into the fused time_emb_proj output
  int temb_total = 0;
  std::vector<int> tkv_off;         // per transformer column offset into the fused text K/V projection
  int tkv_total = 0;
  // optional per-kernel-class profiling (HIP events on the launch stream)
  bool prof = false;
  bool prof_overlap = false;      // mvd_engine_set_profiling(e, 2): record launches WITHOUT giving up the two-stream schedule
  struct ProfRec { int cls; double flops; double bytes; hipEvent_t e0, e1; int M, N, K, tag; };
  int prof_M = 0, prof_N = 0, prof_K = 0, prof_tag = 0;   // shape of the launch being recorded (per-shape dump)
  std::vector<ProfRec> prof_recs;
  std::vector<hipEvent_t> ev_pool; size_t ev_used = 0;
  hipEvent_t get_event() {
    if (ev_used == ev_pool.size()) { hipEvent_t ev = nullptr; (void)hipEventCreate(&ev); ev_pool.push_back(ev); }
    return ev_pool[ev_used++];
  }
};

// profiling class (MvdProfClass, kernels.h) of a launch of the tiled kernels with tile config `cfg`
static inline int gemm_class(const MvdGemmArgs& g, int cfg, int splitk) {
  if (cfg == 8) return MVD_PC_GEMM_128X320;
  if (cfg == 7) return splitk > 1 ? MVD_PC_PP_SPLITK : (g.seg[0].mode == MVD_A_CONV3 ? MVD_PC_PP_CONV3 : (g.ln_c1 ? MVD_PC_PP_LN_DENSE : MVD_PC_PP_DENSE));
  return MVD_PC_GEMM_256X160 + cfg;       // (configs 0..5 of gemm.hip, 6 = MVD_PC_PP_GEGLU)
}
int mvd_attention_pick_nw(const MvdAttnArgs& a);

namespace {

#ifdef MVD_PROBE
struct WsCheckRec { std::string slot; int set; bool side; const char* p[4]; size_t n[4]; };
static std::vector<WsCheckRec> g_ws_recs;
static unsigned long long* g_ws_cnt = nullptr;      // pinned: [launch][2] = {elements beyond tolerance, elements compared}
__global__ void ws_check_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ b, long n, unsigned long long* cnt_l, unsigned long long* cnt, unsigned long long launch) {
  unsigned long long bad = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float va = bflo((unsigned)a[i]), vb = bflo((unsigned)b[i]);
    if (!(fabsf(va - vb) <= 0.03f * fabsf(vb) + 0.05f)) {
      ++bad;
      const unsigned long long k = __hip_atomic_fetch_add(cnt + 8192 * 2 - 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      if (k < 4096) { cnt[8192 * 2 + 2 * k] = (unsigned long long)i | (launch << 40); cnt[8192 * 2 + 2 * k + 1] = ((unsigned long long)__float_as_uint(va) << 32) | __float_as_uint(vb); }
    }
  }
  if (bad) __hip_atomic_fetch_add(cnt_l, bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_fetch_add(cnt_l + 1, (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
extern "C" void mvd_debug_ws_check_report(void);
static const char* g_ws_ptrs[4]; static size_t g_ws_lens[4];
static void ws_check_launch(const std::string& slot, int set, bool side, const bf16_t* a, const bf16_t* b, long n, hipStream_t s) {
  if (!g_ws_cnt) {
    (void)hipHostMalloc(&g_ws_cnt, (8192 * 2 + 8192) * sizeof(unsigned long long), hipHostMallocMapped); memset(g_ws_cnt, 0, (8192 * 2 + 8192) * sizeof(unsigned long long));
    atexit(mvd_debug_ws_check_report);
  }
  if (g_ws_recs.size() >= 4096) return;
  g_ws_recs.push_back({slot, set, side, {g_ws_ptrs[0], g_ws_ptrs[1], g_ws_ptrs[2], g_ws_ptrs[3]}, {g_ws_lens[0], g_ws_lens[1], g_ws_lens[2], g_ws_lens[3]}});
  hipLaunchKernelGGL(ws_check_kernel, dim3(64), dim3(256), 0, s, a, b, n, g_ws_cnt + 2 * (g_ws_recs.size() - 1), g_ws_cnt, (unsigned long long)(g_ws_recs.size() - 1));
}
extern "C" void mvd_debug_ws_check_report(void) {
  (void)hipDeviceSynchronize();
  int nbad = 0;
  for (size_t i = 0; i < g_ws_recs.size(); ++i)
    if (g_ws_cnt[2 * i]) { ++nbad; fprintf(stderr, "ws check: launch %zu %s (set %d, %s stream): %llu of %llu elements beyond tolerance\n", i, g_ws_recs[i].slot.c_str(), g_ws_recs[i].set, g_ws_recs[i].side ? "side" : "main", g_ws_cnt[2 * i], g_ws_cnt[2 * i + 1]); }
  {   // where the mismatches sit
    const unsigned long long nlog = g_ws_cnt[8192 * 2 - 1] < 4096 ? g_ws_cnt[8192 * 2 - 1] : 4096;
    // print the first 24 raw entries (index decoded by the reader: idx = m * N + n)
    for (unsigned long long k = 0; k < nlog && k < 24; ++k) {
      const unsigned long long v = g_ws_cnt[8192 * 2 + 2 * k], w = g_ws_cnt[8192 * 2 + 2 * k + 1];
      const unsigned ua = (unsigned)(w >> 32), ub = (unsigned)w; float fa, fb; memcpy(&fa, &ua, 4); memcpy(&fb, &ub, 4);
      fprintf(stderr, "ws check: mismatch launch %llu idx %llu: ws %g tiled %g\n", v >> 40, v & ((1ull << 40) - 1), fa, fb);
    }
  }
  // operand ranges (x, sc0, sc1, out) of launches of DIFFERENT passes of one forward must never overlap
  static const char* kind[4] = {"x", "sc0", "sc1", "out"};
  int nov = 0;
  for (size_t i = 0; i < g_ws_recs.size() && nov < 12; ++i)
    for (size_t j = i + 1; j < g_ws_recs.size() && j < i + 40 && nov < 12; ++j) {
      if (g_ws_recs[i].side == g_ws_recs[j].side) continue;
      for (int u = 0; u < 4; ++u) for (int v = 0; v < 4; ++v) {
        const char* a0 = g_ws_recs[i].p[u]; const char* b0 = g_ws_recs[j].p[v];
        if (!a0 || !b0 || (u != 3 && v != 3)) continue;               // (an overlap matters when one side writes)
        if (a0 < b0 + g_ws_recs[j].n[v] && b0 < a0 + g_ws_recs[i].n[u]) {
          ++nov; fprintf(stderr, "ws check: OVERLAP launch %zu %s (%s stream) %s [%p, +%zu) with launch %zu %s (%s stream) %s [%p, +%zu)\n", i, g_ws_recs[i].slot.c_str(), g_ws_recs[i].side ? "side" : "main", kind[u], (const void*)a0, g_ws_recs[i].n[u], j, g_ws_recs[j].slot.c_str(), g_ws_recs[j].side ? "side" : "main", kind[v], (const void*)b0, g_ws_recs[j].n[v]);
        }
      }
    }
  fprintf(stderr, "ws check: %d operand overlaps between the two passes\n", nov);
  fprintf(stderr, "ws check: %zu conv_ws launches compared with the tiled kernel, %d with elements beyond tolerance\n", g_ws_recs.size(), nbad);
}
#endif

struct Ctx {
  mvd_engine* e;
  hipStream_t s;
  int set;          // weight set of the current UNet pass
  bool dry;
  int err = 0;
  bool nowait = false;   // split-K combines must not wait for other workgroups (kernels of two streams share the chip)
  int tag_base = -1;     // >= 0: the shape table's tag of the next GEMM launches instead of mode * 100 + geglu * 10 (the split is added)

  const void* W(const std::string& name, int dtype, int64_t numel, int set_override = -1) {
    if (dry) return nullptr;  // sizing run: weights need not be registered
    const int st = set_override >= 0 ? set_override : set;
    return e->w[st].find(name, dtype, numel, &err, "", st);
  }
  const bf16_t* WB(const std::string& n, int64_t numel, int so = -1) { return (const bf16_t*)W(n, 1, numel, so); }
  const float* WF(const std::string& n, int64_t numel, int so = -1) { return (const float*)W(n, 0, numel, so); }
  bool has(const std::string& n, int so = -1) { return e->w[so >= 0 ? so : set].has(n); }

  template <class T> T* talloc(size_t n) { return e->tmp.alloc_n<T>(n); }
  template <class T> T* aalloc(size_t n) { return e->act.alloc_n<T>(n); }
  Act new_act(int B, int H, int W_, int C, bool longlived) { return arena_act(longlived ? e->act : e->tmp, B, H, W_, C); }

  // ------------------------------------------------------------------ op wrappers
  template <class F> int profiled(int cls, double flops, double bytes, F&& launch) {
    if (!e->prof) return launch();
    hipEvent_t e0 = e->get_event(), e1 = e->get_event();
    (void)hipEventRecord(e0, s);
    const int r = launch();
    (void)hipEventRecord(e1, s);
    e->prof_recs.push_back({cls, flops, bytes, e0, e1, e->prof_M, e->prof_N, e->prof_K, e->prof_tag});
    return r;
  }
  // whether the small-M kernels (gemm_sm.hip) are in use at all: ONE predicate for Ctx::gemm's route and for ln_linear's
  // "the fold is available through them" test (a kill switch must make the forward fall back, not fail)
  static bool sm_enabled() {
    static const bool use_sm = MVD_ENV_INT("MVD_GEMM_SM", 1) != 0;
    return use_sm && !(g_debug_flags & MVD_DBG_NO_SM);
  }
  // split factor and forced tile config (-1: the heuristic's) of a launch of the tiled kernels
  void tiled_plan(const MvdGemmArgs& g, int& S, int& fc) {
    // split-K for tile grids that cannot fill the chip: fp32 partials in scoped workspace + a reduce/epilogue pass
    S = mvd_gemm_pick_splitk(g);
    fc = -1;
    // While the encoder pass runs beside the main pass (two streams, forward_impl) a launch need not fill the chip by itself --
    // the other stream's kernels take the idle CUs -- so the two devices that exist only to fill it are dropped: the 256x320
    // tile is not split along K at 128 tiles (16x16 level; no fp32 partials, no reduce pass), and 100+ tiles of it are preferred
    // to 512 of the 128x160 tile (measured on one box, cfg4 cold: 65.6 -> 64.6 -> 63.5 ms per step; halving or dropping the
    // four-way split of the 8x8 level instead: no gain / a loss; profiles/r03_probe_dual_stream_policies.log).
    if (e->dual_now && !e->dual_late && !(g_debug_flags & MVD_DBG_SINGLE_STREAM_POLICY) && !g.geglu && !g.ln_c1 && !g.out_f32 && g.N % 320 == 0 && mvd_gemm_pp_applicable(g)) {
      const int cfg = mvd_gemm_pick_config(g);
      const long t7 = (long)((g.M + 255) / 256) * (g.N / 320);
      if (t7 >= 100) { S = 1; if (cfg != 7) fc = 7; }      // (below 100 tiles -- the 8x8 level -- the heuristic's tile and split stand)
    }
  }
  int gemm(MvdGemmArgs& g) {
    if (err) return err;
    // small problems (one image's feature maps): the latency-oriented kernels of gemm_sm.hip, split-K combined in the kernel
    int sm_tile = 0, sm_ns = 0, sm_S = 1;
    if (sm_enabled() && mvd_gemm_sm_plan(g, &sm_tile, &sm_ns, &sm_S)) {
      if (g_debug_flags & MVD_DBG_SM_NO_SPLITK) sm_S = 1;
      const size_t mark = e->tmp.off;
      if (sm_S > 1) {
        g.splitk = sm_S; g.splitk_nowait = nowait ? 1 : 0; g.part = talloc<float>((size_t)sm_S * g.M * g.N);
        const int tiles = ((g.M + 63) / 64) * (g.N / 64);           // (an upper bound for every tile shape)
        g.tile_cnt = e->cnt_base + e->cnt_used;
        e->cnt_used += tiles;
        if (!dry && e->cnt_used > e->cnt_cap) { mvd_set_error("forward: split-K tile counters exhausted (%d > %d)", e->cnt_used, e->cnt_cap); return err = -15; }
      }
      int r = 0;
      if (!dry) {
        const double fl = 2.0 * g.M * (double)g.N * g.Ktot;
        e->prof_M = g.M; e->prof_N = g.N; e->prof_K = g.Ktot; e->prof_tag = (tag_base >= 0 ? tag_base : g.seg[0].mode * 100 + g.geglu * 10) + (sm_S > 1 ? sm_S : 0);
        r = profiled(MVD_PC_SM_64X64 + sm_tile, fl, 0.0, [&] { return mvd_launch_gemm_sm(g, s, sm_tile, sm_ns); });
      }
      e->tmp.off = mark;
      return r;
    }
    int S = 1, fc = -1;
    tiled_plan(g, S, fc);
    const size_t mark = e->tmp.off;
    if (S > 1) { g.splitk = S; g.part = talloc<float>((size_t)S * g.M * g.N); } else g.splitk = 1;   // (decided: 0 = undecided)
    static const bool trace = MVD_ENV_INT("MVD_TRACE_GEMM", 0) != 0;
    if (trace && !dry) fprintf(stderr, "gemm M=%d N=%d K=%d mode=%d nseg=%d geglu=%d cfg=%d splitk=%d\n", g.M, g.N, g.Ktot, g.seg[0].mode, g.nseg, g.geglu, mvd_gemm_pick_config(g), S);
    int r = 0;
    if (!dry) {
      const double fl = 2.0 * g.M * (double)g.N * g.Ktot;
      e->prof_M = g.M; e->prof_N = g.N; e->prof_K = g.Ktot; e->prof_tag = (tag_base >= 0 ? tag_base : g.seg[0].mode * 100 + g.geglu * 10) + (S > 1 ? S : 0);
      r = launch_tiled(g, s, fc, [&](auto&& launch) { return profiled(e->prof ? gemm_class(g, mvd_gemm_pick_config(g), S) : 0, fl, 0.0, launch); });
    }
    e->tmp.off = mark;
    return r;
  }

  // X-stationary form (gemm_xs.hip) of a K = 320 projection over many rows: taken when the packed twin `<slot>.wx`
  // (packing.pack_xs: weights in fragment order, bias -- or the LayerNorm-folded c2 -- inside) is registered.  Returns 1 when
  // it launched, 0 when the caller should go on with the general kernels, < 0 on error.  `n_full`: rows of the packed matrix
  // (a pass may use a prefix of them: the q/k/v rows without the adapter's q_ref).
  int try_xs(const bf16_t* x, int K, int M, const std::string& slot, int64_t n_full, int N, bool geglu, bool ln,
             const bf16_t* res, int ldres, void* out, int ldo, int set_override = -1) {
    if (err) return err;
    if (dry || (g_debug_flags & MVD_DBG_NO_XS) || K != 320 || slot.empty() || !has(slot, set_override)) return 0;
    MvdXsArgs a; memset(&a, 0, sizeof(a));
    a.x = x; a.ldx = K; a.M = M; a.K = K; a.units = N / 32; a.geglu = geglu; a.ln = ln; a.ln_eps = 1e-5f;
    a.res = res; a.ldres = ldres; a.out = (bf16_t*)out; a.ldo = ldo;
    if (N % 64 || !mvd_gemm_xs_applicable(a)) return 0;
    // two workgroups per CU or nothing: with fewer work items than ~1.75 per CU (N = 320 cannot be split into column parts: five
    // store groups) the ping-pong / lock-step tiles fill the chip better
    if ((long)((M + 255) / 256) * mvd_gemm_xs_pick_csplit(a) < 448) return 0;
    a.w = WB(slot, (n_full / 32) * 21 * 512, set_override);
    if (!a.w) return err;
    e->prof_M = M; e->prof_N = N; e->prof_K = K; e->prof_tag = geglu * 10 + (ln ? 1 : 0);
    const int r = profiled(geglu ? MVD_PC_XS_GEGLU : (res ? MVD_PC_XS_RESIDUAL : (ln ? MVD_PC_XS_LN_DENSE : MVD_PC_XS_DENSE)), 2.0 * M * (double)N * K, 0.0, [&] { return mvd_launch_gemm_xs(a, s); });
    return r ? r : 1;
  }

  // dense linear: out[M][N] = alpha*(A.W^T + bias) + res       (xs: slot name of the X-stationary twin, if the site has one)
  int linear(const bf16_t* a, const bf16_t* a2, int k1, int k2, int M, const bf16_t* w, const float* bias, int N,
             const bf16_t* res, int ldres, void* out, int ldo, bool geglu = false, bool out_f32 = false, int ldw = 0,
             const std::string& xs = std::string(), int xs_set = -1) {
    if (!xs.empty() && !a2 && !k2 && !geglu && !out_f32) {
      const int r = try_xs(a, k1, M, xs, N, N, false, false, res, ldres, out, ldo, xs_set);
      if (r) return r < 0 ? r : 0;
    }
    MvdGemmArgs g = gemm_dense(a, a2, k1, k2, M, w, ldw, bias, N, out, ldo);
    g.res = res; g.ldres = ldres; g.geglu = geglu; g.out_f32 = out_f32;
    return gemm(g);
  }

  // out = LayerNorm(x; gamma, beta).W^T + b (optionally GEGLU).  With the folded slots <slot>.wf (W.diag(gamma), bf16) and
  // <slot>.cf ([2][n_full]: c1 | c2) registered and a shape the fused kernel takes, ONE launch (gemm_pp.hip, LNF) that reads
  // the un-normalised rows; otherwise ln_kernel into `ln_tmp` and the plain GEMM.
  int ln_linear(const bf16_t* x, int M, int C, const std::string& ln_key, const std::string& slot, int64_t n_full, int N,
                const float* bias, bf16_t* ln_tmp, void* out, int ldo, bool geglu) {
    MvdGemmArgs g = gemm_dense(x, nullptr, C, 0, M, nullptr, 0, nullptr, N, out, ldo);    // (W and bias: below, per route)
    g.geglu = geglu;
    {
      const int r = try_xs(x, C, M, slot + ".wx", n_full, N, geglu, true, nullptr, 0, out, ldo);
      if (r) return r < 0 ? r : 0;
    }
    static const bool use_fold = MVD_ENV_INT("MVD_LN_FOLD", 1) != 0;
    auto sm_fold_ok = [&]() {      // the small-M kernels (batch 1) fold at every level
      MvdGemmArgs t = g;
      static const float dummy = 0.f;
      t.ln_c1 = &dummy; t.bias = &dummy; t.W = reinterpret_cast<const bf16_t*>(&dummy);
      int a_, b_, c_;
      return sm_enabled() && !(g_debug_flags & MVD_DBG_NO_SM_LN_FOLD) && mvd_gemm_sm_plan(t, &a_, &b_, &c_);
    };
    if (use_fold && !dry && has(slot + ".wf") && has(slot + ".cf") && (mvd_gemm_ln_fold_ok(g) || sm_fold_ok())) {
      const float* cf = WF(slot + ".cf", 2 * n_full);
      g.W = WB(slot + ".wf", n_full * C);
      g.ln_c1 = cf; g.bias = cf ? cf + n_full : nullptr; g.ln_eps = 1e-5f;
      return gemm(g);
    }
    CHECK(layernorm(x, M, C, WF(ln_key + ".g", C), WF(ln_key + ".b", C), ln_tmp));
    g.seg[0].p0 = ln_tmp; g.W = WB(slot + ".w", n_full * C); g.bias = bias;
    return gemm(g);
  }

  // Weight-streaming form (conv_ws.hip) of a stride-1 resnet convolution on one image's 8- or 16-wide map, taken when the packed
  // twin `<slot>.ws` (packing.pack_ws) is registered: batch 1 at the 8x8 / 16x16 / 32x32 levels is a weight stream, which the
  // implicit-GEMM kernels cut along K with a rendezvous between workgroups (21-63 us against 15-48 us, profiles/r04_probe_conv_ws.log).
  // Returns 1 when it launched, 0 when the caller should go on, < 0 on error.
  int try_ws(const Act& x, int ups, const std::string& slot, const float* bias, const float* rowvec, int ld_rowvec, const bf16_t* res,
             const bf16_t* sc0, const bf16_t* sc1, int scc0, int scc1, Act& out) {
    if (err) return err;
    if (dry || (g_debug_flags & MVD_DBG_NO_WS) || slot.empty() || !has(slot)) return 0;
    MvdWsArgs a; memset(&a, 0, sizeof(a));
    a.x = x.p; a.B = x.B; a.H = x.H; a.W = x.W; a.C = x.C; a.ups = ups; a.sc0 = sc0; a.sc1 = sc1; a.scc0 = scc0; a.scc1 = scc1;
    a.bias = bias; a.rowvec = rowvec; a.ld_rowvec = ld_rowvec; a.res = res; a.ldres = out.C; a.out = out.p; a.ldo = out.C;
    a.M = out.rows(); a.N = out.C;
    // (debug flags, A/B only; nowait = the encoder pass of a two-stream forward)
    if ((g_debug_flags & MVD_DBG_WS_SMALL_MAPS) && a.M > 256) return 0;
    if (g_debug_flags & MVD_DBG_WS_BLOCK64) a.variant = 1;
    if ((g_debug_flags & MVD_DBG_WS_NO_SHORTCUT) && scc0) return 0;
    if ((g_debug_flags & MVD_DBG_WS_NOT_IN_ENCODER) && nowait) return 0;
    if ((g_debug_flags & MVD_DBG_WS_ONLY_IN_ENCODER) && !nowait) return 0;
    if (out.H != (ups ? 2 : 1) * x.H || out.W != (ups ? 2 : 1) * x.W || out.B != x.B || a.M > 1024) return 0;
    // every 64-pixel row block streams its column tile's whole weight panel (from L2 at best): with 16 row blocks x 80 column tiles
    // (the 16 -> 32 upsampling convolution, N = 1280) that is a tie with the tiled kernel (62.9 vs 60.5 us) -- not taken
    if ((long)(a.M / 64) * (a.N / 16) > 1000) return 0;     // (one 32x32 map at most: beyond, the tiled kernels have the FLOPs to win)
    a.w = reinterpret_cast<const bf16_t*>(&a);                                     // (placeholder for the shape test)
    if (!mvd_conv_ws_applicable(a)) return 0;
    a.w = WB(slot, (int64_t)mvd_conv_ws_packed_elems(x.C, scc0 + scc1, out.C));
    if (!a.w) return err;
    e->prof_M = a.M; e->prof_N = a.N; e->prof_K = 9 * x.C + scc0 + scc1; e->prof_tag = 100 + (scc0 ? 1 : 0);
    const int r = profiled(MVD_PC_CONV_WS, 2.0 * a.M * (double)a.N * (9.0 * x.C + scc0 + scc1), 0.0, [&] { return mvd_launch_conv_ws(a, s); });
    if (!r && (g_debug_flags & MVD_DBG_WS_THEN_TILED)) return 0;   // (A/B only: the tiled kernel runs as well and overwrites the result)
#ifdef MVD_PROBE
    // probe builds, MVD_DBG_WS_CHECK: the tiled kernel computes the same launch into a scratch tensor and a compare kernel counts the
    // elements that differ by more than rounding into pinned host memory -- no synchronise; mvd_debug_ws_check_report() prints
    if (!r && (g_debug_flags & MVD_DBG_WS_CHECK)) {
      const size_t mark = e->tmp.off;
      Act chk = new_act(out.B, out.H, out.W, out.C, false);
      const bf16_t* wold = WB(slot.substr(0, slot.size() - 1), (int64_t)out.C * (9 * x.C + scc0 + scc1));   // "<..>.convN.ws" -> "<..>.convN.w"
      if (wold) {
        const int saved = g_debug_flags; g_debug_flags |= MVD_DBG_NO_WS;
        conv3(x, 1, ups, wold, bias, rowvec, ld_rowvec, res, sc0, sc1, scc0, scc1, chk);
        g_debug_flags = saved;
        g_ws_ptrs[0] = (const char*)x.p; g_ws_lens[0] = (size_t)x.rows() * x.C * 2;   // (input rows)
        g_ws_ptrs[1] = (const char*)sc0; g_ws_lens[1] = (size_t)out.rows() * scc0 * 2;
        g_ws_ptrs[2] = (const char*)sc1; g_ws_lens[2] = (size_t)out.rows() * scc1 * 2;
        g_ws_ptrs[3] = (const char*)out.p; g_ws_lens[3] = (size_t)out.rows() * out.C * 2;
        ws_check_launch(slot, set, nowait, out.p, chk.p, (long)out.rows() * out.C, s);
      }
      e->tmp.off = mark;
    }
#endif
    return r ? r : 1;
  }

  int conv3(const Act& x, int stride, int ups, const bf16_t* w, const float* bias, const float* rowvec, int ld_rowvec,
            const bf16_t* res, const bf16_t* sc0, const bf16_t* sc1, int scc0, int scc1, Act& out, const std::string& ws = std::string(),
            const std::string& w4 = std::string()) {
    if (!ws.empty() && stride == 1) {
      const int r = try_ws(x, ups, ws, bias, rowvec, ld_rowvec, res, sc0, sc1, scc0, scc1, out);
      if (r) return r < 0 ? r : 0;
    }
    MvdGemmArgs g = gemm_conv3(x.p, x.H, x.W, x.C, stride, ups, 0, sc0, sc1, scc0, scc1, w, bias, out.B, out.H, out.W, out.C, out.p);
    g.rowvec = rowvec; g.ld_rowvec = ld_rowvec; g.res = res;
    // Upsampling convolution as four 2x2 sub-pixel convolutions of the source map (gemm_pp.hip AMODE 4: K = 4 C instead of 9 C,
    // the same result up to one bf16 rounding of the pre-summed weights), taken when the packed twin `w4` (packing.pack_up4) is
    // registered and the schedule would put the nine-tap problem on the unsplit 256x320 ping-pong tile anyway: batch-1 forwards
    // keep their conv_ws / small-M route, a split launch (the 8x8 -> 16x16 site outside a two-stream forward) and source widths
    // the mode does not take (12, 24) keep the nine-tap kernel.  MVD_DBG_NO_UP4 turns the route off (A/B).
    if (!w4.empty() && !dry && !err && ups == 1 && stride == 1 && !sc0 && !res && !rowvec && !(g_debug_flags & MVD_DBG_NO_UP4) && has(w4)) {
      int t_ = 0, n_ = 0, s_ = 1, S = 1, fc = -1;
      if (!(sm_enabled() && mvd_gemm_sm_plan(g, &t_, &n_, &s_))) {
        tiled_plan(g, S, fc);
        MvdGemmArgs u = g;
        u.splitk = 1;
        if (S == 1 && (fc >= 0 ? fc : mvd_gemm_pick_config(u)) == 7 && mvd_gemm_pp_applicable(u)) {
          gemm_conv3_to_up4(u);
          if (mvd_gemm_pp_up4_applicable(u)) {
            u.W = WB(w4, (int64_t)4 * out.C * 4 * x.C);
            if (!u.W) return err;
            // (executed FLOPs: 4/9 of the algorithmic count of the nine-tap form; tag 140 tells the rows apart in the shape table)
            e->prof_M = u.M; e->prof_N = u.N; e->prof_K = u.Ktot; e->prof_tag = 140;
            return profiled(MVD_PC_PP_CONV3, 2.0 * u.M * (double)u.N * u.Ktot, 0.0, [&] { return mvd_launch_gemm(u, s, 7); });
          }
        }
      }
    }
    return gemm(g);
  }

  int groupnorm(const bf16_t* x0, const bf16_t* x1, int c0, int c1, int B, int hw, float eps, const float* g, const float* b,
                int silu, bf16_t* y) {
    if (err) return err;
    const int groups = e->cfg.norm_num_groups;
    float* ws = talloc<float>((size_t)B * MVD_GN_MAXCHUNK * groups * 2);
    if (dry) return 0;
    const double by = 3.0 * B * (double)hw * (c0 + c1) * 2;   // 2 reads + 1 write of the activation
    e->prof_M = B * hw; e->prof_N = c0 + c1; e->prof_K = 0; e->prof_tag = 2000 + silu;
    return profiled(MVD_PC_GROUPNORM, 0.0, by, [&] { return mvd_launch_groupnorm(x0, x1, c0, c1, B, hw, groups, eps, g, b, silu, y, ws, s); });
  }
  int layernorm(const bf16_t* x, int rows, int c, const float* g, const float* b, bf16_t* y) {
    if (err) return err; if (dry) return 0;
    e->prof_M = rows; e->prof_N = c; e->prof_K = 0; e->prof_tag = 3000;
    return profiled(MVD_PC_LAYERNORM, 0.0, 2.0 * rows * (double)c * 2, [&] { return mvd_launch_layernorm(x, rows, c, 1e-5f, g, b, y, s); });
  }
  int attention(MvdAttnArgs& a) {
    if (err) return err;
    // batch 1: split the keys over several workgroups (partials + counters from the scoped workspace / the call's counter block)
    const size_t mark = e->tmp.off;
    const int ns = (g_debug_flags & MVD_DBG_NO_SPLIT_KV) ? 1 : mvd_attention_pick_split(a);
    if (ns > 1) {
      a.nsplit = ns;
      a.split_ws = e->tmp.alloc(mvd_attention_split_ws_bytes(a, ns));
      a.split_cnt = e->cnt_base + e->cnt_used;
      e->cnt_used += mvd_attention_split_counters(a);
      if (!dry && e->cnt_used > e->cnt_cap) { mvd_set_error("forward: tile counters exhausted (%d > %d)", e->cnt_used, e->cnt_cap); return err = -15; }
    }
    e->tmp.off = mark;
    if (dry) return 0;
    double fl = 0;
    for (int i = 0; i < a.nprob; ++i) fl += 4.0 * a.batch * a.heads * (double)a.p[i].nq * a.p[i].nk * 64;
    e->prof_M = a.p[0].nq; e->prof_N = a.p[0].nk; e->prof_K = a.heads; e->prof_tag = 1000 + a.nprob;
    return profiled(MVD_PC_ATTN_1WAVE + (e->prof ? mvd_attention_pick_nw(a) : 0), fl, 0.0, [&] { return mvd_launch_attention(a, s); });
  }
};

// ---------------------------------------------------------------------- structure helpers
struct ResnetDesc { std::string key; int cin0, cin1, cout; };

std::vector<ResnetDesc> enumerate_resnets(const mvd_config_t& c) {
  std::vector<ResnetDesc> v;
  const int n = c.num_levels, L = c.layers_per_block;
  int prev = c.block_out_channels[0];
  for (int i = 0; i < n; ++i) {
    const int co = c.block_out_channels[i];
    for (int j = 0; j < L; ++j) v.push_back({"down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), j == 0 ? prev : co, 0, co});
    prev = co;
  }
  const int cm = c.block_out_channels[n - 1];
  v.push_back({"mid_block.resnets.0", cm, 0, cm});
  v.push_back({"mid_block.resnets.1", cm, 0, cm});
  int prev_out = cm;
  for (int i = 0; i < n; ++i) {
    const int out_c = c.block_out_channels[n - 1 - i];
    const int in_c = c.block_out_channels[n - 1 - (i + 1 < n ? i + 1 : n - 1)];
    for (int j = 0; j <= L; ++j) {
      const int skip = (j == L) ? in_c : out_c;
      const int hid = (j == 0) ? prev_out : out_c;
      v.push_back({"up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), hid, skip, out_c});
    }
    prev_out = out_c;
  }
  return v;
}

std::vector<FeatureInfo> enumerate_features(const mvd_config_t& c) {
  std::vector<FeatureInfo> f;
  const int n = c.num_levels, L = c.layers_per_block;
  for (int i = 0; i + 1 < n; ++i)
    for (int j = 0; j < L; ++j) f.push_back({"down_block_" + std::to_string(i) + "_attn_" + std::to_string(j), i, c.block_out_channels[i], c.num_heads[i],
                   "down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j)});
  f.push_back({"mid_block_attn_0", n - 1, c.block_out_channels[n - 1], c.num_heads[n - 1], "mid_block.attentions.0"});
  for (int i = 1; i < n; ++i)
    for (int j = 0; j <= L; ++j) f.push_back({"up_block_" + std::to_string(i) + "_attn_" + std::to_string(j), n - 1 - i, c.block_out_channels[n - 1 - i], c.num_heads[n - 1 - i],
                   "up_blocks." + std::to_string(i) + ".attentions." + std::to_string(j)});
  return f;
}

struct PassOpts {
  bool adapter = false;       // add the cross-view attention branch (needs e->refkv)
  bool film = false;          // apply camera FiLM hooks
  bool capture = false;       // encoder pass: produce reference K/V (+ keep features)
  bool defer_norm = false;    // capture, global-statistics form: per-pixel local (mean, M2) go to `stats`, the features are
  float* stats = nullptr;     // kept raw and normalisation + K/V projection wait for mvd_engine_reference_finish
  int ref_batch = 0;          // batch of the reference features (Q4 re-chunking)
  const ViewLayout* layout = nullptr;   // the forward's batch layout (ragged.h): the adapter pass's K/V maps, the encoder pass's statistics
  const MainOpts* main = nullptr;   // the main pass: the engine's options; null for the encoder pass, which none of them touches
  int deep = 0;               // main pass, DeepCache: MVD_DEEPCACHE_REFRESH (store the deep feature) / _SHALLOW (start from it); 0: neither
  bf16_t* deep_buf = nullptr; // the bound buffer: [B][H0][W0][C of the deep feature]
  int late_from = 99;         // main pass of a two-stream forward: up-block index from which it takes the single-stream launch policy (99: never)
  const std::unordered_map<std::string, std::pair<float*, float*>>* film_ss = nullptr;  // name -> (scale, shift) [B][dim]
};

// ---------------------------------------------------------------------- one UNet pass
struct UNetPass {
  Ctx& c;
  const mvd_config_t& cfg;
  PassOpts o;
  int B, H0, W0, L;
  const bf16_t* text;      // [B*L][xdim] bf16
  const float* tproj;      // [B][temb_total] fp32 (all time_emb_proj outputs incl. bias)
  bf16_t* tkv = nullptr;   // [B*L][tkv_total] bf16: text K/V of every attn2 site (one GEMM per pass)
  int resnet_idx = 0;
  int feat_idx = 0;
  int text_rows = 0;       // rows of `text` when they are fewer than B (MVD_SHARE_REF: one per guidance half); 0: B

  int resnet(const std::string& key, const Act& x0, const Act* x1, int cout, Act& out) {
    const int cin0 = x0.C, cin1 = x1 ? x1->C : 0, cin = cin0 + cin1;
    const int B_ = x0.B, hw = x0.hw();
    const size_t mark = c.e->tmp.off;
    Act t1 = c.new_act(B_, x0.H, x0.W, cin, false);
    CHECK(c.groupnorm(x0.p, x1 ? x1->p : nullptr, cin0, cin1, B_, hw, cfg.norm_eps, c.WF(key + ".norm1.g", cin), c.WF(key + ".norm1.b", cin), 1, t1.p));
    Act h1 = c.new_act(B_, x0.H, x0.W, cout, false);
    const int toff = c.e->temb_off[resnet_idx++];
    CHECK(c.conv3(t1, 1, 0, c.WB(key + ".conv1.w", (int64_t)cout * 9 * cin), c.WF(key + ".conv1.b", cout), tproj + toff, c.e->temb_total,
                  nullptr, nullptr, nullptr, 0, 0, h1, key + ".conv1.ws"));
    Act t2 = c.new_act(B_, x0.H, x0.W, cout, false);
    CHECK(c.groupnorm(h1.p, nullptr, cout, 0, B_, hw, cfg.norm_eps, c.WF(key + ".norm2.g", cout), c.WF(key + ".norm2.b", cout), 1, t2.p));
    if (cin != cout) {
      CHECK(c.conv3(t2, 1, 0, c.WB(key + ".conv2.w", (int64_t)cout * (9 * cout + cin)), c.WF(key + ".conv2.b", cout), nullptr, 0, nullptr,
                    x0.p, x1 ? x1->p : nullptr, cin0, cin1, out, key + ".conv2.ws"));
    } else {
      CHECK(c.conv3(t2, 1, 0, c.WB(key + ".conv2.w", (int64_t)cout * 9 * cout), c.WF(key + ".conv2.b", cout), nullptr, 0, x0.p, nullptr,
                    nullptr, 0, 0, out, key + ".conv2.ws"));
    }
    c.e->tmp.off = mark;
    return c.err;
  }

  int transformer(const std::string& key, const Act& x, int heads, Act& out) {
    const int C = x.C, M = x.rows(), hw = x.hw(), B_ = x.B;
    const bool ad = o.adapter;
    // set 0 may carry the adapter rows/columns even when this pass does not use them (no image conditioning):
    // q/k/v rows are a prefix of the fused matrix, the out-projection is addressed with its packed row stride.
    const bool packed = c.set == 0 && (c.dry || c.has(key + ".ref_kv.w", 0));
    if (ad && !packed) { mvd_set_error("adapter requested but no adapter weights registered for %s", key.c_str()); return -14; }
    const int ld_out = packed ? 2 * C : C;
    const char* bias_slot = (packed && !ad) ? ".out.b0" : ".out.b";
    const size_t mark = c.e->tmp.off;
    bf16_t* n0 = c.talloc<bf16_t>((size_t)M * C);
    CHECK(c.groupnorm(x.p, nullptr, C, 0, B_, hw, 1e-6f, c.WF(key + ".norm.g", C), c.WF(key + ".norm.b", C), 0, n0));
    bf16_t* h = c.talloc<bf16_t>((size_t)M * C);
    CHECK(c.linear(n0, nullptr, C, 0, M, c.WB(key + ".proj_in.w", (int64_t)C * C), c.WF(key + ".proj_in.b", C), C, nullptr, 0, h, C, false, false, 0, key + ".proj_in.wx"));
    bf16_t* ln = n0;  // reuse
    const float scale = 0.125f;   // (folded, with log2 e, into the packed to_q / to_q_ref rows: a.prescaled)
    bf16_t* o_self = c.talloc<bf16_t>((size_t)M * C);
    bf16_t* o_ref = ad ? c.talloc<bf16_t>((size_t)M * C) : nullptr;
    const bf16_t* rkv = ad ? c.e->refkv[feat_idx] : nullptr;
    // Q4: K/V rows of the reference are re-chunked by the HIDDEN batch size (a shared forward: by the batch g of ONE view's call --
    // the views of a guidance half share that half's chunk; objects: each object's hw tokens, K/V elements [object][half])
    const int Bq = ad ? o.layout->text_rows(B_) : B_;
    const int ref_nk = ad ? (int)((int64_t)o.ref_batch * hw / Bq) : 0;
    if (ad && (int64_t)ref_nk * Bq != (int64_t)o.ref_batch * hw) { mvd_set_error("adapter: ref tokens %d x %d not divisible by batch %d", o.ref_batch, hw, Bq); return -12; }

    // (dual-stream forwards: this feature's adapter K/V come from the encoder pass on the side stream)
    if (ad && c.e->dual_now && !c.dry && !c.err && hipStreamWaitEvent(c.s, c.e->feat_ev[feat_idx], 0) != hipSuccess) { mvd_set_error("forward: hipStreamWaitEvent failed"); return -3; }
    // ---- attn1 (self) + adapter branch "<feature>_self"
    const int tome_r = tome_merged(x.H, x.W);
    if (tome_r > 0) {
      // token merging (include/mvd_hip.h mvd_engine_set_tome): attn1 on the N' = hw - r merged rows of every image
      if (hw > MVD_TOME_MAX_TOKENS || (C & 63)) { mvd_set_error("forward: token merging in %s: a %d x %d map of %d channels (the select kernel takes at most %d tokens, channels in multiples of 64)", key.c_str(), x.H, x.W, C, MVD_TOME_MAX_TOKENS); return c.err = -1; }
      const int Nm = hw - tome_r, Mm = B_ * Nm;
      const int nq = ad ? 4 * C : 3 * C;
      CHECK(c.layernorm(h, M, C, c.WF(key + ".ln1.g", C), c.WF(key + ".ln1.b", C), ln));
      int* slot = o.main->tome_keep ? c.aalloc<int>((size_t)M) : c.talloc<int>((size_t)M);
      int* members = c.talloc<int>((size_t)M);
      int* starts = c.talloc<int>((size_t)B_ * (Nm + 1));
      const int64_t wsb = mvd_tome_workspace_bytes(B_, x.H, x.W);
      void* tws = c.e->tmp.alloc((size_t)wsb);
      bf16_t* lnm = c.talloc<bf16_t>((size_t)Mm * C);      // the merged rows; after the q/k/v GEMM, the out-projection's result
      bf16_t* qkv = c.talloc<bf16_t>((size_t)Mm * nq);
      if (!c.dry && !c.err) {
        if (o.main->tome_keep && feat_idx < (int)c.e->tome_tab.size()) c.e->tome_tab[feat_idx] = {slot, (int64_t)M};
        CHECK(mvd_launch_tome_match(ln, B_, x.H, x.W, C, tome_r, slot, members, starts, nullptr, nullptr, tws, wsb, c.s));
        CHECK(mvd_launch_tome_merge(ln, B_, x.H, x.W, C, tome_r, members, starts, lnm, c.s));
      }
      CHECK(c.linear(lnm, nullptr, C, 0, Mm, c.WB(key + ".attn1.qkv.w", (int64_t)(packed ? 4 : 3) * C * C), nullptr, nq, nullptr, 0, qkv, nq));
      MvdAttnArgs a; memset(&a, 0, sizeof(a));
      a.batch = B_; a.heads = heads; a.scale = scale; a.prescaled = 1; a.nprob = ad ? 2 : 1;
      a.p[0] = {qkv, qkv + C, qkv + 2 * C, o_self, nq, nq, nq, C, (int64_t)Nm * nq, (int64_t)Nm * nq, (int64_t)Nm * nq, (int64_t)Nm * C, Nm, Nm};
      if (ad) a.p[1] = {qkv + 3 * C, rkv, rkv + C, o_ref, nq, 4 * C, 4 * C, C, (int64_t)Nm * nq, (int64_t)ref_nk * 4 * C, (int64_t)ref_nk * 4 * C, (int64_t)Nm * C, Nm, ref_nk};
      if (ad) o.layout->fill_map(true, &a.kv_group[1], &a.kv_objects[1], &a.kv_index[1]);
      CHECK(c.attention(a));
      CHECK(c.linear(o_self, o_ref, C, ad ? C : 0, Mm, c.WB(key + ".attn1.out.w", (int64_t)C * ld_out), c.WF(key + ".attn1" + bias_slot, C), C, nullptr, 0, lnm, C, false, false, ld_out,
                     ad ? std::string() : key + ".attn1.out.wx"));
      if (!c.dry && !c.err) CHECK(mvd_launch_tome_unmerge_add(h, lnm, B_, x.H, x.W, C, tome_r, slot, c.s));
    } else {
      const int nq = ad ? 4 * C : 3 * C;
      bf16_t* qkv = c.talloc<bf16_t>((size_t)M * nq);
      CHECK(c.ln_linear(h, M, C, key + ".ln1", key + ".attn1.qkv", (int64_t)(packed ? 4 : 3) * C, nq, nullptr, ln, qkv, nq, false));
      MvdAttnArgs a; memset(&a, 0, sizeof(a));
      a.batch = B_; a.heads = heads; a.scale = scale; a.prescaled = 1; a.nprob = ad ? 2 : 1;
      a.p[0] = {qkv, qkv + C, qkv + 2 * C, o_self, nq, nq, nq, C, (int64_t)hw * nq, (int64_t)hw * nq, (int64_t)hw * nq, (int64_t)hw * C, hw, hw};
      const int todo_f = todo_factor(x.H, x.W);
      if (todo_f > 1) {
        // token downsampling (include/mvd_hip.h mvd_engine_set_todo): the self problem's keys and values from the pooled K/V rows;
        // the queries, the adapter's problem and the out-projection are untouched
        const int Nk = (x.H / todo_f) * (x.W / todo_f);
        bf16_t* kv = c.talloc<bf16_t>((size_t)B_ * Nk * 2 * C);
        if (!c.dry && !c.err) {
          if (feat_idx < (int)c.e->todo_nk.size()) c.e->todo_nk[feat_idx] = Nk;
          CHECK(mvd_launch_todo_downsample(qkv + C, qkv + 2 * C, nq, B_, x.H, x.W, C, todo_f, o.main->todo_method, kv, c.s));
        }
        a.p[0].k = kv; a.p[0].v = kv + C; a.p[0].ldk = a.p[0].ldv = 2 * C; a.p[0].bsk = a.p[0].bsv = (int64_t)Nk * 2 * C; a.p[0].nk = Nk;
      }
      if (ad) a.p[1] = {qkv + 3 * C, rkv, rkv + C, o_ref, nq, 4 * C, 4 * C, C, (int64_t)hw * nq, (int64_t)ref_nk * 4 * C, (int64_t)ref_nk * 4 * C, (int64_t)hw * C, hw, ref_nk};
      if (ad) o.layout->fill_map(true, &a.kv_group[1], &a.kv_objects[1], &a.kv_index[1]);
      CHECK(c.attention(a));
      CHECK(c.linear(o_self, o_ref, C, ad ? C : 0, M, c.WB(key + ".attn1.out.w", (int64_t)C * ld_out), c.WF(key + ".attn1" + bias_slot, C), C, h, C, h, C, false, false, ld_out,
                     ad ? std::string() : key + ".attn1.out.wx"));
    }
    // ---- attn2 (text cross) + adapter branch "<feature>_cross"
    {
      const int nq = ad ? 2 * C : C;
      bf16_t* q2 = c.talloc<bf16_t>((size_t)M * nq);
      const bf16_t* kv2 = tkv + c.e->tkv_off[feat_idx];   // [B*L][2C] slice of the fused text K/V ([text_rows*L] in a shared forward)
      const int ldkv = c.e->tkv_total;
      CHECK(c.ln_linear(h, M, C, key + ".ln2", key + ".attn2.q", (int64_t)(packed ? 2 : 1) * C, nq, nullptr, ln, q2, nq, false));
      MvdAttnArgs a; memset(&a, 0, sizeof(a));
      a.batch = B_; a.heads = heads; a.scale = scale; a.prescaled = 1; a.nprob = ad ? 2 : 1;
      a.p[0] = {q2, kv2, kv2 + C, o_self, nq, ldkv, ldkv, C, (int64_t)hw * nq, (int64_t)L * ldkv, (int64_t)L * ldkv, (int64_t)hw * C, hw, L};
      if (ad) a.p[1] = {q2 + C, rkv + 2 * C, rkv + 3 * C, o_ref, nq, 4 * C, 4 * C, C, (int64_t)hw * nq, (int64_t)ref_nk * 4 * C, (int64_t)ref_nk * 4 * C, (int64_t)hw * C, hw, ref_nk};
      if (ad) o.layout->fill_map(false, &a.kv_group[0], &a.kv_objects[0], &a.kv_index[0]);     // (the text K/V: one row per half and object)
      if (ad) o.layout->fill_map(true, &a.kv_group[1], &a.kv_objects[1], &a.kv_index[1]);
      CHECK(c.attention(a));
      CHECK(c.linear(o_self, o_ref, C, ad ? C : 0, M, c.WB(key + ".attn2.out.w", (int64_t)C * ld_out), c.WF(key + ".attn2" + bias_slot, C), C, h, C, h, C, false, false, ld_out,
                     ad ? std::string() : key + ".attn2.out.wx"));
    }
    // ---- GEGLU feed-forward
    {
      bf16_t* ff = c.talloc<bf16_t>((size_t)M * 4 * C);
      CHECK(c.ln_linear(h, M, C, key + ".ln3", key + ".ff1", (int64_t)8 * C, 8 * C, c.WF(key + ".ff1.b", 8 * C), ln, ff, 4 * C, true));
      // Tail of the block.  h = h + ff.W2^T + b2 and out = x + h.Wp^T + bp have nothing non-linear between them and h dies here, so
      // with the composed slot `<key>.tail.w` = [Wp.W2 | Wp] registered (packing.fold_tail; bias Wp.b2 + bp) both are ONE GEMM over
      // the two sources [ff | h], K = 4C + C -- the form of the attention out-projections.  Without the slot: the two launches.
      // (a sizing run reads the same weight table as the run it sizes and takes the same branch; one that comes before any weight
      //  is registered -- mvd_engine_workspace_bytes on a fresh engine -- sizes BOTH forms: their split-K partials may differ)
      const bool tail = c.has(key + ".tail.w");
      if (tail || c.dry) {
        c.tag_base = 50;      // (shape table: 50 + split, next to no other dense launch's tag)
        const int r = c.linear(ff, h, 4 * C, C, M, c.WB(key + ".tail.w", (int64_t)C * 5 * C), c.WF(key + ".tail.b", C), C, x.p, C, out.p, C);
        c.tag_base = -1;
        CHECK(r);
      }
      if (!tail) {
        CHECK(c.linear(ff, nullptr, 4 * C, 0, M, c.WB(key + ".ff2.w", (int64_t)C * 4 * C), c.WF(key + ".ff2.b", C), C, h, C, h, C));
        CHECK(c.linear(h, nullptr, C, 0, M, c.WB(key + ".proj_out.w", (int64_t)C * C), c.WF(key + ".proj_out.b", C), C, x.p, C, out.p, C, false, false, 0, key + ".proj_out.wx"));
      }
    }
    c.e->tmp.off = mark;

    if (o.capture) {  // encoder pass: reference normalisation (Q2) + adapter K/V for both processors of this feature
      const size_t mk = c.e->tmp.off;
      bf16_t* rn = c.talloc<bf16_t>((size_t)M * C);        // (also sized in the deferred form: _finish needs the same scratch)
      if (o.defer_norm) {
        if (!c.dry && !c.err) CHECK(mvd_launch_refstats(out.p, B_, hw, C, o.stats + 2 * c.e->feat_pixel_off(feat_idx), c.s));
      } else {
        if (!c.dry && !c.err) CHECK(o.layout->per_object_stats() ? mvd_launch_refnorm_grouped(out.p, B_, 1, hw, C, rn, c.s) : mvd_launch_refnorm(out.p, B_, hw, C, rn, c.s));
        CHECK(c.linear(rn, nullptr, C, 0, M, c.WB(key + ".ref_kv.w", (int64_t)4 * C * C, 0), nullptr, 4 * C, nullptr, 0, c.e->refkv[feat_idx], 4 * C, false, false, 0,
                       key + ".ref_kv.wx", 0));
        if (c.e->dual_now && !c.dry && !c.err && hipEventRecord(c.e->feat_ev[feat_idx], c.s) != hipSuccess) { mvd_set_error("forward: hipEventRecord failed"); return -3; }
      }
      if (c.e->rc_keep && !c.dry && !c.err)
        CHECK((int)hipMemcpyAsync(c.e->feat_keep[feat_idx], out.p, (size_t)M * C * sizeof(bf16_t), hipMemcpyDeviceToDevice, c.s));
      c.e->tmp.off = mk;
    }
    ++feat_idx;
    return c.err;
  }

  // how many times coarser than the latent a block's H x W map is: ceil(sqrt(N0 / N)) (tomesd's `down`)
  long down_of(int H, int W) const {
    const long q = ((long)H0 * W0) / ((long)H * W);
    long down = 0;
    while (down * down < q) ++down;
    return down;
  }

  // merged src per image of a block whose map is H x W; 0: the block does not merge (tomesd: `down <= max_downsample`, r = int(N ratio))
  int tome_merged(int H, int W) const {
    if (!o.main || !o.main->merges() || H < 2 || W < 2 || down_of(H, W) > o.main->tome_maxds) return 0;
    const int ns = H * W - (H / 2) * (W / 2);
    const int r = (int)((double)(H * W) * o.main->tome_ratio);
    return r < ns ? r : ns;
  }

  // the K/V factor of a block whose map is H x W; 1: attn1 reads its own K/V rows (deeper than down 2: never)
  int todo_factor(int H, int W) const {
    if (!o.main || !o.main->downsamples()) return 1;
    const long down = down_of(H, W);
    if (down < 1 || down > 2) return 1;
    const int f = o.main->todo_f[down - 1];
    return (f > 1 && H / f >= 1 && W / f >= 1) ? f : 1;
  }

  int film(const std::string& name, const Act& x, Act& out) {
    auto it = o.film_ss->find(name);
    if (it == o.film_ss->end()) { out = x; return 0; }   // unknown modulator ("mid_0") -> identity (Q3)
    if (c.dry || c.err) return c.err;
    return mvd_launch_film(x.p, x.B, x.hw(), x.C, it->second.first, it->second.second, x.C, out.p, c.s);
  }

  // main-pass taps (mvd_engine::taps): the record of a block output; nothing is launched
  bool tapping() const { return o.main && o.main->taps_on; }
  void tap(const std::string& name, const Act& a) {
    if (tapping() && !c.dry && !c.err) c.e->taps.push_back({name, a.p, a.B, a.H, a.W, a.C});
  }
  // a FiLM hook of the mid / up blocks, which modulates h in place -- with taps on into a tensor of its own (the same launch, the
  // same values), so that the block output in front of it stays readable
  int film_hook(const std::string& name, Act& h) {
    Act res = h;
    const bool known = o.film_ss->find(name) != o.film_ss->end();
    if (known && tapping()) res = c.new_act(h.B, h.H, h.W, h.C, true);
    CHECK(film(name, h, res));
    h = res;
    if (known) tap("film." + name, h);
    return c.err;
  }

  // positions of a layer in the FULL schedule (the order of enumerate_resnets / enumerate_features): what temb_off, tkv_off, refkv
  // and feat_ev are indexed by.  run() SETS resnet_idx / feat_idx from these in front of every layer it executes -- a shallow
  // (DeepCache) pass skips layers, and a count from 0 would hand its up block the down blocks' slices.
  int down_resnet_pos(int i, int j) const { return i * cfg.layers_per_block + j; }
  int mid_resnet_pos(int j) const { return cfg.num_levels * cfg.layers_per_block + j; }
  int up_resnet_pos(int i, int j) const { return cfg.num_levels * cfg.layers_per_block + 2 + i * (cfg.layers_per_block + 1) + j; }
  int down_feat_pos(int i, int j) const { return i * cfg.layers_per_block + j; }
  int mid_feat_pos() const { return (cfg.num_levels - 1) * cfg.layers_per_block; }
  int up_feat_pos(int i, int j) const { return (cfg.num_levels - 1) * cfg.layers_per_block + 1 + (i - 1) * (cfg.layers_per_block + 1) + j; }

  int run(const Act& x_in, float* out_nchw) {
    const int n = cfg.num_levels, Lb = cfg.layers_per_block;
    const int C0 = cfg.block_out_channels[0];
    // DeepCache (include/mvd_hip.h): `shallow` runs down_blocks.0 layers 0..b and up_blocks.{n-1} layers j0..Lb around the stored
    // deep feature; `refresh` is the full pass, which copies that feature out where the shallow pass will put it in
    const bool shallow = o.deep == MVD_DEEPCACHE_SHALLOW, refresh = o.deep == MVD_DEEPCACHE_REFRESH;
    const int branch = o.main ? o.main->dc_branch : 0, j0 = Lb - 1 - branch;   // (o.deep is set on the main pass only)
    std::vector<Act> skips;
    // text K/V for all attn2 sites of this pass: one [B*L][xdim] x [tkv_total][xdim]^T GEMM instead of 16 small ones
    // (a shallow pass computes all of it as well: the GEMM is small, and the executed sites read the slices of their full-schedule
    //  positions from a buffer laid out as ever)
    const int TB = text_rows > 0 ? text_rows : B;
    tkv = c.aalloc<bf16_t>((size_t)TB * L * c.e->tkv_total);
    CHECK(c.linear(text, nullptr, cfg.cross_attention_dim, 0, TB * L, c.WB("text_kv.w", (int64_t)c.e->tkv_total * cfg.cross_attention_dim), nullptr,
                   c.e->tkv_total, nullptr, 0, tkv, c.e->tkv_total));
    Act h = c.new_act(B, H0, W0, C0, true);
    // conv_in: x_in holds im2col rows [B*H*W][64] (k = tap*Cin + ch, zero padded) -> one K=64 MFMA GEMM
    CHECK(c.linear(x_in.p, nullptr, 64, 0, B * H0 * W0, c.WB("conv_in.w", (int64_t)C0 * 64), c.WF("conv_in.b", C0), C0, nullptr, 0, h.p, C0));
    tap("conv_in", h);
    skips.push_back(h);
    for (int i = 0; i < (shallow ? 1 : n); ++i) {
      const int co = cfg.block_out_channels[i];
      const std::string bk = "down_blocks." + std::to_string(i);
      for (int j = 0; j < (shallow ? branch + 1 : Lb); ++j) {
        Act r = c.new_act(B, h.H, h.W, co, true);
        resnet_idx = down_resnet_pos(i, j);
        CHECK(resnet(bk + ".resnets." + std::to_string(j), h, nullptr, co, r));
        h = r;
        tap(bk + ".resnets." + std::to_string(j), h);
        if (i + 1 < n) {
          Act t = c.new_act(B, h.H, h.W, co, true);
          feat_idx = down_feat_pos(i, j);
          CHECK(transformer(bk + ".attentions." + std::to_string(j), h, cfg.num_heads[i], t));
          h = t;
          tap(bk + ".attentions." + std::to_string(j), h);
        }
        skips.push_back(h);
      }
      if (shallow) break;     // (no downsampler, no down_0 hook: the hook modulates what goes DOWN, which a shallow pass never reads)
      if (i + 1 < n) {
        Act d = c.new_act(B, (h.H + 1) / 2, (h.W + 1) / 2, co, true);
        CHECK(c.conv3(h, 2, 0, c.WB(bk + ".down.w", (int64_t)co * 9 * co), c.WF(bk + ".down.b", co), nullptr, 0, nullptr, nullptr, nullptr, 0, 0, d));
        h = d;
        tap(bk + ".downsamplers.0", h);
        skips.push_back(h);
      }
      if (o.film) {  // hook modulates the block's returned hidden_states only; skips stay unmodulated (Q6)
        Act m = c.new_act(B, h.H, h.W, h.C, true);
        Act res = m;
        CHECK(film("down_" + std::to_string(i), h, res));
        h = res;
        tap("film.down_" + std::to_string(i), h);
      }
    }
    if (!shallow) {
      const int cm = cfg.block_out_channels[n - 1];
      Act r = c.new_act(B, h.H, h.W, cm, true);
      resnet_idx = mid_resnet_pos(0);
      CHECK(resnet("mid_block.resnets.0", h, nullptr, cm, r));
      tap("mid_block.resnets.0", r);
      Act t = c.new_act(B, h.H, h.W, cm, true);
      feat_idx = mid_feat_pos();
      CHECK(transformer("mid_block.attentions.0", r, cfg.num_heads[n - 1], t));
      tap("mid_block.attentions.0", t);
      Act r2 = c.new_act(B, h.H, h.W, cm, true);
      resnet_idx = mid_resnet_pos(1);
      CHECK(resnet("mid_block.resnets.1", t, nullptr, cm, r2));
      h = r2;
      tap("mid_block.resnets.1", h);
      if (o.film) CHECK(film_hook("mid_0", h));
    } else {
      // the stored deep feature, read where it lies (nothing below writes its hidden input: the resnet and FreeU only read it)
      h = Act{o.deep_buf, B, H0, W0, c.e->dc_hidden_channels()};
    }
    for (int i = shallow ? n - 1 : 0; i < n; ++i) {
      const int co = cfg.block_out_channels[n - 1 - i];
      const std::string bk = "up_blocks." + std::to_string(i);
      // main pass of a two-stream forward: from up block `late_from` on the encoder pass (41 % of the work, ahead by design
      // and on the higher-priority stream) has normally drained -- launches must fill the chip by themselves again
      if (!o.capture && i >= o.late_from) c.e->dual_late = true;
      for (int j = (shallow ? j0 : 0); j <= Lb; ++j) {
        Act skip = skips.back(); skips.pop_back();
        if (skip.H != h.H || skip.W != h.W) { mvd_set_error("up block %d: skip %dx%d vs hidden %dx%d (odd latent size unsupported)", i, skip.H, skip.W, h.H, h.W); return -13; }
        if (refresh && i == n - 1 && j == j0 && !c.dry && !c.err)
          CHECK((int)hipMemcpyAsync(o.deep_buf, h.p, (size_t)h.rows() * h.C * sizeof(bf16_t), hipMemcpyDeviceToDevice, c.s));
        Act r = c.new_act(B, h.H, h.W, co, true);
        resnet_idx = up_resnet_pos(i, j);
        if (o.main && o.main->freeu_on && i < 2) {
          // FreeU: the resnet (GroupNorm and the folded 1x1 shortcut alike) reads the re-weighted pair; h and skip stay as they were
          const size_t fm = c.e->tmp.off;
          Act hf = c.new_act(B, h.H, h.W, h.C, false), sf = c.new_act(B, skip.H, skip.W, skip.C, false);
          if (!c.dry && !c.err) CHECK(mvd_launch_freeu(h.p, h.C, skip.p, skip.C, B, h.H, h.W, o.main->freeu_b[i], o.main->freeu_s[i], hf.p, sf.p, c.s));
          CHECK(resnet(bk + ".resnets." + std::to_string(j), hf, &sf, co, r));
          c.e->tmp.off = fm;
        } else {
          CHECK(resnet(bk + ".resnets." + std::to_string(j), h, &skip, co, r));
        }
        h = r;
        tap(bk + ".resnets." + std::to_string(j), h);
        if (i > 0) {
          Act t = c.new_act(B, h.H, h.W, co, true);
          feat_idx = up_feat_pos(i, j);
          CHECK(transformer(bk + ".attentions." + std::to_string(j), h, cfg.num_heads[n - 1 - i], t));
          h = t;
          tap(bk + ".attentions." + std::to_string(j), h);
        }
      }
      if (i + 1 < n) {
        Act u = c.new_act(B, h.H * 2, h.W * 2, co, true);
        CHECK(c.conv3(h, 1, 1, c.WB(bk + ".up.w", (int64_t)co * 9 * co), c.WF(bk + ".up.b", co), nullptr, 0, nullptr, nullptr, nullptr, 0, 0, u, bk + ".up.ws", bk + ".up.w4"));
        h = u;
        tap(bk + ".upsamplers.0", h);
      }
      if (o.film) CHECK(film_hook("up_" + std::to_string(i), h));
    }
    if (out_nchw) {
      tap("conv_norm_out.in", h);
      Act t = c.new_act(B, h.H, h.W, C0, false);
      CHECK(c.groupnorm(h.p, nullptr, C0, 0, B, h.hw(), cfg.norm_eps, c.WF("conv_norm_out.g", C0), c.WF("conv_norm_out.b", C0), 1, t.p));
      const bf16_t* wo = c.WB("conv_out.w", (int64_t)cfg.out_channels * 9 * C0);
      const float* bo = c.WF("conv_out.b", cfg.out_channels);
      if (!c.dry && !c.err) CHECK(mvd_launch_conv_out(t.p, B, h.H, h.W, C0, wo, bo, cfg.out_channels, out_nchw, c.s));
    }
    return c.err;
  }
};

// time embedding -> fused time_emb_proj for every resnet: returns [B][temb_total] fp32
int time_path(Ctx& c, const float* timesteps, int B, const float** tproj_out) {
  const mvd_config_t& cfg = c.e->cfg;
  const int C0 = cfg.block_out_channels[0], TD = 4 * C0;
  float* sinus = c.talloc<float>((size_t)B * C0);
  float* t1 = c.talloc<float>((size_t)B * TD);
  float* emb = c.talloc<float>((size_t)B * TD);
  bf16_t* act = c.talloc<bf16_t>((size_t)B * TD);
  float* tproj = c.aalloc<float>((size_t)B * c.e->temb_total);
  const bf16_t* w1 = c.WB("time.l1.w", (int64_t)TD * C0);
  const float* b1 = c.WF("time.l1.b", TD);
  const bf16_t* w2 = c.WB("time.l2.w", (int64_t)TD * TD);
  const float* b2 = c.WF("time.l2.b", TD);
  const bf16_t* wp = c.WB("temb_proj.w", (int64_t)c.e->temb_total * TD);
  const float* bp = c.WF("temb_proj.b", c.e->temb_total);
  *tproj_out = tproj;
  if (c.err) return c.err;
  if (c.dry) return 0;
  CHECK(mvd_launch_timestep_embedding(timesteps, B, C0, sinus, c.s));
  CHECK(mvd_launch_skinny_linear(sinus, C0, B, C0, w1, 1, b1, TD, 0, t1, TD, c.s));
  CHECK(mvd_launch_skinny_linear(t1, TD, B, TD, w2, 1, b2, TD, 1, emb, TD, c.s));
  // SiLU(emb) -> bf16 operand of the fused time_emb_proj GEMM (resnet: time_emb_proj(nonlinearity(temb)))
  CHECK(mvd_launch_silu_to_bf16(emb, (int64_t)B * TD, act, c.s));
  CHECK(c.linear(act, nullptr, TD, 0, B, wp, bp, c.e->temb_total, nullptr, 0, tproj, c.e->temb_total, false, true));
  return 0;
}

// camera encoder (fp32, Q9): cameras -> embedding [B][D]   (camera_encoder.py:160-196)
int camera_embed(Ctx& c, const float* src, const float* tgt, int cam_rows, const float* proj, int B, float* emb) {
  const mvd_config_t& cfg = c.e->cfg;
  const int D = cfg.cam_output_dim, Hd = cfg.cam_hidden_dim;
  const int nfreq = (D / 2) / 3, encd = 6 * nfreq;
  const bool simple = cfg.simple_cam_encoder != 0;
  float* rflat = c.talloc<float>((size_t)B * 9);
  float* enc = c.talloc<float>((size_t)B * encd);
  float* encp = c.talloc<float>((size_t)B * D);
  float* cat = c.talloc<float>((size_t)B * 2 * D);
  float* bufa = c.talloc<float>((size_t)B * (D > Hd ? D : Hd));
  float* bufb = c.talloc<float>((size_t)B * (D > Hd ? D : Hd));
  auto lin = [&](const std::string& k, const float* x, int ldx, int kin, int nout, float* y, int ldy) -> int {
    const float* w = c.WF("cam." + k + ".weight", (int64_t)nout * kin, 0);
    const float* b = c.WF("cam." + k + ".bias", nout, 0);
    if (c.err) return c.err; if (c.dry) return 0;
    return mvd_launch_skinny_linear(x, ldx, B, kin, w, 0, b, nout, 0, y, ldy, c.s);
  };
  auto lnorm = [&](const std::string& k, const float* x, int n, int silu, float* y) -> int {
    const float* g = c.WF("cam." + k + ".weight", n, 0);
    const float* b = c.WF("cam." + k + ".bias", n, 0);
    if (c.err) return c.err; if (c.dry) return 0;
    return mvd_launch_layernorm_f32(x, B, n, 1e-5f, g, b, silu, y, c.s);
  };
  if (!c.dry && !c.err) {
    CHECK(mvd_launch_camera_features(src, tgt, B, cam_rows, nfreq, 10.0f, rflat, enc, c.s));
    // Q1: projection by the per-call random matrix (no bias)
    CHECK(mvd_launch_skinny_linear(enc, encd, B, encd, proj, 0, nullptr, D, 0, encp, D, c.s));
  }
  const char* encs[2] = {"rotation_encoder", "translation_encoder"};
  for (int t = 0; t < 2; ++t) {   // -> cat[:, :D] and cat[:, D:]
    const std::string p = encs[t];
    const float* x = t == 0 ? rflat : encp;
    const int kin = t == 0 ? 9 : D;
    CHECK(lin(p + ".0", x, kin, kin, Hd, bufa, Hd));
    CHECK(lnorm(p + ".1", bufa, Hd, 1, bufb));
    if (simple) {
      CHECK(lin(p + ".3", bufb, Hd, Hd, D, cat + t * D, 2 * D));
    } else {
      CHECK(lin(p + ".3", bufb, Hd, Hd, Hd, bufa, Hd));
      CHECK(lnorm(p + ".4", bufa, Hd, 1, bufb));
      CHECK(lin(p + ".6", bufb, Hd, Hd, D, cat + t * D, 2 * D));
    }
  }
  CHECK(lin("final_projection.0", cat, 2 * D, 2 * D, D, bufa, D));
  CHECK(lnorm("final_projection.1", bufa, D, 1, bufb));
  CHECK(lin("final_projection.3", bufb, D, D, D, bufa, D));
  CHECK(lnorm("final_projection.4", bufa, D, 0, bufb));
  CHECK(lnorm("output_norm", bufb, D, 0, emb));
  return c.err;
}

// one modulator MLP: emb [B][D] -> processed FiLM scale/shift [B][dim]   (camera_encoder.py:215-222)
// (out_rows >= B: the processed scale/shift rows are replicated cyclically up to the sample batch)
int modulator(Ctx& c, const std::string& name, int dim, const float* emb, int B, float* sc, float* sh, int out_rows = 0) {
  const mvd_config_t& cfg = c.e->cfg;
  const int D = cfg.cam_output_dim;
  float* mh = c.talloc<float>((size_t)B * (D / 2));
  float* mh2 = c.talloc<float>((size_t)B * (D / 2));
  float* raw = c.talloc<float>((size_t)B * 2 * dim);
  const std::string k = "cam.modulators." + name;
  const float* w0 = c.WF(k + ".0.weight", (int64_t)(D / 2) * D, 0);
  const float* b0 = c.WF(k + ".0.bias", D / 2, 0);
  const float* g1 = c.WF(k + ".1.weight", D / 2, 0);
  const float* b1 = c.WF(k + ".1.bias", D / 2, 0);
  const float* w3 = c.WF(k + ".3.weight", (int64_t)2 * dim * (D / 2), 0);
  const float* b3 = c.WF(k + ".3.bias", 2 * dim, 0);
  if (c.err) return c.err;
  if (c.dry) return 0;
  CHECK(mvd_launch_skinny_linear(emb, D, B, D, w0, 0, b0, D / 2, 0, mh, D / 2, c.s));
  CHECK(mvd_launch_layernorm_f32(mh, B, D / 2, 1e-5f, g1, b1, 1, mh2, c.s));
  CHECK(mvd_launch_skinny_linear(mh2, D / 2, B, D / 2, w3, 0, b3, 2 * dim, 0, raw, 2 * dim, c.s));
  return mvd_launch_film_params(raw, B, dim, cfg.cam_modulation_strength, sc, sh, out_rows > B ? out_rows : B, c.s);
}

// modulators addressed by the hooks: name -> dim (mvd_unet.py:63-80); "mid" exists as a parameter but
// is never addressed (the hook asks for "mid_0", Q3)
std::vector<std::pair<std::string, int>> modulator_dims(const mvd_config_t& cfg, bool include_mid) {
  std::vector<std::pair<std::string, int>> mods;
  for (int i = 0; i < cfg.num_levels; ++i) mods.push_back({"down_" + std::to_string(i), cfg.block_out_channels[i]});
  for (int i = 0; i < cfg.num_levels; ++i) mods.push_back({"up_" + std::to_string(i), cfg.block_out_channels[cfg.num_levels - 1 - i]});
  if (include_mid) mods.push_back({"mid", cfg.block_out_channels[cfg.num_levels - 1]});
  mods.push_back({"output", 4});
  return mods;
}

// FiLM scale/shift of every hooked modulator: emb [Bc][D] -> ss[name] = {scale [B][dim], shift [B][dim]}, rows beyond Bc
// replicated cyclically (B >= Bc).  The forward (camera_path) and mvd_engine_film_params both run this.  `concat`: the
// concatenated slots are there (a sizing pass that cannot know assumes so; one that can must size the form that will run).
int film_params_all(Ctx& c, const float* emb, int Bc, int B, std::unordered_map<std::string, std::pair<float*, float*>>& ss, bool concat) {
  const mvd_config_t& cfg = c.e->cfg;
  const int D = cfg.cam_output_dim;
  // all hooked modulators at once when the concatenated slots are registered (packing.pack_camera): 4 launches instead of 4 each
  const auto mods = modulator_dims(cfg, false);
  if (concat && mods.size() <= 16) {
    const int nm = (int)mods.size(), Hh = D / 2;
    MvdSegTable seg; memset(&seg, 0, sizeof(seg));
    seg.n = nm;
    int tot = 0;
    for (int i = 0; i < nm; ++i) { tot += 2 * mods[i].second; seg.end[i] = tot; }
    float* ssbuf = c.aalloc<float>((size_t)B * tot);                  // per modulator: scale [B][dim] | shift [B][dim]
    const size_t mk = c.e->tmp.off;
    float* h1 = c.talloc<float>((size_t)Bc * nm * Hh);
    float* h2 = c.talloc<float>((size_t)Bc * nm * Hh);
    float* raw = c.talloc<float>((size_t)Bc * tot);
    const float* w0 = c.WF("cam.modcat.w0", (int64_t)nm * Hh * D, 0);
    const float* b0 = c.WF("cam.modcat.b0", (int64_t)nm * Hh, 0);
    const float* g1 = c.WF("cam.modcat.g1", (int64_t)nm * Hh, 0);
    const float* be1 = c.WF("cam.modcat.be1", (int64_t)nm * Hh, 0);
    const float* w3 = c.WF("cam.modcat.w3", (int64_t)tot * Hh, 0);
    const float* b3 = c.WF("cam.modcat.b3", tot, 0);
    if (!c.dry && !c.err) {
      CHECK(mvd_launch_skinny_linear(emb, D, Bc, D, w0, 0, b0, nm * Hh, 0, h1, nm * Hh, c.s));
      CHECK(mvd_launch_layernorm_f32(h1, Bc * nm, Hh, 1e-5f, g1, be1, 1, h2, c.s, nm));
      CHECK(mvd_launch_skinny_linear_grouped(h2, nm * Hh, Hh, Bc, Hh, w3, b3, tot, seg, raw, tot, c.s));
      CHECK(mvd_launch_film_params_grouped(raw, Bc, seg, cfg.cam_modulation_strength, ssbuf, B, c.s));
    }
    c.e->tmp.off = mk;
    int c0 = 0;
    for (int i = 0; i < nm; ++i) {
      float* sc = ssbuf + (size_t)B * 2 * c0;
      ss[mods[i].first] = {sc, sc + (size_t)B * mods[i].second};
      c0 += mods[i].second;
    }
    return c.err;
  }
  for (auto& m : mods) {
    float* sc = c.aalloc<float>((size_t)B * m.second);
    float* sh = c.aalloc<float>((size_t)B * m.second);
    const size_t mk = c.e->tmp.off;
    CHECK(modulator(c, m.first, m.second, emb, Bc, sc, sh, B));
    c.e->tmp.off = mk;
    ss[m.first] = {sc, sh};
  }
  return c.err;
}

// The camera batch Bc may be smaller than the sample batch B (classifier-free guidance doubles the latents but not the
// cameras, pipeline.py:141-152): the (Bc, C, 1, 1) scale/shift then broadcasts over the sample rows like torch does for
// Bc == 1; for 1 < Bc < B (Bc | B) row b takes camera b % Bc, i.e. the [uncond | cond] halves share their cameras.
int camera_path(Ctx& c, const mvd_forward_args_t& a, std::unordered_map<std::string, std::pair<float*, float*>>& ss) {
  const mvd_config_t& cfg = c.e->cfg;
  const int B = a.batch, D = cfg.cam_output_dim;
  const int Bc = a.cam_batch > 0 ? a.cam_batch : B;
  float* emb = c.aalloc<float>((size_t)Bc * D);
  c.e->cam_emb = emb; c.e->cam_batch = Bc;
  CHECK(camera_embed(c, a.source_camera, a.target_camera, a.cam_rows, a.fourier_proj, Bc, emb));
  return film_params_all(c, emb, Bc, B, ss, c.dry || c.has("cam.modcat.w0", 0));
}

// Split-K arrival counters for one entry call: a block of the workspace, zeroed once (one memset node in front of the
// call's first kernel); Ctx::gemm hands every split-K launch its own slice.
constexpr int MVD_TILE_COUNTERS = 32768;
int setup_tile_counters(mvd_engine* e, unsigned int* block, hipStream_t s, bool dry) {
  e->cnt_base = block; e->cnt_used = 0; e->cnt_cap = MVD_TILE_COUNTERS;
  if (dry) return 0;
  hipError_t he = hipMemsetAsync(block, 0, MVD_TILE_COUNTERS * sizeof(unsigned int), s);
  if (he != hipSuccess) { mvd_set_error("forward: hipMemsetAsync(tile counters): %s", hipGetErrorString(he)); return -3; }
  return 0;
}

int forward_body(mvd_engine* e, const mvd_forward_args_t& a, hipStream_t s, bool dry, const ViewLayout& lay) {
  const mvd_config_t& cfg = e->cfg;
  if (a.batch <= 0 || a.height <= 0 || a.width <= 0 || a.text_len <= 0) { mvd_set_error("forward: bad shape"); return -1; }
  const int div = 1 << (cfg.num_levels - 1);
  if (a.height % div || a.width % div) { mvd_set_error("forward: latent %dx%d must be divisible by %d", a.height, a.width, div); return -1; }
  // ref_only: mvd_engine_reference_encode -- the reference pass alone, normalisation deferred (global Q2 statistics)
  const bool ref_only = a.flags & MVD_REF_ONLY_INTERNAL;
  const bool use_cam = (a.flags & MVD_USE_CAMERA) && !ref_only, use_img = a.flags & MVD_USE_IMAGE, reuse = a.flags & MVD_REUSE_REF;
  if (ref_only && (!use_img || reuse)) { mvd_set_error("reference_encode: needs MVD_USE_IMAGE without MVD_REUSE_REF"); return -1; }
  // ---- DeepCache (include/mvd_hip.h): every rejection comes here, in the dry run that precedes any launch
  const int deep = a.flags & (MVD_DEEPCACHE_REFRESH | MVD_DEEPCACHE_SHALLOW);
  const bool shallow = deep == MVD_DEEPCACHE_SHALLOW;
  if (deep) {
    if (deep == (MVD_DEEPCACHE_REFRESH | MVD_DEEPCACHE_SHALLOW)) { mvd_set_error("forward: MVD_DEEPCACHE_REFRESH and MVD_DEEPCACHE_SHALLOW are one or the other, got both"); return -1; }
    if (!e->opt.dc_on) { mvd_set_error("forward: %s without mvd_engine_set_deepcache", shallow ? "MVD_DEEPCACHE_SHALLOW" : "MVD_DEEPCACHE_REFRESH"); return -1; }
    if (e->opt.dc_branch < 0 || e->opt.dc_branch >= cfg.layers_per_block) { mvd_set_error("forward: DeepCache branch %d outside [0, %d)", e->opt.dc_branch, cfg.layers_per_block); return -1; }
    if (shallow && use_img && !reuse) { mvd_set_error("forward: MVD_DEEPCACHE_SHALLOW with MVD_USE_IMAGE needs MVD_REUSE_REF (a shallow forward never runs the encoder pass)"); return -1; }
    if (shallow && !e->dc_sizing) {
      const mvd_engine::DeepRecord& r = e->dc_rec;
      if (!r.valid) { mvd_set_error("forward: MVD_DEEPCACHE_SHALLOW without a stored deep feature (run a MVD_DEEPCACHE_REFRESH forward first)"); return -1; }
      if (r.batch != a.batch) { mvd_set_error("forward: MVD_DEEPCACHE_SHALLOW: the stored deep feature is of batch %d, this forward of batch %d", r.batch, a.batch); return -1; }
      if (r.h != a.height || r.w != a.width) { mvd_set_error("forward: MVD_DEEPCACHE_SHALLOW: the stored deep feature is of latent size %dx%d, this forward of %dx%d", r.h, r.w, a.height, a.width); return -1; }
      if (r.layout != lay.key()) { mvd_set_error("forward: MVD_DEEPCACHE_SHALLOW: the stored deep feature is of another batch layout (views / objects / view counts)"); return -1; }
      if (r.cam != (use_cam ? 1 : 0) || r.img != (use_img ? 1 : 0)) {
        mvd_set_error("forward: MVD_DEEPCACHE_SHALLOW: the stored deep feature is of a forward with camera conditioning %s and image conditioning %s, this one has them %s and %s",
                      r.cam ? "on" : "off", r.img ? "on" : "off", use_cam ? "on" : "off", use_img ? "on" : "off"); return -1;
      }
      if (r.branch != e->opt.dc_branch) { mvd_set_error("forward: MVD_DEEPCACHE_SHALLOW: the stored deep feature is of branch %d, the engine is set to branch %d", r.branch, e->opt.dc_branch); return -1; }
      if (r.wgen != e->weight_gen) { mvd_set_error("forward: MVD_DEEPCACHE_SHALLOW: weights were registered or cleared since the deep feature was stored"); return -1; }
    }
    if (!e->dc_sizing) {
      const int64_t need = (int64_t)a.batch * a.height * a.width * e->dc_hidden_channels() * (int64_t)sizeof(bf16_t);
      if (!e->dc_ptr || e->dc_bytes < need) { mvd_set_error("forward: DeepCache buffer not bound or too small (%lld bytes bound, %lld needed; mvd_engine_bind_deepcache)", (long long)e->dc_bytes, (long long)need); return -1; }
    }
  }
  if (!dry) {
    if (!ref_only && (!a.sample || !a.timesteps || !a.text || !a.out)) { mvd_set_error("forward: null sample/timesteps/text/out"); return -1; }
    if (use_cam && (!a.source_camera || !a.target_camera || !a.fourier_proj || (a.cam_rows != 3 && a.cam_rows != 4))) { mvd_set_error("forward: camera inputs missing"); return -1; }
    if (use_img && !reuse && (!a.source_latents || !a.encoder_text || a.ref_batch <= 0)) { mvd_set_error("forward: image-conditioning inputs missing"); return -1; }
    if (!e->ws_ptr) { mvd_set_error("forward: workspace not bound"); return -1; }
  }
  if (use_img && a.ref_batch <= 0) { mvd_set_error("forward: ref_batch must be > 0 with MVD_USE_IMAGE"); return -1; }
  // ---- the batch layout (ragged.h; include/mvd_hip.h): everything is checked here, before any launch
  if (!(a.flags & MVD_SHARE_REF) && a.views > 1) { mvd_set_error("forward: views = %d needs MVD_SHARE_REF", a.views); return -1; }
  char msg[256];
  if (lay.validate(a.flags & MVD_SHARE_REF, use_img, a.batch, a.ref_batch, use_cam ? a.cam_batch : INT_MIN, a.height, a.width, cfg.num_levels, msg, sizeof(msg))) { mvd_set_error("%s", msg); return -1; }
  // FreeU filters the maps of up blocks 0 and 1 (levels n - 1 and n - 2): a map of one row or column has no frequency -1
  if (e->opt.freeu_on && !ref_only && ((a.height >> (cfg.num_levels - 1)) < 2 || (a.width >> (cfg.num_levels - 1)) < 2)) {
    mvd_set_error("forward: FreeU needs maps of at least 2 x 2 in up block 0, latent %dx%d gives %dx%d", a.height, a.width, a.height >> (cfg.num_levels - 1), a.width >> (cfg.num_levels - 1)); return -1;
  }
  if (use_cam && a.cam_batch > 0 && (a.cam_batch > a.batch || a.batch % a.cam_batch)) { mvd_set_error("forward: camera batch %d must divide the sample batch %d", a.cam_batch, a.batch); return -1; }
  // the input FiLM uses the 4-wide "output" modulator (mvd_unet.py:74-80, 256-258): any other in_channels is a broadcast
  // error in the reference and would read past the [B][4] scale/shift rows here -- reject before any launch
  if (!dry && use_cam && cfg.in_channels != 4) { mvd_set_error("forward: camera conditioning needs in_channels == 4 (the 'output' modulator is 4 wide), got %d", cfg.in_channels); return -1; }

  e->tmp.reset(dry); e->act.reset(dry);
  Ctx c{e, s, 0, dry};
  CHECK(setup_tile_counters(e, (unsigned int*)e->act.alloc(MVD_TILE_COUNTERS * sizeof(unsigned int)), s, dry));
  const int B = a.batch, H = a.height, Wd = a.width, L = a.text_len, xd = cfg.cross_attention_dim;

  // ---- persistent reference cache layout
  if (use_img) {
    const bool keep = (a.flags & MVD_KEEP_FEATURES) || ref_only;
    if (reuse) {
      if (!e->rc_valid || e->rc_batch != a.ref_batch || e->rc_h != H || e->rc_w != Wd || e->rc_layout != lay.key()) { mvd_set_error("forward: MVD_REUSE_REF without a matching cached reference"); return -1; }
    } else {
      e->persist.reset(dry);
      e->refkv.assign(e->feats.size(), nullptr);
      e->feat_keep.assign(e->feats.size(), nullptr);
      for (size_t i = 0; i < e->feats.size(); ++i) {
        const int lv = e->feats[i].level;
        const size_t hw = (size_t)(H >> lv) * (Wd >> lv);
        e->refkv[i] = (bf16_t*)e->persist.alloc((size_t)a.ref_batch * hw * 4 * e->feats[i].C * sizeof(bf16_t));
        if (keep) e->feat_keep[i] = (bf16_t*)e->persist.alloc((size_t)a.ref_batch * hw * e->feats[i].C * sizeof(bf16_t));
      }
      if (e->persist.overflow()) { mvd_set_error("forward: reference cache too small (%zu > %zu bytes)", e->persist.high, e->persist.cap); return -4; }
      e->rc_keep = keep; e->rc_batch = a.ref_batch; e->rc_h = H; e->rc_w = Wd; e->rc_layout = lay.key();
      if (!dry) { e->rc_valid = false; e->rc_pending = false; }
    }
  }

  // ---- the encoder pass goes to the side stream (see mvd_engine::side): at batch 1 the two passes overlap almost completely
  // (cfg3 cold 9.8 -> 7.0 ms), at 32 pairs the second stream still fills the tails and the under-filled launches of the deep
  // levels (cfg4 65.0 -> 63.5 ms, same box).  `dual` (a function of the call's flags only) decides the workspace layout -- in
  // the sizing runs too; whether the side stream is really used also needs: no per-launch profiling.
  const bool dual = use_img && !reuse && !ref_only;
  e->dual_late = false;
  // (Round 5: under hipGraph capture too.  The fork event is recorded on the capturing stream and waited for by the side stream,
  //  which thereby joins the capture; the per-feature events and the join event become edges of the graph, so a replayed
  //  forward keeps the two-branch schedule instead of serialising the passes.  MVD_DBG_GRAPH_ONE_STREAM restores the one-stream capture.)
  e->dual_now = dual && !dry && !(e->graph_on && (g_debug_flags & MVD_DBG_GRAPH_ONE_STREAM)) && (!e->prof || e->prof_overlap) && !(g_debug_flags & MVD_DBG_ONE_STREAM);
  // Where the side stream forks: in front of everything (the encoder pass needs nothing of the camera path).  Round 5's two-stream
  // kernel stats showed what that does to the ~30 latency-bound launches in front of the main pass (camera MLPs, time MLPs): the
  // encoder's persistent 256-workgroup kernels fill every CU's register file, so a small kernel of the other stream waits for
  // a whole big kernel to retire -- 145 us per time-MLP launch, 390 us for the grouped modulator layer, ~1.6 ms before the main
  // pass (the step's critical path) can start.  The alternative `early` (MVD_DBG_FORK_LATE: those launches of BOTH passes first,
  // on an otherwise idle chip, the fork behind them) was measured and LOSES: cfg4 60.19 -> 60.96 ms, cfg3 6.46 -> 6.67 ms (three /
  // two same-box alternations) -- an idle chip for 0.75 ms costs more than the slowed-down front matter.  What helped instead is
  // making those launches cheap (misc.hip skinny_mfma_kernel).  `early` is a function of the call's flags only, so the sizing run
  // allocates in the same order.
  const bool early = dual && (g_debug_flags & MVD_DBG_FORK_LATE);
  auto fork = [&]() -> int {
    if (!e->dual_now) return 0;
    CHECK(e->ensure_side_stream());
    if (hipEventRecord(e->fork_ev, s) != hipSuccess || hipStreamWaitEvent(e->side, e->fork_ev, 0) != hipSuccess) { mvd_set_error("forward: stream fork failed"); return -3; }
    return 0;
  };
  if (!early) CHECK(fork());

  // ---- camera path (fp32) -> embedding + FiLM scale/shift per modulator
  std::unordered_map<std::string, std::pair<float*, float*>> film_ss;
  // (running this path on a side stream concurrently with the reference pass was measured: +0.1 %, within noise --
  //  the persistent GEMMs leave no free CU resources for it -- so it stays on the caller's stream)
  if (use_cam) CHECK(camera_path(c, a, film_ss));
  const float* tproj_main = nullptr;
  const float* tproj_enc = nullptr;
  if (early) {
    c.set = 0;
    CHECK(time_path(c, a.timesteps, B, &tproj_main));
    c.set = e->share_encoder ? 0 : 1;
    float* tz = c.aalloc<float>(a.ref_batch);
    if (!dry) CHECK((int)hipMemsetAsync(tz, 0, a.ref_batch * sizeof(float), s));
    CHECK(time_path(c, tz, a.ref_batch, &tproj_enc));
    c.set = 0;
    CHECK(fork());
  }

  // ---- reference image encoder pass (frozen UNet at t = 0, plain attention) -> adapter K/V
  // Small batches: on the side stream, concurrently with the main pass (see mvd_engine::side).  Not under graph capture /
  // per-launch profiling (one stream each), not for the deferred-statistics form.
  if (use_img && !reuse) {
    // (dual: the camera path's kernels on the caller's stream may still be using their scoped temporaries when the side
    //  stream starts -- the encoder pass gets a region of its own behind them)
    if (dual) e->tmp.off = e->tmp.high;
    const size_t tm = e->tmp.off, am = e->act.off;
    if (e->dual_now) { c.s = e->side; c.nowait = true; }
    c.set = e->share_encoder ? 0 : 1;
    const int Br = a.ref_batch;
    const float* tproj = tproj_enc;
    if (!tproj) {
      float* tz = c.talloc<float>(Br);
      if (!dry) CHECK((int)hipMemsetAsync(tz, 0, Br * sizeof(float), c.s));
      CHECK(time_path(c, tz, Br, &tproj));
    }
    bf16_t* tx = c.aalloc<bf16_t>((size_t)Br * L * xd);
    Act xin = c.new_act(Br, H, Wd, 64, true);   // im2col rows for conv_in
    if (!dry && !c.err) {
      CHECK(mvd_launch_f32_to_bf16(a.encoder_text, (int64_t)Br * L * xd, tx, c.s));
      CHECK(mvd_launch_im2col_in(a.source_latents, Br, cfg.in_channels, H, Wd, nullptr, nullptr, 0, xin.p, c.s));
    }
    PassOpts po; po.capture = true; po.ref_batch = Br; po.layout = &lay;
    po.defer_norm = ref_only; po.stats = e->ref_stats_out;
    UNetPass pass{c, cfg, po, Br, H, Wd, L, tx, tproj};
    CHECK(pass.run(xin, nullptr));
    if (!dry) { e->rc_valid = !ref_only; e->rc_pending = ref_only; }
    if (dual) {
      // the encoder pass may still be RUNNING while the main pass is issued: its activations stay, the main pass's scoped
      // temporaries start behind the encoder's high-water mark.  (Main-pass kernels may rendezvous again: the side stream's
      // never wait, so every workgroup of a main-pass kernel becomes resident eventually.)
      e->tmp.off = e->tmp.high;
      if (e->dual_now && hipEventRecord(e->join_ev, e->side) != hipSuccess) { mvd_set_error("forward: hipEventRecord failed"); return -3; }
      c.s = s; c.nowait = false;
    } else {
      e->tmp.off = tm; e->act.off = am;   // encoder activations are dead; reuse their memory
    }
  }
  if (ref_only) {
    if (c.err) return c.err;
    if (!dry && (e->tmp.high + e->act.high > (size_t)e->ws_bytes)) { mvd_set_error("reference_encode: workspace too small"); return -4; }
    return 0;
  }

  // ---- main pass
  c.set = 0;
  const float* tproj = tproj_main;
  if (!tproj) CHECK(time_path(c, a.timesteps, B, &tproj));
  const int TB = lay.text_rows(B);          // text rows: one per guidance half (and object) in a shared forward
  bf16_t* tx = c.aalloc<bf16_t>((size_t)TB * L * xd);
  Act xin = c.new_act(B, H, Wd, 64, true);   // im2col rows for conv_in
  if (!dry && !c.err) {
    CHECK(mvd_launch_f32_to_bf16(a.text, (int64_t)TB * L * xd, tx, s));
    const float* sc = nullptr; const float* sh = nullptr;
    if (use_cam) { sc = film_ss["output"].first; sh = film_ss["output"].second; }   // mvd_unet.py:256-258 (input FiLM)
    CHECK(mvd_launch_im2col_in(a.sample, B, cfg.in_channels, H, Wd, sc, sh, 4, xin.p, s));
  }
  PassOpts po; po.adapter = use_img; po.film = use_cam; po.ref_batch = a.ref_batch; po.film_ss = &film_ss;
  // (decided per forward, not kept on the engine: clearing the flag restores the product's schedule.  "From up_blocks.2"
  //  measured no difference and has no switch.)
  static const int late_dflt = MVD_ENV_INT("MVD_DUAL_LATE_FROM", 99);
  po.late_from = (g_debug_flags & MVD_DBG_LATE_FROM_UP1) ? 1 : late_dflt;
  po.layout = &lay;
  po.main = &e->opt;
  if (e->opt.tome_keep && !dry) e->tome_tab.assign(e->feats.size(), {});
  if (!dry) e->todo_nk.assign(e->feats.size(), 0);
  if (!dry) e->taps.clear();
  po.deep = deep; po.deep_buf = (bf16_t*)e->dc_ptr;
  UNetPass pass{c, cfg, po, B, H, Wd, L, tx, tproj};
  pass.text_rows = TB;
  CHECK(pass.run(xin, a.out));
  if (e->dual_now) {   // join: everything the side stream did (kept features included) precedes whatever follows on s
    if (hipStreamWaitEvent(s, e->join_ev, 0) != hipSuccess) { mvd_set_error("forward: stream join failed"); return -3; }
    e->dual_now = false;
  }
  if (c.err) return c.err;
  if (!dry && (e->tmp.high + e->act.high > (size_t)e->ws_bytes)) { mvd_set_error("forward: workspace too small"); return -4; }
  return 0;
}

// Every exit of a forward that forked the side stream joins it: an error return between fork and join (a failed check in the
// camera path or a pass, a workspace that is too small) must not leave the encoder pass writing the reference cache and the
// activation arena while the caller frees or reuses them.  The success path has joined with an event already.
int forward_impl(mvd_engine* e, const mvd_forward_args_t& a, hipStream_t s, bool dry, const ViewLayout& lay = ViewLayout()) {
  const int r = forward_body(e, a, s, dry, lay);
  if (e->dual_now) {
    if (e->side) (void)hipStreamSynchronize(e->side);      // error path only: the cheap join is not worth an event here
    e->dual_now = false;
  }
  return r;
}

// Second half of the global-statistics path: normalise the kept raw features with the merged per-pixel (mean, k) and
// project them to the adapter K/V -- the same two launches per feature the encoder pass makes in the local form.
int reference_finish_impl(mvd_engine* e, const float* mean_k, hipStream_t s, bool dry) {
  e->tmp.reset(dry);
  Ctx c{e, s, 0, dry};
  CHECK(setup_tile_counters(e, (unsigned int*)e->tmp.alloc(MVD_TILE_COUNTERS * sizeof(unsigned int)), s, dry));
  c.set = 0;                                         // the adapter's ref_kv weights live with the base set
  for (size_t i = 0; i < e->feats.size(); ++i) {
    const int lv = e->feats[i].level, C = e->feats[i].C;
    const int hw = (e->rc_h >> lv) * (e->rc_w >> lv), M = e->rc_batch * hw;
    const std::string& key = e->feats[i].key;
    const size_t mk = e->tmp.off;
    bf16_t* rn = c.talloc<bf16_t>((size_t)M * C);
    if (!dry && !c.err) CHECK(mvd_launch_refapply(e->feat_keep[i], e->rc_batch, hw, C, mean_k + 2 * e->feat_pixel_off((int)i), rn, s));
    CHECK(c.linear(rn, nullptr, C, 0, M, c.WB(key + ".ref_kv.w", (int64_t)4 * C * C, 0), nullptr, 4 * C, nullptr, 0, e->refkv[i], 4 * C));
    e->tmp.off = mk;
  }
  return c.err;
}

}  // namespace

// silu -> bf16 helper kernel (time embedding activation)
__global__ void silu_to_bf16_kernel(const float* __restrict__ x, long n, bf16_t* __restrict__ y) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) y[i] = f2bf(silu_f(x[i]));
}
int mvd_launch_silu_to_bf16(const float* x, int64_t n, bf16_t* y, hipStream_t s) {
  int grid = (int)((n + 255) / 256); if (grid > 1024) grid = 1024;
  hipLaunchKernelGGL(silu_to_bf16_kernel, dim3(grid), dim3(256), 0, s, x, (long)n, y);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { mvd_set_error("silu_to_bf16 launch: %s", hipGetErrorString(e)); return -3; }
  return 0;
}

// =========================================================================== C ABI
extern "C" {

int mvd_engine_create(const mvd_config_t* cfg, mvd_engine_t** out) {
  if (!cfg || !out) { mvd_set_error("engine_create: null argument"); return -1; }
  if (cfg->num_levels < 2 || cfg->num_levels > MVD_MAX_LEVELS || cfg->layers_per_block < 1) { mvd_set_error("engine_create: unsupported topology"); return -1; }
  for (int i = 0; i < cfg->num_levels; ++i) {
    const int c = cfg->block_out_channels[i];
    if (c % 64 || c % cfg->norm_num_groups || cfg->num_heads[i] * 64 != c) { mvd_set_error("engine_create: level %d: channels %d must be a multiple of 64/groups with head_dim 64 (heads %d)", i, c, cfg->num_heads[i]); return -1; }
  }
  if (cfg->cross_attention_dim % 64) { mvd_set_error("engine_create: cross_attention_dim must be a multiple of 64"); return -1; }
  if (cfg->in_channels > 7 || cfg->out_channels > 8) { mvd_set_error("engine_create: in_channels must be <= 7 (9*Cin <= 64) and out_channels <= 8"); return -1; }
  mvd_engine* e = new mvd_engine();
  e->cfg = *cfg;
  e->feats = enumerate_features(*cfg);
  int off = 0;
  for (auto& r : enumerate_resnets(*cfg)) { e->temb_off.push_back(off); off += r.cout; }
  e->temb_total = off;
  off = 0;
  for (auto& f : e->feats) { e->tkv_off.push_back(off); off += 2 * f.C; }
  e->tkv_total = off;
  *out = e;
  return 0;
}

int mvd_engine_destroy(mvd_engine_t* e) { delete e; return 0; }

int mvd_engine_set_weight(mvd_engine_t* e, int set, const char* slot, const void* ptr, int64_t numel, int dtype) {
  if (e) e->drop_graphs();
  if (!e || set < 0 || set > 1 || !slot || !ptr || numel <= 0 || dtype < 0 || dtype > 1) { mvd_set_error("set_weight: bad argument"); return -1; }
  if ((uintptr_t)ptr & 15) { mvd_set_error("set_weight: '%s' must be 16-byte aligned", slot); return -1; }
  e->w[set].m[slot] = Weight{ptr, numel, dtype};
  ++e->weight_gen;
  return 0;
}
int mvd_engine_clear_weights(mvd_engine_t* e, int set) {
  if (e) e->drop_graphs();
  if (!e || set < 0 || set > 1) { mvd_set_error("clear_weights: bad argument"); return -1; }
  e->w[set].m.clear();
  ++e->weight_gen;
  return 0;
}

static void fill_dry_args(mvd_forward_args_t& a, int batch, int h, int w, int L, int ref_batch) {
  memset(&a, 0, sizeof(a));
  a.batch = batch; a.height = h; a.width = w; a.text_len = L; a.ref_batch = ref_batch; a.cam_rows = 4;
  a.flags = MVD_USE_CAMERA | (ref_batch > 0 ? MVD_USE_IMAGE : 0);
}

int64_t mvd_engine_workspace_bytes(mvd_engine_t* e, int batch, int height, int width, int text_len, int ref_batch) {
  if (!e) { mvd_set_error("workspace_bytes: null engine"); return -1; }
  mvd_forward_args_t a; fill_dry_args(a, batch, height, width, text_len, ref_batch);
  const mvd_engine::HostState before = e->host_state();     // (a sizing call leaves no dry pointers behind)
  int r = forward_impl(e, a, nullptr, true);
  e->set_host_state(before);
  if (r) return r;
  // act and tmp arenas share one buffer: [act | tmp]
  return (int64_t)(((e->act.high + 255) & ~size_t(255)) + e->tmp.high + 4096);
}

// The layout of mvd_unet_forward (objects = 0) / mvd_unet_forward_objects and their sizing entries (null args: the callee says so)
static ViewLayout uniform_layout(const mvd_forward_args_t* args, int objects) {
  return args ? ViewLayout::uniform(objects, args->views, args->flags & MVD_SHARE_REF) : ViewLayout();
}

static int64_t workspace_bytes_args(mvd_engine_t* e, const mvd_forward_args_t* args, const ViewLayout& lay) {
  if (!e || !args) { mvd_set_error("workspace_bytes_args: null argument"); return -1; }
  if (args->flags & MVD_REF_ONLY_INTERNAL) { mvd_set_error("workspace_bytes_args: unknown flag bits 0x%x", args->flags); return -1; }
  const mvd_engine::HostState before = e->host_state();
  // (a sizing call must not depend on the cache state: size the forward that runs the encoder pass, the larger of the two)
  mvd_forward_args_t a = *args;
  a.flags &= ~MVD_REUSE_REF;
  auto total = [&]() { return (int64_t)(((e->act.high + 255) & ~size_t(255)) + e->tmp.high + 4096); };
  if (a.flags & MVD_DEEPCACHE_SHALLOW) {
    // a shallow forward is sized as what it is -- no encoder pass (MVD_REUSE_REF stays, the cache state is not consulted: dc_sizing
    // and a cache record that matches by construction) -- and must never need more than the full forward of the same arguments
    mvd_forward_args_t f = a;
    f.flags &= ~(MVD_DEEPCACHE_SHALLOW | MVD_DEEPCACHE_REFRESH);
    int r = forward_impl(e, f, nullptr, true, lay);
    const int64_t full = total();
    if (!r) {
      if (a.flags & MVD_USE_IMAGE) a.flags |= MVD_REUSE_REF;   // (the dry run above left a matching record: rc_batch, rc_h, rc_w, rc_layout)
      const bool was_valid = e->rc_valid;
      e->rc_valid = true; e->dc_sizing = true;
      r = forward_impl(e, a, nullptr, true, lay);
      e->dc_sizing = false; e->rc_valid = was_valid;
    }
    const int64_t sh = total();
    e->set_host_state(before);
    if (r) return r;
    if (sh > full) { mvd_set_error("workspace_bytes: a shallow forward needs %lld bytes, more than the full forward's %lld", (long long)sh, (long long)full); return -1; }
    return sh;
  }
  e->dc_sizing = true;          // (a refresh forward is sized without a bound buffer)
  int r = forward_impl(e, a, nullptr, true, lay);
  e->dc_sizing = false;
  e->set_host_state(before);
  if (r) return r;
  return total();
}
int64_t mvd_engine_workspace_bytes_args(mvd_engine_t* e, const mvd_forward_args_t* args) { return workspace_bytes_args(e, args, uniform_layout(args, 0)); }
int64_t mvd_engine_workspace_bytes_objects(mvd_engine_t* e, const mvd_forward_args_t* args, int objects) {
  return workspace_bytes_args(e, args, uniform_layout(args, objects));
}

int64_t mvd_engine_refcache_bytes(mvd_engine_t* e, int ref_batch, int height, int width, int keep_features) {
  if (!e || ref_batch <= 0) { mvd_set_error("refcache_bytes: bad argument"); return -1; }
  size_t total = 0;
  for (auto& f : e->feats) {
    const size_t hw = (size_t)(height >> f.level) * (width >> f.level);
    total += (((size_t)ref_batch * hw * 4 * f.C * 2) + 255) & ~size_t(255);
    if (keep_features) total += (((size_t)ref_batch * hw * f.C * 2) + 255) & ~size_t(255);
  }
  return (int64_t)total + 4096;
}

int mvd_engine_bind_workspace(mvd_engine_t* e, void* ws, int64_t ws_bytes, void* refcache, int64_t refcache_bytes) {
  if (e) e->drop_graphs();
  if (!e || !ws || ws_bytes <= 0) { mvd_set_error("bind_workspace: bad argument"); return -1; }
  if (((uintptr_t)ws & 255) || (refcache && ((uintptr_t)refcache & 255))) { mvd_set_error("bind_workspace: buffers must be 256-byte aligned"); return -1; }
  e->ws_ptr = ws; e->ws_bytes = ws_bytes;
  e->rc_ptr = refcache; e->rc_bytes = refcache_bytes;
  e->persist.base = (char*)refcache; e->persist.cap = (size_t)(refcache ? refcache_bytes : 0);
  e->rc_valid = false; e->rc_pending = false;
  e->taps.clear();
  return 0;
}

int64_t mvd_engine_reference_pixels(mvd_engine_t* e, int height, int width) {
  if (!e || height <= 0 || width <= 0) { mvd_set_error("reference_pixels: bad argument"); return -1; }
  return e->ref_pixels(height, width);
}

int mvd_engine_reference_encode(mvd_engine_t* e, const mvd_forward_args_t* args, float* local_stats, void* stream) {
  if (!e || !args || !local_stats) { mvd_set_error("reference_encode: null argument"); return -1; }
  if ((args->flags & MVD_SHARE_REF) || args->views > 1) { mvd_set_error("reference_encode: MVD_SHARE_REF does not go with the global-statistics path (one object, one rank)"); return -1; }
  if (args->flags & (MVD_DEEPCACHE_REFRESH | MVD_DEEPCACHE_SHALLOW)) { mvd_set_error("reference_encode: the DeepCache bits do not go with the encoder pass alone"); return -1; }
  e->drop_graphs();
  mvd_forward_args_t a = *args;
  a.flags = (a.flags & ~MVD_REUSE_REF) | MVD_USE_IMAGE | MVD_KEEP_FEATURES | MVD_REF_ONLY_INTERNAL;
  if (a.batch <= 0) a.batch = a.ref_batch;
  int r = forward_impl(e, a, nullptr, true);
  e->rc_valid = false; e->rc_pending = false;
  if (r) return r;
  const size_t act_bytes = (e->act.high + 255) & ~size_t(255);
  if (!e->ws_ptr || act_bytes + e->tmp.high > (size_t)e->ws_bytes) {
    mvd_set_error("reference_encode: workspace too small: need %zu bytes, bound %lld", act_bytes + e->tmp.high, (long long)e->ws_bytes);
    return -4;
  }
  e->act.base = (char*)e->ws_ptr; e->act.cap = act_bytes;
  e->tmp.base = (char*)e->ws_ptr + act_bytes; e->tmp.cap = (size_t)e->ws_bytes - act_bytes;
  e->ref_stats_out = local_stats;
  r = forward_impl(e, a, (hipStream_t)stream, false);
  e->ref_stats_out = nullptr;
  return r;
}

int mvd_engine_reference_finish(mvd_engine_t* e, const float* mean_k, void* stream) {
  if (!e || !mean_k) { mvd_set_error("reference_finish: null argument"); return -1; }
  if (!e->rc_pending) { mvd_set_error("reference_finish: no pending reference (call mvd_engine_reference_encode first)"); return -1; }
  e->drop_graphs();
  int r = reference_finish_impl(e, mean_k, nullptr, true);
  if (r) return r;
  if (!e->ws_ptr || e->tmp.high > (size_t)e->ws_bytes) { mvd_set_error("reference_finish: workspace too small (%zu > %lld bytes)", e->tmp.high, (long long)e->ws_bytes); return -4; }
  e->tmp.base = (char*)e->ws_ptr; e->tmp.cap = (size_t)e->ws_bytes;
  r = reference_finish_impl(e, mean_k, (hipStream_t)stream, false);
  if (r) return r;
  e->rc_pending = false; e->rc_valid = true;
  return 0;
}

// after a dry run: do the two arenas it sized fit the bound workspace?
static int workspace_fits(mvd_engine_t* e, size_t* act_bytes_out) {
  const size_t act_bytes = (e->act.high + 255) & ~size_t(255);
  if (!e->ws_ptr || act_bytes + e->tmp.high > (size_t)e->ws_bytes) {
    mvd_set_error("forward: workspace too small: need %zu bytes, bound %lld", act_bytes + e->tmp.high, (long long)e->ws_bytes);
    return -4;
  }
  *act_bytes_out = act_bytes;
  return 0;
}

// A ragged layout gets the device tables of its slot (mvd_engine::kv_slots), uploaded from its host tables on first use
static int kv_slot_tables(mvd_engine_t* e, ViewLayout* host, hipStream_t st) {
  const ViewLayout& lay = *host;
  const int O = lay.objects, n = lay.g * lay.rows;
  std::vector<int> layout(lay.counts, lay.counts + O); layout.push_back(lay.g);
  mvd_engine::KvSlot* slot = nullptr;
  for (auto& sl : e->kv_slots) if (sl.layout == layout) slot = &sl;
  if (!slot) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (st && hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
      mvd_set_error("forward_ragged: the first forward of a layout uploads its K/V tables and cannot run inside a stream capture"); return -7;
    }
    if (e->kv_slots.size() >= mvd_engine::KV_SLOTS) {
      // no room: the least recently used slot goes -- after every captured graph (one of them may point at it) and after the
      // device has finished whatever still reads it (hipFree synchronises)
      e->drop_graphs();
      size_t lru = 0;
      for (size_t i = 1; i < e->kv_slots.size(); ++i) if (e->kv_slots[i].used < e->kv_slots[lru].used) lru = i;
      if (e->kv_slots[lru].dev) (void)hipFree(e->kv_slots[lru].dev);
      e->kv_slots.erase(e->kv_slots.begin() + lru);
    }
    mvd_engine::KvSlot sl;
    sl.layout = layout;
    sl.host.assign(lay.kvi_ref, lay.kvi_ref + (size_t)2 * n);          // [adapter | text], as ragged_layout built them
    // (valid by construction; they pass the same host check as a caller's table all the same before they are uploaded)
    if (mvd_attention_check_index(sl.host.data(), n, lay.g * O) || mvd_attention_check_index(sl.host.data() + n, n, lay.g * O)) return -1;
    if (hipMalloc((void**)&sl.dev, sl.host.size() * sizeof(int)) != hipSuccess) { mvd_set_error("forward_ragged: hipMalloc of the K/V tables failed"); return -3; }
    e->kv_slots.push_back(std::move(sl));
    slot = &e->kv_slots.back();
    if (hipMemcpyAsync(slot->dev, slot->host.data(), slot->host.size() * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess) {
      (void)hipFree(slot->dev); e->kv_slots.pop_back();
      mvd_set_error("forward_ragged: upload of the K/V tables failed"); return -3;
    }
  }
  slot->used = ++e->kv_tick;
  *host = lay.with_tables(slot->dev);
  return 0;
}

// The three forward entries.  `host`: the layout as its entry built it -- a ragged one with HOST tables, which size the call; the
// launches read the device tables of its slot, which is touched only once the call has passed every check and fits its workspace.
static int unet_forward_issue(mvd_engine_t* e, const mvd_forward_args_t* args, const ViewLayout& host, void* stream) {
  if (!e || !args) { mvd_set_error("forward: null argument"); return -1; }
  if (args->flags & MVD_REF_ONLY_INTERNAL) { mvd_set_error("forward: unknown flag bits 0x%x", args->flags); return -1; }
  // size the two arenas for this shape with a dry run (pure host arithmetic), then run for real
  const mvd_engine::HostState before = e->host_state();
  int r = forward_impl(e, *args, nullptr, true, host);
  e->set_host_state(before);
  if (r) return r;
  size_t act_bytes = 0;
  if ((r = workspace_fits(e, &act_bytes))) return r;
  hipStream_t st = (hipStream_t)stream;
  ViewLayout lay = host;
  if (host.counts && (r = kv_slot_tables(e, &lay, st))) return r;
  // (a refresh forward that has passed every check overwrites the stored deep feature: unet_forward writes its record afterwards)
  if (args->flags & MVD_DEEPCACHE_REFRESH) e->dc_rec.valid = false;
  e->act.base = (char*)e->ws_ptr; e->act.cap = act_bytes;
  e->tmp.base = (char*)e->ws_ptr + act_bytes; e->tmp.cap = (size_t)e->ws_bytes - act_bytes;
  if (!e->graph_on || e->prof || !st) return forward_impl(e, *args, st, false, lay);
  // ---- hipGraph replay.  A forward is a pure function of the argument block (pointers, shapes, flags), its layout, the bound
  // buffers and the reference-cache state it starts from; the host-side state it leaves behind is the same every time.  The
  // first call with a given key runs as usual (kernels' first-use set-up must not happen inside a capture), the second is
  // captured and instantiated, later ones are one hipGraphLaunch.
  std::string key((const char*)args, sizeof(*args));
  const int st6[6] = {e->rc_valid, e->rc_batch, e->rc_h, e->rc_w, e->rc_keep, e->share_encoder};
  key.append((const char*)st6, sizeof(st6));
  // (the layout of this call -- objects, views, counts, g, the slot its tables live in -- and the one the cached reference was encoded under)
  const std::vector<int> lk = lay.key();
  key.append((const char*)lk.data(), lk.size() * sizeof(int));
  key.append((const char*)&lay.g, sizeof(int));
  key.append((const char*)&lay.kvi_ref, sizeof(void*));
  key.push_back('|');
  key.append((const char*)e->rc_layout.data(), e->rc_layout.size() * sizeof(int));
  key.push_back('|');
  key.append((const char*)&e->ws_ptr, sizeof(void*));
  key.append((const char*)&e->rc_ptr, sizeof(void*));
  for (auto& ge : e->graphs)
    if (ge.key == key) {
      hipError_t he = hipGraphLaunch(ge.x, st);
      if (he != hipSuccess) { mvd_set_error("forward: hipGraphLaunch: %s", hipGetErrorString(he)); return -7; }
      e->set_host_state(ge.after);        // (same key => the captured run started from this state and ended in that one)
      return 0;
    }
  bool seen = false;
  for (auto& k : e->graph_seen) seen |= k == key;
  if (!seen) { e->graph_seen.push_back(key); return forward_impl(e, *args, st, false, lay); }
  if (e->graphs.size() >= 8) e->drop_graphs();
  hipError_t he = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
  if (he != hipSuccess) { mvd_set_error("forward: hipStreamBeginCapture: %s", hipGetErrorString(he)); return -7; }
  r = forward_impl(e, *args, st, false, lay);
  hipGraph_t g = nullptr;
  he = hipStreamEndCapture(st, &g);
  if (r) { if (g) (void)hipGraphDestroy(g); return r; }
  if (he != hipSuccess || !g) { mvd_set_error("forward: hipStreamEndCapture: %s", hipGetErrorString(he)); return -7; }
  hipGraphExec_t x = nullptr;
  he = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
  if (he != hipSuccess) { (void)hipGraphDestroy(g); mvd_set_error("forward: hipGraphInstantiate: %s", hipGetErrorString(he)); return -7; }
  e->graphs.push_back({key, g, x, e->host_state()});
  he = hipGraphLaunch(x, st);
  if (he != hipSuccess) { mvd_set_error("forward: hipGraphLaunch: %s", hipGetErrorString(he)); return -7; }
  return 0;
}

// The record of the stored deep feature follows the forward that wrote it, however that forward was issued (launched, captured,
// replayed): it is host state of the engine beside the graphs' HostState (see mvd_engine::dc_rec)
static int unet_forward(mvd_engine_t* e, const mvd_forward_args_t* args, const ViewLayout& host, void* stream) {
  const int r = unet_forward_issue(e, args, host, stream);
  if (!r && (args->flags & MVD_DEEPCACHE_REFRESH)) {
    mvd_engine::DeepRecord& d = e->dc_rec;
    d.batch = args->batch; d.h = args->height; d.w = args->width; d.layout = host.key();
    d.cam = (args->flags & MVD_USE_CAMERA) ? 1 : 0; d.img = (args->flags & MVD_USE_IMAGE) ? 1 : 0;
    d.branch = e->opt.dc_branch; d.wgen = e->weight_gen; d.valid = true;
  }
  return r;
}

int mvd_unet_forward(mvd_engine_t* e, const mvd_forward_args_t* args, void* stream) { return unet_forward(e, args, uniform_layout(args, 0), stream); }
int mvd_unet_forward_objects(mvd_engine_t* e, const mvd_forward_args_t* args, int objects, void* stream) {
  return unet_forward(e, args, uniform_layout(args, objects), stream);
}

// ---- ragged view counts (include/mvd_hip.h): the counts' own rules, then the layout.  Equal counts ARE the objects forward (one object:
// the views forward): *a is the call with `views` set.  Counts that differ: *a is the call as it came, `tab` the layout's two host tables.
static int ragged_layout(const mvd_forward_args_t* args, const int* view_counts, int objects, mvd_forward_args_t* a, std::vector<int>* tab, ViewLayout* lay) {
  if (!args || !view_counts || objects < 1) { mvd_set_error("forward_ragged: null argument or %d objects", objects); return -1; }
  if (args->views != 0) { mvd_set_error("forward_ragged: args->views must be 0 (the view counts come beside the arguments), got %d", args->views); return -1; }
  const int R = mvd_ragged_rows(view_counts, objects);
  if (R < 0) { mvd_set_error("forward_ragged: every object needs at least one view (the counts must be >= 1 and their sum must fit an int)"); return -1; }
  if (args->batch <= 0 || args->batch % R || args->batch / R > 2) {
    mvd_set_error("forward_ragged: batch %d is not 1 or 2 (classifier-free guidance) rows for each of the %d views", args->batch, R); return -1;
  }
  const int g = args->batch / R;
  *a = *args;
  bool uniform = true;
  for (int o = 1; o < objects; ++o) uniform &= view_counts[o] == view_counts[0];
  if (uniform) { a->views = view_counts[0]; *lay = uniform_layout(a, objects); return 0; }
  tab->resize((size_t)2 * g * R);
  mvd_ragged_build_tables(view_counts, objects, g, tab->data(), tab->data() + (size_t)g * R);
  *lay = ViewLayout::ragged(view_counts, objects, g, R, tab->data());
  return 0;
}

int64_t mvd_engine_workspace_bytes_ragged(mvd_engine_t* e, const mvd_forward_args_t* args, const int* view_counts, int objects) {
  if (!e) { mvd_set_error("workspace_bytes_ragged: null engine"); return -1; }
  mvd_forward_args_t a; std::vector<int> tab; ViewLayout lay;
  if (ragged_layout(args, view_counts, objects, &a, &tab, &lay)) return -1;
  return workspace_bytes_args(e, &a, lay);
}

int mvd_unet_forward_ragged(mvd_engine_t* e, const mvd_forward_args_t* args, const int* view_counts, int objects, void* stream) {
  if (!e) { mvd_set_error("forward_ragged: null engine"); return -1; }
  mvd_forward_args_t a; std::vector<int> tab; ViewLayout lay;
  if (ragged_layout(args, view_counts, objects, &a, &tab, &lay)) return -1;
  return unet_forward(e, &a, lay, stream);
}

int mvd_engine_set_graph(mvd_engine_t* e, int enable) {
  if (!e) { mvd_set_error("set_graph: null engine"); return -1; }
  e->graph_on = enable != 0;
  if (!e->graph_on) e->drop_graphs();
  return 0;
}

int mvd_engine_set_profiling(mvd_engine_t* e, int enable) {
  if (!e) { mvd_set_error("set_profiling: null engine"); return -1; }
  // 1: one stream, launches back to back (serial kernel times); 2: the forward's own schedule (the encoder pass on the side
  // stream): durations of launches that share the chip with the other pass's -- what rocprofv3 sees in the timed region
  e->prof = enable != 0; e->prof_overlap = enable == 2; e->prof_recs.clear(); e->ev_used = 0;
  return 0;
}

// Sums the recorded launches per kernel class (after synchronising the last event) and resets the records.
// Arrays hold `cap` entries; returns the number of classes written (<0 on error).
int mvd_engine_profile_summary(mvd_engine_t* e, int cap, int* cls, int* launches, double* ms, double* flops, double* bytes) {
  if (!e || cap <= 0 || !cls || !launches || !ms || !flops || !bytes) { mvd_set_error("profile_summary: bad argument"); return -1; }
  int n = 0;
  for (auto& r : e->prof_recs) {
    if (hipEventSynchronize(r.e1) != hipSuccess) { mvd_set_error("profile_summary: event sync failed"); return -2; }
    float t = 0.f;
    if (hipEventElapsedTime(&t, r.e0, r.e1) != hipSuccess) { mvd_set_error("profile_summary: elapsed time failed"); return -2; }
    int j = 0;
    while (j < n && cls[j] != r.cls) ++j;
    if (j == n) { if (n == cap) continue; cls[n] = r.cls; launches[n] = 0; ms[n] = 0; flops[n] = 0; bytes[n] = 0; ++n; }
    launches[j] += 1; ms[j] += t; flops[j] += r.flops; bytes[j] += r.bytes;
  }
  e->prof_recs.clear(); e->ev_used = 0;
  return n;
}

int mvd_engine_profile_shapes(mvd_engine_t* e, char* buf, int cap) {
  if (!e || !buf || cap <= 0) { mvd_set_error("profile_shapes: bad argument"); return -1; }
  struct Acc { int cls, M, N, K, tag, n; double ms, fl; };
  std::vector<Acc> v;
  for (auto& r : e->prof_recs) {
    if (hipEventSynchronize(r.e1) != hipSuccess) { mvd_set_error("profile_shapes: event sync failed"); return -2; }
    float t = 0.f; (void)hipEventElapsedTime(&t, r.e0, r.e1);
    size_t j = 0;
    while (j < v.size() && !(v[j].cls == r.cls && v[j].M == r.M && v[j].N == r.N && v[j].K == r.K && v[j].tag == r.tag)) ++j;
    if (j == v.size()) v.push_back({r.cls, r.M, r.N, r.K, r.tag, 0, 0.0, 0.0});
    v[j].n++; v[j].ms += t; v[j].fl += r.flops;
  }
  int off = 0;
  for (auto& x : v) {
    const int w = snprintf(buf + off, (size_t)(cap - off), "cls=%d M=%d N=%d K=%d tag=%d launches=%d ms=%.3f tflops=%.0f\n", x.cls, x.M, x.N, x.K,
                           x.tag, x.n, x.ms, x.ms > 0 ? x.fl / x.ms / 1e9 : 0.0);
    if (w < 0 || off + w >= cap) break;
    off += w;
  }
  return off;
}

int mvd_engine_share_encoder_weights(mvd_engine_t* e, int enable) {
  if (e) e->drop_graphs();
  if (!e) { mvd_set_error("share_encoder_weights: null engine"); return -1; }
  e->share_encoder = enable != 0;
  return 0;
}

// The main-pass options (include/mvd_hip.h "main-pass options: what setting or clearing one invalidates").  The only code that assigns
// e->opt: every setter and clearer below builds `next` from e->opt and names the option it changes.  A refused call changes nothing.
static int apply_main_opts(mvd_engine* e, const MainOpts& next, MainOptField what) {
  // token merging and token downsampling are alternatives (only one of the two changes per call: the other's state is e->opt's)
  if (what == OPT_TOME && next.merges() && next.downsamples()) { mvd_set_error("set_tome: token downsampling is set (factors %d, %d): the two are alternatives, clear it first (mvd_engine_clear_todo)", next.todo_f[0], next.todo_f[1]); return -1; }
  if (what == OPT_TODO && next.merges() && next.downsamples()) { mvd_set_error("set_todo: token merging is set (ratio %g): the two are alternatives, clear it first (mvd_engine_clear_tome)", next.tome_ratio); return -1; }
  // what a change of each option invalidates beside the captured graphs, which every one drops (a graph captured under one setting is
  // never replayed under another).  FreeU and token merging leave a stored deep feature valid: recorded as found.
  static const struct { bool dc_rec, tome_tab, todo_nk, taps; } invalidates[] = {
    /* OPT_FREEU     */ {false, false, false, false},
    /* OPT_TOME      */ {false, true,  false, false},
    /* OPT_TODO      */ {true,  false, true,  false},
    /* OPT_DEEPCACHE */ {true,  false, false, false},
    /* OPT_TAPS      */ {false, false, false, true},
  };
  e->drop_graphs();
  if (invalidates[what].dc_rec) e->dc_rec.valid = false;
  if (invalidates[what].tome_tab) e->tome_tab.clear();
  if (invalidates[what].todo_nk) e->todo_nk.clear();
  if (invalidates[what].taps) e->taps.clear();
  e->opt = next;
  return 0;
}

int mvd_engine_set_freeu(mvd_engine_t* e, float s1, float s2, float b1, float b2) {
  if (!e) { mvd_set_error("set_freeu: null engine"); return -1; }
  const float v[4] = {s1, s2, b1, b2};
  for (float x : v) if (!(x > 0.f) || !(x < INFINITY)) { mvd_set_error("set_freeu: s1, s2, b1, b2 must be positive and finite, got %g, %g, %g, %g", (double)s1, (double)s2, (double)b1, (double)b2); return -1; }
  MainOpts next = e->opt; next.freeu_on = true; next.freeu_s[0] = s1; next.freeu_s[1] = s2; next.freeu_b[0] = b1; next.freeu_b[1] = b2;
  return apply_main_opts(e, next, OPT_FREEU);
}
int mvd_engine_clear_freeu(mvd_engine_t* e) {
  if (!e) { mvd_set_error("clear_freeu: null engine"); return -1; }
  MainOpts next = e->opt; next.freeu_on = false;
  return apply_main_opts(e, next, OPT_FREEU);
}

int mvd_engine_set_tome(mvd_engine_t* e, double ratio, int max_downsample, int keep_tables) {
  if (!e) { mvd_set_error("set_tome: null engine"); return -1; }
  if (!(ratio >= 0.0) || !(ratio <= 0.75)) { mvd_set_error("set_tome: ratio must lie in [0, 0.75] (a quarter of the tokens are dst and stay), got %g", ratio); return -1; }
  if (max_downsample != 1 && max_downsample != 2 && max_downsample != 4 && max_downsample != 8) { mvd_set_error("set_tome: max_downsample must be one of 1, 2, 4, 8, got %d", max_downsample); return -1; }
  MainOpts next = e->opt; next.tome_ratio = ratio; next.tome_maxds = max_downsample; next.tome_keep = keep_tables != 0;
  return apply_main_opts(e, next, OPT_TOME);
}
int mvd_engine_clear_tome(mvd_engine_t* e) {
  if (!e) { mvd_set_error("clear_tome: null engine"); return -1; }
  MainOpts next = e->opt; next.tome_ratio = 0.0; next.tome_maxds = 1; next.tome_keep = false;
  return apply_main_opts(e, next, OPT_TOME);
}
int64_t mvd_engine_tome_table(mvd_engine_t* e, int feature_idx, int* out, void* stream) {
  if (!e || feature_idx < 0 || feature_idx >= (int)e->feats.size()) { mvd_set_error("tome_table: bad argument"); return -1; }
  if (!e->opt.tome_keep) { mvd_set_error("tome_table: tables are not kept (mvd_engine_set_tome with keep_tables)"); return -1; }
  if (feature_idx >= (int)e->tome_tab.size() || !e->tome_tab[feature_idx].p) return 0;
  const auto& t = e->tome_tab[feature_idx];
  if (out && hipMemcpyAsync(out, t.p, (size_t)t.n * sizeof(int), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) { mvd_set_error("tome_table: copy failed"); return -3; }
  return t.n;
}

int mvd_engine_set_todo(mvd_engine_t* e, int factor, int factor_level_2, int method) {
  if (!e) { mvd_set_error("set_todo: null engine"); return -1; }
  if (factor < 1 || factor > 4 || factor_level_2 < 1 || factor_level_2 > 4) { mvd_set_error("set_todo: factor and factor_level_2 must lie in [1, 4], got %d and %d", factor, factor_level_2); return -1; }
  if (method != 0 && method != 1) { mvd_set_error("set_todo: the method is 0 (nearest) or 1 (area), got %d", method); return -1; }
  MainOpts next = e->opt; next.todo_f[0] = factor; next.todo_f[1] = factor_level_2; next.todo_method = method;
  return apply_main_opts(e, next, OPT_TODO);
}
int mvd_engine_clear_todo(mvd_engine_t* e) {
  if (!e) { mvd_set_error("clear_todo: null engine"); return -1; }
  MainOpts next = e->opt; next.todo_f[0] = next.todo_f[1] = 1; next.todo_method = 0;
  return apply_main_opts(e, next, OPT_TODO);
}
int mvd_engine_todo_keys(mvd_engine_t* e, int* out, int n) {
  if (!e || !out || n < 0) { mvd_set_error("todo_keys: bad argument"); return -1; }
  const int nf = (int)e->feats.size();
  for (int i = 0; i < n && i < nf; ++i) out[i] = i < (int)e->todo_nk.size() ? e->todo_nk[i] : 0;
  return nf;
}

// (binding a buffer changes no option, but a graph's nodes hold the buffer's address and the stored feature lies in it: it takes
//  DeepCache's row of the table)
int mvd_engine_set_deepcache(mvd_engine_t* e, int branch) {
  if (!e) { mvd_set_error("set_deepcache: null engine"); return -1; }
  if (branch < 0 || branch >= e->cfg.layers_per_block) { mvd_set_error("set_deepcache: branch %d outside [0, %d) (layers_per_block)", branch, e->cfg.layers_per_block); return -1; }
  MainOpts next = e->opt; next.dc_on = true; next.dc_branch = branch;
  return apply_main_opts(e, next, OPT_DEEPCACHE);
}
int mvd_engine_clear_deepcache(mvd_engine_t* e) {
  if (!e) { mvd_set_error("clear_deepcache: null engine"); return -1; }
  MainOpts next = e->opt; next.dc_on = false; next.dc_branch = 0;
  return apply_main_opts(e, next, OPT_DEEPCACHE);
}
int64_t mvd_engine_deepcache_bytes(mvd_engine_t* e, int batch, int height, int width) {
  if (!e || batch <= 0 || height <= 0 || width <= 0) { mvd_set_error("deepcache_bytes: bad argument"); return -1; }
  // (any branch: the wider of the two channel counts a deep feature can have)
  const int c = e->cfg.block_out_channels[0] > e->cfg.block_out_channels[1] ? e->cfg.block_out_channels[0] : e->cfg.block_out_channels[1];
  return (((int64_t)batch * height * width * c * (int64_t)sizeof(bf16_t)) + 255) & ~(int64_t)255;
}
int mvd_engine_bind_deepcache(mvd_engine_t* e, void* ptr, int64_t bytes) {
  if (e) (void)apply_main_opts(e, e->opt, OPT_DEEPCACHE);
  if (!e || (ptr && bytes <= 0)) { mvd_set_error("bind_deepcache: bad argument"); return -1; }
  if ((uintptr_t)ptr & 255) { mvd_set_error("bind_deepcache: the buffer must be 256-byte aligned"); return -1; }
  e->dc_ptr = ptr; e->dc_bytes = ptr ? bytes : 0;
  return 0;
}

int mvd_engine_set_taps(mvd_engine_t* e, int enable) {
  if (!e) { mvd_set_error("set_taps: null engine"); return -1; }
  MainOpts next = e->opt; next.taps_on = enable != 0;
  return apply_main_opts(e, next, OPT_TAPS);
}
int mvd_engine_num_taps(mvd_engine_t* e) {
  if (!e) { mvd_set_error("num_taps: null engine"); return -1; }
  if (!e->opt.taps_on) { mvd_set_error("num_taps: taps are not kept (mvd_engine_set_taps)"); return -1; }
  return (int)e->taps.size();
}
int mvd_engine_tap_info(mvd_engine_t* e, int idx, char* name, int cap, int* batch, int* channels, int* height, int* width) {
  if (!e || !name || cap <= 0 || !batch || !channels || !height || !width) { mvd_set_error("tap_info: bad argument"); return -1; }
  if (!e->opt.taps_on || idx < 0 || idx >= (int)e->taps.size()) { mvd_set_error("tap_info: no tap %d (%d kept; mvd_engine_set_taps, then a forward)", idx, e->opt.taps_on ? (int)e->taps.size() : 0); return -1; }
  const mvd_engine::Tap& t = e->taps[idx];
  if ((int)t.name.size() >= cap) { mvd_set_error("tap_info: the name '%s' needs %d bytes, the buffer has %d", t.name.c_str(), (int)t.name.size() + 1, cap); return -1; }
  memcpy(name, t.name.c_str(), t.name.size() + 1);
  *batch = t.B; *channels = t.C; *height = t.H; *width = t.W;
  return 0;
}
int mvd_engine_get_tap(mvd_engine_t* e, int idx, float* out_nchw, void* stream) {
  if (!e || !out_nchw) { mvd_set_error("get_tap: bad argument"); return -1; }
  if (!e->opt.taps_on || idx < 0 || idx >= (int)e->taps.size()) { mvd_set_error("get_tap: no tap %d (%d kept; mvd_engine_set_taps, then a forward)", idx, e->opt.taps_on ? (int)e->taps.size() : 0); return -1; }
  const mvd_engine::Tap& t = e->taps[idx];
  return mvd_launch_nhwc_to_nchw_f32(t.p, t.B, t.H * t.W, t.C, out_nchw, (hipStream_t)stream);
}

int mvd_engine_num_features(mvd_engine_t* e) { return e ? (int)e->feats.size() : -1; }
int mvd_engine_feature_shape(mvd_engine_t* e, int idx, int* channels, int* height, int* width) {
  if (!e || idx < 0 || idx >= (int)e->feats.size() || !e->rc_h) { mvd_set_error("feature_shape: bad index or no reference pass yet"); return -1; }
  *channels = e->feats[idx].C; *height = e->rc_h >> e->feats[idx].level; *width = e->rc_w >> e->feats[idx].level;
  return 0;
}
int mvd_engine_get_feature(mvd_engine_t* e, int idx, float* out_nchw, void* stream) {
  if (!e || idx < 0 || idx >= (int)e->feats.size() || !out_nchw) { mvd_set_error("get_feature: bad argument"); return -1; }
  if (!e->rc_valid || !e->rc_keep || !e->feat_keep[idx]) { mvd_set_error("get_feature: no kept features (run forward with MVD_KEEP_FEATURES)"); return -1; }
  const int lv = e->feats[idx].level;
  return mvd_launch_nhwc_to_nchw_f32(e->feat_keep[idx], e->rc_batch, (e->rc_h >> lv) * (e->rc_w >> lv), e->feats[idx].C, out_nchw, (hipStream_t)stream);
}
// Standalone CameraEncoder.encode_cameras (camera_encoder.py:160-176) through the engine's kernels.
int mvd_engine_encode_cameras(mvd_engine_t* e, const float* source_camera, const float* target_camera, int cam_rows,
                              int batch, const float* fourier_proj, float* out_emb, void* stream) {
  if (!e || !source_camera || !target_camera || !fourier_proj || !out_emb || batch <= 0 || (cam_rows != 3 && cam_rows != 4)) { mvd_set_error("encode_cameras: bad argument"); return -1; }
  if (!e->ws_ptr) { mvd_set_error("encode_cameras: workspace not bound"); return -1; }
  {   // size the scratch with a dry pass: nothing is launched into a workspace that is too small
    e->tmp.reset(true);
    Ctx d{e, nullptr, 0, true};
    if (int r = camera_embed(d, source_camera, target_camera, cam_rows, fourier_proj, batch, out_emb)) return r;
    if (e->tmp.high > (size_t)e->ws_bytes) { mvd_set_error("encode_cameras: workspace too small (%zu > %lld bytes)", e->tmp.high, (long long)e->ws_bytes); return -4; }
  }
  e->tmp.reset(false); e->tmp.base = (char*)e->ws_ptr; e->tmp.cap = (size_t)e->ws_bytes;
  Ctx c{e, (hipStream_t)stream, 0, false};
  return camera_embed(c, source_camera, target_camera, cam_rows, fourier_proj, batch, out_emb);
}

// Standalone CameraEncoder.apply_modulation_to_tensor (camera_encoder.py:207-255) on an NCHW fp32 tensor.
// Unknown modulator names are the identity (returns 1 and leaves `out` untouched), like the reference.
int mvd_engine_apply_modulation(mvd_engine_t* e, const char* name, const float* emb, int batch, const float* x_nchw,
                                int channels, int hw, float* out_nchw, void* stream) {
  if (!e || !name || !emb || !x_nchw || !out_nchw || batch <= 0 || channels <= 0 || hw <= 0) { mvd_set_error("apply_modulation: bad argument"); return -1; }
  if (!e->ws_ptr) { mvd_set_error("apply_modulation: workspace not bound"); return -1; }
  int dim = -1;
  for (auto& m : modulator_dims(e->cfg, true)) if (m.first == name) dim = m.second;
  if (dim < 0) return 1;
  if (dim != channels) { mvd_set_error("apply_modulation: modulator '%s' has %d channels, tensor has %d", name, dim, channels); return -1; }
  {   // dry sizing pass first (see encode_cameras)
    e->tmp.reset(true);
    Ctx d{e, nullptr, 0, true};
    float* sc0 = d.talloc<float>((size_t)batch * dim);
    float* sh0 = d.talloc<float>((size_t)batch * dim);
    if (int r = modulator(d, name, dim, emb, batch, sc0, sh0)) return r;
    if (e->tmp.high > (size_t)e->ws_bytes) { mvd_set_error("apply_modulation: workspace too small (%zu > %lld bytes)", e->tmp.high, (long long)e->ws_bytes); return -4; }
  }
  e->tmp.reset(false); e->tmp.base = (char*)e->ws_ptr; e->tmp.cap = (size_t)e->ws_bytes;
  Ctx c{e, (hipStream_t)stream, 0, false};
  float* sc = c.talloc<float>((size_t)batch * dim);
  float* sh = c.talloc<float>((size_t)batch * dim);
  if (int r = modulator(c, name, dim, emb, batch, sc, sh)) return r;
  return mvd_launch_film_nchw_f32(x_nchw, batch, channels, hw, sc, sh, out_nchw, (hipStream_t)stream);
}

int mvd_engine_get_camera_embedding(mvd_engine_t* e, float* out, void* stream) {
  if (!e || !out || !e->cam_emb) { mvd_set_error("get_camera_embedding: no camera pass yet"); return -1; }
  return (int)hipMemcpyAsync(out, e->cam_emb, (size_t)e->cam_batch * e->cfg.cam_output_dim * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream);
}

// Both arenas of a stand-alone entry that runs forward code: sized by the dry pass that precedes it, laid out like unet_forward's.
static int bind_standalone_arenas(mvd_engine_t* e) {
  size_t act_bytes = 0;
  if (int r = workspace_fits(e, &act_bytes)) return r;
  e->act.reset(false); e->act.base = (char*)e->ws_ptr; e->act.cap = act_bytes;
  e->tmp.reset(false); e->tmp.base = (char*)e->ws_ptr + act_bytes; e->tmp.cap = (size_t)e->ws_bytes - act_bytes;
  return 0;
}

// Stand-alone FiLM parameters of every hooked modulator, through the function the forward's camera path runs.
int mvd_engine_film_params(mvd_engine_t* e, const float* emb, int cam_batch, int out_rows, float* out, void* stream) {
  if (!e || !emb || !out || cam_batch <= 0 || out_rows < cam_batch) { mvd_set_error("film_params: bad argument"); return -1; }
  if (!e->ws_ptr) { mvd_set_error("film_params: workspace not bound"); return -1; }
  std::unordered_map<std::string, std::pair<float*, float*>> ss;
  const bool concat = e->w[0].has("cam.modcat.w0");
  {   // dry sizing pass first (see encode_cameras)
    e->tmp.reset(true); e->act.reset(true);
    Ctx d{e, nullptr, 0, true};
    if (int r = film_params_all(d, emb, cam_batch, out_rows, ss, concat)) return r;
  }
  if (int r = bind_standalone_arenas(e)) return r;
  Ctx c{e, (hipStream_t)stream, 0, false};
  ss.clear();
  if (int r = film_params_all(c, emb, cam_batch, out_rows, ss, concat)) return r;
  for (auto& m : modulator_dims(e->cfg, false)) {   // the engine's layout: per modulator scale [out_rows][dim] | shift [out_rows][dim]
    const size_t n = (size_t)out_rows * m.second;
    const auto& p = ss[m.first];
    if (hipMemcpyAsync(out, p.first, n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess ||
        hipMemcpyAsync(out + n, p.second, n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) { mvd_set_error("film_params: hipMemcpyAsync failed"); return -3; }
    out += 2 * n;
  }
  return 0;
}

// Stand-alone time path (weight set 0): timesteps [batch] -> out [batch][temb_total], every resnet's time_emb_proj output.
int mvd_engine_time_projection(mvd_engine_t* e, const float* timesteps, int batch, float* out, void* stream) {
  if (!e || !timesteps || !out || batch <= 0) { mvd_set_error("time_projection: bad argument"); return -1; }
  if (!e->ws_ptr) { mvd_set_error("time_projection: workspace not bound"); return -1; }
  const float* tproj = nullptr;
  for (int dry = 1; dry >= 0; --dry) {   // dry sizing pass first (see encode_cameras)
    if (dry) { e->tmp.reset(true); e->act.reset(true); }
    else if (int r = bind_standalone_arenas(e)) return r;
    Ctx c{e, dry ? nullptr : (hipStream_t)stream, 0, dry != 0};
    if (int r = setup_tile_counters(e, (unsigned int*)e->act.alloc(MVD_TILE_COUNTERS * sizeof(unsigned int)), c.s, c.dry)) return r;
    if (int r = time_path(c, timesteps, batch, &tproj)) return r;
  }
  if (hipMemcpyAsync(out, tproj, (size_t)batch * e->temb_total * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) { mvd_set_error("time_projection: hipMemcpyAsync failed"); return -3; }
  return 0;
}

// ------------------------------------------------------------------ operator-level entry points
// small-M kernels with split-K (force_cfg >= 100): the tile counters live behind the partials in the caller's split-K
// workspace (MVD_OP_SPLITK_COUNTERS extra 4-byte words, zeroed here per call); the kernel combines the slices itself
static int op_sm_splitk(MvdGemmArgs& g, hipStream_t s, int force_cfg) {
  g.tile_cnt = reinterpret_cast<unsigned int*>(g.part + (size_t)g.splitk * g.M * g.N);
  hipError_t e = hipMemsetAsync(g.tile_cnt, 0, MVD_OP_SPLITK_COUNTERS * sizeof(unsigned int), s);
  if (e != hipSuccess) { mvd_set_error("op split-K: hipMemsetAsync: %s", hipGetErrorString(e)); return -3; }
  if ((long)((g.M + 63) / 64) * (g.N / 64) > MVD_OP_SPLITK_COUNTERS) { mvd_set_error("op split-K: more than %d output tiles", MVD_OP_SPLITK_COUNTERS); return -1; }
  return mvd_launch_gemm(g, s, force_cfg);
}
// splitk <= 1: the caller DECIDED not to split (g.splitk = 1; 0 would mean "undecided": the tile heuristic may then assume a
// deep split)
static int op_launch(MvdGemmArgs& g, int force_cfg, int splitk, float* splitk_ws, hipStream_t s) {
  g.part = splitk_ws;      // (also the stamp buffer of probe builds)
  g.splitk = splitk > 1 ? splitk : 1;
  if (splitk > 1 && force_cfg >= 100) return op_sm_splitk(g, s, force_cfg);
  return launch_tiled(g, s, force_cfg);
}
int mvd_op_linear(const void* a, const void* a2, int k1, int k2, const void* w, const float* bias, const float* rowvec,
                  int ld_rowvec, int rows_per_batch, const void* res, float alpha, int geglu, void* out, int out_f32, int m,
                  int n, int force_cfg, int splitk, float* splitk_ws, void* stream) {
  const int on = geglu ? n / 2 : n;
  MvdGemmArgs g = gemm_dense((const bf16_t*)a, (const bf16_t*)a2, k1, k2, m, (const bf16_t*)w, 0, bias, n, out, on);
  if (rows_per_batch > 0) g.rows_per_batch = g.outW = rows_per_batch;
  g.rowvec = rowvec; g.ld_rowvec = ld_rowvec; g.res = (const bf16_t*)res; g.ldres = on; g.alpha = alpha; g.geglu = geglu; g.out_f32 = out_f32;
  return op_launch(g, force_cfg, splitk, splitk_ws, (hipStream_t)stream);
}
// the same with the leading dimensions the engine's call sites use: a weight read with a row stride ldw >= k1 + k2 (a packed
// [o_self | o_ref] out-projection with the adapter off), res / out as column slices of wider buffers, res == out (in place)
int mvd_op_linear_ld(const void* a, const void* a2, int k1, int k2, const void* w, int ldw, const float* bias, const float* rowvec,
                     int ld_rowvec, int rows_per_batch, const void* res, int ldres, float alpha, int geglu, void* out, int ldo,
                     int out_f32, int m, int n, int force_cfg, int splitk, float* splitk_ws, void* stream) {
  const int on = geglu ? n / 2 : n;
  if (!a || !w || !out || m <= 0 || n <= 0 || k1 <= 0 || k2 < 0) { mvd_set_error("mvd_op_linear_ld: bad argument"); return -1; }
  if (ldw < k1 + k2 || ldo < on || (res && ldres < on)) { mvd_set_error("mvd_op_linear_ld: a leading dimension is shorter than its row (ldw=%d ldres=%d ldo=%d)", ldw, ldres, ldo); return -1; }
  if (splitk > 1 && !splitk_ws) { mvd_set_error("mvd_op_linear_ld: split-K needs a workspace"); return -1; }
  MvdGemmArgs g = gemm_dense((const bf16_t*)a, (const bf16_t*)a2, k1, k2, m, (const bf16_t*)w, ldw, bias, n, out, ldo);
  if (rows_per_batch > 0) g.rows_per_batch = g.outW = rows_per_batch;
  g.rowvec = rowvec; g.ld_rowvec = ld_rowvec; g.res = (const bf16_t*)res; g.ldres = ldres; g.alpha = alpha; g.geglu = geglu; g.out_f32 = out_f32;
  return op_launch(g, force_cfg, splitk, splitk_ws, (hipStream_t)stream);
}

int mvd_op_ln_linear(const void* x, int k, const void* w_folded, const float* c1, const float* c2, float eps, int geglu,
                     void* out, int m, int n, void* stream) {
  MvdGemmArgs g = gemm_dense((const bf16_t*)x, nullptr, k, 0, m, (const bf16_t*)w_folded, 0, c2, n, out, geglu ? n / 2 : n);
  g.ln_c1 = c1; g.ln_eps = eps; g.geglu = geglu; g.ldres = g.ldo;
  if (!c1 || !c2) { mvd_set_error("mvd_op_ln_linear: c1 and c2 are required"); return -1; }
  if (!mvd_gemm_ln_fold_ok(g)) {
    int tile = 0, ns = 0, S = 1;           // small problems (batch 1): the fold of the small-M kernels
    if (mvd_gemm_sm_plan(g, &tile, &ns, &S) && S == 1) {
      g_mvd_last_gemm.cfg = 100 + 10 * tile + ns; g_mvd_last_gemm.splitk = 1;    // as mvd_launch_gemm records a forced small-M launch
      return mvd_launch_gemm_sm(g, (hipStream_t)stream, tile, ns);
    }
    mvd_set_error("mvd_op_ln_linear: M=%d N=%d K=%d geglu=%d is not a shape of the fused LayerNorm GEMMs", m, n, k, geglu);
    return -1;
  }
  return mvd_launch_gemm(g, (hipStream_t)stream);
}

int mvd_op_conv3x3(const void* x, int batch, int in_h, int in_w, int cin, int stride, int upsample, int asym_pad, const void* w,
                   const float* bias, const float* rowvec, int ld_rowvec, const void* res, const void* sc, const void* sc2,
                   int sc_c1, int sc_c2, void* out, int cout, int force_cfg, int splitk, float* splitk_ws, void* stream) {
  const int oh = upsample ? in_h * 2 : (stride == 2 ? (in_h + 1) / 2 : in_h);
  const int ow = upsample ? in_w * 2 : (stride == 2 ? (in_w + 1) / 2 : in_w);
  MvdGemmArgs g = gemm_conv3((const bf16_t*)x, in_h, in_w, cin, stride, upsample, asym_pad, (const bf16_t*)sc, (const bf16_t*)sc2, sc_c1, sc_c2,
                             (const bf16_t*)w, bias, batch, oh, ow, cout, out);
  g.rowvec = rowvec; g.ld_rowvec = ld_rowvec; g.res = (const bf16_t*)res;
  return op_launch(g, force_cfg, splitk, splitk_ws, (hipStream_t)stream);
}

// the upsampling convolution as four 2x2 sub-pixel convolutions (w4 = packing.pack_up4: [4][cout][4 * cin] bf16); an error --
// never another kernel -- for a problem the mode does not take (mvd_gemm_pp_up4_applicable)
int mvd_op_conv3x3_up4(const void* x, int batch, int in_h, int in_w, int cin, const void* w4, const float* bias, void* out, int cout,
                       int force_cfg, void* stream) {
  if (!x || !w4 || !out || batch <= 0 || in_h <= 0 || in_w <= 0 || cin <= 0 || cout <= 0) { mvd_set_error("mvd_op_conv3x3_up4: bad argument"); return -1; }
  MvdGemmArgs g = gemm_conv3((const bf16_t*)x, in_h, in_w, cin, 1, 1, 0, nullptr, nullptr, 0, 0, (const bf16_t*)w4, bias, batch, 2 * in_h, 2 * in_w,
                             cout, out);
  gemm_conv3_to_up4(g);
  g.splitk = 1;
  return mvd_launch_gemm(g, (hipStream_t)stream, force_cfg);
}

int mvd_op_attention(const void* q, const void* k, const void* v, void* o, int batch, int heads, int nq, int nk, int ldq,
                     int ldk, int ldv, int ldo, float scale, void* stream) {
  MvdAttnArgs a; memset(&a, 0, sizeof(a));
  a.nprob = 1; a.batch = batch; a.heads = heads; a.scale = scale;
  a.prescaled = scale == 0.f;   // q already carries softmax_scale * log2(e)
  a.p[0] = {(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o, ldq, ldk, ldv, ldo,
            (int64_t)nq * ldq, (int64_t)nk * ldk, (int64_t)nk * ldv, (int64_t)nq * ldo, nq, nk};
  return mvd_launch_attention(a, (hipStream_t)stream);
}

int mvd_op_attention_grouped(const void* q, const void* k, const void* v, void* o, int batch, int heads, int nq, int nk, int ldq,
                             int ldk, int ldv, int ldo, float scale, int kv_group, void* stream) {
  return mvd_op_attention_objects(q, k, v, o, batch, heads, nq, nk, ldq, ldk, ldv, ldo, scale, kv_group, 0, stream);
}

int mvd_op_attention_objects(const void* q, const void* k, const void* v, void* o, int batch, int heads, int nq, int nk, int ldq,
                             int ldk, int ldv, int ldo, float scale, int kv_group, int kv_objects, void* stream) {
  MvdAttnArgs a; memset(&a, 0, sizeof(a));
  a.nprob = 1; a.batch = batch; a.heads = heads; a.scale = scale;
  a.prescaled = scale == 0.f;
  a.p[0] = {(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o, ldq, ldk, ldv, ldo,
            (int64_t)nq * ldq, (int64_t)nk * ldk, (int64_t)nk * ldv, (int64_t)nq * ldo, nq, nk};
  a.kv_group[0] = kv_group; a.kv_objects[0] = kv_objects;
  return mvd_launch_attention(a, (hipStream_t)stream);
}

// split-KV form of mvd_op_attention (prescaled queries only: scale == 0): ws = mvd_op_attention_split_ws_bytes(...) bytes
// (partials + the arrival counters, which the call zeroes)
int64_t mvd_op_attention_split_ws_bytes(int batch, int heads, int nq, int nsplit) {
  MvdAttnArgs a; memset(&a, 0, sizeof(a));
  a.nprob = 1; a.batch = batch; a.heads = heads; a.p[0].nq = nq;
  return (int64_t)mvd_attention_split_ws_bytes(a, nsplit) + (int64_t)mvd_attention_split_counters(a) * 4 + 256;
}
// One library-owned device buffer for the operator entries' tables (grow-only; growing frees the old one, which synchronises): two
// regions of g_op_kvi_cap entries, one per problem of a launch (region 1 starts at g_op_kvi + g_op_kvi_cap).  The
// upload is stream-ordered in front of the launch; calls on one stream are ordered among themselves
static int* g_op_kvi = nullptr; static size_t g_op_kvi_cap = 0; static std::mutex g_op_kvi_mu;
// (under g_op_kvi_mu) both regions hold at least n entries; 0, or -3 with mvd_set_error
static int op_kvi_reserve(size_t n) {
  if (n <= g_op_kvi_cap) return 0;
  if (g_op_kvi) (void)hipFree(g_op_kvi);
  g_op_kvi = nullptr; g_op_kvi_cap = 0;
  const size_t cap = n < 256 ? 256 : n;
  if (hipMalloc((void**)&g_op_kvi, 2 * cap * sizeof(int)) != hipSuccess) { mvd_set_error("attention: hipMalloc of the K/V table failed"); return -3; }
  g_op_kvi_cap = cap;
  return 0;
}
static int attention_mapped(const void* q, const void* k, const void* v, void* o, int batch, int heads, int nq, int nk, int ldq, int ldk,
                            int ldv, int ldo, float scale, int kv_group, int kv_objects, const int* kv_index_host, int kv_elements,
                            void* stream) {
  if (batch <= 0) { mvd_set_error("attention: bad problem count/batch/heads"); return -1; }
  // before anything is uploaded or launched: the entries, and a table together with a group (mvd_launch_attention's own rule)
  if (mvd_attention_check_index(kv_index_host, batch, kv_elements)) return -1;
  if (kv_group > 1 || kv_objects > 1) { mvd_set_error("attention: problem 0 sets a K/V table together with K/V group %d / objects %d", kv_group, kv_objects); return -1; }
  MvdAttnArgs a; memset(&a, 0, sizeof(a));
  a.nprob = 1; a.batch = batch; a.heads = heads; a.scale = scale;
  a.prescaled = scale == 0.f;
  a.p[0] = {(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o, ldq, ldk, ldv, ldo,
            (int64_t)nq * ldq, (int64_t)nk * ldk, (int64_t)nk * ldv, (int64_t)nq * ldo, nq, nk};
  std::lock_guard<std::mutex> lk(g_op_kvi_mu);
  if (op_kvi_reserve((size_t)batch)) return -3;
  // (pageable source: the call returns once the table has been read)
  if (hipMemcpyAsync(g_op_kvi, kv_index_host, (size_t)batch * sizeof(int), hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess) { mvd_set_error("attention: upload of the K/V table failed"); return -3; }
  a.kv_index[0] = g_op_kvi; a.kv_group[0] = kv_group; a.kv_objects[0] = kv_objects;
  return mvd_launch_attention(a, (hipStream_t)stream);
}
int mvd_op_attention_mapped(const void* q, const void* k, const void* v, void* o, int batch, int heads, int nq, int nk, int ldq,
                            int ldk, int ldv, int ldo, float scale, const int* kv_index_host, int kv_elements, void* stream) {
  return attention_mapped(q, k, v, o, batch, heads, nq, nk, ldq, ldk, ldv, ldo, scale, 0, 0, kv_index_host, kv_elements, stream);
}
// test hook: the same entry with a group beside the table -- a combination the host rejects
extern "C" int mvd_debug_attention_mapped_grouped(const void* q, const void* k, const void* v, void* o, int batch, int heads, int nq, int nk,
                                                  int ldq, int ldk, int ldv, int ldo, float scale, int kv_group, int kv_objects,
                                                  const int* kv_index_host, int kv_elements, void* stream) {
  return attention_mapped(q, k, v, o, batch, heads, nq, nk, ldq, ldk, ldv, ldo, scale, kv_group, kv_objects, kv_index_host, kv_elements, stream);
}

// test hook: ONE launch of two problems, as transformer() issues them for an image-conditioned block (MvdAttnArgs::nprob = 2) --
// the arguments go into one MvdAttnArgs and to mvd_launch_attention, no other path.  ptrs = {q0, k0, v0, o0, q1, k1, v1, o1};
// dims = per problem MVD_PAIR_DIMS ints {nq, nk, ldq, ldk, ldv, ldo, kv_group, kv_objects, kv_elements}; table0 / table1: null, or
// `batch` host entries naming one of that problem's kv_elements K/V elements.  Batch strides are n * ld.  scale == 0: the
// prescaled engine form.  nsplit: 1 off, 2..8 forced, 0 = mvd_attention_pick_split on these arguments.
enum { MVD_PAIR_DIMS = 9 };
static int pair_args(MvdAttnArgs& a, const void* const* ptrs, const int* dims, int batch, int heads, float scale) {
  if (!dims || batch <= 0 || heads <= 0) { mvd_set_error("attention: bad problem count/batch/heads"); return -1; }
  memset(&a, 0, sizeof(a));
  a.nprob = 2; a.batch = batch; a.heads = heads; a.scale = scale;
  a.prescaled = scale == 0.f;
  for (int i = 0; i < 2; ++i) {
    const int* d = dims + i * MVD_PAIR_DIMS;
    const int nq = d[0], nk = d[1], ldq = d[2], ldk = d[3], ldv = d[4], ldo = d[5];
    if (ptrs) a.p[i] = {(const bf16_t*)ptrs[4 * i], (const bf16_t*)ptrs[4 * i + 1], (const bf16_t*)ptrs[4 * i + 2], (bf16_t*)ptrs[4 * i + 3]};
    a.p[i].ldq = ldq; a.p[i].ldk = ldk; a.p[i].ldv = ldv; a.p[i].ldo = ldo;
    a.p[i].bsq = (int64_t)nq * ldq; a.p[i].bsk = (int64_t)nk * ldk; a.p[i].bsv = (int64_t)nk * ldv; a.p[i].bso = (int64_t)nq * ldo;
    a.p[i].nq = nq; a.p[i].nk = nk;
    a.kv_group[i] = d[6]; a.kv_objects[i] = d[7];
  }
  return 0;
}
// the split this launch gets (nsplit == 0: the engine's heuristic, which never splits a launch with a table)
static int pair_split(MvdAttnArgs& a, const int* table0, const int* table1, int nsplit) {
  if (nsplit) return nsplit;
  a.kv_index[0] = table0; a.kv_index[1] = table1;       // (host pointers: the heuristic only tests them)
  const int ns = mvd_attention_pick_split(a);
  a.kv_index[0] = a.kv_index[1] = nullptr;
  return ns;
}
// bytes of the workspace of such a launch: the partials, then the arrival counters (which the call zeroes); 0 without a split
extern "C" int64_t mvd_debug_attention_pair_ws_bytes(const int* dims, const int* table0, const int* table1, int batch, int heads,
                                                     float scale, int nsplit) {
  MvdAttnArgs a;
  if (pair_args(a, nullptr, dims, batch, heads, scale)) return -1;
  const int ns = pair_split(a, table0, table1, nsplit);
  if (ns <= 1) return 0;
  return (int64_t)((mvd_attention_split_ws_bytes(a, ns) + 255) & ~size_t(255)) + (int64_t)mvd_attention_split_counters(a) * 4 + 256;
}
extern "C" int mvd_debug_attention_pair(const void* const* ptrs, const int* dims, const int* table0, const int* table1, int batch,
                                        int heads, float scale, int nsplit, void* ws, void* stream) {
  MvdAttnArgs a;
  if (!ptrs) { mvd_set_error("attention_pair: null argument"); return -1; }
  if (pair_args(a, ptrs, dims, batch, heads, scale)) return -1;
  // before anything is uploaded or launched: the entries, and a table together with a group (mvd_launch_attention's own rule)
  const int* tables[2] = {table0, table1};
  for (int i = 0; i < 2; ++i) {
    if (!tables[i]) continue;
    if (mvd_attention_check_index(tables[i], batch, dims[i * MVD_PAIR_DIMS + 8])) return -1;
    if (a.kv_group[i] > 1 || a.kv_objects[i] > 1) { mvd_set_error("attention: problem %d sets a K/V table together with K/V group %d / objects %d", i, a.kv_group[i], a.kv_objects[i]); return -1; }
  }
  const int ns = pair_split(a, table0, table1, nsplit);
  if (ns > 1) {     // (a split the launcher refuses -- more than 8 ranges, a null workspace ... -- goes to the launcher as it is)
    a.nsplit = ns; a.split_ws = ws;
    if (ws && ns <= 8) {
      const size_t pb = (mvd_attention_split_ws_bytes(a, ns) + 255) & ~size_t(255);
      a.split_cnt = reinterpret_cast<unsigned int*>(reinterpret_cast<char*>(ws) + pb);
    }
  }
  std::unique_lock<std::mutex> lk(g_op_kvi_mu, std::defer_lock);
  if (table0 || table1) {
    lk.lock();
    if (op_kvi_reserve((size_t)batch)) return -3;
    for (int i = 0; i < 2; ++i) {
      if (!tables[i]) continue;
      int* dst = g_op_kvi + (size_t)i * g_op_kvi_cap;
      if (hipMemcpyAsync(dst, tables[i], (size_t)batch * sizeof(int), hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess) { mvd_set_error("attention: upload of the K/V table failed"); return -3; }
      a.kv_index[i] = dst;
    }
  }
  if (a.split_cnt && hipMemsetAsync(a.split_cnt, 0, (size_t)mvd_attention_split_counters(a) * 4, (hipStream_t)stream) != hipSuccess) { mvd_set_error("attention_pair: hipMemsetAsync failed"); return -3; }
  return mvd_launch_attention(a, (hipStream_t)stream);
}

// measurement / test hook: the two tables the engine builds for a ragged layout (host arrays of g * sum(counts) entries);
// returns the number of entries, or -1
extern "C" int mvd_debug_ragged_tables(const int* view_counts, int objects, int g, int* adapter, int* text) {
  if (!view_counts || !adapter || !text || objects < 1 || g < 1 || g > 2) { mvd_set_error("ragged_tables: bad argument"); return -1; }
  const int R = mvd_ragged_rows(view_counts, objects);
  if (R < 0) { mvd_set_error("ragged_tables: every object needs at least one view"); return -1; }
  mvd_ragged_build_tables(view_counts, objects, g, adapter, text);
  if (mvd_attention_check_index(adapter, g * R, g * objects) || mvd_attention_check_index(text, g * R, g * objects)) return -1;
  return g * R;
}

int mvd_op_attention_split(const void* q, const void* k, const void* v, void* o, int batch, int heads, int nq, int nk, int ldq,
                           int ldk, int ldv, int ldo, int nsplit, void* ws, void* stream) {
  MvdAttnArgs a; memset(&a, 0, sizeof(a));
  a.nprob = 1; a.batch = batch; a.heads = heads; a.scale = 0.f; a.prescaled = 1;
  a.p[0] = {(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o, ldq, ldk, ldv, ldo,
            (int64_t)nq * ldq, (int64_t)nk * ldk, (int64_t)nk * ldv, (int64_t)nq * ldo, nq, nk};
  if (nsplit > 1) {
    if (!ws) { mvd_set_error("op_attention_split: null workspace"); return -1; }
    const size_t pb = (mvd_attention_split_ws_bytes(a, nsplit) + 255) & ~size_t(255);
    a.nsplit = nsplit; a.split_ws = ws; a.split_cnt = reinterpret_cast<unsigned int*>(reinterpret_cast<char*>(ws) + pb);
    if (hipMemsetAsync(a.split_cnt, 0, (size_t)mvd_attention_split_counters(a) * 4, (hipStream_t)stream) != hipSuccess) { mvd_set_error("op_attention_split: hipMemsetAsync failed"); return -3; }
  }
  return mvd_launch_attention(a, (hipStream_t)stream);
}

int mvd_op_groupnorm(const void* x0, const void* x1, int c0, int c1, int batch, int hw, int groups, float eps,
                     const float* gamma, const float* beta, int silu, void* y, float* ws, void* stream) {
  return mvd_launch_groupnorm((const bf16_t*)x0, (const bf16_t*)x1, c0, c1, batch, hw, groups, eps, gamma, beta, silu, (bf16_t*)y, ws, (hipStream_t)stream);
}
int mvd_op_layernorm(const void* x, int rows, int c, float eps, const float* gamma, const float* beta, void* y, void* stream) {
  return mvd_launch_layernorm((const bf16_t*)x, rows, c, eps, gamma, beta, (bf16_t*)y, (hipStream_t)stream);
}
int mvd_op_refnorm(const void* x, int batch, int hw, int c, void* y, void* stream) {
  return mvd_launch_refnorm((const bf16_t*)x, batch, hw, c, (bf16_t*)y, (hipStream_t)stream);
}
int mvd_op_refnorm_grouped(const void* x, int batch, int group, int hw, int c, void* y, void* stream) {
  return mvd_launch_refnorm_grouped((const bf16_t*)x, batch, group, hw, c, (bf16_t*)y, (hipStream_t)stream);
}
int mvd_op_film(const void* x, int batch, int hw, int c, const float* scale, const float* shift, void* y, void* stream) {
  return mvd_launch_film((const bf16_t*)x, batch, hw, c, scale, shift, c, (bf16_t*)y, (hipStream_t)stream);
}
int mvd_op_conv_in(const void* x, int batch, int h, int w, int cin, const float* wt, const float* bias, int cout, void* y, void* stream) {
  return mvd_launch_conv_in((const bf16_t*)x, batch, h, w, cin, wt, bias, cout, (bf16_t*)y, (hipStream_t)stream);
}
int mvd_op_conv_out(const void* x, int batch, int h, int w, int c, const void* wt, const float* bias, int cout, float* y, void* stream) {
  return mvd_launch_conv_out((const bf16_t*)x, batch, h, w, c, (const bf16_t*)wt, bias, cout, y, (hipStream_t)stream);
}
int mvd_op_nchw_to_nhwc(const float* x, int batch, int c, int hw, const float* scale, const float* shift, void* y, void* stream) {
  return mvd_launch_nchw_to_nhwc(x, batch, c, hw, scale, shift, c, (bf16_t*)y, (hipStream_t)stream);
}
int mvd_op_nhwc_to_nchw(const void* x, int batch, int hw, int c, float* y, void* stream) {
  return mvd_launch_nhwc_to_nchw_f32((const bf16_t*)x, batch, hw, c, y, (hipStream_t)stream);
}
int mvd_op_f32_to_bf16(const float* x, int64_t n, void* y, void* stream) {
  return mvd_launch_f32_to_bf16(x, n, (bf16_t*)y, (hipStream_t)stream);
}
// the fp32 linear layer of the camera / time MLPs: y[b][o] = sum_k act(x[b][k]) W[o][k] + bias[o]  (W fp32, or bf16 with wbf16 = 1;
// act_in = 1: SiLU on the inputs)
int mvd_op_skinny_linear(const float* x, int ldx, int batch, int k, const void* w, int wbf16, const float* bias, int n, int act_in,
                         float* y, int ldy, void* stream) {
  return mvd_launch_skinny_linear(x, ldx, batch, k, w, wbf16, bias, n, act_in, y, ldy, (hipStream_t)stream);
}
/* the remaining kernels of the fp32 camera / time conditioning path, one launcher each (the launchers check the arguments) */
int mvd_op_timestep_embedding(const float* t, int batch, int dim, float* y, void* stream) {
  return mvd_launch_timestep_embedding(t, batch, dim, y, (hipStream_t)stream);
}
int mvd_op_camera_features(const float* src, const float* tgt, int batch, int cam_rows, int nfreq, float max_freq, float* rflat, float* enc,
                           void* stream) {
  return mvd_launch_camera_features(src, tgt, batch, cam_rows, nfreq, max_freq, rflat, enc, (hipStream_t)stream);
}
int mvd_op_layernorm_f32(const float* x, int rows, int c, float eps, const float* gamma, const float* beta, int silu, int nseg, float* y,
                         void* stream) {
  return mvd_launch_layernorm_f32(x, rows, c, eps, gamma, beta, silu, y, (hipStream_t)stream, nseg);
}
static int op_seg_table(const int* seg_end, int nseg, MvdSegTable* seg, const char* what) {
  if (!seg_end || nseg < 1 || nseg > 16) { mvd_set_error("%s: 1..16 segment ends", what); return -1; }
  memset(seg, 0, sizeof(*seg));
  seg->n = nseg;
  for (int g = 0; g < nseg; ++g) {
    if (seg_end[g] <= (g ? seg_end[g - 1] : 0)) { mvd_set_error("%s: segment ends must increase", what); return -1; }
    seg->end[g] = seg_end[g];
  }
  return 0;
}
int mvd_op_skinny_linear_grouped(const float* x, int ldx, int xseg, int batch, int k, const float* w, const float* bias, int n,
                                 const int* seg_end, int nseg, float* y, int ldy, void* stream) {
  MvdSegTable seg;
  if (int r = op_seg_table(seg_end, nseg, &seg, "skinny_linear_grouped")) return r;
  return mvd_launch_skinny_linear_grouped(x, ldx, xseg, batch, k, w, bias, n, seg, y, ldy, (hipStream_t)stream);
}
int mvd_op_film_params(const float* raw, int batch, int dim, float strength, float* scale, float* shift, int out_rows, void* stream) {
  return mvd_launch_film_params(raw, batch, dim, strength, scale, shift, out_rows, (hipStream_t)stream);
}
int mvd_op_film_params_grouped(const float* raw, int batch, const int* seg_end, int nseg, float strength, float* out, int out_rows,
                               void* stream) {
  MvdSegTable seg;
  if (int r = op_seg_table(seg_end, nseg, &seg, "film_params_grouped")) return r;
  return mvd_launch_film_params_grouped(raw, batch, seg, strength, out, out_rows, (hipStream_t)stream);
}
int mvd_op_im2col_in(const float* x, int batch, int c, int h, int w, const float* scale, const float* shift, int ld_ss, void* y,
                     void* stream) {
  return mvd_launch_im2col_in(x, batch, c, h, w, scale, shift, ld_ss, (bf16_t*)y, (hipStream_t)stream);
}
int mvd_op_film_nchw_f32(const float* x, int batch, int c, int hw, const float* scale, const float* shift, float* y, void* stream) {
  return mvd_launch_film_nchw_f32(x, batch, c, hw, scale, shift, y, (hipStream_t)stream);
}

}  // extern "C"
