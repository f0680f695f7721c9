// The batch layout of a forward: how the rows of the main batch map to objects, reference, text and
// camera rows -- an ordinary forward, V views of one object, O objects x V views, or O objects with V_o views each.  Host code only, no
// HIP: what validates a call and builds the K/V tables the attention kernel reads unchecked can be compiled and run by itself.
#pragma once
#include <limits.h>
#include <stdio.h>
#include <vector>

// R = sum of the counts; -1 when a count is < 1 or g * R could overflow an int (g <= 2)
inline int mvd_ragged_rows(const int* counts, int objects) {
  long long r = 0;
  for (int o = 0; o < objects; ++o) {
    if (counts[o] < 1) return -1;
    r += counts[o];
    if (r > INT_MAX / 2) return -1;
  }
  return objects > 0 ? (int)r : -1;
}

// The main batch holds g * R rows [half j][object o][view v]: row r = j * R + c with c = (views of the objects before o) + v.
//   adapter[r] = o * g + j   element of the reference K/V [object][half] (O * g elements, as the ref_kv GEMM writes them)
//   text[r]    = j * O + o   row of the text K/V [negative x O | positive x O]
// Both are < g * O by construction.
inline void mvd_ragged_build_tables(const int* counts, int objects, int g, int* adapter, int* text) {
  const int R = mvd_ragged_rows(counts, objects);
  for (int j = 0; j < g; ++j) {
    int c = 0;
    for (int o = 0; o < objects; ++o)
      for (int v = 0; v < counts[o]; ++v, ++c) {
        adapter[(long long)j * R + c] = o * g + j;
        text[(long long)j * R + c] = j * objects + o;
      }
  }
}

struct ViewLayout {
  int objects = 0;              // O > 1 objects (0: one object, or an ordinary forward)
  int views = 0;                // the uniform V of an MVD_SHARE_REF forward; 0 when the counts differ, and in an ordinary forward
  const int* counts = nullptr;  // ragged only: O view counts that differ, rows = R = their sum, g rows per view
  int g = 0, rows = 0;
  // ragged only: tables of g * R entries (kernels.h MvdAttnArgs::kv_index) -- row r reads reference K/V element kvi_ref[r] of the
  // g * O elements [object][half] and text row kvi_text[r].  Device memory (a slot of the engine) in a forward that launches; host
  // memory in a sizing pass, which dereferences neither.  Uniform layouts keep the kernel's arithmetic map: null.
  const int* kvi_ref = nullptr; const int* kvi_text = nullptr;

  // mvd_unet_forward / mvd_unet_forward_objects: objects <= 1 IS the call without it, messages included
  static ViewLayout uniform(int objects, int views, bool share) { ViewLayout l; l.objects = objects > 1 ? objects : 0; l.views = share ? views : 0; return l; }
  // mvd_unet_forward_ragged: O >= 2 objects with counts that differ (equal counts take uniform()), [adapter | text] tables
  static ViewLayout ragged(const int* counts, int objects, int g, int rows, const int* tables) { ViewLayout l; l.objects = objects; l.counts = counts; l.g = g; l.rows = rows; return l.with_tables(tables); }
  ViewLayout with_tables(const int* t) const { ViewLayout l = *this; l.kvi_ref = t; l.kvi_text = t + (size_t)g * rows; return l; }

  int text_rows(int B) const { return counts ? g * objects : (views ? B / views : B); }   // = elements of the reference K/V: one per half (and object)
  bool per_object_stats() const { return objects > 1; }     // encoder pass: Q2 statistics per object
  // the K/V map of one attention problem (kv_group[i], kv_objects[i], kv_index[i] of an MvdAttnArgs): the adapter's reference K/V
  // [object][half], or the text K/V, which hold one row per half and object in the batch's own order (no object map)
  void fill_map(bool adapter, int* kv_group, int* kv_objects, const int** kv_index) const {
    *kv_group = counts ? 0 : views; *kv_objects = adapter && !counts ? objects : 0; *kv_index = adapter ? kvi_ref : kvi_text;
  }
  // What the cached reference is bound to (MVD_REUSE_REF needs an equal one): objects, views and the counts that differ -- not g
  std::vector<int> key() const { std::vector<int> k{objects, views}; if (counts) k.insert(k.end(), counts, counts + objects); return k; }

  // Every rule of a shared forward (`share`: MVD_SHARE_REF is set; cam_batch INT_MIN: no camera conditioning), in one order for the three
  // entries, each in its own words (tests pin them): w = 0 mvd_unet_forward, 1 _objects, 2 _ragged.  0, or -1 with the message.
  int validate(bool share, bool use_img, int batch, int ref_batch, int cam_batch, int height, int width, int levels, char* msg, size_t cap) const {
    if (!share && !objects && !counts) return 0;                  // an ordinary forward
    const int O = objects, w = counts ? 2 : O ? 1 : 0;
    static const char* const pre[3] = {"forward: MVD_SHARE_REF:", "forward_objects:", "forward_ragged:"};
    static const char* const cams[3] = {"views", "objects x views", "sum of the view counts"};
    const long long R = counts ? rows : (long long)(O ? O : 1) * views;
    const int G = R >= 1 && R <= INT_MAX && batch % R == 0 && (!counts || batch / R == g) ? (int)(batch / R) : 0;   // rows per view; 0: none
#define MVD_LAYOUT_REJECT(...) return (snprintf(msg, cap, __VA_ARGS__), -1)
    if (!share || !use_img) {
      if (w == 2) MVD_LAYOUT_REJECT("forward_ragged: view counts need MVD_SHARE_REF with MVD_USE_IMAGE");
      if (w == 1) MVD_LAYOUT_REJECT("forward_objects: objects = %d needs MVD_SHARE_REF with MVD_USE_IMAGE", O);
      MVD_LAYOUT_REJECT("forward: MVD_SHARE_REF needs MVD_USE_IMAGE");
    }
    if (w == 2 && (G < 1 || G > 2)) MVD_LAYOUT_REJECT("forward_ragged: batch %d is not 1 or 2 (classifier-free guidance) rows for each of the %d views", batch, rows);
    if (w == 1 && !G) MVD_LAYOUT_REJECT("forward_objects: batch %d is not a multiple of objects %d x views %d", batch, O, views);
    if (w == 1 && G > 2) MVD_LAYOUT_REJECT("forward_objects: %d rows per view (batch %d / (objects %d x views %d)); 1 or 2 (classifier-free guidance) are supported", G, batch, O, views);
    if (w == 0 && !G) MVD_LAYOUT_REJECT("forward: MVD_SHARE_REF: batch %d is not a multiple of views %d", batch, views);
    if (w == 0 && G > 2) MVD_LAYOUT_REJECT("forward: MVD_SHARE_REF: %d rows per view (batch %d / views %d); 1 or 2 (classifier-free guidance) are supported", G, batch, views);
    if (w == 0 && ref_batch != 1) MVD_LAYOUT_REJECT("forward: MVD_SHARE_REF needs ref_batch == 1 (one object), got %d", ref_batch);
    if (w != 0 && ref_batch != O) MVD_LAYOUT_REJECT("%s needs ref_batch == objects = %d (one reference row per object), got %d", pre[w], O, ref_batch);
    if (cam_batch != INT_MIN && cam_batch != 1 && cam_batch != R) MVD_LAYOUT_REJECT("%s the cameras must hold 1 or %s = %d rows, got %d", pre[w], cams[w], (int)R, cam_batch);
    for (int lv = 0; lv < levels; ++lv) {
      const long long hw = (long long)(height >> lv) * (width >> lv);
      if (hw % G) MVD_LAYOUT_REJECT("%s the %lld reference tokens of level %d do not divide over %d rows per view", pre[w], hw, lv, G);
    }
#undef MVD_LAYOUT_REJECT
    return 0;
  }
};
