// Ragged turntables: the row maps of a forward of O objects with V_o views each.  Host code only, no
// HIP: what builds the K/V tables the attention kernel reads unchecked can be compiled and run by itself.
#pragma once
#include <limits.h>

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
