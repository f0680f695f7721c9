// Image front end of the data loader: what the reference's dataset does to every decoded render on the
// host with PIL (src/data/objaverse_dataset.py:279-294 and :259-266), on the device.
//
//   composite  RGBA over opaque white, Pillow's Image.alpha_composite followed by convert("RGB") (channels == 4 only)
//   resize     Pillow's 8-bit two-pass resample with the LANCZOS filter: horizontal pass -> uint8 -> vertical pass -> uint8
//   normalise  float(byte) / 127.5f - 1.0f, the two fp32 operations of `tensor.float() / 127.5 - 1.0`
//
// Everything up to the bytes is integer arithmetic, so the output equals PIL's byte for byte; the normalisation is two
// correctly rounded fp32 operations, so it equals the CPU's bit for bit.
//
// Two launches.  imgfe_h_kernel: a workgroup owns HS_COLS output columns of HS_ROWS source rows (one row per wave); it loads
// the source span of those columns with 16-byte loads (four RGBA pixels per lane), composites every source pixel ONCE (not
// once per tap: 13 taps at scale 2), keeps the three planes in LDS, runs the horizontal taps from LDS and writes the planar
// uint8 intermediate -- only the source rows the vertical pass reads.  imgfe_v_kernel: lanes run along out_w, four adjacent
// columns of all three planes per lane, so every tap row is one coalesced dword read per plane and a lane ends with whole
// 16-byte fp32 stores (store16 of bufaddr.h) and one 12-byte uint8 store.  No atomics: two calls give the same bits.
#include <math.h>

#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "bufaddr.h"
#include "host_util.h"

namespace {

// ---------------------------------------------------------------- Pillow's resampling coefficients, on the host
// Pillow (Resample.c, precompute_coeffs + normalize_coeffs_8bpc): per output position xx of a pass in -> out with
// scale = in / out, filterscale = max(scale, 1), support = 3 * filterscale (the Lanczos filter's support is 3):
//   center = (xx + 0.5) * scale;  xmin = max(int(center - support + 0.5), 0);  xmax = min(int(center + support + 0.5), in)
//   w[x] = lanczos((x + xmin - center + 0.5) / filterscale), summed in order in double, then w[x] /= sum
//   kk[x] = int(+-0.5 + w[x] * 2^22)        (the sign of the 0.5 is the sign of w[x]; truncation towards zero)
// The accumulator of an output byte starts at 2^21, is shifted right by 22 and clipped to [0, 255].  A pass whose sizes are
// equal is skipped.
constexpr int PRECISION_BITS = 32 - 8 - 2;
constexpr double LANCZOS_SUPPORT = 3.0;
constexpr double PI = 3.14159265358979323846;

double sinc_filter(double x) {
  if (x == 0.0) return 1.0;
  x = x * PI;
  return sin(x) / x;
}
double lanczos_filter(double x) {            // truncated sinc: sinc(x) sinc(x / 3) on -3 <= x < 3
  if (-3.0 <= x && x < 3.0) return sinc_filter(x) * sinc_filter(x / 3);
  return 0.0;
}

struct PassTable {
  int in = 0, out = 0, ksize = 0;
  std::vector<int> kk, lo, cnt;              // kk [out][ksize]
  bool skipped() const { return in == out; }
};
int pass_ksize(int in, int out) {
  const double scale = (double)in / out;
  return (int)ceil(LANCZOS_SUPPORT * (scale < 1.0 ? 1.0 : scale)) * 2 + 1;
}
int build_pass(int in, int out, PassTable* t) {
  t->in = in; t->out = out; t->ksize = 0;
  t->kk.clear(); t->lo.clear(); t->cnt.clear();
  if (in == out) return 0;
  const double scale = (double)in / out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = LANCZOS_SUPPORT * fs;
  const int ksize = pass_ksize(in, out);
  t->ksize = ksize;
  t->kk.assign((size_t)out * ksize, 0);
  t->lo.resize(out); t->cnt.resize(out);
  std::vector<double> k(ksize);
  const double ss = 1.0 / fs;
  for (int xx = 0; xx < out; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) { const double w = lanczos_filter((x + xmin - center + 0.5) * ss); k[x] = w; ww += w; }
    long worst = 0;
    for (int x = 0; x < xmax; ++x) {
      if (ww != 0.0) k[x] /= ww;
      const int q = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << PRECISION_BITS)) : (int)(0.5 + k[x] * (1 << PRECISION_BITS));
      t->kk[(size_t)xx * ksize + x] = q;
      worst += q < 0 ? -(long)q : (long)q;
    }
    // the accumulator is a 32-bit integer: 2^21 + 255 * sum |kk| must stay below 2^31
    if (255 * worst + (1L << (PRECISION_BITS - 1)) >= (1L << 31)) { mvd_set_error("image_frontend: resampling weights overflow 32 bits (%d -> %d)", in, out); return -1; }
    t->lo[xx] = xmin; t->cnt[xx] = xmax;
  }
  return 0;
}

// ---------------------------------------------------------------- tile sizes (mvd_op_image_frontend_spans reports them)
constexpr int HS_COLS = 64;     // output columns of one workgroup of the horizontal kernel (one per lane)
constexpr int HS_ROWS = 4;      // source rows of that workgroup (one per wave)
constexpr int HS_SPAN = 640;    // source pixels of one row an LDS plane holds: 64 columns up to scale ~9.1
constexpr int VS_COLS = 256;    // output columns of one workgroup of the vertical kernel (four per lane)
constexpr int VS_ROWS = 4;      // output rows of that workgroup (one per wave)

// One geometry: the tables as one int32 blob, laid out for the kernels --
//   [kkT_h [ksize_h][ow] | xmin [ow] | xcnt [ow] | kk_v [oh][ksize_v] | ymin [oh] | ycnt [oh]]
// (the horizontal weights tap-major: lane = output column, so a tap is one coalesced read; the vertical weights row-major:
// an output row is wave-uniform, so its taps are scalar loads).  `pinned` is the page-locked copy the uploads read
// (null: none yet, or the MAX_PINNED copies are taken).
struct Geometry {
  PassTable hp, vp;
  std::vector<int> blob;
  size_t off_h = 0, off_v = 0;
  int row0 = 0, nrows = 0;      // the source rows the vertical pass reads: [row0, row0 + nrows)
  int* pinned = nullptr;
};
using GeoKey = std::tuple<int, int, int, int>;
std::mutex g_mu;
std::map<GeoKey, Geometry> g_geo;            // (h, w, out_h, out_w) -> host tables, built once, kept for the life of the process
constexpr int MAX_PINNED = 64;               // geometries that keep a page-locked copy (each at most a few hundred KB)
int g_pinned = 0;                            // (under g_mu, like every access to `pinned`)

size_t table_bytes(int h, int w, int oh, int ow) {
  size_t n = 0;
  if (w != ow) n += (size_t)ow * (pass_ksize(w, ow) + 2);
  if (h != oh) n += (size_t)oh * (pass_ksize(h, oh) + 2);
  return align256(n * 4 + 16);
}
int pitch_of(int ow) { return (ow + 15) & ~15; }

int check_shape(const char* who, int batch, int h, int w, int channels, int oh, int ow) {
  if (batch < 1 || batch > 4096 || h < 1 || w < 1 || oh < 1 || ow < 1 || h > 16384 || w > 16384 || oh > 16384 || ow > 16384) { mvd_set_error("%s: bad shape (batch %d, %d x %d -> %d x %d)", who, batch, h, w, oh, ow); return -1; }
  if (channels != 3 && channels != 4) { mvd_set_error("%s: channels %d (3 = RGB, 4 = RGBA)", who, channels); return -1; }
  const long lim = 1L << 31;
  if ((long)batch * h * w * channels + 16 >= lim || (long)batch * 3 * h * pitch_of(ow) >= lim || (long)batch * 3 * oh * ow * 4 >= lim) { mvd_set_error("%s: batch %d of %d x %d -> %d x %d is beyond what one call takes (2^31 bytes per buffer)", who, batch, h, w, oh, ow); return -1; }
  return 0;
}

// the geometry's tables (built on first use); null with the error set
const Geometry* geometry(int h, int w, int oh, int ow) {
  std::lock_guard<std::mutex> lock(g_mu);
  const GeoKey key{h, w, oh, ow};
  auto it = g_geo.find(key);
  if (it != g_geo.end()) return &it->second;
  Geometry g;
  if (build_pass(w, ow, &g.hp) || build_pass(h, oh, &g.vp)) return nullptr;
  if (!g.hp.skipped()) {
    // a workgroup's source span (+ up to 3 pixels in front and behind for the 16-byte chunks) must fit an LDS plane row
    for (int x0 = 0; x0 < ow; x0 += HS_COLS) {
      const int x1 = x0 + HS_COLS < ow ? x0 + HS_COLS : ow;
      const int span = g.hp.lo[x1 - 1] + g.hp.cnt[x1 - 1] - g.hp.lo[x0];
      if (span + 6 > HS_SPAN) { mvd_set_error("image_frontend: width %d -> %d: %d output columns read %d source pixels, more than the %d a workgroup stages (scale above %.1f)", w, ow, HS_COLS, span, HS_SPAN - 6, (double)(HS_SPAN - 6) / (HS_COLS + 6)); return nullptr; }
    }
    g.off_h = g.blob.size();
    const int ks = g.hp.ksize;
    for (int t = 0; t < ks; ++t) for (int x = 0; x < ow; ++x) g.blob.push_back(g.hp.kk[(size_t)x * ks + t]);
    g.blob.insert(g.blob.end(), g.hp.lo.begin(), g.hp.lo.end());
    g.blob.insert(g.blob.end(), g.hp.cnt.begin(), g.hp.cnt.end());
  }
  g.row0 = 0; g.nrows = h;
  if (!g.vp.skipped()) {
    g.off_v = g.blob.size();
    g.blob.insert(g.blob.end(), g.vp.kk.begin(), g.vp.kk.end());
    g.blob.insert(g.blob.end(), g.vp.lo.begin(), g.vp.lo.end());
    g.blob.insert(g.blob.end(), g.vp.cnt.begin(), g.vp.cnt.end());
    g.row0 = g.vp.lo[0];
    g.nrows = g.vp.lo[oh - 1] + g.vp.cnt[oh - 1] - g.row0;      // (lo and lo + cnt are non-decreasing)
  }
  return &g_geo.emplace(key, std::move(g)).first->second;
}

// ---------------------------------------------------------------- kernels
typedef __attribute__((ext_vector_type(3))) unsigned int u32x3;

// Pillow's alpha_composite (AlphaComposite.c) with dst = opaque white: blend = 255 (255 - a), outa255 = 255 a + blend = 65025
// for every a, so coef1 = a * 255 * 255 * 128 / 65025 = 128 a exactly and the division is gone; coef2 = 255 * 128 - coef1;
// tmp = src coef1 + 255 coef2 + (0x80 << 7); out = ((tmp + (tmp >> 8)) >> 8) >> 7.  (tmp < 2^24.)
MVD_DEVINL unsigned int over_white(unsigned int s, unsigned int a) {
  const unsigned int coef1 = a << 7, coef2 = 255u * 128u - coef1;
  const unsigned int tmp = s * coef1 + 255u * coef2 + (0x80u << 7);
  return ((tmp + (tmp >> 8)) >> 8) >> 7;
}
MVD_DEVINL int clip8(int acc) {
  const int v = acc >> PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// composite + horizontal pass.  grid (ceil(ow / HS_COLS), ceil(nrows / HS_ROWS), batch).  src_al = src rounded down to 16
// bytes, mis = src - src_al; src_rsrc_bytes = mis + the bytes of src (what the descriptor covers; a chunk that reaches past it
// reads zeros for pixels no tap uses).  kkT == null: the pass is skipped and a column copies its own (composited) pixel.
// inter [batch][3][nrows][pitch] uint8.
__global__ __launch_bounds__(256) void imgfe_h_kernel(const unsigned char* __restrict__ src, const unsigned char* __restrict__ src_al, unsigned int mis,
                                                      unsigned int src_rsrc_bytes, int h, int w, int ch, int ow, int row0, int nrows, int pitch,
                                                      const int* __restrict__ kkT, const int* __restrict__ xmin, const int* __restrict__ xcnt,
                                                      int ksize, unsigned char* __restrict__ inter) {
  __shared__ __attribute__((aligned(16))) unsigned char pl[HS_ROWS][3][HS_SPAN];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int x0 = blockIdx.x * HS_COLS, x1 = x0 + HS_COLS < ow ? x0 + HS_COLS : ow;
  const int b = blockIdx.z, row = blockIdx.y * HS_ROWS + wave;         // row: index into the intermediate's rows
  const bool live = row < nrows;
  int xs = x0, xe = x1;                                                // source pixels [xs, xe) of this workgroup
  if (kkT) { xs = xmin[x0]; xe = xmin[x1 - 1] + xcnt[x1 - 1]; }
  int xbase = xs;                                                      // the source pixel at LDS position 0
  if (live) {
    const size_t rowpix = ((size_t)b * h + row0 + row) * w;
    if (ch == 4 && !(mis & 3)) {
      // 16-byte chunks of the aligned buffer: each holds four whole pixels; chunk 0 holds pixel xs
      const unsigned int first = mis + (unsigned int)(rowpix + xs) * 4u, c0 = first & ~15u;
      const int nchunk = (int)((mis + (unsigned int)(rowpix + xe) * 4u - c0 + 15u) >> 4);
      xbase = xs - (int)((first - c0) >> 2);
      const __amdgpu_buffer_rsrc_t rs = buf_rsrc(src_al, src_rsrc_bytes);
      for (int c = lane; c < nchunk; c += 64) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(c0 + 16u * c), 0, 0);
        unsigned int p0 = 0, p1 = 0, p2 = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned int a = v[j] >> 24;
          p0 |= over_white(v[j] & 255u, a) << (8 * j);
          p1 |= over_white((v[j] >> 8) & 255u, a) << (8 * j);
          p2 |= over_white((v[j] >> 16) & 255u, a) << (8 * j);
        }
        *reinterpret_cast<unsigned int*>(&pl[wave][0][4 * c]) = p0;
        *reinterpret_cast<unsigned int*>(&pl[wave][1][4 * c]) = p1;
        *reinterpret_cast<unsigned int*>(&pl[wave][2][4 * c]) = p2;
      }
    } else {
      // RGB, or RGBA at an address that is no multiple of 4: pixel by pixel
      for (int p = lane; p < xe - xs; p += 64) {
        const unsigned char* px = src + (rowpix + xs + p) * ch;
        unsigned int r = px[0], g = px[1], bl = px[2];
        if (ch == 4) { const unsigned int a = px[3]; r = over_white(r, a); g = over_white(g, a); bl = over_white(bl, a); }
        pl[wave][0][p] = (unsigned char)r; pl[wave][1][p] = (unsigned char)g; pl[wave][2][p] = (unsigned char)bl;
      }
    }
  }
  __syncthreads();
  const int col = x0 + lane;
  if (!live || col >= x1) return;
  int v0, v1, v2;
  if (kkT) {
    const int xm = xmin[col] - xbase, n = xcnt[col];
    const int* k = kkT + col;
    int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
    for (int t = 0; t < n; ++t) {
      const int kw = k[(size_t)t * ow];
      a0 += (int)pl[wave][0][xm + t] * kw;
      a1 += (int)pl[wave][1][xm + t] * kw;
      a2 += (int)pl[wave][2][xm + t] * kw;
    }
    v0 = clip8(a0); v1 = clip8(a1); v2 = clip8(a2);
  } else {
    const int p = col - xbase;
    v0 = pl[wave][0][p]; v1 = pl[wave][1][p]; v2 = pl[wave][2][p];
  }
  const size_t plane = (size_t)nrows * pitch;
  unsigned char* o = inter + (size_t)b * 3 * plane + (size_t)row * pitch + col;
  o[0] = (unsigned char)v0; o[plane] = (unsigned char)v1; o[2 * plane] = (unsigned char)v2;
}

// vertical pass + outputs.  grid (ceil(ow / VS_COLS), ceil(oh / VS_ROWS), batch); a lane owns columns x .. x + 3 of output row y
// in all three planes.  kk == null: the pass is skipped.  vec_u8 / vec_f32: the output takes whole-lane vector stores (out_w a
// multiple of 4 and the pointer aligned); otherwise element by element.  out_u8 [batch][oh][ow][3], out_f32 [batch][3][oh][ow].
__global__ __launch_bounds__(256) void imgfe_v_kernel(const unsigned char* __restrict__ inter, int row0, int nrows, int pitch, int oh, int ow,
                                                      const int* __restrict__ kk, const int* __restrict__ ymin, const int* __restrict__ ycnt, int ksize,
                                                      unsigned char* __restrict__ out_u8, float* __restrict__ out_f32, unsigned int u8_bytes,
                                                      unsigned int f32_bytes, int vec_u8, int vec_f32) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int y = blockIdx.y * VS_ROWS + wave, x = blockIdx.x * VS_COLS + lane * 4, b = blockIdx.z;
  if (y >= oh || x >= ow) return;
  const size_t plane = (size_t)nrows * pitch;
  const unsigned char* ip = inter + (size_t)b * 3 * plane + x;         // (pitch is a multiple of 16 and x of 4: dword reads)
  unsigned int r[3][4];
  if (kk) {
    const int y0 = ymin[y] - row0, n = ycnt[y];
    const int* k = kk + (size_t)y * ksize;
    int acc[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[c][j] = 1 << (PRECISION_BITS - 1);
    for (int t = 0; t < n; ++t) {
      const int kw = k[t];
      const size_t ro = (size_t)(y0 + t) * pitch;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const unsigned int word = *reinterpret_cast<const unsigned int*>(ip + c * plane + ro);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[c][j] += (int)((word >> (8 * j)) & 255u) * kw;
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) r[c][j] = (unsigned int)clip8(acc[c][j]);
  } else {
    const size_t ro = (size_t)(y - row0) * pitch;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const unsigned int word = *reinterpret_cast<const unsigned int*>(ip + c * plane + ro);
#pragma unroll
      for (int j = 0; j < 4; ++j) r[c][j] = (word >> (8 * j)) & 255u;
    }
  }
  if (out_f32) {
    // float(byte) / 127.5f - 1.0f: an IEEE fp32 division, then an fp32 subtraction (no reciprocal, no contraction)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      f32x4 f;
#pragma unroll
      for (int j = 0; j < 4; ++j) f[j] = __fsub_rn(__fdiv_rn((float)r[c][j], 127.5f), 1.0f);
      const size_t e = (((size_t)b * 3 + c) * oh + y) * ow + x;
      if (vec_f32) store16(__builtin_bit_cast(u32x4, f), buf_rsrc(out_f32, f32_bytes), (int)(e * 4), 0);
      else
        for (int j = 0; j < 4; ++j) if (x + j < ow) out_f32[e + j] = f[j];
    }
  }
  if (out_u8) {
    const size_t e = (((size_t)b * oh + y) * ow + x) * 3;
    if (vec_u8) {
      u32x3 v;
      v[0] = r[0][0] | r[1][0] << 8 | r[2][0] << 16 | r[0][1] << 24;
      v[1] = r[1][1] | r[2][1] << 8 | r[0][2] << 16 | r[1][2] << 24;
      v[2] = r[2][2] | r[0][3] << 8 | r[1][3] << 16 | r[2][3] << 24;
      __builtin_amdgcn_raw_buffer_store_b96(v, buf_rsrc(out_u8, u8_bytes), (int)e, 0, 0);
      asm volatile("s_nop 1" :: "v"(v));        // (the wait states of bufaddr.h's store16, for the 12-byte form)
    } else {
      for (int j = 0; j < 4; ++j)
        if (x + j < ow) { out_u8[e + 3 * j] = (unsigned char)r[0][j]; out_u8[e + 3 * j + 1] = (unsigned char)r[1][j]; out_u8[e + 3 * j + 2] = (unsigned char)r[2][j]; }
    }
  }
}

}  // namespace

extern "C" {

int mvd_op_image_frontend_spans(int* out4) {
  if (!out4) { mvd_set_error("image_frontend_spans: null argument"); return -1; }
  out4[0] = HS_COLS; out4[1] = HS_ROWS; out4[2] = VS_COLS; out4[3] = VS_ROWS;
  return 0;
}

int64_t mvd_op_image_frontend_workspace_bytes(int batch, int h, int w, int channels, int out_h, int out_w) {
  if (int r = check_shape("image_frontend_workspace_bytes", batch, h, w, channels, out_h, out_w)) return r;
  const Geometry* g = geometry(h, w, out_h, out_w);
  if (!g) return -1;
  return (int64_t)(table_bytes(h, w, out_h, out_w) + align256((size_t)batch * 3 * g->nrows * pitch_of(out_w)));
}

int mvd_op_image_frontend(const uint8_t* src, int batch, int h, int w, int channels, int out_h, int out_w, uint8_t* out_u8, float* out_f32,
                          void* workspace, int64_t workspace_bytes, void* stream) {
  if (int r = check_shape("image_frontend", batch, h, w, channels, out_h, out_w)) return r;
  if (!src) { mvd_set_error("image_frontend: null source"); return -1; }
  if (!out_u8 && !out_f32) { mvd_set_error("image_frontend: nothing to write (no out_u8, no out_f32)"); return -1; }
  if ((uintptr_t)out_f32 & 3) { mvd_set_error("image_frontend: out_f32 must be 4-byte aligned"); return -1; }
  if (!workspace || ((uintptr_t)workspace & 255)) { mvd_set_error("image_frontend: the workspace must be a 256-byte aligned buffer"); return -1; }
  const Geometry* g = geometry(h, w, out_h, out_w);
  if (!g) return -1;
  const size_t head = table_bytes(h, w, out_h, out_w);
  const int pitch = pitch_of(out_w);
  const size_t need = head + align256((size_t)batch * 3 * g->nrows * pitch);
  if (g->blob.size() * 4 > head) { mvd_set_error("image_frontend: internal: table region too small"); return -1; }
  if ((size_t)workspace_bytes < need) { mvd_set_error("image_frontend: workspace too small: need %zu bytes, given %lld", need, (long long)workspace_bytes); return -4; }
  hipStream_t s = (hipStream_t)stream;
  char* base = reinterpret_cast<char*>(workspace);
  if (!g->blob.empty()) {
    // the uploads read a page-locked copy of the tables (made once per geometry), so they never wait for the stream.  Page-locked
    // memory is bounded: the first MAX_PINNED geometries get a copy, later ones upload from the (equally long-lived) pageable blob.
    const int* from = nullptr;
    {
      std::lock_guard<std::mutex> lock(g_mu);
      Geometry* gm = const_cast<Geometry*>(g);
      if (!gm->pinned && g_pinned < MAX_PINNED) {
        void* p = nullptr;
        if (hipHostMalloc(&p, g->blob.size() * 4, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); mvd_set_error("image_frontend: hipHostMalloc of %zu bytes failed", g->blob.size() * 4); return -3; }
        memcpy(p, g->blob.data(), g->blob.size() * 4);
        gm->pinned = reinterpret_cast<int*>(p);
        ++g_pinned;
      }
      from = gm->pinned ? gm->pinned : g->blob.data();
    }
    if (hipMemcpyAsync(base, from, g->blob.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess) { mvd_set_error("image_frontend: hipMemcpyAsync failed"); return -3; }
  }
  const int* tab = reinterpret_cast<const int*>(base);
  unsigned char* inter = reinterpret_cast<unsigned char*>(base + head);
  const int *kh = nullptr, *xh = nullptr, *ch_ = nullptr, *kv = nullptr, *yv = nullptr, *cv = nullptr;
  if (!g->hp.skipped()) { kh = tab + g->off_h; xh = kh + (size_t)out_w * g->hp.ksize; ch_ = xh + out_w; }
  if (!g->vp.skipped()) { kv = tab + g->off_v; yv = kv + (size_t)out_h * g->vp.ksize; cv = yv + out_h; }
  const unsigned int mis = (unsigned int)((uintptr_t)src & 15);
  const unsigned int src_bytes = mis + (unsigned int)((size_t)batch * h * w * channels);
  hipLaunchKernelGGL(imgfe_h_kernel, dim3((out_w + HS_COLS - 1) / HS_COLS, (g->nrows + HS_ROWS - 1) / HS_ROWS, batch), dim3(256), 0, s, src, src - mis, mis,
                     src_bytes, h, w, channels, out_w, g->row0, g->nrows, pitch, kh, xh, ch_, g->hp.ksize, inter);
  CHECK(launch_check("image front end (composite + horizontal)"));
  const unsigned int u8_bytes = (unsigned int)((size_t)batch * out_h * out_w * 3), f32_bytes = (unsigned int)((size_t)batch * 3 * out_h * out_w * 4);
  const int vec_u8 = out_w % 4 == 0 && !((uintptr_t)out_u8 & 3), vec_f32 = out_w % 4 == 0 && !((uintptr_t)out_f32 & 15);
  hipLaunchKernelGGL(imgfe_v_kernel, dim3((out_w + VS_COLS - 1) / VS_COLS, (out_h + VS_ROWS - 1) / VS_ROWS, batch), dim3(256), 0, s, inter, g->row0, g->nrows,
                     pitch, out_h, out_w, kv, yv, cv, g->vp.ksize, out_u8, out_f32, u8_bytes, f32_bytes, vec_u8, vec_f32);
  return launch_check("image front end (vertical)");
}

}  // extern "C"
