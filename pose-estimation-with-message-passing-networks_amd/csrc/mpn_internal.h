// What the translation units of the inference MPN share (mpn.hip has the overview): the constants, the workspace, the
// argument records of the edge-order prepares and the host launch functions through which mpn.hip's forward driver
// reaches the kernels of mpn_order.hip. No kernels here.
#pragma once
#include <algorithm>

#include "pemp_common.h"

namespace pemp {
namespace {

constexpr int D = 64;
constexpr int LDW = 72;     // LDS row stride of a 64x64 weight tile (conflict-free ds_read_b128)
constexpr int MAXT = 17;
constexpr int EDGE_WAVES = 16;   // waves per edge-pass workgroup (one workgroup per CU)
// edge embedding: EMB_WAVES waves per workgroup, EMB_PER_CU workgroups per CU (each with its own LDS image; the
// register target follows: EMB_WAVES x EMB_PER_CU / 4 waves per SIMD)
// (10 x 2 and 8 x 2 measured against 16 x 1 in round 6, profiles/r06_embed_two_wg.md: not faster)
constexpr int EMB_WAVES = 16, EMB_PER_CU = 1;
constexpr int EMB_MIN_WAVES_EU = EMB_WAVES * EMB_PER_CU / 4 > 1 ? EMB_WAVES * EMB_PER_CU / 4 : 1;
// CUs that the one-workgroup-per-CU launches of a forward over E edges (edge passes, edge embedding, and the prepares'
// per-workgroup split) spread over. From RESERVE_MIN_EDGES edges on, PEMP_RESERVE_CUS of them (rounded down to
// a multiple of 8, so the XCD-aware placement still sees whole XCD rows) are left free: with two batches in flight
// the other batch's small latency-bound kernels run there instead of waiting for the full-chip launches (c3 +4 %,
// c3knn10 / c5ms +11 % images/s, one batch at a time -1.5 %). Smaller graphs (batch 1) keep
// every CU. The edge embedding leaves the reserved CUs free too (spread over every CU: serial steps +1 % / +3.4 %,
// two batches in flight slower).
constexpr int RESERVE_CUS_DEFAULT = 64;        // (the PEMP_RESERVE_CUS environment variable overrides it)
constexpr int64_t RESERVE_MIN_EDGES = 65536;   // (batch 1 stays below it: one batch at a time lost 1.5 % to a reservation)
// The reservation is capped at a quarter of the device (rounded down to a multiple of 8): 64 of the MI355X's 256
// CUs, less on a smaller device or a compute partition, where a fixed 64 would take most of the chip.
static inline int edge_cus_policy(int cus, int64_t E, int request) {
  if (E < RESERVE_MIN_EDGES || cus <= 8) return cus;
  const int r = std::min(std::max(request, 0), cus / 4) & ~7;
  return cus - r;
}
static inline int edge_cus(int64_t E) {
  static const int request = [] {
    const char* e = getenv("PEMP_RESERVE_CUS");
    return e ? atoi(e) : RESERVE_CUS_DEFAULT;
  }();
  return edge_cus_policy(num_cus(), E, request);
}

constexpr int IMG_FLOATS = 112 * 1024;  // >= LDS image of a node embedding (<= 4 layers, <= 128 wide) + both heads (<= 64 wide)
constexpr int EIMG_MAX_STRIDE = 4 * D * LDW + (2 * D + 4) + (D + 32) * LDW + D + 32 + 32 + 4;   // edge image floats per type (max)

// limits of the closed-form fully prepare (mpn_order.h), checked by the driver
constexpr int FULLY_MAXB = 64;      // images per batch
constexpr int FULLY_MAXN = 2048;    // nodes per image (LDS lists)
constexpr int FULLY_PARTS = 4;   // threads per (type, target) segment in fully_prepare_kernel

// symmetric prepare (mpn_order.hip); the driver sends graphs whose node ids need more bits to the sorting prepare
constexpr int SYM_TBITS = 24;        // packed row entry: dst (< 2^24) | type << 24 (type 31: invalid, never matched)

// knn prepare (knn_prepare_kernel, mpn_order.hip)
constexpr int KP_MAXB = 64, KP_MAXN = 4096, KP_W = 8;   // images, nodes per batch, bit words per row (512 nodes)
constexpr int KP_LIST = 12288;                          // sources one block lists in LDS (else placed row by row)
constexpr int KP_CH = 256;                              // rows placed per block (a divisor of 1024)

}  // namespace

// (the records below cross translation units, so they sit outside the unnamed namespace)
// ---------------------------------------------------------------------------------------------
// Workspace
// ---------------------------------------------------------------------------------------------
struct MpnWs {
  int *cnt, *seg, *wg_start, *perm, *s_src, *s_dst, *s_orig, *err, *sym;
  float *X, *NT, *agg, *Q0, *EA, *EB, *img, *eimg;
  int4* ranges;
};

struct FullyPrepArgs {
  const int64_t* node_off;          // [B + 1] device
  int B;
  const int64_t* types;
  int64_t ts, N;
  int T, Gsplit;
  int *seg, *wg_start, *s_src, *s_dst, *s_orig, *err;
  const int64_t* ne;   // capacity mode: device-side (N, E, overflow); an overflowed batch prepares as empty images
};

struct KnnPrepArgs {
  const unsigned long long* R;   // [N][KP_W]
  const int* rowstart;           // [N] row start inside its image
  const int64_t* node_off;       // [B + 1]
  const int64_t* ecount;         // [B] edges per image
  int B;
  const int64_t* types;
  int64_t ts, N, E;
  int T, G;
  int *seg, *wg_start, *s_src, *s_dst, *s_orig, *err;
  int list_cap;                  // <= KP_LIST (PEMP_KNN_LIST_CAP: the row-by-row placement in tests)
};

namespace {

// order_offs (pemp_mpn_order_layout): the byte offsets of seg, wg_start, s_src, s_dst and s_orig
inline MpnWs mpn_carve(void* base, int T, int64_t N, int64_t E, size_t* bytes, size_t* order_offs = nullptr) {
  Carver c(base);
  MpnWs w;
  size_t oo[5];
  const int64_t K = (int64_t)T * N;
  w.err = c.take<int>(64);               // err[0..3] then cnt: zeroed together
  w.cnt = w.err + 64;
  c.take<int>(K + 1);
  w.seg = c.take<int>(K + 1);
  oo[0] = c.last;
  w.wg_start = c.take<int>(MAXT + 2);
  oo[1] = c.last;
  w.perm = c.take<int>(E);
  w.s_src = c.take<int>(E);
  oo[2] = c.last;
  w.s_dst = c.take<int>(E);
  oo[3] = c.last;
  w.s_orig = c.take<int>(E);
  oo[4] = c.last;
  if (order_offs) std::copy(oo, oo + 5, order_offs);
  w.X = c.take<float>(N * 128);
  w.NT = c.take<float>(N * (128 + 64 * (int64_t)T));
  w.agg = c.take<float>(N * T * D);
  w.Q0 = c.take<float>(E * D);
  w.EA = c.take<float>(E * D);
  w.EB = c.take<float>(E * D);
  w.img = c.take<float>(IMG_FLOATS);
  const int G = std::max(num_cus(), T);        // edge-pass grid (at most)
  w.ranges = c.take<int4>((size_t)G * (EDGE_WAVES + 12));
  w.eimg = c.take<float>((size_t)T * EIMG_MAX_STRIDE);   // edge-pass weight image when the caller has none
  w.sym = c.take<int>(3 * N);                           // symmetric prepare: row bounds + check flags per node
  if (bytes) *bytes = c.used;
  return w;
}

}  // namespace

// Host launch functions of mpn_order.hip: each enqueues on `st` and returns a PEMP_* code. Internal to the library:
// hidden, so the exported symbols stay those of include/pemp.h
#pragma GCC visibility push(hidden)
int launch_prepare(const pemp_mpn_desc* desc, const int64_t* edge_index, const int64_t* node_types, int64_t N,
                   int64_t E, const MpnWs& ws, hipStream_t st);
int launch_prepare_sym(const pemp_mpn_desc* desc, const int64_t* edge_index, const int64_t* node_types, int64_t N,
                       int64_t E, const MpnWs& ws, hipStream_t st);
int launch_prepare_fully(const FullyPrepArgs& a, int gx, hipStream_t st);   // gx blocks per image, a.B images
int launch_prepare_knn(const KnnPrepArgs& a, hipStream_t st);
#pragma GCC visibility pop

}  // namespace pemp
