// Graph operators of the training-mode MPN (mpn/train.py): the per-(target node, source type) segmented
// aggregations with their backwards, and the backward of the x[dst] / x[src] row gathers.
//
// Every kernel is the "store once, sum per destination through an inverted index" form: the contribution rows
// already lie in memory once (messages, per-edge gradients), the plan (perm_dst / seg_off, perm_src / src_off) is
// the inverted index, and one wave owns one destination (a segment or a node). No atomics; every output element
// is written exactly once per call; a destination's rows are read in list order, so results are bitwise
// reproducible.
//
// Mapping: 256-thread blocks, one wave per destination. A 64-float row is 16 lanes x float4, so one wave
// instruction moves four rows (two 128-float rows): row group g = lane / 16 takes the list's rows g, g + 4, ...
// in order, and the four group partials are added as (g0 + g1) + (g2 + g3) in every lane. The workload's lists
// are short and even (tens of edges per segment, images of <= 512 nodes), so no list is split across waves.
#include <limits.h>

#include "pemp_common.h"

namespace pemp {
namespace {

constexpr int kWaves = 4;   // destinations per 256-thread block

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// g . m over the 16 lanes of a row group, in each of its lanes. In double: the products of two floats are exact
// and the 64-term sum is good to 1e-16, so the score gradients below are correctly rounded values of their formula
// (the per-row cost is a few fp64 FMAs next to a 256-byte row read)
__device__ __forceinline__ double dot16(float4 a, float4 b) {
  double v = fma((double)a.w, (double)b.w,
                 fma((double)a.z, (double)b.z, fma((double)a.y, (double)b.y, (double)a.x * (double)b.x)));
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// [b, b + cnt) of a destination's list, clamped into [0, E] (a plan is trusted, but never followed out of bounds)
__device__ __forceinline__ int list_range(const int32_t* off, int64_t d, int64_t E, int64_t* b) {
  int64_t lo = off[d], hi = off[d + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > E ? E : hi;
  *b = lo;
  return hi > lo ? (int)(hi - lo) : 0;
}

template <int KIND>
__global__ __launch_bounds__(64 * kWaves) void seg_aggr_fwd_kernel(int64_t nseg, int64_t E, const float* __restrict__ msgs,
                                                                  const float* __restrict__ scores,
                                                                  const int32_t* __restrict__ perm,
                                                                  const int32_t* __restrict__ off, float* __restrict__ out,
                                                                  float* __restrict__ alpha, int32_t* __restrict__ arg) {
  const int lane = threadIdx.x & 63, grp = lane >> 4, c = (lane & 15) * 4;
  const int64_t seg = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (seg >= nseg) return;                        // wave-uniform
  int64_t b;
  const int cnt = list_range(off, seg, E, &b);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (KIND == PEMP_AGGR_MAX) {
    int4 pos = make_int4(-1, -1, -1, -1);         // position in the segment of the running maximum (-1: none yet)
    for (int r = grp; r < cnt; r += 4) {
      const uint32_t e = (uint32_t)perm[b + r];
      if (e >= (uint64_t)E) continue;
      const float4 m = ld4(msgs + (size_t)e * 64 + c);
      if (pos.x < 0 || m.x > acc.x) acc.x = m.x, pos.x = r;
      if (pos.y < 0 || m.y > acc.y) acc.y = m.y, pos.y = r;
      if (pos.z < 0 || m.z > acc.z) acc.z = m.z, pos.z = r;
      if (pos.w < 0 || m.w > acc.w) acc.w = m.w, pos.w = r;
    }
    // the other groups' candidates: the larger value wins, the earlier position on a tie (-1 is the largest unsigned)
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
#define PEMP_TAKE(f)                                                                        \
  {                                                                                         \
    const float ov = __shfl_xor(acc.f, o);                                                  \
    const int op = __shfl_xor(pos.f, o);                                                    \
    if (op >= 0 && (pos.f < 0 || ov > acc.f || (ov == acc.f && op < pos.f))) acc.f = ov, pos.f = op; \
  }
      PEMP_TAKE(x) PEMP_TAKE(y) PEMP_TAKE(z) PEMP_TAKE(w)
#undef PEMP_TAKE
    }
    if (grp == 0) {
      int4 a;
      a.x = pos.x < 0 ? -1 : perm[b + pos.x];
      a.y = pos.y < 0 ? -1 : perm[b + pos.y];
      a.z = pos.z < 0 ? -1 : perm[b + pos.z];
      a.w = pos.w < 0 ? -1 : perm[b + pos.w];
      if (pos.x < 0) acc.x = 0.f;
      if (pos.y < 0) acc.y = 0.f;
      if (pos.z < 0) acc.z = 0.f;
      if (pos.w < 0) acc.w = 0.f;
      st4(out + (size_t)seg * 64 + c, acc);
      if (arg) *reinterpret_cast<int4*>(arg + (size_t)seg * 64 + c) = a;
    }
    return;
  }
  float mx = 0.f, den = 1.f;
  if (KIND == PEMP_AGGR_ATTN) {                   // scatter_softmax: exp(s - max_seg) / (sum_seg + 1e-12)
    mx = -INFINITY;
    for (int k = lane; k < cnt; k += 64) {
      const uint32_t e = (uint32_t)perm[b + k];
      if (e < (uint64_t)E) mx = fmaxf(mx, scores[e]);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float sm = 0.f;                               // lane k sums the edges k, k + 64, ... in order; then a fixed tree
    for (int k = lane; k < cnt; k += 64) {
      const uint32_t e = (uint32_t)perm[b + k];
      if (e < (uint64_t)E) sm += expf(scores[e] - mx);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sm += __shfl_xor(sm, o);
    den = sm + 1e-12f;
  }
#pragma unroll 2
  for (int r = grp; r < cnt; r += 4) {
    const uint32_t e = (uint32_t)perm[b + r];
    if (e >= (uint64_t)E) continue;
    const float4 m = ld4(msgs + (size_t)e * 64 + c);
    if (KIND == PEMP_AGGR_ATTN) {
      const float a = expf(scores[e] - mx) / den;  // the same value in the group's 16 lanes; one of them stores it
      if (alpha && (lane & 15) == 0) alpha[e] = a;
      acc.x = fmaf(a, m.x, acc.x), acc.y = fmaf(a, m.y, acc.y), acc.z = fmaf(a, m.z, acc.z), acc.w = fmaf(a, m.w, acc.w);
    } else {
      acc.x += m.x, acc.y += m.y, acc.z += m.z, acc.w += m.w;
    }
  }
  acc.x = xsum_rows(acc.x), acc.y = xsum_rows(acc.y), acc.z = xsum_rows(acc.z), acc.w = xsum_rows(acc.w);
  if (KIND == PEMP_AGGR_MEAN) {
    const float n = (float)(cnt > 1 ? cnt : 1);
    acc.x /= n, acc.y /= n, acc.z /= n, acc.w /= n;
  }
  if (grp == 0) st4(out + (size_t)seg * 64 + c, acc);
}

template <int KIND>
__global__ __launch_bounds__(64 * kWaves) void seg_aggr_bwd_kernel(int64_t nseg, int64_t E, const float* __restrict__ gout,
                                                                  const float* __restrict__ msgs,
                                                                  const float* __restrict__ alpha,
                                                                  const int32_t* __restrict__ arg,
                                                                  const int32_t* __restrict__ perm,
                                                                  const int32_t* __restrict__ off, float* __restrict__ gmsgs,
                                                                  float* __restrict__ gscores) {
  const int lane = threadIdx.x & 63, grp = lane >> 4, c = (lane & 15) * 4;
  const int64_t seg = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (seg >= nseg) return;
  int64_t b;
  const int cnt = list_range(off, seg, E, &b);
  if (cnt == 0) return;
  float4 g = ld4(gout + (size_t)seg * 64 + c);
  double go = 0.0;
  int4 win = make_int4(-1, -1, -1, -1);
  if (KIND == PEMP_AGGR_ATTN) {
    // g . out[seg] = sum_k alpha_k (g . msgs[k]), evaluated from the very products the rows' own terms use below
    // and divided by sum_k alpha_k (1 up to the softmax's 1e-12 term and the alphas' rounding): a segment's score
    // gradients then sum to zero up to their own roundings, as they do analytically (a shift of all its scores
    // leaves a segment's softmax unchanged), instead of to go (sum alpha - 1). That residue is all there is to the
    // gradient of a score bias. The scalars are kept in double.
    double part = 0.0, wsum = 0.0;
    for (int r = grp; r < cnt; r += 4) {
      const uint32_t e = (uint32_t)perm[b + r];
      if (e >= (uint64_t)E) continue;
      const double a = alpha[e];
      part = fma(a, dot16(g, ld4(msgs + (size_t)e * 64 + c)), part);
      wsum += a;
    }
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) part += __shfl_xor(part, o), wsum += __shfl_xor(wsum, o);
    go = wsum > 0.0 ? part / wsum : 0.0;
  }
  if (KIND == PEMP_AGGR_MAX) win = *reinterpret_cast<const int4*>(arg + (size_t)seg * 64 + c);
  if (KIND == PEMP_AGGR_MEAN) {
    const float n = (float)cnt;
    g.x /= n, g.y /= n, g.z /= n, g.w /= n;
  }
  for (int r = grp; r < cnt; r += 4) {            // (dot16 stays inside the row group, whose lanes run together)
    const uint32_t e = (uint32_t)perm[b + r];
    if (e >= (uint64_t)E) continue;
    float4 v = g;
    if (KIND == PEMP_AGGR_ATTN) {
      const float a = alpha[e];
      const double d = dot16(g, ld4(msgs + (size_t)e * 64 + c));
      v = make_float4(a * g.x, a * g.y, a * g.z, a * g.w);
      if (gscores && (lane & 15) == 0) gscores[e] = (float)((double)a * (d - go));
    } else if (KIND == PEMP_AGGR_MAX) {           // one winner per feature (torch_scatter's arg rule)
      v = make_float4(win.x == (int)e ? g.x : 0.f, win.y == (int)e ? g.y : 0.f, win.z == (int)e ? g.z : 0.f,
                      win.w == (int)e ? g.w : 0.f);
    }
    st4(gmsgs + (size_t)e * 64 + c, v);
  }
}

// out[n] = sum of ga rows of list a, then of gb rows of list b (W / 4 lanes per row, 256 / W row groups)
template <int W>
__global__ __launch_bounds__(64 * kWaves) void seg_rows_sum_kernel(int64_t N, int64_t E, const float* __restrict__ ga,
                                                                  const int32_t* __restrict__ perm_a,
                                                                  const int32_t* __restrict__ off_a,
                                                                  const float* __restrict__ gb,
                                                                  const int32_t* __restrict__ perm_b,
                                                                  const int32_t* __restrict__ off_b, float* __restrict__ out) {
  constexpr int LPR = W / 4, R = 64 / LPR;
  const int lane = threadIdx.x & 63, grp = lane / LPR, c = (lane % LPR) * 4;
  const int64_t n = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (n >= N) return;
  int64_t ba, bb = 0;
  const int na = list_range(off_a, n, E, &ba);
  const int nb = gb ? list_range(off_b, n, E, &bb) : 0;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 2
  for (int r = grp; r < na + nb; r += R) {
    const bool first = r < na;
    const uint32_t e = (uint32_t)(first ? perm_a[ba + r] : perm_b[bb + (r - na)]);
    if (e >= (uint64_t)E) continue;
    const float4 m = ld4((first ? ga : gb) + (size_t)e * W + c);
    acc.x += m.x, acc.y += m.y, acc.z += m.z, acc.w += m.w;
  }
  if (W == 64) {
    acc.x = xsum_rows(acc.x), acc.y = xsum_rows(acc.y), acc.z = xsum_rows(acc.z), acc.w = xsum_rows(acc.w);
  } else {
    acc.x = xsum32(acc.x), acc.y = xsum32(acc.y), acc.z = xsum32(acc.z), acc.w = xsum32(acc.w);
  }
  if (grp == 0) st4(out + (size_t)n * W + c, acc);
}

inline unsigned blocks_for(int64_t dests) { return (unsigned)((dests + kWaves - 1) / kWaves); }

int check_sizes(const char* fn, int kind, int T, int64_t N, int64_t E) {
  PEMP_CHECK_ARG(kind >= PEMP_AGGR_ATTN && kind <= PEMP_AGGR_MAX, "%s: unknown kind %d", fn, kind);
  PEMP_CHECK_ARG(T >= 1, "%s: T = %d < 1", fn, T);
  PEMP_CHECK_ARG(N >= 0 && E >= 0, "%s: negative size (N = %lld, E = %lld)", fn, (long long)N, (long long)E);
  PEMP_CHECK_ARG(E <= INT_MAX && N < INT_MAX / T, "%s: int32 indices (E = %lld, N = %lld, T = %d)", fn, (long long)E,
                 (long long)N, T);
  return PEMP_OK;
}

}  // namespace
}  // namespace pemp

using namespace pemp;

extern "C" int pemp_seg_aggr_fwd(int kind, int T, int64_t N, int64_t E, const float* msgs, const float* scores,
                                 const int32_t* perm_dst, const int32_t* seg_off, float* out, float* alpha,
                                 int32_t* arg, void* stream) {
  if (int rc = check_sizes("pemp_seg_aggr_fwd", kind, T, N, E)) return rc;
  PEMP_CHECK_ARG(kind != PEMP_AGGR_ATTN || scores || N == 0 || E == 0, "pemp_seg_aggr_fwd: ATTN needs scores");
  if (N == 0) return PEMP_OK;
  PEMP_CHECK_ARG(out && seg_off, "pemp_seg_aggr_fwd: NULL out / seg_off");
  PEMP_CHECK_ARG(E == 0 || (msgs && perm_dst), "pemp_seg_aggr_fwd: NULL msgs / perm_dst");
  hipStream_t st = as_stream(stream);
  const int64_t nseg = N * T;
  if (E == 0) {                                   // every segment is empty: zeros (and no winner)
    PEMP_HIP(hipMemsetAsync(out, 0, (size_t)nseg * 64 * sizeof(float), st));
    if (kind == PEMP_AGGR_MAX && arg) PEMP_HIP(hipMemsetAsync(arg, 0xFF, (size_t)nseg * 64 * sizeof(int32_t), st));
    return PEMP_OK;
  }
  ProfScope prof("seg_aggr_fwd", st);
  const dim3 grid(blocks_for(nseg)), block(64 * kWaves);
  switch (kind) {
    case PEMP_AGGR_ATTN:
      seg_aggr_fwd_kernel<PEMP_AGGR_ATTN><<<grid, block, 0, st>>>(nseg, E, msgs, scores, perm_dst, seg_off, out, alpha, arg);
      break;
    case PEMP_AGGR_SUM:
      seg_aggr_fwd_kernel<PEMP_AGGR_SUM><<<grid, block, 0, st>>>(nseg, E, msgs, scores, perm_dst, seg_off, out, alpha, arg);
      break;
    case PEMP_AGGR_MEAN:
      seg_aggr_fwd_kernel<PEMP_AGGR_MEAN><<<grid, block, 0, st>>>(nseg, E, msgs, scores, perm_dst, seg_off, out, alpha, arg);
      break;
    default:
      seg_aggr_fwd_kernel<PEMP_AGGR_MAX><<<grid, block, 0, st>>>(nseg, E, msgs, scores, perm_dst, seg_off, out, alpha, arg);
      break;
  }
  PEMP_LAUNCH_CHECK();
  return PEMP_OK;
}

extern "C" int pemp_seg_aggr_bwd(int kind, int T, int64_t N, int64_t E, const float* grad_out, const float* msgs,
                                 const float* alpha, const float* out, const int32_t* arg, const int32_t* perm_dst,
                                 const int32_t* seg_off, float* grad_msgs, float* grad_scores, void* stream) {
  if (int rc = check_sizes("pemp_seg_aggr_bwd", kind, T, N, E)) return rc;
  if (N == 0 || E == 0) return PEMP_OK;           // no edge: grad_msgs / grad_scores have no row
  PEMP_CHECK_ARG(grad_out && perm_dst && seg_off && grad_msgs, "pemp_seg_aggr_bwd: NULL grad_out / plan / grad_msgs");
  PEMP_CHECK_ARG(kind != PEMP_AGGR_ATTN || (msgs && alpha), "pemp_seg_aggr_bwd: ATTN needs msgs and alpha");
  PEMP_CHECK_ARG(kind != PEMP_AGGR_MAX || arg, "pemp_seg_aggr_bwd: MAX needs arg");
  hipStream_t st = as_stream(stream);
  ProfScope prof("seg_aggr_bwd", st);
  const int64_t nseg = N * T;
  const dim3 grid(blocks_for(nseg)), block(64 * kWaves);
  switch (kind) {
    case PEMP_AGGR_ATTN:
      seg_aggr_bwd_kernel<PEMP_AGGR_ATTN><<<grid, block, 0, st>>>(nseg, E, grad_out, msgs, alpha, arg, perm_dst, seg_off, grad_msgs, grad_scores);
      break;
    case PEMP_AGGR_SUM:
      seg_aggr_bwd_kernel<PEMP_AGGR_SUM><<<grid, block, 0, st>>>(nseg, E, grad_out, msgs, alpha, arg, perm_dst, seg_off, grad_msgs, grad_scores);
      break;
    case PEMP_AGGR_MEAN:
      seg_aggr_bwd_kernel<PEMP_AGGR_MEAN><<<grid, block, 0, st>>>(nseg, E, grad_out, msgs, alpha, arg, perm_dst, seg_off, grad_msgs, grad_scores);
      break;
    default:
      seg_aggr_bwd_kernel<PEMP_AGGR_MAX><<<grid, block, 0, st>>>(nseg, E, grad_out, msgs, alpha, arg, perm_dst, seg_off, grad_msgs, grad_scores);
      break;
  }
  PEMP_LAUNCH_CHECK();
  return PEMP_OK;
}

extern "C" int pemp_seg_rows_sum(int64_t N, int64_t E, int W, const float* ga, const int32_t* perm_a,
                                 const int32_t* off_a, const float* gb, const int32_t* perm_b, const int32_t* off_b,
                                 float* out, void* stream) {
  PEMP_CHECK_ARG(W == 64 || W == 128, "pemp_seg_rows_sum: W = %d (64 or 128)", W);
  PEMP_CHECK_ARG(N >= 0 && E >= 0, "pemp_seg_rows_sum: negative size (N = %lld, E = %lld)", (long long)N, (long long)E);
  PEMP_CHECK_ARG(E <= INT_MAX && N < INT_MAX, "pemp_seg_rows_sum: int32 indices (N = %lld, E = %lld)", (long long)N,
                 (long long)E);
  if (N == 0) return PEMP_OK;
  PEMP_CHECK_ARG(out, "pemp_seg_rows_sum: NULL out");
  hipStream_t st = as_stream(stream);
  if (E == 0) {
    PEMP_HIP(hipMemsetAsync(out, 0, (size_t)N * W * sizeof(float), st));
    return PEMP_OK;
  }
  PEMP_CHECK_ARG(ga && perm_a && off_a, "pemp_seg_rows_sum: NULL list a");
  PEMP_CHECK_ARG(!gb || (perm_b && off_b), "pemp_seg_rows_sum: gb without perm_b / off_b");
  ProfScope prof("seg_rows_sum", st);
  const dim3 grid(blocks_for(N)), block(64 * kWaves);
  if (W == 64)
    seg_rows_sum_kernel<64><<<grid, block, 0, st>>>(N, E, ga, perm_a, off_a, gb, perm_b, off_b, out);
  else
    seg_rows_sum_kernel<128><<<grid, block, 0, st>>>(N, E, ga, perm_a, off_a, gb, perm_b, off_b, out);
  PEMP_LAUNCH_CHECK();
  return PEMP_OK;
}
