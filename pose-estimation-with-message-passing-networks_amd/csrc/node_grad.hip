// The gradient of the node features x with respect to the maps they were read from (node_gather.py): the backward
// of x[n] = features[b_n, :, y_n, x_n] and of x[n] = feature_gather(raw)[b_n, :, y_n, x_n] evaluated under the nodes
// only (graph.hip gather_projected_conv_kernel with one map of the conv output's size). No float atomics; every
// sum below has an order fixed by the arguments alone, never by the grid or the device.
//
// Per-pixel sums (pemp_node_grad_pixels; the second stage of draw): the caller keys every row of a [M][C] buffer by
// the pixel it lands on and sorts the keys once (a stable sort, so equal keys stay in ascending row order). One wave
// per sorted position; the wave at a segment head (its key differs from its predecessor's) adds the segment front to
// back in fp32, lane on the channel, and is the only writer of that pixel. Rows with a key outside [0, npix) are
// skipped; pixels nobody touches are zeroed by a hipMemsetAsync in front.
//
// draw, first stage: D = g W2, [N][k k][Cin] from g [N][Cout] and W2 = weight as [Cout][k][k][Cin], one fp32 fma
// chain over co = 0 .. Cout - 1 per element (v_mfma_f32_16x16x4_f32 when Cin and Cout are multiples of 16, else the
// same chain with fmaf).
//
// dW, db: the nodes are the reduction dimension, in node order, cut into chunks of 256: per chunk one fma chain per
// element (MFMA with the nodes as K, or fmaf) over P[n][ci][dy][dx], the zero-padded input window under node n read
// straight from raw, stored as one partial [dW | db] into the caller's workspace; a second kernel adds the partials
// in a fixed pairwise tree, 32 per pass (the scheme of train_edge.hip, its own copy).
#include <limits.h>

#include <algorithm>

#include "pemp_common.h"

namespace pemp {
namespace {

constexpr int kChunk = 256;      // nodes per weight-gradient partial: the longest fp32 chain over nodes
constexpr int kLeaves = 32;      // partials added per tree pass
constexpr int kMaxCout = 512, kMaxK = 7;   // the forward's limits (graph.hip PCONV_THREADS * PCONV_MAXQ, ksize)

__global__ __launch_bounds__(256) void node_grad_pixels_kernel(const float* __restrict__ D, int64_t M, int C,
                                                               const int64_t* __restrict__ skey,
                                                               const int64_t* __restrict__ perm, int64_t npix,
                                                               int64_t hw, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);      // wave-uniform from here on
  if (j >= M) return;
  const int64_t key = skey[j];
  if ((uint64_t)key >= (uint64_t)npix) return;                         // out of bounds: the sentinel
  if (j > 0 && skey[j - 1] == key) return;                             // not a segment head
  int64_t end = j + 1;
  while (end < M && skey[end] == key) ++end;
  const int64_t b = key / hw, pix = key - b * hw;
  float* o = out + (size_t)b * C * hw + pix;
  for (int c = lane; c < C; c += 64) {
    float acc = 0.f;                                                   // 0 + g0 + g1 + ..., as an accumulating scatter
    for (int64_t t = j; t < end; ++t) {
      const int64_t row = perm[t];
      if ((uint64_t)row < (uint64_t)M) acc += D[(size_t)row * C + c];
    }
    o[(size_t)c * hw] = acc;
  }
}

// D[n][col] = sum_co g[n][co] W2[co][col], KC = k k Cin columns. A wave owns 16 nodes x 64 columns (four independent
// accumulators); lane (i, q) feeds A[node i][co q] and B[co q][column i] and holds rows 4 q + r, column i of D.
__global__ __launch_bounds__(256) void node_conv_dgemm_mfma_kernel(const float* __restrict__ g,
                                                                   const float* __restrict__ W2, int64_t N, int Cout,
                                                                   int KC, float* __restrict__ D) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
  const int64_t n0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
  if (n0 >= N) return;
  const int c0 = blockIdx.y * 64;
  const bool okn = n0 + i < N;
  const size_t nc = okn ? (size_t)(n0 + i) : 0;
  f32x4 acc[4];
  bool okt[4];
  int col[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    okt[t] = c0 + 16 * t < KC;                                          // (KC is a multiple of 16: whole tiles)
    col[t] = okt[t] ? c0 + 16 * t + i : 0;
  }
  for (int k0 = 0; k0 < Cout; k0 += 4) {
    const float av = g[nc * Cout + k0 + q];
    const float a = okn ? av : 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float bv = W2[(size_t)(k0 + q) * KC + col[t]];
      acc[t] = mfma4(a, okt[t] ? bv : 0.f, acc[t]);
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (!okt[t]) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t n = n0 + 4 * q + r;
      if (n < N) D[(size_t)n * KC + col[t]] = acc[t][r];
    }
  }
}

__global__ __launch_bounds__(256) void node_conv_dgemm_fma_kernel(const float* __restrict__ g,
                                                                  const float* __restrict__ W2, int64_t N, int Cout,
                                                                  int KC, float* __restrict__ D) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= N * KC) return;
  const int64_t n = idx / KC;
  const int col = (int)(idx - n * KC);
  float acc = 0.f;
  for (int co = 0; co < Cout; ++co) acc = fmaf(g[(size_t)n * Cout + co], W2[(size_t)co * KC + col], acc);
  D[idx] = acc;
}

// where element (ci, oy + pad, ox + pad) of the window of a node at pixel (px, py) of image b lies in raw, or -1
__device__ __forceinline__ int64_t window_el(int ci, int oy, int ox, int Cin, int h, int w, int B, int64_t b, int64_t px,
                                             int64_t py) {
  const int64_t yy = py + oy, xx = px + ox;
  if ((uint64_t)b >= (uint64_t)B || yy < 0 || yy >= h || xx < 0 || xx >= w) return -1;
  return ((b * Cin + ci) * h + yy) * w + xx;
}
// the same for column col = (ci k + dy) k + dx of the window
__device__ __forceinline__ int64_t window_at(int col, int k, int pad, int Cin, int h, int w, int B, int64_t b,
                                             int64_t px, int64_t py) {
  const int ci = col / (k * k), rem = col - ci * k * k, dy = rem / k, dx = rem - dy * k;
  if ((uint64_t)px >= (uint64_t)(w + 2 * pad - k + 1) || (uint64_t)py >= (uint64_t)(h + 2 * pad - k + 1)) return -1;
  return window_el(ci, dy - pad, dx - pad, Cin, h, w, B, b, px, py);
}

// One chunk's dW partial with the nodes as the MFMA's K: a wave owns 16 output channels x 64 columns; lane (i, q)
// feeds A[co i][node q] and B[node q][column i] and holds rows 4 q + r, column i.
__global__ __launch_bounds__(256) void node_conv_wgrad_mfma_kernel(const float* __restrict__ g,
                                                                   const float* __restrict__ raw,
                                                                   const int64_t* __restrict__ jdet,
                                                                   const int64_t* __restrict__ bidx, int64_t N, int B,
                                                                   int Cin, int h, int w, int Cout, int k, int pad,
                                                                   float* __restrict__ part, int len) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
  const int64_t chunk = blockIdx.x;
  const int co0 = (blockIdx.y * 4 + wave) * 16;
  if (co0 >= Cout) return;                                              // (Cout is a multiple of 16)
  const int c0 = blockIdx.z * 64, KC = Cin * k * k;
  f32x4 acc[4];
  bool okt[4];
  int col[4], oy[4], ox[4];
  int64_t off[4];                       // of the column's window element from the node's pixel in plane 0
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    okt[t] = c0 + 16 * t < KC;
    col[t] = okt[t] ? c0 + 16 * t + i : 0;
    const int ci = col[t] / (k * k), rem = col[t] - ci * k * k;
    oy[t] = rem / k - pad, ox[t] = rem % k - pad;
    off[t] = ((int64_t)ci * h + oy[t]) * w + ox[t];
  }
  // SB steps of four nodes at a time: their node records, then their window elements, are loaded together (the
  // loads of a step depend on each other, not on the other steps'), then the MFMAs run in node order
  constexpr int SB = 8;
  for (int s0 = 0; s0 < kChunk / 4; s0 += SB) {
    const int64_t base = chunk * kChunk + 4 * s0;
    if (base >= N) break;                                               // wave-uniform
    int64_t px[SB], py[SB], b[SB];
    float a[SB], v[SB][4];
    bool okn[SB];
#pragma unroll
    for (int u = 0; u < SB; ++u) {
      okn[u] = base + 4 * u + q < N;
      const size_t nc = okn[u] ? (size_t)(base + 4 * u + q) : 0;
      px[u] = jdet[nc * 3], py[u] = jdet[nc * 3 + 1], b[u] = bidx[nc];
      a[u] = g[nc * Cout + co0 + i];
    }
#pragma unroll
    for (int u = 0; u < SB; ++u) {
      // a node on the conv's output map (the forward's precondition): its coordinates fit an int, the window tests
      // are 32-bit
      const bool on = okn[u] && (uint64_t)b[u] < (uint64_t)B && (uint64_t)px[u] < (uint64_t)(w + 2 * pad - k + 1) &&
                      (uint64_t)py[u] < (uint64_t)(h + 2 * pad - k + 1);
      const int xi = on ? (int)px[u] : 0, yi = on ? (int)py[u] : 0;
      const int64_t at0 = on ? ((b[u] * Cin) * h + yi) * w + xi : 0;
      a[u] = okn[u] ? a[u] : 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const bool ok = on && okt[t] && (unsigned)(yi + oy[t]) < (unsigned)h && (unsigned)(xi + ox[t]) < (unsigned)w;
        const float x = raw[ok ? at0 + off[t] : 0];
        v[u][t] = ok ? x : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < SB; ++u)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = mfma4(a[u], v[u][t], acc[t]);
  }
  float* out = part + (size_t)chunk * len;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (!okt[t]) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) out[(size_t)(co0 + 4 * q + r) * KC + col[t]] = acc[t][r];
  }
}

__global__ __launch_bounds__(256) void node_conv_wgrad_fma_kernel(const float* __restrict__ g,
                                                                  const float* __restrict__ raw,
                                                                  const int64_t* __restrict__ jdet,
                                                                  const int64_t* __restrict__ bidx, int64_t N, int B,
                                                                  int Cin, int h, int w, int Cout, int k, int pad,
                                                                  float* __restrict__ part, int len) {
  const int KC = Cin * k * k;
  const int el = blockIdx.y * 256 + threadIdx.x;
  if (el >= Cout * KC) return;
  const int co = el / KC, col = el - co * KC;
  const int64_t chunk = blockIdx.x, n0 = chunk * kChunk, n1 = std::min<int64_t>(n0 + kChunk, N);
  float acc = 0.f;
  for (int64_t n = n0; n < n1; ++n) {
    const int64_t at = window_at(col, k, pad, Cin, h, w, B, bidx[n], jdet[n * 3], jdet[n * 3 + 1]);
    const float v = raw[at >= 0 ? at : 0];
    acc = fmaf(g[(size_t)n * Cout + co], at >= 0 ? v : 0.f, acc);
  }
  part[(size_t)chunk * len + el] = acc;
}

// One chunk's db partial (behind the chunk's dW): the rows of g added in node order
__global__ __launch_bounds__(256) void node_conv_bgrad_kernel(const float* __restrict__ g, int64_t N, int Cout,
                                                              float* __restrict__ part, int len, int off) {
  const int co = blockIdx.y * 256 + threadIdx.x;
  if (co >= Cout) return;
  const int64_t chunk = blockIdx.x, n0 = chunk * kChunk, n1 = std::min<int64_t>(n0 + kChunk, N);
  float acc = 0.f;
  for (int64_t n = n0; n < n1; ++n) acc += g[(size_t)n * Cout + co];
  part[(size_t)chunk * len + off + co] = acc;
}

// out[grp] = the pairwise tree over in[32 grp .. 32 grp + 31] (zeros past n_in), for the elements lo .. hi - 1 of a
// partial. The last pass (one group left) writes the gradients instead: elements below nW to dW, the others to db.
__global__ __launch_bounds__(256) void node_conv_tree_kernel(const float* __restrict__ in, int64_t n_in, int len, int lo,
                                                             int hi, float* __restrict__ out, float* __restrict__ dW,
                                                             float* __restrict__ db, int nW) {
  const int el = lo + blockIdx.y * 256 + threadIdx.x;
  if (el >= hi) return;
  const int64_t grp = blockIdx.x, c0 = grp * kLeaves;
  float v[kLeaves];
#pragma unroll
  for (int k = 0; k < kLeaves; ++k) {                          // (unconditional loads from a clamped partial, masked after)
    const float x = in[(size_t)(c0 + k < n_in ? c0 + k : n_in - 1) * len + el];
    v[k] = c0 + k < n_in ? x : 0.f;
  }
#pragma unroll
  for (int s = 1; s < kLeaves; s <<= 1)
#pragma unroll
    for (int k = 0; k < kLeaves; k += 2 * s) v[k] += v[k + s];
  if (out)
    out[(size_t)grp * len + el] = v[0];
  else if (el < nW)
    dW[el] = v[0];
  else
    db[el - nW] = v[0];
}

inline int64_t chunks_of(int64_t N) { return (N + kChunk - 1) / kChunk; }
inline int64_t groups_of(int64_t n) { return (n + kLeaves - 1) / kLeaves; }
inline size_t part_floats(int Cin, int Cout, int k) { return (size_t)Cout * Cin * k * k + Cout; }

// the shape checks the conv entries share; 0 or an error code with the message set
int check_conv(const char* fn, int64_t N, int B, int Cin, int h, int w, int Cout, int k, int pad) {
  PEMP_CHECK_ARG(N >= 0 && B > 0 && Cin > 0 && h > 0 && w > 0 && Cout > 0 && k >= 1 && pad >= 0 && pad < k,
                 "%s: bad sizes (N = %lld, B = %d, Cin = %d, h = %d, w = %d, Cout = %d, k = %d, 0 <= pad < k)", fn,
                 (long long)N, B, Cin, h, w, Cout, k);
  if (Cout > kMaxCout || k > kMaxK) {
    set_error("%s: Cout = %d, k = %d beyond the forward's limits %d, %d", fn, Cout, k, kMaxCout, kMaxK);
    return PEMP_ERR_UNSUPPORTED;
  }
  PEMP_CHECK_ARG((size_t)Cin * (k + 1) * (k + 1) * 4 <= 64 * 1024,
                 "%s: Cin * (k+1)^2 patch exceeds 64 KB of LDS (the forward's limit)", fn);
  PEMP_CHECK_ARG(h + 2 * pad - k + 1 > 0 && w + 2 * pad - k + 1 > 0, "%s: conv output empty", fn);
  if (N * k * k > INT_MAX || (int64_t)B * Cin * h * w > (1ll << 40) || part_floats(Cin, Cout, k) > (size_t)INT_MAX) {
    set_error("%s: N k^2 = %lld rows or the map exceed the index range", fn, (long long)(N * k * k));
    return PEMP_ERR_UNSUPPORTED;
  }
  return PEMP_OK;
}

int launch_pixels(const float* D, int64_t M, int C, const int64_t* skey, const int64_t* perm, int B, int64_t hw,
                  float* out, hipStream_t st) {
  ProfScope prof("node_grad_pixels", st);
  node_grad_pixels_kernel<<<dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st>>>(D, M, C, skey, perm, (int64_t)B * hw, hw,
                                                                               out);
  PEMP_LAUNCH_CHECK();
  return PEMP_OK;
}

}  // namespace
}  // namespace pemp

using namespace pemp;

extern "C" int pemp_node_grad_pixels(const float* g, int64_t N, int C, const int64_t* sorted_keys, const int64_t* perm,
                                     int B, int H, int W, float* dfeat, void* stream) {
  PEMP_CHECK_ARG(N >= 0 && C > 0 && B > 0 && H > 0 && W > 0, "pemp_node_grad_pixels: bad sizes (N = %lld, C = %d, B = %d, "
                 "H = %d, W = %d)", (long long)N, C, B, H, W);
  PEMP_CHECK_ARG(dfeat, "pemp_node_grad_pixels: NULL dfeat");
  PEMP_CHECK_ARG(N == 0 || (g && sorted_keys && perm), "pemp_node_grad_pixels: NULL g / sorted_keys / perm");
  if (N > INT_MAX || (int64_t)B * C * H * W > (1ll << 40)) {
    set_error("pemp_node_grad_pixels: N = %lld or the map exceed the index range", (long long)N);
    return PEMP_ERR_UNSUPPORTED;
  }
  hipStream_t st = as_stream(stream);
  PEMP_HIP(hipMemsetAsync(dfeat, 0, (size_t)B * C * H * W * sizeof(float), st));
  if (N == 0) return PEMP_OK;
  return launch_pixels(g, N, C, sorted_keys, perm, B, (int64_t)H * W, dfeat, st);
}

extern "C" size_t pemp_node_conv_workspace_size(int64_t N, int Cin, int Cout, int ksize) {
  if (N <= 0 || Cin <= 0 || Cout <= 0 || Cout > kMaxCout || ksize < 1 || ksize > kMaxK) return 0;
  const int64_t n = chunks_of(N);
  return align_up((size_t)N * ksize * ksize * Cin * sizeof(float), 256) +
         (size_t)(n + groups_of(n)) * part_floats(Cin, Cout, ksize) * sizeof(float);
}

extern "C" int pemp_node_conv_bwd(const float* g, const float* raw, const float* weight_khwc, const int64_t* joint_det,
                                  const int64_t* batch_index, int64_t N, int B, int Cin, int h, int w, int Cout,
                                  int ksize, int pad, const int64_t* sorted_keys, const int64_t* perm, float* draw,
                                  float* dW, float* db, void* workspace, size_t workspace_bytes, void* stream) {
  const int k = ksize;
  if (int rc = check_conv("pemp_node_conv_bwd", N, B, Cin, h, w, Cout, k, pad)) return rc;
  const int KC = Cin * k * k;
  if (N > 0) {
    PEMP_CHECK_ARG(g && joint_det && batch_index, "pemp_node_conv_bwd: NULL g / joint_det / batch_index");
    PEMP_CHECK_ARG(!draw || (weight_khwc && sorted_keys && perm), "pemp_node_conv_bwd: draw needs weight_khwc, "
                   "sorted_keys and perm");
    PEMP_CHECK_ARG(!(dW) || raw, "pemp_node_conv_bwd: dW needs raw");
    const size_t need = pemp_node_conv_workspace_size(N, Cin, Cout, k);
    PEMP_CHECK_ARG(workspace && workspace_bytes >= need, "pemp_node_conv_bwd: workspace of %zu bytes, %zu needed",
                   workspace ? workspace_bytes : (size_t)0, need);
    PEMP_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "pemp_node_conv_bwd: workspace not 16-byte aligned");
  }
  hipStream_t st = as_stream(stream);
  if (draw) PEMP_HIP(hipMemsetAsync(draw, 0, (size_t)B * Cin * h * w * sizeof(float), st));
  if (N == 0) {                                   // no node: zero gradients (where given), no launch
    if (dW) PEMP_HIP(hipMemsetAsync(dW, 0, (size_t)Cout * KC * sizeof(float), st));
    if (db) PEMP_HIP(hipMemsetAsync(db, 0, (size_t)Cout * sizeof(float), st));
    return PEMP_OK;
  }
  const bool mfma = Cin % 16 == 0 && Cout % 16 == 0;
  float* D = static_cast<float*>(workspace);
  const int64_t M = N * k * k;
  if (draw) {
    {
      ProfScope prof("node_conv_bwd", st);
      if (mfma)
        node_conv_dgemm_mfma_kernel<<<dim3((unsigned)((N + 63) / 64), (unsigned)((KC + 63) / 64)), dim3(256), 0, st>>>(
            g, weight_khwc, N, Cout, KC, D);
      else
        node_conv_dgemm_fma_kernel<<<dim3((unsigned)((N * KC + 255) / 256)), dim3(256), 0, st>>>(g, weight_khwc, N, Cout,
                                                                                                 KC, D);
      PEMP_LAUNCH_CHECK();
    }
    if (int rc = launch_pixels(D, M, Cin, sorted_keys, perm, B, (int64_t)h * w, draw, st)) return rc;
  }
  if (!dW && !db) return PEMP_OK;
  const int64_t nchunk = chunks_of(N);
  const int len = (int)part_floats(Cin, Cout, k), nW = Cout * KC;
  float* bufA = reinterpret_cast<float*>(static_cast<char*>(workspace) + align_up((size_t)M * Cin * sizeof(float), 256));
  float* bufB = bufA + (size_t)nchunk * len;
  {
    ProfScope prof("node_conv_bwd", st);
    if (dW) {
      if (mfma)
        node_conv_wgrad_mfma_kernel<<<dim3((unsigned)nchunk, (unsigned)((Cout + 63) / 64), (unsigned)((KC + 63) / 64)),
                                      dim3(256), 0, st>>>(g, raw, joint_det, batch_index, N, B, Cin, h, w, Cout, k, pad,
                                                          bufA, len);
      else
        node_conv_wgrad_fma_kernel<<<dim3((unsigned)nchunk, (unsigned)((nW + 255) / 256)), dim3(256), 0, st>>>(
            g, raw, joint_det, batch_index, N, B, Cin, h, w, Cout, k, pad, bufA, len);
      PEMP_LAUNCH_CHECK();
    }
    if (db) {
      node_conv_bgrad_kernel<<<dim3((unsigned)nchunk, (unsigned)((Cout + 255) / 256)), dim3(256), 0, st>>>(g, N, Cout, bufA,
                                                                                                          len, nW);
      PEMP_LAUNCH_CHECK();
    }
  }
  ProfScope prof("node_conv_tree", st);
  const int lo = dW ? 0 : nW, hi = db ? len : nW;
  const float* cur = bufA;
  float* other = bufB;
  for (int64_t n = nchunk;;) {
    const int64_t ng = groups_of(n);
    const bool last = ng == 1;
    node_conv_tree_kernel<<<dim3((unsigned)ng, (unsigned)((hi - lo + 255) / 256)), dim3(256), 0, st>>>(
        cur, n, len, lo, hi, last ? nullptr : other, dW, db, nW);
    PEMP_LAUNCH_CHECK();
    if (last) break;
    float* written = other;
    other = const_cast<float*>(cur);
    cur = written;
    n = ng;
  }
  return PEMP_OK;
}
