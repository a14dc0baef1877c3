// The type-major edge order of the MPN forward (mpn.hip has the overview): the sorting prepare, the closed-form prepare
// of a fully-connected batch, the symmetric prepare and the knn prepare, with their launch functions.
#include "mpn_internal.h"
#include "mpn_order.h"

namespace pemp {
namespace {

// First kernel of a forward: zero the counters.
__global__ __launch_bounds__(256) void zero_words_kernel(int* __restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = 0;
}

// ---------------------------------------------------------------------------------------------
// Prepare: type-major counting sort of the edges (deterministic: ties kept in edge-id order)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mpn_count_kernel(const int64_t* __restrict__ ei, const int64_t* __restrict__ types,
                                                        int64_t ts, int64_t N, int64_t E, int T, int* __restrict__ cnt,
                                                        int* __restrict__ err) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = ei[e], d = ei[E + e];
    if (s < 0 || s >= N || d < 0 || d >= N) { atomicOr(err, 1); continue; }
    const int64_t t = T == 1 ? 0 : types[s * ts];   // MPLayer (one message MLP) ignores types
    if (t < 0 || t >= T) { atomicOr(err, 2); continue; }
    atomicAdd(&cnt[t * N + d], 1);
  }
}

// Exclusive scan of the (type, target) counts into the segment starts seg, and the type split (mpn_order.h) of
// the edge-step grid (wg_start). One 1024-thread block, 16 contiguous counts per thread per pass
// (all loads of a pass in flight together), carry across passes. The per-type segment starts
// seg[t*N] are captured from LDS on the way out (no read-back of seg).
constexpr int SCAN_SPT = 16;
// With `flags` (the symmetric prepare, which has no zeroing launch): err[0..3] are written here, err[0] = the OR of
// flags[0..nflags) | 4 if the counts do not sum to E_all.
__global__ __launch_bounds__(1024) void mpn_scan_kernel(const int* __restrict__ cnt, int64_t K, int64_t N, int T,
                                                        int G, int* __restrict__ seg, int* __restrict__ wg_start,
                                                        const int* __restrict__ flags = nullptr, int64_t nflags = 0,
                                                        int64_t E_all = 0, int* __restrict__ err = nullptr) {
  __shared__ int sh[20 + 2 * (MAXT + 1)];
  __shared__ int out[1024 * SCAN_SPT];          // one pass of exclusive offsets, stored coalesced
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x <= T) sh[20 + threadIdx.x] = 0;   // (K = 0: every segment start is 0)
  if (threadIdx.x == 0) sh[17] = 0;
  __syncthreads();
  int carry = 0;
  for (int64_t base = 0; base < K; base += 1024 * SCAN_SPT) {
    const int64_t k0 = base + (int64_t)threadIdx.x * SCAN_SPT;
    int v[SCAN_SPT];
    if (k0 + SCAN_SPT <= K) {
#pragma unroll
      for (int j = 0; j < SCAN_SPT; j += 4) {
        const int4 q = *reinterpret_cast<const int4*>(cnt + k0 + j);
        v[j] = q.x; v[j + 1] = q.y; v[j + 2] = q.z; v[j + 3] = q.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < SCAN_SPT; ++j) v[j] = k0 + j < K ? cnt[k0 + j] : 0;
    }
    int local = 0;
#pragma unroll
    for (int j = 0; j < SCAN_SPT; ++j) local += v[j];
    int x = local;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(x, off);
      if (lane >= off) x += o;
    }
    if (lane == 63) sh[wave] = x;
    __syncthreads();
    if (wave == 0) {
      const int wv = lane < 16 ? sh[lane] : 0;
      int inc = wv;
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) {
        const int o = __shfl_up(inc, off);
        if (lane >= off) inc += o;
      }
      if (lane < 16) sh[lane] = inc - wv;
      if (lane == 15) sh[16] = inc;
    }
    __syncthreads();
    int run = carry + sh[wave] + x - local;
#pragma unroll
    for (int j = 0; j < SCAN_SPT; ++j) { out[threadIdx.x * SCAN_SPT + j] = run; run += v[j]; }
    carry += sh[16];
    __syncthreads();
    const int64_t lim = K - base < 1024 * SCAN_SPT ? K - base : 1024 * SCAN_SPT;
    for (int k = threadIdx.x; k < lim; k += 1024) seg[base + k] = out[k];
    if (threadIdx.x < T) {                                  // seg[t * N] of this pass
      const int64_t key = (int64_t)threadIdx.x * N;
      if (key >= base && key < base + lim) sh[20 + threadIdx.x] = out[key - base];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    seg[K] = carry;
    sh[20 + T] = carry;
  }
  if (flags) {
    int f = 0;
    for (int64_t i = threadIdx.x; i < nflags; i += 1024) f |= flags[i];
    if (f) atomicOr(&sh[17], f);                             // (sh[17..19]: free after the scan)
  }
  __syncthreads();
  if (flags && threadIdx.x < 4) err[threadIdx.x] = threadIdx.x ? 0 : (sh[17] | (carry != E_all ? 4 : 0));
  type_split(sh + 20, carry, T, G, sh + 20 + MAXT + 1, wg_start);
}

// counts are consumed here: cnt[key] counts down, so edges land in a key's segment in arbitrary
// order; mpn_segsort_kernel restores edge-id order inside each segment.
__global__ __launch_bounds__(256) void mpn_scatter_kernel(const int64_t* __restrict__ ei, const int64_t* __restrict__ types,
                                                          int64_t ts, int64_t N, int64_t E, int T, const int* __restrict__ seg,
                                                          int* __restrict__ cnt, int* __restrict__ perm) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = ei[e], d = ei[E + e];
    if (s < 0 || s >= N || d < 0 || d >= N) continue;
    const int64_t t = T == 1 ? 0 : types[s * ts];
    if (t < 0 || t >= T) continue;
    const int64_t key = t * N + d;
    perm[seg[key] + atomicSub(&cnt[key], 1) - 1] = (int)e;
  }
}

// 16 lanes per (type, target) key: order the key's edges by original id (rank by counting).
__global__ __launch_bounds__(256) void mpn_segsort_kernel(const int64_t* __restrict__ ei, int64_t E, int64_t K,
                                                          const int* __restrict__ seg, const int* __restrict__ perm,
                                                          int* __restrict__ s_src, int* __restrict__ s_dst,
                                                          int* __restrict__ s_orig) {
  const int sub = threadIdx.x & 15;
  const int64_t key = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (key >= K) return;
  const int s0 = seg[key], n = seg[key + 1] - s0;
  for (int a = sub; a < n; a += 16) {
    const int v = perm[s0 + a];
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += perm[s0 + j] < v;
    const int pos = s0 + rank;
    s_orig[pos] = v;
    s_src[pos] = (int)ei[v];
    s_dst[pos] = (int)ei[E + v];
  }
}

__global__ __launch_bounds__(256) void fully_prepare_kernel(FullyPrepArgs a) {
  __shared__ FullyPrepLds s;
  fully_prepare_role(a, s, blockIdx.x, blockIdx.y, gridDim.x);
}

// ---- Symmetric prepare: edge_index sorted by (src, dst) without duplicates and symmetric (PyG to_undirected's
// coalesced output: knn_mpn_graph, feature_knn_mpn_graph, score_based_graph, ConstructGraph.py:363-422).
// The incoming edges of d are then the entries of row d read backwards: segment (t, d) = the type-t entries of
// row d in ascending source order (= edge-id order, the sorting prepare's tie order), and the id of the incoming
// edge (x -> d) is the position of d in row x. Three launches, no zeroing, no atomics on the data path:
//   sym_rows_kernel   one wave per node n: row n's bounds (64-way probes + one coalesced run), its entries packed
//                     as (dst | type(dst) << 24), the (type, n) counts written directly (all T of them), checks;
//   mpn_scan_kernel   (shared with the sorting prepare) + the reduction of the per-node check flags;
//   sym_place_kernel  one wave per node d: each entry's rank among the same-type entries before it (ballots),
//                     its segment slot, and the incoming edge's id by a binary search of d in row x.
// Measured alternatives: per-image blocks over LDS adjacency bit rows (8 busy CUs) 31-35 us; a per-edge walk along
// row d (knn rows hold ~60 entries) 25 us for the placement alone; the sorting prepare 25 us (C3 knn).

constexpr unsigned SYM_NMASK = (1u << SYM_TBITS) - 1u;   // the node id of a packed row entry (SYM_TBITS: mpn_internal.h)

// first position p in [0, n) with a[p] >= key (n if none), by one wave: 64-way probes per round (E = 250k:
// 3 rounds of one load per lane, no barriers); bounded on an unsorted list too
__device__ int64_t wave_lower_bound(const int64_t* __restrict__ a, int64_t n, int64_t key) {
  const int lane = threadIdx.x & 63;
  int64_t lo = 0, hi = n;                          // a[< lo] < key <= a[>= hi]
  while (lo < hi) {                                // (uniform)
    const int64_t s = (hi - lo + 63) / 64;
    const int64_t q = lo + (int64_t)lane * s;
    const unsigned long long m = __ballot(q < hi && a[q] < key);
    const int c = __popcll(m);                     // probes below key form a prefix
    if (c == 0) break;                             // a[lo] >= key
    const int64_t nlo = lo + (int64_t)(c - 1) * s + 1, nhi = min(hi, lo + (int64_t)c * s);
    lo = nlo;
    hi = nhi;
  }
  return lo;
}

__global__ __launch_bounds__(256) void sym_rows_kernel(const int64_t* __restrict__ ei, const int64_t* __restrict__ types,
                                                       int64_t ts, int64_t N, int64_t E, int T, int* __restrict__ cnt,
                                                       int2* __restrict__ rows, unsigned* __restrict__ packed,
                                                       int* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;                                         // (wave-uniform)
  const int64_t r0 = wave_lower_bound(ei, E, n);              // row n starts here if the list is sorted
  int f = 0, tcount = 0;                                      // lane t < T: type-t entries of row n
  int64_t r = r0, prev = -1;
  for (;;) {                                                  // the run of source n, 64 entries per round
    const int64_t e = r + lane;
    const bool in = e < E && ei[e] == n;
    const unsigned long long out = __ballot(!in);
    const int len = out ? __builtin_ctzll(out) : 64;          // (entries past a mismatch are not the row's)
    const bool mine = lane < len;
    const int64_t d = mine ? ei[E + e] : 0;
    int t = 31;
    if (mine) {
      if (d < 0 || d >= N) f |= 1;
      else {
        const int64_t tt = T == 1 ? 0 : types[d * ts];
        if (tt >= 0 && tt < T) t = (int)tt;
        else f |= 2;                                          // (d is a source too: the list is symmetric)
      }
      packed[e] = (unsigned)d | ((unsigned)t << SYM_TBITS);
    }
    const int64_t dp = __shfl_up(d, 1);
    if (mine && (lane ? dp : prev) >= d) f |= 4;              // targets of a row strictly ascending
    unsigned long long rem = __ballot(mine && t < T);
    while (rem) {                                             // one round per distinct type in the chunk
      const int tu = __shfl(t, __builtin_ctzll(rem));
      const unsigned long long m = __ballot(mine && t == tu);
      if (lane == tu) tcount += __popcll(m);
      rem &= ~m;
    }
    prev = __shfl(d, 63);
    r += len;
    if (len < 64) break;
  }
  if ((r0 > 0 && ei[r0 - 1] >= n) || (r < E && ei[r] < n)) f |= 4;   // neighbouring runs: ascending sources
  if (lane < T) cnt[(int64_t)lane * N + n] = tcount;
  for (int o = 32; o; o >>= 1) f |= __shfl_xor(f, o);
  if (lane == 0) {
    rows[n] = make_int2((int)r0, (int)r);
    flags[n] = f;
  }
}

__global__ __launch_bounds__(256) void sym_place_kernel(int64_t N, int T, const int* __restrict__ seg,
                                                        const int2* __restrict__ rows,
                                                        const unsigned* __restrict__ packed, int* __restrict__ s_src,
                                                        int* __restrict__ s_dst, int* __restrict__ s_orig,
                                                        int* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const int64_t d = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (d >= N) return;                                         // (wave-uniform)
  const int2 rb = rows[d];
  const unsigned long long below = (1ull << lane) - 1ull;
  int carry = 0, bad = 0;                                     // lane t: type-t entries of row d in earlier chunks
  for (int c = rb.x; c < rb.y; c += 64) {
    const int e = c + lane;
    const bool mine = e < rb.y;
    const unsigned w = mine ? packed[e] : 0u;
    const int x = (int)(w & SYM_NMASK), t = (int)(w >> SYM_TBITS);
    const bool ok = mine && t < T;
    int rank = 0;
    unsigned long long rem = __ballot(ok);
    while (rem) {
      const int tu = __shfl(t, __builtin_ctzll(rem));
      const unsigned long long m = __ballot(ok && t == tu);
      const int cu = __shfl(carry, tu);
      if (ok && t == tu) rank = cu + __popcll(m & below);
      if (lane == tu) carry += __popcll(m);
      rem &= ~m;
    }
    if (ok) {
      const int pos = seg[(int64_t)t * N + d] + rank;
      const int2 rx = rows[x];                                // row x holds d if the list is symmetric
      int lo = rx.x, hi = rx.y;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int)(packed[mid] & SYM_NMASK) < (int)d) lo = mid + 1; else hi = mid;
      }
      const bool found = lo < rx.y && (int)(packed[lo] & SYM_NMASK) == (int)d;
      bad |= !found;
      s_src[pos] = x;
      s_dst[pos] = (int)d;
      s_orig[pos] = found ? lo : 0;
    }
  }
  if (__ballot(bad) && lane == 0) atomicOr(err, 8);          // (x -> d) missing: not symmetric
}

// Symmetric prepare, step 2 (instead of the one-block mpn_scan): one 1024-thread block per source type t. The
// segment starts are seg[t N + d] = base_t + sum_{d' < d} cnt[t, d'] with base_t = the edges of all types before
// t: every block sums every type's counts (one wave per type, T N ints, L2-resident) and scans its own type's N
// counts, so the T scans run side by side instead of one block walking all T N counts. The last block also writes
// seg[T N], the edge passes' type split (wg_start) and the contract flags (err[0..3]), as mpn_scan does.
__global__ __launch_bounds__(1024) void sym_scan_kernel(const int* __restrict__ cnt, int64_t N, int T, int G,
                                                        int* __restrict__ seg, int* __restrict__ wg_start,
                                                        const int* __restrict__ flags, int64_t E_all,
                                                        int* __restrict__ err) {
  __shared__ int tb[MAXT + 1], gt[MAXT + 1], wsum[16], sh[4];
  __shared__ int out[1024 * SCAN_SPT];
  const int t = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool last = t == T - 1;
  if (threadIdx.x < 4) sh[threadIdx.x] = 0;
  // every type's total, one wave per type (wave w: types w, w + 16), all of a wave's loads in flight together
  for (int tt = wave; tt < T; tt += 16) {
    int v = 0;
    const int* ct = cnt + (int64_t)tt * N;
#pragma unroll 8
    for (int64_t n = lane; n < N; n += 64) v += ct[n];
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) tb[tt] = v;
  }
  if (last) {                                          // the contract flags of every node (sym_rows_kernel)
    int f = 0;
    for (int64_t i = threadIdx.x; i < N; i += 1024) f |= flags[i];
    if (f) atomicOr(&sh[0], f);
  }
  __syncthreads();
  int base = 0;
  for (int tt = 0; tt < t; ++tt) base += tb[tt];
  // this type's segment starts: passes of 1024 x SCAN_SPT counts, carry across passes
  int carry = base;
  const int* c = cnt + (int64_t)t * N;
  for (int64_t b0 = 0; b0 < N; b0 += 1024 * SCAN_SPT) {
    const int64_t k0 = b0 + (int64_t)threadIdx.x * SCAN_SPT;
    int v[SCAN_SPT];
#pragma unroll
    for (int j = 0; j < SCAN_SPT; ++j) v[j] = k0 + j < N ? c[k0 + j] : 0;
    int local = 0;
#pragma unroll
    for (int j = 0; j < SCAN_SPT; ++j) local += v[j];
    int x = local;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(x, off);
      if (lane >= off) x += o;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w2 = 0; w2 < 16; ++w2) {
      before += w2 < wave ? wsum[w2] : 0;
      all += wsum[w2];
    }
    int run = carry + before + x - local;
#pragma unroll
    for (int j = 0; j < SCAN_SPT; ++j) { out[threadIdx.x * SCAN_SPT + j] = run; run += v[j]; }
    carry += all;
    __syncthreads();
    const int64_t lim = N - b0 < 1024 * SCAN_SPT ? N - b0 : 1024 * SCAN_SPT;
    for (int64_t k = threadIdx.x; k < lim; k += 1024) seg[(int64_t)t * N + b0 + k] = out[k];
    __syncthreads();
  }
  if (!last) return;                                   // (block-uniform)
  if (threadIdx.x == 0) {                              // type starts for the split; the total closes seg
    int acc = 0;
    for (int tt = 0; tt < T; ++tt) {
      const int v = tb[tt];
      tb[tt] = acc;
      acc += v;
    }
    tb[T] = acc;
    seg[(int64_t)T * N] = acc;
    sh[1] = acc;
  }
  __syncthreads();
  if (threadIdx.x < 4) err[threadIdx.x] = threadIdx.x ? 0 : (sh[0] | (sh[1] != E_all ? 4 : 0));
  type_split(tb, sh[1], T, G, gt, wg_start);
}

// ---- knn prepare (pemp_mpn_forward_knn): the graph constructor's knn graph (knn_mpn_graph / feature_knn_mpn_graph,
// ConstructGraph.py:363-374) handed over as the bit rows its build emitted the edges from (graph.hip,
// knn_rows_kernel / knn_emit_rows_kernel): row n = bit mask R[n][w] over the image-local nodes 64 w + j, the edge
// (n -> m) has id ebase_b + rowstart[n] + #{bits of row n below m}, and R is symmetric (A | A^T). Then
//   cnt(t, d)  = sum_w popcount(R[d][w] & M_t[b][w])     (M_t: the type-t nodes of d's image as bit words),
//   E_t        = sum over type-t nodes x of popcount(R[x]) (symmetry: the type-t sources of every row),
//   the (x -> d) id is a popcount of row x below d (no search),
// so the three launches of the symmetric prepare (rows with their binary searches, the scan, the placement)
// collapse into one: blocks (t, chunk of KP_CH rows) each count and scan all N rows for type t in LDS (one round
// of row loads, the type masks from the rows' own types) and place their chunk's sources through an LDS list,
// entry-parallel (a second round of loads: one word of each source row and its start). The same arrays as
// launch_prepare_sym's (tested bit for bit).
#ifndef PEMP_KP_CLOCKS
#define PEMP_KP_CLOCKS 0
#endif
__device__ __forceinline__ int kp_image(const int* noff, int B, int d) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (noff[mid] <= d) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(1024) void knn_prepare_kernel(KnnPrepArgs a) {
  __shared__ unsigned long long M[KP_MAXB * KP_W];   // bit j of word (b, w): node 64 w + j of image b has type t
  __shared__ int noff[KP_MAXB + 1], ebase[KP_MAXB + 1];
  __shared__ int tot[MAXT + 1], tst[MAXT + 1], gt[MAXT], wsum[16];
  __shared__ int bad_sh;
  __shared__ int cs[KP_MAXN];                        // cnt(t, d), then the segment starts
  __shared__ unsigned short pw[KP_MAXN][KP_W];       // entries of row n in its words before w
  __shared__ int lst[KP_LIST];                       // the chunk's sources in segment order: x << 10 | (d - d0)
  __shared__ int cend;
  constexpr int SPT = KP_MAXN / 1024;
  const int t = blockIdx.x, T = a.T, B = a.B, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = (int)a.N;
#if PEMP_KP_CLOCKS   // diagnostics: per-phase wall clock (100 MHz) of two blocks, printed
  long long clk[6];
  clk[0] = wall_clock64();
#define KP_CLK(i) clk[i] = wall_clock64()
#else
#define KP_CLK(i) (void)0
#endif
  // the offsets first (the in-order load counter: the barrier below then waits for them, not for the rows), then
  // the words and types of this thread's first two rows (words past a row's image are masked below: R is [N][KP_W])
  // (clamped indices, no branches: straight-line loads let the barrier wait count exactly)
  const int no = (int)a.node_off[min(tid, B)];
  const int ec = (int)a.ecount[min(lane, B - 1)];
  __builtin_amdgcn_sched_barrier(0);                 // (keeps the offsets' loads ahead of the rows')
  unsigned long long rr[2][KP_W];
  int64_t tr[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int d = min(tid + 1024 * i, N - 1);        // (rows past N are loaded but never used)
#pragma unroll
    for (int w = 0; w < KP_W; ++w) rr[i][w] = a.R[(int64_t)d * KP_W + w];
    tr[i] = a.types[(int64_t)d * a.ts];
  }
  if (T == 1) tr[0] = tr[1] = 0;                     // one message MLP ignores the types, like mpn_count_kernel
  if (tid <= B) noff[tid] = no;
  if (wave == 1) {                                   // edge id base of every image (B <= 64)
    const int e = lane < B ? ec : 0;
    int x = e;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(x, o);
      if (lane >= o) x += v;
    }
    if (lane < B) ebase[lane] = x - e;
    if (lane == B - 1) ebase[B] = x;
  }
  if (tid <= MAXT) tot[tid] = 0;
  if (tid == 0) bad_sh = 0;
  for (int q = tid; q < B * KP_W; q += 1024) M[q] = 0ull;
  __syncthreads();
  KP_CLK(1);
  // type-t masks of every image word, from the rows' own types (no second round of loads)
  bool bad = false;
  auto mark = [&](int d, int64_t tt) {
    if (tt < 0 || tt >= T) bad = true;               // skipped as a source, like mpn_count_kernel
    if (tt == t) {
      const int b = kp_image(noff, B, d), dl = d - noff[b];
      atomicOr(&M[b * KP_W + (dl >> 6)], 1ull << (dl & 63));
    }
  };
#pragma unroll
  for (int i = 0; i < 2; ++i)
    if (tid + 1024 * i < N) mark(tid + 1024 * i, tr[i]);
  for (int d = tid + 2048; d < N; d += 1024) mark(d, T == 1 ? 0 : a.types[(int64_t)d * a.ts]);
  if (__ballot(bad) && lane == 0) bad_sh = 1;
  __syncthreads();
  KP_CLK(2);
  // every row: cnt(t, d), its word prefix counts and its degree (the per-type edge totals)
  auto row = [&](int d, const unsigned long long* v, int64_t tt) {
    const int b = kp_image(noff, B, d), nb = noff[b + 1] - noff[b], wpr = (nb + 63) >> 6;
    int c = 0, deg = 0;
#pragma unroll
    for (int w = 0; w < KP_W; ++w) {
      pw[d][w] = (unsigned short)deg;
      if (w < wpr) {
        c += __popcll(v[w] & M[b * KP_W + w]);
        deg += __popcll(v[w]);
      }
    }
    cs[d] = c;
    if (tt >= 0 && tt < T) atomicAdd(&tot[tt], deg);
  };
#pragma unroll
  for (int i = 0; i < 2; ++i)
    if (tid + 1024 * i < N) row(tid + 1024 * i, rr[i], tr[i]);
  for (int d = tid + 2048; d < N; d += 1024) {
    unsigned long long v[KP_W];
#pragma unroll
    for (int w = 0; w < KP_W; ++w) v[w] = a.R[(int64_t)d * KP_W + w];
    row(d, v, T == 1 ? 0 : a.types[(int64_t)d * a.ts]);
  }
  __syncthreads();
  KP_CLK(3);
  int base = 0;
  for (int u = 0; u < t; ++u) base += tot[u];
  const int d0 = blockIdx.y * KP_CH, d1 = min(N, d0 + KP_CH);   // this block's rows (placement, seg)
  {                                                  // exclusive scan of cs in place (SPT counts per thread)
    int v[SPT], local = 0;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      const int d = tid * SPT + j;
      v[j] = d < N ? cs[d] : 0;
      local += v[j];
    }
    int x = local;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(x, o);
      if (lane >= o) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    int run = base + x - local;
    for (int w2 = 0; w2 < wave; ++w2) run += wsum[w2];
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      const int d = tid * SPT + j;
      if (d < N) cs[d] = run;
      if (d >= d0 && d < d1) a.seg[(int64_t)t * N + d] = run;
      run += v[j];
    }
    if (tid == 1023) cend = run;                     // the end of type t's segments
  }
  __syncthreads();
  KP_CLK(4);
  // placement: the type-t sources x of row d in ascending order; the (x -> d) id = the image's base + row x's
  // start + its entries before d (word prefix from LDS + one word of row x). The chunk's positions are contiguous
  // ([p0, p1)): each row lists its sources in LDS, then the list is placed entry-parallel (coalesced stores).
  const int p0 = d0 < d1 ? cs[d0] : 0, p1 = d1 < N ? cs[d1] : cend;
  if (p1 - p0 <= a.list_cap) {                       // (block-uniform)
    // row d is listed by the thread that loaded it (d = tid + 1024 i, rr[i])
    const int dr = (d0 & ~1023) + tid, ir = d0 >> 10;
    if (dr >= d0 && dr < d1) {
      const int b = kp_image(noff, B, dr), ob = noff[b], nb = noff[b + 1] - ob, wpr = (nb + 63) >> 6;
      int q = cs[dr] - p0;
#pragma unroll
      for (int w = 0; w < KP_W; ++w) {               // (static word indices: rr stays in registers)
        if (w >= wpr) break;
        unsigned long long r = ir == 0 ? rr[0][w] : ir == 1 ? rr[1][w] : a.R[(int64_t)dr * KP_W + w];
        r &= M[b * KP_W + w];
        while (r) {
          lst[q++] = (ob + 64 * w + __builtin_ctzll(r)) << 10 | (dr - d0);
          r &= r - 1ull;
        }
      }
    }
    __syncthreads();
    for (int i0 = 0; i0 < p1 - p0; i0 += 4096) {
      int xs[4], ds[4], rs[4];
      unsigned long long wd[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {                  // 4 entries per thread, all loads in flight together
        const int i = i0 + k * 1024 + tid;
        xs[k] = -1;
        if (i < p1 - p0) {
          const int v = lst[i];
          xs[k] = v >> 10;
          ds[k] = d0 + (v & 1023);
          const int b = kp_image(noff, B, ds[k]);
          wd[k] = a.R[(int64_t)xs[k] * KP_W + ((ds[k] - noff[b]) >> 6)];
          rs[k] = a.rowstart[xs[k]] + ebase[b];
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (xs[k] >= 0) {
          const int i = i0 + k * 1024 + tid;
          const int dl = ds[k] - noff[kp_image(noff, B, ds[k])];
          a.s_src[p0 + i] = xs[k];
          a.s_dst[p0 + i] = ds[k];
          a.s_orig[p0 + i] = rs[k] + pw[xs[k]][dl >> 6] + __popcll(wd[k] & ((1ull << (dl & 63)) - 1ull));
        }
      }
    }
  } else if (d0 + tid < d1) {                        // row by row, 8 sources at a time
    const int d = d0 + tid;
    const int b = kp_image(noff, B, d), ob = noff[b], nb = noff[b + 1] - ob, wpr = (nb + 63) >> 6;
    const int dl = d - ob, dw = dl >> 6;
    const unsigned long long below = (1ull << (dl & 63)) - 1ull;
    const int eb = ebase[b];
    int pos = cs[d];
    unsigned long long rw[KP_W];
#pragma unroll
    for (int w = 0; w < KP_W; ++w) rw[w] = w < wpr ? a.R[(int64_t)d * KP_W + w] & M[b * KP_W + w] : 0ull;
    for (;;) {
      int xs[8], n = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {                  // the next (up to) 8 sources, from the bits alone
        xs[k] = -1;                                  // (static indices only: rw stays in registers)
        bool got = false;
#pragma unroll
        for (int w = 0; w < KP_W; ++w) {
          if (!got && rw[w] != 0ull) {
            xs[k] = ob + 64 * w + __builtin_ctzll(rw[w]);
            rw[w] &= rw[w] - 1ull;
            got = true;
          }
        }
        if (got) n = k + 1;
      }
      if (n == 0) break;
      unsigned long long wd[8];
      int rs[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {                  // all their loads in flight together
        wd[k] = xs[k] >= 0 ? a.R[(int64_t)xs[k] * KP_W + dw] : 0ull;
        rs[k] = xs[k] >= 0 ? a.rowstart[xs[k]] : 0;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (xs[k] >= 0) {
          a.s_src[pos + k] = xs[k];
          a.s_dst[pos + k] = d;
          a.s_orig[pos + k] = eb + rs[k] + pw[xs[k]][dw] + __popcll(wd[k] & below);
        }
      }
      pos += n;
      if (n < 8) break;
    }
  }
#if PEMP_KP_CLOCKS
  __syncthreads();
  KP_CLK(5);
  if (tid == 0 && (t == 0 || t == T - 1))
    printf("kp block %d,%d: start %lld init +%lld masks +%lld rows +%lld scan +%lld placed +%lld\n", t, blockIdx.y,
           clk[0], clk[1] - clk[0], clk[2] - clk[0], clk[3] - clk[0], clk[4] - clk[0], clk[5] - clk[0]);
#endif
  if (t != T - 1 || blockIdx.y != 0) return;         // (block-uniform) one block closes seg and the split
  if (tid == 0) {
    int acc = 0;
    for (int u = 0; u < T; ++u) { tst[u] = acc; acc += tot[u]; }
    tst[T] = acc;
    a.seg[(int64_t)T * N] = acc;
    a.err[0] = (bad_sh ? 2 : 0) | (acc != a.E || ebase[B] != a.E ? 4 : 0);
    a.err[1] = a.err[2] = a.err[3] = 0;
  }
  __syncthreads();
  type_split(tst, tst[T], T, a.G, gt, a.wg_start);
}

static int grid1d(int64_t total, int block, int cap = 65536) {
  int64_t g = (total + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace

int launch_prepare(const pemp_mpn_desc* desc, const int64_t* edge_index, const int64_t* node_types, int64_t N,
                   int64_t E, const MpnWs& ws, hipStream_t st) {
  const int T = desc->num_types;
  const int64_t tstride = desc->types_stride > 0 ? desc->types_stride : 1;   // node_types may be a strided view
  const int64_t K = (int64_t)T * N;
  ProfScope prof("mpn_prepare", st);
  hipLaunchKernelGGL(zero_words_kernel, dim3((unsigned)std::min<int64_t>((K + 64 + 255) / 256, 1024)), dim3(256), 0,
                     st, ws.err, K + 65);
  PEMP_LAUNCH_CHECK();
  if (E > 0) {
    hipLaunchKernelGGL(mpn_count_kernel, dim3(grid1d(E, 256)), dim3(256), 0, st, edge_index, node_types, tstride, N, E, T,
                       ws.cnt, ws.err);
    PEMP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(mpn_scan_kernel, dim3(1), dim3(1024), 0, st, ws.cnt, K, N, T, std::max(edge_cus(E), T), ws.seg,
                     ws.wg_start);
  PEMP_LAUNCH_CHECK();
  if (E > 0) {
    hipLaunchKernelGGL(mpn_scatter_kernel, dim3(grid1d(E, 256)), dim3(256), 0, st, edge_index, node_types, tstride, N, E, T,
                       ws.seg, ws.cnt, ws.perm);
    PEMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(mpn_segsort_kernel, dim3((unsigned)((K + 15) / 16)), dim3(256), 0, st, edge_index, E, K, ws.seg,
                       ws.perm, ws.s_src, ws.s_dst, ws.s_orig);
    PEMP_LAUNCH_CHECK();
  }
  return PEMP_OK;
}

int launch_prepare_sym(const pemp_mpn_desc* desc, const int64_t* edge_index, const int64_t* node_types,
                       int64_t N, int64_t E, const MpnWs& ws, hipStream_t st) {
  const int T = desc->num_types;
  const int64_t tstride = desc->types_stride > 0 ? desc->types_stride : 1;
  ProfScope prof("mpn_prepare_sym", st);
  int2* rows = reinterpret_cast<int2*>(ws.sym);
  int* flags = ws.sym + 2 * N;
  unsigned* packed = reinterpret_cast<unsigned*>(ws.perm);
  const unsigned g = (unsigned)((N + 3) / 4);                 // one wave per node
  hipLaunchKernelGGL(sym_rows_kernel, dim3(g), dim3(256), 0, st, edge_index, node_types, tstride, N, E, T, ws.cnt, rows,
                     packed, flags);
  PEMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(sym_scan_kernel, dim3((unsigned)T), dim3(1024), 0, st, ws.cnt, N, T, std::max(edge_cus(E), T), ws.seg,
                     ws.wg_start, flags, E, ws.err);
  PEMP_LAUNCH_CHECK();
  hipLaunchKernelGGL(sym_place_kernel, dim3(g), dim3(256), 0, st, N, T, ws.seg, rows, packed, ws.s_src, ws.s_dst,
                     ws.s_orig, ws.err);
  PEMP_LAUNCH_CHECK();
  return PEMP_OK;
}

int launch_prepare_fully(const FullyPrepArgs& a, int gx, hipStream_t st) {
  hipLaunchKernelGGL(fully_prepare_kernel, dim3((unsigned)gx, (unsigned)a.B), dim3(256), 0, st, a);
  PEMP_LAUNCH_CHECK();
  return PEMP_OK;
}

int launch_prepare_knn(const KnnPrepArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(knn_prepare_kernel, dim3((unsigned)a.T, (unsigned)((a.N + KP_CH - 1) / KP_CH)), dim3(1024), 0, st,
                     a);
  PEMP_LAUNCH_CHECK();
  return PEMP_OK;
}

}  // namespace pemp
