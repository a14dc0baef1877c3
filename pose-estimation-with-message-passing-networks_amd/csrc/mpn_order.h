// What the closed-form fully prepare shares with launch A of the paired prelude (device; no kernels): the edge passes'
// type split and the prepare's role. Included by mpn_order.hip (fully_prepare_kernel) and mpn.hip (prelude_a_kernel).
#pragma once
#include "mpn_internal.h"

namespace pemp {
namespace {

// Split G edge-pass workgroups (one per CU) over the types so that the largest share, in 16-edge tiles per
// workgroup, is as small as possible: L = the least tile load with sum_t ceil(tiles_t / L) <= G, then
// gt = ceil(tiles_t / L) (>= 1 per non-empty type; sum <= G, spare workgroups get no range). The kernel's time is
// its busiest CU's, so this, not proportional shares, is the balanced split. tstart[t] (LDS, t <= T) = first edge
// of type t; gt = LDS scratch [MAXT]. Wave 0 does the search (T <= MAXT < 64); block-wide (contains
// __syncthreads).
__device__ void type_split(const int* tstart, int64_t etot, int T, int G, int* gt, int* wg_start) {
  (void)etot;
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const int tiles = lane < T ? (tstart[lane + 1] - tstart[lane] + 15) / 16 : 0;
    int hi = tiles;
    for (int o = 32; o >= 1; o >>= 1) hi = max(hi, __shfl_xor(hi, o));
    int lo = 1;
    hi = max(hi, 1);
    while (lo < hi) {   // (uniform)
      const int mid = (lo + hi) >> 1;
      int need = tiles > 0 ? (tiles + mid - 1) / mid : 0;
      for (int o = 32; o >= 1; o >>= 1) need += __shfl_xor(need, o);
      if (need <= G) hi = mid;
      else lo = mid + 1;
    }
    const int share = tiles > 0 ? (tiles + lo - 1) / lo : 0;
    int incl = share;   // inclusive prefix over the types
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    if (lane < T) {
      gt[lane] = share;
      wg_start[lane + 1] = incl;
    }
    if (lane == 0) wg_start[0] = 0;
  }
  __syncthreads();
}

// ---- prepare for a fully-connected batch (pemp_mpn_forward_fully) -----------------------------
// For the graph constructor's fully graph (every ordered pair i != j of an image, edge id
// eoff_b + i (n_b - 1) + (j < i ? j : j - 1), ConstructGraph.py:376-381) the type-major order is
// known in closed form, so the four sorting kernels collapse into one: segment (t, d) holds the
// type-t nodes of d's image except d, in index order, and starts at
//   seg(t, d) = sum_{t' < t} E_t' + sum_{b' < b} n_{b',t} (n_b' - 1) + d_local n_{b,t} - #{type-t nodes before d}
// with E_t = sum_b n_{b,t} (n_b - 1). Identical arrays to launch_prepare's (tested bit for bit).
// the LDS of one fully_prepare workgroup
struct FullyPrepLds {
  long long et_sh[MAXT], cb_sh[MAXT];
  long long eoff_sh;
  int cnt_bt[FULLY_MAXB][MAXT];
  int tbase[MAXT + 1];        // sum_{t' < t} E_t' (fits int: E < 2^31)
  int noff[FULLY_MAXB + 1];
  int sorted[FULLY_MAXN], lty[FULLY_MAXN];
  int tstart_l[MAXT + 1], gt_sh[MAXT];
  int bad_sh;
};

// block (bx of gx, image by) over its LDS (the body of fully_prepare_kernel, and a role of prelude_a_kernel)
__device__ __forceinline__ void fully_prepare_role(const FullyPrepArgs& a, FullyPrepLds& s, int bx, int by, int gx) {
  auto& cnt_bt = s.cnt_bt;
  auto& et_sh = s.et_sh;
  auto& cb_sh = s.cb_sh;
  auto& tbase = s.tbase;
  auto& noff = s.noff;
  auto& sorted = s.sorted;
  auto& lty = s.lty;
  auto& tstart_l = s.tstart_l;
  auto& gt_sh = s.gt_sh;
  int& bad_sh = s.bad_sh;
  long long& eoff_sh = s.eoff_sh;
  const int b = by, T = a.T, B = a.B;
  const int64_t N = a.ne ? a.ne[0] : a.N;
  const bool empty = a.ne && a.ne[2];   // capacity overflow: node_off was not written
  for (int i = threadIdx.x; i <= B; i += 256) noff[i] = empty ? 0 : (int)a.node_off[i];
  for (int i = threadIdx.x; i < FULLY_MAXB * MAXT; i += 256) (&cnt_bt[0][0])[i] = 0;
  if (threadIdx.x == 0) bad_sh = 0;
  __syncthreads();
  // per-(image, type) node counts of the whole batch (every block: N is a few thousand at most); a thread's type
  // loads go out 8 at a time, ahead of the searches and the LDS counts that use them
  for (int64_t n0 = threadIdx.x; n0 < N; n0 += 256 * 8) {
    int64_t tv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t n = n0 + 256 * k;
      tv[k] = n < N ? a.types[n * a.ts] : 0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t n = n0 + 256 * k;
      if (n >= N) break;
      int lo = 0, hi = B - 1;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (noff[mid] <= n) lo = mid; else hi = mid - 1;
      }
      const int64_t t = T == 1 ? 0 : tv[k];          // one message MLP ignores the types, like mpn_count_kernel
      if (t >= 0 && t < T) atomicAdd(&cnt_bt[lo][t], 1);
      else bad_sh = 1;                               // skipped as a source, like mpn_count_kernel
    }
  }
  __syncthreads();
  if (threadIdx.x < T) {
    const int t = threadIdx.x;
    long long e = 0, cb = 0;
    for (int bb = 0; bb < B; ++bb) {
      const int nb = noff[bb + 1] - noff[bb];
      const long long v = (long long)cnt_bt[bb][t] * (nb > 0 ? nb - 1 : 0);
      if (bb < b) cb += v;
      e += v;
    }
    et_sh[t] = e;
    cb_sh[t] = cb;
  }
  const int ob = noff[b], nb = noff[b + 1] - noff[b];
  for (int i = threadIdx.x; i < nb; i += 256) {
    const int64_t t = T == 1 ? 0 : a.types[(int64_t)(ob + i) * a.ts];
    lty[i] = (t >= 0 && t < T) ? (int)t : -1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int t = 0; t < T; ++t) { tbase[t] = acc; acc += (int)et_sh[t]; }
    tbase[T] = acc;
    acc = 0;
    for (int t = 0; t < T; ++t) { tstart_l[t] = acc; acc += cnt_bt[b][t]; }
    tstart_l[T] = acc;
    long long eo = 0;
    for (int bb = 0; bb < b; ++bb) { const long long m = noff[bb + 1] - noff[bb]; eo += m * (m > 0 ? m - 1 : 0); }
    eoff_sh = eo;
  }
  __syncthreads();
  // the image's nodes grouped by type, index order kept (rank = same-type nodes before i)
  for (int i = threadIdx.x; i < nb; i += 256) {
    const int t = lty[i];
    if (t < 0) continue;
    int r = 0;
    for (int j = 0; j < i; ++j) r += lty[j] == t;
    sorted[tstart_l[t] + r] = i;
  }
  __syncthreads();
  // segments (t, d): one thread each
  const long long eoff = eoff_sh;
  // FULLY_PARTS consecutive threads per segment, entry m of the segment on thread (m - s0) % FULLY_PARTS: its slot is
  // the segment start + its rank, one less past d when d itself is of type t (d is left out)
  for (int q = bx * 256 + threadIdx.x; q < T * nb * FULLY_PARTS; q += gx * 256) {
    const int sq = q / FULLY_PARTS, part = q - sq * FULLY_PARTS;
    const int t = sq / nb, dl = sq - t * nb;
    const int s0 = tstart_l[t], s1 = tstart_l[t + 1];
    int lo = s0, hi = s1;                              // type-t nodes before dl
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (sorted[mid] < dl) lo = mid + 1; else hi = mid;
    }
    const int before = lo - s0;
    const int64_t d = ob + dl;
    const int pos = tbase[t] + (int)cb_sh[t] + dl * (s1 - s0) - before;
    const bool d_in = lty[dl] == t;
    if (part == 0) a.seg[(int64_t)t * N + d] = pos;
    for (int m = s0 + part; m < s1; m += FULLY_PARTS) {   // the segment: type-t nodes except d, in order
      const int i = sorted[m];
      if (i == dl) continue;
      const int p = pos + (m - s0) - (d_in && i > dl ? 1 : 0);
      a.s_src[p] = ob + i;
      a.s_dst[p] = (int)d;
      a.s_orig[p] = (int)(eoff + (long long)i * (nb - 1) + (dl < i ? dl : dl - 1));
    }
  }
  if (bx == 0 && by == 0) {
    if (threadIdx.x == 0) {
      a.seg[(int64_t)T * N] = tbase[T];
      a.err[0] = bad_sh ? 2 : 0;
      a.err[1] = a.err[2] = a.err[3] = 0;
    }
    type_split(tbase, tbase[T], T, a.Gsplit, gt_sh, a.wg_start);
  }
}

}  // namespace
}  // namespace pemp
