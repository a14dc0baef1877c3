// Training labels for EDGE_LABEL_METHOD 4 and 6 (the label half) — restates:
//   ConstructGraph.py:627-646, 769-785   the [G, N] similarity of the visible ground-truth joints and the
//                                        detections: sim = exp(-d2 / factor), d2 from the rounded, clamped
//                                        ground-truth position (pemp_label_candidates, device)
//   ConstructGraph.py:646-694, 807-942   the two assignments, the neighbour fill and the per-node labels
//                                        (pemp_label_assign, host: label_assign.h)
//   ConstructGraph.py:1096-1158, 145-146 match_cc, create_loss_mask and the per-image "no positive edge" rule
//                                        (pemp_label_edges, device)
// The dense matrix stays on the device: only the pairs at or above the smaller radius leave it, in (g, n) order.
#include <math.h>

#include <vector>

#include "label_assign.h"
#include "pemp_common.h"

using namespace pemp;

namespace {

constexpr int CAND_THREADS = 1024;
constexpr int CAND_WAVES = CAND_THREADS / 64;

__device__ __forceinline__ float sim_of(float d2, float f) { return expf(div_rn(-d2, f)); }
__device__ __forceinline__ double sim_of(float d2, double f) { return exp(-(double)d2 / f); }

// inclusive scan over the 64 lanes
__device__ __forceinline__ int wave_scan_incl(int v) {
  const int lane = lane_id();
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(v, off);
    if (lane >= off) v += o;
  }
  return v;
}

// One workgroup per image. Phase A lists the visible ground-truth joints in (person, joint) order; phase B counts
// each row's pairs at or above thr (one wave per row, 64 detections per step); a scan of the row counts gives every
// row its place; phase C recomputes the row and stores its pairs there. The list is therefore in (g, n) order
// whatever the scheduling. An image that needs more than cap records stores none and raises hdr[2 B].
template <typename T>
__global__ __launch_bounds__(CAND_THREADS) void label_cand_kernel(
    const float* __restrict__ joints_gt, const T* __restrict__ factors, int B, int PJ, int J,
    const int64_t* __restrict__ joint_det, const int64_t* __restrict__ node_off, float clamp_max, T thr, int64_t cap,
    pemp_label_cand* __restrict__ recs, int32_t* __restrict__ hdr, int32_t* __restrict__ gt_tab,
    int32_t* __restrict__ row_off) {
  __shared__ int s_wc[CAND_WAVES];
  __shared__ int s_total;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* gt = joints_gt + (size_t)b * PJ * 3;
  const T* fac = factors + (size_t)b * PJ;
  int32_t* tab = gt_tab + (size_t)b * PJ;
  int32_t* roff = row_off + (size_t)b * (PJ + 1);
  const int64_t n0 = node_off[b];
  const int N = (int)(node_off[b + 1] - n0);
  const int64_t* det = joint_det + n0 * 3;

  // ---- A: visible joints, in order ----
  int G = 0;
  for (int i0 = 0; i0 < PJ; i0 += CAND_THREADS) {
    const int i = i0 + tid;
    const bool vis = i < PJ && gt[(size_t)i * 3 + 2] != 0.f;
    const uint64_t m = __ballot(vis);
    if (lane == 0) s_wc[wave] = __popcll(m);
    __syncthreads();
    int off = G, tot = 0;
#pragma unroll
    for (int w = 0; w < CAND_WAVES; ++w) {
      if (w < wave) off += s_wc[w];
      tot += s_wc[w];
    }
    if (vis) tab[off + __popcll(m & ((1ull << lane) - 1))] = i;
    G += tot;
    __syncthreads();
  }
  __syncthreads();   // tab[0, G) is visible to the whole workgroup

  // ---- B / C: one wave per row ----
  for (int pass = 0; pass < 2; ++pass) {
    for (int g = wave; g < G; g += CAND_WAVES) {
      const int i = tab[g];
      const float gx = fminf(fmaxf(rintf(gt[(size_t)i * 3]), 0.f), clamp_max);
      const float gy = fminf(fmaxf(rintf(gt[(size_t)i * 3 + 1]), 0.f), clamp_max);
      const T f = fac[i];
      const int jt = i % J;
      int pos = pass ? roff[g] : 0;
      for (int nb = 0; nb < N; nb += 64) {
        const int n = nb + lane;
        bool keep = false;
        T sim = 0;
        bool same = false;
        if (n < N) {
          const float dx = gx - (float)det[(size_t)n * 3], dy = gy - (float)det[(size_t)n * 3 + 1];
          sim = sim_of(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), f);
          same = det[(size_t)n * 3 + 2] == jt;
          keep = sim >= thr;
        }
        const uint64_t m = __ballot(keep);
        if (pass && keep) {
          pemp_label_cand r;
          r.g = g;
          r.n = (uint32_t)n | (same ? 0x80000000u : 0u);
          r.sim = (double)sim;
          recs[(size_t)b * cap + pos + __popcll(m & ((1ull << lane) - 1))] = r;
        }
        pos += __popcll(m);
      }
      if (!pass && lane == 0) roff[g] = pos;
    }
    if (pass) break;
    __syncthreads();
    // exclusive scan of the row counts by wave 0
    if (wave == 0) {
      int run = 0;
      for (int g0 = 0; g0 < G; g0 += 64) {
        const int g = g0 + lane;
        const int c = g < G ? roff[g] : 0;
        const int inc = wave_scan_incl(c);
        if (g < G) roff[g] = run + inc - c;
        run += __shfl(inc, 63);
      }
      if (lane == 0) {
        s_total = run;
        hdr[b] = run;
        hdr[B + b] = G;
        if (run > cap) atomicOr(&hdr[2 * B], 1);
      }
    }
    __syncthreads();
    if (s_total > cap) return;   // (uniform) the caller retries with hdr[b] records
  }
}

// ---- edge pass ----
// image of a node: the last b with node_off[b] <= node (node_off [B + 1] is cache resident). The batched edge list
// never joins two images, so an edge's image is its source's.
__device__ __forceinline__ int node_image(const int64_t* __restrict__ node_off, int B, int64_t node) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (node_off[mid] <= node) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Which images have a positive edge: every workgroup of the main kernel keeps a bit per image in LDS (a wave inside
// one image -- nearly all are -- votes and lane 0 alone sets the bit) and stores its words into a slot of its own;
// the second kernel ORs the slots. No global atomics and no shared global word: an earlier form, in which the waves
// set one global flag per image, spent most of its time queueing on that cache line.
constexpr int EDGE_MAX_BLOCKS = 1024;   // workgroups of the main kernel (grid stride beyond)
constexpr int EDGE_MAX_WORDS = 64;      // 64 images per word: B <= 4096

__device__ __forceinline__ void raise_flags(bool active, bool pos, int img, unsigned long long* s_flags) {
  const uint64_t act = __ballot(active);
  if (!act) return;
  const int first = __shfl(img, __ffsll((unsigned long long)act) - 1);
  const bool uniform = __all(!active || img == first);
  if (uniform) {
    if (__ballot(active && pos) && lane_id() == 0) atomicOr(&s_flags[first >> 6], 1ull << (first & 63));
  } else if (active && pos) {
    atomicOr(&s_flags[img >> 6], 1ull << (img & 63));
  }
}

// two edges per lane (16-byte loads of both rows when they are 16-byte aligned), the labels and mask as 8-byte
// stores; nodes are read from the small per-node arrays (cache resident)
template <bool VEC>
__global__ __launch_bounds__(256) void label_edges_kernel(const int64_t* __restrict__ src,
                                                          const int64_t* __restrict__ dst, int64_t E, int64_t N,
                                                          const int64_t* __restrict__ persons,
                                                          const uint8_t* __restrict__ amb,
                                                          const int64_t* __restrict__ node_off, int B, int words,
                                                          float* __restrict__ labels, float* __restrict__ mask,
                                                          unsigned long long* __restrict__ block_flags) {
  __shared__ unsigned long long s_flags[EDGE_MAX_WORDS];
  for (int w = threadIdx.x; w < words; w += blockDim.x) s_flags[w] = 0;
  __syncthreads();
  const int64_t pairs = (E + 1) / 2;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < (pairs + 63) / 64 * 64;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e0 = 2 * t;
    const bool a0 = e0 < E, a1 = e0 + 1 < E;
    int64_t s[2] = {0, 0}, d[2] = {0, 0};
    if (VEC && a1) {
      const longlong2 sv = *reinterpret_cast<const longlong2*>(src + e0);
      const longlong2 dv = *reinterpret_cast<const longlong2*>(dst + e0);
      s[0] = sv.x, s[1] = sv.y, d[0] = dv.x, d[1] = dv.y;
    } else {
      if (a0) s[0] = src[e0], d[0] = dst[e0];
      if (a1) s[1] = src[e0 + 1], d[1] = dst[e0 + 1];
    }
    float lab[2] = {0.f, 0.f}, msk[2] = {1.f, 1.f};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const bool act = k ? a1 : a0;
      const bool ok = act && (uint64_t)s[k] < (uint64_t)N && (uint64_t)d[k] < (uint64_t)N;   // (a stray index: 0)
      int img = 0;
      if (ok) {
        const int64_t ps = persons[s[k]], pd = persons[d[k]];
        lab[k] = (ps >= 0 && ps == pd) ? 1.f : 0.f;
        msk[k] = (amb[s[k]] | amb[d[k]]) ? 0.f : 1.f;
        if (lab[k] == 1.f) img = node_image(node_off, B, s[k]);
      }
      raise_flags(ok && lab[k] == 1.f, true, img, s_flags);
    }
    if (a1 && VEC) {
      *reinterpret_cast<float2*>(labels + e0) = make_float2(lab[0], lab[1]);
      *reinterpret_cast<float2*>(mask + e0) = make_float2(msk[0], msk[1]);
    } else {
      if (a0) labels[e0] = lab[0], mask[e0] = msk[0];
      if (a1) labels[e0 + 1] = lab[1], mask[e0 + 1] = msk[1];
    }
  }
  __syncthreads();
  for (int w = threadIdx.x; w < words; w += blockDim.x) block_flags[(size_t)blockIdx.x * words + w] = s_flags[w];
}

// second touch: the mask of an image without a positive edge is zero (ConstructGraph.py:145-146). Every workgroup
// ORs the main kernel's slots; a batch whose images all have a positive edge leaves at once, otherwise the sources
// are read again and the edges of the images without one are cleared.
__global__ __launch_bounds__(256) void label_mask_fix_kernel(const int64_t* __restrict__ src, int64_t E, int64_t N,
                                                             const int64_t* __restrict__ node_off, int B, int words,
                                                             const unsigned long long* __restrict__ block_flags,
                                                             int nblocks, float* __restrict__ mask) {
  __shared__ unsigned long long s_flags[EDGE_MAX_WORDS];
  __shared__ int s_any;
  for (int w = threadIdx.x; w < words; w += blockDim.x) s_flags[w] = 0;
  if (threadIdx.x == 0) s_any = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < nblocks * words; i += blockDim.x) {
    const unsigned long long v = block_flags[i];
    if (v) atomicOr(&s_flags[i % words], v);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < B; b += blockDim.x)
    if (!((s_flags[b >> 6] >> (b & 63)) & 1) && node_off[b + 1] > node_off[b]) s_any = 1;
  __syncthreads();
  if (!s_any) return;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = src[e];
    if ((uint64_t)s >= (uint64_t)N) continue;
    const int b = node_image(node_off, B, s);
    if (!((s_flags[b >> 6] >> (b & 63)) & 1)) mask[e] = 0.f;
  }
}

}  // namespace

extern "C" size_t pemp_label_candidates_scratch_size(int B, int P, int J) {
  if (B <= 0 || P <= 0 || J <= 0) return 0;
  return align_up(sizeof(int32_t) * (size_t)B * ((size_t)P * J + 1), 256);
}

extern "C" int pemp_label_candidates(const float* joints_gt, const void* factors, int factors_f64, int B, int P, int J,
                                     const int64_t* joint_det, const int64_t* node_off, int H, int W, double threshold,
                                     int64_t cap, pemp_label_cand* recs, int32_t* hdr, int32_t* gt_tab, void* scratch,
                                     size_t scratch_bytes, void* stream) {
  PEMP_CHECK_ARG(B > 0 && P > 0 && J > 0 && H > 0 && W > 0 && cap >= 0 && (int64_t)P * J < (1 << 24),
                 "pemp_label_candidates: bad sizes B=%d P=%d J=%d H=%d W=%d cap=%lld", B, P, J, H, W, (long long)cap);
  PEMP_CHECK_ARG(joints_gt && factors && node_off && hdr && gt_tab && scratch && (recs || cap == 0),
                 "pemp_label_candidates: null pointer");
  PEMP_CHECK_ARG(cap < (int64_t(1) << 31), "pemp_label_candidates: cap %lld too large", (long long)cap);
  if (scratch_bytes < pemp_label_candidates_scratch_size(B, P, J)) {
    set_error("pemp_label_candidates: scratch %zu < %zu bytes", scratch_bytes,
              pemp_label_candidates_scratch_size(B, P, J));
    return PEMP_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  PEMP_HIP(hipMemsetAsync(hdr + 2 * B, 0, sizeof(int32_t), st));
  ProfScope prof("label_candidates", st);
  const float cm = (float)std::max(H, W);
  if (factors_f64)
    hipLaunchKernelGGL(label_cand_kernel<double>, dim3(B), dim3(CAND_THREADS), 0, st, joints_gt,
                       static_cast<const double*>(factors), B, P * J, J, joint_det, node_off, cm, threshold, cap, recs,
                       hdr, gt_tab, static_cast<int32_t*>(scratch));
  else
    hipLaunchKernelGGL(label_cand_kernel<float>, dim3(B), dim3(CAND_THREADS), 0, st, joints_gt,
                       static_cast<const float*>(factors), B, P * J, J, joint_det, node_off, cm, (float)threshold, cap,
                       recs, hdr, gt_tab, static_cast<int32_t*>(scratch));
  PEMP_LAUNCH_CHECK();
  return PEMP_OK;
}

extern "C" int pemp_label_assign(int B, int P, int J, const int32_t* hdr, const int32_t* gt_tab,
                                 const pemp_label_cand* recs, int64_t cap, const int64_t* node_off_host, int method,
                                 int use_neighbours, int with_background, double matching_radius,
                                 double inclusion_radius, float* node_labels, int64_t* node_persons,
                                 int64_t* node_classes, float* label_mask_node, float* class_mask,
                                 uint8_t* ambiguous) {
  PEMP_CHECK_ARG(B > 0 && P > 0 && J > 0 && cap >= 0, "pemp_label_assign: bad sizes B=%d P=%d J=%d", B, P, J);
  PEMP_CHECK_ARG(hdr && gt_tab && node_off_host && (recs || cap == 0), "pemp_label_assign: null pointer");
  if (method != 4 && method != 6) {
    set_error("pemp_label_assign: EDGE_LABEL_METHOD %d (4 and 6 are built)", method);
    return PEMP_ERR_UNSUPPORTED;
  }
  const int64_t N = node_off_host[B];
  PEMP_CHECK_ARG(N == 0 || (node_labels && node_persons && label_mask_node && ambiguous &&
                            (method == 4 || (node_classes && class_mask))),
                 "pemp_label_assign: null output");
  if (hdr[2 * B]) return PEMP_LABEL_OVERFLOW;
  const labels::Params p{method, use_neighbours, with_background, matching_radius, inclusion_radius, J};
  for (int b = 0; b < B; ++b) {
    const int64_t o = node_off_host[b], n = node_off_host[b + 1] - o;
    PEMP_CHECK_ARG(o >= 0 && n >= 0 && n < (int64_t(1) << 31), "pemp_label_assign: node_off_host not ascending");
    PEMP_CHECK_ARG(hdr[b] >= 0 && hdr[b] <= cap && hdr[B + b] >= 0 && hdr[B + b] <= P * J,
                   "pemp_label_assign: image %d header (%d records, %d joints) out of range", b, hdr[b], hdr[B + b]);
    for (int g = 0; g < hdr[B + b]; ++g)
      PEMP_CHECK_ARG(gt_tab[(size_t)b * P * J + g] >= 0 && gt_tab[(size_t)b * P * J + g] < P * J,
                     "pemp_label_assign: image %d joint table entry %d out of range", b, g);
    const bool ok = labels::assign_image(
        recs + (size_t)b * cap, hdr[b], gt_tab + (size_t)b * P * J, hdr[B + b], (int)n, p, node_labels + o,
        node_persons + o, node_classes ? node_classes + o : nullptr, label_mask_node + o,
        class_mask ? class_mask + o : nullptr, ambiguous + o);
    PEMP_CHECK_ARG(ok, "pemp_label_assign: image %d has a record outside its %d x %lld matrix", b, hdr[B + b],
                   (long long)n);
  }
  return PEMP_OK;
}

extern "C" size_t pemp_label_edges_scratch_size(int B) {
  return B <= 0 ? 0 : align_up(sizeof(uint64_t) * (size_t)EDGE_MAX_BLOCKS * (((size_t)B + 63) / 64), 256);
}

extern "C" int pemp_label_edges(const int64_t* edge_index, int64_t E, const int64_t* node_off, int B, int64_t N,
                                const int64_t* node_persons, const uint8_t* ambiguous, float* edge_labels,
                                float* label_mask, void* scratch, size_t scratch_bytes, void* stream) {
  PEMP_CHECK_ARG(B > 0 && E >= 0 && N >= 0, "pemp_label_edges: bad sizes B=%d E=%lld N=%lld", B, (long long)E,
                 (long long)N);
  if (B > 64 * EDGE_MAX_WORDS) {
    set_error("pemp_label_edges: B=%d images (at most %d)", B, 64 * EDGE_MAX_WORDS);
    return PEMP_ERR_UNSUPPORTED;
  }
  if (E == 0) return PEMP_OK;
  PEMP_CHECK_ARG(edge_index && node_off && node_persons && ambiguous && edge_labels && label_mask && scratch,
                 "pemp_label_edges: null pointer");
  if (scratch_bytes < pemp_label_edges_scratch_size(B)) {
    set_error("pemp_label_edges: scratch %zu < %zu bytes", scratch_bytes, pemp_label_edges_scratch_size(B));
    return PEMP_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  unsigned long long* block_flags = static_cast<unsigned long long*>(scratch);
  const int words = (B + 63) / 64;
  const int64_t* src = edge_index;
  const int64_t* dst = edge_index + E;
  ProfScope prof("label_edges", st);
  const int64_t pairs = (E + 1) / 2;
  const int blocks = (int)std::min<int64_t>((pairs + 255) / 256, EDGE_MAX_BLOCKS);
  const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0 &&
                   ((reinterpret_cast<uintptr_t>(edge_labels) | reinterpret_cast<uintptr_t>(label_mask)) & 7) == 0;
  if (vec)
    hipLaunchKernelGGL(label_edges_kernel<true>, dim3(blocks), dim3(256), 0, st, src, dst, E, N, node_persons,
                       ambiguous, node_off, B, words, edge_labels, label_mask, block_flags);
  else
    hipLaunchKernelGGL(label_edges_kernel<false>, dim3(blocks), dim3(256), 0, st, src, dst, E, N, node_persons,
                       ambiguous, node_off, B, words, edge_labels, label_mask, block_flags);
  PEMP_LAUNCH_CHECK();
  const unsigned fblocks = (unsigned)std::min<int64_t>((E + 255) / 256, (int64_t)num_cus() * 2);
  hipLaunchKernelGGL(label_mask_fix_kernel, dim3(fblocks), dim3(256), 0, st, src, E, N, node_off, B, words,
                     block_flags, blocks, label_mask);
  PEMP_LAUNCH_CHECK();
  return PEMP_OK;
}
