// The MPN training loss (pemp_amd/loss.py): the node, edge and class terms of the reference's ClassMPNLossFactory /
// ClassMultiLossFactory (Utils/loss.py:606-621, 668-689, 785-862) with the graph reduction of train.py:104-112,
// 140-154, fused each way.
//
// Forward: one pass over the [K_e, E] edge logits and the [K_n, N] node rows, then a one-block reduction.
//   Edge blocks take chunks of kChunk consecutive edges; a thread takes four consecutive edges (16-byte loads when
//   every row is 16-byte aligned) and walks all K_e predictions for them, so the edge's ends, label and mask are
//   read once. The per-prediction mask mask_k = label_mask * (sel_k[src] op sel_k[dst]) is formed on the fly from
//   the node logits (or read from the caller's edge_mask[k]). Node blocks take (prediction, 256 nodes): one node per
//   lane, the class row's log-softmax over J <= 32 in registers.
//   Sums: fp32 inside a thread's at most 8 elements of a chunk and through the wave (pemp_common.h's in-VALU lane
//   sums), fp64 from there on: per wave across chunks, across the block's four waves, and in the reduction. Every
//   block stores its partials into a slot of its own and the reduction adds the slots in a fixed order: no atomics,
//   bitwise reproducible, and the order depends on (N, E, K) alone, never on the device.
// Backward: one elementwise pass of the same shape that recomputes dF/dx from the logits and multiplies by the
//   per-prediction scale the reduction left in `out` and by the device scalar grad_total.
#include <limits.h>
#include <math.h>

#include "pemp_common.h"

namespace pemp {
namespace {

constexpr int kBlock = 256;
constexpr int kChunk = PEMP_LOSS_CHUNK;     // edges per edge-block iteration: 2 x 256 threads x 4
constexpr int kMaxEdgeBlocks = 1024;        // memory-bound cap (Guideline 11); the rest is grid-strided
constexpr int kMaxNodeBlocks = 64;          // per prediction
constexpr int kNodeSlots = 3;               // per node block: sum F, sum mask, sum CE * label
// out[] layout (floats): 0..3 node, edge, class, total; 4 the class scale; 8 + k the edge scales; 16 + k the node ones
constexpr int kOutClassScale = 4, kOutEdgeScale = 8, kOutNodeScale = 16;

struct Grid {
  int nbe;   // edge blocks
  int bpn;   // node blocks per prediction
  int nbn;   // node blocks
};

Grid grid_for(int64_t N, int64_t E, int K_n) {
  Grid g;
  const int64_t chunks = (E + kChunk - 1) / kChunk;
  g.nbe = (int)(chunks < kMaxEdgeBlocks ? chunks : kMaxEdgeBlocks);
  const int64_t nb = (N + kBlock - 1) / kBlock;
  g.bpn = (int)(nb < kMaxNodeBlocks ? nb : kMaxNodeBlocks);
  g.nbn = g.bpn * K_n;
  return g;
}

// (1 - pt)^gamma off the multiply form; kept out of line: 32 inlined copies of powf would be most of the kernel
__device__ __noinline__ float pow_gamma(float q, float gamma) { return powf(q, gamma); }

struct Elem {
  int kind;       // PEMP_LOSS_FOCAL / PEMP_LOSS_BCE
  int g2;         // gamma == 2: the multiply form
  float alpha, gamma, pos_weight;
};

// binary_cross_entropy_with_logits(x, t) = max(x, 0) - x t + log1p(exp(-|x|)); *e = exp(-|x|)
__device__ __forceinline__ float bce_logits(float x, float t, float* e) {
  *e = expf(-fabsf(x));
  return fmaxf(x, 0.f) - x * t + log1pf(*e);
}

// FocalLoss.forward's F (Utils/loss.py:875-881) or BCELossWtihLogits' element (:900-904)
__device__ __forceinline__ float elem_fwd(const Elem& c, float x, float t, float m) {
  float e;
  const float bce = bce_logits(x, t, &e);
  if (c.kind == PEMP_LOSS_BCE) {
    const float v = bce * m;
    return t == 1.0f ? v * c.pos_weight : v;
  }
  const float q = -expm1f(-bce);                               // 1 - pt without the cancellation
  const float p = c.g2 ? q * q : pow_gamma(q, c.gamma);
  return c.alpha * p * bce * m;
}

// dF/dx of the same element
__device__ __forceinline__ float elem_bwd(const Elem& c, float x, float t, float m) {
  float e;
  const float bce = bce_logits(x, t, &e);
  const float r = e / (1.f + e);                               // sigmoid(-|x|)
  const float d = x >= 0.f ? (1.f - t) - r : r - t;            // sigmoid(x) - t
  if (c.kind == PEMP_LOSS_BCE) {
    const float v = d * m;
    return t == 1.0f ? v * c.pos_weight : v;
  }
  const float q = -expm1f(-bce);
  const float pt = expf(-bce);
  float w;
  if (c.g2)
    w = q * (q + 2.f * pt * bce);
  else      // torch's pow backward: exponent 0 gives 0, else gamma q^(gamma - 1) (inf at q = 0 for gamma < 1)
    w = pow_gamma(q, c.gamma) + (c.gamma == 0.f ? 0.f : c.gamma * pow_gamma(q, c.gamma - 1.f) * pt * bce);
  return c.alpha * w * d * m;
}

__device__ __forceinline__ bool selected(float x, float label, float th) {
  const float e = expf(-fabsf(x));
  const float s = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
  return s > th || label == 1.0f;
}

// Four consecutive edges of a thread: labels, label masks and, without caller masks, the ends' node labels.
struct Quad {
  float t[4], lm[4], ls[4], ld[4];
  int32_t s[4], d[4];     // node ids, -1 when outside [0, N)
  int n;                  // valid edges (0..4)
};

template <bool VEC>
__device__ __forceinline__ void load4(const float* p, int64_t e0, int n, float* v) {
  if (VEC && n == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p + e0);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = i < n ? p[e0 + i] : 0.f;
  }
}

template <bool VEC>
__device__ __forceinline__ void store4(float* p, int64_t e0, int n, const float* v) {
  if (VEC && n == 4) {
    *reinterpret_cast<float4*>(p + e0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < n) p[e0 + i] = v[i];
  }
}

template <bool VEC>
__device__ __forceinline__ void load_quad(const pemp_loss_rec& r, bool own_mask, int64_t e0, Quad* q) {
  const int64_t left = r.E - e0;
  q->n = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
  load4<VEC>(r.edge_labels, e0, q->n, q->t);
  load4<VEC>(r.label_mask, e0, q->n, q->lm);
  if (!own_mask) return;
  int64_t s[4], d[4];
  if (VEC && q->n == 4) {
    const longlong2 a = *reinterpret_cast<const longlong2*>(r.edge_index + e0);
    const longlong2 b = *reinterpret_cast<const longlong2*>(r.edge_index + e0 + 2);
    const longlong2 c = *reinterpret_cast<const longlong2*>(r.edge_index + r.E + e0);
    const longlong2 f = *reinterpret_cast<const longlong2*>(r.edge_index + r.E + e0 + 2);
    s[0] = a.x, s[1] = a.y, s[2] = b.x, s[3] = b.y;
    d[0] = c.x, d[1] = c.y, d[2] = f.x, d[3] = f.y;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s[i] = i < q->n ? r.edge_index[e0 + i] : -1;
      d[i] = i < q->n ? r.edge_index[r.E + e0 + i] : -1;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {       // an id outside [0, N) is never followed: its end counts as not selected
    q->s[i] = (s[i] >= 0 && s[i] < r.N) ? (int32_t)s[i] : -1;
    q->d[i] = (d[i] >= 0 && d[i] < r.N) ? (int32_t)d[i] : -1;
    q->ls[i] = q->s[i] >= 0 ? r.node_labels[q->s[i]] : 0.f;
    q->ld[i] = q->d[i] >= 0 ? r.node_labels[q->d[i]] : 0.f;
  }
}

// mask_k of the quad: the caller's, or label_mask * (sel_k[src] op sel_k[dst]) from node prediction k
template <bool VEC>
__device__ __forceinline__ void quad_mask(const pemp_loss_rec& r, bool own_mask, int k, int64_t e0, const Quad& q,
                                          float* m) {
  if (!own_mask) {
    load4<VEC>(r.edge_mask[k], e0, q.n, m);
    return;
  }
  const float* pn = r.pn[k];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bool a = q.s[i] >= 0 && selected(pn[q.s[i]], q.ls[i], r.node_threshold);
    const bool b = q.d[i] >= 0 && selected(pn[q.d[i]], q.ld[i], r.node_threshold);
    const bool on = r.include_bordering ? (a || b) : (a && b);
    m[i] = i < q.n ? q.lm[i] * (on ? 1.f : 0.f) : 0.f;
  }
}

__device__ __forceinline__ Elem edge_elem(const pemp_loss_rec& r) {
  return Elem{r.edge_kind, r.gamma == 2.0f, r.alpha, r.gamma, r.edge_pos_weight};
}
__device__ __forceinline__ Elem node_elem(const pemp_loss_rec& r) {
  return Elem{r.node_kind, r.gamma == 2.0f, r.alpha, r.gamma, r.node_pos_weight};
}

// log-softmax of the J <= 32 class logits of one node, in registers: v[j] = x[j] - max (exact for the entries near
// the maximum, the ones that matter), sum = sum_j exp(v[j]) and v of class `cls` (NaN when cls lies outside [0, J):
// nothing is indexed by it). log_softmax[j] = v[j] - log(sum), torch's own form.
__device__ __forceinline__ void class_row(const float* row, int J, int64_t cls, float* v, float* sum_out, float* picked) {
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < PEMP_LOSS_MAXJ; ++j) {
    v[j] = j < J ? row[j] : -INFINITY;
    mx = fmaxf(mx, v[j]);
  }
  float sum = 0.f, pk = NAN;
#pragma unroll
  for (int j = 0; j < PEMP_LOSS_MAXJ; ++j) {
    v[j] -= mx;
    if (j < J) sum += expf(v[j]);
    if ((int64_t)j == cls && j < J) pk = v[j];
  }
  *sum_out = sum;
  *picked = pk;
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void loss_fwd_kernel(pemp_loss_rec r, int nbe, int bpn, double* __restrict__ epart,
                                                          double* __restrict__ npart) {
  __shared__ double sh[4][2 * PEMP_LOSS_MAXKE];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x;
  if (b < nbe) {                                         // ---- edge block
    const bool own_mask = r.edge_mask[0] == nullptr;
    const Elem ce = edge_elem(r);
    double accF[PEMP_LOSS_MAXKE], accM[PEMP_LOSS_MAXKE];
#pragma unroll
    for (int k = 0; k < PEMP_LOSS_MAXKE; ++k) accF[k] = accM[k] = 0.0;
    const int64_t chunks = (r.E + kChunk - 1) / kChunk;
    for (int64_t c = b; c < chunks; c += nbe) {
      float f[PEMP_LOSS_MAXKE], ms[PEMP_LOSS_MAXKE];
#pragma unroll
      for (int k = 0; k < PEMP_LOSS_MAXKE; ++k) f[k] = ms[k] = 0.f;
      for (int it = 0; it < kChunk / (4 * kBlock); ++it) {
        const int64_t e0 = c * kChunk + ((int64_t)it * kBlock + tid) * 4;
        if (e0 >= r.E) continue;
        Quad q;
        load_quad<VEC>(r, own_mask, e0, &q);
#pragma unroll
        for (int k = 0; k < PEMP_LOSS_MAXKE; ++k) {
          if (k < r.K_e) {
            float x[4], m[4];
            load4<VEC>(r.pe[k], e0, q.n, x);
            quad_mask<VEC>(r, own_mask, k, e0, q, m);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              if (i < q.n) {
                f[k] += elem_fwd(ce, x[i], q.t[i], m[i]);
                ms[k] += m[i];
              }
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < PEMP_LOSS_MAXKE; ++k) {
        if (k < r.K_e) {
          accF[k] += (double)wave_sum_f32(f[k]);
          accM[k] += (double)wave_sum_f32(ms[k]);
        }
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < PEMP_LOSS_MAXKE; ++k) sh[wave][2 * k] = accF[k], sh[wave][2 * k + 1] = accM[k];
    }
    __syncthreads();
    if (tid < 2 * r.K_e) epart[(size_t)b * 2 * r.K_e + tid] = (sh[0][tid] + sh[1][tid]) + (sh[2][tid] + sh[3][tid]);
    return;
  }
  // ---- node block: prediction k, nodes c * 256 + tid for c = j, j + bpn, ...
  const int nb = b - nbe, k = nb / bpn, j = nb % bpn;
  const Elem cn = node_elem(r);
  const bool has_class = r.node_classes != nullptr && (r.terms & PEMP_LOSS_TERM_CLASS);
  double accF = 0.0, accM = 0.0, accC = 0.0;
  const int64_t chunks = (r.N + kBlock - 1) / kBlock;
  for (int64_t c = j; c < chunks; c += bpn) {
    const int64_t n = c * kBlock + tid;
    float f = 0.f, m = 0.f, cl = 0.f;
    if (n < r.N) {
      const float t = r.node_labels[n];
      m = r.label_mask_node[n];
      f = elem_fwd(cn, r.pn[k][n], t, m);
      if (has_class) {
        float v[PEMP_LOSS_MAXJ], sum, picked;
        class_row(r.pc[k] + n * r.J, r.J, r.node_classes[n], v, &sum, &picked);
        cl = (logf(sum) - picked) * t;
      }
    }
    accF += (double)wave_sum_f32(f);
    accM += (double)wave_sum_f32(m);
    accC += (double)wave_sum_f32(cl);
  }
  if (lane == 0) sh[wave][0] = accF, sh[wave][1] = accM, sh[wave][2] = accC;
  __syncthreads();
  if (tid < kNodeSlots) npart[(size_t)nb * kNodeSlots + tid] = (sh[0][tid] + sh[1][tid]) + (sh[2][tid] + sh[3][tid]);
}

// One block. Slot sums in fp64 (a wave per slot: lane l adds blocks l, l + 64, ... in order, then the lane tree), then
// the means, the NaN rule of the edge term, the weights, and the scales the backward multiplies by.
__global__ __launch_bounds__(kBlock) void loss_reduce_kernel(pemp_loss_rec r, int nbe, int bpn,
                                                             const double* __restrict__ epart,
                                                             const double* __restrict__ npart, float* __restrict__ out) {
  __shared__ double es[2 * PEMP_LOSS_MAXKE], ns[kNodeSlots * PEMP_LOSS_MAXKN];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n_es = 2 * r.K_e, n_ns = kNodeSlots * r.K_n;
  for (int s = wave; s < n_es + n_ns; s += kBlock / 64) {
    double v = 0.0;
    if (s < n_es) {
      for (int blk = lane; blk < nbe; blk += 64) v += epart[(size_t)blk * n_es + s];
    } else {
      const int k = (s - n_es) / kNodeSlots, slot = (s - n_es) % kNodeSlots;
      for (int blk = lane; blk < bpn; blk += 64) v += npart[((size_t)k * bpn + blk) * kNodeSlots + slot];
    }
    v = wave_sum_f64(v);
    if (lane == 0) (s < n_es ? es[s] : ns[s - n_es]) = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const bool use_node = r.terms & PEMP_LOSS_TERM_NODE, use_edge = r.terms & PEMP_LOSS_TERM_EDGE;
  const bool use_class = (r.terms & PEMP_LOSS_TERM_CLASS) && r.node_classes != nullptr;
  double node = 0.0, edge = 0.0, cls = 0.0;
  for (int k = 0; k < PEMP_LOSS_MAXKN; ++k) out[kOutNodeScale + k] = 0.f;
  for (int k = 0; k < PEMP_LOSS_MAXKE; ++k) out[kOutEdgeScale + k] = 0.f;
  out[5] = out[6] = out[7] = 0.f;
  if (use_node) {
    for (int k = 0; k < r.K_n; ++k) {
      const double den = r.node_kind == PEMP_LOSS_FOCAL ? ns[kNodeSlots * k + 1] : (double)r.N;
      node += ns[kNodeSlots * k] / den;
      out[kOutNodeScale + k] = (float)((double)r.node_weight / ((double)r.K_n * den));
    }
    node /= (double)r.K_n;
  }
  if (use_edge) {
    for (int k = 0; k < r.K_e; ++k) {
      const double den = r.edge_kind == PEMP_LOSS_FOCAL ? es[2 * k + 1] : (double)r.E;
      edge += es[2 * k] / den;
    }
    edge /= (double)r.K_e;
    if (edge != edge) {                      // Utils/loss.py:844-845: a NaN edge term is 0.0 and carries no gradient
      edge = 0.0;
    } else {
      for (int k = 0; k < r.K_e; ++k) {
        const double den = r.edge_kind == PEMP_LOSS_FOCAL ? es[2 * k + 1] : (double)r.E;
        out[kOutEdgeScale + k] = (float)((double)r.edge_weight / ((double)r.K_e * den));
      }
    }
  }
  float class_scale = 0.f;
  if (use_class) {
    for (int k = 0; k < r.K_n; ++k) cls += ns[kNodeSlots * k + 2] / (double)r.N;
    cls /= (double)r.K_n;
    class_scale = (float)((double)r.class_weight / ((double)r.K_n * (double)r.N));
  }
  out[kOutClassScale] = class_scale;
  out[0] = (float)node;
  out[1] = (float)edge;
  out[2] = (float)cls;
  out[3] = (float)((double)r.node_weight * node + (double)r.edge_weight * edge + (double)r.class_weight * cls);
}

struct Grads {
  float* pe[PEMP_LOSS_MAXKE];
  float* pn[PEMP_LOSS_MAXKN];
  float* pc[PEMP_LOSS_MAXKN];
};

template <bool VEC>
__global__ __launch_bounds__(kBlock) void loss_bwd_kernel(pemp_loss_rec r, int nbe, int bpn, const float* __restrict__ out,
                                                          const float* __restrict__ grad_total, Grads g) {
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const float gt = grad_total ? grad_total[0] : 1.f;
  if (b < nbe) {
    const bool own_mask = r.edge_mask[0] == nullptr;
    const Elem ce = edge_elem(r);
    const int64_t chunks = (r.E + kChunk - 1) / kChunk;
    for (int64_t c = b; c < chunks; c += nbe) {
      for (int it = 0; it < kChunk / (4 * kBlock); ++it) {
        const int64_t e0 = c * kChunk + ((int64_t)it * kBlock + tid) * 4;
        if (e0 >= r.E) continue;
        Quad q;
        load_quad<VEC>(r, own_mask, e0, &q);
#pragma unroll
        for (int k = 0; k < PEMP_LOSS_MAXKE; ++k) {
          if (k < r.K_e && g.pe[k]) {
            const float scale = out[kOutEdgeScale + k];
            float d[4] = {0.f, 0.f, 0.f, 0.f};
            if (scale != 0.f) {              // the NaN rule (and a skipped edge term): exact zeros
              float x[4], m[4];
              load4<VEC>(r.pe[k], e0, q.n, x);
              quad_mask<VEC>(r, own_mask, k, e0, q, m);
#pragma unroll
              for (int i = 0; i < 4; ++i) d[i] = i < q.n ? elem_bwd(ce, x[i], q.t[i], m[i]) * scale * gt : 0.f;
            }
            store4<VEC>(g.pe[k], e0, q.n, d);
          }
        }
      }
    }
    return;
  }
  const int nb = b - nbe, k = nb / bpn, j = nb % bpn;
  const Elem cn = node_elem(r);
  const bool use_node = r.terms & PEMP_LOSS_TERM_NODE;
  const bool has_class = r.node_classes != nullptr && (r.terms & PEMP_LOSS_TERM_CLASS);
  const float nscale = out[kOutNodeScale + k], cscale = out[kOutClassScale];
  const int64_t chunks = (r.N + kBlock - 1) / kBlock;
  for (int64_t c = j; c < chunks; c += bpn) {
    const int64_t n = c * kBlock + tid;
    if (n >= r.N) continue;
    const float t = r.node_labels[n];
    if (g.pn[k]) g.pn[k][n] = use_node ? elem_bwd(cn, r.pn[k][n], t, r.label_mask_node[n]) * nscale * gt : 0.f;
    if (g.pc[k]) {
      float* row = g.pc[k] + n * r.J;
      if (has_class) {
        float v[PEMP_LOSS_MAXJ], sum, picked;
        const int64_t cls = r.node_classes[n];
        class_row(r.pc[k] + n * r.J, r.J, cls, v, &sum, &picked);
        const float w = t * cscale * gt * (picked == picked ? 1.f : NAN);
#pragma unroll
        for (int jj = 0; jj < PEMP_LOSS_MAXJ; ++jj)
          if (jj < r.J) row[jj] = (expf(v[jj]) / sum - ((int64_t)jj == cls ? 1.f : 0.f)) * w;
      } else {
        for (int jj = 0; jj < r.J; ++jj) row[jj] = 0.f;
      }
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int check_rec(const char* who, const pemp_loss_rec* r) {
  PEMP_CHECK_ARG(r, "%s: NULL record", who);
  PEMP_CHECK_ARG(r->N >= 0 && r->E >= 0, "%s: negative size (N = %lld, E = %lld)", who, (long long)r->N, (long long)r->E);
  PEMP_CHECK_ARG(r->N < INT_MAX, "%s: N = %lld exceeds the int32 node ids", who, (long long)r->N);
  PEMP_CHECK_ARG(r->K_e >= 1 && r->K_n >= 1, "%s: K_e = %d, K_n = %d (at least one prediction each)", who, r->K_e, r->K_n);
  if (r->K_e > PEMP_LOSS_MAXKE || r->K_n > PEMP_LOSS_MAXKN || r->J > PEMP_LOSS_MAXJ) {
    set_error("%s: K_e = %d, K_n = %d, J = %d beyond the limits %d, %d, %d", who, r->K_e, r->K_n, r->J, PEMP_LOSS_MAXKE,
              PEMP_LOSS_MAXKN, PEMP_LOSS_MAXJ);
    return PEMP_ERR_UNSUPPORTED;
  }
  PEMP_CHECK_ARG((r->edge_kind == PEMP_LOSS_FOCAL || r->edge_kind == PEMP_LOSS_BCE) &&
                     (r->node_kind == PEMP_LOSS_FOCAL || r->node_kind == PEMP_LOSS_BCE),
                 "%s: unknown kind (edge %d, node %d)", who, r->edge_kind, r->node_kind);
  PEMP_CHECK_ARG((r->terms & ~(PEMP_LOSS_TERM_NODE | PEMP_LOSS_TERM_EDGE | PEMP_LOSS_TERM_CLASS)) == 0,
                 "%s: unknown bits in terms (%d)", who, r->terms);
  const bool with_class = r->node_classes && (r->terms & PEMP_LOSS_TERM_CLASS);
  PEMP_CHECK_ARG(!with_class || r->J >= 1, "%s: J = %d with a class term", who, r->J);
  const bool own_mask = r->edge_mask[0] == nullptr;
  for (int k = 0; k < r->K_e; ++k) {
    PEMP_CHECK_ARG(r->E == 0 || r->pe[k], "%s: NULL pe[%d]", who, k);
    PEMP_CHECK_ARG(own_mask == (r->edge_mask[k] == nullptr), "%s: edge_mask holds %s at [%d]", who,
                   own_mask ? "a pointer" : "NULL", k);
  }
  PEMP_CHECK_ARG(!own_mask || r->K_n >= r->K_e, "%s: mask_k needs node prediction k (K_n = %d < K_e = %d)", who, r->K_n,
                 r->K_e);
  if (r->N > 0) {
    for (int k = 0; k < r->K_n; ++k) {
      PEMP_CHECK_ARG(r->pn[k], "%s: NULL pn[%d]", who, k);
      PEMP_CHECK_ARG(!with_class || r->pc[k], "%s: NULL pc[%d]", who, k);
    }
    PEMP_CHECK_ARG(r->node_labels && r->label_mask_node, "%s: NULL node_labels / label_mask_node", who);
  }
  if (r->E > 0) {
    PEMP_CHECK_ARG(r->edge_labels && r->label_mask, "%s: NULL edge_labels / label_mask", who);
    PEMP_CHECK_ARG(!own_mask || r->edge_index, "%s: NULL edge_index", who);
  }
  return PEMP_OK;
}

bool rec_aligned(const pemp_loss_rec* r) {
  bool ok = aligned16(r->edge_labels) && aligned16(r->label_mask);
  if (r->edge_index) ok = ok && aligned16(r->edge_index) && aligned16(r->edge_index + r->E);
  for (int k = 0; k < r->K_e; ++k) ok = ok && aligned16(r->pe[k]) && aligned16(r->edge_mask[k]);
  return ok;
}

}  // namespace
}  // namespace pemp

using namespace pemp;

extern "C" size_t pemp_loss_workspace_size(int64_t N, int64_t E, int K_e, int K_n) {
  if (N < 0 || E < 0 || K_e < 1 || K_n < 1 || K_e > PEMP_LOSS_MAXKE || K_n > PEMP_LOSS_MAXKN) return 0;
  const Grid g = grid_for(N, E, K_n);
  return align_up((size_t)g.nbe * 2 * K_e * sizeof(double), 256) + align_up((size_t)g.nbn * kNodeSlots * sizeof(double), 256) +
         256;
}

extern "C" int pemp_loss_fwd(const pemp_loss_rec* rec, void* workspace, size_t workspace_bytes, float* out, void* stream) {
  const int rc = check_rec("pemp_loss_fwd", rec);
  if (rc != PEMP_OK) return rc;
  PEMP_CHECK_ARG(out, "pemp_loss_fwd: NULL out");
  const size_t need = pemp_loss_workspace_size(rec->N, rec->E, rec->K_e, rec->K_n);
  if (!workspace || workspace_bytes < need) {
    set_error("pemp_loss_fwd: workspace of %zu bytes, %zu needed", workspace ? workspace_bytes : (size_t)0, need);
    return PEMP_ERR_WORKSPACE;
  }
  const Grid g = grid_for(rec->N, rec->E, rec->K_n);
  Carver cv(workspace);
  double* epart = cv.take<double>((size_t)g.nbe * 2 * rec->K_e);
  double* npart = cv.take<double>((size_t)g.nbn * kNodeSlots);
  hipStream_t st = as_stream(stream);
  if (g.nbe + g.nbn > 0) {
    ProfScope prof("loss_fwd", st);
    if (rec_aligned(rec))
      loss_fwd_kernel<true><<<dim3(g.nbe + g.nbn), dim3(kBlock), 0, st>>>(*rec, g.nbe, g.bpn, epart, npart);
    else
      loss_fwd_kernel<false><<<dim3(g.nbe + g.nbn), dim3(kBlock), 0, st>>>(*rec, g.nbe, g.bpn, epart, npart);
    PEMP_LAUNCH_CHECK();
  }
  {
    ProfScope prof("loss_reduce", st);
    loss_reduce_kernel<<<dim3(1), dim3(kBlock), 0, st>>>(*rec, g.nbe, g.bpn, epart, npart, out);
    PEMP_LAUNCH_CHECK();
  }
  return PEMP_OK;
}

extern "C" int pemp_loss_bwd(const pemp_loss_rec* rec, const float* out, const float* grad_total, float* const* g_pe,
                             float* const* g_pn, float* const* g_pc, void* stream) {
  const int rc = check_rec("pemp_loss_bwd", rec);
  if (rc != PEMP_OK) return rc;
  PEMP_CHECK_ARG(out, "pemp_loss_bwd: NULL out");
  Grads g;
  bool vec = rec_aligned(rec);
  for (int k = 0; k < PEMP_LOSS_MAXKE; ++k) {
    g.pe[k] = (g_pe && k < rec->K_e) ? g_pe[k] : nullptr;
    vec = vec && aligned16(g.pe[k]);
  }
  for (int k = 0; k < PEMP_LOSS_MAXKN; ++k) {
    g.pn[k] = (g_pn && k < rec->K_n) ? g_pn[k] : nullptr;
    g.pc[k] = (g_pc && k < rec->K_n) ? g_pc[k] : nullptr;
    PEMP_CHECK_ARG(!g.pc[k] || rec->J >= 1, "pemp_loss_bwd: g_pc[%d] with J = %d", k, rec->J);
  }
  const Grid gr = grid_for(rec->N, rec->E, rec->K_n);
  if (gr.nbe + gr.nbn == 0) return PEMP_OK;
  hipStream_t st = as_stream(stream);
  ProfScope prof("loss_bwd", st);
  if (vec)
    loss_bwd_kernel<true><<<dim3(gr.nbe + gr.nbn), dim3(kBlock), 0, st>>>(*rec, gr.nbe, gr.bpn, out, grad_total, g);
  else
    loss_bwd_kernel<false><<<dim3(gr.nbe + gr.nbn), dim3(kBlock), 0, st>>>(*rec, gr.nbe, gr.bpn, out, grad_total, g);
  PEMP_LAUNCH_CHECK();
  return PEMP_OK;
}
