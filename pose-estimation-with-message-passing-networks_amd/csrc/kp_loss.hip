// The keypoint losses (pemp_amd/kp_loss.py): the heatmap and associative-embedding terms of the reference's
// ClassMultiLossFactory (Utils/loss.py:641-665; HeatmapLoss :17-27, AELoss :37-98) over up to four stages, fused each
// way. The contract is in pemp.h (pemp_kp_loss_*).
//
// Forward: one launch of streaming blocks and AE blocks, then a one-block reduction.
//   Streaming blocks: the J heatmap planes of an image are J H W contiguous floats of pred (image stride C H W) and of
//   gt; a unit is (image, kChunk consecutive elements of them), a stage's blocks stride over its units. A thread takes
//   four quads of a unit (16-byte loads when H W is a multiple of 4 and the three bases are 16-byte aligned: a quad
//   then lies inside one plane and its mask quad is aligned too; one element at a time otherwise). The mask, 1 / J of
//   the pred bytes, is fetched from HBM once and comes from the L2 for the other planes.
//   Sums: fp32 inside a thread's 16 elements and through the wave, fp64 per wave across units, across the four waves
//   and in the reduction; every block stores one partial into a slot of its own.
//   AE blocks, one per (stage, image): the P J listed tags go to LDS as fp64; a lane per person forms n_p, m_p and
//   pull_p in joint order, then wave 0 forms the P' x P' push rows, a lane per row, and the lane tree adds them.
// Backward: one streaming launch that owns every element of g_pred (the heatmap planes recomputed from pred, gt and
//   mask, the tag planes zero), then, behind it on the stream, one block per (stage, image) that writes the listed tag
//   entries. Entries of an image that share an index are added in entry order by the lane of the first of them.
#include <limits.h>
#include <math.h>

#include "pemp_common.h"

namespace pemp {
namespace {

constexpr int kBlock = 256;
constexpr int kChunk = PEMP_KP_CHUNK;            // elements per unit: 4 x 256 threads x 4
constexpr int kQuads = kChunk / (4 * kBlock);
constexpr int kMaxBlocks = PEMP_KP_MAXBLOCKS;    // per stage (memory-bound cap; the rest is strided)
constexpr int kMaxEntries = PEMP_KP_MAXP * PEMP_KP_MAXJ;
constexpr int64_t kMaxImage = (int64_t)INT_MAX - 2 * kChunk;   // C H W of an image: element ids stay int32
constexpr int kOutStage = 3;                     // out[3 + 3 s + {0, 1, 2}]: heatmap, push, pull of stage s

// Workspace: [status 256 B][block partials][per (s, b): push, pull][bad][P'][m (s, b, p)][n (s, b, p)]
struct Ws {
  int32_t* status;
  double* hpart;
  double* ae;        // [S B 2]
  int32_t* bad;      // [S B] visible entries with an index outside [0, T)
  int32_t* pcount;   // [S B] P'
  double* m;         // [S B P]
  int32_t* n;        // [S B P]
  size_t bytes;
};

int64_t units_of(int64_t per_image, int B) { return (int64_t)B * ((per_image + kChunk - 1) / kChunk); }
int blocks_of(int64_t units) { return (int)(units < kMaxBlocks ? units : kMaxBlocks); }

// the forward's block table: heatmap blocks of every stage with with_heatmap, then B AE blocks per stage with with_ae;
// blk0[s] for s >= S repeats the end of the streaming blocks, so [s + 1] - [s] is a stage's count for every s
void plan_fwd(pemp_kp_loss_rec* r) {
  int b = 0;
  for (int s = 0; s < PEMP_KP_MAXS; ++s) {
    r->blk0[s] = b;
    if (s < r->S && r->stage[s].with_heatmap)
      b += blocks_of(units_of((int64_t)r->J * r->stage[s].H * r->stage[s].W, r->B));
  }
  r->blk0[PEMP_KP_MAXS] = b;
  for (int s = 0; s < r->S; ++s)
    if (r->stage[s].with_ae) b += r->B;
  r->blk0[PEMP_KP_MAXS + 1] = b;
}

Ws carve(const pemp_kp_loss_rec* r, void* base) {
  pemp_kp_loss_rec c = *r;
  plan_fwd(&c);
  Carver cv(base);
  Ws w;
  const size_t SB = (size_t)r->S * r->B;
  w.status = cv.take<int32_t>(64);
  w.hpart = cv.take<double>((size_t)c.blk0[PEMP_KP_MAXS]);
  w.ae = cv.take<double>(SB * 2);
  w.bad = cv.take<int32_t>(SB);
  w.pcount = cv.take<int32_t>(SB);
  w.m = cv.take<double>(SB * r->P);
  w.n = cv.take<int32_t>(SB * r->P);
  w.bytes = align_up(cv.used, 256);
  return w;
}

__device__ __forceinline__ bool aligned16_dev(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the stage of streaming block b
__device__ __forceinline__ int stage_of(const pemp_kp_loss_rec& r, int b) {
  int s = 0;
#pragma unroll
  for (int k = 1; k < PEMP_KP_MAXS; ++k) s += b >= r.blk0[k] ? 1 : 0;
  return s;
}

// the stage of AE block number a (B per stage with the flag, stages ascending) among the stages `on` marks
__device__ __forceinline__ int ae_stage_of(const pemp_kp_loss_rec& r, int a, unsigned on) {
  int k = a / r.B, s = 0;
  for (; s < r.S; ++s) {
    if (!((on >> s) & 1)) continue;
    if (k == 0) break;
    --k;
  }
  return s;
}

// ---- the AE entries of one image in LDS ---------------------------------------------------------------------
struct alignas(16) Entries {
  int idx[kMaxEntries];       // the tag index, -1 for an entry that is not visible or out of range (and for the
                              // padding up to a multiple of 4 entries)
  double t[kMaxEntries];
};

// returns this thread's count of visible entries with an index outside [0, T)
__device__ __forceinline__ int load_entries(const pemp_kp_loss_rec& r, const pemp_kp_stage& st, int img, Entries* e) {
  const int PJ = r.P * r.J;
  const int64_t HW = (int64_t)st.H * st.W, T = (int64_t)(st.C - r.J) * HW;
  const float* tags = st.pred + ((int64_t)img * st.C + r.J) * HW;
  const int32_t* tg = st.tag + (int64_t)img * PJ * 2;
  int bad = 0;
  for (int i = threadIdx.x; i < ((PJ + 3) & ~3); i += kBlock) {
    const bool in = i < PJ;
    const int32_t id = in ? tg[2 * i] : 0, vis = in ? tg[2 * i + 1] : 0;
    int keep = -1;
    if (vis > 0) {
      if (id >= 0 && (int64_t)id < T)
        keep = id;
      else
        ++bad;
    }
    e->idx[i] = keep;
    e->t[i] = keep >= 0 ? (double)tags[keep] : 0.0;
  }
  return bad;
}

__device__ __forceinline__ double push_f(int kind, double d) {
  return kind == PEMP_KP_AE_EXP ? exp(-d * d) : fmax(0.0, 1.0 - fabs(d));
}
// d f / d d; the 'max' form as autograd has it away from its kinks (abs' (0) = 0)
__device__ __forceinline__ double push_df(int kind, double d) {
  if (kind == PEMP_KP_AE_EXP) return -2.0 * d * exp(-d * d);
  return fabs(d) < 1.0 ? (d > 0.0 ? -1.0 : (d < 0.0 ? 1.0 : 0.0)) : 0.0;
}

__global__ __launch_bounds__(kBlock) void kp_loss_fwd_kernel(pemp_kp_loss_rec r, Ws w) {
  __shared__ Entries ent;
  __shared__ double sh[kBlock / 64];
  __shared__ double m_s[PEMP_KP_MAXP], pull_s[PEMP_KP_MAXP];
  __shared__ int n_s[PEMP_KP_MAXP], bad_s[kBlock / 64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // the AE blocks come first in the grid: each is one long dependent chain, and started last it would be the tail
  const int nae = r.blk0[PEMP_KP_MAXS + 1] - r.blk0[PEMP_KP_MAXS];
  const int b = (int)blockIdx.x - nae;
  if (b >= 0) {                                         // ---- streaming block
    const int s = stage_of(r, b);
    const pemp_kp_stage& st = r.stage[s];
    const int32_t HW = st.H * st.W, n = r.J * HW;
    const int32_t cpi = (n + kChunk - 1) / kChunk;      // units per image
    const int64_t units = (int64_t)r.B * cpi;
    const int nblk = r.blk0[s + 1] - r.blk0[s];
    const bool vec = (HW & 3) == 0 && aligned16_dev(st.pred) && aligned16_dev(st.gt) && aligned16_dev(st.mask);
    double acc = 0.0;
    for (int64_t u = b - r.blk0[s]; u < units; u += nblk) {
      const int img = (int)(u / cpi);
      const int32_t c0 = (int32_t)(u % cpi) * kChunk;
      const float* p = st.pred + (int64_t)img * st.C * HW;
      const float* g = st.gt + (int64_t)img * n;
      const float* m = st.mask + (int64_t)img * HW;
      float f = 0.f;
      if (vec) {
        float4 a[kQuads], c[kQuads], k[kQuads];
#pragma unroll
        for (int it = 0; it < kQuads; ++it) {
          const int32_t i = c0 + (it * kBlock + tid) * 4;
          if (i < n) {
            a[it] = *reinterpret_cast<const float4*>(p + i);
            c[it] = *reinterpret_cast<const float4*>(g + i);
            k[it] = *reinterpret_cast<const float4*>(m + (uint32_t)i % (uint32_t)HW);
          } else {
            a[it] = c[it] = k[it] = make_float4(0.f, 0.f, 0.f, 0.f);
          }
        }
#pragma unroll
        for (int it = 0; it < kQuads; ++it) {
          const float dx = a[it].x - c[it].x, dy = a[it].y - c[it].y, dz = a[it].z - c[it].z, dw = a[it].w - c[it].w;
          f += dx * dx * k[it].x;
          f += dy * dy * k[it].y;
          f += dz * dz * k[it].z;
          f += dw * dw * k[it].w;
        }
      } else {
#pragma unroll 4
        for (int it = 0; it < kChunk / kBlock; ++it) {
          const int32_t i = c0 + it * kBlock + tid;
          if (i < n) {
            const float d = p[i] - g[i];
            f += d * d * m[(uint32_t)i % (uint32_t)HW];
          }
        }
      }
      acc += (double)wave_sum_f32(f);
    }
    if (lane == 0) sh[wave] = acc;
    __syncthreads();
    if (tid == 0) w.hpart[b] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    return;
  }
  // ---- AE block: (stage, image)
  unsigned on = 0;
  for (int s = 0; s < r.S; ++s) on |= r.stage[s].with_ae ? 1u << s : 0u;
  const int a = blockIdx.x;
  const int s = ae_stage_of(r, a, on), img = a % r.B;
  const pemp_kp_stage& st = r.stage[s];
  const int bad = wave_sum_i32(load_entries(r, st, img, &ent));
  if (lane == 0) bad_s[wave] = bad;
  __syncthreads();
  if (tid < r.P) {                                      // a lane per person, joints in order
    const int base = tid * r.J;
    int n = 0;
    double sum = 0.0;
    for (int j = 0; j < r.J; ++j)
      if (ent.idx[base + j] >= 0) sum += ent.t[base + j], ++n;
    const double m = n ? sum / n : 0.0;
    double pull = 0.0;
    for (int j = 0; j < r.J; ++j)
      if (ent.idx[base + j] >= 0) pull += (ent.t[base + j] - m) * (ent.t[base + j] - m);
    m_s[tid] = m, n_s[tid] = n, pull_s[tid] = n ? pull / n : 0.0;
  }
  __syncthreads();
  if (wave != 0) return;
  const size_t sb = (size_t)s * r.B + img;
  const bool person = lane < r.P && n_s[lane] > 0;
  double row = 0.0;
  if (person)
    for (int q = 0; q < r.P; ++q)
      if (n_s[q] > 0) row += push_f(r.ae_kind, m_s[lane] - m_s[q]);
  row = wave_sum_f64(row);
  const double pulls = wave_sum_f64(person ? pull_s[lane] : 0.0);
  const int pc = wave_sum_i32(person ? 1 : 0);
  if (lane < r.P) w.m[sb * r.P + lane] = m_s[lane], w.n[sb * r.P + lane] = n_s[lane];
  if (lane == 0) {
    w.ae[2 * sb] = pc >= 2 ? 0.5 * (row - pc) / ((double)(pc - 1) * pc) : 0.0;
    w.ae[2 * sb + 1] = pc >= 1 ? pulls / pc : 0.0;
    w.pcount[sb] = pc;
    w.bad[sb] = (bad_s[0] + bad_s[1]) + (bad_s[2] + bad_s[3]);
  }
}

// One block: wave s adds the partials of stage s (lane l the blocks l, l + 64, ... in order, then the lane tree);
// thread 0 then adds the images' push and pull in image order and forms the terms.
__global__ __launch_bounds__(kBlock) void kp_loss_reduce_kernel(pemp_kp_loss_rec r, Ws w, float* __restrict__ out) {
  __shared__ double hs[PEMP_KP_MAXS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  {
    double v = 0.0;
#pragma unroll 4
    for (int blk = r.blk0[wave] + lane; blk < r.blk0[wave + 1]; blk += 64) v += w.hpart[blk];
    v = wave_sum_f64(v);
    if (lane == 0) hs[wave] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double heat = 0.0, ae = 0.0;
  int bad = 0;
  for (int s = 0; s < PEMP_KP_MAXS; ++s) {
    double h = 0.0, push = 0.0, pull = 0.0;
    if (s < r.S) {
      const pemp_kp_stage& st = r.stage[s];
      if (st.with_heatmap) h = (double)st.heatmap_factor * hs[s] / ((double)r.B * r.J * st.H * st.W);
      if (st.with_ae) {
        for (int b = 0; b < r.B; ++b) {
          const size_t sb = (size_t)s * r.B + b;
          push += w.ae[2 * sb], pull += w.ae[2 * sb + 1], bad += w.bad[sb];
        }
        push = (double)st.push_factor * push / r.B;
        pull = (double)st.pull_factor * pull / r.B;
      }
    }
    heat += h;
    ae += push + pull;
    out[kOutStage + 3 * s] = (float)h, out[kOutStage + 3 * s + 1] = (float)push, out[kOutStage + 3 * s + 2] = (float)pull;
  }
  out[0] = (float)heat, out[1] = (float)ae, out[2] = (float)(heat + ae);
  out[PEMP_KP_OUT - 1] = 0.f;
  w.status[0] = bad;
}

struct Grads {
  float* g[PEMP_KP_MAXS];
};

// every element of g_pred[s]: units over the C H W floats of an image; the first J H W get the heatmap gradient
__global__ __launch_bounds__(kBlock) void kp_loss_bwd_kernel(pemp_kp_loss_rec r, const float* __restrict__ grad_total,
                                                             Grads gr) {
  const int tid = threadIdx.x, b = blockIdx.x;
  const int s = stage_of(r, b);
  const pemp_kp_stage& st = r.stage[s];
  const int32_t HW = st.H * st.W, n = r.J * HW, tot = st.C * HW;
  const int32_t cpi = (tot + kChunk - 1) / kChunk;
  const int64_t units = (int64_t)r.B * cpi;
  const int nblk = r.blk0[s + 1] - r.blk0[s];
  const bool heat = st.with_heatmap != 0;
  const bool vec = (HW & 3) == 0 && aligned16_dev(gr.g[s]) &&
                   (!heat || (aligned16_dev(st.pred) && aligned16_dev(st.gt) && aligned16_dev(st.mask)));
  const double gt = grad_total ? (double)grad_total[0] : 1.0;
  const float c = heat ? (float)(2.0 * (double)st.heatmap_factor / ((double)r.B * (double)n) * gt) : 0.f;
  for (int64_t u = b - r.blk0[s]; u < units; u += nblk) {
    const int img = (int)(u / cpi);
    const int32_t c0 = (int32_t)(u % cpi) * kChunk;
    const float* p = st.pred + (int64_t)img * tot;
    const float* g = st.gt + (int64_t)img * n;
    const float* m = st.mask + (int64_t)img * HW;
    float* o = gr.g[s] + (int64_t)img * tot;
    if (vec) {
      float4 a[kQuads], q[kQuads], k[kQuads];
#pragma unroll
      for (int it = 0; it < kQuads; ++it) {
        const int32_t i = c0 + (it * kBlock + tid) * 4;
        if (heat && i < n) {
          a[it] = *reinterpret_cast<const float4*>(p + i);
          q[it] = *reinterpret_cast<const float4*>(g + i);
          k[it] = *reinterpret_cast<const float4*>(m + (uint32_t)i % (uint32_t)HW);
        } else {
          a[it] = q[it] = k[it] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
#pragma unroll
      for (int it = 0; it < kQuads; ++it) {
        const int32_t i = c0 + (it * kBlock + tid) * 4;
        if (i < tot)
          *reinterpret_cast<float4*>(o + i) =
              make_float4((a[it].x - q[it].x) * k[it].x * c, (a[it].y - q[it].y) * k[it].y * c,
                          (a[it].z - q[it].z) * k[it].z * c, (a[it].w - q[it].w) * k[it].w * c);
      }
    } else {
#pragma unroll 4
      for (int it = 0; it < kChunk / kBlock; ++it) {
        const int32_t i = c0 + it * kBlock + tid;
        if (i < tot) o[i] = (heat && i < n) ? (p[i] - g[i]) * m[(uint32_t)i % (uint32_t)HW] * c : 0.f;
      }
    }
  }
}

// One block per (stage, image) of the stages `on` marks: d total / d t_i of the listed entries, from the forward's
// m_p, n_p and P'. d pull_b / d t_i = 2 (t_i - m_p) / (n_p P') (the terms through m_p cancel: sum_i (t_i - m_p) = 0);
// d push_b / d t_i = sum_q f'(m_p - m_q) / ((P' - 1) P' n_p) (f is even, so the two places of m_p give the same sum).
__global__ __launch_bounds__(kBlock) void kp_loss_bwd_tags_kernel(pemp_kp_loss_rec r, Ws w, unsigned on,
                                                                  const float* __restrict__ grad_total, Grads gr) {
  __shared__ Entries ent;
  __shared__ alignas(16) float g_s[kMaxEntries];
  __shared__ double m_s[PEMP_KP_MAXP], cpull[PEMP_KP_MAXP], cpush[PEMP_KP_MAXP];
  __shared__ int n_s[PEMP_KP_MAXP];
  const int tid = threadIdx.x;
  const int s = ae_stage_of(r, blockIdx.x, on), img = blockIdx.x % r.B;
  const pemp_kp_stage& st = r.stage[s];
  const size_t sb = (size_t)s * r.B + img;
  const int pc = w.pcount[sb];
  if (pc == 0) return;                                  // no person: no gradient (block-uniform)
  load_entries(r, st, img, &ent);
  if (tid < r.P) m_s[tid] = w.m[sb * r.P + tid], n_s[tid] = w.n[sb * r.P + tid];
  __syncthreads();
  const double gt = grad_total ? (double)grad_total[0] : 1.0;
  if (tid < r.P) {
    double cl = 0.0, cs = 0.0;
    if (n_s[tid] > 0) {
      cl = (double)st.pull_factor * gt * 2.0 / ((double)r.B * pc * n_s[tid]);
      if (pc >= 2) {
        double d = 0.0;
        for (int q = 0; q < r.P; ++q)
          if (n_s[q] > 0) d += push_df(r.ae_kind, m_s[tid] - m_s[q]);
        cs = (double)st.push_factor * gt * d / ((double)r.B * (double)(pc - 1) * pc * n_s[tid]);
      }
    }
    cpull[tid] = cl, cpush[tid] = cs;
  }
  __syncthreads();
  const int PJ = r.P * r.J, PJ4 = (PJ + 3) & ~3;
  for (int i = tid; i < PJ4; i += kBlock) {
    const int p = i / r.J;
    g_s[i] = ent.idx[i] >= 0 ? (float)(cpull[p] * (ent.t[i] - m_s[p]) + cpush[p]) : 0.f;
  }
  __syncthreads();
  float* o = gr.g[s] + ((int64_t)img * st.C + r.J) * ((int64_t)st.H * st.W);
  for (int i = tid; i < PJ; i += kBlock) {
    const int id = ent.idx[i];
    if (id < 0) continue;
    // one pass over all entries, four per LDS read: an equal index before i means an earlier entry owns this one;
    // the equal ones from i on are added in entry order (0 + g_i first, which is g_i)
    bool first = true;
    float sum = 0.f;
#pragma unroll 2
    for (int k = 0; k < PJ4; k += 4) {
      const int4 q = *reinterpret_cast<const int4*>(&ent.idx[k]);
      const float4 v = *reinterpret_cast<const float4*>(&g_s[k]);
      const bool e0 = q.x == id, e1 = q.y == id, e2 = q.z == id, e3 = q.w == id;
      first = first && !((e0 && k < i) || (e1 && k + 1 < i) || (e2 && k + 2 < i) || (e3 && k + 3 < i));
      sum += (e0 && k >= i) ? v.x : 0.f;
      sum += (e1 && k + 1 >= i) ? v.y : 0.f;
      sum += (e2 && k + 2 >= i) ? v.z : 0.f;
      sum += (e3 && k + 3 >= i) ? v.w : 0.f;
    }
    if (first) o[id] = sum;                             // id < T was checked when the entry was loaded
  }
}

int check_rec(const char* who, const pemp_kp_loss_rec* r) {
  PEMP_CHECK_ARG(r, "%s: NULL record", who);
  if (r->S > PEMP_KP_MAXS || r->P > PEMP_KP_MAXP || r->J > PEMP_KP_MAXJ) {
    set_error("%s: S = %d, P = %d, J = %d beyond the limits %d, %d, %d", who, r->S, r->P, r->J, PEMP_KP_MAXS,
              PEMP_KP_MAXP, PEMP_KP_MAXJ);
    return PEMP_ERR_UNSUPPORTED;
  }
  PEMP_CHECK_ARG(r->S >= 1 && r->B >= 1 && r->J >= 1 && r->P >= 0, "%s: S = %d, B = %d, J = %d, P = %d", who, r->S, r->B,
                 r->J, r->P);
  PEMP_CHECK_ARG(r->ae_kind == PEMP_KP_AE_EXP || r->ae_kind == PEMP_KP_AE_MAX, "%s: unknown ae_kind %d", who, r->ae_kind);
  for (int s = 0; s < r->S; ++s) {
    const pemp_kp_stage& st = r->stage[s];
    PEMP_CHECK_ARG(st.H >= 1 && st.W >= 1 && st.C >= r->J, "%s: stage %d: C = %d, H = %d, W = %d with J = %d", who, s, st.C,
                   st.H, st.W, r->J);
    PEMP_CHECK_ARG((int64_t)st.C * st.H * st.W <= kMaxImage, "%s: stage %d: C H W = %lld exceeds the int32 element ids", who, s,
                   (long long)st.C * st.H * st.W);
    PEMP_CHECK_ARG(st.pred, "%s: stage %d: NULL pred", who, s);
    PEMP_CHECK_ARG(!st.with_heatmap || (st.gt && st.mask), "%s: stage %d: NULL gt / mask with with_heatmap", who, s);
    PEMP_CHECK_ARG(!st.with_ae || (st.tag && st.C > r->J && r->P >= 1),
                   "%s: stage %d: with_ae needs tag, C > J and P >= 1 (C = %d, P = %d)", who, s, st.C, r->P);
  }
  return PEMP_OK;
}

}  // namespace
}  // namespace pemp

using namespace pemp;

extern "C" size_t pemp_kp_loss_workspace_size(const pemp_kp_loss_rec* rec) {
  if (!rec || rec->S < 1 || rec->S > PEMP_KP_MAXS || rec->B < 1 || rec->J < 1 || rec->J > PEMP_KP_MAXJ || rec->P < 0 ||
      rec->P > PEMP_KP_MAXP)
    return 0;
  for (int s = 0; s < rec->S; ++s)
    if (rec->stage[s].H < 1 || rec->stage[s].W < 1 || (int64_t)rec->stage[s].C * rec->stage[s].H * rec->stage[s].W > kMaxImage)
      return 0;
  return carve(rec, nullptr).bytes;
}

extern "C" int pemp_kp_loss_fwd(const pemp_kp_loss_rec* rec, void* workspace, size_t workspace_bytes, float* out,
                                void* stream) {
  const int rc = check_rec("pemp_kp_loss_fwd", rec);
  if (rc != PEMP_OK) return rc;
  PEMP_CHECK_ARG(out, "pemp_kp_loss_fwd: NULL out");
  const Ws w = carve(rec, workspace);
  if (!workspace || workspace_bytes < w.bytes) {
    set_error("pemp_kp_loss_fwd: workspace of %zu bytes, %zu needed", workspace ? workspace_bytes : (size_t)0, w.bytes);
    return PEMP_ERR_WORKSPACE;
  }
  pemp_kp_loss_rec r = *rec;
  plan_fwd(&r);
  hipStream_t st = as_stream(stream);
  if (r.blk0[PEMP_KP_MAXS + 1] > 0) {
    ProfScope prof("kp_loss_fwd", st);
    kp_loss_fwd_kernel<<<dim3(r.blk0[PEMP_KP_MAXS + 1]), dim3(kBlock), 0, st>>>(r, w);
    PEMP_LAUNCH_CHECK();
  }
  {
    ProfScope prof("kp_loss_reduce", st);
    kp_loss_reduce_kernel<<<dim3(1), dim3(kBlock), 0, st>>>(r, w, out);
    PEMP_LAUNCH_CHECK();
  }
  return PEMP_OK;
}

extern "C" int pemp_kp_loss_bwd(const pemp_kp_loss_rec* rec, const void* workspace, const float* grad_total,
                                float* const* g_pred, void* stream) {
  const int rc = check_rec("pemp_kp_loss_bwd", rec);
  if (rc != PEMP_OK) return rc;
  PEMP_CHECK_ARG(workspace && g_pred, "pemp_kp_loss_bwd: NULL workspace / g_pred");
  const Ws w = carve(rec, const_cast<void*>(workspace));
  pemp_kp_loss_rec r = *rec;
  Grads gr;
  int blocks = 0, ae_blocks = 0;
  unsigned on = 0;
  for (int s = 0; s < PEMP_KP_MAXS; ++s) {
    gr.g[s] = s < r.S ? g_pred[s] : nullptr;
    r.blk0[s] = blocks;
    if (!gr.g[s]) continue;
    blocks += blocks_of(units_of((int64_t)r.stage[s].C * r.stage[s].H * r.stage[s].W, r.B));
    if (r.stage[s].with_ae) on |= 1u << s, ae_blocks += r.B;
  }
  r.blk0[PEMP_KP_MAXS] = r.blk0[PEMP_KP_MAXS + 1] = blocks;
  if (blocks == 0) return PEMP_OK;
  hipStream_t st = as_stream(stream);
  {
    ProfScope prof("kp_loss_bwd", st);
    kp_loss_bwd_kernel<<<dim3(blocks), dim3(kBlock), 0, st>>>(r, grad_total, gr);
    PEMP_LAUNCH_CHECK();
  }
  if (ae_blocks > 0) {
    ProfScope prof("kp_loss_bwd_tags", st);
    kp_loss_bwd_tags_kernel<<<dim3(ae_blocks), dim3(kBlock), 0, st>>>(r, w, on, grad_total, gr);
    PEMP_LAUNCH_CHECK();
  }
  return PEMP_OK;
}
