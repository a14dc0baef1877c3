// Message-passing network, inference, for gfx950 — restates
//   NodeClassificationMPNSimple.py:62-97  embeddings, STEPS iterations with skip concat, heads
//   layers.py:157-258 TypeAwareMPNLayer (per-source-type messages, attention softmax per
//                     (target, source type) segment, update_mlp)
//   layers.py:32-86   MPLayer (single message MLP, scatter max/mean/add)
//   torch_scatter 2.0.4 scatter_softmax (exp(a - max) / (sum + 1e-12)), scatter sum/mean/max
//                     (empty segments -> 0).
//
// Layout (all fp32, hidden width 64). Edges are re-ordered once per call into type-major order
// (source type t, target i, original edge id) so that every (i, t) aggregation segment is
// contiguous and every 16-edge MFMA tile shares one message weight W_t. Per iteration:
//   node_step_kernel   : node table NT[n] = [W1_xi·x | W1_xj·x | W_t_xi·x + b_t (t < T)], x = [x0 | x],
//                        fused with the node update of the previous pass and the node/class heads
//   edge_step_kernel   : per 16-edge wave tile, three chained 64x64 MFMA GEMMs (edge MLP layer 1 on
//                        e_cur, layer 2, message), attention logit, segmented online softmax, and
//                        (recorded iterations) the fused edge-classification head. No atomics.
// MFMA: v_mfma_f32_16x16x4_f32 (exact fp32). Fragment convention per wave: item (edge or node)
// c = lane & 15 on the MFMA N dimension, features 16*blk + 4*(lane >> 4) + r in registers, so one
// layer's accumulator is the next layer's B operand with no data movement.
// The edge-order prepares (the first kernels of a forward) are in mpn_order.hip, reached through the launch functions
// of mpn_internal.h; mpn_order.h holds what the closed-form prepare shares with launch A of the paired prelude here.
#include <limits.h>

#include <algorithm>
#include <atomic>
#include <type_traits>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include <string.h>
#include <math.h>

#include "mpn_internal.h"
#include "mpn_order.h"

namespace pemp {
namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float a, float b, float c, float d) {
  *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
}

// acc[ob] += W[16ob + i][.] · in   (W row-major, row stride ldw; KB input / OB output blocks of 16)
// (The weight pointers of the GEMM helpers carry no __restrict__: the inliner's noalias scopes would
// replace the per-variable LDS scopes, and hipcc would then wait for every in-flight LDS-DMA of the edge
// pass before each weight read.)
template <int KB, int OB>
__device__ __forceinline__ void gemm_frag(const float* W, int ldw, const float (&in)[KB][4],
                                          float (&acc)[OB][4]) {
  const int lane = __lane_id(), i = lane & 15, g = lane >> 4;
#pragma unroll
  for (int ob = 0; ob < OB; ++ob) {
    f32x4 c = {acc[ob][0], acc[ob][1], acc[ob][2], acc[ob][3]};
#pragma unroll
    for (int mb = 0; mb < KB; ++mb) {
      const float4 w = ld4(W + (16 * ob + i) * ldw + 16 * mb + 4 * g);
      c = mfma4(w.x, in[mb][0], c);
      c = mfma4(w.y, in[mb][1], c);
      c = mfma4(w.z, in[mb][2], c);
      c = mfma4(w.w, in[mb][3], c);
    }
    acc[ob][0] = c[0]; acc[ob][1] = c[1]; acc[ob][2] = c[2]; acc[ob][3] = c[3];
  }
}

// ReLU as one integer max on the bit pattern (non-negative floats order as non-negative ints, every
// negative float is a negative int): fmaxf on an MFMA result compiles to a canonicalising max plus the
// max, two VALU issues per value. (An inline-asm v_max_f32 is not an option: the hazard recognizer does
// not pad an asm read of a fresh MFMA result.) -0.0 -> +0.0; NaN with a clear sign bit stays NaN.
__device__ __forceinline__ float relu1(float x) { return __int_as_float(max(__float_as_int(x), 0)); }

template <int NB>
__device__ __forceinline__ void relu_frag(float (&v)[NB][4]) {
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) v[b][r] = relu1(v[b][r]);
}

// One Linear (+ReLU) of a pemp_mlp with runtime dims <= 16*MAXB, weights from global memory.
template <int MAXKB, int MAXOB>
__device__ __forceinline__ void layer_rt(const pemp_layer& L, const float (&in)[MAXKB][4], float (&out)[MAXOB][4]) {
  const int lane = __lane_id(), i = lane & 15, g = lane >> 4;
  const int KB = (L.in_dim + 15) >> 4, OB = (L.out_dim + 15) >> 4, ldw = KB * 16;
#pragma unroll
  for (int ob = 0; ob < MAXOB; ++ob) {
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    if (ob < OB) {
      const float4 bb = ld4(L.b + 16 * ob + 4 * g);
      c[0] = bb.x; c[1] = bb.y; c[2] = bb.z; c[3] = bb.w;
#pragma unroll
      for (int mb = 0; mb < MAXKB; ++mb) {
        if (mb < KB) {
          const float4 w = ld4(L.w + (16 * ob + i) * ldw + 16 * mb + 4 * g);
          c = mfma4(w.x, in[mb][0], c);
          c = mfma4(w.y, in[mb][1], c);
          c = mfma4(w.z, in[mb][2], c);
          c = mfma4(w.w, in[mb][3], c);
        }
      }
      if (L.relu) {
#pragma unroll
        for (int r = 0; r < 4; ++r) c[r] = relu1(c[r]);
      }
    }
    out[ob][0] = c[0]; out[ob][1] = c[1]; out[ob][2] = c[2]; out[ob][3] = c[3];
  }
}

// Whole pemp_mlp on fragments (<= 4 layers, widths <= 16*MAXB). Result in `a`.
template <int MAXB>
__device__ __forceinline__ void mlp_frag(const pemp_mlp& m, float (&a)[MAXB][4], float (&b)[MAXB][4]) {
  layer_rt<MAXB, MAXB>(m.layer[0], a, b);
  if (m.n_layers > 1) layer_rt<MAXB, MAXB>(m.layer[1], b, a);
  if (m.n_layers > 2) layer_rt<MAXB, MAXB>(m.layer[2], a, b);
  if (m.n_layers > 3) layer_rt<MAXB, MAXB>(m.layer[3], b, a);
  if (m.n_layers == 1 || m.n_layers == 3) {
#pragma unroll
    for (int x = 0; x < MAXB; ++x)
#pragma unroll
      for (int r = 0; r < 4; ++r) a[x][r] = b[x][r];
  }
}

// ---------------------------------------------------------------------------------------------
// Row MLPs (node embedding, node/class heads): 16 rows per workgroup, 4 waves split outputs.
// ---------------------------------------------------------------------------------------------
constexpr int RS = 136;  // LDS row stride (<= 128 features), = 8 mod 64 dwords: conflict-free b128

struct RowsMlpArgs {
  pemp_mlp mlp;
  const float* in;
  int64_t ld_in, M;
  float* out;
  int64_t ld_out;
  float* out2;
  int64_t ld_out2;
};

__global__ __launch_bounds__(256) void rows_mlp_kernel(RowsMlpArgs a) {
  __shared__ __attribute__((aligned(16))) float act[2][16 * RS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * 16;
  const int K0 = a.mlp.layer[0].in_dim, KP = (K0 + 15) & ~15;
  for (int idx = threadIdx.x; idx < 16 * KP; idx += 256) {
    const int r = idx / KP, k = idx - r * KP;
    act[0][r * RS + k] = (row0 + r < a.M && k < K0) ? a.in[(row0 + r) * a.ld_in + k] : 0.0f;
  }
  __syncthreads();
  int cur = 0;
  for (int l = 0; l < a.mlp.n_layers; ++l) {
    const pemp_layer& L = a.mlp.layer[l];
    const int KB = (L.in_dim + 15) >> 4, OB = (L.out_dim + 15) >> 4, ldw = KB * 16;
    for (int ob = wave; ob < OB; ob += 4) {
      const float4 bb = ld4(L.b + 16 * ob + 4 * g);
      f32x4 c = {bb.x, bb.y, bb.z, bb.w};
      for (int mb = 0; mb < KB; ++mb) {
        const float4 w = ld4(L.w + (16 * ob + i) * ldw + 16 * mb + 4 * g);
        const float4 x = ld4(&act[cur][i * RS + 16 * mb + 4 * g]);
        c = mfma4(w.x, x.x, c);
        c = mfma4(w.y, x.y, c);
        c = mfma4(w.z, x.z, c);
        c = mfma4(w.w, x.w, c);
      }
      if (L.relu) {
#pragma unroll
        for (int r = 0; r < 4; ++r) c[r] = relu1(c[r]);
      }
      st4(&act[cur ^ 1][i * RS + 16 * ob + 4 * g], c[0], c[1], c[2], c[3]);
    }
    __syncthreads();
    cur ^= 1;
  }
  const int OD = a.mlp.layer[a.mlp.n_layers - 1].out_dim;
  for (int idx = threadIdx.x; idx < 16 * OD; idx += 256) {
    const int r = idx / OD, f = idx - r * OD;
    if (row0 + r < a.M) {
      const float v = act[cur][r * RS + f];
      a.out[(row0 + r) * a.ld_out + f] = v;
      if (a.out2) a.out2[(row0 + r) * a.ld_out2 + f] = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Edge embedding (sorted order): e_init = MLP(edge_attr[orig]); Q0 = W1_e_init·e_init + b1.
// ---------------------------------------------------------------------------------------------
// Widths up to 128 (not the published configuration): weights read from global memory.
__global__ __launch_bounds__(256) void edge_embed_wide_kernel(pemp_mlp emb, const float* __restrict__ ea, int A,
                                                         const int* __restrict__ s_orig, int64_t E,
                                                         const float* __restrict__ q0_w,
                                                         const float* __restrict__ q0_b, const float* __restrict__ e1_w,
                                                         float* __restrict__ r0, float* __restrict__ q0, float out_scale) {
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int64_t p = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16 + c;
  const bool valid = p < E;
  const int64_t o = valid ? s_orig[p] : 0;
  float a[8][4], b[8][4];
#pragma unroll
  for (int mb = 0; mb < 8; ++mb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int f = 16 * mb + 4 * g + r;
      a[mb][r] = (valid && f < A) ? ea[o * A + f] : 0.0f;
    }
  mlp_frag<8>(emb, a, b);
  float e[4][4], acc[4][4];
#pragma unroll
  for (int ob = 0; ob < 4; ++ob) {
    const float4 bb = ld4(q0_b + 16 * ob + 4 * g);
    acc[ob][0] = bb.x; acc[ob][1] = bb.y; acc[ob][2] = bb.z; acc[ob][3] = bb.w;
#pragma unroll
    for (int r = 0; r < 4; ++r) e[ob][r] = a[ob][r];
  }
  gemm_frag<4, 4>(q0_w, 64, e, acc);
  const float s = out_scale;                       // the edge passes' domain (f16x3: 2^11)
  if (valid) {
#pragma unroll
    for (int ob = 0; ob < 4; ++ob) st4(q0 + p * D + 16 * ob + 4 * g, acc[ob][0] * s, acc[ob][1] * s, acc[ob][2] * s, acc[ob][3] * s);
  }
  gemm_frag<4, 4>(e1_w, 64, e, acc);              // R0 = Q0 + W1_e_cur · e_init
  if (valid) {
#pragma unroll
    for (int ob = 0; ob < 4; ++ob) st4(r0 + p * D + 16 * ob + 4 * g, acc[ob][0] * s, acc[ob][1] * s, acc[ob][2] * s, acc[ob][3] * s);
  }
}

// ---- bf16x3 split precision (PREC 1): x·w ~= xh·wh + xl·wh + xh·wl with x = xh + xl, w = wh + wl,
// each part bf16 (RNE) and fp32 accumulation in v_mfma_f32_16x16x32_bf16; the dropped xl·wl term
// and the rounding of the low parts leave ~2^-16 relative error per product. Fragment mapping:
// B (activations) lane (g, c) holds, for k-block kb, slots 8g + j = features
// 32 kb + 16 (j >> 2) + 4 g + (j & 3) — exactly its fp32 accumulator registers x[2 kb + (j >> 2)][j & 3]
// — so layer outputs feed the next layer unchanged; the host stores the weights with their input
// columns in the same slot order (mpn/fold.py::bf16_pack).
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void split_bf16(const float (&x)[4][4], bf16x8_t (&hi)[2], bf16x8_t (&lo)[2]) {
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float f = x[2 * kb + (j >> 2)][j & 3];
      const __bf16 h = (__bf16)f;
      hi[kb][j] = h;
      lo[kb][j] = (__bf16)(f - (float)h);
    }
}

// acc[ob] += W[16 ob + i][.] · x, K = 64, W in LDS as interleaved bf16 rows of 2 LDW elements:
// [hi 64 | lo 64 | pad 16]. The row stride (LDW = 72 dwords, = 8 mod 64) keeps the fragment reads
// (row = lane & 15, 16 B at 8 (lane >> 4)) bank-conflict free for both parts (ds_read_b128 lane groups).
template <int OB>
__device__ __forceinline__ void gemm_bf3(const __bf16* W, const bf16x8_t (&hi)[2], const bf16x8_t (&lo)[2],
                                         float (&acc)[OB][4]) {
  const int lane = __lane_id(), i = lane & 15, g = lane >> 4;
#pragma unroll
  for (int ob = 0; ob < OB; ++ob) {
    f32x4 c = {acc[ob][0], acc[ob][1], acc[ob][2], acc[ob][3]};
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const int o = (16 * ob + i) * 2 * LDW + 32 * kb + 8 * g;
      const bf16x8_t ah = *reinterpret_cast<const bf16x8_t*>(W + o);
      const bf16x8_t al = *reinterpret_cast<const bf16x8_t*>(W + o + 64);
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, hi[kb], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, lo[kb], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, hi[kb], c, 0, 0, 0);
    }
    acc[ob][0] = c[0]; acc[ob][1] = c[1]; acc[ob][2] = c[2]; acc[ob][3] = c[3];
  }
}

// ---- f16x3 split precision (PREC 2, the default): with w' = 2^11 w split into f16 parts
// wh = f16(w'), wl = f16(w' - wh) (mpn/fold.py::split_pack "f16") and x split into xh = f16(x),
// xl = f16(x - xh), one fp32 accumulator takes 2^11 x·w ~= wl·xh + wh·xl + wh·xh on
// v_mfma_f32_16x16x32_f16 (the f16 products are exact in fp32). Each pair carries 22 bits of its
// operand (bf16x3: 16), so the dropped wl·xl term leaves ~2^-22 relative error per product:
// fp32-level logits at trained-checkpoint magnitudes, where bf16x3 misses the 1e-4 bar
// (tests/test_gpu_mpn.py::test_trained_scale).
// Scale domain: the accumulators are never rescaled. Every GEMM output of the edge passes, and the
// per-edge state r, Q0 and the node table that feed them, live in the 2^11 domain (dom<PREC>());
// the split of a fragment folds the 2^-11 back in (v_fma_mix with a scale operand), biases and
// attention rows come pre-scaled in the weight image, and results leave the domain once, where the
// segments are normalised. Range: f16 holds |x| < 65504, so an item (edge / node column) whose (scaled)
// values reach 2^14 is split at x·2^-k, the smallest such power of two that brings it under 2^14, and the
// GEMMs rescale that item's accumulator column by 2^k (exact; rare: a uniform branch selects the rescaling
// body when any item of the wave needs it, and the other items keep factor 1, so their precision does not
// depend on their neighbours); the host keeps |w'| <= 65504. Same fragment slot order and LDS row layout
// as bf16x3.
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
constexpr float F16_BIG = 16384.0f, F16_DOWN = 1.0f / 65536.0f;
template <int PREC>
__host__ __device__ constexpr float dom() { return PREC == 2 ? 2048.0f : 1.0f; }
template <int PREC>
__host__ __device__ constexpr float dom_inv() { return PREC == 2 ? 1.0f / 2048.0f : 1.0f; }

// f16 pair of (s x0, s x1): hi = f16(s x), lo = f16(s x - hi) -- v_fma_mix: exact fp32 fma, one rounding.
// s is a per-lane factor (a VGPR operand): the item's power-of-two range scale folded into the split.
__device__ __forceinline__ void split_pair(float x0, float x1, float s, uint32_t& hi, uint32_t& lo) {
  asm("v_fma_mixlo_f16 %0, %2, %4, 0\n\t"
      "v_fma_mixhi_f16 %0, %3, %4, 0\n\t"
      "v_fma_mixlo_f16 %1, %2, %4, -%0 op_sel_hi:[0,0,1]\n\t"
      "v_fma_mixhi_f16 %1, %3, %4, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
      : "=&v"(hi), "=&v"(lo)
      : "v"(x0), "v"(x1), "v"(s));
}

__device__ __forceinline__ float frag_absmax(const float (&x)[4][4]) {
  float m = 0.0f;
#pragma unroll
  for (int b = 0; b < 4; ++b) m = fmaxf(m, fmaxf(fmaxf(fabsf(x[b][0]), fabsf(x[b][1])), fmaxf(fabsf(x[b][2]), fabsf(x[b][3]))));
  return m;
}

// Range scale of one item (the lane column c = lane & 15; its 64 features sit in lanes c, c+16, c+32, c+48):
// the largest power of two 2^-k, k >= 0, that brings the item's max |s x| under 2^14 -- 1 for every item
// already in range, so an item's precision never depends on the other items of the wave. m = item max
// (partial: this lane's values; the cross-lane max is taken here).
__device__ __forceinline__ float f16_item_scale(float m, float s) {
  m = xmax_rows(m);
  m *= s;
  if (m < F16_BIG) return 1.0f;
  if (!(m <= 3.4028235e38f)) return F16_DOWN;      // inf / NaN: any scale (the result is not finite anyway)
  int e;
  frexpf(m, &e);                                   // 2^(e-1) <= m < 2^e, e >= 15
  return ldexpf(1.0f, 14 - e);                     // m 2^(14-e) < 2^14, and >= 2^13
}

// largest value of a fragment known to hold no negative value (after relu1): non-negative floats order
// as their bit patterns, so one v_max3_i32 chain (no fabs, no canonicalising moves); a NaN with a clear
// sign bit sorts above +inf and still reaches the range check as a NaN
__device__ __forceinline__ float frag_max_nonneg(const float (&x)[4][4]) {
  int m = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b)
    m = max(m, max(max(__float_as_int(x[b][0]), __float_as_int(x[b][1])), max(__float_as_int(x[b][2]), __float_as_int(x[b][3]))));
  return __int_as_float(m);
}

// split of the fragment s·x (s a power of two); returns the wave's range flag. When it is set, `sc` is each
// item's range factor (the parts hold s·x·sc and a GEMM over them rescales the item's column by 1/sc); else 1.
// NONNEG: x holds no negative value (relu1 output)
// extra: a per-lane factor in (0, 1] folded into the parts (the parts then hold s x sc extra; one rounding, in
// the split: the attention weight of the edge, PE_FOLD in edge_step_kernel); the range check stays on s x.
template <bool NONNEG = false>
__device__ __forceinline__ bool split_f16(const float (&x)[4][4], float s, f16x8_t (&hi)[2], f16x8_t (&lo)[2],
                                          float& sc, float extra = 1.0f) {
  const float m = NONNEG ? frag_max_nonneg(x) : frag_absmax(x);
  const bool big = __any(!(m * s < F16_BIG));
  sc = big ? f16_item_scale(m, s) : 1.0f;
  const float ss = s * sc * extra;
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    uint32_t h[4], l[4];
#pragma unroll
    for (int d = 0; d < 4; ++d)
      split_pair(x[2 * kb + (d >> 1)][2 * (d & 1)], x[2 * kb + (d >> 1)][2 * (d & 1) + 1], ss, h[d], l[d]);
    const u32x4_t hv = {h[0], h[1], h[2], h[3]}, lv = {l[0], l[1], l[2], l[3]};
    hi[kb] = __builtin_bit_cast(f16x8_t, hv);
    lo[kb] = __builtin_bit_cast(f16x8_t, lv);
  }
  return big;
}

// acc[ob] += W'[16 ob + i][.] · x (K = 64) in the 2^11 domain: acc raw in, raw out. W = interleaved f16
// rows [wh 64 | wl 64 | pad] (gemm_bf3 layout); BIG: the split carried the item factor sc (a power of two:
// the accumulator is scaled by sc on the way in and by 1/sc on the way out, both exact)
template <int OB, bool BIG>
__device__ __forceinline__ void gemm_h3_body(const _Float16* W, const f16x8_t (&hi)[2],
                                             const f16x8_t (&lo)[2], float sc, float (&acc)[OB][4]) {
  const int lane = __lane_id(), i = lane & 15, g = lane >> 4;
  const float isc = BIG ? 1.0f / sc : 1.0f;
#pragma unroll
  for (int ob = 0; ob < OB; ++ob) {
    f32x4 c = {acc[ob][0], acc[ob][1], acc[ob][2], acc[ob][3]};
    if (BIG) c *= sc;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const int o = (16 * ob + i) * 2 * LDW + 32 * kb + 8 * g;
      const f16x8_t ah = *reinterpret_cast<const f16x8_t*>(W + o);
      const f16x8_t al = *reinterpret_cast<const f16x8_t*>(W + o + 64);
      c = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, hi[kb], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, lo[kb], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, hi[kb], c, 0, 0, 0);
    }
    if (BIG) c *= isc;
    acc[ob][0] = c[0]; acc[ob][1] = c[1]; acc[ob][2] = c[2]; acc[ob][3] = c[3];
  }
}

// the range flag picks one of two whole GEMM bodies (a uniform branch: the common body has no rescaling)
template <int OB>
__device__ __forceinline__ void gemm_h3(const _Float16* W, const f16x8_t (&hi)[2], const f16x8_t (&lo)[2],
                                        bool big, float sc, float (&acc)[OB][4]) {
  if (__builtin_expect(big, 0)) gemm_h3_body<OB, true>(W, hi, lo, sc, acc);
  else gemm_h3_body<OB, false>(W, hi, lo, 1.0f, acc);
}

// A GEMM input fragment prepared once for the precision (split parts), reusable by several GEMMs.
template <int PREC>
struct Frag {
  bf16x8_t bh[2], bl[2];
  f16x8_t hh[2], hl[2];
  bool big;
  float sc;   // f16x3, big: the item's range factor (split_f16)
};

// x in the precision's domain (dom<PREC>() x_true for f16x3): split for the GEMMs that read it
// (NONNEG: x is a relu1 output)
template <int PREC, bool NONNEG = false>
__device__ __forceinline__ void prep(const float (&x)[4][4], Frag<PREC>& f) {
  if constexpr (PREC == 1) split_bf16(x, f.bh, f.bl);
  else if constexpr (PREC == 2) f.big = split_f16<NONNEG>(x, dom_inv<PREC>(), f.hh, f.hl, f.sc);
}

// f16x3: x in the domain, split with the per-lane factor `extra` folded in (see split_f16)
template <bool NONNEG = false>
__device__ __forceinline__ void prep_f16_scaled(const float (&x)[4][4], Frag<2>& f, float extra) {
  f.big = split_f16<NONNEG>(x, dom_inv<2>(), f.hh, f.hl, f.sc, extra);
}

// x in the true domain (f16x3: split with scale 1)
template <int PREC>
__device__ __forceinline__ void prep_true(const float (&x)[4][4], Frag<PREC>& f) {
  if constexpr (PREC == 1) split_bf16(x, f.bh, f.bl);
  else if constexpr (PREC == 2) f.big = split_f16(x, 1.0f, f.hh, f.hl, f.sc);
}

// acc (domain) += W · x_true over one prepared fragment; W = the LDS image of the matrix
// (PREC 0: fp32 [out][LDW]; PREC 1 / 2: interleaved 16-bit rows [out][hi 64 | lo 64 | pad])
template <int PREC, int OB>
__device__ __forceinline__ void gemm_f(const void* W, const float (&x)[4][4], const Frag<PREC>& f, float (&acc)[OB][4]) {
  if constexpr (PREC == 0) gemm_frag<4, OB>(static_cast<const float*>(W), LDW, x, acc);
  else if constexpr (PREC == 1) gemm_bf3<OB>(static_cast<const __bf16*>(W), f.bh, f.bl, acc);
  else gemm_h3<OB>(static_cast<const _Float16*>(W), f.hh, f.hl, f.big, f.sc, acc);
}

// global [hi rows][lo rows] bf16 pack row `row` (< 2 rows_per_part) -> its place in an interleaved
// LDS image with rows of `ld` bf16 elements and parts of `part_len` elements
__device__ __forceinline__ int interleaved_slot(int row, int rows_per_part, int ld, int part_len) {
  const int part = row >= rows_per_part, r = row - part * rows_per_part;
  return r * ld + part * part_len;
}

// LDS row stride for a weight tile with in_pad columns: >= in_pad and = 8 (mod 64) dwords, so the
// fragment reads (row = lane & 15, 16 B at column 4 * (lane >> 4)) are bank-conflict free.
__host__ __device__ constexpr int lds_stride(int in_pad) { return (in_pad - 8 + 63) / 64 * 64 + 8; }

// LDS image of the edge embedding: n layers + the Q0 tile, then biases (floats).
//   PREC 0: each layer [out_pad][stride] fp32, in_pad = 16 kb
//   PREC 1: each layer bf16 hi [out_pad][stride] then lo [out_pad][stride], in_pad = 32 kb; the
//           global pack (pemp_mpn_weights.emb_bf) is [2][out_pad][in_pad] per layer, concatenated.
struct EmbedLayout {
  int n, prec, w_off[5], stride[5], kb[5], ob[5], b_off[5], relu[5], g_off[5], total;
};

// interleaved bf16 row [hi in_pad | lo in_pad | pad 16] (elements): in_pad + 8 dwords, = 8 * odd
// (mod 64) for in_pad = 32 kb, which keeps the ds_read_b128 fragment reads conflict free
__host__ __device__ constexpr int lds_stride_bf(int in_pad) { return 2 * in_pad + 16; }

// (from the layers' dimensions: a constant expression for the published shape, embed_layout_published)
__host__ __device__ constexpr EmbedLayout embed_layout_dims(int n, const int* in_dim, const int* out_dim, const int* relu,
                                                            int prec) {
  EmbedLayout L{};
  L.n = n;
  L.prec = prec;
  int off = 0, goff = 0;
  for (int l = 0; l <= L.n; ++l) {
    const int in = l < L.n ? in_dim[l] : 64, out = l < L.n ? out_dim[l] : 64;
    L.ob[l] = (out + 15) / 16;
    L.relu[l] = l < L.n ? relu[l] : 0;
    L.w_off[l] = off;
    if (prec != PEMP_PREC_FP32) {
      L.kb[l] = (in + 31) / 32;
      L.stride[l] = lds_stride_bf(32 * L.kb[l]);
      off += 16 * L.ob[l] * L.stride[l] / 2;             // interleaved hi | lo rows, stride bf16 elements
      L.g_off[l] = goff;
      goff += 2 * 16 * L.ob[l] * 32 * L.kb[l];
    } else {
      L.kb[l] = (in + 15) / 16;
      L.stride[l] = lds_stride(16 * L.kb[l]);
      off += 16 * L.ob[l] * L.stride[l];
    }
  }
  for (int l = 0; l <= L.n; ++l) {
    L.b_off[l] = off;
    off += 16 * L.ob[l];
  }
  L.total = off;
  return L;
}

static EmbedLayout embed_layout(const pemp_mlp& m, int prec) {
  int in[4] = {}, out[4] = {}, relu[4] = {};
  const int n = m.n_layers < 4 ? m.n_layers : 4;   // (mlp_ok: <= 4 layers)
  for (int l = 0; l < n; ++l) {
    in[l] = m.layer[l].in_dim;
    out[l] = m.layer[l].out_dim;
    relu[l] = m.layer[l].relu;
  }
  return embed_layout_dims(n, in, out, relu, prec);
}

// the split-precision layout of the published embedding (A <= 32 -> 32 -> 64 -> 64 -> 64): what embed_layout gives for
// every model that passes embed_fixed_shape, known at compile time (the fused first pass, edge_step_kernel STAGE_FIRST)
__host__ __device__ constexpr EmbedLayout embed_layout_published() {
  constexpr int in[4] = {32, 32, 64, 64}, out[4] = {32, 64, 64, 64}, relu[4] = {1, 1, 1, 0};
  return embed_layout_dims(4, in, out, relu, PEMP_PREC_F16X3);
}

// One Linear (+ReLU) on fragments, weights and bias in LDS, runtime block counts <= 4.
__device__ __forceinline__ void layer_lds(const float* __restrict__ W, int ldw, const float* __restrict__ bias, int KB,
                                          int OB, int relu, const float (&in)[4][4], float (&out)[4][4]) {
  const int lane = __lane_id(), i = lane & 15, g = lane >> 4;
#pragma unroll
  for (int ob = 0; ob < 4; ++ob) {
    if (ob < OB) {
      const float4 bb = ld4(bias + 16 * ob + 4 * g);
      f32x4 c = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) {
        if (mb < KB) {
          const float4 w = ld4(W + (16 * ob + i) * ldw + 16 * mb + 4 * g);
          c = mfma4(w.x, in[mb][0], c);
          c = mfma4(w.y, in[mb][1], c);
          c = mfma4(w.z, in[mb][2], c);
          c = mfma4(w.w, in[mb][3], c);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) out[ob][r] = relu ? relu1(c[r]) : c[r];
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) out[ob][r] = 0.0f;
    }
  }
}

// split-precision variants (PREC 1 bf16x3, PREC 2 f16x3): W = interleaved rows
// [16 OB][hi 32 KB32 | lo 32 KB32 | pad], stride ldw; KB32 (<= 2) k-blocks of 32 inputs. True-domain
// input and output (f16x3: the bias enters scaled by 2^11, the result leaves scaled by 2^-11).
template <int PREC>
__device__ __forceinline__ void layer_lds_p(const uint16_t* __restrict__ W, int ldw, const float* __restrict__ bias,
                                            int KB32, int OB, int relu, const float (&in)[4][4], float (&out)[4][4]) {
  const int lane = __lane_id(), i = lane & 15, g = lane >> 4;
  bf16x8_t hb[2], lb[2];
  f16x8_t hh[2], lh[2];
  float s_in = 1.0f, s_out = 1.0f;
  if (PREC == 1) {
    split_bf16(in, hb, lb);
  } else {
    float sc;
    split_f16(in, 1.0f, hh, lh, sc);              // sc: the item's range factor (1 in range)
    s_in = 2048.0f * sc;
    s_out = (1.0f / 2048.0f) / sc;
  }
  const int lo_off = 32 * KB32;                 // interleaved rows: [hi | lo | pad]
#pragma unroll
  for (int ob = 0; ob < 4; ++ob) {
    if (ob < OB) {
      const float4 bb = ld4(bias + 16 * ob + 4 * g);
      f32x4 c = {bb.x * s_in, bb.y * s_in, bb.z * s_in, bb.w * s_in};
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        if (kb < KB32) {
          const int o = (16 * ob + i) * ldw + 32 * kb + 8 * g;
          if (PREC == 1) {
            const bf16x8_t ah = *reinterpret_cast<const bf16x8_t*>(W + o);
            const bf16x8_t al = *reinterpret_cast<const bf16x8_t*>(W + o + lo_off);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, hb[kb], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, lb[kb], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, hb[kb], c, 0, 0, 0);
          } else {
            const f16x8_t ah = *reinterpret_cast<const f16x8_t*>(W + o);
            const f16x8_t al = *reinterpret_cast<const f16x8_t*>(W + o + lo_off);
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, hh[kb], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, lh[kb], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, hh[kb], c, 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = c[r] * s_out;
        out[ob][r] = relu ? fmaxf(v, 0.0f) : v;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) out[ob][r] = 0.0f;
    }
  }
}

// ---- buffer-resource memory ops of the edge pass: a per-array SGPR descriptor and 32-bit lane offsets
// (no 64-bit per-lane pointers to keep live across the tile loop; reads past the array end return 0)
typedef __amdgpu_buffer_rsrc_t rsrc_t;
typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
constexpr int RSRC_DW3 = 0x00020000;   // raw buffer, gfx950
// (32-bit size: a 64-bit clamp here makes hipcc treat the descriptor as divergent and wrap every access
// in a readfirstlane waterfall loop; the host keeps the arrays below 2^31 bytes)
__device__ __forceinline__ rsrc_t make_rsrc(const void* p, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, RSRC_DW3);
}
__device__ __forceinline__ float4 bld4(rsrc_t rs, int voff, int soff = 0) {
  const u32x4v v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0);
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
__device__ __forceinline__ int bld1(rsrc_t rs, int voff) { return (int)__builtin_amdgcn_raw_buffer_load_b32(rs, voff, 0, 0); }
constexpr int OOB_VOFF = (int)0x80000000u;   // buffer offset past every descriptor's size: store dropped
__device__ __forceinline__ void bst4(rsrc_t rs, int voff, float a, float b, float c, float d) {
  const u32x4v v = {__float_as_uint(a), __float_as_uint(b), __float_as_uint(c), __float_as_uint(d)};
  __builtin_amdgcn_raw_buffer_store_b128(v, rs, voff, 0, 0);
}

// edge_attr row of the tile's edge (lane column c): features 16 mb + 4 g + r < A. Every load is
// unconditional (clamped column; the value masked afterwards) so that all of them issue back to back
// under one wait -- a guard per element (or per block) made the compiler wait for each one.
__device__ __forceinline__ void load_edge_attr(rsrc_t rs_ea, int A, int o, float (&x)[4][4]) {
  const int g = __lane_id() >> 4;
  const int row = o * A * 4;   // byte offset of the row (32-bit: the host keeps E * A * 4 < 2^31)
  float v[4][4];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int r = 0; r < 4; ++r)   // 16-feature blocks past A are not loaded (uniform; A = 19 reads 2 of 4)
      v[mb][r] = 16 * mb < A ? __int_as_float(bld1(rs_ea, row + 4 * min(16 * mb + 4 * g + r, A - 1))) : 0.0f;
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int r = 0; r < 4; ++r) x[mb][r] = 16 * mb + 4 * g + r < A ? v[mb][r] : 0.0f;
}

// the first 32 features of the tile's edge_attr rows (A <= 32: the fixed published shape), raw and unmasked,
// issued one tile ahead of their use (ea_mask). g: the lane's row group (a caller inside a register-tight loop passes
// it re-derived per trip, so that the eight column terms are recomputed instead of kept live or spilled)
__device__ __forceinline__ void load_edge_attr32(rsrc_t rs_ea, int A, int o, float (&v)[2][4], int g = __lane_id() >> 4) {
  const int row = o * A * 4;
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int r = 0; r < 4; ++r) v[mb][r] = __int_as_float(bld1(rs_ea, row + 4 * min(16 * mb + 4 * g + r, A - 1)));
}
__device__ __forceinline__ void ea_mask(int A, const float (&v)[2][4], float (&x)[4][4], int g = __lane_id() >> 4) {
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int r = 0; r < 4; ++r) x[mb][r] = (mb < 2 && 16 * mb + 4 * g + r < A) ? v[mb < 2 ? mb : 0][r] : 0.0f;
}

// embedding MLP then the Q0 layer on one tile: in x = edge_attr; out x = e_init, y = Q0 (+ b1)
template <int PREC>
__device__ __forceinline__ void embed_tile(const float* smz, const EmbedLayout& Lo, float (&x)[4][4], float (&y)[4][4]) {
  // layers alternate x -> y -> x ...; the result ends in x, then Q0 -> y
  for (int l = 0; l <= Lo.n; ++l) {
    const float* W = smz + Lo.w_off[l];
    const float* bias = smz + Lo.b_off[l];
    const int relu = Lo.relu[l];
    const bool odd = (l & 1) != 0;
    if (l == Lo.n && (Lo.n & 1)) {               // the embedding result is in y: move it to x
#pragma unroll
      for (int ob = 0; ob < 4; ++ob)
#pragma unroll
        for (int r = 0; r < 4; ++r) x[ob][r] = y[ob][r];
    }
    const bool to_y = l == Lo.n || !odd;
    if (PREC == 0) {
      if (to_y) layer_lds(W, Lo.stride[l], bias, Lo.kb[l], Lo.ob[l], relu, x, y);
      else layer_lds(W, Lo.stride[l], bias, Lo.kb[l], Lo.ob[l], relu, y, x);
    } else {
      const uint16_t* Wb = reinterpret_cast<const uint16_t*>(W);
      if (to_y) layer_lds_p<PREC>(Wb, Lo.stride[l], bias, Lo.kb[l], Lo.ob[l], relu, x, y);
      else layer_lds_p<PREC>(Wb, Lo.stride[l], bias, Lo.kb[l], Lo.ob[l], relu, y, x);
    }
  }
}

// The published edge embedding ([J+2 <= 32] -> 32 -> 64 -> 64 -> 64, then Q0 64 -> 64) with the block
// counts known at compile time: straight-line layers (the runtime-shaped loop above keeps its loop state,
// per-layer guards and LDS offsets live and spilled). Split precisions only.
// DOM (the Q0 layer): the output stays in the f16x3 domain (x 2^11, as the edge passes keep Q0 and R0) and
// the input's split is handed back for the R0 GEMM on the same e_init
template <int PREC, int KB32, int OB, bool DOM = false>
__device__ __forceinline__ void layer_fixed(const float* smz, const EmbedLayout& Lo, int l, const float (&in)[4][4],
                                            float (&out)[4][4], Frag<PREC>* split_out = nullptr) {
  const uint16_t* W = reinterpret_cast<const uint16_t*>(smz + Lo.w_off[l]);
  const float* bias = smz + Lo.b_off[l];
  const int ldw = Lo.stride[l], relu = Lo.relu[l];
  const int lane = __lane_id(), i = lane & 15, g = lane >> 4;
  bf16x8_t hb[2], lb[2];
  f16x8_t hh[2], lh[2];
  float s_in = 1.0f, s_out = 1.0f;
  if (PREC == 1) {
    split_bf16(in, hb, lb);
  } else {
    float sc;
    const bool big = split_f16(in, 1.0f, hh, lh, sc);   // sc: the item's range factor (1 in range)
    s_in = 2048.0f * sc;
    s_out = (DOM ? 1.0f : 1.0f / 2048.0f) / sc;
    if constexpr (PREC == 2) {
      if (split_out) {
        split_out->hh[0] = hh[0]; split_out->hh[1] = hh[1];
        split_out->hl[0] = lh[0]; split_out->hl[1] = lh[1];
        split_out->big = big;
        split_out->sc = sc;
      }
    }
  }
  if constexpr (PREC == 1) {
    if (split_out) {
      split_out->bh[0] = hb[0]; split_out->bh[1] = hb[1];
      split_out->bl[0] = lb[0]; split_out->bl[1] = lb[1];
    }
  }
  constexpr int lo_off = 32 * KB32;
#pragma unroll
  for (int ob = 0; ob < 4; ++ob) {
    if (ob < OB) {
      const float4 bb = ld4(bias + 16 * ob + 4 * g);
      f32x4 c = {bb.x * s_in, bb.y * s_in, bb.z * s_in, bb.w * s_in};
#pragma unroll
      for (int kb = 0; kb < KB32; ++kb) {
        const int o = (16 * ob + i) * ldw + 32 * kb + 8 * g;
        if (PREC == 1) {
          const bf16x8_t ah = *reinterpret_cast<const bf16x8_t*>(W + o);
          const bf16x8_t al = *reinterpret_cast<const bf16x8_t*>(W + o + lo_off);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, hb[kb], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, lb[kb], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, hb[kb], c, 0, 0, 0);
        } else {
          const f16x8_t ah = *reinterpret_cast<const f16x8_t*>(W + o);
          const f16x8_t al = *reinterpret_cast<const f16x8_t*>(W + o + lo_off);
          c = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, hh[kb], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, lh[kb], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, hh[kb], c, 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = c[r] * s_out;
        out[ob][r] = relu ? fmaxf(v, 0.0f) : v;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) out[ob][r] = 0.0f;
    }
  }
}

// f16x3 split of the first KB k-blocks (32 features each) of a fragment: split_f16 over 16 KB values per lane instead
// of 32 (the k-blocks past KB hold the zero padding of a narrower layer input and are not read)
template <int KB, bool NONNEG>
__device__ __forceinline__ bool split_f16_kb(const float (&x)[4][4], float s, f16x8_t (&hi)[2], f16x8_t (&lo)[2],
                                             float& sc) {
  float m;
  if constexpr (NONNEG) {
    int mi = 0;
#pragma unroll
    for (int b = 0; b < 2 * KB; ++b)
      mi = max(mi, max(max(__float_as_int(x[b][0]), __float_as_int(x[b][1])), max(__float_as_int(x[b][2]), __float_as_int(x[b][3]))));
    m = __int_as_float(mi);
  } else {
    m = 0.0f;
#pragma unroll
    for (int b = 0; b < 2 * KB; ++b)
      m = fmaxf(m, fmaxf(fmaxf(fabsf(x[b][0]), fabsf(x[b][1])), fmaxf(fabsf(x[b][2]), fabsf(x[b][3]))));
  }
  const bool big = __any(!(m * s < F16_BIG));
  sc = big ? f16_item_scale(m, s) : 1.0f;
  const float ss = s * sc;
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    uint32_t h[4], l[4];
#pragma unroll
    for (int d = 0; d < 4; ++d)
      split_pair(x[2 * kb + (d >> 1)][2 * (d & 1)], x[2 * kb + (d >> 1)][2 * (d & 1) + 1], ss, h[d], l[d]);
    const u32x4_t hv = {h[0], h[1], h[2], h[3]}, lv = {l[0], l[1], l[2], l[3]};
    hi[kb] = __builtin_bit_cast(f16x8_t, hv);
    lo[kb] = __builtin_bit_cast(f16x8_t, lv);
  }
  return big;
}

// One layer of the fixed embedding in the f16x3 domain: input x 2^11 (IN_DOM; the first layer's edge_attr is true),
// output x 2^11, the biases staged x 2^11 in LDS (edge_embed_kernel FIXED) -- so no per-value scaling on the way in
// or out, only where an item's range factor applies (BIG, a uniform branch to a second body). The values are
// bitwise 2^11 times those of layer_fixed (power-of-two scalings are exact). ReLU and the sign of the input are
// compile-time (NONNEG: the input is a ReLU output, so its range max is one integer max3 chain).
template <int KB32, int OB, bool RELU, bool NONNEG, bool BIG>
__device__ __forceinline__ void layer_h3_body(const _Float16* W, int ldw, const float* bias, const f16x8_t (&hh)[2],
                                              const f16x8_t (&lh)[2], float sc, float (&out)[4][4]) {
  const int lane = __lane_id(), i = lane & 15, g = lane >> 4;
  constexpr int lo_off = 32 * KB32;
  const float isc = BIG ? 1.0f / sc : 1.0f;
#pragma unroll
  for (int ob = 0; ob < 4; ++ob) {
    if (ob < OB) {
      const float4 bb = ld4(bias + 16 * ob + 4 * g);
      f32x4 c = {bb.x, bb.y, bb.z, bb.w};
      if (BIG) c *= sc;
#pragma unroll
      for (int kb = 0; kb < KB32; ++kb) {
        const int o = (16 * ob + i) * ldw + 32 * kb + 8 * g;
        const f16x8_t ah = *reinterpret_cast<const f16x8_t*>(W + o);
        const f16x8_t al = *reinterpret_cast<const f16x8_t*>(W + o + lo_off);
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, hh[kb], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, lh[kb], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, hh[kb], c, 0, 0, 0);
      }
      if (BIG) c *= isc;
#pragma unroll
      for (int r = 0; r < 4; ++r) out[ob][r] = RELU ? fmaxf(c[r], 0.0f) : c[r];
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) out[ob][r] = 0.0f;
    }
  }
}

template <int KB32, int OB, bool RELU, bool NONNEG, bool IN_DOM>
__device__ __forceinline__ void layer_h3(const float* smz, const EmbedLayout& Lo, int l, const float (&in)[4][4],
                                         float (&out)[4][4], Frag<2>* split_out = nullptr) {
  const _Float16* W = reinterpret_cast<const _Float16*>(smz + Lo.w_off[l]);
  const float* bias = smz + Lo.b_off[l];
  f16x8_t hh[2], lh[2];
  float sc;
  const bool big = split_f16_kb<KB32, NONNEG>(in, IN_DOM ? dom_inv<2>() : 1.0f, hh, lh, sc);
  if (split_out) {
    split_out->hh[0] = hh[0]; split_out->hh[1] = hh[1];
    split_out->hl[0] = lh[0]; split_out->hl[1] = lh[1];
    split_out->big = big;
    split_out->sc = sc;
  }
  if (__builtin_expect(big, 0)) layer_h3_body<KB32, OB, RELU, NONNEG, true>(W, Lo.stride[l], bias, hh, lh, sc, out);
  else layer_h3_body<KB32, OB, RELU, NONNEG, false>(W, Lo.stride[l], bias, hh, lh, 1.0f, out);
}

template <int PREC, bool COMP = false>
__device__ __forceinline__ void embed_tile_fixed(const float* smz, const EmbedLayout& Lo, float (&x)[4][4],
                                                 float (&y)[4][4], Frag<PREC>& fx) {
  if constexpr (PREC == 2 && COMP) {
    // composed (round 6): the last embedding layer has no ReLU, so e_init = W4 h3 + b4 is linear in h3 and
    // Q0 = W1_e_init e_init + b1 = (W1_e_init W4) h3 + (W1_e_init b4 + b1); likewise
    // R0 = Q0 + W1_e_cur e_init = ((W1_e_init + W1_e_cur) W4) h3 + (...). The products are formed once in fp64
    // (mpn/fold.py, pemp_mpn_weights.emb_comp_bf / emb_comp_b) and staged in slots 3 (Q0) and 4 (R0): e_init is
    // never computed, one 64x64 GEMM and one split per tile fewer
    layer_h3<1, 2, true, false, false>(smz, Lo, 0, x, y);   // A -> 32
    layer_h3<1, 4, true, true, true>(smz, Lo, 1, y, x);     // 32 -> 64
    layer_h3<2, 4, true, true, true>(smz, Lo, 2, x, y);     // 64 -> 64 (h3 in y, a ReLU output)
    layer_h3<2, 4, false, true, true>(smz, Lo, 3, y, x, &fx);   // Q0 in x (domain), h3's split in fx
  } else if constexpr (PREC == 2) {   // every activation in the 2^11 domain (edge_attr in: true values)
    layer_h3<1, 2, true, false, false>(smz, Lo, 0, x, y);   // A -> 32
    layer_h3<1, 4, true, true, true>(smz, Lo, 1, y, x);     // 32 -> 64
    layer_h3<2, 4, true, true, true>(smz, Lo, 2, x, y);     // 64 -> 64
    layer_h3<2, 4, false, true, true>(smz, Lo, 3, y, x);    // 64 -> 64  (e_init in x)
    layer_h3<2, 4, false, false, true>(smz, Lo, 4, x, y, &fx);   // Q0 = W1_e_init e_init + b1, e_init's split
  } else {
    layer_fixed<PREC, 1, 2>(smz, Lo, 0, x, y);   // A -> 32
    layer_fixed<PREC, 1, 4>(smz, Lo, 1, y, x);   // 32 -> 64
    layer_fixed<PREC, 2, 4>(smz, Lo, 2, x, y);   // 64 -> 64
    layer_fixed<PREC, 2, 4>(smz, Lo, 3, y, x);   // 64 -> 64  (e_init in x)
    layer_fixed<PREC, 2, 4, true>(smz, Lo, 4, x, y, &fx);   // Q0 = W1_e_init e_init + b1 (domain), e_init's split
  }
}

// the layout embed_tile_fixed assumes (ReLU after the first three embedding layers, none after the last and Q0)
static bool embed_fixed_shape(const EmbedLayout& L) {
  static const int kb[5] = {1, 1, 2, 2, 2}, ob[5] = {2, 4, 4, 4, 4}, relu[5] = {1, 1, 1, 0, 0};
  if (L.prec == PEMP_PREC_FP32 || L.n != 4) return false;
  for (int l = 0; l < 5; ++l)
    if (L.kb[l] != kb[l] || L.ob[l] != ob[l] || (L.relu[l] != 0) != (relu[l] != 0)) return false;
  return true;
}
// the composed form of the fixed f16x3 embedding (embed_tile_fixed COMP) runs when the caller supplied its packs
static bool embed_composed(const EmbedLayout& L, int prec, const pemp_mpn_weights& w) {
  return prec == PEMP_PREC_F16X3 && embed_fixed_shape(L) && w.emb_comp_bf && w.emb_comp_b;
}

// Stage one 64x64 edge-pass matrix into LDS (PREC 0: fp32 rows of LDW; PREC 1: interleaved bf16)
template <int PREC>
__device__ __forceinline__ void stage_tile64(float* dst, const float* w32, int64_t ld32, const uint16_t* wbf) {
  if (PREC == 0) {
    for (int idx = threadIdx.x; idx < D * 16; idx += blockDim.x) {
      const int row = idx >> 4, c4 = (idx & 15) * 4;
      *reinterpret_cast<float4*>(&dst[row * LDW + c4]) = ld4(w32 + row * ld32 + c4);
    }
  } else {
    __bf16* db = reinterpret_cast<__bf16*>(dst);
    for (int idx = threadIdx.x; idx < 2 * D * 8; idx += blockDim.x) {
      const int row = idx >> 3, c8 = (idx & 7) * 8;
      *reinterpret_cast<uint4*>(&db[interleaved_slot(row, D, 2 * LDW, D) + c8]) =
          *reinterpret_cast<const uint4*>(wbf + row * D + c8);
    }
  }
}

// The edge embedding's LDS image (every embedding layer, Q0's layer and W1_e_cur, biases x 2^11 for the fixed
// f16x3 layers): written by threads tid, tid + nthreads, ... into dst, which is the kernel's LDS or, once per weight
// set (pemp_mpn_edge_image, embed_image_kernel), a global buffer of embed_image_floats() floats that the kernel then
// copies with one LDS-DMA round instead of these loops' dependent global-load rounds (one or two per layer).
// comp_bf / comp_b (FIXED f16x3 only, the composed form of embed_tile_fixed): slots 3 and 4 hold the composed Q0 and
// R0 matrices and biases instead of the last embedding layer and Q0's layer, and the W1_e_cur tile is not staged.
template <int PREC, bool FIXED>
__device__ __forceinline__ void embed_stage(float* dst, int tid, int nthreads, const pemp_mlp& emb, const EmbedLayout& Lo,
                                            const uint16_t* __restrict__ emb_bf, const float* __restrict__ q0_w,
                                            const float* __restrict__ q0_b, const float* __restrict__ e1_w,
                                            const uint16_t* __restrict__ e1_bf, const uint16_t* __restrict__ comp_bf,
                                            const float* __restrict__ comp_b) {
  const bool comp = FIXED && PREC == 2 && comp_bf && comp_b;
  // W1_e_cur after the embedding image (stage_tile64's layout)
  float* d64 = dst + Lo.total;
  if (comp) {
  } else if (PREC == 0) {
    for (int idx = tid; idx < D * 16; idx += nthreads) {
      const int row = idx >> 4, c4 = (idx & 15) * 4;
      *reinterpret_cast<float4*>(&d64[row * LDW + c4]) = ld4(e1_w + row * D + c4);
    }
  } else {
    __bf16* db = reinterpret_cast<__bf16*>(d64);
    for (int idx = tid; idx < 2 * D * 8; idx += nthreads) {
      const int row = idx >> 3, c8 = (idx & 7) * 8;
      *reinterpret_cast<uint4*>(&db[interleaved_slot(row, D, 2 * LDW, D) + c8]) =
          *reinterpret_cast<const uint4*>(e1_bf + row * D + c8);
    }
  }
  for (int l = 0; l <= Lo.n; ++l) {
    const bool cl = comp && l >= Lo.n - 1;   // composed slot: 3 = Q0, 4 = R0 (64 x 64 each)
    const float* bsrc = cl ? comp_b + 64 * (l - (Lo.n - 1)) : l < Lo.n ? emb.layer[l].b : q0_b;
    const int rows = 16 * Lo.ob[l];
    if (PREC == 0) {
      const float* src = l < Lo.n ? emb.layer[l].w : q0_w;
      const int ip = 16 * Lo.kb[l], q4 = ip / 4;
      for (int idx = tid; idx < rows * q4; idx += nthreads) {
        const int row = idx / q4, c4 = (idx - row * q4) * 4;
        *reinterpret_cast<float4*>(&dst[Lo.w_off[l] + row * Lo.stride[l] + c4]) = ld4(src + row * ip + c4);
      }
    } else {
      const uint16_t* src = cl ? comp_bf + 2 * 64 * 64 * (l - (Lo.n - 1)) : emb_bf + Lo.g_off[l];
      const int ip = 32 * Lo.kb[l], q8 = ip / 8;
      __bf16* dstb = reinterpret_cast<__bf16*>(dst + Lo.w_off[l]);
      for (int idx = tid; idx < 2 * rows * q8; idx += nthreads) {   // hi rows, then lo rows
        const int row = idx / q8, c8 = (idx - row * q8) * 8;
        *reinterpret_cast<uint4*>(&dstb[interleaved_slot(row, rows, Lo.stride[l], ip) + c8]) =
            *reinterpret_cast<const uint4*>(src + row * ip + c8);
      }
    }
    // (the fixed f16x3 layers keep every activation in the 2^11 domain: their biases are staged scaled, exactly)
    const float bscale = (FIXED && PREC == 2) ? dom<2>() : 1.0f;
    for (int idx = tid; idx < rows; idx += nthreads) dst[Lo.b_off[l] + idx] = bsrc[idx] * bscale;
  }
}

__host__ __device__ inline int embed_image_floats(const EmbedLayout& Lo) { return (Lo.total + D * LDW + 3) & ~3; }

template <int PREC, bool FIXED>
__global__ __launch_bounds__(256) void embed_image_kernel(pemp_mlp emb, EmbedLayout Lo, const uint16_t* emb_bf,
                                                          const float* q0_w, const float* q0_b, const float* e1_w,
                                                          const uint16_t* e1_bf, const uint16_t* comp_bf,
                                                          const float* comp_b, float* img) {
  embed_stage<PREC, FIXED>(img, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256, emb, Lo, emb_bf, q0_w, q0_b, e1_w,
                           e1_bf, comp_bf, comp_b);
}
// floats of the composed image the kernel copies (no W1_e_cur tile)
__host__ __device__ constexpr int embed_comp_floats(const EmbedLayout& Lo) { return (Lo.total + 3) & ~3; }

// 16-byte LDS-DMA load per lane into the wave-contiguous LDS block at `l` (lane i -> l + 16 i bytes).
// (A non-template function: hipcc drops the host stub of a kernel template that calls the builtin
// directly.)
__device__ __forceinline__ void dma16(const float* g, float* l) {
  __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

// flat copy of `n` floats from global to LDS by LDS-DMA (copy_to_lds is the register form) (n multiple of 4, both ends 16-byte aligned): 1 KB per wave instruction,
// the block's waves interleaved, nothing held in registers and nothing waited for here, so the loads
// that follow overlap it; lds_drain() before the barrier that publishes it
__device__ inline void dma_to_lds(float* __restrict__ lds, const float* __restrict__ src, int n) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int pieces = n >> 8, tail = n - (pieces << 8);
  for (int k = wave; k < pieces; k += nw) dma16(src + 256 * k + 4 * lane, lds + 256 * k);
  if (tail && wave == nw - 1 && 4 * lane < tail)
    *reinterpret_cast<float4*>(&lds[256 * pieces + 4 * lane]) = ld4(src + 256 * pieces + 4 * lane);
}
__device__ __forceinline__ void lds_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Edge embedding (sorted order), the fallback of the fused first pass: e_init = MLP(edge_attr[orig]),
// Q0 = W1_e_init·e_init + b1 and R0 = Q0 + W1_e_cur·e_init (the first pass's layer-1 input).
// One 16-wave workgroup per CU, weights staged once in LDS (from the prebuilt image when there is one); a wave
// walks an equal share of the sorted positions in 16-edge tiles.
// FX: 0 runtime-shaped layers, 1 the fixed published shape, 2 the same composed (embed_tile_fixed COMP: f16x3 only,
// with the caller's composed packs)
template <int PREC, int FX>
__global__ __launch_bounds__(64 * EMB_WAVES) __attribute__((amdgpu_waves_per_eu(EMB_MIN_WAVES_EU, 8)))
void edge_embed_kernel(pemp_mlp emb, EmbedLayout Lo,
                                                                     const uint16_t* __restrict__ emb_bf,
                                                                     const float* __restrict__ ea, int A,
                                                                     const int* __restrict__ s_orig, int64_t E,
                                                                     const float* __restrict__ q0_w,
                                                                     const float* __restrict__ q0_b,
                                                                     const float* __restrict__ e1_w,
                                                                     const uint16_t* __restrict__ e1_bf,
                                                                     float* __restrict__ r0, float* __restrict__ q0,
                                                                     const int64_t* __restrict__ ne,
                                                                     const float* __restrict__ img,
                                                                     const uint16_t* __restrict__ comp_bf,
                                                                     const float* __restrict__ comp_b) {
  constexpr bool FIXED = FX >= 1, COMP = FX == 2;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  if (ne) E = ne[1];   // capacity mode: the device-side edge count
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  if (img) {
    dma_to_lds(sm, img, COMP ? embed_comp_floats(Lo) : embed_image_floats(Lo));
    lds_drain();
  } else {
    embed_stage<PREC, FIXED>(sm, threadIdx.x, 64 * EMB_WAVES, emb, Lo, emb_bf, q0_w, q0_b, e1_w, e1_bf,
                             COMP ? comp_bf : nullptr, COMP ? comp_b : nullptr);
  }
  __syncthreads();
  const int64_t gw = (int64_t)blockIdx.x * EMB_WAVES + wave, nw = (int64_t)gridDim.x * EMB_WAVES;
  const int first = __builtin_amdgcn_readfirstlane((int)(E * gw / nw));
  const int end = __builtin_amdgcn_readfirstlane((int)(E * (gw + 1) / nw));
  // buffer descriptors + 32-bit offsets: no 64-bit lane pointers live across the tile loop
  const rsrc_t rs_ea = make_rsrc(ea, (int)E * A * 4), rs_orig = make_rsrc(s_orig, (int)E * 4);
  const rsrc_t rs_q0 = make_rsrc(q0, (int)E * 256), rs_r0 = make_rsrc(r0, (int)E * 256);
  // original edge ids one tile ahead (the edge_attr gather of a tile then waits for one round trip, not two);
  // FIXED: ids two tiles ahead and the edge_attr rows themselves one tile ahead
  int o_next = first < end ? bld1(rs_orig, 4 * min(first + c, end - 1)) : 0;
  float ea_n[2][4];
  if (FIXED && first < end) {
    load_edge_attr32(rs_ea, A, o_next, ea_n);
    o_next = bld1(rs_orig, 4 * min(first + 16 + c, end - 1));
  }
  for (int base = first; base < end; base += 16) {
    int z = 0;
    asm volatile("" : "+s"(z));                  // keep the LDS fragment reads inside the loop
    const float* smz = sm + z;
    const int p = base + c;
    const bool valid = p < end;
    float x[4][4], y[4][4];
    if constexpr (FIXED) {
      ea_mask(A, ea_n, x);
      load_edge_attr32(rs_ea, A, o_next, ea_n);   // the next tile's rows (clamped ids past the range: harmless)
      o_next = bld1(rs_orig, 4 * min(base + 32 + c, end - 1));
    } else {
      const int o = o_next;
      o_next = bld1(rs_orig, 4 * min(base + 16 + c, end - 1));
      load_edge_attr(rs_ea, A, o, x);
    }
    Frag<PREC> fx;
    const int vo = valid ? p * 256 + 16 * g : OOB_VOFF;   // masked lanes: stores dropped
    if constexpr (COMP) {
      embed_tile_fixed<PREC, true>(smz, Lo, x, y, fx);   // x = Q0 (domain), y = h3, fx = h3's split
#pragma unroll
      for (int ob = 0; ob < 4; ++ob) bst4(rs_q0, vo + 64 * ob, x[ob][0], x[ob][1], x[ob][2], x[ob][3]);
      // R0 = W_r h3 + b_r (slot 4, bias staged x 2^11): its own accumulator, no dependence on Q0's
      const float* br = smz + Lo.b_off[4];
#pragma unroll
      for (int ob = 0; ob < 4; ++ob) {
        const float4 bb = ld4(br + 16 * ob + 4 * g);
        x[ob][0] = bb.x; x[ob][1] = bb.y; x[ob][2] = bb.z; x[ob][3] = bb.w;
      }
      gemm_f<PREC, 4>(smz + Lo.w_off[4], y, fx, x);
#pragma unroll
      for (int ob = 0; ob < 4; ++ob) bst4(rs_r0, vo + 64 * ob, x[ob][0], x[ob][1], x[ob][2], x[ob][3]);
      continue;
    }
    if constexpr (FIXED) {
      embed_tile_fixed<PREC>(smz, Lo, x, y, fx);   // x = e_init, y = Q0 in the domain, fx = e_init's split
    } else {
      embed_tile<PREC>(smz, Lo, x, y);             // x = e_init, y = Q0 (true values)
      if (PREC == 2) {                             // Q0 and R0 are kept in the f16x3 domain (x 2^11)
#pragma unroll
        for (int ob = 0; ob < 4; ++ob)
#pragma unroll
          for (int r = 0; r < 4; ++r) y[ob][r] *= dom<PREC>();
      }
      prep_true<PREC>(x, fx);
    }
#pragma unroll
    for (int ob = 0; ob < 4; ++ob) bst4(rs_q0, vo + 64 * ob, y[ob][0], y[ob][1], y[ob][2], y[ob][3]);
    gemm_f<PREC, 4>(smz + Lo.total, x, fx, y);    // R0 = Q0 + W1_e_cur · e_init
#pragma unroll
    for (int ob = 0; ob < 4; ++ob) bst4(rs_r0, vo + 64 * ob, y[ob][0], y[ob][1], y[ob][2], y[ob][3]);
  }
}

// ---------------------------------------------------------------------------------------------
// One message-passing iteration over all edges.
// ---------------------------------------------------------------------------------------------
struct EdgeStepArgs {
  int64_t N, E;
  int T, t_nt_ld;   // node-table row length = 128 + 64 T
  const int4* ranges;             // per (block, wave): first, end, source type (edge_ranges_fill)
  const int *s_src, *s_dst, *s_orig;
  const float *NT, *Q0, *r_cur;   // r = Q0 + W1_e_cur · e_cur (layer-1 input without the node terms)
  float* r_next;                  // r_next = Q0 + W1_e_cur · e' (middle passes)
  const float* img;               // edge-pass weight image, per type (edge_image_kernel)
  int64_t img_stride;             // floats per type
  float* agg;
  pemp_mlp head;                  // HEAD 2: generic edge head, weights in global memory
  float* edge_logits;
  int write_next;
  unsigned long long* stamps;   // diagnostic builds (-DPEMP_STAMPS) only: per-wave phase timestamps
  const int64_t* ne;            // capacity mode: device-side (N, E); N / E above are then the capacities
  int rec;                      // capacity mode: edge_logits is the base, the pass writes row rec (of E)
  // fused first pass (STAGE_FIRST): the edge_attr rows [E][A] and the composed embedding's prebuilt LDS image; the pass
  // computes R0 in registers instead of reading r_cur and writes the Q0 rows
  const float* ea;
  int A;
  const float* emb_img;
};

// Diagnostic phase timestamps (-DPEMP_STAMPS builds only; tools/edge_timeline.py): lane 0 of each
// wave stores s_memrealtime (100 MHz) into stamps[16 * global_wave + k].
#ifdef PEMP_STAMPS
// the edge pass `g_diag_stamp_pass` of every forward records the stamps (pemp_diag_stamps, after the kernels below;
// launch_edge_step / launch_edge_first set EdgeStepArgs::stamps from the pass index they are given)
static unsigned long long* g_diag_stamps = nullptr;
static int g_diag_stamp_pass = 0;
#define EDGE_STAMP(k)                                                                               \
  do {                                                                                              \
    if (a.stamps && lane == 0) {                                                                    \
      unsigned long long t_;                                                                        \
      asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                \
      a.stamps[16 * ((int64_t)blockIdx.x * NW + wave) + (k)] = t_;                                  \
    }                                                                                               \
  } while (0)
#else
#define EDGE_STAMP(k) \
  do {                \
  } while (0)
#endif

// ---- in-row (16-lane) DPP primitives: lane c = lane & 15 of every row holds edge c of the tile ----
constexpr int DPP_SHR1 = 0x111, DPP_SHR2 = 0x112, DPP_SHR4 = 0x114, DPP_SHR8 = 0x118;
constexpr int DPP_SHL1 = 0x101, DPP_SHL2 = 0x102, DPP_SHL4 = 0x104, DPP_SHL8 = 0x108, DPP_SHL15 = 0x10F;

// value of lane c -/+ k of the same row; lanes whose source is outside the row get `old`
template <int CTRL>
__device__ __forceinline__ float dppf(float v, float old) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ int dppi(int v, int old) {
  return __builtin_amdgcn_update_dpp(old, v, CTRL, 0xF, 0xF, false);
}

// Chunk structure of a tile: a chunk = the edges of one (target, type) segment inside the tile.
// d = distance to the chunk head, u = distance to the chunk tail.
struct Chunks {
  int d, u;
  bool head, tail;
};

// The chunk structure is static across the passes of a forward (it follows from the sorted target list and the tile
// origins of the range table), so it is not scanned out of the targets in every tile: edge_ranges_kernel leaves each
// edge's position in its (target, type) segment in the spare high byte of its s_dst entry (node ids stay below 2^23,
// pemp_mpn_forward's range check) -- bits 28-31 the distance to the segment's first edge, bits 24-27 the distance to
// its last, each clamped to 15, which loses nothing: a tile only needs min(pos, c) and min(rem, last lane - c).
constexpr int SDST_ID_BITS = 24, SDST_ID_MASK = (1 << SDST_ID_BITS) - 1;
constexpr int64_t MPN_MAX_NODES = 1ll << 23;   // (also keeps the passes' 32-bit byte offsets in range)
static_assert(MPN_MAX_NODES <= (1ll << SDST_ID_BITS), "node ids must leave the high byte of an s_dst entry free");
__device__ __forceinline__ int sdst_id(int e) { return e & SDST_ID_MASK; }
__device__ __forceinline__ int sdst_pack(int id, int pos, int rem) {
  return (id & SDST_ID_MASK) | (min(max(rem, 0), 15) << SDST_ID_BITS) | (int)((unsigned)min(max(pos, 0), 15) << 28);
}

// e = the lane's packed s_dst entry, c = its lane in the row, lastc = the tile's last lane inside the wave's range
// (uniform; 15 except in a range's last tile: a segment that runs on past the range end is cut there). Lanes past
// the range end (!valid) are singleton chunks.
__device__ __forceinline__ Chunks chunks_of(int e, int c, int lastc, bool valid) {
  const int pos = (int)((unsigned)e >> 28), rem = (e >> SDST_ID_BITS) & 15;
  Chunks k;
  k.d = valid ? min(pos, c) : 0;
  k.u = max(min(rem, lastc - c), 0);   // (lastc - c < 0 past the range end)
  k.head = k.d == 0;
  k.tail = k.u == 0;
  return k;
}

// segmented inclusive scans along the row (Hillis-Steele; step k adds lane c-k when it is in
// the same chunk, i.e. when d >= k)
template <int CTRL>
__device__ __forceinline__ float dpp0(float v) {   // lane c -/+ k of the row, 0 outside the row
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}

struct ScanMask {
  float m1, m2, m4, m8;   // 1.0f where d >= k
};

__device__ __forceinline__ ScanMask scan_mask(int d) {
  return {d >= 1 ? 1.0f : 0.0f, d >= 2 ? 1.0f : 0.0f, d >= 4 ? 1.0f : 0.0f, d >= 8 ? 1.0f : 0.0f};
}

// sum: one v_fmac_f32 with a DPP source per step
__device__ __forceinline__ float seg_sum(float v, const ScanMask& m) {
  v = fmaf(dpp0<DPP_SHR1>(v), m.m1, v);
  v = fmaf(dpp0<DPP_SHR2>(v), m.m2, v);
  v = fmaf(dpp0<DPP_SHR4>(v), m.m4, v);
  v = fmaf(dpp0<DPP_SHR8>(v), m.m8, v);
  return v;
}

__device__ __forceinline__ float seg_max(float v, int d) {
  float o;
  o = dppf<DPP_SHR1>(v, -INFINITY); v = fmaxf(v, d >= 1 ? o : -INFINITY);
  o = dppf<DPP_SHR2>(v, -INFINITY); v = fmaxf(v, d >= 2 ? o : -INFINITY);
  o = dppf<DPP_SHR4>(v, -INFINITY); v = fmaxf(v, d >= 4 ? o : -INFINITY);
  o = dppf<DPP_SHR8>(v, -INFINITY); v = fmaxf(v, d >= 8 ? o : -INFINITY);
  return v;
}

// every lane of a chunk gets the value at the chunk tail (v non-decreasing along the chunk); the PEMP_ASM_SCANS=0 path
[[maybe_unused]] __device__ __forceinline__ float seg_bcast_tail_max(float v, int u) {
  float o;
  o = dppf<DPP_SHL1>(v, -INFINITY); v = fmaxf(v, u >= 1 ? o : -INFINITY);
  o = dppf<DPP_SHL2>(v, -INFINITY); v = fmaxf(v, u >= 2 ? o : -INFINITY);
  o = dppf<DPP_SHL4>(v, -INFINITY); v = fmaxf(v, u >= 4 ? o : -INFINITY);
  o = dppf<DPP_SHL8>(v, -INFINITY); v = fmaxf(v, u >= 8 ? o : -INFINITY);
  return v;
}

__device__ __forceinline__ float readlane_f(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// ---- the segmented max in hand-placed DPP instructions (PEMP_ASM_SCANS, the default) ----
// hipcc turns every fmaxf of seg_max into a mov_dpp + cndmask + canonicalising max + max. Here: one v_max_f32_dpp
// (source lane outside the row: not written) + one v_cndmask on a lane mask per step; the chain is serial, with an
// s_nop 1 per step. hipcc inserts no hazard wait states in front of inline asm: an asm block that reads an MFMA result
// (or writes a register an MFMA still reads) right after the MFMA would see the stale value. The block therefore opens
// with the longest XDL -> VALU distance (19 wait states: a 16-pass MFMA) before its first VALU instruction ...
#define PEMP_XDL_GUARD "s_nop 7\n\ts_nop 7\n\ts_nop 4\n\t"
// ... and closes with the 2 VALU-write -> DPP-read wait states: the compiler does not see the asm's last writes
// either, and its next DPP read of one of them would otherwise read the stale value
#define PEMP_DPP_TAIL "s_nop 1\n\t"
#ifndef PEMP_ASM_SCANS
#define PEMP_ASM_SCANS 1
#endif
// (Round 6: the 17 segmented SUMS no longer have an asm form. Through round 5 a hand-placed v_fmac_f32_dpp block
// (seg_sum17_asm) summed them in the f16x3 attention passes. It computed the same bits as the compiler's scans on every
// lane, yet any instantiation that carried it outside that path (bf16x3) became timing-dependent across forwards, the
// same with the DPP moved onto a v_mov_b32 and a plain fmac, and no cause was found. In the default
// path it was worth <= 1 % of an edge pass (profiles/r06_asm_sums.md), so it was removed: no instantiation carries it.)
#if PEMP_ASM_SCANS
struct ChunkMasks {
  uint64_t f1, f2, f4, f8, b1, b2, b4, b8;   // lanes with d >= k (forward steps) / u >= k (backward steps)
};
__device__ __forceinline__ ChunkMasks chunk_masks(const Chunks& k) {
  return {__builtin_amdgcn_ballot_w64(k.d >= 1), __builtin_amdgcn_ballot_w64(k.d >= 2),
          __builtin_amdgcn_ballot_w64(k.d >= 4), __builtin_amdgcn_ballot_w64(k.d >= 8),
          __builtin_amdgcn_ballot_w64(k.u >= 1), __builtin_amdgcn_ballot_w64(k.u >= 2),
          __builtin_amdgcn_ballot_w64(k.u >= 4), __builtin_amdgcn_ballot_w64(k.u >= 8)};
}

// every lane of a chunk gets the chunk's maximum (forward segmented max, then the tail's value backwards)
__device__ __forceinline__ float chunk_max_asm(float v, const ChunkMasks& mk) {
  float t;
#define PEMP_MAXSTEP(ctl, m)                                                   \
  "s_nop 1\n\t"                                                                \
  "v_max_f32_dpp %1, %0, %0 " ctl " row_mask:0xf bank_mask:0xf\n\t"            \
  "v_cndmask_b32_e64 %0, %0, %1, %" #m "\n\t"
  asm(PEMP_XDL_GUARD PEMP_MAXSTEP("row_shr:1", 2) PEMP_MAXSTEP("row_shr:2", 3) PEMP_MAXSTEP("row_shr:4", 4)
      PEMP_MAXSTEP("row_shr:8", 5) PEMP_MAXSTEP("row_shl:1", 6) PEMP_MAXSTEP("row_shl:2", 7)
      PEMP_MAXSTEP("row_shl:4", 8) PEMP_MAXSTEP("row_shl:8", 9) PEMP_DPP_TAIL
      : "+v"(v), "=&v"(t)
      : "s"(mk.f1), "s"(mk.f2), "s"(mk.f4), "s"(mk.f8), "s"(mk.b1), "s"(mk.b2), "s"(mk.b4), "s"(mk.b8));
#undef PEMP_MAXSTEP
  return v;
}
#endif


// ---- edge-pass weight image --------------------------------------------------------------------
// The LDS image of one edge pass, prepared once per weight set in global memory (one block per source
// type t, edge_image_kernel / pemp_mpn_edge_image) and copied into LDS with 16-byte LDS-DMA loads:
//   common [W1_e_cur | W2 | W_t (message) | U_t (UPD only)]   64 x LDW floats each (PREC 0: fp32 rows;
//          PREC 1/2: interleaved 16-bit rows [hi 64 | lo 64 | pad], gemm_bf3)
//          vec [e2_b 64 | attention row t 64 | attention bias t | pad 3]
//   head   (published 64 -> 64 -> 32 -> 1 edge head) [L1 64 x LDW | L2 32 x LDW | b1 64 | b2 32 | w3 32 | b3 | pad 3]
// Middle passes copy the common part, the recorded (head) pass both.
constexpr int IMG_VEC = 2 * D + 4;
constexpr int IMG_HEAD = (D + 32) * LDW + D + 32 + 32 + 4;
__host__ __device__ constexpr int img_common(int upd) { return (3 + upd) * D * LDW + IMG_VEC; }
__host__ __device__ constexpr int img_stride(int upd, int head) { return img_common(upd) + (head ? IMG_HEAD : 0); }
// floats of one wave's piece record (edge_step_kernel: raw aggregate, running max, normaliser, pad)
constexpr int EDGE_PIECE_F = 68;
// static LDS of the fused first pass (edge_step_kernel STAGE_FIRST): the pass image, the composed embedding image in
// place of the row buffers, and the piece records
__host__ __device__ constexpr size_t edge_first_lds_bytes() {
  return (size_t)(img_common(1) + embed_comp_floats(embed_layout_published()) + 16 * 2 * EDGE_PIECE_F) * sizeof(float);
}

struct EdgeImgArgs {
  int T, prec, upd, head, aggr;
  const float *e1_w, *e2_w, *e2_b, *msg_w, *attn_w, *attn_bv, *upd_w;
  float attn_b;
  const uint16_t *e1_bf, *e2_bf, *msg_bf, *upd_bf, *head_bf;
  pemp_mlp head_mlp;
  float* img;
};

// one 64-row matrix block of the image: float `f` of row `row` (< rows), stride LDW
__device__ inline float img_matrix_elem(int prec, int row, int f, const float* w32, int64_t ld32, const uint16_t* w16,
                                        int rows16) {
  if (prec == PEMP_PREC_FP32) return f < D ? w32[row * ld32 + f] : 0.0f;
  // interleaved 16-bit row: floats 0..31 = hi pairs, 32..63 = lo pairs, 64..71 pad
  if (f >= 2 * (D / 2)) return 0.0f;
  const int part = f >= D / 2, e = 2 * (f - part * (D / 2));
  const uint16_t* src = w16 + (int64_t)part * rows16 * D + (int64_t)row * D + e;
  return __uint_as_float((uint32_t)src[0] | ((uint32_t)src[1] << 16));
}

__global__ __launch_bounds__(256) void edge_image_kernel(EdgeImgArgs a) {
  const int t = blockIdx.y, T = a.T;
  const int common = img_common(a.upd), total = img_stride(a.upd, a.head);
  // f16x3 keeps the pass's GEMM outputs x 2^11: biases enter scaled up, the rows that reduce e' or the
  // head's last hidden layer to a scalar scaled down (dom<2>)
  const float dm = a.prec == PEMP_PREC_F16X3 ? dom<2>() : 1.0f, di = 1.0f / dm;
  float* out = a.img + (int64_t)t * total;
  for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
    float v = 0.0f;
    if (idx < (3 + a.upd) * D * LDW) {
      const int m = idx / (D * LDW), r = idx - m * D * LDW, row = r / LDW, f = r - row * LDW;
      if (m == 0) v = img_matrix_elem(a.prec, row, f, a.e1_w, D, a.e1_bf, D);
      else if (m == 1) v = img_matrix_elem(a.prec, row, f, a.e2_w, D, a.e2_bf, D);
      else if (m == 2) v = img_matrix_elem(a.prec, row, f, a.msg_w + (int64_t)t * D * D, D, a.msg_bf + (int64_t)t * 2 * D * D, D);
      else v = img_matrix_elem(a.prec, row, f, a.upd_w + 64 * t, 64 * T, a.upd_bf ? a.upd_bf + (int64_t)t * 2 * D * D : nullptr, D);
    } else if (idx < common) {
      const int k = idx - (3 + a.upd) * D * LDW;
      if (k < D) v = a.e2_b[k] * dm;
      else if (k < 2 * D) v = a.aggr == PEMP_AGGR_ATTN ? a.attn_w[(a.attn_bv ? t * D : 0) + k - D] * di : 0.0f;
      else if (k == 2 * D) v = a.aggr == PEMP_AGGR_ATTN ? (a.attn_bv ? a.attn_bv[t] : a.attn_b) : 0.0f;
    } else {
      const int k = idx - common;
      const pemp_mlp& h = a.head_mlp;
      if (k < (D + 32) * LDW) {
        const int row = k / LDW, f = k - row * LDW;
        if (row < D) v = img_matrix_elem(a.prec, row, f, h.layer[0].w, D, a.head_bf, D);
        else v = img_matrix_elem(a.prec, row - D, f, h.layer[1].w, D, a.head_bf ? a.head_bf + 2 * D * D : nullptr, 32);
      } else {
        const int q = k - (D + 32) * LDW;
        if (q < D) v = h.layer[0].b[q] * dm;
        else if (q < D + 32) v = h.layer[1].b[q - D] * dm;
        else if (q < D + 64) v = h.layer[2].w[q - D - 32] * di;
        else if (q == D + 64) v = h.layer[2].b[0];
      }
    }
    out[idx] = v;
  }
}

// ---- one message-passing iteration over all edges -------------------------------------------------
// HEAD: 0 = no edge head, 1 = published head 64 -> 64 -> 32 -> 1 (ReLU, ReLU), 2 = generic pemp_mlp
// UPD 1 (linear aggregations with an update MLP): each message is multiplied by the type's update
// block U_t before aggregation, so agg holds U_t · agg[n, t] (the per-type term of update_mlp.0,
// layers.py:253-258) and the node update is a plain sum over types.
//
// Work split (balanced, no atomics): the edges of source type t (contiguous in the type-major
// order) are cut into equal workgroup ranges, each cut into NW equal wave ranges; every range
// boundary is moved forward to the next segment start, so each (target, type) segment is reduced
// by exactly one wave (edge_wave_range, computed once per forward into a table). A wave walks its
// range in 16-edge tiles; a segment that crosses a tile boundary is carried in registers.
// Memory pipeline per tile k: the r rows of tile k+1 (the only per-edge stream besides Q0) are in
// flight as LDS-DMA loads into the wave's 4 KB buffer (XOR-swizzled by row: conflict-free reads)
// while tile k computes; Q0 rows and the node-table gathers of tile k are issued before that DMA,
// so waiting for them never waits for it; the indices run two tiles ahead.
// PREC: 0 = exact fp32 MFMA (v_mfma_f32_16x16x4_f32), 1 = bf16x3, 2 = f16x3 (gemm_bf3 / gemm_h3).
// STAGE_FIRST (with STAGE_MID; f16x3, attention, UPD, no head, the composed published embedding): the first pass with
// the edge embedding fused in. Per tile it runs edge_embed_kernel<2, 2>'s arithmetic on the tile's edge_attr rows --
// the same device functions in the same order, so Q0 and R0 have the same bits -- uses R0 as the tile's r, stores Q0
// for the later passes and keeps it in registers for its own r_next. R0 never reaches memory. No LDS-DMA row buffer:
// its LDS holds the composed embedding image instead, and every memory wait is the compiler's.
enum { STAGE_MID = 1, STAGE_LAST = 2, STAGE_EPT = 4, STAGE_FIRST = 8 };

// waves per workgroup (one workgroup per CU): 16 (<= 128 VGPRs); a recorded pass carries the head
// weights in LDS and needs more registers: 12
template <int HEAD>
constexpr int edge_waves() { return HEAD == 1 ? 12 : EDGE_WAVES; }
// the last pass (no next r, no W1 in its image) fits 16 waves with the head too: it shares the middle passes'
// range table
template <int HEAD, int STAGE>
constexpr int edge_waves_s() { return (HEAD == 1 && (STAGE & 3) == STAGE_MID) ? 12 : EDGE_WAVES; }

// wave range table entry: first, end (sorted positions), source type, flags. A workgroup's range is its type's
// equal share of 16-edge tiles (type_split), moved forward to the next segment start, so that no (target, type)
// segment spans two workgroups. Inside it the waves take whole tiles, q or q + 1 each (the older waves, which
// the SIMD arbitration favours, the extra ones; waves w, w + 4, w + 8, w + 12 share a SIMD and their sums differ
// by at most one tile). A segment may then run across a wave boundary: its pieces go to the waves' LDS records
// and the wave holding its first piece combines them after the tile loop (edge_step_kernel).
// flags: 1 = the range starts inside a segment begun by the previous wave, 2 = its last segment continues into
// the next wave, 4 = the whole range is one segment
enum { RANGE_CONT_IN = 1, RANGE_CONT_OUT = 2, RANGE_ONE_SEG = 4 };
__device__ inline int4 edge_wave_range(const int* __restrict__ seg, const int* __restrict__ wg_start,
                                       const int* __restrict__ s_dst, int T, int64_t N, int blk, int wave, int NW) {
  if (blk >= wg_start[T]) return make_int4(0, 0, 0, 0);
  int t = 0;
  while (t + 1 < T && wg_start[t + 1] <= blk) ++t;
  const int ts = seg[t * N], te = seg[(t + 1) * N];
  const int gt = wg_start[t + 1] - wg_start[t], j = blk - wg_start[t];
  const int64_t tiles_t = (te - ts + 15) / 16;
  auto snap = [&](int p) -> int {               // first segment start at or after p
    if (p <= ts || p >= te) return min(p, te);
    const int dp = min(sdst_id(s_dst[p]), (int)N - 1);   // (clamped: in range for any prepared list)
    return dp == sdst_id(s_dst[p - 1]) ? seg[t * N + dp + 1] : p;
  };
  const int lo = snap(ts + 16 * (int)(tiles_t * j / gt)), hi = snap(ts + 16 * (int)(tiles_t * (j + 1) / gt));
  const int ntile = (hi - lo + 15) / 16;
  const int q = ntile / NW, r = ntile % NW;
  const int a0 = wave * q + min(wave, r), a1 = a0 + q + (wave < r ? 1 : 0);
  const int first = min(hi, lo + 16 * a0), end = min(hi, lo + 16 * a1);
  int flags = 0;
  if (first < end) {
    if (first > lo && sdst_id(s_dst[first - 1]) == sdst_id(s_dst[first])) flags |= RANGE_CONT_IN;
    if (end < hi && sdst_id(s_dst[end - 1]) == sdst_id(s_dst[end])) flags |= RANGE_CONT_OUT;
    if (sdst_id(s_dst[first]) == sdst_id(s_dst[end - 1])) flags |= RANGE_ONE_SEG;
  }
  return make_int4(first, end, t, flags);
}

// ranges for the middle passes (EDGE_WAVES waves) then the recorded passes (edge_waves<1>()), G blocks
__device__ inline void edge_ranges_fill(const int* seg, const int* wg_start, const int* s_dst, int T, int64_t N, int G,
                                        int4* __restrict__ ranges, int blk, int nblk) {
  const int n_mid = G * EDGE_WAVES, n_all = n_mid + G * edge_waves<1>();
  for (int q = blk * blockDim.x + threadIdx.x; q < n_all; q += nblk * blockDim.x) {
    const int NW = q < n_mid ? EDGE_WAVES : edge_waves<1>(), r = q < n_mid ? q : q - n_mid;
    ranges[q] = edge_wave_range(seg, wg_start, s_dst, T, N, r / NW, r % NW, NW);
  }
}

// Each edge's position in its (target, type) segment into the high byte of its s_dst entry (sdst_pack; read by
// chunks_of in every tile of every pass). One thread per edge, read off the segment table, so it holds for both
// range tables and after every prepare path; a list prepared by an earlier call is packed again to the same bits.
// The range table's threads read neighbouring entries while this runs: they look at the id bits only, which are
// rewritten unchanged (aligned 32-bit stores).
__device__ inline void edge_positions_fill(const int* __restrict__ seg, int* s_dst, int T, int64_t N, int blk, int nblk) {
  const int etot = seg[T * N];
  for (int p = blk * blockDim.x + threadIdx.x; p < etot; p += nblk * blockDim.x) {
    const int e = s_dst[p], dp = min(sdst_id(e), (int)N - 1);
    int t = 0;
    for (int k = 1; k < T; ++k) t += seg[k * N] <= p ? 1 : 0;   // (uniform loads)
    const int s0 = seg[t * N + dp], s1 = seg[t * N + dp + 1];
    s_dst[p] = sdst_pack(e, p - s0, s1 - 1 - p);
  }
}

// The first RB blocks fill the range tables, the others the segment positions (two short chains of dependent loads
// side by side instead of one after the other).
struct EdgeRangesArgs {
  const int *seg, *wg_start;
  int* s_dst;
  int T;
  int64_t N;
  int G;
  int4* ranges;
  const int64_t* ne;   // capacity mode: the device-side node count (N: the capacity)
  int RB, blocks;      // range-table blocks, and all blocks of the role
};

// block bx of a.blocks (the body of edge_ranges_kernel, and a role of prelude_b_kernel)
__device__ __forceinline__ void edge_ranges_role(const EdgeRangesArgs& a, int bx) {
  const int64_t N = a.ne ? a.ne[0] : a.N;
  if (bx < a.RB) edge_ranges_fill(a.seg, a.wg_start, a.s_dst, a.T, N, a.G, a.ranges, bx, a.RB);
  else edge_positions_fill(a.seg, a.s_dst, a.T, N, bx - a.RB, a.blocks - a.RB);
}

__global__ __launch_bounds__(256) void edge_ranges_kernel(EdgeRangesArgs a) { edge_ranges_role(a, blockIdx.x); }

// LDS-DMA of the r rows of one 16-edge tile (sorted positions base .. base + 15; rows past the array
// read 0, rows past the wave's range are loaded and ignored) into a 4 KB buffer: instruction i moves
// rows 4i .. 4i+3, LDS row rho holding global row base + rho with its 16-byte chunks XOR-permuted by
// 4 (rho & 3) -- the fragment reads (row c, chunk (4 ob + g) ^ 4 (c & 3)) are at most 2-way bank
// conflicted, and the four instructions share one lane offset (immediate 1 KB steps)
__device__ __forceinline__ void dma_rows(rsrc_t rs, int base, float* buf, int lane) {
  const int voff = (base + (lane >> 4)) * 256 + 16 * ((lane & 15) ^ (4 * (lane >> 4)));
  auto* l = (__attribute__((address_space(3))) void*)buf;
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, l, 16, voff, 0, 0, 0);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, l, 16, voff, 0, 1024, 0);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, l, 16, voff, 0, 2048, 0);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, l, 16, voff, 0, 3072, 0);
}

// The same DMA for the tile loop, issued from inline asm: hipcc's wait-count pass cannot tell these
// LDS writes from the weight image (its LDS alias scopes stop a few address steps deep) and would
// drain them before every weight read, serialising the prefetch with the tile's compute. Invisible to
// the compiler, they are waited for by hand (dma_wait below) and the compiler's own counts only
// over-wait. M0 is saved and restored; `s_nop 0` covers the M0-write -> LDS-DMA hazard, and the
// lgkmcnt(0) keeps the DMA behind the buffer's outstanding fragment reads.
typedef uint32_t u32x4v_s __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4v_s rsrc_words(const void* p, int bytes) {
  const uint64_t a = reinterpret_cast<uint64_t>(p);
  return u32x4v_s{(uint32_t)a, (uint32_t)(a >> 32) & 0xffffu, (uint32_t)bytes, (uint32_t)RSRC_DW3};
}
__device__ __forceinline__ void dma_rows_async(u32x4v_s rs, int base, float* buf, int lane) {
  const int voff = (base + (lane >> 4)) * 256 + 16 * ((lane & 15) ^ (4 * (lane >> 4)));
  const uint32_t m = __builtin_amdgcn_readfirstlane(
      (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float*)buf);
  uint32_t saved;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_waitcnt lgkmcnt(0)\n\t"
      "s_mov_b32 m0, %3\n\t"
      "s_nop 0\n\t"
      "buffer_load_dwordx4 %1, %2, 0 offen lds\n\t"
      "buffer_load_dwordx4 %1, %2, 0 offen offset:1024 lds\n\t"
      "buffer_load_dwordx4 %1, %2, 0 offen offset:2048 lds\n\t"
      "buffer_load_dwordx4 %1, %2, 0 offen offset:3072 lds\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(saved)
      : "v"(voff), "s"(rs), "s"(m)
      : "memory");
}
// Wait until at most N vector-memory operations are outstanding: with exactly N issued after the DMA
// above (the tile's unconditional stores), its rows have landed.
template <int N>
__device__ __forceinline__ void dma_wait() {
#ifdef PEMP_DMA_DRAIN   // diagnostics: wait for every outstanding vector-memory op instead of the hand count
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#else
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
#endif
}

// softmax exponent: the bare v_exp_f32 path (__expf) instead of expf (correctly rounded to ~1 ulp): the exponent is
// <= 0 and its relative error |x| 2^-24 ln 2 stays far below the 1e-4 logit bar
__device__ __forceinline__ float pemp_exp(float x) { return __expf(x); }
// segment normaliser: v_rcp_f32 (1 ulp) instead of the IEEE division
__device__ __forceinline__ float pemp_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
template <int AGG, int HEAD, int PREC, int UPD, int STAGE>
__global__ __launch_bounds__((64 * edge_waves_s<HEAD, STAGE>())) void edge_step_kernel(EdgeStepArgs a) {
  constexpr int NW = edge_waves_s<HEAD, STAGE>();
  // STAGE bit 2 (STAGE_EPT): EDGE_MLP per_type (TypeAwareEdgeUpdate, layers.py:275-303). The node
  // terms A'[dst] + B'[src] (already through their own ReLU and out-block, node_ept_kernel) join
  // after the e-block GEMM instead of inside the first ReLU.
  constexpr bool EPT = (STAGE & STAGE_EPT) != 0;
  constexpr bool MID = (STAGE & 3) == STAGE_MID;
  // attention with the update block pre-applied, f16x3: each message's softmax weight exp(a - M) is folded into
  // the split of m for the update GEMM (split_f16's per-lane factor) instead of a multiply of its 64 values
  constexpr bool PE_FOLD = AGG == PEMP_AGGR_ATTN && UPD && PREC == 2;
  // the last pass writes no next r: its copy of the image starts past W1 (SKIP floats)
  constexpr int SKIP = MID ? 0 : D * LDW;
  constexpr int IMG_F = img_common(UPD) + (HEAD == 1 ? IMG_HEAD : 0) - SKIP;
  constexpr bool FIRST = (STAGE & STAGE_FIRST) != 0;
  static_assert(!FIRST || (MID && !EPT && HEAD == 0 && PREC == 2 && UPD == 1 && AGG == PEMP_AGGR_ATTN),
                "the fused first pass is built for the published composed shape only");
  constexpr EmbedLayout ELO = embed_layout_published();
  constexpr int EMB_F = embed_comp_floats(ELO);
  __shared__ __attribute__((aligned(16))) float img[IMG_F];
  // the waves' 4 KB row buffers; FIRST: the composed embedding image (no rows are read)
  __shared__ __attribute__((aligned(16))) float rbuf[FIRST ? EMB_F : NW * 1024];
  // per wave: the pieces of the segments cut by its range ends ([0] the first segment, begun by an earlier wave;
  // [1] the last, continued by later waves): raw aggregate (64 floats), running max, normaliser
  constexpr int PREC_F = EDGE_PIECE_F;
  static_assert(!FIRST || (NW == 16 && edge_first_lds_bytes() <= 160 * 1024), "the fused first pass's LDS");
  __shared__ __attribute__((aligned(16))) float pieces[NW * 2 * PREC_F];
  float* vec = img + (3 + UPD) * D * LDW - SKIP;   // e2_b[64] | attn_w[64] | attn_b
  float* hw = img + img_common(UPD) - SKIP;        // HEAD 1: L1 [64][LDW], L2 [32][LDW], b1[64], b2[32], w3[32], b3
  float* hb_l = hw + (D + 32) * LDW;
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int T = a.T;
  EDGE_STAMP(0);
  // XCD-aware placement: blocks b and b + 8 share an XCD (round-robin dispatch), so logical block
  // (b % 8) * G/8 + b / 8 gives each XCD a contiguous run of logical blocks, i.e. few source types,
  // and its L2 holds only those types' node-table columns
  int lb = blockIdx.x;
  // (round 6: placing each XCD's workgroups on an eighth of the targets for every type instead -- one image's node-table
  // rows per XCD -- fetched 113.5 vs 107.8 MB per c3 pass and was no faster; profiles/r06_build_counts_xcd.md)
  if ((gridDim.x & 7) == 0) lb = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  const int4 rg = a.ranges[lb * NW + wave];
  // wave-uniform by construction; readfirstlane tells hipcc (else the tile loop and every buffer access
  // downstream are compiled as divergent)
  const int first = __builtin_amdgcn_readfirstlane(rg.x), end = __builtin_amdgcn_readfirstlane(rg.y);
  const int t = __builtin_amdgcn_readfirstlane(rg.z);
  const int rflags = __builtin_amdgcn_readfirstlane(rg.w);
  float* mybuf = rbuf + wave * 1024;
#ifdef PEMP_LDS_ZERO   // diagnostics: this wave's row buffer and piece records zeroed before first use
#pragma unroll
  for (int k = 0; k < 4; ++k) *reinterpret_cast<float4*>(mybuf + 256 * k + 4 * lane) = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int k = lane; k < 2 * PREC_F; k += 64) pieces[2 * wave * PREC_F + k] = 0.f;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
  const int E = (int)(a.ne ? a.ne[1] : a.E);
  float* const logits = a.edge_logits && a.ne ? a.edge_logits + (int64_t)a.rec * E : a.edge_logits;
  // r / Q0 rows past the wave's range end are out of the descriptor: the last tile's DMA moves no bytes
  // for them (its masked lanes read 0)
  const rsrc_t rs_r = make_rsrc(a.r_cur, end * 256);
  const rsrc_t rs_dst = make_rsrc(a.s_dst, E * 4), rs_src = make_rsrc(a.s_src, E * 4);
  const rsrc_t rs_nt = make_rsrc(a.NT, (int)a.N * a.t_nt_ld * 4);
  const rsrc_t rs_orig = make_rsrc(a.s_orig, E * 4);
  const rsrc_t rs_ea = make_rsrc(a.ea, FIRST ? E * a.A * 4 : 0);   // (32-bit: the host keeps E * A * 4 < 2^31)
  const int nt_row = a.t_nt_ld * 4;                  // bytes per node-table row
  const int nt_p = (128 + 64 * t) * 4;               // byte offset of P_t in a row (SGPR soffset)
  // a tile's gathers, issued at the end of the previous tile (the first tile's while the weight image is
  // copied): node-table rows of target and source, original ids
  float4 xa[4], xb[4], xp[4];
  int orig_t = 0;
  auto gather_nt = [&](int dstv, int srcv, bool on) {
    const int va = on ? sdst_id(dstv) * nt_row + 16 * g : OOB_VOFF, vb = on ? srcv * nt_row + 256 + 16 * g : OOB_VOFF;
#pragma unroll
    for (int ob = 0; ob < 4; ++ob) {
      xa[ob] = bld4(rs_nt, va + 64 * ob);
      xb[ob] = bld4(rs_nt, vb + 64 * ob);
      xp[ob] = bld4(rs_nt, va + 64 * ob, nt_p);
    }
  };
  // FIRST: the same gathers in two parts, each issued inside the tile where its registers come free
  auto gather_ab = [&](int dstv, int srcv) {
    const int va = sdst_id(dstv) * nt_row + 16 * g, vb = srcv * nt_row + 256 + 16 * g;
#pragma unroll
    for (int ob = 0; ob < 4; ++ob) {
      xa[ob] = bld4(rs_nt, va + 64 * ob);
      xb[ob] = bld4(rs_nt, vb + 64 * ob);
    }
  };
  auto gather_p = [&](int dstv) {
    const int va = sdst_id(dstv) * nt_row + 16 * g;
#pragma unroll
    for (int ob = 0; ob < 4; ++ob) xp[ob] = bld4(rs_nt, va + 64 * ob, nt_p);
  };
  // prologue order: the first two tiles' indices (the only loads the first gathers wait for: small, ahead of the
  // kernel-start burst), the type image, the first tile's node-table gathers, then its r rows
  int dst_n = 0, src_n = 0, dst_nn = 0, src_nn = 0;
  if (first < end) {   // (uniform)
    dst_n = bld1(rs_dst, 4 * min(first + c, end - 1));
    src_n = bld1(rs_src, 4 * min(first + c, end - 1));
    dst_nn = bld1(rs_dst, 4 * min(first + 16 + c, end - 1));
    src_nn = bld1(rs_src, 4 * min(first + 16 + c, end - 1));
  }
  // FIRST: original ids two tiles ahead and the edge_attr rows one tile ahead, as edge_embed_kernel reads them
  int o_next = 0;
  float ea_n[2][4];
  if (FIRST && first < end) o_next = bld1(rs_orig, 4 * min(first + c, end - 1));
  {
    // the block's type image: IMG_F floats, 1 KB per wave instruction, waves interleaved
    const float* src = a.img + (int64_t)t * a.img_stride + SKIP;
    constexpr int PIECES = IMG_F / 256, TAIL = IMG_F - PIECES * 256;
    for (int k = wave; k < PIECES; k += NW)
      dma16(src + 256 * k + 4 * lane, img + 256 * k);
    if (TAIL && wave == NW - 1 && 4 * lane < TAIL)
      *reinterpret_cast<float4*>(&img[256 * PIECES + 4 * lane]) = ld4(src + 256 * PIECES + 4 * lane);
    if constexpr (FIRST) {   // then the composed embedding image (a multiple of 4 floats)
      constexpr int EP = EMB_F / 256, ET = EMB_F - EP * 256;
      for (int k = wave; k < EP; k += NW) dma16(a.emb_img + 256 * k + 4 * lane, rbuf + 256 * k);
      if (ET && wave == NW - 2 && 4 * lane < ET)
        *reinterpret_cast<float4*>(&rbuf[256 * EP + 4 * lane]) = ld4(a.emb_img + 256 * EP + 4 * lane);
    }
  }
  if (FIRST) {
    // (the tile's node-table gathers are issued inside the tile, behind the embedding layers)
    if (first < end) {
      load_edge_attr32(rs_ea, a.A, o_next, ea_n);
      o_next = bld1(rs_orig, 4 * min(first + 16 + c, end - 1));
    }
  } else if (first < end) {
    gather_nt(dst_n, src_n, true);
    dma_rows(rs_r, first, mybuf, lane);
    if (HEAD == 1) orig_t = bld1(rs_orig, 4 * min(first + c, end - 1));
  }
  __syncthreads();
  EDGE_STAMP(1);
  EDGE_STAMP(2);
  // target of the segment begun by the previous wave (lane 0 of the first tile's indices; wave-uniform)
  const int seg_first = (rflags & RANGE_CONT_IN) ? sdst_id(__builtin_amdgcn_readfirstlane(dst_n)) : -1;
  const rsrc_t rs_next = make_rsrc(a.r_next, E * 256);
  const rsrc_t rs_agg = make_rsrc(a.agg, (int)a.N * T * 256);
  const u32x4v_s rw_r = rsrc_words(a.r_cur, end * 256);
  const u32x4v_s rw_q = rsrc_words(a.Q0, end * 256);
  const rsrc_t rs_q0 = make_rsrc(a.Q0, FIRST ? E * 256 : 0);   // FIRST: the Q0 rows are written here
  // stores issued after a tile's DMA, all unconditional (masked lanes write past the buffer end): the
  // r_next rows (middle passes that write them) and the aggregate rows
  const bool store_next = MID && a.write_next;

  // carry of the chunk continuing into the next tile: features in lane c == 0 of each row,
  // running max / normaliser wave-uniform
  float cacc[4][4];
  float cM = 0.f, cl = 0.f;
  bool have_carry = false;
  int tile_no = 0;
  for (int base = first; base < end; base += 16, ++tile_no) {
    if (tile_no < 4) EDGE_STAMP(3 + 3 * tile_no);
    // progress-ordered issue priority: a wave that has finished fewer tiles than its SIMD partners goes first
    // (the hardware otherwise favours the oldest wave, which then finishes long before the youngest)
    if (tile_no == 0) __builtin_amdgcn_s_setprio(3);
    else if (tile_no == 1) __builtin_amdgcn_s_setprio(2);
    else if (tile_no == 2) __builtin_amdgcn_s_setprio(1);
    else if (tile_no == 3) __builtin_amdgcn_s_setprio(0);
    // opaque zero: keeps the compiler from hoisting the LDS weight fragments out of the loop
    // (192+ VGPRs of loop-invariant loads would spill)
    int z = 0;
    asm volatile("" : "+s"(z));
    const float* W1 = img + z;                    // each matrix: 64 x LDW floats (or its hi + lo 16-bit parts)
    const float* W2 = img + z + D * LDW - SKIP;   // (W1: middle passes only, SKIP = 0)
    const float* WM = img + z + 2 * D * LDW - SKIP;
    const float* UW = img + z + 3 * D * LDW - SKIP;
    const float* hwz = hw + z;
    const int p = base + c;
    const bool valid = p < end;
    const int dst = dst_n, src = src_n;
    const bool more = base + 16 < end;
    dst_n = dst_nn;
    src_n = src_nn;
    // this tile's rows (DMA issued one tile ago) have landed: the ops issued after that DMA are the
    // previous tile's unconditional stores and this tile's gathers
    constexpr int NG = 12 + (HEAD == 1 ? 1 : 0);
    if (!FIRST && tile_no > 0) {
      if (store_next) dma_wait<8 + NG>();
      else dma_wait<4 + NG>();
    }
    float h[4][4], m[4][4], q0r[4][4];
    float4 rr[4];
    if constexpr (FIRST) {
      // the tile's embedding (edge_embed_kernel's composed body): q0r = Q0, stored for the later passes and kept for
      // this pass's r_next; rr = R0 = W_r h3 + b_r on its own accumulator
      const float* smz = rbuf + z;
      float y[4][4], r0[4][4];
      Frag<PREC> fx;
      ea_mask(a.A, ea_n, q0r, g + z);
      load_edge_attr32(rs_ea, a.A, o_next, ea_n, g + z);   // the next tile's rows (clamped ids past the range: harmless)
      o_next = bld1(rs_orig, 4 * min(base + 32 + c, end - 1));
      embed_tile_fixed<PREC, true>(smz, ELO, q0r, y, fx);   // q0r = Q0 (domain), y = h3, fx = h3's split
      const int vq0 = valid ? p * 256 + 16 * g : OOB_VOFF;   // masked lanes: stores dropped
#pragma unroll
      for (int ob = 0; ob < 4; ++ob) bst4(rs_q0, vq0 + 64 * ob, q0r[ob][0], q0r[ob][1], q0r[ob][2], q0r[ob][3]);
      gather_ab(dst, src);                          // this tile's A / B node-table rows, in flight over the R0 GEMM
      const float* br = smz + ELO.b_off[4];
#pragma unroll
      for (int ob = 0; ob < 4; ++ob) {
        const float4 bb = ld4(br + 16 * ob + 4 * g);
        r0[ob][0] = bb.x; r0[ob][1] = bb.y; r0[ob][2] = bb.z; r0[ob][3] = bb.w;
      }
      gemm_f<PREC, 4>(smz + ELO.w_off[4], y, fx, r0);
#pragma unroll
      for (int ob = 0; ob < 4; ++ob) rr[ob] = make_float4(r0[ob][0], r0[ob][1], r0[ob][2], r0[ob][3]);
    } else {
      // this tile's r rows from the DMA buffer (row c, chunk (4 ob + g) ^ 4 (c & 3)); the lane terms are
      // re-derived from the opaque zero each tile (kept live across the loop they would be spilled)
      const int cz = c + z, rowb = 64 * cz + 4 * g;
#pragma unroll
      for (int ob = 0; ob < 4; ++ob) rr[ob] = ld4(mybuf + (rowb ^ (16 * (ob ^ (cz & 3)))));
    }
    // this tile's gathers were issued at the end of the previous tile. Middle passes that write the next r:
    // once they have landed (waited for here, so that no later compiler wait can also wait on the DMA) the
    // Q0 rows of this tile go by LDS-DMA into the buffer just read, overlapping the first half of the tile
    const int vq = p * 256 + 16 * g;
    const int orig = orig_t;
    if (MID && !FIRST) {
#pragma unroll
      for (int ob = 0; ob < 4; ++ob) asm volatile("" ::"v"(xa[ob].x), "v"(xb[ob].x), "v"(xp[ob].x));
      if (store_next) dma_rows_async(rw_q, base, mybuf, lane);
    }
    {
      const int qn = min(base + 32 + c, end - 1);
      dst_nn = bld1(rs_dst, 4 * qn);
      src_nn = bld1(rs_src, 4 * qn);
    }
    float ab[4][4];                               // EPT: A'[dst] + B'[src]
#pragma unroll
    for (int ob = 0; ob < 4; ++ob) {
      if (EPT) {
        h[ob][0] = rr[ob].x; h[ob][1] = rr[ob].y; h[ob][2] = rr[ob].z; h[ob][3] = rr[ob].w;
        ab[ob][0] = xa[ob].x + xb[ob].x; ab[ob][1] = xa[ob].y + xb[ob].y;
        ab[ob][2] = xa[ob].z + xb[ob].z; ab[ob][3] = xa[ob].w + xb[ob].w;
      } else {
        h[ob][0] = rr[ob].x + xa[ob].x + xb[ob].x; h[ob][1] = rr[ob].y + xa[ob].y + xb[ob].y;
        h[ob][2] = rr[ob].z + xa[ob].z + xb[ob].z; h[ob][3] = rr[ob].w + xa[ob].w + xb[ob].w;
      }
    }
    if constexpr (FIRST) {
      // the P_t rows (read at the message GEMM) and this wave's own Q0 rows back through the descriptor they were
      // stored with (read at the r_next GEMM; kept in 16 registers from the embedding instead they cost more,
      // DESIGN §4): issued once the A / B rows are consumed
#pragma unroll
      for (int ob = 0; ob < 4; ++ob) asm volatile("" ::"v"(h[ob][0]), "v"(h[ob][1]), "v"(h[ob][2]), "v"(h[ob][3]));
      gather_p(dst);
#pragma unroll
      for (int ob = 0; ob < 4; ++ob) {
        const float4 q = bld4(rs_q0, min(p, end - 1) * 256 + 16 * g + 64 * ob);
        q0r[ob][0] = q.x; q0r[ob][1] = q.y; q0r[ob][2] = q.z; q0r[ob][3] = q.w;
      }
    }
    // other passes: the r rows of tile k+1 into the buffer this tile's rows were read from, once every
    // gather of this tile has returned (the compiler's waits on those would otherwise also wait on the DMA)
    if (!MID) {
#pragma unroll
      for (int ob = 0; ob < 4; ++ob) asm volatile("" ::"v"(xa[ob].x), "v"(xb[ob].x), "v"(xp[ob].x));
      if (HEAD == 1) asm volatile("" ::"v"(orig));
      if (more) dma_rows_async(rw_r, base + 16, mybuf, lane);
    }
#pragma unroll
    for (int ob = 0; ob < 4; ++ob) {
      m[ob][0] = xp[ob].x; m[ob][1] = xp[ob].y; m[ob][2] = xp[ob].z; m[ob][3] = xp[ob].w;
    }
#ifdef PEMP_STAMPS
    asm volatile("" ::"v"(h[0][0]), "v"(h[3][3]));
    if (tile_no < 4) EDGE_STAMP(4 + 3 * tile_no);
#endif
    // edge MLP layer 1: h = ReLU(r + A[dst] + B[src]), r = Q0 + W1_e_cur · e_cur
    relu_frag<4>(h);
    // layer 2: e' = ReLU(W2 · h + b2)
    float ep[4][4];
#pragma unroll
    for (int ob = 0; ob < 4; ++ob) {
      const float4 b2 = ld4(vec + 16 * ob + 4 * g);
      ep[ob][0] = b2.x; ep[ob][1] = b2.y; ep[ob][2] = b2.z; ep[ob][3] = b2.w;
      if (EPT) { ep[ob][0] += ab[ob][0]; ep[ob][1] += ab[ob][1]; ep[ob][2] += ab[ob][2]; ep[ob][3] += ab[ob][3]; }
    }
    {
      Frag<PREC> fh;
      prep<PREC, true>(h, fh);                    // (h, e', the head's h1 and m are relu1 outputs)
      gemm_f<PREC, 4>(W2, h, fh, ep);
    }
    relu_frag<4>(ep);
    float av = 0.f;
    if (AGG == PEMP_AGGR_ATTN) {                  // attention row pre-scaled by dom_inv in the image
#pragma unroll
      for (int ob = 0; ob < 4; ++ob) {
        const float4 w = ld4(vec + D + 16 * ob + 4 * g);
        av = fmaf(w.x, ep[ob][0], av); av = fmaf(w.y, ep[ob][1], av);
        av = fmaf(w.z, ep[ob][2], av); av = fmaf(w.w, ep[ob][3], av);
      }
      av = xsum_rows(av);
      av += vec[z + 2 * D];                      // attention bias (re-read: a register copy spills)
    }
    // chunk structure of the tile and each edge's softmax weight pe = exp(a - M), M = its segment's maximum so far
    // (computed before the message GEMMs: with PE_FOLD it rides in the split of m)
    const int seg = valid ? sdst_id(dst) : -1 - c;   // padding lanes: singleton chunks, never written
    const Chunks ck = chunks_of(dst, c, min(end - 1 - base, 15), valid);
    const bool carry_in = have_carry;            // wave-uniform: set only when the segment continues
    float M = 0.f, pe = 1.0f;
    if (AGG == PEMP_AGGR_ATTN) {
#if PEMP_ASM_SCANS
      M = chunk_max_asm(av, chunk_masks(ck));   // (checked on the GPU in every precision)
#else
      M = seg_bcast_tail_max(seg_max(av, ck.d), ck.u);
#endif
      if (carry_in && ck.d == c) M = fmaxf(M, cM);   // head chunk continues the carried segment
      pe = pemp_exp(av - M);
    }
    if (HEAD == 2) {   // generic edge head (weights in global memory, true domain)
      float h1[4][4], h2[4][4];
#pragma unroll
      for (int ob = 0; ob < 4; ++ob)
#pragma unroll
        for (int r = 0; r < 4; ++r) h1[ob][r] = ep[ob][r] * dom_inv<PREC>();
      mlp_frag<4>(a.head, h1, h2);
      if (valid && g == 0)   // (descriptor store: an out-of-range id from a contract-breaking list is dropped)
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(h1[0][0]), make_rsrc(logits, E * 4),
                                              4 * a.s_orig[p], 0, 0);
    }
    Frag<PREC> fe;                                // e' split once for the r_next, head and message GEMMs
    prep<PREC, true>(ep, fe);
    if (MID && !FIRST) {
      // this tile's Q0 rows have landed (only the two index loads were issued after their DMA): read them,
      // then the r rows of tile k+1 into the same buffer
      if (store_next) {
        dma_wait<2>();
        const int cz = c + z, rowb = 64 * cz + 4 * g;
#pragma unroll
        for (int ob = 0; ob < 4; ++ob) {
          const float4 q = ld4(mybuf + (rowb ^ (16 * (ob ^ (cz & 3)))));
          q0r[ob][0] = q.x; q0r[ob][1] = q.y; q0r[ob][2] = q.z; q0r[ob][3] = q.w;
        }
      }
      if (more) dma_rows_async(rw_r, base + 16, mybuf, lane);
    }
    if (MID && a.write_next) {                    // next pass's r = Q0 + W1_e_cur · e'
      gemm_f<PREC, 4>(W1, ep, fe, q0r);
      const int vn = valid ? vq : OOB_VOFF;
#pragma unroll
      for (int ob = 0; ob < 4; ++ob) bst4(rs_next, vn + 64 * ob, q0r[ob][0], q0r[ob][1], q0r[ob][2], q0r[ob][3]);
    }
    if (HEAD == 1) {   // fused edge-classification head on e' (image: b1, b2 x dom, w3 x dom_inv)
      const float* hb = hb_l + z;
      float h1[4][4], h2[2][4];
#pragma unroll
      for (int ob = 0; ob < 4; ++ob) {
        const float4 bb = ld4(hb + 16 * ob + 4 * g);
        h1[ob][0] = bb.x; h1[ob][1] = bb.y; h1[ob][2] = bb.z; h1[ob][3] = bb.w;
      }
      gemm_f<PREC, 4>(hwz, ep, fe, h1);
      relu_frag<4>(h1);
#pragma unroll
      for (int ob = 0; ob < 2; ++ob) {
        const float4 bb = ld4(hb + D + 16 * ob + 4 * g);
        h2[ob][0] = bb.x; h2[ob][1] = bb.y; h2[ob][2] = bb.z; h2[ob][3] = bb.w;
      }
      {
        Frag<PREC> f1;
        prep<PREC, true>(h1, f1);
        gemm_f<PREC, 2>(hwz + D * LDW, h1, f1, h2);
      }
      relu_frag<2>(h2);
      float lg = 0.f;
#pragma unroll
      for (int ob = 0; ob < 2; ++ob) {
        const float4 w = ld4(hb + D + 32 + 16 * ob + 4 * g);
        lg = fmaf(w.x, h2[ob][0], lg); lg = fmaf(w.y, h2[ob][1], lg);
        lg = fmaf(w.z, h2[ob][2], lg); lg = fmaf(w.w, h2[ob][3], lg);
      }
      lg = xsum_rows(lg);
      if (valid && g == 0)   // (descriptor store: an out-of-range id from a contract-breaking list is dropped)
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(lg + hb[D + 64]), make_rsrc(logits, E * 4),
                                              4 * orig, 0, 0);
    }
    // message: m = ReLU(P_t[dst] + W_t_e · e')
    gemm_f<PREC, 4>(WM, ep, fe, m);
    relu_frag<4>(m);
    if (UPD) {                                    // m <- U_t · m (no bias: added once per node)
      float u[4][4];
#pragma unroll
      for (int ob = 0; ob < 4; ++ob)
#pragma unroll
        for (int r = 0; r < 4; ++r) u[ob][r] = 0.0f;
      Frag<PREC> fm;
      if constexpr (PE_FOLD) prep_f16_scaled<true>(m, fm, pe);
      else prep<PREC, true>(m, fm);
      gemm_f<PREC, 4>(UW, m, fm, u);
#pragma unroll
      for (int ob = 0; ob < 4; ++ob)
#pragma unroll
        for (int r = 0; r < 4; ++r) m[ob][r] = u[ob][r];
    }

    // ---- segmented reduction of the tile, carry in / out ----
    float l = (AGG == PEMP_AGGR_ATTN) ? pe : 1.0f;
    float v[4][4];
#pragma unroll
    for (int ob = 0; ob < 4; ++ob)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[ob][r] = (AGG == PEMP_AGGR_ATTN && !PE_FOLD) ? pe * m[ob][r] : m[ob][r];
    if (carry_in && c == 0) {
      if (AGG == PEMP_AGGR_ATTN) {
        const float f = pemp_exp(cM - M);
        l += cl * f;
#pragma unroll
        for (int ob = 0; ob < 4; ++ob)
#pragma unroll
          for (int r = 0; r < 4; ++r) v[ob][r] = fmaf(cacc[ob][r], f, v[ob][r]);
      } else {
        l += cl;
#pragma unroll
        for (int ob = 0; ob < 4; ++ob)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            v[ob][r] = (AGG == PEMP_AGGR_MAX) ? fmaxf(v[ob][r], cacc[ob][r]) : v[ob][r] + cacc[ob][r];
      }
    }
    const ScanMask smk = scan_mask(ck.d);
    {
      if (AGG == PEMP_AGGR_ATTN || AGG == PEMP_AGGR_MEAN) l = seg_sum(l, smk);   // normaliser / count
#pragma unroll
      for (int ob = 0; ob < 4; ++ob)
#pragma unroll
        for (int r = 0; r < 4; ++r) v[ob][r] = (AGG == PEMP_AGGR_MAX) ? seg_max(v[ob][r], ck.d) : seg_sum(v[ob][r], smk);
    }
    // the chunk at the tile end continues iff the next tile starts with the same target
    const int seg15 = __builtin_amdgcn_readlane(seg, 15);
    const bool carry_out = more && sdst_id(__builtin_amdgcn_readlane(dst_n, 0)) == seg15;
    if (carry_out) {
      cl = readlane_f(l, 15);
      cM = readlane_f(M, 15);
#pragma unroll
      for (int ob = 0; ob < 4; ++ob)
#pragma unroll
        for (int r = 0; r < 4; ++r) cacc[ob][r] = dppf<DPP_SHL15>(v[ob][r], 0.0f);   // lane 15 -> lane 0
    }
    have_carry = carry_out;
    {
      // the aggregate leaves the f16x3 domain here (dom_inv)
      const float inv = ((AGG == PEMP_AGGR_ATTN) ? pemp_rcp(l + 1e-12f) : (AGG == PEMP_AGGR_MEAN) ? pemp_rcp(l) : 1.0f) *
                        dom_inv<PREC>();
      const bool out = valid && ck.tail && !(carry_out && c == 15);
      // a segment cut by a range end: its raw piece goes to this wave's record instead (at most two per wave; the
      // last segment of the range ends at the last tile's last valid lane)
      const bool pin = seg == seg_first;
      const bool pout = (rflags & RANGE_CONT_OUT) && !more && seg == __builtin_amdgcn_readlane(seg, end - 1 - base);
      const bool piece = out && (pin || pout);
      const int vo = out && !piece ? (seg * T + t) * 256 + 16 * g : OOB_VOFF;
#pragma unroll
      for (int ob = 0; ob < 4; ++ob) bst4(rs_agg, vo + 64 * ob, v[ob][0] * inv, v[ob][1] * inv, v[ob][2] * inv, v[ob][3] * inv);
      if (piece) {
        float* rec = pieces + (2 * wave + (pin ? 0 : 1)) * PREC_F;
#pragma unroll
        for (int ob = 0; ob < 4; ++ob)
          *reinterpret_cast<float4*>(rec + 16 * ob + 4 * g) = make_float4(v[ob][0], v[ob][1], v[ob][2], v[ob][3]);
        if (g == 0) { rec[64] = M; rec[65] = l; }
      }
    }
    {   // the next tile's gathers, unconditional (past the range: OOB offsets, no traffic). (Issued ahead of this
      // tile's aggregate stores instead, so that the next tile's wait skips those stores: no gain)
      if (!FIRST) gather_nt(dst_n, src_n, more);
      if (HEAD == 1) orig_t = bld1(rs_orig, 4 * min(p + 16, end - 1));
    }
#ifdef PEMP_STAMPS
    asm volatile("" ::"v"(v[0][0]), "v"(v[3][3]));
    if (tile_no < 4) EDGE_STAMP(5 + 3 * tile_no);
#endif
  }
  // segments cut by wave boundaries: the wave holding the first piece combines the pieces in range order (the
  // later waves' [0] records, while those are whole-range middle pieces) and writes the aggregate row
  __syncthreads();
  constexpr int MIDDLE = RANGE_CONT_IN | RANGE_CONT_OUT | RANGE_ONE_SEG;   // a whole range inside one segment
  if ((rflags & RANGE_CONT_OUT) && (rflags & MIDDLE) != MIDDLE) {
    const float* r0 = pieces + (2 * wave + 1) * PREC_F;
    float M = r0[64], l = r0[65], v = r0[lane];
    for (int k = wave + 1; k < NW; ++k) {
      const float* rk = pieces + 2 * k * PREC_F;
      const float Mk = rk[64], lk = rk[65], vk = rk[lane];
      if (AGG == PEMP_AGGR_ATTN) {
        const float Mn = fmaxf(M, Mk), fa = pemp_exp(M - Mn), fb = pemp_exp(Mk - Mn);
        l = l * fa + lk * fb;
        v = v * fa + vk * fb;
        M = Mn;
      } else if (AGG == PEMP_AGGR_MAX) {
        v = fmaxf(v, vk);
      } else {
        l += lk;
        v += vk;
      }
      const int fk = __builtin_amdgcn_readfirstlane(a.ranges[lb * NW + k].w);
      if ((fk & MIDDLE) != MIDDLE) break;
    }
    const float inv = ((AGG == PEMP_AGGR_ATTN) ? 1.0f / (l + 1e-12f) : (AGG == PEMP_AGGR_MEAN) ? 1.0f / l : 1.0f) *
                      dom_inv<PREC>();
    const int seg_last = sdst_id(__builtin_amdgcn_readfirstlane(a.s_dst[end - 1]));
    a.agg[((int64_t)seg_last * T + t) * 64 + lane] = v * inv;
  }
  EDGE_STAMP(15);
}

// Node update (separate launch, the whole edge pass must have finished): one workgroup per
// (16-node tile, 16-output block), one wave per type (wave w: types w and w + 16, T <= 17);
// fixed-order reduction over waves.
//   x_new[n] = ReLU(b + sum_t U_t · agg[n, t])   (layers.py:253-258; empty segments read as 0)
//   without an update MLP: x_new[n] = agg[n, 0]  (MPLayer, layers.py:32-86)
// Written to X[:, 64:128]. Every load of a wave is issued before its first MFMA.
// ---- generic node-update MLP on the per-type aggregates (UPDATE_TYPE hierarch_mlp / hierarch_cnn,
// layers.py:89-154): the host folds each variant into up to 4 dense layers over agg[n] flattened
// to [T*64] (block-sparse structure as explicit zeros, the Conv1d / permute / reshape orders as
// column permutations), every layer ReLU'd. One 256-thread block per 16 nodes; activations stay in
// LDS; layer l: each wave owns 16-output blocks, K in chunks of 16 on v_mfma_f32_16x16x4_f32
// (weights float4 from global / L2, activations float4 from LDS).
struct NodeMlpArgs {
  const float* agg;
  const int* seg;
  int T;
  int64_t N;
  pemp_mlp mlp;
  int max_out;      // widest layer output
  float* X;
  const int64_t* ne;   // capacity mode: device-side node count (N: the capacity)
};

__host__ __device__ inline int nmlp_stride(int k) { return (k + 15) / 16 * 16 + 8; }   // 8 * odd mod 64 dwords

__global__ __launch_bounds__(256) void node_mlp_kernel(NodeMlpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int64_t n0 = (int64_t)blockIdx.x * 16, N = a.ne ? a.ne[0] : a.N;
  if (n0 >= N) return;   // (capacity grids)
  const int T = a.T, K0 = 64 * T;
  const int S[2] = {nmlp_stride(K0 > a.max_out ? K0 : a.max_out), nmlp_stride(a.max_out)};
  float* buf[2] = {lds, lds + 16 * S[0]};
  // agg rows of the 16 nodes; an empty (n, t) segment was never written by the edge pass -> 0
  for (int idx = threadIdx.x; idx < 16 * K0 / 4; idx += 256) {
    const int r = idx / (K0 / 4), col = (idx - r * (K0 / 4)) * 4, t = col >> 6;
    const int64_t n = n0 + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n < N && a.seg[t * N + n + 1] > a.seg[t * N + n]) v = ld4(a.agg + n * K0 + col);
    *reinterpret_cast<float4*>(&buf[0][r * S[0] + col]) = v;
  }
  __syncthreads();
  const int L = a.mlp.n_layers;
  for (int l = 0; l < L; ++l) {
    const pemp_layer ly = a.mlp.layer[l];
    const float* in = buf[l & 1];
    float* out = buf[(l + 1) & 1];
    const int si = S[l & 1], so = S[(l + 1) & 1];
    const int K = ly.in_dim, M = ly.out_dim;
    const bool last = l + 1 == L;
    for (int jb = wave; jb < M / 16; jb += 4) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const float* wrow = ly.w + (int64_t)(16 * jb + c) * K + 4 * g;
      const float* arow = in + c * si + 4 * g;
      for (int k0 = 0; k0 < K; k0 += 16) {
        const float4 w4 = ld4(wrow + k0);
        const float4 x4 = *reinterpret_cast<const float4*>(arow + k0);
        acc = mfma4(w4.x, x4.x, acc);
        acc = mfma4(w4.y, x4.y, acc);
        acc = mfma4(w4.z, x4.z, acc);
        acc = mfma4(w4.w, x4.w, acc);
      }
      // lane (c, g) holds outputs 16 jb + 4 g + r of node c
      const float4 b4 = ld4(ly.b + 16 * jb + 4 * g);
      float4 o = make_float4(acc[0] + b4.x, acc[1] + b4.y, acc[2] + b4.z, acc[3] + b4.w);
      if (ly.relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
      if (!last) *reinterpret_cast<float4*>(&out[c * so + 16 * jb + 4 * g]) = o;
      else if (n0 + c < N) *reinterpret_cast<float4*>(&a.X[(n0 + c) * 128 + 64 + 16 * jb + 4 * g]) = o;
    }
    __syncthreads();
  }
}

// ---- EDGE_MLP per_type node terms (TypeAwareEdgeUpdate, layers.py:288-303) -------------------
// NT[n][0:64]   = O1 · ReLU(L1[type n] · x_n + c1[type n])   (the x_i = target block)
// NT[n][64:128] = O2 · ReLU(L2[type n] · x_n + c2[type n])   (the x_j = source block)
// Nodes of a type >= T keep zero (the reference leaves their rows of tmp_1 / tmp_2 at 0). One block
// per 16 nodes: for every type present in the tile the 16 rows run through that type's weights on
// fp32 MFMA and only the rows of that type are kept; then the shared out-block GEMM.
struct NodeEptArgs {
  const float* X;             // [N][128] = [x_init | x_cur]
  const int64_t* types;
  int64_t ts;                 // node_types stride
  int T;
  int64_t N;
  const float *l1_w, *l1_b, *l2_w, *l2_b, *o1_w, *o2_w;
  float* NT;
  int ldnt;
  float out_scale;            // the edge passes' domain (dom<PREC>())
  const int64_t* ne;          // capacity mode: device-side node count (N: the capacity)
};

__global__ __launch_bounds__(256) void node_ept_kernel(NodeEptArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[16 * 136];   // strides 136, 72: 8 * odd mod 64 dwords
  __shared__ __attribute__((aligned(16))) float us[16 * 72];
  __shared__ int tys[16];
  __shared__ unsigned tmask;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int64_t n0 = (int64_t)blockIdx.x * 16, N = a.ne ? a.ne[0] : a.N;
  if (n0 >= N) return;   // (capacity grids)
  for (int idx = threadIdx.x; idx < 16 * 32; idx += 256) {
    const int r = idx >> 5, c4 = (idx & 31) * 4;
    const int64_t n = n0 + r;
    *reinterpret_cast<float4*>(&xs[r * 136 + c4]) = n < N ? ld4(a.X + n * 128 + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (threadIdx.x < 16) {
    const int64_t n = n0 + threadIdx.x;
    const int64_t t = n < N ? a.types[n * a.ts] : -1;
    tys[threadIdx.x] = (t >= 0 && t < a.T) ? (int)t : -1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned m = 0;
    for (int i = 0; i < 16; ++i) m |= tys[i] >= 0 ? 1u << tys[i] : 0u;
    tmask = m;
  }
  const int jb = wave;                              // 4 waves x 16 outputs = 64
  for (int part = 0; part < 2; ++part) {
    for (int idx = threadIdx.x; idx < 16 * 72; idx += 256) us[idx] = 0.f;
    __syncthreads();
    const float* Lw = part ? a.l2_w : a.l1_w;
    const float* Lb = part ? a.l2_b : a.l1_b;
    for (unsigned m = tmask; m; m &= m - 1) {
      const int t = __ffs(m) - 1;
      const float* wrow = Lw + ((int64_t)t * 64 + 16 * jb + c) * 128 + 4 * g;
      const float* xrow = xs + c * 136 + 4 * g;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k0 = 0; k0 < 128; k0 += 16) {
        const float4 w4 = ld4(wrow + k0);
        const float4 x4 = *reinterpret_cast<const float4*>(xrow + k0);
        acc = mfma4(w4.x, x4.x, acc); acc = mfma4(w4.y, x4.y, acc);
        acc = mfma4(w4.z, x4.z, acc); acc = mfma4(w4.w, x4.w, acc);
      }
      if (tys[c] == t) {   // lane (c, g): outputs 16 jb + 4 g + r of node c
        const float4 b4 = ld4(Lb + t * 64 + 16 * jb + 4 * g);
        *reinterpret_cast<float4*>(&us[c * 72 + 16 * jb + 4 * g]) =
            make_float4(fmaxf(acc[0] + b4.x, 0.f), fmaxf(acc[1] + b4.y, 0.f), fmaxf(acc[2] + b4.z, 0.f),
                        fmaxf(acc[3] + b4.w, 0.f));
      }
    }
    __syncthreads();
    const float* orow = (part ? a.o2_w : a.o1_w) + (16 * jb + c) * 64 + 4 * g;
    const float* urow = us + c * 72 + 4 * g;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k0 = 0; k0 < 64; k0 += 16) {
      const float4 w4 = ld4(orow + k0);
      const float4 u4 = *reinterpret_cast<const float4*>(urow + k0);
      acc = mfma4(w4.x, u4.x, acc); acc = mfma4(w4.y, u4.y, acc);
      acc = mfma4(w4.z, u4.z, acc); acc = mfma4(w4.w, u4.w, acc);
    }
    if (n0 + c < N)
      *reinterpret_cast<float4*>(&a.NT[(n0 + c) * a.ldnt + 64 * part + 16 * jb + 4 * g]) =
          make_float4(acc[0] * a.out_scale, acc[1] * a.out_scale, acc[2] * a.out_scale, acc[3] * a.out_scale);
    __syncthreads();
  }
}

inline int nmlp_max_out(const pemp_mlp& m) {
  int mx = 0;
  for (int l = 0; l < m.n_layers; ++l) mx = std::max(mx, m.layer[l].out_dim);
  return mx;
}

inline size_t nmlp_lds_bytes(int T, const pemp_mlp& m) {
  const int mo = nmlp_max_out(m);
  return (size_t)16 * (nmlp_stride(std::max(64 * T, mo)) + nmlp_stride(mo)) * sizeof(float);
}

struct NodeUpdateArgs {
  const float* agg;
  const int* seg;
  int T;
  int64_t N;
  const float *upd_w, *upd_b;
  float* X;
  const int64_t* ne;   // capacity mode: device-side node count (N: the capacity)
};

constexpr int UPD_WAVES = 16;

__global__ __launch_bounds__(64 * UPD_WAVES) void node_update_kernel(NodeUpdateArgs a) {
  __shared__ __attribute__((aligned(16))) float red[UPD_WAVES][16 * 17];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int64_t n0 = (int64_t)blockIdx.x * 16, N = a.ne ? a.ne[0] : a.N;
  if (n0 >= N) return;   // (capacity grids)
  const int ob = blockIdx.y, T = a.T;
  if (!a.upd_w) {   // x_new = agg[n, 0] (T == 1), this block's 16 features
    if (threadIdx.x < 256) {
      const int r = threadIdx.x >> 4, f = threadIdx.x & 15;
      const int64_t n = n0 + r;
      if (n < N) {
        const float v = a.seg[n + 1] > a.seg[n] ? a.agg[n * D + 16 * ob + f] : 0.0f;
        a.X[n * 128 + 64 + 16 * ob + f] = v;
      }
    }
    return;
  }
  const int64_t n = n0 + c, nc = n < N ? n : N - 1;   // clamped: every load below is unconditional
  const int ldu = 64 * T;
  const float* wrow = a.upd_w + (int64_t)(16 * ob + c) * ldu + 4 * g;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (wave < T) {
    const int tt[2] = {wave, min(wave + UPD_WAVES, T - 1)};
    float4 xv[2][4], wv[2][4];
    int s0[2], s1[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) {
        xv[k][mb] = ld4(a.agg + (nc * T + tt[k]) * D + 16 * mb + 4 * g);
        wv[k][mb] = ld4(wrow + 64 * tt[k] + 16 * mb);
      }
      s0[k] = a.seg[tt[k] * N + nc];
      s1[k] = a.seg[tt[k] * N + nc + 1];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      // an empty (n, t) segment was never written by the edge pass; the second slot is live only
      // for wave + 16 < T
      const int keep = (n < N && s1[k] > s0[k] && (k == 0 || wave + UPD_WAVES < T)) ? -1 : 0;
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) {
        acc = mfma4(wv[k][mb].x, __int_as_float(__float_as_int(xv[k][mb].x) & keep), acc);
        acc = mfma4(wv[k][mb].y, __int_as_float(__float_as_int(xv[k][mb].y) & keep), acc);
        acc = mfma4(wv[k][mb].z, __int_as_float(__float_as_int(xv[k][mb].z) & keep), acc);
        acc = mfma4(wv[k][mb].w, __int_as_float(__float_as_int(xv[k][mb].w) & keep), acc);
      }
    }
  }
  // lane (c, g) holds outputs 16 ob + 4 g + r of node c
  *reinterpret_cast<float4*>(&red[wave][c * 17 + 4 * g]) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  __syncthreads();
  if (threadIdx.x < 256) {
    const int r = threadIdx.x >> 4, f = threadIdx.x & 15;
    float sum = 0.f;
#pragma unroll
    for (int w = 0; w < UPD_WAVES; ++w) sum += red[w][r * 17 + f];
    if (n0 + r < N) a.X[(n0 + r) * 128 + 64 + 16 * ob + f] = fmaxf(sum + a.upd_b[16 * ob + f], 0.0f);
  }
}

// ---- small MLPs staged in LDS (node embedding, node/class heads) ----
// Layer l of a pemp_mlp: weights [16 OB][16 KB] (fold.py zero-pads to 16) -> LDS rows of stride
// lds_stride(16 KB), then the bias (16 OB floats).
__host__ __device__ inline int mlp_lds_floats(const pemp_mlp& m) {
  int n = 0;
  for (int l = 0; l < m.n_layers; ++l) {
    const int KB = (m.layer[l].in_dim + 15) >> 4, OB = (m.layer[l].out_dim + 15) >> 4;
    n += 16 * OB * lds_stride(16 * KB) + 16 * OB;
  }
  return n;
}

// Stage up to three MLPs back to back (the layout mlp_lds_frag / mlp_lds_floats assume) with ONE
// batched pass: every thread issues 8 float4 loads before its first LDS store, over the
// concatenation of all weight and bias segments (weights row-major [16 OB][16 KB], biases one row).
// The segment table is built on the host and passed by value (kernel arguments, scalar loads).
constexpr int STAGE_MAXSEG = 24;
struct StagePlan {
  const float* src[STAGE_MAXSEG];
  int q[STAGE_MAXSEG], ld[STAGE_MAXSEG], dst[STAGE_MAXSEG], cum[STAGE_MAXSEG];
  int n, total;
};

static StagePlan stage_plan(const pemp_mlp* m0, const pemp_mlp* m1 = nullptr, const pemp_mlp* m2 = nullptr) {
  StagePlan p{};
  int off = 0;
  for (const pemp_mlp* m : {m0, m1, m2}) {
    if (!m) continue;
    for (int l = 0; l < m->n_layers; ++l) {
      const pemp_layer& L = m->layer[l];
      const int KB = (L.in_dim + 15) >> 4, OB = (L.out_dim + 15) >> 4, ld = lds_stride(16 * KB);
      p.src[p.n] = L.w; p.q[p.n] = 4 * KB; p.ld[p.n] = ld; p.dst[p.n] = off; p.cum[p.n] = p.total; ++p.n;
      p.total += 16 * OB * 4 * KB;
      off += 16 * OB * ld;
      p.src[p.n] = L.b; p.q[p.n] = 4 * OB; p.ld[p.n] = 0; p.dst[p.n] = off; p.cum[p.n] = p.total; ++p.n;
      p.total += 4 * OB;
      off += 16 * OB;
    }
  }
  return p;
}

// one element (float4) of the LDS image described by a plan: source address and image offset
__device__ inline void plan_element(const StagePlan& p, int idx, const float** src, int* dst) {
  const float* sp = p.src[0];
  int q = p.q[0], ld = p.ld[0], d0 = p.dst[0], cum = 0;
  for (int j = 1; j < p.n; ++j)
    if (idx >= p.cum[j]) { sp = p.src[j]; q = p.q[j]; ld = p.ld[j]; d0 = p.dst[j]; cum = p.cum[j]; }
  const int local = idx - cum, r = local / q;
  *src = sp + 4 * local;
  *dst = d0 + r * ld + 4 * (local - r * q);
}

// LDS image of the node-side MLPs ([emb | node head | class head], mlp_lds_floats layouts): built once
// per weight set (pemp_mpn_node_image) or, without one, once per forward into the workspace
__global__ __launch_bounds__(256) void stage_image_kernel(StagePlan plan, float* __restrict__ img) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gs = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = gid; i < plan.total; i += gs) {
    const float* src;
    int dst;
    plan_element(plan, (int)i, &src, &dst);
    *reinterpret_cast<float4*>(img + dst) = ld4(src);
  }
}

// flat copy of `n` floats (multiple of 4) from global to LDS, 8 float4 loads in flight per thread
__device__ inline void copy_to_lds(float* __restrict__ lds, const float* __restrict__ src, int n) {
  const int n4 = n >> 2, bs = blockDim.x;
  for (int base = threadIdx.x; base < n4; base += 8 * bs) {
    float4 t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = ld4(src + 4 * min(base + k * bs, n4 - 1));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (base + k * bs < n4) *reinterpret_cast<float4*>(&lds[4 * (base + k * bs)]) = t[k];
  }
}


// whole staged MLP on one wave's fragments (widths <= 64); result in `a`
__device__ inline void mlp_lds_frag(const float* lds, const pemp_mlp& m, float (&a)[4][4]) {
  float b[4][4];
  int off = 0;
  for (int l = 0; l < m.n_layers; ++l) {
    const pemp_layer& L = m.layer[l];
    const int KB = (L.in_dim + 15) >> 4, OB = (L.out_dim + 15) >> 4, ld = lds_stride(16 * KB);
    layer_lds(lds + off, ld, lds + off + 16 * OB * ld, KB, OB, L.relu, a, b);
    off += 16 * OB * ld + 16 * OB;
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
      for (int r = 0; r < 4; ++r) a[x][r] = b[x][r];
  }
}

// Node rows: one workgroup per 16-node tile (256 threads), producing x = X[:, 64:128] by mode and
// optionally the node / class heads on it (published widths <= 64, weights staged in LDS).
//   ROWS_EMBED: node embedding MLP -> X = [emb | emb] (NodeClassificationMPNSimple.py:67-69)
//   ROWS_SUM:   x_new = ReLU(b + sum_t y[n, t]), y[n, t] = U_t · agg[n, t] written by the edge pass
//               (UPD 1); empty (n, t) segments were never written and read as 0 (layers.py:253-258)
//   ROWS_COPY:  x_new = agg[n, 0] (MPLayer without an update MLP; empty segment -> 0)
//   ROWS_NONE:  x already in X (node_update_kernel ran): heads only
// Dynamic LDS (floats): xs [16][RS] | embed: act [2][16][RS] + staged embedding | heads.
enum { ROWS_NONE = 0, ROWS_EMBED = 1, ROWS_SUM = 2, ROWS_COPY = 3 };

struct NodeRowsArgs {
  int mode;
  const float* x_in;     // ROWS_EMBED: node inputs [N][in_ld]
  int in_ld;
  pemp_mlp emb;
  const float* agg;      // [N][T][64]
  const int* seg;
  int T;
  const float* upd_b;
  int64_t N;
  float* X;
  pemp_mlp node_head, class_head;
  int J;
  float *node_out, *node_out2, *class_out, *class_out2;
  const float* img;      // LDS image [emb | node head | class head] built by zero_words_kernel
  int head_off, head_floats;   // heads block: offset (= embedding image size, or 0) and size
  const int64_t* ne;     // capacity mode: device-side node count (N: the capacity); node_out / class_out are then
  int slot, dup;         // the bases of the logit arrays, the rows written are slot (and slot + 1 when dup) of N
  int emb_whole;         // ROWS_EMBED: the whole embedding image fits in LDS (one DMA up front)
};

static int max_layer_floats(const pemp_mlp& m) {
  int mx = 0;
  for (int l = 0; l < m.n_layers; ++l) {
    const int KB = (m.layer[l].in_dim + 15) >> 4, OB = (m.layer[l].out_dim + 15) >> 4;
    mx = std::max(mx, 16 * OB * lds_stride(16 * KB) + 16 * OB);
  }
  return mx;
}

constexpr int NODE_ROWS_LDS_MAX = 160 * 1024;

static bool node_emb_whole(const pemp_mlp& emb) {
  return (size_t)(3 * 16 * RS + mlp_lds_floats(emb)) * sizeof(float) <= (size_t)NODE_ROWS_LDS_MAX;
}

static size_t node_rows_lds_bytes(const NodeRowsArgs& a) {
  int region = 0;
  if (a.mode == ROWS_EMBED) region = a.emb_whole ? mlp_lds_floats(a.emb) : max_layer_floats(a.emb);
  if (a.node_out) region = std::max(region, a.head_floats);
  return (size_t)(3 * 16 * RS + region) * sizeof(float);
}

// 16-node tile bx over the workgroup's dynamic LDS (the body of node_rows_kernel, and a role of prelude_a_kernel)
__device__ __forceinline__ void node_rows_role(const NodeRowsArgs& a, float* lds, int bx) {
  float* xs = lds;
  float* act0 = lds + 16 * RS;
  float* act1 = act0 + 16 * RS;
  float* wreg = act1 + 16 * RS;                  // one embedding layer at a time, then the heads
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int64_t n0 = (int64_t)bx * 16, N = a.ne ? a.ne[0] : a.N;
  if (n0 >= N) return;   // (capacity grids)
  const bool heads = a.node_out != nullptr;
  float *node_out = a.node_out, *node_out2 = a.node_out2, *class_out = a.class_out, *class_out2 = a.class_out2;
  if (a.ne && heads) {   // capacity mode: rows slot (and slot + 1) of the device-side N
    node_out = a.node_out + (int64_t)a.slot * N;
    class_out = a.class_out + (int64_t)a.slot * N * a.J;
    node_out2 = a.dup ? node_out + N : nullptr;
    class_out2 = a.dup ? class_out + N * a.J : nullptr;
  }
  const int r = threadIdx.x >> 4, q = threadIdx.x & 15;   // row r of the tile, features 4 q .. 4 q + 3
  const int64_t n = n0 + r, nc = n < N ? n : N - 1;
  if (a.mode == ROWS_EMBED) {
    // whole image: every layer's weights in one DMA, in flight with the input rows (one latency
    // round instead of one per layer)
    const bool whole = a.emb_whole != 0;
    if (whole) dma_to_lds(wreg, a.img, mlp_lds_floats(a.emb));
    const int K0 = a.emb.layer[0].in_dim, KP = (K0 + 15) & ~15;
    for (int base = threadIdx.x; base < 16 * KP; base += 8 * 256) {   // 16 x K0 inputs, 8 loads in flight
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int idx = base + 256 * k, rr = idx / KP, kk = idx - rr * KP;
        v[k] = (idx < 16 * KP && kk < K0) ? a.x_in[min(n0 + rr, N - 1) * a.in_ld + kk] : 0.0f;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int idx = base + 256 * k, rr = idx / KP, kk = idx - rr * KP;
        if (idx < 16 * KP) act0[rr * RS + kk] = v[k];
      }
    }
    int cur = 0, off = 0;
    for (int l = 0; l < a.emb.n_layers; ++l) {
      const pemp_layer& L = a.emb.layer[l];
      const int KB = (L.in_dim + 15) >> 4, OB = (L.out_dim + 15) >> 4, ld = lds_stride(16 * KB);
      const int lf = 16 * OB * ld + 16 * OB;
      if (whole) {
        if (l == 0) lds_drain();
      } else {
        if (l > 0) __syncthreads();              // the previous layer is done with wreg
        copy_to_lds(wreg, a.img + off, lf);
      }
      __syncthreads();                           // layer l - 1's activations (and the weights) visible
      const float* Wl = whole ? wreg + off : wreg;
      off += lf;
      const float* bl = Wl + 16 * OB * ld;
      const float* src = cur ? act1 : act0;
      float* dst = cur ? act0 : act1;
      for (int ob = wave; ob < OB; ob += 4) {
        const float4 bb = ld4(bl + 16 * ob + 4 * g);
        f32x4 acc = {bb.x, bb.y, bb.z, bb.w};
        for (int mb = 0; mb < KB; ++mb) {
          const float4 w = ld4(Wl + (16 * ob + c) * ld + 16 * mb + 4 * g);
          const float4 xv = ld4(&src[c * RS + 16 * mb + 4 * g]);
          acc = mfma4(w.x, xv.x, acc);
          acc = mfma4(w.y, xv.y, acc);
          acc = mfma4(w.z, xv.z, acc);
          acc = mfma4(w.w, xv.w, acc);
        }
        if (L.relu) {
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] = fmaxf(acc[k], 0.0f);
        }
        st4(&dst[c * RS + 16 * ob + 4 * g], acc[0], acc[1], acc[2], acc[3]);
      }
      cur ^= 1;
    }
    __syncthreads();
    if (heads) dma_to_lds(wreg, a.img + a.head_off, a.head_floats);
    const float* res = cur ? act1 : act0;
    const float4 v = ld4(&res[r * RS + 4 * q]);
    *reinterpret_cast<float4*>(&xs[r * RS + 64 + 4 * q]) = v;
    if (n < N) {
      *reinterpret_cast<float4*>(a.X + n * 128 + 4 * q) = v;
      *reinterpret_cast<float4*>(a.X + n * 128 + 64 + 4 * q) = v;
    }
  } else {
    if (heads) dma_to_lds(wreg, a.img + a.head_off, a.head_floats);   // in flight with the row loads
    float4 v;
    if (a.mode == ROWS_SUM) {
      // all T rows and segment bounds in flight together; fixed summation order t = 0 .. T-1
      float4 y[MAXT];
      int s0[MAXT], s1[MAXT];
      const int T = a.T;
#pragma unroll
      for (int t = 0; t < MAXT; ++t) {
        const int tc = min(t, T - 1);
        y[t] = ld4(a.agg + (nc * T + tc) * D + 4 * q);
        s0[t] = a.seg[tc * N + nc];
        s1[t] = a.seg[tc * N + nc + 1];
      }
      v = ld4(a.upd_b + 4 * q);
#pragma unroll
      for (int t = 0; t < MAXT; ++t) {
        if (t < T && s1[t] > s0[t]) { v.x += y[t].x; v.y += y[t].y; v.z += y[t].z; v.w += y[t].w; }
      }
      v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
    } else if (a.mode == ROWS_COPY) {
      const float4 y = ld4(a.agg + nc * D + 4 * q);
      v = a.seg[nc + 1] > a.seg[nc] ? y : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      v = ld4(a.X + nc * 128 + 64 + 4 * q);
    }
    *reinterpret_cast<float4*>(&xs[r * RS + 64 + 4 * q]) = v;
    if (a.mode != ROWS_NONE && n < N) *reinterpret_cast<float4*>(a.X + n * 128 + 64 + 4 * q) = v;
  }
  if (!heads) return;
  lds_drain();
  __syncthreads();
  if (wave < 2) {   // wave 0: node head, wave 1: class head
    float in[4][4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
      const float4 x = ld4(&xs[c * RS + 64 + 16 * mb + 4 * g]);
      in[mb][0] = x.x; in[mb][1] = x.y; in[mb][2] = x.z; in[mb][3] = x.w;
    }
    const pemp_mlp& m = wave == 0 ? a.node_head : a.class_head;
    mlp_lds_frag(wave == 0 ? wreg : wreg + mlp_lds_floats(a.node_head), m, in);
    const int od = wave == 0 ? 1 : a.J;
    float* o1 = wave == 0 ? node_out : class_out;
    float* o2 = wave == 0 ? node_out2 : class_out2;
    const int64_t nn = n0 + c;
    if (nn < N) {
#pragma unroll
      for (int ob = 0; ob < 4; ++ob)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int f = 16 * ob + 4 * g + k;
          if (f < od) {
            o1[nn * od + f] = in[ob][k];
            if (o2) o2[nn * od + f] = in[ob][k];
          }
        }
    }
  }
}

__global__ __launch_bounds__(256) void node_rows_kernel(NodeRowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  node_rows_role(a, lds, blockIdx.x);
}

// Node table NT = [x0 | x] · pre_w^T + pre_b for the next edge pass. 1-D grid of
// (16 TILES-node chunk, 64-column group) workgroups, chunk-major; each of the 4 waves owns one 16-column
// block (weight fragment in registers, loaded before the barrier) and walks the chunk's TILES node
// tiles from LDS. L2 traffic ~ X · groups + pre_w · chunks: more tiles per chunk re-read the weights less, fewer
// give more workgroups to a launch that mostly runs beside the other batch's edge pass (TBL_TILES below).
// PREC 1: bf16x3 (pre_bf pack, K = 128 = 4 slot blocks).
struct NodeTableArgs {
  const float* X;
  int64_t N;
  const float *pre_w, *pre_b;
  const uint16_t* pre_bf;
  int NO, groups;
  float* NT;
  const int64_t* ne;   // capacity mode: device-side node count (N: the capacity)
  // SUM variant (node_table_kernel<PREC, 1, true>): the node update of the same step first, from the aggregates
  const float* agg;
  const int* seg;
  int T;
  const float* upd_b;
};

// the middle steps' node update runs inside the node-table launch while its aggregate re-reads (N T 256 B x column
// groups) stay below this many MB
constexpr int64_t NODE_SUM_TABLE_MAX_MB = 16;
// (1 / 2 / 4 / 8 measured: 2 gives the shortest isolated MPN, c3knn10 0.423-0.426 vs 0.435 ms with 4, c3 0.235 vs
// 0.239 ms; tools/experiments/round5/nn.sh)
constexpr int TBL_TILES = 2;           // 16-node tiles per workgroup

// SUM: the node update x = ReLU(b + sum_t agg[n, t]) (node_rows_kernel ROWS_SUM, same operations and order) is
// computed here for the tile's 16 rows, by every column group of the tile (the aggregates are re-read from L2 by
// each group instead of a separate launch writing x and this one reading it back); group 0 also stores x.
// block bx over xs [16 TILES][RS] of LDS (the body of node_table_kernel, and a role of prelude_b_kernel)
template <int PREC, int TILES, bool SUM>
__device__ __forceinline__ void node_table_role(const NodeTableArgs& a, float* xs, int bx) {
  static_assert(!SUM || TILES == 1, "the summing variant takes one 16-node tile per workgroup");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int chunk = bx / a.groups, grp = bx - chunk * a.groups;
  const int64_t n0 = (int64_t)chunk * 16 * TILES, N = a.ne ? a.ne[0] : a.N;
  if (n0 >= N) return;   // (capacity grids)
  const int nob = a.NO / 16, ob = grp * 4 + wave, obc = min(ob, nob - 1);
  // this wave's weight fragment (rows 16 ob + c), issued first
  float4 w[8];
  bf16x8_t wh[4], wlo[4];
  f16x8_t fh[4], flo[4];
  if (PREC == 0) {
#pragma unroll
    for (int mb = 0; mb < 8; ++mb) w[mb] = ld4(a.pre_w + (int64_t)(16 * obc + c) * 128 + 16 * mb + 4 * g);
  } else {
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      const int64_t o = (int64_t)(16 * obc + c) * 128 + 32 * kb + 8 * g;
      if (PREC == 1) {
        const __bf16* Wb = reinterpret_cast<const __bf16*>(a.pre_bf);
        wh[kb] = *reinterpret_cast<const bf16x8_t*>(Wb + o);
        wlo[kb] = *reinterpret_cast<const bf16x8_t*>(Wb + (int64_t)a.NO * 128 + o);
      } else {
        const _Float16* Wh = reinterpret_cast<const _Float16*>(a.pre_bf);
        fh[kb] = *reinterpret_cast<const f16x8_t*>(Wh + o);
        flo[kb] = *reinterpret_cast<const f16x8_t*>(Wh + (int64_t)a.NO * 128 + o);
      }
    }
  }
  const float4 bb = ld4(a.pre_b + 16 * obc + 4 * g);
  if constexpr (SUM) {
    // row r of the tile, features 4 q .. 4 q + 3: x0 and every type's aggregate and segment bounds in flight together
    const int r = threadIdx.x >> 4, q = threadIdx.x & 15;
    const int64_t n = n0 + r, nc = n < N ? n : N - 1;
    const int T = a.T;
    const float4 x0 = ld4(a.X + nc * 128 + 4 * q);
    float4 y[MAXT];
    int s0[MAXT], s1[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      const int tc = min(t, T - 1);
      y[t] = ld4(a.agg + (nc * T + tc) * D + 4 * q);
      s0[t] = a.seg[tc * N + nc];
      s1[t] = a.seg[tc * N + nc + 1];
    }
    float4 v = ld4(a.upd_b + 4 * q);
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      if (t < T && s1[t] > s0[t]) { v.x += y[t].x; v.y += y[t].y; v.z += y[t].z; v.w += y[t].w; }
    }
    v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
    *reinterpret_cast<float4*>(&xs[r * RS + 4 * q]) = x0;
    *reinterpret_cast<float4*>(&xs[r * RS + 64 + 4 * q]) = v;
    if (grp == 0 && n < N) *reinterpret_cast<float4*>(const_cast<float*>(a.X) + n * 128 + 64 + 4 * q) = v;
  } else {
  // X chunk -> LDS: 16 TILES rows x 32 float4, 2 TILES per thread
    float4 t[2 * TILES];
#pragma unroll
    for (int k = 0; k < 2 * TILES; ++k) {
      const int idx = threadIdx.x + 256 * k, row = idx >> 5, c4 = (idx & 31) * 4;
      const int64_t nn = min(n0 + row, N - 1);
      t[k] = ld4(a.X + nn * 128 + c4);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 2 * TILES; ++k) {
      const int idx = threadIdx.x + 256 * k, row = idx >> 5, c4 = (idx & 31) * 4;
      *reinterpret_cast<float4*>(&xs[row * RS + c4]) = t[k];
    }
  }
  __syncthreads();
  if (ob >= nob) return;
#pragma unroll
  for (int tile = 0; tile < TILES; ++tile) {
    const int64_t nn = n0 + 16 * tile + c;
    if (n0 + 16 * tile >= N) break;               // uniform
    float x[8][4];
#pragma unroll
    for (int mb = 0; mb < 8; ++mb) {
      const float4 v = ld4(&xs[(16 * tile + c) * RS + 16 * mb + 4 * g]);
      x[mb][0] = v.x; x[mb][1] = v.y; x[mb][2] = v.z; x[mb][3] = v.w;
    }
    f32x4 acc = {bb.x, bb.y, bb.z, bb.w};
    if (PREC == 0) {
#pragma unroll
      for (int mb = 0; mb < 8; ++mb) {
        acc = mfma4(w[mb].x, x[mb][0], acc);
        acc = mfma4(w[mb].y, x[mb][1], acc);
        acc = mfma4(w[mb].z, x[mb][2], acc);
        acc = mfma4(w[mb].w, x[mb][3], acc);
      }
    } else if (PREC == 1) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float (&xh)[4][4] = *reinterpret_cast<const float (*)[4][4]>(&x[4 * h][0]);
        bf16x8_t hi[2], lo[2];
        split_bf16(xh, hi, lo);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wlo[2 * h + kb], hi[kb], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[2 * h + kb], lo[kb], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[2 * h + kb], hi[kb], acc, 0, 0, 0);
        }
      }
    } else {
      // f16x3 over K = 128 (two 64-input halves, one range check for both); the table stays in the
      // 2^11 domain of the edge passes (the bias enters x 2^11, nothing is scaled on the way out)
      const float (&x0)[4][4] = *reinterpret_cast<const float (*)[4][4]>(&x[0][0]);
      const float (&x1)[4][4] = *reinterpret_cast<const float (*)[4][4]>(&x[4][0]);
      const float mx = fmaxf(frag_absmax(x0), frag_absmax(x1));
      const bool big = __any(!(mx < F16_BIG));
      const float ss = big ? f16_item_scale(mx, 1.0f) : 1.0f;   // the node's range factor (1 in range)
      acc *= 2048.0f * ss;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        f16x8_t hi[2], lo[2];
        const float (&xh)[4][4] = h ? x1 : x0;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
          uint32_t hw[4], lw[4];
#pragma unroll
          for (int d = 0; d < 4; ++d)
            split_pair(xh[2 * kb + (d >> 1)][2 * (d & 1)], xh[2 * kb + (d >> 1)][2 * (d & 1) + 1], ss, hw[d], lw[d]);
          const u32x4_t hv = {hw[0], hw[1], hw[2], hw[3]}, lv = {lw[0], lw[1], lw[2], lw[3]};
          hi[kb] = __builtin_bit_cast(f16x8_t, hv);
          lo[kb] = __builtin_bit_cast(f16x8_t, lv);
        }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
          acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(flo[2 * h + kb], hi[kb], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(fh[2 * h + kb], lo[kb], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(fh[2 * h + kb], hi[kb], acc, 0, 0, 0);
        }
      }
      if (big) acc *= 1.0f / ss;
    }
    if (nn < N) st4(a.NT + nn * a.NO + 16 * ob + 4 * g, acc[0], acc[1], acc[2], acc[3]);
  }
}

template <int PREC, int TILES = TBL_TILES, bool SUM = false>
__global__ __launch_bounds__(256) void node_table_kernel(NodeTableArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[16 * TILES * RS];
  node_table_role<PREC, TILES, SUM>(a, xs, blockIdx.x);
}

// Launch B of the paired prelude (Forward::prelude): the wave ranges and segment positions of the edge order
// (blocks [0, split), edge_ranges_role) beside the first node table (blocks [split, gridDim.x), node_table_role).
// Both read what launch A and the launches before it wrote and nothing of each other; no workgroup waits for
// another. The range blocks come first: each is one chain of dependent loads as long as the whole role, the table's
// are many and short.
template <int PREC>
__global__ __launch_bounds__(256) void prelude_b_kernel(EdgeRangesArgs ra, NodeTableArgs ta, int split) {
  __shared__ __attribute__((aligned(16))) float xs[16 * TBL_TILES * RS];
  const int bx = blockIdx.x;   // (block-uniform dispatch)
  if (bx < split) edge_ranges_role(ra, bx);
  else node_table_role<PREC, TBL_TILES, false>(ta, xs, bx - split);
}

static bool published_head(const pemp_mlp& m) {
  return m.n_layers == 3 && m.layer[0].in_dim == 64 && m.layer[0].out_dim == 64 && m.layer[0].relu &&
         m.layer[1].in_dim == 64 && m.layer[1].out_dim == 32 && m.layer[1].relu && m.layer[2].in_dim == 32 &&
         m.layer[2].out_dim == 1 && !m.layer[2].relu;
}

template <int AGG, int PREC, int UPD, int STAGE>
static void launch_edge_step_s(const EdgeStepArgs& a, bool head, bool pub, int grid, hipStream_t st) {
  if (!head)
    hipLaunchKernelGGL((edge_step_kernel<AGG, 0, PREC, UPD, STAGE>), dim3(grid), dim3(64 * edge_waves<0>()), 0, st, a);
  else if (pub)
    hipLaunchKernelGGL((edge_step_kernel<AGG, 1, PREC, UPD, STAGE>), dim3(grid), dim3(64 * edge_waves_s<1, STAGE>()), 0,
                       st, a);
  else
    hipLaunchKernelGGL((edge_step_kernel<AGG, 2, PREC, UPD, STAGE>), dim3(grid), dim3(64 * edge_waves<2>()), 0, st, a);
}

template <int AGG, int PREC, int UPD>
static void launch_edge_step_p(const EdgeStepArgs& a, bool head, bool pub, int grid, int stage, hipStream_t st) {
  if constexpr (AGG == PEMP_AGGR_ATTN) {          // EDGE_MLP per_type: the published configs use attention
    if (stage == (STAGE_MID | STAGE_EPT)) { launch_edge_step_s<AGG, PREC, UPD, STAGE_MID | STAGE_EPT>(a, head, pub, grid, st); return; }
    if (stage == (STAGE_LAST | STAGE_EPT)) { launch_edge_step_s<AGG, PREC, UPD, STAGE_LAST | STAGE_EPT>(a, head, pub, grid, st); return; }
  }
  if (stage == STAGE_MID) launch_edge_step_s<AGG, PREC, UPD, STAGE_MID>(a, head, pub, grid, st);
  else launch_edge_step_s<AGG, PREC, UPD, STAGE_LAST>(a, head, pub, grid, st);
}

// whether the edge passes pre-apply the update block (UPD) and carry the published head (HEAD 1)
static bool edge_upd_fused(const pemp_mpn_desc& d, const pemp_mpn_weights& w) {
  return (d.aggr == PEMP_AGGR_ATTN || d.aggr == PEMP_AGGR_MEAN) && w.upd_w && (d.precision == PEMP_PREC_FP32 || w.upd_bf);
}
static bool edge_pub_head(const pemp_mpn_desc& d, const pemp_mpn_weights& w) {
  return published_head(w.edge_head) && (d.precision == PEMP_PREC_FP32 || w.head_bf);
}
// the edge embedding's arithmetic (ForwardPlan::emb_prec) and where its LDS image follows the passes' image
static int embed_prec(const pemp_mpn_desc& d, const pemp_mpn_weights& w) {
  return d.precision != PEMP_PREC_FP32 && w.emb_bf ? d.precision : PEMP_PREC_FP32;
}
static size_t edge_image_base_floats(const pemp_mpn_desc& d, const pemp_mpn_weights& w) {
  return (size_t)d.num_types * img_stride(edge_upd_fused(d, w), edge_pub_head(d, w));
}
static size_t embed_image_offset(const pemp_mpn_desc& d, const pemp_mpn_weights& w) {
  return (edge_image_base_floats(d, w) + 63) & ~(size_t)63;
}

static EdgeImgArgs edge_image_args(const pemp_mpn_desc& d, const pemp_mpn_weights& w, bool upd, bool head, float* img) {
  EdgeImgArgs a{};
  a.T = d.num_types; a.prec = d.precision; a.upd = upd ? 1 : 0; a.head = head ? 1 : 0; a.aggr = d.aggr;
  a.e1_w = w.e1_w; a.e2_w = w.e2_w; a.e2_b = w.e2_b; a.msg_w = w.msg_w; a.attn_w = w.attn_w; a.attn_bv = w.attn_bv;
  a.upd_w = w.upd_w; a.attn_b = w.attn_b;
  a.e1_bf = w.e1_bf; a.e2_bf = w.e2_bf; a.msg_bf = w.msg_bf; a.upd_bf = w.upd_bf; a.head_bf = w.head_bf;
  a.head_mlp = w.edge_head;
  a.img = img;
  return a;
}

// The one dispatch from a run-time PEMP_PREC_* to a template argument: f(std::integral_constant<int, PREC>{}).
template <class F>
static void with_prec(int prec, F&& f) {
  if (prec == PEMP_PREC_F16X3) f(std::integral_constant<int, PEMP_PREC_F16X3>{});
  else if (prec == PEMP_PREC_BF16X3) f(std::integral_constant<int, PEMP_PREC_BF16X3>{});
  else f(std::integral_constant<int, PEMP_PREC_FP32>{});
}

// UPD is instantiated for the linear aggregations only (U · max(m) != max(U · m))
// -DPEMP_STAMPS builds: the pass chosen through pemp_diag_stamps records its phase stamps
static void set_stamps(EdgeStepArgs& a, int pass) {
#ifdef PEMP_STAMPS
  a.stamps = pass == g_diag_stamp_pass ? g_diag_stamps : nullptr;
#else
  (void)a;
  (void)pass;
#endif
}

// `pass`: the iteration (for the phase stamps)
template <int AGG>
static void launch_edge_step(EdgeStepArgs a, int pass, bool head, bool pub, int grid, int prec, bool upd, int stage,
                             hipStream_t st) {
  set_stamps(a, pass);
  constexpr int U = AGG == PEMP_AGGR_ATTN || AGG == PEMP_AGGR_MEAN ? 1 : 0;
  with_prec(prec, [&](auto P) {
    if (U && upd) launch_edge_step_p<AGG, decltype(P)::value, U>(a, head, pub, grid, stage, st);
    else launch_edge_step_p<AGG, decltype(P)::value, 0>(a, head, pub, grid, stage, st);
  });
}

// embedding + pass 0 in one launch (edge_step_kernel STAGE_FIRST)
static void launch_edge_first(EdgeStepArgs a, int pass, int grid, hipStream_t st) {
  set_stamps(a, pass);
  hipLaunchKernelGGL((edge_step_kernel<PEMP_AGGR_ATTN, 0, 2, 1, STAGE_MID | STAGE_FIRST>), dim3(grid),
                     dim3(64 * EDGE_WAVES), 0, st, a);
}

static int rows_mlp(const char* label, const pemp_mlp& m, const float* in, int64_t ld_in, int64_t M, float* out,
                    int64_t ld_out, float* out2, int64_t ld_out2, hipStream_t st) {
  if (M <= 0) return PEMP_OK;
  ProfScope prof(label, st);
  RowsMlpArgs a{m, in, ld_in, M, out, ld_out, out2, ld_out2};
  hipLaunchKernelGGL(rows_mlp_kernel, dim3((unsigned)((M + 15) / 16)), dim3(256), 0, st, a);
  PEMP_LAUNCH_CHECK();
  return PEMP_OK;
}

static bool mlp_ok(const pemp_mlp& m, int in_max, int width_max) {
  if (m.n_layers < 1 || m.n_layers > 4) return false;
  for (int l = 0; l < m.n_layers; ++l) {
    const pemp_layer& L = m.layer[l];
    if (!L.w || !L.b || L.in_dim <= 0 || L.out_dim <= 0) return false;
    if (L.in_dim > (l == 0 ? in_max : width_max) || L.out_dim > width_max) return false;
    if (l > 0 && L.in_dim != m.layer[l - 1].out_dim) return false;
  }
  return true;
}

static bool node_heads_fused(const pemp_mpn_weights& w) { return mlp_ok(w.node_head, 64, 64) && mlp_ok(w.class_head, 64, 64); }
static bool node_embed_fused(const pemp_mpn_weights& w) { return mlp_ok(w.node_emb, 128, 128); }   // one layer at a time in LDS

// floats of the image (the LDS layouts of mlp_lds_floats, [emb | node head | class head])
static size_t node_image_extent(const pemp_mpn_weights& w) {
  size_t n = node_embed_fused(w) ? mlp_lds_floats(w.node_emb) : 0;
  if (node_heads_fused(w)) n += mlp_lds_floats(w.node_head) + mlp_lds_floats(w.class_head);
  return n;
}

static StagePlan node_image_plan(const pemp_mpn_weights& w) {
  const bool heads = node_heads_fused(w);
  return stage_plan(node_embed_fused(w) ? &w.node_emb : nullptr, heads ? &w.node_head : nullptr,
                    heads ? &w.class_head : nullptr);
}

// Launch A of the paired prelude (Forward::prelude): the closed-form edge order (blocks [0, split): block x of gx
// of image y at y gx + x, fully_prepare_role) beside the node embedding (blocks [split, gridDim.x): one 16-node tile
// each, node_rows_role in ROWS_EMBED mode). Both read the call's inputs and what earlier launches wrote, nothing of
// each other; no workgroup waits for another. The order's blocks come first: its chain (order -> ranges) feeds the
// larger consumer and its blocks are the longer ones. Dynamic LDS: the larger of the two roles' (prelude_a_lds_bytes).
__global__ __launch_bounds__(256) void prelude_a_kernel(FullyPrepArgs fa, NodeRowsArgs na, int split, int gx) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int bx = blockIdx.x;   // (block-uniform dispatch)
  if (bx < split) fully_prepare_role(fa, *reinterpret_cast<FullyPrepLds*>(lds), bx % gx, bx / gx, gx);
  else node_rows_role(na, lds, bx - split);
}

static size_t prelude_a_lds_bytes(const NodeRowsArgs& na) {
  return std::max(node_rows_lds_bytes(na), sizeof(FullyPrepLds));
}

}  // namespace
}  // namespace pemp

using namespace pemp;

#ifdef PEMP_STAMPS
// diagnostic builds (the state sits beside EDGE_STAMP): which pass of every forward records its phase stamps, and where
extern "C" int pemp_diag_stamps(void* buf, int pass) {
  g_diag_stamps = static_cast<unsigned long long*>(buf);
  g_diag_stamp_pass = pass;
  return PEMP_OK;
}
#endif

extern "C" size_t pemp_mpn_workspace_size(const pemp_mpn_desc* desc, int64_t N, int64_t E) {
  if (!desc || N < 0 || E < 0 || desc->num_types < 1) return 0;
  size_t bytes = 0;
  mpn_carve(nullptr, desc->num_types, N, E, &bytes);
  return bytes;
}

// (Exact forwards launch directly: a HIP-graph replay of repeated identical exact forwards measured slower (the
// isolated forward 0.252 vs 0.242 ms, re-captured whenever N / E or the allocator's buffers change). The
// capacity-mode forward, whose arguments repeat from step to step, is replayed from a graph:
// pemp_mpn_forward_fully_cap.)
// ---- the inference forward: what a call is given (ForwardCall), its argument checks, everything derived from it
// on the host (ForwardPlan), and the launches (Forward) ------------------------------------------------------------
// where the type-major edge order of a forward comes from
struct EdgeOrder {
  enum Kind { SORT, FULLY, SYM, KNN } kind = SORT;   // SORT: the sorting prepare on edge_index (launch_prepare)
  // FULLY: edge_index is the fully graph of the batch with these per-image node offsets (device, [B + 1]) -> the
  // closed-form prepare (fully_prepare_kernel); nmax bounds the nodes of one image
  const int64_t* node_off = nullptr;
  int B = 0, nmax = 0;
  const KnnPrepArgs* knn = nullptr;   // KNN: the graph build's row lists (knn_prepare_kernel)
};

// capacity mode (pemp_mpn_forward_fully_cap): N and E are capacities; the device-side counts ne = (N, E, overflow) are
// the capacity graph build's, after its node offsets. A batch past any capacity (an image over the detection
// capacity, N > n_cap or E > e_cap: the build wrote nothing) has (0, 0, 1), and every kernel of the forward then
// runs empty.
struct CapMode {
  const int64_t* ne = nullptr;   // device; NULL: an exact forward
};

struct ForwardCall {
  const pemp_mpn_desc* desc;
  const pemp_mpn_weights* w;
  const float *x, *edge_attr;
  const int64_t *edge_index, *node_types;
  int64_t N, E;
  float *edge_logits, *node_logits, *class_logits;   // bases of the three logit arrays
  void* workspace;
  size_t workspace_bytes;
  void* stream;
  EdgeOrder order;
  CapMode cap;
};

static int check_forward_args(const ForwardCall& c) {
  const pemp_mpn_desc* desc = c.desc;
  const pemp_mpn_weights* w = c.w;
  PEMP_CHECK_ARG(desc && w, "pemp_mpn_forward: null desc/weights");
  const int T = desc->num_types, J = desc->num_joints;
  const int64_t N = c.N, E = c.E;
  PEMP_CHECK_ARG(desc->hidden == 64, "pemp_mpn_forward: hidden width must be 64 (got %d)", desc->hidden);
  PEMP_CHECK_ARG(T >= 1 && T <= MAXT, "pemp_mpn_forward: num_types must be in [1, %d]", MAXT);
  // (the edge passes address r, Q0 and the aggregates with 32-bit byte offsets: E, T N < 2^23; the sorted target
  // list carries each edge's segment position above its node id, MPN_MAX_NODES)
  PEMP_CHECK_ARG(N >= 0 && E >= 0 && N < MPN_MAX_NODES && E < (1ll << 23) && (int64_t)T * N < (1ll << 23),
                 "pemp_mpn_forward: N=%lld E=%lld out of range (N, E and num_types * N must stay below 2^23)",
                 (long long)N, (long long)E);
  PEMP_CHECK_ARG(desc->steps >= 0 && desc->aux_loss_steps >= 0, "pemp_mpn_forward: bad steps");
  PEMP_CHECK_ARG(desc->aggr >= PEMP_AGGR_ATTN && desc->aggr <= PEMP_AGGR_MAX, "pemp_mpn_forward: bad aggr");
  PEMP_CHECK_ARG(desc->aggr != PEMP_AGGR_ATTN || w->attn_w, "pemp_mpn_forward: attention needs attn_w");
  if (w->ept_l1_w) {   // EDGE_MLP per_type
    PEMP_CHECK_ARG(w->ept_l1_b && w->ept_l2_w && w->ept_l2_b && w->ept_o1_w && w->ept_o2_w,
                   "pemp_mpn_forward: EDGE_MLP per_type needs every ept_* array");
    if (desc->aggr != PEMP_AGGR_ATTN) {
      set_error("pemp_mpn_forward: EDGE_MLP per_type is built for the attention aggregation");
      return PEMP_ERR_UNSUPPORTED;
    }
  }
  if (w->upd_mlp.n_layers > 0) {   // hierarchical update (dense-folded): T*64 -> ... -> 64, widths % 16
    const pemp_mlp& m = w->upd_mlp;
    PEMP_CHECK_ARG(!w->upd_w && m.n_layers <= 4, "pemp_mpn_forward: upd_mlp excludes upd_w (<= 4 layers)");
    for (int l = 0; l < m.n_layers; ++l) {
      const pemp_layer& ly = m.layer[l];
      PEMP_CHECK_ARG(ly.w && ly.b && ly.in_dim % 16 == 0 && ly.out_dim % 16 == 0 && ly.out_dim > 0 &&
                         ly.in_dim == (l == 0 ? 64 * desc->num_types : m.layer[l - 1].out_dim),
                     "pemp_mpn_forward: upd_mlp layer %d is %d -> %d", l, ly.in_dim, ly.out_dim);
    }
    PEMP_CHECK_ARG(m.layer[m.n_layers - 1].out_dim == 64, "pemp_mpn_forward: upd_mlp must end at 64");
    PEMP_CHECK_ARG(nmlp_lds_bytes(desc->num_types, m) <= 160 * 1024, "pemp_mpn_forward: upd_mlp too wide");
  }
  PEMP_CHECK_ARG(mlp_ok(w->node_emb, 128, 128) && w->node_emb.layer[w->node_emb.n_layers - 1].out_dim == 64 &&
                     w->node_emb.layer[0].in_dim == desc->node_in_dim,
                 "pemp_mpn_forward: node embedding must map node_in_dim (<=128) -> 64");
  PEMP_CHECK_ARG(mlp_ok(w->edge_emb, 128, 128) && w->edge_emb.layer[w->edge_emb.n_layers - 1].out_dim == 64 &&
                     w->edge_emb.layer[0].in_dim == desc->edge_attr_dim,
                 "pemp_mpn_forward: edge embedding must map edge_attr_dim (<=128) -> 64");
  PEMP_CHECK_ARG(mlp_ok(w->edge_head, 64, 64) && w->edge_head.layer[0].in_dim == 64 &&
                     w->edge_head.layer[w->edge_head.n_layers - 1].out_dim == 1,
                 "pemp_mpn_forward: edge head must map 64 -> 1 with widths <= 64");
  PEMP_CHECK_ARG(mlp_ok(w->node_head, 64, 128) && mlp_ok(w->class_head, 64, 128) &&
                     w->class_head.layer[w->class_head.n_layers - 1].out_dim == J,
                 "pemp_mpn_forward: node/class heads must start at 64 and end at 1 / num_joints");
  PEMP_CHECK_ARG(w->pre_w && w->pre_b && w->q0_w && w->q0_b && w->e1_w && w->e2_w && w->e2_b && w->msg_w,
                 "pemp_mpn_forward: null layer weights");
  PEMP_CHECK_ARG(desc->precision == PEMP_PREC_FP32 || desc->precision == PEMP_PREC_BF16X3 ||
                     desc->precision == PEMP_PREC_F16X3,
                 "pemp_mpn_forward: unknown precision %d", desc->precision);
  PEMP_CHECK_ARG(desc->precision == PEMP_PREC_FP32 ||
                     (w->e1_bf && w->e2_bf && w->msg_bf && w->pre_bf && (w->emb_bf || !mlp_ok(w->edge_emb, 64, 64))),
                 "pemp_mpn_forward: split precisions need the e1_bf / e2_bf / msg_bf / pre_bf / emb_bf weight packs");
  PEMP_CHECK_ARG(N == 0 || (c.x && c.node_logits && c.class_logits && c.node_types),
                 "pemp_mpn_forward: null node tensors");
  PEMP_CHECK_ARG(E == 0 || (c.edge_attr && (c.edge_index || c.order.kind == EdgeOrder::FULLY) && c.edge_logits),
                 "pemp_mpn_forward: null edge tensors");
  size_t need = 0;
  mpn_carve(nullptr, T, N, E, &need);
  if (c.workspace_bytes < need) {
    set_error("pemp_mpn_forward: workspace %zu < %zu bytes", c.workspace_bytes, need);
    return PEMP_ERR_WORKSPACE;
  }
  return PEMP_OK;
}

// how the node update of an iteration runs (node_step's mode: a ROWS_* mode of node_rows_kernel, or the update MLP
// in a launch of its own ahead of it)
constexpr int NODE_UPDATE_MLP = -1;

// The grids of the prelude's four kernels (order, node embedding, wave ranges, first node table) and, for the paired
// form (Forward::prelude), the block at which the second role starts in each of its two launches. Eight ints in this
// order: pemp_mpn_prelude_grids.
struct PreludeGrids {
  int prep_gx;                    // fully_prepare in a launch of its own: blocks per image (x B images)
  int a_gx;                       // ... and in launch A (see below)
  int rows_blocks;                // node embedding: 16-node tiles
  int a_split;                    // launch A: [0, a_split = a_gx B) the order, then rows_blocks of the embedding
  int ranges_rb, ranges_blocks;   // edge_ranges: range-table blocks, and all blocks (none without edges)
  int table_blocks;               // node table: 16 TBL_TILES-node chunks x column groups
  int b_split;                    // launch B: [0, b_split) the ranges, [b_split, b_split + table_blocks) the table
};

// B images of at most nmax nodes (0: no closed-form order), G workgroups per edge pass, a device of `cus` CUs.
// Every block of launch A asks for the node embedding's LDS (the whole embedding image, ~121 KB at the published
// shape), so a CU holds one of them at a time, where it holds several blocks of the order's own launch. The order's
// share is therefore cut down to the CUs the embedding leaves (its segment loop strides by the grid: the same
// arrays from any grid, and every block repeats the per-batch counts, so fewer blocks do less in all). Where the
// embedding's tiles alone fill the device (N > 16 cus) the order keeps one block per image and the launch's blocks
// run in rounds, in block order: the order's first, then the embedding's as CUs come free -- slower than the two
// launches side by side would be, still correct: no block waits for another.
static PreludeGrids prelude_grids(int64_t N, int64_t E, int B, int T, int nmax, int G, int cus) {
  PreludeGrids g{};
  // FULLY_PARTS threads per (type, target) segment (a per-edge mapping with binary searches measured 41 us
  // vs 15 us at C3)
  g.prep_gx = (int)std::max<int64_t>(1, std::min<int64_t>(64, ((int64_t)T * nmax * FULLY_PARTS + 511) / 512));
  g.rows_blocks = (int)((N + 15) / 16);
  g.a_gx = B > 0 ? std::max(1, std::min(g.prep_gx, (cus - g.rows_blocks) / B)) : g.prep_gx;
  g.a_split = g.a_gx * B;
  if (E > 0) {
    g.ranges_rb = std::min(64, (G * (EDGE_WAVES + 12) + 255) / 256);
    g.ranges_blocks = g.ranges_rb + (int)std::min<int64_t>(1024, (E + 255) / 256);
  }
  const int groups = ((128 + 64 * T) / 16 + 3) / 4;
  g.table_blocks = (int)(((N + 16 * TBL_TILES - 1) / (16 * TBL_TILES)) * groups);
  g.b_split = g.ranges_blocks;
  return g;
}

// Everything a forward derives from its call on the host, each value once. Nothing here launches.
struct ForwardPlan {
  int T, J, steps, aux;
  int64_t tstride;        // node_types may be a strided view
  bool upd_fused;         // U_t pre-applied in the edge pass: the node update is a sum (edge_upd_fused)
  bool pub_head;          // the published head's weights ride in the passes' LDS image
  bool ept;               // EDGE_MLP per_type
  // the edge embedding: in LDS (else the `wide` kernel, weights from global memory), its arithmetic and LDS layout,
  // and which form of the LDS kernel runs (`generic`: the runtime-shaped form for a shape off the fixed layout -- no
  // precision has a straight-line kernel for it)
  bool emb_lds, emb_generic, comp, fixed;
  int emb_prec;
  EmbedLayout emb_lo;
  bool fused_heads, fused_embed;   // the node / class heads and the node embedding inside node_rows_kernel
  int edge_grid;                   // workgroups of the edge passes (and of the prepares' per-workgroup split)
  int NO, table_prec, table_groups;
  unsigned node_grid, table_grid, table_grid1;
  int node_mode;
  bool sum_in_table;    // middle steps: the node update inside the node-table launch (node_step)
  bool fused_first;
  PreludeGrids grids;
  bool paired;          // the prelude as two launches of two roles each (Forward::prelude)
};

static ForwardPlan plan_forward(const ForwardCall& c) {
  const pemp_mpn_desc& d = *c.desc;
  const pemp_mpn_weights& w = *c.w;
  const int64_t N = c.N, E = c.E;
  ForwardPlan p{};
  p.T = d.num_types; p.J = d.num_joints; p.steps = d.steps; p.aux = d.aux_loss_steps;
  p.tstride = d.types_stride > 0 ? d.types_stride : 1;
  // U_t pre-applied in the edge pass (linear aggregations with an update MLP): the node update is a sum
  // (ATTN / MEAN only: for the unnormalised SUM the reordered fp32 rounding of sum_e U m_e vs
  // U sum_e m_e grows with the in-degree past the logit tolerance)
  p.upd_fused = edge_upd_fused(d, w);
  p.pub_head = edge_pub_head(d, w);
  p.ept = w.ept_l1_w != nullptr;
  p.emb_lds = mlp_ok(w.edge_emb, 64, 64);
  p.emb_prec = embed_prec(d, w);
  p.emb_lo = embed_layout(w.edge_emb, p.emb_prec);
  p.emb_generic = p.emb_lds && !embed_fixed_shape(p.emb_prec == PEMP_PREC_FP32
                                                      ? embed_layout(w.edge_emb, PEMP_PREC_F16X3)
                                                      : p.emb_lo);
  p.fixed = embed_fixed_shape(p.emb_lo);
  p.comp = embed_composed(p.emb_lo, p.emb_prec, w);
  p.fused_heads = node_heads_fused(w);
  p.fused_embed = node_embed_fused(w);   // (embedding widths > 128 would not fit the node step's LDS rows)
  p.edge_grid = std::max(edge_cus(E), p.T);   // >= wg_start[T] (see mpn_scan_kernel)
  p.NO = 128 + 64 * p.T;
  p.table_prec = d.precision != PEMP_PREC_FP32 && w.pre_bf ? d.precision : PEMP_PREC_FP32;
  p.table_groups = (p.NO / 16 + 3) / 4;
  p.grids = prelude_grids(N, E, c.order.kind == EdgeOrder::FULLY ? c.order.B : 0, p.T, c.order.nmax, p.edge_grid,
                          num_cus());
  p.node_grid = (unsigned)p.grids.rows_blocks;
  p.table_grid = (unsigned)p.grids.table_blocks;
  p.table_grid1 = (unsigned)(((N + 15) / 16) * p.table_groups);
  p.node_mode = p.upd_fused ? ROWS_SUM : (w.upd_w || w.upd_mlp.n_layers > 0) ? NODE_UPDATE_MLP : ROWS_COPY;
  // (every column group re-reads the tile's aggregates: worth it while those re-reads stay small -- C2 -- not at
  // C3, where they are ~100 MB per call and the fused launch only ties the two it replaces. Round 6: a wide form,
  // 16 waves = 256 columns per workgroup so a tile's aggregates are summed 5 instead of 19 times, took 24 us per
  // call against 8 + 10 us for the two launches at c3 / c3knn10 (profiles/r06_node_sum_wide.md); not kept.)
  p.sum_in_table = !p.ept && N * p.T * 256 * (int64_t)p.table_groups <= NODE_SUM_TABLE_MAX_MB << 20;
  // The fused first pass (edge_step_kernel STAGE_FIRST) replaces the embedding launch and pass 0 where pass 0 is a
  // plain middle pass of the published composed shape: f16x3, attention with the update block pre-applied, no
  // per-type edge MLP, the caller's composed packs and prebuilt image, steps >= 2 and pass 0 not recorded. Every other
  // case, a profiler repeat of the passes and PEMP_MPN_TWO_LAUNCH_FIRST keep the two launches -- and so does a forward
  // the library profiler records (its per-kernel labels stay those of the separate kernels) unless the caller asks for
  // the fused pass there too (PEMP_MPN_FUSED_FIRST_PROFILED). R0's buffer (ws.EA) is then not touched.
  p.fused_first = E > 0 && p.steps >= 2 && p.steps - p.aux - 1 > 0 && !(d.flags & PEMP_MPN_TWO_LAUNCH_FIRST) &&
                  d.precision == PEMP_PREC_F16X3 && d.aggr == PEMP_AGGR_ATTN && p.upd_fused && !p.ept &&
                  p.emb_lds && p.comp && w.edge_img &&
                  prof_repeat("edge_step") == 1 &&
                  (!prof_active() || (d.flags & PEMP_MPN_FUSED_FIRST_PROFILED));
  // The paired prelude: the closed-form order beside the node embedding, then the wave ranges beside the first node
  // table. The separate launches stay for the other prepares (several launches each), embedding widths that take
  // rows_mlp, a forward without iterations, one the library profiler records (its labels are those of the separate
  // kernels) and PEMP_MPN_SEPARATE_PRELUDE.
  p.paired = c.order.kind == EdgeOrder::FULLY && !(d.flags & (PEMP_MPN_PREPARED | PEMP_MPN_SEPARATE_PRELUDE)) &&
             p.fused_embed && p.steps >= 1 && !prof_active();
  return p;
}

// The launches of one forward. Every member function enqueues and returns a PEMP_* code.
struct Forward {
  const ForwardCall& c;
  const ForwardPlan& p;
  const MpnWs ws;
  const hipStream_t st;       // the launch stream
  const int64_t* ne = nullptr;      // capacity mode: the device-side {N, E}
  const float* node_img = nullptr;  // LDS image of the node-side MLPs
  const float* eimg = nullptr;      // the edge-pass weight image
  float* r_cur;               // r of the pass (R0 from the separate embedding)
  float* r_next;
  int rec = 0;                // recorded iterations so far

  Forward(const ForwardCall& call, const ForwardPlan& plan)
      : c(call), p(plan), ws(mpn_carve(call.workspace, plan.T, call.N, call.E, nullptr)), st(as_stream(call.stream)),
        r_cur(ws.EA), r_next(ws.EB) {}

  bool recorded(int it) const { return it >= p.steps - p.aux - 1; }
  bool last(int it) const { return it + 1 == p.steps; }

  // what comes ahead of everything else on the launch stream: the two weight images where the caller did not
  // prebuild them
  int launch_setup() {
    const pemp_mpn_weights& w = *c.w;
    ne = c.cap.ne;
    // LDS image of the node-side MLPs: the caller's (pemp_mpn_node_image) or built here
    node_img = w.node_img;
    if (!node_img && (p.fused_heads || p.fused_embed)) {
      const StagePlan plan = node_image_plan(w);
      hipLaunchKernelGGL(stage_image_kernel, dim3((unsigned)std::min(64, (plan.total + 255) / 256)), dim3(256), 0, st,
                         plan, ws.img);
      PEMP_LAUNCH_CHECK();
      node_img = ws.img;
    }
    // the edge-pass weight image: the caller's (pemp_mpn_edge_image, built once per weight set) or built here
    eimg = w.edge_img;
    if (!eimg && c.E > 0 && p.steps >= 1) {
      EdgeImgArgs ia = edge_image_args(*c.desc, w, p.upd_fused, p.pub_head, ws.eimg);
      hipLaunchKernelGGL(edge_image_kernel, dim3(16, (unsigned)p.T), dim3(256), 0, st, ia);
      PEMP_LAUNCH_CHECK();
      eimg = ws.eimg;
    }
    return PEMP_OK;
  }

  // the type-major edge order (unless the caller prepared it: PEMP_MPN_PREPARED)
  int launch_order() {
    if (c.desc->flags & PEMP_MPN_PREPARED) return PEMP_OK;
    switch (c.order.kind) {
      case EdgeOrder::FULLY: {
        const FullyPrepArgs fa = fully_args();
        ProfScope prof("mpn_prepare_fully", st);
        return launch_prepare_fully(fa, p.grids.prep_gx, st);
      }
      case EdgeOrder::KNN: {
        KnnPrepArgs ka = *c.order.knn;
        ka.types = c.node_types; ka.ts = p.tstride; ka.N = c.N; ka.E = c.E; ka.T = p.T; ka.G = p.edge_grid;
        ka.seg = ws.seg; ka.wg_start = ws.wg_start; ka.s_src = ws.s_src; ka.s_dst = ws.s_dst; ka.s_orig = ws.s_orig;
        ka.err = ws.err;
        ProfScope prof("mpn_prepare_knn", st);
        return launch_prepare_knn(ka, st);
      }
      case EdgeOrder::SYM: return launch_prepare_sym(c.desc, c.edge_index, c.node_types, c.N, c.E, ws, st);
      default: return launch_prepare(c.desc, c.edge_index, c.node_types, c.N, c.E, ws, st);
    }
  }

  FullyPrepArgs fully_args() const {
    return FullyPrepArgs{c.order.node_off, c.order.B, c.node_types, p.tstride, c.N, p.T, p.edge_grid,
                         ws.seg, ws.wg_start, ws.s_src, ws.s_dst, ws.s_orig, ws.err, ne};
  }

  // the passes' per-wave range table (static across iterations), right behind the order: its chains of dependent
  // small loads stay off the edge embedding's workgroups
  int launch_ranges() {
    if (c.E == 0 || p.steps < 1) return PEMP_OK;
    const EdgeRangesArgs ra = ranges_args();
    hipLaunchKernelGGL(edge_ranges_kernel, dim3((unsigned)ra.blocks), dim3(256), 0, st, ra);
    PEMP_LAUNCH_CHECK();
    return PEMP_OK;
  }

  // (behind the range table's blocks: the per-edge segment positions, one edge per thread)
  EdgeRangesArgs ranges_args() const {
    return EdgeRangesArgs{ws.seg, ws.wg_start, ws.s_dst, p.T, c.N, p.edge_grid, ws.ranges, ne, p.grids.ranges_rb,
                          p.grids.ranges_blocks};
  }

  // ---- edge embedding: its own launch writes Q0 and R0 = Q0 + W1_e_cur · e_init (edge_embed_kernel;
  // the published shape takes the straight-line edge_embed_kernel<PREC, true>) ----
  int launch_embed() {
    if (p.fused_first || c.E == 0 || p.steps < 1) return PEMP_OK;
    const pemp_mpn_desc& d = *c.desc;
    const pemp_mpn_weights& w = *c.w;
    const int64_t E = c.E;
    // (the label names the fall-backs apart: `wide` and `generic`, ForwardPlan)
    ProfScope prof(!p.emb_lds ? "edge_embed_wide" : p.emb_generic ? "edge_embed_generic" : "edge_embed", st);
    if (p.emb_lds) {
      // (over the edge passes' CUs: the embedding leaves the reserved CUs free too, edge_cus)
      const int grid = (int)std::min<int64_t>((int64_t)edge_cus(E) * EMB_PER_CU,
                                              (E + 16 * EMB_WAVES - 1) / (16 * EMB_WAVES));
      const size_t lds = (size_t)(p.comp ? embed_comp_floats(p.emb_lo) : embed_image_floats(p.emb_lo)) * sizeof(float);
      // the caller's prebuilt LDS image (pemp_mpn_edge_image appends it to the edge-pass image), else staged here
      const float* emb_img = w.edge_img ? w.edge_img + embed_image_offset(d, w) : nullptr;
      // (fp32 embeds only as <0, 0>, and only f16x3 has the composed form <2, 2>)
      with_prec(p.emb_prec, [&](auto P) {
        constexpr int PREC = decltype(P)::value;
        auto launch = [&](auto FX) {
          hipLaunchKernelGGL((edge_embed_kernel<PREC, decltype(FX)::value>), dim3(grid), dim3(64 * EMB_WAVES), lds, st,
                             w.edge_emb, p.emb_lo, w.emb_bf, c.edge_attr, d.edge_attr_dim, ws.s_orig, E, w.q0_w, w.q0_b,
                             w.e1_w, w.e1_bf, ws.EA, ws.Q0, ne, emb_img, w.emb_comp_bf, w.emb_comp_b);
        };
        if constexpr (PREC == PEMP_PREC_F16X3)
          if (p.comp) return launch(std::integral_constant<int, 2>{});
        if constexpr (PREC != PEMP_PREC_FP32)
          if (p.fixed) return launch(std::integral_constant<int, 1>{});
        launch(std::integral_constant<int, 0>{});
      });
    } else {
      hipLaunchKernelGGL(edge_embed_wide_kernel, dim3((unsigned)((E + 63) / 64)), dim3(256), 0, st, w.edge_emb,
                         c.edge_attr, d.edge_attr_dim, ws.s_orig, E, w.q0_w, w.q0_b, w.e1_w, ws.EA, ws.Q0,
                         d.precision == PEMP_PREC_F16X3 ? dom<2>() : 1.0f);
    }
    PEMP_LAUNCH_CHECK();
    return PEMP_OK;
  }

  // node_rows_kernel's arguments: x by `mode`, heads into slot (and slot + 1 when dup) when slot >= 0
  NodeRowsArgs rows_args(int mode, int slot, bool dup) const {
    const pemp_mpn_weights& w = *c.w;
    const int64_t N = c.N;
    const int J = p.J;
    NodeRowsArgs na{};
    na.mode = mode;
    if (mode == ROWS_EMBED) { na.x_in = c.x; na.in_ld = c.desc->node_in_dim; }
    na.agg = ws.agg; na.seg = ws.seg; na.T = p.T; na.upd_b = w.upd_b; na.N = N; na.X = ws.X;
    na.node_head = w.node_head; na.class_head = w.class_head; na.J = J;
    na.ne = ne;
    if (slot >= 0 && p.fused_heads && ne) {   // capacity mode: bases, the kernel places rows slot (+ 1) of its N
      na.node_out = c.node_logits;
      na.class_out = c.class_logits;
      na.slot = slot;
      na.dup = dup ? 1 : 0;
    } else if (slot >= 0 && p.fused_heads) {
      na.node_out = c.node_logits + (int64_t)slot * N;
      na.class_out = c.class_logits + (int64_t)slot * N * J;
      na.node_out2 = dup ? na.node_out + N : nullptr;
      na.class_out2 = dup ? na.class_out + N * J : nullptr;
    }
    na.emb = w.node_emb;
    na.img = node_img;
    na.head_off = p.fused_embed ? mlp_lds_floats(w.node_emb) : 0;
    na.head_floats = mlp_lds_floats(w.node_head) + mlp_lds_floats(w.class_head);
    na.emb_whole = mode == ROWS_EMBED && node_emb_whole(w.node_emb);
    return na;
  }

  NodeTableArgs table_args() const {
    return NodeTableArgs{ws.X, c.N, c.w->pre_w, c.w->pre_b, c.w->pre_bf, p.NO, p.table_groups, ws.NT, ne};
  }

  // The paired prelude (ForwardPlan::paired), two launches on the launch stream, each holding the blocks of two
  // independent kernels: A = the closed-form order beside the node embedding, B = the wave ranges and segment
  // positions beside the first node table. Each role reads only what earlier launches wrote.
  int launch_paired() {
    const PreludeGrids& g = p.grids;
    const FullyPrepArgs fa = fully_args();
    const NodeRowsArgs na = rows_args(ROWS_EMBED, -1, false);
    hipLaunchKernelGGL(prelude_a_kernel, dim3((unsigned)(g.a_split + g.rows_blocks)), dim3(256),
                       prelude_a_lds_bytes(na), st, fa, na, g.a_split, g.a_gx);
    PEMP_LAUNCH_CHECK();
    const EdgeRangesArgs ra = ranges_args();
    const NodeTableArgs ta = table_args();
    with_prec(p.table_prec, [&](auto P) {
      hipLaunchKernelGGL(prelude_b_kernel<decltype(P)::value>, dim3((unsigned)(g.b_split + g.table_blocks)), dim3(256),
                         0, st, ra, ta, g.b_split);
    });
    PEMP_LAUNCH_CHECK();
    return PEMP_OK;
  }

  // x for the next stage (mode) + heads when slot >= 0, then the node table when `table`
  int node_step(int mode, bool table, int slot, bool dup) {
    const pemp_mpn_weights& w = *c.w;
    const int64_t N = c.N;
    const int T = p.T, J = p.J;
    // middle steps of the attention model (update block in the edge pass, no heads): the node update runs inside the
    // node-table launch (node_table_kernel<PREC, 1, true>) instead of a launch of its own
    if (mode == ROWS_SUM && table && slot < 0 && p.sum_in_table) {
      NodeTableArgs ta{ws.X, N, w.pre_w, w.pre_b, w.pre_bf, p.NO, p.table_groups, ws.NT, ne, ws.agg, ws.seg, T,
                       w.upd_b};
      ProfScope prof("node_update_table", st);
      with_prec(p.table_prec, [&](auto P) {
        hipLaunchKernelGGL((node_table_kernel<decltype(P)::value, 1, true>), dim3(p.table_grid1), dim3(256), 0, st, ta);
      });
      PEMP_LAUNCH_CHECK();
      return PEMP_OK;
    }
    if (mode == NODE_UPDATE_MLP && w.upd_mlp.n_layers > 0) {   // hierarchical update MLP (dense-folded)
      NodeMlpArgs ma{ws.agg, ws.seg, T, N, w.upd_mlp, nmlp_max_out(w.upd_mlp), ws.X, ne};
      ProfScope prof("node_update", st);
      hipLaunchKernelGGL(node_mlp_kernel, dim3(p.node_grid), dim3(256), nmlp_lds_bytes(T, w.upd_mlp), st, ma);
      PEMP_LAUNCH_CHECK();
      mode = ROWS_NONE;
    } else if (mode == NODE_UPDATE_MLP) {                      // update MLP on non-linear aggregates
      NodeUpdateArgs ua{ws.agg, ws.seg, T, N, w.upd_w, w.upd_b, ws.X, ne};
      ProfScope prof("node_update", st);
      hipLaunchKernelGGL(node_update_kernel, dim3(p.node_grid, 4), dim3(64 * UPD_WAVES), 0, st, ua);
      PEMP_LAUNCH_CHECK();
      mode = ROWS_NONE;
    }
    const NodeRowsArgs na = rows_args(mode, slot, dup);
    if (na.mode != ROWS_NONE || na.node_out) {
      ProfScope prof(mode == ROWS_EMBED ? "node_embed" : "node_update", st);
      hipLaunchKernelGGL(node_rows_kernel, dim3(p.node_grid), dim3(256), node_rows_lds_bytes(na), st, na);
      PEMP_LAUNCH_CHECK();
    }
    if (slot >= 0 && !p.fused_heads) {
      for (int k = 0; k < (dup ? 2 : 1); ++k) {
        int r2;
        if ((r2 = rows_mlp("heads", w.node_head, ws.X + 64, 128, N, c.node_logits + (int64_t)(slot + k) * N, 1, nullptr,
                           0, st)))
          return r2;
        if ((r2 = rows_mlp("heads", w.class_head, ws.X + 64, 128, N, c.class_logits + (int64_t)(slot + k) * N * J, J,
                           nullptr, 0, st)))
          return r2;
      }
    }
    if (table) {
      const NodeTableArgs ta = table_args();
      ProfScope prof("node_table", st);
      with_prec(p.table_prec, [&](auto P) {
        hipLaunchKernelGGL(node_table_kernel<decltype(P)::value>, dim3(p.table_grid), dim3(256), 0, st, ta);
      });
      PEMP_LAUNCH_CHECK();
      return launch_ept();
    }
    return PEMP_OK;
  }

  // EDGE_MLP per_type: columns 0..127 of the table, the per-type node terms (zero rows in pre_w)
  int launch_ept() {
    if (!p.ept) return PEMP_OK;
    const pemp_mpn_weights& w = *c.w;
    NodeEptArgs xa{ws.X, c.node_types, p.tstride, p.T, c.N, w.ept_l1_w, w.ept_l1_b, w.ept_l2_w, w.ept_l2_b,
                   w.ept_o1_w, w.ept_o2_w, ws.NT, p.NO,
                   c.desc->precision == PEMP_PREC_F16X3 ? dom<2>() : 1.0f, ne};
    hipLaunchKernelGGL(node_ept_kernel, dim3(p.node_grid), dim3(256), 0, st, xa);
    PEMP_LAUNCH_CHECK();
    return PEMP_OK;
  }

  // the edge pass of iteration `it`: reads r_cur / NT / Q0, writes r_next / agg / (recorded) the edge logits
  int edge_pass(int it) {
    const pemp_mpn_desc& d = *c.desc;
    const bool record = recorded(it), is_last = last(it);
    EdgeStepArgs ea{};
    ea.N = c.N; ea.E = c.E; ea.T = p.T; ea.t_nt_ld = p.NO;
    const bool pub = record && p.pub_head;         // the published head's weights ride in the LDS image
    // (12-wave table: recorded middle passes with the published head; every other pass runs 16 waves)
    ea.ranges = ws.ranges + (pub && !is_last ? (int64_t)p.edge_grid * EDGE_WAVES : 0);
    ea.s_src = ws.s_src; ea.s_dst = ws.s_dst; ea.s_orig = ws.s_orig;
    const int stage = (is_last ? STAGE_LAST : STAGE_MID) | (p.ept ? STAGE_EPT : 0);
    ea.NT = ws.NT; ea.Q0 = ws.Q0; ea.r_cur = r_cur; ea.r_next = r_next;
    ea.img = eimg; ea.img_stride = img_stride(p.upd_fused, p.pub_head);
    ea.agg = ws.agg; ea.head = c.w->edge_head;
    ea.edge_logits = record ? (ne ? c.edge_logits : c.edge_logits + (int64_t)rec * c.E) : nullptr;
    ea.ne = ne;
    ea.rec = rec;
    ea.write_next = !is_last;
    if (it == 0 && p.fused_first) {   // embedding + pass 0 in one launch (it reads the first node table)
      ea.ea = c.edge_attr; ea.A = d.edge_attr_dim;
      ea.emb_img = c.w->edge_img + embed_image_offset(d, *c.w);
      ProfScope prof("edge_first", st);
      launch_edge_first(ea, it, p.edge_grid, st);
      PEMP_LAUNCH_CHECK();
      return PEMP_OK;
    }
    const char* label = !record ? "edge_step" : pub ? "edge_step_head" : "edge_step_head_generic";
    ProfScope prof(label, st);
    // a pass is idempotent (reads r_cur / NT / Q0, rewrites r_next / agg / logits), so the profiler
    // may repeat it between one event pair ("edge_step@R")
    for (int rep = prof_repeat(label); rep > 0; --rep) {
      switch (d.aggr) {
        case PEMP_AGGR_ATTN: launch_edge_step<PEMP_AGGR_ATTN>(ea, it, record, pub, p.edge_grid, d.precision, p.upd_fused, stage, st); break;
        case PEMP_AGGR_SUM: launch_edge_step<PEMP_AGGR_SUM>(ea, it, record, pub, p.edge_grid, d.precision, p.upd_fused, stage, st); break;
        case PEMP_AGGR_MEAN: launch_edge_step<PEMP_AGGR_MEAN>(ea, it, record, pub, p.edge_grid, d.precision, p.upd_fused, stage, st); break;
        default: launch_edge_step<PEMP_AGGR_MAX>(ea, it, record, pub, p.edge_grid, d.precision, false, stage, st); break;
      }
      PEMP_LAUNCH_CHECK();
    }
    return PEMP_OK;
  }

  // The prelude. The edge prelude (order, wave ranges, edge embedding) needs nothing the node embedding and the first
  // node table produce (their 16-row grids leave most CUs idle). In the paired form (ForwardPlan::paired,
  // launch_paired) the two chains share two launches. The separate form is the same kernels in launches of their
  // own, one after the other. Everything is on the launch stream: a side stream for the node chain cost a 7 us fork
  // and a 13 us join wait in front of the first pass.
  int prelude() {
    int rc;
    if (p.paired) {   // (T = 1 model steps and the other shapes without a fused first pass: the embedding follows B)
      if (!(rc = launch_paired()) && !(rc = launch_ept())) rc = launch_embed();
      return rc;
    }
    // node embedding + node table of the first iteration (or, without iterations, the heads on the embedding);
    // embedding widths > 128 would not fit the node step's LDS rows: separate launch
    rc = p.fused_embed ? PEMP_OK
                       : rows_mlp("node_embed", c.w->node_emb, c.x, c.desc->node_in_dim, c.N, ws.X, 128, ws.X + 64, 128, st);
    if (!rc) rc = node_step(p.fused_embed ? ROWS_EMBED : ROWS_NONE, p.steps > 0, p.steps > 0 ? -1 : 0, false);
    if (!rc && !(rc = launch_order()) && !(rc = launch_ranges())) rc = launch_embed();
    return rc;
  }

  int run() {
    int rc;
    if ((rc = launch_setup()) || (rc = prelude())) return rc;
    for (int it = 0; it < p.steps; ++it) {
      if (c.E > 0 && (rc = edge_pass(it))) return rc;
      // node update + next node table; heads when recorded (the last iteration's heads also fill
      // the post-loop slot: NODE_STEPS = 0 leaves x unchanged, NodeClassificationMPNSimple.py:93-94)
      if ((rc = node_step(p.node_mode, !last(it), recorded(it) ? rec : -1, last(it)))) return rc;
      if (recorded(it)) ++rec;
      std::swap(r_cur, r_next);
    }
    return PEMP_OK;
  }
};

// One inference forward: every C entry point below fills a ForwardCall and ends here.
static int mpn_forward(const ForwardCall& c) {
  if (const int rc = check_forward_args(c)) return rc;
  if (c.N == 0) return PEMP_OK;   // (with or without edges: nothing is launched or written)
  const ForwardPlan p = plan_forward(c);
  return Forward(c, p).run();
}

extern "C" int pemp_mpn_forward(const pemp_mpn_desc* desc, const pemp_mpn_weights* w, const float* x,
                                const float* edge_attr, const int64_t* edge_index, const int64_t* node_types,
                                int64_t N, int64_t E, float* edge_logits, float* node_logits, float* class_logits,
                                void* workspace, size_t workspace_bytes, void* stream) {
  ForwardCall c{};
  c.desc = desc; c.w = w; c.x = x; c.edge_attr = edge_attr; c.edge_index = edge_index; c.node_types = node_types;
  c.N = N; c.E = E; c.edge_logits = edge_logits; c.node_logits = node_logits; c.class_logits = class_logits;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  return mpn_forward(c);
}

extern "C" int pemp_mpn_forward_fully(const pemp_mpn_desc* desc, const pemp_mpn_weights* w, const float* x,
                                      const float* edge_attr, const int64_t* edge_index, const int64_t* node_types,
                                      int64_t N, int64_t E, const int64_t* node_off, const int64_t* node_off_host,
                                      int B, float* edge_logits, float* node_logits, float* class_logits,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  PEMP_CHECK_ARG(node_off && node_off_host && B >= 1 && B <= FULLY_MAXB, "pemp_mpn_forward_fully: bad node offsets");
  PEMP_CHECK_ARG(node_off_host[0] == 0 && node_off_host[B] == N, "pemp_mpn_forward_fully: offsets do not sum to N");
  int64_t e_full = 0, nmax = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t n = node_off_host[b + 1] - node_off_host[b];
    PEMP_CHECK_ARG(n >= 0, "pemp_mpn_forward_fully: decreasing offsets");
    e_full += n * (n > 0 ? n - 1 : 0);
    nmax = std::max(nmax, n);
  }
  PEMP_CHECK_ARG(e_full == E, "pemp_mpn_forward_fully: E=%lld is not the fully graph's %lld", (long long)E,
                 (long long)e_full);
  ForwardCall c{};
  c.desc = desc; c.w = w; c.x = x; c.edge_attr = edge_attr; c.edge_index = edge_index; c.node_types = node_types;
  c.N = N; c.E = E; c.edge_logits = edge_logits; c.node_logits = node_logits; c.class_logits = class_logits;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  if (nmax <= FULLY_MAXN) {   // closed-form lists live in LDS: larger images take the sorting prepare
    c.order.kind = EdgeOrder::FULLY; c.order.node_off = node_off; c.order.B = B; c.order.nmax = (int)nmax;
  }
  return mpn_forward(c);
}

// ---- HIP graphs of the capacity-mode forward ------------------------------------------------------------------
// A capacity-mode forward's launches depend only on its arguments (pointers, capacities, descriptor, weight set),
// never on the batch's counts, so the whole sequence (~13 launches, all on one stream) is
// captured into a HIP graph the second time the same arguments come (the first time they launch directly: one-off
// argument sets never pay a capture) and replayed with one launch from then on -- a serving loop whose allocator
// hands back the same buffers every step. Keyed by the bytes of every argument; a small LRU.
// Opt-in (PEMP_GRAPHS=1; PEMP_NO_GRAPHS wins): on this image a replay costs the host more than the direct launches
// (58-72 vs 44 us per call at c2, where the host bounds the batch-1 step) and gave the GPU nothing measurable at c2,
// c3 or c3knn10 (tools/experiments/round5/gg.sh, ii.sh). The library profiler (per-kernel
// events) runs the launches directly.
struct CapGraph {
  std::string key;
  hipGraphExec_t exec = nullptr;
  uint64_t used = 0;
};

static bool graphs_off() {
  static const bool v = [] {
    const char* on = getenv("PEMP_GRAPHS");
    return getenv("PEMP_NO_GRAPHS") != nullptr || !(on && atoi(on) != 0);
  }();
  return v;
}

// The null (legacy) stream cannot be captured: a caller on it gets its graphs captured on and replayed from a
// private stream of the device, joined to the null stream by events around each replay. Every use of that stream
// (capture, first launch, replays) holds its mutex: a replay queued on it while another thread captures would
// invalidate the capture.
struct GraphStream {
  hipStream_t s = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  std::mutex mu;
};

static GraphStream* graph_stream(int dev) {
  static std::mutex mu;
  static std::map<int, GraphStream*> table;
  std::lock_guard<std::mutex> lk(mu);
  auto it = table.find(dev);
  if (it != table.end()) return it->second;
  GraphStream* g = new GraphStream();
  if (hipStreamCreateWithFlags(&g->s, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&g->fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&g->join, hipEventDisableTiming) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;   // (leaked once; graphs are then not used on the null stream)
  }
  table[dev] = g;
  return g;
}

// Graph statistics for the tests (pemp_mpn_graph_stats): captures made, replays launched, captures refused.
static std::atomic<uint64_t> g_graph_captures{0}, g_graph_replays{0}, g_graph_refused{0};

extern "C" size_t pemp_abi_struct_size(int which) {
  switch (which) {
    case 0: return sizeof(pemp_mpn_weights);
    case 1: return sizeof(pemp_mpn_desc);
    case 2: return sizeof(pemp_mlp);
    case 3: return sizeof(pemp_proj_maps);
    case 4: return sizeof(pemp_step_plan);
    case 5: return sizeof(pemp_loss_rec);
    case 6: return sizeof(pemp_kp_loss_rec);
    default: return 0;
  }
}

extern "C" int pemp_edge_cus_policy(int num_cus_, int64_t E, int reserve_request) {
  PEMP_CHECK_ARG(num_cus_ >= 1 && E >= 0, "pemp_edge_cus_policy: bad args");
  if (reserve_request < 0) {
    const char* e = getenv("PEMP_RESERVE_CUS");
    reserve_request = e ? atoi(e) : RESERVE_CUS_DEFAULT;
  }
  return edge_cus_policy(num_cus_, E, reserve_request);
}

extern "C" int pemp_mpn_graph_stats(uint64_t* out3) {
  PEMP_CHECK_ARG(out3, "pemp_mpn_graph_stats: null output");
  out3[0] = g_graph_captures.load();
  out3[1] = g_graph_replays.load();
  out3[2] = g_graph_refused.load();
  return PEMP_OK;
}

extern "C" int pemp_mpn_forward_fully_cap(const pemp_mpn_desc* desc, const pemp_mpn_weights* w, const float* x,
                                          const float* edge_attr, const int64_t* node_types, int64_t n_cap,
                                          int64_t e_cap, const int32_t* n_det, int det_cap, const int64_t* node_off,
                                          int B, float* edge_logits, float* node_logits, float* class_logits,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  PEMP_CHECK_ARG(desc && w && n_det && node_off && B >= 1 && B <= FULLY_MAXB, "pemp_mpn_forward_fully_cap: bad args");
  PEMP_CHECK_ARG(n_cap >= 1 && e_cap >= 0 && det_cap >= 1, "pemp_mpn_forward_fully_cap: bad capacities");
  if (det_cap > FULLY_MAXN || !node_heads_fused(*w) || !node_embed_fused(*w) || !mlp_ok(w->edge_emb, 64, 64)) {
    set_error("pemp_mpn_forward_fully_cap: this model / capacity takes the exact forward");
    return PEMP_ERR_UNSUPPORTED;
  }
  // the forward's own launches on stream `s`: N and E are the capacities, the closed-form order takes det_cap as
  // the bound of an image's nodes
  auto direct = [&](void* s) {
    ForwardCall c{};
    c.desc = desc; c.w = w; c.x = x; c.edge_attr = edge_attr; c.node_types = node_types;
    c.N = n_cap; c.E = e_cap; c.edge_logits = edge_logits; c.node_logits = node_logits; c.class_logits = class_logits;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = s;
    c.order.kind = EdgeOrder::FULLY; c.order.node_off = node_off; c.order.B = B; c.order.nmax = det_cap;
    c.cap.ne = node_off + B + 1;
    return mpn_forward(c);
  };
  // PEMP_DEBUG_SYNC synchronises the device after every launch, which a capturing stream does not allow
  if (graphs_off() || prof_active() || debug_sync()) return direct(stream);
  int dev = 0;
  PEMP_HIP(hipGetDevice(&dev));
  std::string key;
  auto put = [&key](const void* p, size_t n) { key.append(static_cast<const char*>(p), n); };
  const void* ptrs[] = {x, edge_attr, node_types, n_det, node_off, edge_logits, node_logits, class_logits, workspace,
                        stream};
  const int64_t nums[] = {n_cap, e_cap, det_cap, B, (int64_t)workspace_bytes, dev};
  put(desc, sizeof(*desc));
  put(w, sizeof(*w));
  put(ptrs, sizeof(ptrs));
  put(nums, sizeof(nums));
  static std::mutex mu;
  static std::vector<CapGraph> cache;
  static std::vector<std::string> seen;   // argument sets launched directly once (most recent last)
  static uint64_t tick = 0;
  const hipStream_t ust = as_stream(stream);
  GraphStream* gs = ust ? nullptr : graph_stream(dev);
  if (!ust && !gs) return direct(stream);
  // a null-stream caller holds the private stream for the whole call (replay, or capture + first launch)
  std::unique_lock<std::mutex> gs_lock;
  if (gs) gs_lock = std::unique_lock<std::mutex>(gs->mu);
  const hipStream_t st = ust ? ust : gs->s;   // capture / replay stream
  auto launch = [&](hipGraphExec_t exec) -> int {
    if (gs) {                                 // null-stream caller: fork to the private stream and back
      PEMP_HIP(hipEventRecord(gs->fork, ust));
      PEMP_HIP(hipStreamWaitEvent(gs->s, gs->fork, 0));
    }
    PEMP_HIP(hipGraphLaunch(exec, st));
    if (gs) {
      PEMP_HIP(hipEventRecord(gs->join, gs->s));
      PEMP_HIP(hipStreamWaitEvent(ust, gs->join, 0));
    }
    g_graph_replays.fetch_add(1);
    return PEMP_OK;
  };
  {
    std::unique_lock<std::mutex> lk(mu);
    for (auto& e : cache)
      if (e.key == key) {
        e.used = ++tick;
        return launch(e.exec);
      }
    auto it = std::find(seen.begin(), seen.end(), key);
    const bool second_sight = it != seen.end();
    if (second_sight) {
      seen.erase(it);                       // captured below
    } else {                                // first sight: direct launches
      if (seen.size() >= 32) seen.erase(seen.begin());
      seen.push_back(key);
      lk.unlock();
      return direct(stream);
    }
  }
  // capture (thread-local mode: other threads' launches on other streams are unaffected)
  if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    g_graph_refused.fetch_add(1);
    return direct(stream);
  }
  const int rc = direct(st);
  hipGraph_t graph = nullptr;
  const hipError_t ec = hipStreamEndCapture(st, &graph);
  if (rc != PEMP_OK || ec != hipSuccess || !graph) {
    // a launch refused while capturing, or the capture itself invalidated: nothing was queued, so the forward
    // runs directly on the caller's stream (an argument error repeats there and is returned from there)
    if (graph) (void)hipGraphDestroy(graph);
    (void)hipGetLastError();
    g_graph_refused.fetch_add(1);
    return direct(stream);
  }
  hipGraphExec_t exec = nullptr;
  const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (ei != hipSuccess || !exec) {
    (void)hipGetLastError();
    g_graph_refused.fetch_add(1);
    return direct(stream);
  }
  g_graph_captures.fetch_add(1);
  const int rl = launch(exec);
  if (rl != PEMP_OK) {
    (void)hipGraphExecDestroy(exec);
    return rl;
  }
  std::lock_guard<std::mutex> lk(mu);
  constexpr size_t CAP_GRAPHS = 16;
  if (cache.size() >= CAP_GRAPHS) {
    auto lru = std::min_element(cache.begin(), cache.end(),
                                [](const CapGraph& a, const CapGraph& b) { return a.used < b.used; });
    (void)hipDeviceSynchronize();           // (rare: a replay of the evicted graph may still be in flight)
    (void)hipGraphExecDestroy(lru->exec);
    cache.erase(lru);
  }
  cache.push_back(CapGraph{key, exec, ++tick});
  return PEMP_OK;
}

extern "C" int pemp_mpn_forward_sym(const pemp_mpn_desc* desc, const pemp_mpn_weights* w, const float* x,
                                    const float* edge_attr, const int64_t* edge_index, const int64_t* node_types,
                                    int64_t N, int64_t E, float* edge_logits, float* node_logits, float* class_logits,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  ForwardCall c{};
  c.desc = desc; c.w = w; c.x = x; c.edge_attr = edge_attr; c.edge_index = edge_index; c.node_types = node_types;
  c.N = N; c.E = E; c.edge_logits = edge_logits; c.node_logits = node_logits; c.class_logits = class_logits;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  // the packed row entries hold a node id in SYM_TBITS bits: larger graphs take the sorting prepare
  if (N < (1ll << SYM_TBITS)) c.order.kind = EdgeOrder::SYM;
  return mpn_forward(c);
}

extern "C" int pemp_mpn_forward_knn(const pemp_mpn_desc* desc, const pemp_mpn_weights* w, const float* x,
                                    const float* edge_attr, const int64_t* edge_index, const int64_t* node_types,
                                    int64_t N, int64_t E, const void* knn_rows, const int32_t* knn_rowstart,
                                    const int64_t* node_off, const int64_t* node_off_host, const int64_t* ecount, int B,
                                    float* edge_logits, float* node_logits, float* class_logits, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  PEMP_CHECK_ARG(B >= 1 && B <= KP_MAXB && node_off_host && node_off && ecount && (E == 0 || (knn_rows && knn_rowstart)),
                 "pemp_mpn_forward_knn: bad rows / offsets (B=%d, at most %d images)", B, KP_MAXB);
  PEMP_CHECK_ARG(N <= KP_MAXN && node_off_host[0] == 0 && node_off_host[B] == N,
                 "pemp_mpn_forward_knn: N=%lld must equal node_off_host[B] and be <= %d", (long long)N, KP_MAXN);
  for (int b = 0; b < B; ++b)
    PEMP_CHECK_ARG(node_off_host[b + 1] >= node_off_host[b] && node_off_host[b + 1] - node_off_host[b] <= 64 * KP_W,
                   "pemp_mpn_forward_knn: image %d holds more than %d nodes", b, 64 * KP_W);
  KnnPrepArgs ka{};
  ka.R = static_cast<const unsigned long long*>(knn_rows);
  ka.rowstart = knn_rowstart; ka.node_off = node_off; ka.ecount = ecount; ka.B = B;
  const char* cap = getenv("PEMP_KNN_LIST_CAP");
  ka.list_cap = cap ? std::max(0, std::min(KP_LIST, atoi(cap))) : KP_LIST;
  ForwardCall c{};
  c.desc = desc; c.w = w; c.x = x; c.edge_attr = edge_attr; c.edge_index = edge_index; c.node_types = node_types;
  c.N = N; c.E = E; c.edge_logits = edge_logits; c.node_logits = node_logits; c.class_logits = class_logits;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  c.order.kind = EdgeOrder::KNN; c.order.knn = &ka;
  return mpn_forward(c);
}

extern "C" int pemp_mpn_prepare(const pemp_mpn_desc* desc, const int64_t* edge_index, const int64_t* node_types,
                                int64_t N, int64_t E, void* workspace, size_t workspace_bytes, void* stream) {
  PEMP_CHECK_ARG(desc && desc->num_types >= 1 && desc->num_types <= MAXT, "pemp_mpn_prepare: bad desc");
  PEMP_CHECK_ARG(N >= 0 && E >= 0 && N < (1ll << 30) && E < (1ll << 31) - 64 && (int64_t)desc->num_types * N < (1ll << 30),
                 "pemp_mpn_prepare: N=%lld E=%lld out of range", (long long)N, (long long)E);
  PEMP_CHECK_ARG(E == 0 || (edge_index && node_types), "pemp_mpn_prepare: null edge tensors");
  size_t need = 0;
  mpn_carve(nullptr, desc->num_types, N, E, &need);
  if (workspace_bytes < need) {
    set_error("pemp_mpn_prepare: workspace %zu < %zu bytes", workspace_bytes, need);
    return PEMP_ERR_WORKSPACE;
  }
  if (N == 0) return PEMP_OK;
  return launch_prepare(desc, edge_index, node_types, N, E, mpn_carve(workspace, desc->num_types, N, E, nullptr),
                        as_stream(stream));
}

extern "C" int pemp_mpn_order_layout(const pemp_mpn_desc* desc, int64_t N, int64_t E, size_t* offs) {
  PEMP_CHECK_ARG(desc && offs && desc->num_types >= 1 && desc->num_types <= MAXT, "pemp_mpn_order_layout: bad desc");
  PEMP_CHECK_ARG(N >= 0 && E >= 0, "pemp_mpn_order_layout: N=%lld E=%lld out of range", (long long)N, (long long)E);
  mpn_carve(nullptr, desc->num_types, N, E, nullptr, offs);
  return PEMP_OK;
}

extern "C" size_t pemp_mpn_fused_first_lds_bytes(void) { return edge_first_lds_bytes(); }

extern "C" int pemp_mpn_prelude_grids(int64_t N, int64_t E, int B, int T, int nmax, int edge_grid, int cus,
                                      int32_t* out8) {
  PEMP_CHECK_ARG(out8 && N >= 0 && E >= 0 && B >= 0 && B <= FULLY_MAXB && T >= 1 && T <= MAXT && nmax >= 0 &&
                     nmax <= FULLY_MAXN && edge_grid >= 1 && cus >= 1,
                 "pemp_mpn_prelude_grids: bad args");
  const PreludeGrids g = prelude_grids(N, E, B, T, nmax, edge_grid, cus);
  static_assert(sizeof(PreludeGrids) == 8 * sizeof(int32_t), "eight ints");
  memcpy(out8, &g, sizeof(g));
  return PEMP_OK;
}

extern "C" size_t pemp_mpn_edge_image_floats(const pemp_mpn_desc* desc, const pemp_mpn_weights* w) {
  if (!desc || !w || desc->num_types < 1 || desc->num_types > MAXT) return 0;
  if (!mlp_ok(w->edge_emb, 64, 64)) return edge_image_base_floats(*desc, *w);
  return embed_image_offset(*desc, *w) + embed_image_floats(embed_layout(w->edge_emb, embed_prec(*desc, *w)));
}

extern "C" int pemp_mpn_edge_image(const pemp_mpn_desc* desc, const pemp_mpn_weights* w, float* image, size_t floats,
                                   void* stream) {
  PEMP_CHECK_ARG(desc && w && image, "pemp_mpn_edge_image: null pointer");
  PEMP_CHECK_ARG(desc->num_types >= 1 && desc->num_types <= MAXT, "pemp_mpn_edge_image: bad num_types");
  PEMP_CHECK_ARG(desc->precision == PEMP_PREC_FP32 || (w->e1_bf && w->e2_bf && w->msg_bf),
                 "pemp_mpn_edge_image: split precisions need the *_bf packs");
  PEMP_CHECK_ARG(w->e1_w && w->e2_w && w->e2_b && w->msg_w, "pemp_mpn_edge_image: null layer weights");
  PEMP_CHECK_ARG(desc->aggr != PEMP_AGGR_ATTN || w->attn_w, "pemp_mpn_edge_image: attention needs attn_w");
  const size_t need = pemp_mpn_edge_image_floats(desc, w);
  PEMP_CHECK_ARG(floats >= need, "pemp_mpn_edge_image: image needs %zu floats", need);
  EdgeImgArgs ia = edge_image_args(*desc, *w, edge_upd_fused(*desc, *w), edge_pub_head(*desc, *w), image);
  hipLaunchKernelGGL(edge_image_kernel, dim3(16, (unsigned)desc->num_types), dim3(256), 0, as_stream(stream), ia);
  PEMP_LAUNCH_CHECK();
  if (mlp_ok(w->edge_emb, 64, 64)) {   // the edge embedding's LDS image, after the passes' (edge_embed_kernel)
    const int prec = embed_prec(*desc, *w);
    const EmbedLayout lo = embed_layout(w->edge_emb, prec);
    float* eimg = image + embed_image_offset(*desc, *w);
    const bool fixed = embed_fixed_shape(lo);
    const bool comp = embed_composed(lo, prec, *w);
    // (five instantiations: the fixed-shape form exists for the split precisions only)
    with_prec(prec, [&](auto P) {
      constexpr int PREC = decltype(P)::value;
      auto launch = [&](auto FX) {
        hipLaunchKernelGGL((embed_image_kernel<PREC, decltype(FX)::value>), dim3(16), dim3(256), 0, as_stream(stream),
                           w->edge_emb, lo, w->emb_bf, w->q0_w, w->q0_b, w->e1_w, w->e1_bf,
                           comp ? w->emb_comp_bf : nullptr, comp ? w->emb_comp_b : nullptr, eimg);
      };
      if constexpr (PREC != PEMP_PREC_FP32)
        if (fixed) return launch(std::true_type{});
      launch(std::false_type{});
    });
    PEMP_LAUNCH_CHECK();
  }
  return PEMP_OK;
}

extern "C" size_t pemp_mpn_node_image_floats(const pemp_mpn_weights* w) {
  if (!w) return 0;
  return node_image_extent(*w);
}

extern "C" int pemp_mpn_node_image(const pemp_mpn_weights* w, float* image, size_t floats, void* stream) {
  PEMP_CHECK_ARG(w && image, "pemp_mpn_node_image: null pointer");
  const StagePlan plan = node_image_plan(*w);
  PEMP_CHECK_ARG(floats >= node_image_extent(*w), "pemp_mpn_node_image: image needs %zu floats",
                 node_image_extent(*w));
  if (plan.total == 0) return PEMP_OK;
  hipLaunchKernelGGL(stage_image_kernel, dim3((unsigned)std::min(64, (plan.total + 255) / 256)), dim3(256), 0,
                     as_stream(stream), plan, image);
  PEMP_LAUNCH_CHECK();
  return PEMP_OK;
}

extern "C" int pemp_mpn_status(const pemp_mpn_desc* desc, int64_t N, int64_t E, const void* workspace,
                               void* stream) {
  PEMP_CHECK_ARG(desc && workspace, "pemp_mpn_status: null args");
  const MpnWs ws = mpn_carve(const_cast<void*>(workspace), desc->num_types, N, E, nullptr);
  int err = 0;
  PEMP_HIP(hipMemcpyAsync(&err, ws.err, sizeof(int), hipMemcpyDeviceToHost, as_stream(stream)));
  PEMP_HIP(hipStreamSynchronize(as_stream(stream)));
  if (err & 1) { set_error("edge_index has entries outside [0, N)"); return PEMP_ERR_INVALID_ARG; }
  if (err & 2) { set_error("node_types has entries outside [0, num_types)"); return PEMP_ERR_INVALID_ARG; }
  if (err & 12) {
    set_error("edge_index is not a symmetric edge list sorted by (src, dst) (pemp_mpn_forward_sym%s)",
              (err & 4) ? ": order" : ": symmetry");
    return PEMP_ERR_INVALID_ARG;
  }
  return PEMP_OK;
}
