// The edge update of the training-mode MPN as one fused fp32-MFMA operator with its own backward (mpn/train.py
// edge_update): mlp_edge(cat([x[dst], x[src], ef])) in the per-node-table form of the inference path,
//   h = relu(P[dst] + Q[src] + ef C^T),  e_new = relu(h W2^T + b2),
// with P = nf A^T + b1 and Q = nf B^T ([N, 64] tables the caller computes with torch; W1 = [A | B | C]).
//
// Forward: persistent 256-thread workgroups hold C and W2 in LDS (fp32) and walk tiles of 64 edges, one wave per
// 16 edges. The layout is the library's "edge on the lane" one (mpn.hip gemm_frag): lane (i = lane & 15,
// q = lane >> 4) holds features 16 b + 4 q + r of edge i, which is both the B operand and the C/D layout of
// v_mfma_f32_16x16x4_f32, so the two layers chain in registers. Four independent accumulators per wave.
//
// Backward: a workgroup owns one chunk of 256 edges at a time (four tiles). Per tile, phase A is the transposed
// chain in the same layout (g2 = g [e_new > 0], g1 = (g2 W2) [h > 0], g_ef = g1 C; W2^T and C^T in LDS); it leaves
// g1 in LDS. Phase B sums the weight gradients with the edges as the MFMA's K: wave w owns rows 16 w .. 16 w + 15 of
// dW2 = g2^T h, dC = g1^T ef and db2 = g2^T 1, so one accumulation chain runs over the chunk's 256 edges in edge
// order and no two waves add into one element. Each chunk stores one partial into the caller's workspace; a second
// kernel adds the partials in a fixed pairwise tree (32 leaves per pass, zero-padded). No atomics; the result
// depends on neither the grid nor the CU count.
#include <limits.h>

#include <algorithm>

#include "pemp_common.h"

namespace pemp {
namespace {

constexpr int kTile = 64;        // edges per tile (16 per wave)
constexpr int kChunk = 256;      // edges per weight-gradient partial: the longest fp32 chain over edges
constexpr int kLeaves = 32;      // partials added per tree pass
constexpr int kLdH = 64 + 4;     // LDS row stride of a [.][64] weight image (16 rows x float4 cover the banks once)
constexpr int kLdG = 64 + 16;    // LDS row stride of the g1 tile: phase B reads 4 rows x 16 floats, one bank each

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
// v where keep, else zeros: the loads below are unconditional from a clamped (always valid) row and masked after,
// so that a wave's loads issue back to back instead of one branch and one wait per load
__device__ __forceinline__ float4 keep4(bool keep, float4 v) {
  return make_float4(keep ? v.x : 0.f, keep ? v.y : 0.f, keep ? v.z : 0.f, keep ? v.w : 0.f);
}
// ReLU that keeps NaN, as torch.relu does (mpn.hip's integer-max form maps a NaN with the sign bit set to 0)
__device__ __forceinline__ float relu1(float x) { return x < 0.f ? 0.f : x; }

__host__ __device__ constexpr int part_floats(int WE) { return 64 * WE + 64 * 64 + 64; }   // [dC | dW2 | db2]

// acc[ob] += W[16 ob + i][.] . in  for OB output and KB input blocks of 16; W in LDS with row stride LD.
// The OB chains are independent; the k order of a chain is input block, then r, then q inside the MFMA.
template <int KB, int OB, int LD>
__device__ __forceinline__ void gemm_lds(const float* W, const float (&in)[KB][4], f32x4 (&acc)[OB]) {
  const int lane = __lane_id(), i = lane & 15, q = lane >> 4;
#pragma unroll
  for (int mb = 0; mb < KB; ++mb) {
    float4 w[OB];
#pragma unroll
    for (int ob = 0; ob < OB; ++ob) w[ob] = ld4(W + (16 * ob + i) * LD + 16 * mb + 4 * q);
#pragma unroll
    for (int ob = 0; ob < OB; ++ob) acc[ob] = mfma4(w[ob].x, in[mb][0], acc[ob]);
#pragma unroll
    for (int ob = 0; ob < OB; ++ob) acc[ob] = mfma4(w[ob].y, in[mb][1], acc[ob]);
#pragma unroll
    for (int ob = 0; ob < OB; ++ob) acc[ob] = mfma4(w[ob].z, in[mb][2], acc[ob]);
#pragma unroll
    for (int ob = 0; ob < OB; ++ob) acc[ob] = mfma4(w[ob].w, in[mb][3], acc[ob]);
  }
}

template <int WE>
__global__ __launch_bounds__(256, 2) void edge_mlp_fwd_kernel(int64_t N, int64_t E, const float* __restrict__ P,
                                                           const float* __restrict__ Q, const float* __restrict__ ef,
                                                           const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                           const float* __restrict__ C, const float* __restrict__ W2,
                                                           const float* __restrict__ b2, float* __restrict__ h,
                                                           float* __restrict__ e_new) {
  constexpr int LDC = WE + 4, KB = WE / 16;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* sC = lds;                  // [64][LDC]
  float* sW2 = lds + 64 * LDC;      // [64][kLdH]
  for (int t = threadIdx.x; t < 64 * WE / 4; t += 256) {
    const int row = t / (WE / 4), col = (t % (WE / 4)) * 4;
    st4(sC + row * LDC + col, ld4(C + row * WE + col));
  }
  for (int t = threadIdx.x; t < 64 * 64 / 4; t += 256) {
    const int row = t / 16, col = (t % 16) * 4;
    st4(sW2 + row * kLdH + col, ld4(W2 + row * 64 + col));
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
  float4 bias[4];
#pragma unroll
  for (int ob = 0; ob < 4; ++ob) bias[ob] = ld4(b2 + 16 * ob + 4 * q);
  const int64_t ntiles = (E + kTile - 1) / kTile;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    // the weight fragments are read from LDS per tile: hoisted out of the loop they take 190 registers (We = 128)
    // and the second workgroup per CU, which hides this tile's row loads, no longer fits
    asm volatile("" ::: "memory");
    const int64_t e = tile * kTile + wave * 16 + i;
    const bool valid = e < E;
    const size_t ec = valid ? (size_t)e : 0;       // (E > 0: row 0 exists)
    // node ids outside [0, N) are never followed: such an end reads row 0 (N > 0) and contributes zeros
    const uint32_t d = (uint32_t)dst[ec], s = (uint32_t)src[ec];
    const bool okd = valid && d < (uint64_t)N, oks = valid && s < (uint64_t)N;
    const size_t dc = okd ? d : 0, sc = oks ? s : 0;
    f32x4 acc[4];
#pragma unroll
    for (int ob = 0; ob < 4; ++ob) {
      const float4 p = keep4(okd, ld4(P + dc * 64 + 16 * ob + 4 * q));
      const float4 r = keep4(oks, ld4(Q + sc * 64 + 16 * ob + 4 * q));
      acc[ob][0] = p.x + r.x, acc[ob][1] = p.y + r.y, acc[ob][2] = p.z + r.z, acc[ob][3] = p.w + r.w;
    }
    float in[KB][4];
#pragma unroll
    for (int mb = 0; mb < KB; ++mb) {
      const float4 v = keep4(valid, ld4(ef + ec * WE + 16 * mb + 4 * q));
      in[mb][0] = v.x, in[mb][1] = v.y, in[mb][2] = v.z, in[mb][3] = v.w;
    }
    gemm_lds<KB, 4, LDC>(sC, in, acc);
    float hid[4][4];
    f32x4 out[4];
#pragma unroll
    for (int ob = 0; ob < 4; ++ob) {
#pragma unroll
      for (int r = 0; r < 4; ++r) hid[ob][r] = relu1(acc[ob][r]);
      if (valid) st4(h + (size_t)e * 64 + 16 * ob + 4 * q, make_float4(hid[ob][0], hid[ob][1], hid[ob][2], hid[ob][3]));
      out[ob][0] = bias[ob].x, out[ob][1] = bias[ob].y, out[ob][2] = bias[ob].z, out[ob][3] = bias[ob].w;
    }
    gemm_lds<4, 4, kLdH>(sW2, hid, out);
    if (valid) {
#pragma unroll
      for (int ob = 0; ob < 4; ++ob)
        st4(e_new + (size_t)e * 64 + 16 * ob + 4 * q,
            make_float4(relu1(out[ob][0]), relu1(out[ob][1]), relu1(out[ob][2]), relu1(out[ob][3])));
    }
  }
}

template <int WE>
__global__ __launch_bounds__(256, 2) void edge_mlp_bwd_kernel(int64_t E, const float* __restrict__ g,
                                                           const float* __restrict__ ef, const float* __restrict__ h,
                                                           const float* __restrict__ e_new, const float* __restrict__ C,
                                                           const float* __restrict__ W2, float* __restrict__ g1,
                                                           float* __restrict__ g_ef, float* __restrict__ part) {
  constexpr int CB = WE / 16, PART = part_floats(WE);
  // dynamic LDS above 64 KB per workgroup at We = 128 (72.7 KB): gfx950 has 160 KB per CU, and two workgroups fit
  static_assert(2 * ((WE + 64) * kLdH + 64 * kLdG) * sizeof(float) <= 160 * 1024, "two backward workgroups per CU");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* sCt = lds;                        // [WE][kLdH]: sCt[c][j] = C[j][c]
  float* sW2t = sCt + WE * kLdH;           // [64][kLdH]: sW2t[k][j] = W2[j][k]
  float* sG1 = sW2t + 64 * kLdH;           // [64][kLdG]: g1 of the tile's edges
  {  // every global read of the two images in flight at once, then the transposed LDS stores
    constexpr int NC = 64 * WE / 4 / 256, NW = 64 * 64 / 4 / 256;
    float4 vc[NC], vw[NW];
#pragma unroll
    for (int k = 0; k < NC; ++k) vc[k] = ld4(C + 4 * (threadIdx.x + 256 * k));
#pragma unroll
    for (int k = 0; k < NW; ++k) vw[k] = ld4(W2 + 4 * (threadIdx.x + 256 * k));
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const int t = 4 * (threadIdx.x + 256 * k), j = t / WE, c = t % WE;
      sCt[c * kLdH + j] = vc[k].x, sCt[(c + 1) * kLdH + j] = vc[k].y;
      sCt[(c + 2) * kLdH + j] = vc[k].z, sCt[(c + 3) * kLdH + j] = vc[k].w;
    }
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const int t = 4 * (threadIdx.x + 256 * k), j = t / 64, c = t % 64;
      sW2t[c * kLdH + j] = vw[k].x, sW2t[(c + 1) * kLdH + j] = vw[k].y;
      sW2t[(c + 2) * kLdH + j] = vw[k].z, sW2t[(c + 3) * kLdH + j] = vw[k].w;
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
  const int64_t nchunk = (E + kChunk - 1) / kChunk;
  for (int64_t chunk = blockIdx.x; chunk < nchunk; chunk += gridDim.x) {
    f32x4 aW[4], aC[CB], aB = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < 4; ++b) aW[b] = aB;
#pragma unroll
    for (int b = 0; b < CB; ++b) aC[b] = aB;
    for (int t = 0; t < kChunk / kTile; ++t) {
      const int64_t base = chunk * kChunk + t * kTile;
      if (base >= E) break;                                    // block-uniform
      {  // ---- phase A: this wave's 16 edges, edge on the lane
        const int64_t e = base + wave * 16 + i;
        const bool valid = e < E;
        const size_t ec = valid ? (size_t)e : 0;
        float g2[4][4];
        float4 hv[4], gv[4], ev[4];
#pragma unroll
        for (int ob = 0; ob < 4; ++ob) {
          gv[ob] = ld4(g + ec * 64 + 16 * ob + 4 * q);
          ev[ob] = ld4(e_new + ec * 64 + 16 * ob + 4 * q);
          hv[ob] = ld4(h + ec * 64 + 16 * ob + 4 * q);
        }
#pragma unroll
        for (int ob = 0; ob < 4; ++ob) {
          hv[ob] = keep4(valid, hv[ob]);
          g2[ob][0] = (valid && ev[ob].x > 0.f) ? gv[ob].x : 0.f, g2[ob][1] = (valid && ev[ob].y > 0.f) ? gv[ob].y : 0.f;
          g2[ob][2] = (valid && ev[ob].z > 0.f) ? gv[ob].z : 0.f, g2[ob][3] = (valid && ev[ob].w > 0.f) ? gv[ob].w : 0.f;
        }
        f32x4 tacc[4];
#pragma unroll
        for (int ob = 0; ob < 4; ++ob) tacc[ob] = f32x4{0.f, 0.f, 0.f, 0.f};
        gemm_lds<4, 4, kLdH>(sW2t, g2, tacc);
        float g1v[4][4];
#pragma unroll
        for (int ob = 0; ob < 4; ++ob) {
          g1v[ob][0] = hv[ob].x > 0.f ? tacc[ob][0] : 0.f, g1v[ob][1] = hv[ob].y > 0.f ? tacc[ob][1] : 0.f;
          g1v[ob][2] = hv[ob].z > 0.f ? tacc[ob][2] : 0.f, g1v[ob][3] = hv[ob].w > 0.f ? tacc[ob][3] : 0.f;
          const float4 v = make_float4(g1v[ob][0], g1v[ob][1], g1v[ob][2], g1v[ob][3]);
          st4(sG1 + (wave * 16 + i) * kLdG + 16 * ob + 4 * q, v);   // (zeros past E)
          if (valid) st4(g1 + (size_t)e * 64 + 16 * ob + 4 * q, v);
        }
        f32x4 gacc[CB];
#pragma unroll
        for (int ob = 0; ob < CB; ++ob) gacc[ob] = f32x4{0.f, 0.f, 0.f, 0.f};
        gemm_lds<4, CB, kLdH>(sCt, g1v, gacc);
        if (valid) {
#pragma unroll
          for (int ob = 0; ob < CB; ++ob)
            st4(g_ef + (size_t)e * WE + 16 * ob + 4 * q, make_float4(gacc[ob][0], gacc[ob][1], gacc[ob][2], gacc[ob][3]));
        }
      }
      __syncthreads();
      // ---- phase B: rows 16 wave .. + 15 of the weight gradients; four edges (k = q) per MFMA, in edge order.
      // Column i of tile b is column 4 i + b of its 64-column group: one float4 per lane and group, whole rows per
      // wave instruction. The operands of four steps are loaded at once, one batch ahead of the MFMAs.
      constexpr int SB = 4, NBATCH = kTile / 4 / SB;
      float pg[2][SB], pe[2][SB];
      float4 ph[2][SB], pf[2][SB][CB / 4];
      auto load_batch = [&](int buf, int bt) {
#pragma unroll
        for (int k = 0; k < SB; ++k) {
          const int64_t e = base + 4 * (SB * bt + k) + q;
          const size_t row = e < E ? (size_t)e : 0;
          pg[buf][k] = g[row * 64 + 16 * wave + i];
          pe[buf][k] = e_new[row * 64 + 16 * wave + i];
          ph[buf][k] = ld4(h + row * 64 + 4 * i);
#pragma unroll
          for (int c = 0; c < CB / 4; ++c) pf[buf][k][c] = ld4(ef + row * WE + 64 * c + 4 * i);
        }
      };
      load_batch(0, 0);
#pragma unroll
      for (int bt = 0; bt < NBATCH; ++bt) {
        if (bt + 1 < NBATCH) load_batch((bt + 1) & 1, bt + 1);
#pragma unroll
        for (int k = 0; k < SB; ++k) {
          const int s = SB * bt + k, buf = bt & 1;
          const bool valid = base + 4 * s + q < E;
          const float a2 = (valid && pe[buf][k] > 0.f) ? pg[buf][k] : 0.f;
          const float a1 = sG1[(4 * s + q) * kLdG + 16 * wave + i];
          const float4 hv = keep4(valid, ph[buf][k]);
          aW[0] = mfma4(a2, hv.x, aW[0]), aW[1] = mfma4(a2, hv.y, aW[1]);
          aW[2] = mfma4(a2, hv.z, aW[2]), aW[3] = mfma4(a2, hv.w, aW[3]);
          aB = mfma4(a2, 1.f, aB);
#pragma unroll
          for (int c = 0; c < CB / 4; ++c) {
            const float4 f4 = keep4(valid, pf[buf][k][c]);
            aC[4 * c + 0] = mfma4(a1, f4.x, aC[4 * c + 0]), aC[4 * c + 1] = mfma4(a1, f4.y, aC[4 * c + 1]);
            aC[4 * c + 2] = mfma4(a1, f4.z, aC[4 * c + 2]), aC[4 * c + 3] = mfma4(a1, f4.w, aC[4 * c + 3]);
          }
        }
      }
      __syncthreads();                                         // sG1 is rewritten by the next tile
    }
    // the chunk's partial: lane (i, q) register r of tile 4 c + b holds row 16 wave + 4 q + r, column 64 c + 4 i + b
    float* out = part + (size_t)chunk * PART;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = 16 * wave + 4 * q + r;
#pragma unroll
      for (int c = 0; c < CB / 4; ++c)
        st4(out + j * WE + 64 * c + 4 * i, make_float4(aC[4 * c][r], aC[4 * c + 1][r], aC[4 * c + 2][r], aC[4 * c + 3][r]));
      st4(out + 64 * WE + j * 64 + 4 * i, make_float4(aW[0][r], aW[1][r], aW[2][r], aW[3][r]));
      if (i == 0) out[64 * WE + 64 * 64 + j] = aB[r];
    }
  }
}

// out[grp] = the pairwise tree over in[32 grp .. 32 grp + 31] (zeros past n_in), element by element. The last pass
// (one group left) writes the three gradients instead.
__global__ __launch_bounds__(256) void edge_mlp_tree_kernel(const float* __restrict__ in, int64_t n_in, int len,
                                                            float* __restrict__ out, float* __restrict__ dC,
                                                            float* __restrict__ dW2, float* __restrict__ db2, int nC) {
  const int el = blockIdx.y * 256 + threadIdx.x;
  if (el >= len) return;
  const int64_t grp = blockIdx.x, c0 = grp * kLeaves;
  float v[kLeaves];
#pragma unroll
  for (int k = 0; k < kLeaves; ++k) {                          // (unconditional loads from a clamped partial, masked after)
    const float x = in[(size_t)(c0 + k < n_in ? c0 + k : n_in - 1) * len + el];
    v[k] = c0 + k < n_in ? x : 0.f;
  }
#pragma unroll
  for (int w = 1; w < kLeaves; w <<= 1)
#pragma unroll
    for (int k = 0; k < kLeaves; k += 2 * w) v[k] += v[k + w];
  if (out)
    out[(size_t)grp * len + el] = v[0];
  else if (el < nC)
    dC[el] = v[0];
  else if (el < nC + 64 * 64)
    dW2[el - nC] = v[0];
  else
    db2[el - nC - 64 * 64] = v[0];
}

int check_common(const char* fn, int64_t N, int64_t E, int We) {
  PEMP_CHECK_ARG(We == 64 || We == 128, "%s: We = %d (64 or 128)", fn, We);
  PEMP_CHECK_ARG(N >= 0 && E >= 0, "%s: negative size (N = %lld, E = %lld)", fn, (long long)N, (long long)E);
  PEMP_CHECK_ARG(E <= INT_MAX && N < INT_MAX, "%s: int32 indices (N = %lld, E = %lld)", fn, (long long)N, (long long)E);
  return PEMP_OK;
}

inline int64_t chunks_of(int64_t E) { return (E + kChunk - 1) / kChunk; }
inline int64_t groups_of(int64_t n) { return (n + kLeaves - 1) / kLeaves; }

}  // namespace
}  // namespace pemp

using namespace pemp;

extern "C" size_t pemp_edge_mlp_workspace_size(int64_t E, int We) {
  if (E <= 0 || (We != 64 && We != 128)) return 0;
  const int64_t n = chunks_of(E);
  return (size_t)(n + groups_of(n)) * part_floats(We) * sizeof(float);
}

extern "C" int pemp_edge_mlp_fwd(int64_t N, int64_t E, int We, const float* P, const float* Q, const float* ef,
                                 const int32_t* src32, const int32_t* dst32, const float* C, const float* W2,
                                 const float* b2, float* h, float* e_new, void* stream) {
  if (int rc = check_common("pemp_edge_mlp_fwd", N, E, We)) return rc;
  if (N == 0 || E == 0) return PEMP_OK;           // no edge: h / e_new have no row
  PEMP_CHECK_ARG(P && Q && ef && src32 && dst32, "pemp_edge_mlp_fwd: NULL P / Q / ef / src32 / dst32");
  PEMP_CHECK_ARG(C && W2 && b2, "pemp_edge_mlp_fwd: NULL C / W2 / b2");
  PEMP_CHECK_ARG(h && e_new, "pemp_edge_mlp_fwd: NULL h / e_new");
  hipStream_t st = as_stream(stream);
  ProfScope prof("edge_mlp_fwd", st);
  const int64_t ntiles = (E + kTile - 1) / kTile;
  const dim3 grid((unsigned)std::min<int64_t>(ntiles, 2 * (int64_t)num_cus())), block(256);
  const size_t lds = (size_t)(64 * (We + 4) + 64 * kLdH) * sizeof(float);
  if (We == 64)
    edge_mlp_fwd_kernel<64><<<grid, block, lds, st>>>(N, E, P, Q, ef, src32, dst32, C, W2, b2, h, e_new);
  else
    edge_mlp_fwd_kernel<128><<<grid, block, lds, st>>>(N, E, P, Q, ef, src32, dst32, C, W2, b2, h, e_new);
  PEMP_LAUNCH_CHECK();
  return PEMP_OK;
}

extern "C" int pemp_edge_mlp_bwd(int64_t N, int64_t E, int We, const float* g, const float* ef, const float* h,
                                 const float* e_new, const float* C, const float* W2, float* g1, float* g_ef, float* dC,
                                 float* dW2, float* db2, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_common("pemp_edge_mlp_bwd", N, E, We)) return rc;
  hipStream_t st = as_stream(stream);
  if (E == 0) {                                   // no edge: zero weight gradients (where given), no launch
    if (dC) PEMP_HIP(hipMemsetAsync(dC, 0, (size_t)64 * We * sizeof(float), st));
    if (dW2) PEMP_HIP(hipMemsetAsync(dW2, 0, (size_t)64 * 64 * sizeof(float), st));
    if (db2) PEMP_HIP(hipMemsetAsync(db2, 0, (size_t)64 * sizeof(float), st));
    return PEMP_OK;
  }
  PEMP_CHECK_ARG(g && ef && h && e_new && C && W2, "pemp_edge_mlp_bwd: NULL g / ef / h / e_new / C / W2");
  PEMP_CHECK_ARG(g1 && g_ef && dC && dW2 && db2, "pemp_edge_mlp_bwd: NULL g1 / g_ef / dC / dW2 / db2");
  const size_t need = pemp_edge_mlp_workspace_size(E, We);
  PEMP_CHECK_ARG(workspace && workspace_bytes >= need, "pemp_edge_mlp_bwd: workspace of %zu bytes, %zu needed",
                 workspace ? workspace_bytes : (size_t)0, need);
  PEMP_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "pemp_edge_mlp_bwd: workspace not 16-byte aligned");
  const int64_t nchunk = chunks_of(E);
  const int len = part_floats(We);
  float* bufA = static_cast<float*>(workspace);
  float* bufB = bufA + (size_t)nchunk * len;
  {
    ProfScope prof("edge_mlp_bwd", st);
    const dim3 grid((unsigned)std::min<int64_t>(nchunk, 2 * (int64_t)num_cus())), block(256);
    const size_t lds = (size_t)((We + 64) * kLdH + 64 * kLdG) * sizeof(float);
    if (We == 64)
      edge_mlp_bwd_kernel<64><<<grid, block, lds, st>>>(E, g, ef, h, e_new, C, W2, g1, g_ef, bufA);
    else
      edge_mlp_bwd_kernel<128><<<grid, block, lds, st>>>(E, g, ef, h, e_new, C, W2, g1, g_ef, bufA);
    PEMP_LAUNCH_CHECK();
  }
  ProfScope prof("edge_mlp_tree", st);
  const float* cur = bufA;
  float* other = bufB;
  for (int64_t n = nchunk;;) {
    const int64_t ng = groups_of(n);
    const bool last = ng == 1;
    const dim3 grid((unsigned)ng, (unsigned)((len + 255) / 256)), block(256);
    edge_mlp_tree_kernel<<<grid, block, 0, st>>>(cur, n, len, last ? nullptr : other, dC, dW2, db2, 64 * We);
    PEMP_LAUNCH_CHECK();
    if (last) break;
    float* written = other;
    other = const_cast<float*>(cur);
    cur = written;
    n = ng;
  }
  return PEMP_OK;
}
