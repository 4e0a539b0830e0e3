// The pieces the one-workgroup-per-graph, weights-in-registers kernels share (explain.hip: one frozen model, masks, backward;
// ensemble.hip: many frozen models, forward only; shapley.hip: one frozen model, a permutation walk of masked forwards): the
// tile geometry, the shape limits, the sorted packed row list, the masked row sum and the lane-per-column f32 GEMM off an LDS
// tile.  Everything is inlined into the callers; the build's edge pass stays in each kernel
// (graph_csr.h explains why).
#pragma once
#include "common.h"
#include "graph_csr.h"

namespace {

constexpr int XW = 8;                  // waves per workgroup
constexpr int XT = XW * 64;            // threads
constexpr int X_MAX_NODES = 224;
constexpr int X_MAX_EDGES = 1024;
constexpr int XD = 64;                 // embedding_dim
constexpr int XS = XD + 4;             // tile row stride in floats (rows 16-byte aligned, four rows of a wave on different banks)
constexpr int X_EPT = X_MAX_EDGES / XT;
constexpr int X_HEAD = 256;            // floats of the readout's activation / gradient vectors (128 + 64 + 32 + 16 + 8 used)
constexpr int X_RPL = (X_MAX_NODES + 63) / 64;

struct XGraph { int ebase, ne; };   // what EdgeRegs::load reads of a graph

// (a select chain, not an index: a dynamically indexed kernel-argument array would be copied to scratch)
__device__ __forceinline__ const float* x_pick(const float* const (&p)[4], int i) {
  return i == 0 ? p[0] : i == 1 ? p[1] : i == 2 ? p[2] : p[3];
}

// entries [kb, ke) of a packed list in ascending order (neighbour id, then edge position)
__device__ __forceinline__ void x_sort_row(unsigned* ent, int kb, int ke) {
  const int len = ke - kb;
  if (len > 1 && len <= 4) {
    const Sorted4 o = sort4(ent[kb], ent[kb + 1], len > 2 ? ent[kb + 2] : 0xffffffffu, len > 3 ? ent[kb + 3] : 0xffffffffu);
    ent[kb] = o.a0;
    ent[kb + 1] = o.a1;
    if (len > 2) ent[kb + 2] = o.a2;
    if (len > 3) ent[kb + 3] = o.a3;
  } else if (len > 4) {
    for (int a = kb + 1; a < ke; ++a) {
      const unsigned key = ent[a];
      int b = a - 1;
      while (b >= kb && ent[b] > key) { ent[b + 1] = ent[b]; --b; }
      ent[b + 1] = key;
    }
  }
}

// w = row `lane` of a [64][K] weight matrix, zero beyond K (K uniform): ONE uniform base + a 32-bit byte offset per element
// (the scalar-base form of global_load; a 64-bit address per element, vector or scalar, is 128 registers), unconditional
// loads on a clamped flat index
__device__ __forceinline__ void x_weight_row(float (&w)[XD], const char* Wb, int lane, int K) {
  const unsigned row0 = (unsigned)(lane * K), last = (unsigned)(XD * K - 1);
#pragma unroll
  for (int k = 0; k < XD; ++k) {
    const float v = *reinterpret_cast<const float*>(Wb + 4u * min(row0 + (unsigned)k, last));
    w[k] = k < K ? v : 0.f;
    if ((k & 15) == 15) __builtin_amdgcn_sched_barrier(0);
  }
}

// res(r, lane) = sum_k in[r][k] w[k] for the rows r < n of an LDS tile: a wave takes one row at a time; four partial sums
// (k = 0, 1, 2, 3 mod 4, each ascending) combined as (p0 + p1) + (p2 + p3): the same order for every row.  (Four rows at a time
// kept every row's tile reads live at once -- 192 registers beside the 64 of w -- and spilled.)
template <class Store>
__device__ __forceinline__ void x_gemm(const float* in, const float (&w)[XD], int n, int wave, Store store) {
#pragma nounroll
  for (int r = wave; r < n; r += XW) {
    const float* row = in + r * XS;
    float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
#pragma unroll
    for (int k4 = 0; k4 < XD / 4; ++k4) {
      const float4 a = *reinterpret_cast<const float4*>(row + 4 * k4);
      p0 = fmaf(a.x, w[4 * k4], p0);
      p1 = fmaf(a.y, w[4 * k4 + 1], p1);
      p2 = fmaf(a.z, w[4 * k4 + 2], p2);
      p3 = fmaf(a.w, w[4 * k4 + 3], p3);
    }
    store(r, (p0 + p1) + (p2 + p3));
  }
}

// acc = self * t[row] + sum_{k in [kb, ke)} mval[e_k] dinv[c_k] t[c_k]  for this lane's four columns
__device__ __forceinline__ float4 x_row_sum(const float* t, const unsigned* ent, const float* mval, const float* dinv,
                                            int row, int kb, int ke, int c4, float self) {
  const float4 s = *reinterpret_cast<const float4*>(t + row * XS + 4 * c4);
  float4 acc = make_float4(self * s.x, self * s.y, self * s.z, self * s.w);
  for (int k = kb; k < ke; ++k) {
    const unsigned en = ent[k];
    const int c = (int)(en >> 16);
    const float coef = mval[en & 0xffffu] * dinv[c];
    const float4 v = *reinterpret_cast<const float4*>(t + c * XS + 4 * c4);
    acc.x = fmaf(coef, v.x, acc.x);
    acc.y = fmaf(coef, v.y, acc.y);
    acc.z = fmaf(coef, v.z, acc.z);
    acc.w = fmaf(coef, v.w, acc.w);
  }
  return acc;
}

// the model / graph shapes these kernels take (hcg_explain's HCG_ERR_UNSUPPORTED)
inline int x_shapes_ok(const hcg_explain_args* p) {
  return p->D == XD && p->F >= 1 && p->F <= XD && p->C >= 1 && p->C <= 8 && p->n_conv >= 1 && p->n_conv <= HCG_EXPLAIN_MAX_CONVS &&
         p->R >= 1 && p->R <= HCG_HEAD_MAX_LAYERS && p->max_nodes >= 0 && p->max_nodes <= X_MAX_NODES && p->max_edges >= 0 &&
         p->max_edges <= X_MAX_EDGES && p->N >= 0 && p->E >= 0 && p->B >= 0 && p->N < (1ll << 31) / XD && p->E < (1ll << 31);
}

}  // namespace
