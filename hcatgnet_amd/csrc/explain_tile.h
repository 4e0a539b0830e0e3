// What the one-workgroup-per-graph, weights-in-registers kernels of a FROZEN model share (explain.hip: one model, masks,
// backward; ensemble.hip: many models, forward only; shapley.hip: one model, a permutation walk of masked forwards): the tile
// geometry and shape limits, the launch arguments all three take (XCommon) with their one host validation and marshalling,
// and the forward itself -- refusal prologue, edge pass, by-destination row list, lane-per-column f32 GEMM off an LDS tile,
// masked aggregation, [max, mean] pooling, readout.  Each kernel keeps its LDS carve, its barriers' neighbours (what it
// zeroes, stages or stores between the pieces) and whatever only it does.  Everything is inlined into the callers, and only
// these three kernels call it: the edge pass of the mid / wave / tall families stays in those files (graph_csr.h explains why).
// Every piece here left VGPRs, scratch and occupancy of the three kernels what they were with the code written out per kernel.
// shapley.hip keeps its own readout loop (layer 0 off registers): through x_readout with a hook for that layer k_shapley_walk
// took 166 VGPRs instead of 165, whichever way the hook was passed.
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

// the launch arguments every kernel of the family takes: the first member of its argument block (device pointers by value)
struct XCommon {
  const float* x;
  const int64_t* ei;
  const int32_t* graph_ptr;
  const int32_t* edge_ptr;
  const float* cW[HCG_EXPLAIN_MAX_CONVS];
  const float* cb[HCG_EXPLAIN_MAX_CONVS];
  const float* hW[HCG_HEAD_MAX_LAYERS];
  const float* hb[HCG_HEAD_MAX_LAYERS];
  int32_t* status;
  long long E;                          // edges the edge loads may index (>= 1)
  int F, C, n_conv, R, npad, emax, max_nodes, max_edges;
  float slope;
};

// The entry word of a row list and the coefficient it stands for.  XPlain: the neighbour's id, coefficient dinv[c].
// XMasked: (id << 16) | local edge, coefficient mval[edge] dinv[c].
struct XPlain {
  static __device__ __forceinline__ unsigned entry(int c, unsigned) { return (unsigned)c; }
  static __device__ __forceinline__ int col(unsigned en) { return (int)en; }
  __device__ __forceinline__ float coef(unsigned, float dc) const { return dc; }
};
struct XMasked {
  const float* mval;
  static __device__ __forceinline__ unsigned entry(int c, unsigned e) { return ((unsigned)c << 16) | e; }
  static __device__ __forceinline__ int col(unsigned en) { return (int)(en >> 16); }
  __device__ __forceinline__ float coef(unsigned en, float dc) const { return mval[en & 0xffffu] * dc; }
};

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

// acc = self * t[row] + sum_{k in [kb, ke)} coef_k t[c_k]  for this lane's four columns, k ascending
template <class Ent>
__device__ __forceinline__ float4 x_row_sum(const float* t, const unsigned* ent, Ent fmt, const float* dinv, int row, int kb,
                                            int ke, int c4, float self) {
  const float4 s = *reinterpret_cast<const float4*>(t + row * XS + 4 * c4);
  float4 acc = make_float4(self * s.x, self * s.y, self * s.z, self * s.w);
  for (int k = kb; k < ke; ++k) {
    const unsigned en = ent[k];
    const int c = Ent::col(en);
    const float coef = fmt.coef(en, dinv[c]);
    const float4 v = *reinterpret_cast<const float4*>(t + c * XS + 4 * c4);
    acc.x = fmaf(coef, v.x, acc.x);
    acc.y = fmaf(coef, v.y, acc.y);
    acc.z = fmaf(coef, v.z, acc.z);
    acc.w = fmaf(coef, v.w, acc.w);
  }
  return acc;
}

// ---- the graph: refusal, edge pass, row lists ---------------------------------------------------------------------------
struct XSpan { int nbase, ebase, n_raw, ne_raw, n, ne; };   // graph g's node / edge range: as the metadata has it, and as taken

// true: the graph is refused (HCG_STATUS_SHAPE_LIMIT, reported) -- the caller zeroes its outputs and returns
__device__ __forceinline__ bool x_refused(XSpan& s, const XCommon& c, int g, int tid) {
  s.nbase = __builtin_amdgcn_readfirstlane(c.graph_ptr[g]);
  s.ebase = __builtin_amdgcn_readfirstlane(c.edge_ptr[g]);
  s.n_raw = c.graph_ptr[g + 1] - s.nbase;
  s.ne_raw = c.edge_ptr[g + 1] - s.ebase;
  s.n = s.n_raw;
  s.ne = s.ne_raw;
  graph_refuse(s.n, s.ne, c.max_nodes, c.max_edges, tid, c.status);
  return s.n != s.n_raw || s.ne != s.ne_raw;
}

// thread tid's edges tid + j XT: local ids, and whether the edge gets an entry
struct XEdges { int es[X_EPT], ed[X_EPT]; bool live[X_EPT]; };

__device__ __forceinline__ void x_edge_pass(XEdges& q, const EdgeRegs<X_EPT, XT>& er, const XSpan& g, int tid, int32_t* status) {
#pragma unroll
  for (int j = 0; j < X_EPT; ++j) {
    const int e = tid + j * XT;
    const long long s = er.s[j] - g.nbase, d = er.d[j] - g.nbase;
    const bool in = e < g.ne;
    const bool ok = s >= 0 && s < g.n && d >= 0 && d < g.n;
    if (in && !ok) atomicOr(status, HCG_STATUS_EDGE_UNGROUPED);        // (such edges are ignored)
    q.es[j] = (int)s;
    q.ed[j] = (int)d;
    q.live[j] = in && ok && s != d;                                    // an explicit (i, i) edge is the unit self loop
  }
}

struct XRows { unsigned* ent; int* rowptr; int* cnt; };   // [emax], [npad + 4], [npad] (zeroed by the caller; the fill cursor)

// The by-destination list `bd` (and, TWO, the by-source list `bs` in the same barrier intervals) of the live edges, rows
// sorted by the entry word, and dinv from the in-degree.  Opens with a barrier (the zeroed counters); the caller places the
// barrier between the sort and the first reader.
template <class Ent, bool TWO>
__device__ __forceinline__ void x_build_rows(const XEdges& q, XRows bd, XRows bs, float* dinv, int n, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < X_EPT; ++j)
    if (q.live[j]) {
      atomicAdd(&bd.cnt[q.ed[j]], 1);
      if (TWO) atomicAdd(&bs.cnt[q.es[j]], 1);
    }
  __syncthreads();
  if (wave == 0) csr_scan_rows<X_RPL>(bd.cnt, bd.rowptr, n, lane);
  else if (TWO && wave == 1) csr_scan_rows<X_RPL>(bs.cnt, bs.rowptr, n, lane);
  for (int i = tid; i < n; i += XT) dinv[i] = gcn_dinv(bd.cnt[i]);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < X_EPT; ++j)
    if (q.live[j]) {
      const unsigned e = (unsigned)(tid + j * XT);
      const int pd = bd.rowptr[q.ed[j]] + atomicSub(&bd.cnt[q.ed[j]], 1) - 1;
      bd.ent[pd] = Ent::entry(q.es[j], e);
      if (TWO) {
        const int ps = bs.rowptr[q.es[j]] + atomicSub(&bs.cnt[q.es[j]], 1) - 1;
        bs.ent[ps] = Ent::entry(q.ed[j], e);
      }
    }
  __syncthreads();
  if (tid < n) x_sort_row(bd.ent, bd.rowptr[tid], bd.rowptr[tid + 1]);
  else if (TWO && tid >= XT / 2 && tid - XT / 2 < n) x_sort_row(bs.ent, bs.rowptr[tid - XT / 2], bs.rowptr[tid - XT / 2 + 1]);
}

// ---- the forward's pieces behind the GEMM -------------------------------------------------------------------------------
// dst = leaky(dinv_i (dinv_i src_i + sum_k coef_k src_c) + b) for the rows < n: 16 lanes x float4 per row, 32 rows per pass;
// extra(row, c4, y) sees every float4 stored
template <class Ent, class Extra>
__device__ __forceinline__ void x_conv_out(const float* src, float* dst, const unsigned* ent, const int* rowptr, Ent fmt,
                                           const float* dinv, const float* bias, int n, int tid, float slope, Extra extra) {
  const int arow = tid >> 4, c4 = tid & 15;
  float bb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) bb[j] = bias[4 * c4 + j];
  for (int row = arow; row < n; row += XT / 16) {
    const float di = dinv[row];
    const float4 s = x_row_sum(src, ent, fmt, dinv, row, rowptr[row], rowptr[row + 1], c4, di);
    float4 y = make_float4(fmaf(di, s.x, bb[0]), fmaf(di, s.y, bb[1]), fmaf(di, s.z, bb[2]), fmaf(di, s.w, bb[3]));
    y = make_float4(hcg_leaky(y.x, slope), hcg_leaky(y.y, slope), hcg_leaky(y.z, slope), hcg_leaky(y.w, slope));
    *reinterpret_cast<float4*>(dst + row * XS + 4 * c4) = y;
    extra(row, c4, y);
  }
}

// hv[0 .. 128) = [max, mean] over the rows < n of t0 (zeros for n = 0); red: [XW][128] partials.  Ends behind a barrier.
__device__ __forceinline__ void x_pool(const float* t0, float* red, float* hv, int n, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  {
    float mx = -INFINITY, sm = 0.f;
    for (int r = wave; r < n; r += XW) {
      const float v = t0[r * XS + lane];
      mx = fmaxf(mx, v);
      sm += v;
    }
    red[wave * 128 + lane] = mx;
    red[wave * 128 + 64 + lane] = sm;
  }
  __syncthreads();
  if (tid < 64) {
    float mx = red[tid], sm = red[64 + tid];
#pragma unroll
    for (int w = 1; w < XW; ++w) {
      mx = fmaxf(mx, red[w * 128 + tid]);
      sm += red[w * 128 + 64 + tid];
    }
    hv[tid] = n > 0 ? mx : 0.f;
    hv[64 + tid] = n > 0 ? sm / (float)n : 0.f;
  }
  __syncthreads();
}

// The readout of model m of stacked weights ([M][out_i][in_i] / [M][out_i]; one model: m = 0) on hv[0 .. 128), 8 lanes per
// output: hv = emb | v1 | v2 | ... | out.  -> the position of the output row in hv; ends behind a barrier.
__device__ __forceinline__ int x_readout(float* hv, const XCommon& c, int m, int tid) {
  const int o = tid >> 3, sub = tid & 7;
  int off = 0;
  for (int i = 0; i < c.R; ++i) {
    const int in_i = (2 * XD) >> i, out_i = i == c.R - 1 ? c.C : in_i / 2;
    const size_t wskip = (size_t)m * out_i * in_i, bskip = (size_t)m * out_i;
    float p = 0.f;
    if (o < out_i) {
      const float* W = x_pick(c.hW, i) + wskip + (size_t)o * in_i;
      for (int k = sub; k < in_i; k += 8) p = fmaf(W[k], hv[off + k], p);
    }
    p += __shfl_xor(p, 1, 8);
    p += __shfl_xor(p, 2, 8);
    p += __shfl_xor(p, 4, 8);
    if (o < out_i && sub == 0) {
      const float y = p + x_pick(c.hb, i)[bskip + o];
      hv[off + in_i + o] = i == c.R - 1 ? y : hcg_leaky(y, c.slope);
    }
    off += in_i;
    __syncthreads();
  }
  return off;
}

// ---- host ---------------------------------------------------------------------------------------------------------------
// the model / graph shapes these kernels take (hcg_explain's HCG_ERR_UNSUPPORTED)
inline int x_shapes_ok(const hcg_explain_args* p) {
  return p->D == XD && p->F >= 1 && p->F <= XD && p->C >= 1 && p->C <= 8 && p->n_conv >= 1 && p->n_conv <= HCG_EXPLAIN_MAX_CONVS &&
         p->R >= 1 && p->R <= HCG_HEAD_MAX_LAYERS && p->max_nodes >= 0 && p->max_nodes <= X_MAX_NODES && p->max_edges >= 0 &&
         p->max_edges <= X_MAX_EDGES && p->N >= 0 && p->E >= 0 && p->B >= 0 && p->N < (1ll << 31) / XD && p->E < (1ll << 31);
}


// the pointers every mode needs for a launch (the per-mode ones are checked in the mode's file; HCG_EXPLAIN_COALITIONS writes
// its table and no `out`)
inline bool x_common_ok(const hcg_explain_args* p, bool with_out = true) {
  if (!p->graph_ptr || !p->edge_ptr || (with_out && !p->out) || !p->status || (p->N > 0 && !p->x) || (p->E > 0 && !p->edge_index)) return false;
  for (int l = 0; l < p->n_conv; ++l)
    if (!p->conv_W[l] || !p->conv_b[l]) return false;
  for (int i = 0; i < p->R; ++i)
    if (!p->head_W[i] || !p->head_b[i]) return false;
  return true;
}

inline int x_round4(long long v, int least) {
  const long long r = (v + 3) / 4 * 4;
  return (int)(r > least ? r : least);
}

inline void x_fill_common(XCommon& c, const hcg_explain_args* p, int npad_min = 4) {
  c.x = p->x;
  c.ei = p->edge_index;
  c.E = p->E;
  if (p->E == 0) { c.ei = reinterpret_cast<const int64_t*>(p->graph_ptr); c.E = 1; }   // readable dummy; no graph has edges
  c.graph_ptr = p->graph_ptr;
  c.edge_ptr = p->edge_ptr;
  for (int l = 0; l < HCG_EXPLAIN_MAX_CONVS; ++l) { c.cW[l] = p->conv_W[l]; c.cb[l] = p->conv_b[l]; }
  for (int i = 0; i < HCG_HEAD_MAX_LAYERS; ++i) { c.hW[i] = p->head_W[i]; c.hb[i] = p->head_b[i]; }
  c.status = p->status;
  c.F = (int)p->F;
  c.C = (int)p->C;
  c.n_conv = p->n_conv;
  c.R = p->R;
  c.npad = x_round4(p->max_nodes, npad_min);
  c.emax = x_round4(p->max_edges, 4);
  c.max_nodes = (int)p->max_nodes;
  c.max_edges = (int)p->max_edges;
  c.slope = p->slope;
}

// dynamic LDS above 64 KB: allowed once per process and kernel (not per launch: it may be under capture)
template <auto K>
hipError_t x_allow_big_lds() {
  static hipError_t st = hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  return st;
}

template <auto K, class Args>
int x_launch(dim3 grid, unsigned lds, hipStream_t stream, const Args& a) {
  if (lds > 64 * 1024) {
    const hipError_t e = x_allow_big_lds<K>();
    if (e != hipSuccess) return hcg_hip_err(e);
  }
  hipLaunchKernelGGL(K, grid, dim3(XT), lds, stream, a);
  HCG_CHECK_LAUNCH();
  return HCG_OK;
}

}  // namespace
