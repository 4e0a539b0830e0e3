// Ensemble prediction (reference scripts_experiments/predict_test.py:19-103: the 90 models of the nested cross-validation
// predict the same unseen set): M frozen models of one architecture on ONE batch of graphs in ONE launch, forward only.
//
// The graphs are shared and only the weights differ, so the grid runs over (graph, group of models): one workgroup of 8 waves
// builds its graph once and then runs `models_per_group` models on it, one after the other.  Workgroups never depend on each
// other, nothing is reduced across them, no float atomics: every sum has one owner and a fixed order, so the result for
// (model, graph) is bitwise the same run to run, whatever M, the group size and the rest of the batch are.  Per workgroup:
//   build     once: gcn_norm on chip from the raw COO edges (rules: graph_csr.h) -- in-degree, dinv, the by-destination row
//             list sorted by neighbour id.  No mask, no by-source list, no workspace: there is no backward.
//   model m   x -> t0 (zero-padded to 64 columns);  per layer  H = A_prev W_m^T (t0 -> t1: explain_tile.h x_gemm, the lane's
//             weight row in 64 registers, taken from a copy of W_m staged in LDS with coalesced loads),  A = leaky(dinv_i (dinv_i H_i + sum_k dinv_c H_c) + b_m) (t1 -> t0);  [max, mean]
//             pooling -> emb[m, g, :] (max first);  readout of depth R -> out[m, g, :].
// LDS holds the two [npad][64 + 4] f32 tiles, the 16 KB staged weight matrix and ~9 KB of structure, sized at launch from the
// batch's largest graph: 147 KB at the 224 / 1024 limit, 123 KB at the reference's 184 / 390.  A third tile that kept x on chip
// does not fit beside them, and held at its own width it would still not fit at F = 64; the x tile is therefore re-read per
// model from global memory / L2 (n F floats, 18 KB at real sizes, against the n 64 64 FMAs of one layer): one code path for
// every shape.  Resource usage of the built kernel (tools/kres.py): 127 VGPRs, no AGPRs, no scratch, no spills -- registers
// allow 4 waves per SIMD; LDS decides: one workgroup (2 waves per SIMD) per CU at real sizes, two from 57-node batches down.
// Measured (profiles/ensemble_bench.json): 90 models on 52 real-size graphs 0.64 ms against 5.4 ms of the per-model loop; on
// 535 graphs 5.8 ms against 5.7 ms -- with the device full the per-model kernels are as fast.  Where this kernel's time
// goes (the FMAs of x_gemm, or its broadcast tile reads: 16 ds_read_b128 per row and wave, 8 waves on one LDS): not measured.
#include "common.h"
#include "graph_csr.h"
#include "explain_tile.h"

namespace {

struct EArgs {     // the kernel's argument block (device pointers by value)
  const float* x;
  const int64_t* ei;
  const int32_t* graph_ptr;
  const int32_t* edge_ptr;
  const float* cW[HCG_EXPLAIN_MAX_CONVS];   // [M][64][F or 64]
  const float* cb[HCG_EXPLAIN_MAX_CONVS];   // [M][64]
  const float* hW[HCG_HEAD_MAX_LAYERS];     // [M][out_i][in_i]
  const float* hb[HCG_HEAD_MAX_LAYERS];     // [M][out_i]
  float* out;                               // [M][B][C]
  float* emb;                               // [M][B][128] or null
  int32_t* status;
  long long E;
  int B, F, C, n_conv, R, npad, emax, max_nodes, max_edges, M, mpg;
  float slope;
};

constexpr int EWS = XD + 1;            // row stride of the staged weights: lane = row reads hit 64 different banks

struct ELds {
  float* t0;            // [npad][XS]
  float* t1;            // [npad][XS]
  float* ws;            // [64][EWS]  the current layer's weight matrix of the current model
  unsigned* ent;        // [emax]  by destination: the source's local id
  int* rowptr;          // [npad + 4]
  int* cnt;             // [npad]  in-degree, then the fill cursor
  float* dinv;          // [npad]
  float* red;           // [XW][128] pooling partials
  float* hv;            // [X_HEAD] readout activations: emb | v1 | v2 | ... | out
};

__host__ __device__ inline unsigned e_lds_bytes(int npad, int emax) {
  return 2u * npad * XS * 4 + XD * EWS * 4 + (unsigned)emax * 4 + (unsigned)(npad + 4) * 4 + 2u * npad * 4 + XW * 128 * 4 + X_HEAD * 4;
}

// (integer offsets, as mid.hip's carve: the arrays must stay LDS pointers for the compiler)
__device__ __forceinline__ ELds e_carve(char* base, int npad, int emax) {
  ELds L;
  unsigned off = 0;
  L.t0 = reinterpret_cast<float*>(base + off); off += (unsigned)npad * XS * 4;
  L.t1 = reinterpret_cast<float*>(base + off); off += (unsigned)npad * XS * 4;
  L.ws = reinterpret_cast<float*>(base + off); off += XD * EWS * 4;
  L.ent = reinterpret_cast<unsigned*>(base + off); off += (unsigned)emax * 4;
  L.rowptr = reinterpret_cast<int*>(base + off); off += (unsigned)(npad + 4) * 4;
  L.cnt = reinterpret_cast<int*>(base + off); off += (unsigned)npad * 4;
  L.dinv = reinterpret_cast<float*>(base + off); off += (unsigned)npad * 4;
  L.red = reinterpret_cast<float*>(base + off); off += XW * 128 * 4;
  L.hv = reinterpret_cast<float*>(base + off);
  return L;
}

// acc = self * t[row] + sum_{k in [kb, ke)} dinv[c_k] t[c_k]  for this lane's four columns, k ascending
__device__ __forceinline__ float4 e_row_sum(const float* t, const unsigned* ent, const float* dinv, int row, int kb, int ke,
                                            int c4, float self) {
  const float4 s = *reinterpret_cast<const float4*>(t + row * XS + 4 * c4);
  float4 acc = make_float4(self * s.x, self * s.y, self * s.z, self * s.w);
  for (int k = kb; k < ke; ++k) {
    const int c = (int)ent[k];
    const float coef = dinv[c];
    const float4 v = *reinterpret_cast<const float4*>(t + c * XS + 4 * c4);
    acc.x = fmaf(coef, v.x, acc.x);
    acc.y = fmaf(coef, v.y, acc.y);
    acc.z = fmaf(coef, v.z, acc.z);
    acc.w = fmaf(coef, v.w, acc.w);
  }
  return acc;
}

// W [64][K] (one model's layer, contiguous) -> ws[row][k]: consecutive threads read consecutive floats.  (Read straight into
// the lanes' registers as explain.hip does once per graph -- lane = row, stride K floats -- every load instruction touches 64
// cache lines; repeated per MODEL that cost a quarter of this kernel's time: 90 models on 52 real-size graphs 832 -> 626 us.)
__device__ __forceinline__ void e_stage_weights(float* ws, const float* W, int K, int tid) {
  for (int i = tid; i < XD * K; i += XT) {
    const int r = i / K;
    ws[r * EWS + (i - r * K)] = W[i];
  }
}

__global__ __launch_bounds__(XT) void k_ensemble_graphs(const EArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ELds L = e_carve(smem, a.npad, a.emax);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x;
  const int F = a.F, C = a.C, R = a.R, n_conv = a.n_conv, B = a.B;
  const float slope = a.slope;
  const int m_begin = (int)blockIdx.y * a.mpg;
  const int m_end = min(m_begin + a.mpg, a.M);

  const int nbase = __builtin_amdgcn_readfirstlane(a.graph_ptr[g]), ebase = __builtin_amdgcn_readfirstlane(a.edge_ptr[g]);
  const int n_raw = a.graph_ptr[g + 1] - nbase, ne_raw = a.edge_ptr[g + 1] - ebase;
  int n = n_raw, ne = ne_raw;
  graph_refuse(n, ne, a.max_nodes, a.max_edges, tid, a.status);
  if (n != n_raw || ne != ne_raw) {
    // refused (HCG_STATUS_SHAPE_LIMIT): the graph's outputs are zero for every model
    for (int m = m_begin; m < m_end; ++m) {
      const size_t mg = (size_t)m * B + g;
      for (int c = tid; c < C; c += XT) a.out[mg * C + c] = 0.f;
      if (a.emb)
        for (int c = tid; c < 2 * XD; c += XT) a.emb[mg * (2 * XD) + c] = 0.f;
    }
    return;
  }

  // ---------------------------------------------------------------------------------------------- build (once per workgroup)
  XGraph gi{ebase, ne};
  EdgeRegs<X_EPT, XT> er;
  er.load(gi, a.ei, a.E, tid);
  for (int i = tid; i < a.npad; i += XT) L.cnt[i] = 0;
  int es[X_EPT], ed[X_EPT];
  bool live[X_EPT];
#pragma unroll
  for (int j = 0; j < X_EPT; ++j) {
    const int e = tid + j * XT;
    const long long s = er.s[j] - nbase, d = er.d[j] - nbase;
    const bool in = e < ne;
    const bool ok = s >= 0 && s < n && d >= 0 && d < n;
    if (in && !ok) atomicOr(a.status, HCG_STATUS_EDGE_UNGROUPED);      // (such edges are ignored)
    es[j] = (int)s;
    ed[j] = (int)d;
    live[j] = in && ok && s != d;                                      // an explicit (i, i) edge is the unit self loop
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < X_EPT; ++j)
    if (live[j]) atomicAdd(&L.cnt[ed[j]], 1);
  __syncthreads();
  if (wave == 0) csr_scan_rows<X_RPL>(L.cnt, L.rowptr, n, lane);
  for (int i = tid; i < n; i += XT) L.dinv[i] = gcn_dinv(L.cnt[i]);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < X_EPT; ++j)
    if (live[j]) {
      const int pd = L.rowptr[ed[j]] + atomicSub(&L.cnt[ed[j]], 1) - 1;
      L.ent[pd] = (unsigned)es[j];
    }
  __syncthreads();
  if (tid < n) x_sort_row(L.ent, L.rowptr[tid], L.rowptr[tid + 1]);
  // (the first barrier of the model loop orders the sort before the first aggregation)

  const int arow = tid >> 4, c4 = tid & 15;               // aggregation: 16 lanes x float4 per row, 32 rows per pass

#pragma nounroll
  for (int m = m_begin; m < m_end; ++m) {
    const size_t mg = (size_t)m * B + g;
    // x, zero-padded to 64 columns (t0's last readers, the pooling of the model before, are behind the readout's barriers)
    for (int idx = tid; idx < n * XD; idx += XT) {
      const int r = idx >> 6, k = idx & 63;
      L.t0[r * XS + k] = k < F ? a.x[(size_t)(nbase + r) * F + k] : 0.f;
    }
    e_stage_weights(L.ws, a.cW[0] + (size_t)m * XD * F, F, tid);
    __syncthreads();

    // -------------------------------------------------------------------------------------------- conv stack
#pragma nounroll
    for (int l = 0; l < n_conv; ++l) {
      const int K = __builtin_amdgcn_readfirstlane(l == 0 ? F : XD);   // (uniform: keeps the weight addressing scalar)
      {
        float w[XD];           // the lane's weight row, zero beyond K
#pragma unroll
        for (int k = 0; k < XD; ++k) {
          const float v = L.ws[lane * EWS + k];
          w[k] = k < K ? v : 0.f;
        }
        x_gemm(L.t0, w, n, wave, [&](int r, float v) { L.t1[r * XS + lane] = v; });
      }
      __syncthreads();
      // (every wave has its rows of ws in registers: the next layer's matrix goes in beside the aggregation)
      if (l + 1 < n_conv) e_stage_weights(L.ws, x_pick(a.cW, l + 1) + (size_t)m * XD * XD, XD, tid);
      {
        const float* bm = x_pick(a.cb, l) + (size_t)m * XD;
        float bb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bb[j] = bm[4 * c4 + j];
        for (int row = arow; row < n; row += XT / 16) {
          const float di = L.dinv[row];
          const float4 s = e_row_sum(L.t1, L.ent, L.dinv, row, L.rowptr[row], L.rowptr[row + 1], c4, di);
          float4 y = make_float4(fmaf(di, s.x, bb[0]), fmaf(di, s.y, bb[1]), fmaf(di, s.z, bb[2]), fmaf(di, s.w, bb[3]));
          y = make_float4(hcg_leaky(y.x, slope), hcg_leaky(y.y, slope), hcg_leaky(y.z, slope), hcg_leaky(y.w, slope));
          *reinterpret_cast<float4*>(L.t0 + row * XS + 4 * c4) = y;
        }
      }
      __syncthreads();
    }

    // -------------------------------------------------------------------------------------------- pooling: t0 = A of the last layer
    {
      float mx = -INFINITY, sm = 0.f;
      for (int r = wave; r < n; r += XW) {
        const float v = L.t0[r * XS + lane];
        mx = fmaxf(mx, v);
        sm += v;
      }
      L.red[wave * 128 + lane] = mx;
      L.red[wave * 128 + 64 + lane] = sm;
    }
    __syncthreads();
    if (tid < 64) {
      float mx = L.red[tid], sm = L.red[64 + tid];
#pragma unroll
      for (int w = 1; w < XW; ++w) {
        mx = fmaxf(mx, L.red[w * 128 + tid]);
        sm += L.red[w * 128 + 64 + tid];
      }
      mx = n > 0 ? mx : 0.f;
      sm = n > 0 ? sm / (float)n : 0.f;
      L.hv[tid] = mx;
      L.hv[64 + tid] = sm;
      if (a.emb) {
        a.emb[mg * (2 * XD) + tid] = mx;
        a.emb[mg * (2 * XD) + 64 + tid] = sm;
      }
    }
    __syncthreads();

    // -------------------------------------------------------------------------------------------- readout (8 lanes per output)
    int off = 0;
    for (int i = 0; i < R; ++i) {
      const int in_i = (2 * XD) >> i, out_i = i == R - 1 ? C : in_i / 2;
      const size_t wskip = (size_t)m * out_i * in_i, bskip = (size_t)m * out_i;   // model m inside [M][out_i][in_i] / [M][out_i]
      const int o = tid >> 3, sub = tid & 7;
      float p = 0.f;
      if (o < out_i) {
        const float* W = x_pick(a.hW, i) + wskip + (size_t)o * in_i;
        for (int k = sub; k < in_i; k += 8) p = fmaf(W[k], L.hv[off + k], p);
      }
      p += __shfl_xor(p, 1, 8);
      p += __shfl_xor(p, 2, 8);
      p += __shfl_xor(p, 4, 8);
      if (o < out_i && sub == 0) {
        const float y = p + x_pick(a.hb, i)[bskip + o];
        L.hv[off + in_i + o] = i == R - 1 ? y : hcg_leaky(y, slope);
      }
      off += in_i;
      __syncthreads();
    }
    if (tid < C) a.out[mg * C + tid] = L.hv[off + tid];
    // (hv and red are next written behind the barriers of the next model's conv stack)
  }
}

hipError_t ensemble_allow_big_lds() {   // dynamic LDS above 64 KB: allowed once per process (not per launch: it may be under capture)
  static hipError_t st = hipFuncSetAttribute((const void*)k_ensemble_graphs, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  return st;
}

}  // namespace

// hcg_explain, mode HCG_EXPLAIN_ENSEMBLE (explain.hip dispatches here)
int hcg_ensemble_launch(hcg_explain_args* p, hipStream_t stream) {
  if (p->edge_mask || p->node_mask || p->target || p->dout) return HCG_ERR_INVALID_ARG;
  if (!x_shapes_ok(p) || p->n_models < 1 || p->models_per_group < 1 || p->models_per_group > p->n_models) return HCG_ERR_UNSUPPORTED;
  const long long groups = hcg_cdiv(p->n_models, p->models_per_group);
  if (groups > 65535 || (long long)p->n_models * (p->B > 0 ? p->B : 1) >= (1ll << 31) / (2 * XD)) return HCG_ERR_UNSUPPORTED;
  p->workspace_bytes_needed = 0;          // forward only: nothing is kept
  if (p->flags & HCG_EXPLAIN_QUERY) return HCG_OK;
  if (p->B == 0) return HCG_OK;
  if (!p->graph_ptr || !p->edge_ptr || !p->out || !p->status || (p->N > 0 && !p->x) || (p->E > 0 && !p->edge_index))
    return HCG_ERR_INVALID_ARG;
  for (int l = 0; l < p->n_conv; ++l)
    if (!p->conv_W[l] || !p->conv_b[l]) return HCG_ERR_INVALID_ARG;
  for (int i = 0; i < p->R; ++i)
    if (!p->head_W[i] || !p->head_b[i]) return HCG_ERR_INVALID_ARG;

  EArgs a;
  a.x = p->x;
  a.ei = p->edge_index;
  a.E = p->E;
  if (p->E == 0) { a.ei = reinterpret_cast<const int64_t*>(p->graph_ptr); a.E = 1; }   // readable dummy; no graph has edges
  a.graph_ptr = p->graph_ptr;
  a.edge_ptr = p->edge_ptr;
  for (int l = 0; l < HCG_EXPLAIN_MAX_CONVS; ++l) { a.cW[l] = p->conv_W[l]; a.cb[l] = p->conv_b[l]; }
  for (int i = 0; i < HCG_HEAD_MAX_LAYERS; ++i) { a.hW[i] = p->head_W[i]; a.hb[i] = p->head_b[i]; }
  a.out = p->out;
  a.emb = p->emb;
  a.status = p->status;
  a.B = (int)p->B;
  a.F = (int)p->F;
  a.C = (int)p->C;
  a.n_conv = p->n_conv;
  a.R = p->R;
  a.npad = (int)((p->max_nodes + 3) / 4 * 4 > 4 ? (p->max_nodes + 3) / 4 * 4 : 4);
  a.emax = (int)((p->max_edges + 3) / 4 * 4 > 4 ? (p->max_edges + 3) / 4 * 4 : 4);
  a.max_nodes = (int)p->max_nodes;
  a.max_edges = (int)p->max_edges;
  a.M = p->n_models;
  a.mpg = p->models_per_group;
  a.slope = p->slope;
  const unsigned lds = e_lds_bytes(a.npad, a.emax);
  if (lds > 64 * 1024) {
    const hipError_t e = ensemble_allow_big_lds();
    if (e != hipSuccess) return hcg_hip_err(e);
  }
  hipLaunchKernelGGL(k_ensemble_graphs, dim3((unsigned)p->B, (unsigned)groups), dim3(XT), lds, stream, a);
  HCG_CHECK_LAUNCH();
  return HCG_OK;
}
