// Ensemble prediction (reference scripts_experiments/predict_test.py:19-103: the 90 models of the nested cross-validation
// predict the same unseen set): M frozen models of one architecture on ONE batch of graphs in ONE launch, forward only.
//
// The graphs are shared and only the weights differ, so the grid runs over (graph, group of models): one workgroup of 8 waves
// builds its graph once and then runs `models_per_group` models on it, one after the other.  Workgroups never depend on each
// other, nothing is reduced across them, no float atomics: every sum has one owner and a fixed order, so the result for
// (model, graph) is bitwise the same run to run, whatever M, the group size and the rest of the batch are.  Per workgroup:
//   build     once: gcn_norm on chip from the raw COO edges (rules: graph_csr.h) -- in-degree, dinv, the by-destination row
//             list sorted by neighbour id.  No mask, no by-source list, no workspace: there is no backward.
//             (Build, aggregation, pooling and readout are explain_tile.h's, shared with explain.hip and shapley.hip; here
//             with the plain entry word and a model index into the stacked weights.)
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
  XCommon c;                                // cW [M][64][F or 64], cb [M][64], hW [M][out_i][in_i], hb [M][out_i]
  float* out;                               // [M][B][C]
  float* emb;                               // [M][B][128] or null
  int B, M, mpg;
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
  const XCommon& cm = a.c;
  const ELds L = e_carve(smem, cm.npad, cm.emax);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x;
  const int F = cm.F, C = cm.C, n_conv = cm.n_conv, B = a.B;
  const int m_begin = (int)blockIdx.y * a.mpg;
  const int m_end = min(m_begin + a.mpg, a.M);

  XSpan sp;
  if (x_refused(sp, cm, g, tid)) {
    // the graph's outputs are zero for every model
    for (int m = m_begin; m < m_end; ++m) {
      const size_t mg = (size_t)m * B + g;
      for (int k = tid; k < C; k += XT) a.out[mg * C + k] = 0.f;
      if (a.emb)
        for (int k = tid; k < 2 * XD; k += XT) a.emb[mg * (2 * XD) + k] = 0.f;
    }
    return;
  }

  // ---------------------------------------------------------------------------------------------- build (once per workgroup)
  const int nbase = sp.nbase, n = sp.n;
  EdgeRegs<X_EPT, XT> er;
  er.load(XGraph{sp.ebase, sp.ne}, cm.ei, cm.E, tid);
  for (int i = tid; i < cm.npad; i += XT) L.cnt[i] = 0;
  XEdges q;
  x_edge_pass(q, er, sp, tid, cm.status);
  x_build_rows<XPlain, false>(q, {L.ent, L.rowptr, L.cnt}, {}, L.dinv, n, tid);
  // (the first barrier of the model loop orders the sort before the first aggregation)

#pragma nounroll
  for (int m = m_begin; m < m_end; ++m) {
    const size_t mg = (size_t)m * B + g;
    // x, zero-padded to 64 columns (t0's last readers, the pooling of the model before, are behind the readout's barriers)
    for (int idx = tid; idx < n * XD; idx += XT) {
      const int r = idx >> 6, k = idx & 63;
      L.t0[r * XS + k] = k < F ? cm.x[(size_t)(nbase + r) * F + k] : 0.f;
    }
    e_stage_weights(L.ws, cm.cW[0] + (size_t)m * XD * F, F, tid);
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
      if (l + 1 < n_conv) e_stage_weights(L.ws, x_pick(cm.cW, l + 1) + (size_t)m * XD * XD, XD, tid);
      x_conv_out(L.t1, L.t0, L.ent, L.rowptr, XPlain{}, L.dinv, x_pick(cm.cb, l) + (size_t)m * XD, n, tid, cm.slope,
                 [](int, int, float4) {});
      __syncthreads();
    }

    // -------------------------------------------------------------------------------------------- pooling (t0 = A of the last layer; max first), readout
    x_pool(L.t0, L.red, L.hv, n, tid);
    if (a.emb && tid < 2 * XD) a.emb[mg * (2 * XD) + tid] = L.hv[tid];
    const int off = x_readout(L.hv, cm, m, tid);
    if (tid < C) a.out[mg * C + tid] = L.hv[off + tid];
    // (hv and red are next written behind the barriers of the next model's conv stack)
  }
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
  if (!x_common_ok(p)) return HCG_ERR_INVALID_ARG;

  EArgs a;
  x_fill_common(a.c, p);
  a.out = p->out;
  a.emb = p->emb;
  a.B = (int)p->B;
  a.M = p->n_models;
  a.mpg = p->models_per_group;
  return x_launch<k_ensemble_graphs>(dim3((unsigned)p->B, (unsigned)groups), e_lds_bytes(a.c.npad, a.c.emax), stream, a);
}
