// Explain mode for a BATCH of graphs in one launch: outputs and the gradients with respect to an edge mask and a
// node-feature mask, weights frozen -- what one iteration of a GNNExplainer-style loop needs of the model
// (reference scripts_experiments/explain_gnn.py:39-50: Explainer(edge_mask_type='object', node_mask_type='attributes')).
//
// One workgroup of 8 waves per graph (<= 224 nodes, <= 1024 directed edges, D = 64, F <= 64); workgroups never depend on each
// other, nothing is reduced across them, no float atomics: every sum has one owner and a fixed order, so a graph's results are
// bitwise the same run to run and whatever else shares the batch.  Per graph:
//   build     gcn_norm on chip from the raw COO edges (rules: graph_csr.h).  dinv from the UNMASKED in-degree; the mask
//             multiplies the message after the normalisation.  Two entry lists, both with the edge's position in the caller's
//             order packed beside the neighbour id ((id << 16) | local edge): by destination (forward sum, edge gradient) and
//             by source (the backward's transpose sum -- the masked adjacency is not symmetric).  Rows sorted by the packed
//             word.  Explicit (i, i) edges collapse into the unit self loop: no entry, gradient 0.
//   forward   x~ = x s(node_mask) -> t0;  per layer  H = A_prev W^T (t0 -> t1; lane = output column, the lane's weight row in
//             64 registers, the tile row broadcast out of LDS, plain f32 FMAs),  A = leaky(dinv_i (dinv_i H_i + sum_k m_k dinv_c
//             H_c) + b) (t1 -> t0);  [max, mean] pooling;  readout of depth R.
//   backward  readout, pooling (max: even split among exact ties), then per layer from the last:  dY = dA leaky'(A) (t0),
//             d m_e += dinv_dst dinv_src <dY_dst, H_src> (owner: the edge's by-destination entry; layers add in layer order),
//             dH = Ahat_m^T dY (t1),  dA_prev = dH W (t1 -> t0).  No dW, no db.
// LDS holds the two [npad][64 + 4] f32 tiles and ~22 KB of edge-indexed structure (sized at launch from the batch's largest
// graph; 149 KB at the 224 / 1024 limit).  The weights (16 KB per layer, the same for every workgroup) are read from global
// memory / L2 into registers.  H_l and A_l of every layer, which the backward reads again, go to the caller's workspace
// ([2 n_conv][N][64] f32, each graph's rows written and read by its own workgroup only).
#include "common.h"
#include "graph_csr.h"
#include "explain_tile.h"

namespace {

struct XArgs {     // the kernel's argument block (device pointers by value)
  const float* x;
  const int64_t* ei;
  const int32_t* graph_ptr;
  const int32_t* edge_ptr;
  const float* edge_mask;
  const float* node_mask;
  const float* target;
  const float* dout;
  const float* cW[HCG_EXPLAIN_MAX_CONVS];
  const float* cb[HCG_EXPLAIN_MAX_CONVS];
  const float* hW[HCG_HEAD_MAX_LAYERS];
  const float* hb[HCG_HEAD_MAX_LAYERS];
  float* out;
  float* loss;
  float* d_edge_mask;
  float* d_node_mask;
  float* dx;
  int32_t* status;
  float* ws;
  long long E;
  int N, F, C, n_conv, R, npad, emax, max_nodes, max_edges, sigmoid;
  float slope;
};

struct XLds {
  float* t0;            // [npad][XS]
  float* t1;            // [npad][XS]
  unsigned* ent_d;      // [emax]  by destination: (source << 16) | local edge
  unsigned* ent_s;      // [emax]  by source: (destination << 16) | local edge
  float* mval;          // [emax]  the mask value of local edge e (after its sigmoid)
  float* eg;            // [emax]  d J / d mval[e]
  int* rowptr_d;        // [npad + 4]
  int* rowptr_s;        // [npad + 4]
  int* cnt_d;           // [npad]  in-degree, then the fill cursor
  int* cnt_s;           // [npad]
  float* dinv;          // [npad]
  float* red;           // [XW][128] pooling partials
  float* hv;            // [X_HEAD] readout activations: emb | v1 | v2 | ... | out
  float* hg;            // [X_HEAD] their gradients
};

__host__ __device__ inline unsigned x_lds_bytes(int npad, int emax) {
  return 2u * npad * XS * 4 + 4u * emax * 4 + 2u * (npad + 4) * 4 + 3u * npad * 4 + XW * 128 * 4 + 2 * X_HEAD * 4;
}

// (integer offsets, as mid.hip's carve: the arrays must stay LDS pointers for the compiler)
__device__ __forceinline__ XLds x_carve(char* base, int npad, int emax) {
  XLds L;
  unsigned off = 0;
  L.t0 = reinterpret_cast<float*>(base + off); off += (unsigned)npad * XS * 4;
  L.t1 = reinterpret_cast<float*>(base + off); off += (unsigned)npad * XS * 4;
  L.ent_d = reinterpret_cast<unsigned*>(base + off); off += (unsigned)emax * 4;
  L.ent_s = reinterpret_cast<unsigned*>(base + off); off += (unsigned)emax * 4;
  L.mval = reinterpret_cast<float*>(base + off); off += (unsigned)emax * 4;
  L.eg = reinterpret_cast<float*>(base + off); off += (unsigned)emax * 4;
  L.rowptr_d = reinterpret_cast<int*>(base + off); off += (unsigned)(npad + 4) * 4;
  L.rowptr_s = reinterpret_cast<int*>(base + off); off += (unsigned)(npad + 4) * 4;
  L.cnt_d = reinterpret_cast<int*>(base + off); off += (unsigned)npad * 4;
  L.cnt_s = reinterpret_cast<int*>(base + off); off += (unsigned)npad * 4;
  L.dinv = reinterpret_cast<float*>(base + off); off += (unsigned)npad * 4;
  L.red = reinterpret_cast<float*>(base + off); off += XW * 128 * 4;
  L.hv = reinterpret_cast<float*>(base + off); off += X_HEAD * 4;
  L.hg = reinterpret_cast<float*>(base + off);
  return L;
}

__device__ __forceinline__ float x_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

__global__ __launch_bounds__(XT) void k_explain_graphs(const XArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const XLds L = x_carve(smem, a.npad, a.emax);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x;
  const int F = a.F, C = a.C, R = a.R, n_conv = a.n_conv;
  const float slope = a.slope;
  const bool bwd = a.target != nullptr || a.dout != nullptr;
  const bool need_dx = a.d_node_mask != nullptr || a.dx != nullptr;

  const int nbase = __builtin_amdgcn_readfirstlane(a.graph_ptr[g]), ebase = __builtin_amdgcn_readfirstlane(a.edge_ptr[g]);
  const int n_raw = a.graph_ptr[g + 1] - nbase, ne_raw = a.edge_ptr[g + 1] - ebase;
  int n = n_raw, ne = ne_raw;
  graph_refuse(n, ne, a.max_nodes, a.max_edges, tid, a.status);
  if (n != n_raw || ne != ne_raw) {
    // refused (HCG_STATUS_SHAPE_LIMIT): the graph's outputs are zero -- over whatever part of its ranges lies inside the arrays
    for (int c = tid; c < C; c += XT) a.out[(size_t)g * C + c] = 0.f;
    if (a.loss && tid == 0) a.loss[g] = 0.f;
    if (bwd) {
      for (long long e = tid; e < ne_raw; e += XT) {
        const long long p = (long long)ebase + e;
        if (p >= 0 && p < a.E) a.d_edge_mask[p] = 0.f;
      }
      for (long long i = tid; i < (long long)n_raw * F; i += XT) {
        const long long p = (long long)nbase * F + i;
        if (p >= 0 && p < (long long)a.N * F) {
          if (a.d_node_mask) a.d_node_mask[p] = 0.f;
          if (a.dx) a.dx[p] = 0.f;
        }
      }
    }
    return;
  }

  // ---------------------------------------------------------------------------------------------- build
  XGraph gi{ebase, ne};
  EdgeRegs<X_EPT, XT> er;
  er.load(gi, a.ei, a.E, tid);
  for (int i = tid; i < a.npad; i += XT) { L.cnt_d[i] = 0; L.cnt_s[i] = 0; }
  for (int e = tid; e < ne; e += XT) {
    const float v = a.edge_mask[(size_t)ebase + e];
    L.mval[e] = a.sigmoid ? x_sigmoid(v) : v;
    L.eg[e] = 0.f;
  }
  // x~ = x s(node_mask), zero-padded to 64 columns
  for (int idx = tid; idx < n * XD; idx += XT) {
    const int r = idx >> 6, k = idx & 63;
    float v = 0.f;
    if (k < F) {
      const size_t p = (size_t)(nbase + r) * F + k;
      v = a.x[p];
      if (a.node_mask) {
        const float m = a.node_mask[p];
        v *= a.sigmoid ? x_sigmoid(m) : m;
      }
    }
    L.t0[r * XS + k] = v;
  }
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
    if (live[j]) { atomicAdd(&L.cnt_d[ed[j]], 1); atomicAdd(&L.cnt_s[es[j]], 1); }
  __syncthreads();
  if (wave == 0) csr_scan_rows<X_RPL>(L.cnt_d, L.rowptr_d, n, lane);
  else if (wave == 1) csr_scan_rows<X_RPL>(L.cnt_s, L.rowptr_s, n, lane);
  for (int i = tid; i < n; i += XT) L.dinv[i] = gcn_dinv(L.cnt_d[i]);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < X_EPT; ++j)
    if (live[j]) {
      const unsigned e = (unsigned)(tid + j * XT);
      const int pd = L.rowptr_d[ed[j]] + atomicSub(&L.cnt_d[ed[j]], 1) - 1;
      L.ent_d[pd] = ((unsigned)es[j] << 16) | e;
      const int ps = L.rowptr_s[es[j]] + atomicSub(&L.cnt_s[es[j]], 1) - 1;
      L.ent_s[ps] = ((unsigned)ed[j] << 16) | e;
    }
  __syncthreads();
  if (tid < n) x_sort_row(L.ent_d, L.rowptr_d[tid], L.rowptr_d[tid + 1]);
  else if (tid >= XT / 2 && tid - XT / 2 < n) x_sort_row(L.ent_s, L.rowptr_s[tid - XT / 2], L.rowptr_s[tid - XT / 2 + 1]);
  __syncthreads();

  const size_t plane = (size_t)a.N * XD;                  // one [N][64] tensor of the workspace
  float* const wsg = a.ws + (size_t)nbase * XD;           // this graph's rows of plane 0
  const int arow = tid >> 4, c4 = tid & 15;               // aggregation: 16 lanes x float4 per row, 32 rows per pass

  // ---------------------------------------------------------------------------------------------- forward
#pragma nounroll
  for (int l = 0; l < n_conv; ++l) {
    const int K = __builtin_amdgcn_readfirstlane(l == 0 ? F : XD);   // (uniform: keeps the weight addressing scalar)
    {
      float w[XD];
      x_weight_row(w, reinterpret_cast<const char*>(x_pick(a.cW, l)), lane, K);
      float* hws = wsg + (size_t)(2 * l) * plane;
      x_gemm(L.t0, w, n, wave, [&](int r, float v) {
        L.t1[r * XS + lane] = v;
        if (bwd) hws[(size_t)r * XD + lane] = v;
      });
    }
    __syncthreads();
    {
      float bb[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) bb[j] = x_pick(a.cb, l)[4 * c4 + j];
      float* aws = wsg + (size_t)(2 * l + 1) * plane;
      for (int row = arow; row < n; row += XT / 16) {
        const float di = L.dinv[row];
        const float4 s = x_row_sum(L.t1, L.ent_d, L.mval, L.dinv, row, L.rowptr_d[row], L.rowptr_d[row + 1], c4, di);
        float4 y = make_float4(fmaf(di, s.x, bb[0]), fmaf(di, s.y, bb[1]), fmaf(di, s.z, bb[2]), fmaf(di, s.w, bb[3]));
        y = make_float4(hcg_leaky(y.x, slope), hcg_leaky(y.y, slope), hcg_leaky(y.z, slope), hcg_leaky(y.w, slope));
        *reinterpret_cast<float4*>(L.t0 + row * XS + 4 * c4) = y;
        if (bwd && l + 1 < n_conv) *reinterpret_cast<float4*>(aws + (size_t)row * XD + 4 * c4) = y;
      }
    }
    __syncthreads();
  }

  // ---------------------------------------------------------------------------------------------- pooling: t0 = A of the last layer
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
    L.hv[tid] = n > 0 ? mx : 0.f;
    L.hv[64 + tid] = n > 0 ? sm / (float)n : 0.f;
  }
  __syncthreads();

  // ---------------------------------------------------------------------------------------------- readout (8 lanes per output)
  int off = 0;
  for (int i = 0; i < R; ++i) {
    const int in_i = (2 * XD) >> i, out_i = i == R - 1 ? C : in_i / 2;
    const int o = tid >> 3, sub = tid & 7;
    float p = 0.f;
    if (o < out_i) {
      const float* W = x_pick(a.hW, i) + (size_t)o * in_i;
      for (int k = sub; k < in_i; k += 8) p = fmaf(W[k], L.hv[off + k], p);
    }
    p += __shfl_xor(p, 1, 8);
    p += __shfl_xor(p, 2, 8);
    p += __shfl_xor(p, 4, 8);
    if (o < out_i && sub == 0) {
      const float y = p + x_pick(a.hb, i)[o];
      L.hv[off + in_i + o] = i == R - 1 ? y : hcg_leaky(y, slope);
    }
    off += in_i;
    __syncthreads();
  }
  // off = position of the output row in hv / hg
  if (tid < C) {
    const float o = L.hv[off + tid];
    a.out[(size_t)g * C + tid] = o;
    float d = 0.f;
    if (a.target) d = o - a.target[(size_t)g * C + tid];
    L.red[tid] = d * d;
    L.hg[off + tid] = a.target ? 2.f * d / (float)C : (a.dout ? a.dout[(size_t)g * C + tid] : 0.f);
  }
  __syncthreads();
  if (a.loss && tid == 0) {
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += L.red[c];
    a.loss[g] = a.target ? s / (float)C : 0.f;
  }
  if (!bwd) return;

  // ---------------------------------------------------------------------------------------------- readout backward
  for (int i = R - 1; i >= 0; --i) {
    const int in_i = (2 * XD) >> i, out_i = i == R - 1 ? C : in_i / 2;
    off -= in_i;                                        // layer i's input vector; its output sits at off + in_i
    if (tid < in_i) {
      const float* W = x_pick(a.hW, i) + tid;
      float s = 0.f;
      for (int o = 0; o < out_i; ++o) s = fmaf(W[(size_t)o * in_i], L.hg[off + in_i + o], s);
      if (i > 0) s *= hcg_leaky_grad(L.hv[off + tid], slope);
      L.hg[off + tid] = s;
    }
    __syncthreads();
  }
  // hg[0 .. 128) = d J / d emb

  // ---------------------------------------------------------------------------------------------- pooling backward
  {
    const float mx = L.hv[lane];
    float cnt = 0.f;
    for (int r = wave; r < n; r += XW) cnt += L.t0[r * XS + lane] == mx ? 1.f : 0.f;
    L.red[wave * 128 + lane] = cnt;
  }
  __syncthreads();
  if (tid < 64) {
    float cnt = 0.f;
#pragma unroll
    for (int w = 0; w < XW; ++w) cnt += L.red[w * 128 + tid];
    L.red[XW * 128 - 64 + tid] = L.hg[tid] / fmaxf(cnt, 1.f);        // (the upper half of the last wave's slot: unused)
  }
  __syncthreads();
  {
    const float gmax = L.red[XW * 128 - 64 + lane], mx = L.hv[lane];
    const float gmean = n > 0 ? L.hg[64 + lane] / (float)n : 0.f;
    for (int r = wave; r < n; r += XW) {
      const float v = L.t0[r * XS + lane];
      const float da = (v == mx ? gmax : 0.f) + gmean;
      L.t0[r * XS + lane] = da * hcg_leaky_grad(v, slope);          // dY of the last layer
    }
  }
  __syncthreads();

  // ---------------------------------------------------------------------------------------------- conv layers, last to first
#pragma nounroll
  for (int l = n_conv - 1; l >= 0; --l) {
    const int K = __builtin_amdgcn_readfirstlane(l == 0 ? F : XD);   // (uniform: keeps the weight addressing scalar)
    const float* hws = wsg + (size_t)(2 * l) * plane;
    for (int idx = tid; idx < n * (XD / 4); idx += XT) {
      const int r = idx >> 4, q = idx & 15;
      *reinterpret_cast<float4*>(L.t1 + r * XS + 4 * q) = *reinterpret_cast<const float4*>(hws + (size_t)r * XD + 4 * q);
    }
    __syncthreads();
    // edge gradient: every by-destination entry owns its edge's slot
    for (int row = arow; row < n; row += XT / 16) {
      const float4 dy = *reinterpret_cast<const float4*>(L.t0 + row * XS + 4 * c4);
      const float di = L.dinv[row];
      const int kb = L.rowptr_d[row], ke = L.rowptr_d[row + 1];
      for (int k = kb; k < ke; ++k) {
        const unsigned en = L.ent_d[k];
        const int c = (int)(en >> 16), e = (int)(en & 0xffffu);
        const float4 h = *reinterpret_cast<const float4*>(L.t1 + c * XS + 4 * c4);
        float s = fmaf(dy.w, h.w, fmaf(dy.z, h.z, fmaf(dy.y, h.y, dy.x * h.x)));
        s += __shfl_xor(s, 1, 16);
        s += __shfl_xor(s, 2, 16);
        s += __shfl_xor(s, 4, 16);
        s += __shfl_xor(s, 8, 16);
        if (c4 == 0) L.eg[e] += di * L.dinv[c] * s;
      }
    }
    if (l == 0 && !need_dx) break;
    __syncthreads();
    // dH = Ahat_m^T dY: rows of the by-source list
    for (int row = arow; row < n; row += XT / 16) {
      const float di = L.dinv[row];
      const float4 s = x_row_sum(L.t0, L.ent_s, L.mval, L.dinv, row, L.rowptr_s[row], L.rowptr_s[row + 1], c4, di);
      *reinterpret_cast<float4*>(L.t1 + row * XS + 4 * c4) = make_float4(di * s.x, di * s.y, di * s.z, di * s.w);
    }
    __syncthreads();
    // dA_prev = dH W (lane = input column k), times leaky'(A_prev) for a hidden layer
    {
      float w[XD];
      const char* Wb = reinterpret_cast<const char*>(x_pick(a.cW, l));
      const unsigned col = (unsigned)(lane < K ? lane : K - 1);
      unsigned Kv = (unsigned)K;
      asm volatile("" : "+v"(Kv));          // (opaque: the row offsets stay 32-bit vector offsets on the one uniform base)
#pragma unroll
      for (int d = 0; d < XD; ++d) {
        const float v = *reinterpret_cast<const float*>(Wb + 4u * ((unsigned)d * Kv + col));
        w[d] = lane < K ? v : 0.f;
        if ((d & 15) == 15) __builtin_amdgcn_sched_barrier(0);
      }
      const float* aprev = l > 0 ? wsg + (size_t)(2 * (l - 1) + 1) * plane : nullptr;
      x_gemm(L.t1, w, n, wave, [&](int r, float v) {
        if (l > 0) v *= hcg_leaky_grad(aprev[(size_t)r * XD + lane], slope);
        L.t0[r * XS + lane] = v;
      });
    }
    __syncthreads();
  }
  __syncthreads();

  // ---------------------------------------------------------------------------------------------- outputs
  for (int e = tid; e < ne; e += XT) {
    const float m = L.mval[e];
    a.d_edge_mask[(size_t)ebase + e] = a.sigmoid ? L.eg[e] * (m * (1.f - m)) : L.eg[e];
  }
  if (need_dx) {
    for (int idx = tid; idx < n * XD; idx += XT) {
      const int r = idx >> 6, k = idx & 63;
      if (k < F) {
        const size_t p = (size_t)(nbase + r) * F + k;
        const float dxt = L.t0[r * XS + k];
        float s = 1.f, ds = 1.f;
        if (a.node_mask) {
          const float m = a.node_mask[p];
          s = a.sigmoid ? x_sigmoid(m) : m;
          ds = a.sigmoid ? s * (1.f - s) : 1.f;
          a.d_node_mask[p] = dxt * a.x[p] * ds;
        }
        if (a.dx) a.dx[p] = dxt * s;
      }
    }
  }
}

hipError_t explain_allow_big_lds() {   // dynamic LDS above 64 KB: allowed once per process (not per launch: it may be under capture)
  static hipError_t st = hipFuncSetAttribute((const void*)k_explain_graphs, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  return st;
}

}  // namespace

extern "C" int hcg_explain(hcg_explain_args* p, hcg_stream_t stream_) {
  if (!p) return HCG_ERR_INVALID_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  if (p->mode == HCG_EXPLAIN_LAYER_EDGE_GRAD) {
    if (p->flags & HCG_EXPLAIN_QUERY) { p->workspace_bytes_needed = 0; return HCG_OK; }
    return hcg_edge_weight_grad_launch(p->layer_dout, p->layer_out, p->layer_h, p->rowptr, p->col, p->dinv, p->slope,
                                       p->apply_act, p->dew_csr, p->N, p->E, p->D, stream);
  }
  if (p->mode == HCG_EXPLAIN_ENSEMBLE) return hcg_ensemble_launch(p, stream);
  if (p->mode == HCG_EXPLAIN_SHAPLEY) return hcg_shapley_launch(p, stream);
  if (p->mode != HCG_EXPLAIN_GRAPHS) return HCG_ERR_INVALID_ARG;
  if (!x_shapes_ok(p)) return HCG_ERR_UNSUPPORTED;
  // H_l and A_l of every layer, [N][64] f32 each: the backward reads them again
  p->workspace_bytes_needed = hcg_align_up((size_t)2 * p->n_conv * (size_t)(p->N > 0 ? p->N : 1) * XD * sizeof(float), 256);
  if (p->flags & HCG_EXPLAIN_QUERY) return HCG_OK;
  if (p->B == 0) return HCG_OK;
  const bool bwd = p->target || p->dout;
  if (p->target && p->dout) return HCG_ERR_INVALID_ARG;
  if (!p->graph_ptr || !p->edge_ptr || !p->out || !p->status || (p->N > 0 && !p->x) || (p->E > 0 && (!p->edge_index || !p->edge_mask)))
    return HCG_ERR_INVALID_ARG;
  if (bwd && ((p->E > 0 && !p->d_edge_mask) || (p->node_mask && !p->d_node_mask) || (p->target && !p->loss))) return HCG_ERR_INVALID_ARG;
  if (!p->node_mask && p->d_node_mask) return HCG_ERR_INVALID_ARG;
  for (int l = 0; l < p->n_conv; ++l)
    if (!p->conv_W[l] || !p->conv_b[l]) return HCG_ERR_INVALID_ARG;
  for (int i = 0; i < p->R; ++i)
    if (!p->head_W[i] || !p->head_b[i]) return HCG_ERR_INVALID_ARG;
  if (bwd && (!p->workspace || p->workspace_bytes < p->workspace_bytes_needed)) return HCG_ERR_WORKSPACE;

  XArgs a;
  a.x = p->x;
  a.ei = p->edge_index;
  a.E = p->E;
  if (p->E == 0) { a.ei = reinterpret_cast<const int64_t*>(p->graph_ptr); a.E = 1; }   // readable dummy; no graph has edges
  a.graph_ptr = p->graph_ptr;
  a.edge_ptr = p->edge_ptr;
  a.edge_mask = p->edge_mask;
  a.node_mask = p->node_mask;
  a.target = p->target;
  a.dout = p->dout;
  for (int l = 0; l < HCG_EXPLAIN_MAX_CONVS; ++l) { a.cW[l] = p->conv_W[l]; a.cb[l] = p->conv_b[l]; }
  for (int i = 0; i < HCG_HEAD_MAX_LAYERS; ++i) { a.hW[i] = p->head_W[i]; a.hb[i] = p->head_b[i]; }
  a.out = p->out;
  a.loss = p->loss;
  a.d_edge_mask = p->d_edge_mask;
  a.d_node_mask = bwd ? p->d_node_mask : nullptr;
  a.dx = bwd ? p->dx : nullptr;
  a.status = p->status;
  a.ws = (float*)p->workspace;
  a.N = (int)p->N;
  a.F = (int)p->F;
  a.C = (int)p->C;
  a.n_conv = p->n_conv;
  a.R = p->R;
  a.npad = (int)((p->max_nodes + 3) / 4 * 4 > 4 ? (p->max_nodes + 3) / 4 * 4 : 4);
  a.emax = (int)((p->max_edges + 3) / 4 * 4 > 4 ? (p->max_edges + 3) / 4 * 4 : 4);
  a.max_nodes = (int)p->max_nodes;
  a.max_edges = (int)p->max_edges;
  a.sigmoid = (p->flags & HCG_EXPLAIN_SIGMOID) ? 1 : 0;
  a.slope = p->slope;
  const unsigned lds = x_lds_bytes(a.npad, a.emax);
  if (lds > 64 * 1024) {
    const hipError_t e = explain_allow_big_lds();
    if (e != hipSuccess) return hcg_hip_err(e);
  }
  hipLaunchKernelGGL(k_explain_graphs, dim3((unsigned)p->B), dim3(XT), lds, stream, a);
  HCG_CHECK_LAUNCH();
  return HCG_OK;
}
