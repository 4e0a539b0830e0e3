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
//   upstream  at the output row, one of three forms (uniform per launch): target [B, C] -> mean squared error, 2 (out - target) / C;
//             dout [B, C] as given;  target_class [B] (int64 class index) -> cross-entropy -log_softmax(out)[y],
//             softmax(out) - onehot(y), float32 with the maximum subtracted, the index compared and never used as an address.
//   backward  readout, pooling (max: even split among exact ties), then per layer from the last:  dY = dA leaky'(A) (t0),
//             d m_e += dinv_dst dinv_src <dY_dst, H_src> (owner: the edge's by-destination entry; layers add in layer order),
//             dH = Ahat_m^T dY (t1),  dA_prev = dH W (t1 -> t0).  No dW, no db.
// LDS holds the two [npad][64 + 4] f32 tiles and ~22 KB of edge-indexed structure (sized at launch from the batch's largest
// graph; 149 KB at the 224 / 1024 limit).  The weights (16 KB per layer, the same for every workgroup) are read from global
// memory / L2 into registers.  H_l and A_l of every layer, which the backward reads again, go to the caller's workspace
// ([2 n_conv][N][64] f32, each graph's rows written and read by its own workgroup only).
// The build and the forward are the pieces of explain_tile.h, shared with ensemble.hip and shapley.hip (here: both row
// lists in one build, the packed entry word, the workspace store as the aggregation's extra); the backward is this file's.
//
// HCG_EXPLAIN_FIT is the same kernel body instantiated with FIT = true (k_explain_graphs<true>): the whole GNNExplainer
// mask optimisation of every graph in one launch.  The graph is built once; then `epochs` times: mask values and the masked
// input tile from the LOGITS in the caller's state buffers, the forward, the prediction loss, the backward above, and --
// instead of storing the gradients -- the regularisers' gradients, one Adam step on the graph's own entries of the state
// (logit, exp_avg, exp_avg_sq; the rule of common.h hcg_adam_update, bias corrections from the integer step as optim.hip
// derives them) and, in the step-0 epoch, the hard flags (gradient != 0) and their per-graph counts.  Every entry of the
// state is read and written by ONE thread of the graph's workgroup (the same in every epoch); the counts are integers.  So a
// fit split into several launches repeats the single launch bit for bit.  FIT = false compiles to what the kernel was
// before the template existed (same VGPRs, no scratch, same LDS): every FIT branch is `if constexpr`.
//
// HCG_EXPLAIN_INTEGRATED is the third instantiation (k_explain_graphs<false, true>): integrated gradients of one output column
// along the straight path from masks of 0 to masks of 1.  The graph is built once; then for every quadrature point of the
// launch: mask values and the masked input tile from alpha_k (no sigmoid), the forward, the upstream gradient 1 at the
// column, the backward above, and -- instead of storing the two mask gradients -- acc = fmaf(w_k, g, acc) on the caller's
// attribution arrays.  Every accumulator entry belongs to ONE thread of the graph's workgroup (the index maps of the
// outputs below), the same in every step, and step 0 starts from 0 whatever the arrays hold: a path split into several
// launches repeats the single launch bit for bit.  The launch that holds step 0 first runs two forward-only passes (t = -2:
// masks of 1, t = -1: masks of 0) for out_full / out_base.  The other two instantiations compile to what they were.
// With n_models = M the launch is dim3(B, M): workgroup (g, m) runs graph g's path with model m of weights stacked along a
// leading model axis (ensemble.hip's layout) into slice m of the workspace, of the accumulators ([M][N][F], [M][E]) and of
// out_full / out_base ([M][B][C]).  The model index is uniform: scalar offsets only, 148 VGPRs with and without it.
//
// HCG_EXPLAIN_MOMENTS (k_model_moments, at the end of this file): mean and standard deviation over that model axis.
#include "common.h"
#include "graph_csr.h"
#include "explain_tile.h"

namespace {

struct XArgs {     // the kernel's argument block (device pointers by value)
  XCommon c;
  const float* edge_mask;
  const float* node_mask;
  const float* target;
  const float* dout;
  const int64_t* target_class;
  float* out;
  float* loss;
  float* d_edge_mask;
  float* d_node_mask;
  float* dx;
  float* ws;
  int N, sigmoid;
};

struct XFit {      // what HCG_EXPLAIN_FIT adds (FIT = true only)
  float* e_logit; float* e_m; float* e_v; unsigned char* e_hard;     // [E]     edge state
  float* n_logit; float* n_m; float* n_v; unsigned char* n_hard;     // [N][F]  node-feature state
  int32_t* hard_count;                                               // [B][2]  hard edges, hard node entries
  float* loss_hist;                                                  // [epochs][B]
  float* edge_out;                                                   // [E]     s(logit) of the hard entries, else 0
  float* node_out;                                                   // [N][F]
  int step_first, epochs, B;
  float lr, b1, b2, eps;
  float edge_size, edge_ent, node_size, node_ent;
};

struct XFitArgs { XArgs a; XFit f; };

struct XPath {     // what HCG_EXPLAIN_INTEGRATED adds (PATH = true only); a.out is out_full
  const float* alpha; const float* weight;                           // [n_steps] quadrature points and weights
  float* node_attr;                                                  // [N][F]  IN/OUT accumulators
  float* edge_attr;                                                  // [E]
  float* out_base;                                                   // [B][C]
  int step_first, steps, cls;
  int B;                                                             // graphs: the model stride of out_full / out_base is B C
  unsigned long long ws_model;                                       // floats of one model's workspace slice
};

struct XPathArgs { XArgs a; XPath f; };

template <bool FIT, bool PATH = false> struct XKernelArgs { using type = XArgs; };
template <> struct XKernelArgs<true, false> { using type = XFitArgs; };
template <> struct XKernelArgs<false, true> { using type = XPathArgs; };
__device__ __forceinline__ const XArgs& x_base(const XArgs& a) { return a; }
__device__ __forceinline__ const XArgs& x_base(const XFitArgs& a) { return a.a; }
__device__ __forceinline__ const XArgs& x_base(const XPathArgs& a) { return a.a; }

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

// d ent(m) / d m of ent(m) = -m log(m + EPS) - (1 - m) log(1 - m + EPS), differentiated as written
__device__ __forceinline__ float x_dent(float m) {
  constexpr float EPS = 1e-15f;
  const float a = m + EPS, b = (1.f - m) + EPS;
  return (logf(b) + (1.f - m) / b) - (logf(a) + m / a);
}

template <bool FIT, bool PATH = false>
__global__ __launch_bounds__(XT) void k_explain_graphs(const typename XKernelArgs<FIT, PATH>::type args) {
  static_assert(!(FIT && PATH), "one loop or the other");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const XArgs& a = x_base(args);
  const XCommon& cm = a.c;
  const XLds L = x_carve(smem, cm.npad, cm.emax);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x;
  const int F = cm.F, C = cm.C, n_conv = cm.n_conv;
  const float slope = cm.slope;
  // PATH: the model of this workgroup (grid y) of weights stacked [M][...]; uniform, so every offset below is scalar.  The
  // other instantiations have one model: mdl is the constant 0 and every product with it folds away.
  const unsigned mdl = PATH ? blockIdx.y : 0u;
  const bool bwd = FIT || PATH || a.target != nullptr || a.dout != nullptr || a.target_class != nullptr;
  const bool need_dx = FIT || PATH || a.d_node_mask != nullptr || a.dx != nullptr;
  const bool sig = !PATH && (FIT || a.sigmoid);

  XSpan sp;
  if (x_refused(sp, cm, g, tid)) {
    // the graph's outputs are zero -- over whatever part of its ranges lies inside the arrays
    const int nbase = sp.nbase, ebase = sp.ebase, n_raw = sp.n_raw, ne_raw = sp.ne_raw;
    float* out0 = a.out;
    if constexpr (PATH) out0 += (size_t)mdl * args.f.B * C;
    for (int k = tid; k < C; k += XT) out0[(size_t)g * C + k] = 0.f;
    // (FIT: the masks and the loss history; the graph's state is left as it came.  PATH: model mdl's slices)
    float* d_e = a.d_edge_mask;
    float* d_n = a.d_node_mask;
    if constexpr (FIT) {
      d_e = args.f.edge_out;
      d_n = args.f.node_out;
      for (int t = tid; t < args.f.epochs; t += XT) args.f.loss_hist[(size_t)t * args.f.B + g] = 0.f;
    } else if constexpr (PATH) {
      d_e = args.f.edge_attr + (size_t)mdl * (size_t)cm.E;
      d_n = args.f.node_attr + (size_t)mdl * (size_t)a.N * F;
      for (int k = tid; k < C; k += XT) args.f.out_base[((size_t)mdl * args.f.B + g) * C + k] = 0.f;
    } else {
      if (a.loss && tid == 0) a.loss[g] = 0.f;
    }
    if (bwd) {
      for (long long e = tid; e < ne_raw; e += XT) {
        const long long p = (long long)ebase + e;
        if (p >= 0 && p < cm.E) d_e[p] = 0.f;
      }
      for (long long i = tid; i < (long long)n_raw * F; i += XT) {
        const long long p = (long long)nbase * F + i;
        if (p >= 0 && p < (long long)a.N * F) {
          if (d_n) d_n[p] = 0.f;
          if (a.dx) a.dx[p] = 0.f;
        }
      }
    }
    return;
  }

  // ---------------------------------------------------------------------------------------------- build
  const int nbase = sp.nbase, ebase = sp.ebase, n = sp.n, ne = sp.ne;
  EdgeRegs<X_EPT, XT> er;
  er.load(XGraph{sp.ebase, sp.ne}, cm.ei, cm.E, tid);
  for (int i = tid; i < cm.npad; i += XT) { L.cnt_d[i] = 0; L.cnt_s[i] = 0; }
  // the mask values, and x~ = x s(node_mask), zero-padded to 64 columns (once; FIT: from the logits, at every epoch's start)
  auto stage_masks = [&](const float* em, const float* nm) {
    for (int e = tid; e < ne; e += XT) {
      const float v = em[(size_t)ebase + e];
      L.mval[e] = sig ? x_sigmoid(v) : v;
      L.eg[e] = 0.f;
    }
    for (int idx = tid; idx < n * XD; idx += XT) {
      const int r = idx >> 6, k = idx & 63;
      float v = 0.f;
      if (k < F) {
        const size_t p = (size_t)(nbase + r) * F + k;
        v = cm.x[p];
        if (nm) {
          const float m = nm[p];
          v *= sig ? x_sigmoid(m) : m;
        }
      }
      L.t0[r * XS + k] = v;
    }
  };
  if constexpr (!FIT && !PATH) stage_masks(a.edge_mask, a.node_mask);
  XEdges q;
  x_edge_pass(q, er, sp, tid, cm.status);
  const XMasked fmt{L.mval};
  x_build_rows<XMasked, true>(q, {L.ent_d, L.rowptr_d, L.cnt_d}, {L.ent_s, L.rowptr_s, L.cnt_s}, L.dinv, n, tid);
  __syncthreads();

  const size_t plane = (size_t)a.N * XD;                  // one [N][64] tensor of the workspace
  float* wsg = a.ws + (size_t)nbase * XD;                 // this graph's rows of plane 0
  // PATH: model mdl's slices of the workspace, the accumulators and the two output arrays
  [[maybe_unused]] float* p_node = nullptr;
  [[maybe_unused]] float* p_edge = nullptr;
  [[maybe_unused]] float* p_full = nullptr;
  [[maybe_unused]] float* p_base = nullptr;
  if constexpr (PATH) {
    wsg += (size_t)mdl * args.f.ws_model;
    p_node = args.f.node_attr + (size_t)mdl * (size_t)a.N * F;
    p_edge = args.f.edge_attr + (size_t)mdl * (size_t)cm.E;           // (E = 0: nothing is addressed)
    p_full = a.out + (size_t)mdl * args.f.B * C;
    p_base = args.f.out_base + (size_t)mdl * args.f.B * C;
  }

  // FIT: the hard counts (behind the tiles and lists in LDS), from the state unless this launch holds the step-0 epoch
  [[maybe_unused]] int* const hc = reinterpret_cast<int*>(smem + x_lds_bytes(cm.npad, cm.emax));
  int epochs = 1;
  if constexpr (FIT) {
    epochs = args.f.epochs;
    if (tid < 2) hc[tid] = args.f.step_first > 0 ? args.f.hard_count[2 * g + tid] : 0;
  }
  int t = 0;
  if constexpr (PATH) {
    epochs = args.f.steps;
    t = args.f.step_first == 0 ? -2 : 0;                  // (the two forward-only passes come first)
  }

#pragma nounroll
  for (; t < epochs; ++t) {
  float* loss_out = a.loss;
  if constexpr (FIT) {
    loss_out = args.f.loss_hist + (size_t)t * args.f.B;
    stage_masks(args.f.e_logit, args.f.n_logit);
    __syncthreads();
  }
  if constexpr (PATH) {
    // every mask entry of the graph = alpha_k (t = -2: 1, t = -1: 0), x~ = x alpha_k, zero-padded to 64 columns
    const float al = t < 0 ? (t == -2 ? 1.f : 0.f) : args.f.alpha[args.f.step_first + t];
    for (int e = tid; e < ne; e += XT) {
      L.mval[e] = al;
      L.eg[e] = 0.f;
    }
    for (int idx = tid; idx < n * XD; idx += XT) {
      const int r = idx >> 6, k = idx & 63;
      L.t0[r * XS + k] = k < F ? cm.x[(size_t)(nbase + r) * F + k] * al : 0.f;
    }
    __syncthreads();
  }

  // ---------------------------------------------------------------------------------------------- forward
#pragma nounroll
  for (int l = 0; l < n_conv; ++l) {
    const int K = __builtin_amdgcn_readfirstlane(l == 0 ? F : XD);   // (uniform: keeps the weight addressing scalar)
    {
      float w[XD];
      x_weight_row(w, reinterpret_cast<const char*>(x_pick(cm.cW, l) + (size_t)mdl * XD * K), lane, K);
      float* hws = wsg + (size_t)(2 * l) * plane;
      x_gemm(L.t0, w, n, wave, [&](int r, float v) {
        L.t1[r * XS + lane] = v;
        if (bwd) hws[(size_t)r * XD + lane] = v;
      });
    }
    __syncthreads();
    float* aws = wsg + (size_t)(2 * l + 1) * plane;
    x_conv_out(L.t1, L.t0, L.ent_d, L.rowptr_d, fmt, L.dinv, x_pick(cm.cb, l) + (size_t)mdl * XD, n, tid, slope, [&](int row, int c4, float4 y) {
      if (bwd && l + 1 < n_conv) *reinterpret_cast<float4*>(aws + (size_t)row * XD + 4 * c4) = y;
    });
    __syncthreads();
  }

  // ---------------------------------------------------------------------------------------------- pooling (t0 = A of the last layer), readout
  x_pool(L.t0, L.red, L.hv, n, tid);
  int off = x_readout(L.hv, cm, (int)mdl, tid);
  // off = position of the output row in hv / hg
  if (tid < C) {
    const float o = L.hv[off + tid];
    if constexpr (PATH) {
      // out_full / out_base from the forward-only passes; upstream: 1 at the column (compared, never an address)
      if (t == -2) p_full[(size_t)g * C + tid] = o;
      if (t == -1) p_base[(size_t)g * C + tid] = o;
      L.hg[off + tid] = tid == args.f.cls ? 1.f : 0.f;
    } else {
    a.out[(size_t)g * C + tid] = o;
    if (a.target_class) {
      // cross-entropy against class y (uniform per launch): every thread below C restates the row from hv.  y is compared,
      // never used as an address: outside 0 .. C - 1 no class matches -- the loss is NaN, the gradient softmax(out)
      const long long y = a.target_class[g];
      float mx = L.hv[off];
      for (int c = 1; c < C; ++c) mx = fmaxf(mx, L.hv[off + c]);
      // s = sum_c exp(o_c - mx), c ascending; `others` leaves out class y, `rest` the first maximal class (whose term is 1)
      float s = 0.f, others = 0.f, rest = 0.f, oy = __builtin_nanf("");
      bool first = true;
      for (int c = 0; c < C; ++c) {
        const float v = L.hv[off + c], ex = expf(v - mx);
        s += ex;
        if (c == y) oy = v; else others += ex;
        if (first && v == mx) first = false; else rest += ex;
      }
      // softmax(out)_c - [c == y]; for c = y that is -(sum of the others) / s, formed without the cancelling subtraction
      L.hg[off + tid] = tid == y ? -others / s : expf(o - mx) / s;
      L.red[tid] = log1pf(rest) + (mx - oy);              // -log_softmax(out)[y]: two terms that are not negative
    } else {
      float d = 0.f;
      if (a.target) d = o - a.target[(size_t)g * C + tid];
      L.red[tid] = d * d;
      L.hg[off + tid] = a.target ? 2.f * d / (float)C : (a.dout ? a.dout[(size_t)g * C + tid] : 0.f);
    }
    }
  }
  __syncthreads();
  if constexpr (PATH) {
    if (t < 0) continue;                                  // (uniform; nothing reads the tiles behind this barrier)
  }
  if (loss_out && tid == 0) {
    if (a.target_class) {
      loss_out[g] = L.red[0];
    } else {
      float s = 0.f;
      for (int c = 0; c < C; ++c) s += L.red[c];
      loss_out[g] = a.target ? s / (float)C : 0.f;
    }
  }
  if (!bwd) return;

  // ---------------------------------------------------------------------------------------------- readout backward
  for (int i = cm.R - 1; i >= 0; --i) {
    const int in_i = (2 * XD) >> i, out_i = i == cm.R - 1 ? C : in_i / 2;
    off -= in_i;                                        // layer i's input vector; its output sits at off + in_i
    if (tid < in_i) {
      const float* W = x_pick(cm.hW, i) + (size_t)mdl * out_i * in_i + tid;
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
    const int arow = tid >> 4, c4 = tid & 15;             // 16 lanes x float4 per row, 32 rows per pass
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
      const float4 s = x_row_sum(L.t0, L.ent_s, fmt, L.dinv, row, L.rowptr_s[row], L.rowptr_s[row + 1], c4, di);
      *reinterpret_cast<float4*>(L.t1 + row * XS + 4 * c4) = make_float4(di * s.x, di * s.y, di * s.z, di * s.w);
    }
    __syncthreads();
    // dA_prev = dH W (lane = input column k), times leaky'(A_prev) for a hidden layer
    {
      float w[XD];
      const char* Wb = reinterpret_cast<const char*>(x_pick(cm.cW, l) + (size_t)mdl * XD * K);
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

  if constexpr (PATH) {
  // ---------------------------------------------------------------------------------------------- PATH: acc = fmaf(w_k, g, acc)
  // Entry p of the accumulators belongs to the thread that reads it here (the index maps of the outputs below), in every step.
  const XPath& f = args.f;
  const int step = f.step_first + t;
  const float wk = f.weight[step];
  const bool fresh = step == 0;                           // the path starts from 0 whatever the arrays hold
  for (int e = tid; e < ne; e += XT) {
    const size_t p = (size_t)ebase + e;
    p_edge[p] = fmaf(wk, L.eg[e], fresh ? 0.f : p_edge[p]);
  }
  for (int idx = tid; idx < n * XD; idx += XT) {
    const int r = idx >> 6, k = idx & 63;
    if (k < F) {
      const size_t p = (size_t)(nbase + r) * F + k;
      p_node[p] = fmaf(wk, L.t0[r * XS + k] * cm.x[p], fresh ? 0.f : p_node[p]);
    }
  }
  __syncthreads();                                        // (the next step stages over t0 and eg)
  } else if constexpr (!FIT) {
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
          a.d_node_mask[p] = dxt * cm.x[p] * ds;
        }
        if (a.dx) a.dx[p] = dxt * s;
      }
    }
  }
  } else {
  // ---------------------------------------------------------------------------------------------- FIT: regularisers, Adam, hard flags
  // Entry p of the state belongs to the thread that staged it (same index maps as stage_masks), in every epoch.
  const XFit& f = args.f;
  const int step = f.step_first + t;                      // Adam steps taken before this epoch
  const bool reg = step > 0;                              // the hard masks exist from the epoch after step 0
  const float step_size = f.lr / (float)(1.0 - hcg_powi((double)f.b1, step + 1));
  const float bc2_sqrt = (float)sqrt(1.0 - hcg_powi((double)f.b2, step + 1));
  const int hce = hc[0], hcn = hc[1];                     // (written before the barrier that ended the last epoch)
  const float inv_e = hce > 0 ? 1.f / (float)hce : 0.f, inv_n = hcn > 0 ? 1.f / (float)hcn : 0.f;
  int found_e = 0, found_n = 0;
  for (int e = tid; e < ne; e += XT) {
    const size_t p = (size_t)ebase + e;
    const float m = L.mval[e], ds = m * (1.f - m);
    float gr = L.eg[e] * ds;
    if (reg && f.e_hard[p]) gr += (f.edge_size + f.edge_ent * inv_e * x_dent(m)) * ds;
    float mi = f.e_m[p], vi = f.e_v[p];
    f.e_logit[p] = hcg_adam_update(f.e_logit[p], gr, mi, vi, f.b1, f.b2, f.eps, step_size, bc2_sqrt);
    f.e_m[p] = mi;
    f.e_v[p] = vi;
    if (step == 0) {
      f.e_hard[p] = gr != 0.f ? 1 : 0;
      found_e += gr != 0.f ? 1 : 0;
    }
  }
  for (int idx = tid; idx < n * XD; idx += XT) {
    const int r = idx >> 6, k = idx & 63;
    if (k < F) {
      const size_t p = (size_t)(nbase + r) * F + k;
      const float s = x_sigmoid(f.n_logit[p]), ds = s * (1.f - s);
      float gr = L.t0[r * XS + k] * cm.x[p] * ds;
      if (reg && f.n_hard[p]) gr += (f.node_size * inv_n + f.node_ent * inv_n * x_dent(s)) * ds;
      float mi = f.n_m[p], vi = f.n_v[p];
      f.n_logit[p] = hcg_adam_update(f.n_logit[p], gr, mi, vi, f.b1, f.b2, f.eps, step_size, bc2_sqrt);
      f.n_m[p] = mi;
      f.n_v[p] = vi;
      if (step == 0) {
        f.n_hard[p] = gr != 0.f ? 1 : 0;
        found_n += gr != 0.f ? 1 : 0;
      }
    }
  }
  if (step == 0) {                                        // (integer counts: any order gives the same number)
    if (found_e) atomicAdd(&hc[0], found_e);
    if (found_n) atomicAdd(&hc[1], found_n);
    __syncthreads();
    if (tid < 2) f.hard_count[2 * g + tid] = hc[tid];
  }
  __syncthreads();
  }
  }  // epochs

  if constexpr (FIT) {
    // the post-processed masks: s(logit) of the hard entries, 0 elsewhere (each thread reads the logits it wrote)
    const XFit& f = args.f;
    for (int e = tid; e < ne; e += XT) {
      const size_t p = (size_t)ebase + e;
      f.edge_out[p] = f.e_hard[p] ? x_sigmoid(f.e_logit[p]) : 0.f;
    }
    for (int idx = tid; idx < n * XD; idx += XT) {
      const int r = idx >> 6, k = idx & 63;
      if (k < F) {
        const size_t p = (size_t)(nbase + r) * F + k;
        f.node_out[p] = f.n_hard[p] ? x_sigmoid(f.n_logit[p]) : 0.f;
      }
    }
  }
}

constexpr unsigned X_FIT_LDS_EXTRA = 16;

// hcg_explain, mode HCG_EXPLAIN_FIT, behind the shape check and the query
int x_fit_launch(hcg_explain_args* p, hipStream_t stream) {
  if (p->epoch_count < 1 || p->step_first < 0 || (long long)p->step_first + p->epoch_count >= (1ll << 31)) return HCG_ERR_INVALID_ARG;
  if (p->edge_mask || p->node_mask || p->dout || p->dx) return HCG_ERR_INVALID_ARG;
  if (p->B == 0) return HCG_OK;
  if (!x_common_ok(p) || !p->target || !p->fit_hard_count || !p->fit_loss_hist) return HCG_ERR_INVALID_ARG;
  if (p->E > 0 && (!p->fit_edge_logit || !p->fit_edge_exp_avg || !p->fit_edge_exp_avg_sq || !p->fit_edge_hard || !p->fit_edge_mask_out))
    return HCG_ERR_INVALID_ARG;
  if (p->N > 0 && (!p->fit_node_logit || !p->fit_node_exp_avg || !p->fit_node_exp_avg_sq || !p->fit_node_hard || !p->fit_node_mask_out))
    return HCG_ERR_INVALID_ARG;
  if (!p->workspace || p->workspace_bytes < p->workspace_bytes_needed) return HCG_ERR_WORKSPACE;

  XFitArgs k;
  XArgs& a = k.a;
  x_fill_common(a.c, p);
  a.edge_mask = a.node_mask = a.dout = nullptr;
  const bool cls = (p->flags & HCG_EXPLAIN_TARGET_CLASS) != 0;        // which of the slot's two readings
  a.target = cls ? nullptr : p->target;
  a.target_class = cls ? p->target_class : nullptr;
  a.out = p->out;
  a.loss = a.d_edge_mask = a.d_node_mask = a.dx = nullptr;
  a.ws = (float*)p->workspace;
  a.N = (int)p->N;
  a.sigmoid = 1;
  XFit& f = k.f;
  f.e_logit = p->fit_edge_logit; f.e_m = p->fit_edge_exp_avg; f.e_v = p->fit_edge_exp_avg_sq; f.e_hard = p->fit_edge_hard;
  f.n_logit = p->fit_node_logit; f.n_m = p->fit_node_exp_avg; f.n_v = p->fit_node_exp_avg_sq; f.n_hard = p->fit_node_hard;
  f.hard_count = p->fit_hard_count;
  f.loss_hist = p->fit_loss_hist;
  f.edge_out = p->fit_edge_mask_out;
  f.node_out = p->fit_node_mask_out;
  f.step_first = p->step_first;
  f.epochs = p->epoch_count;
  f.B = (int)p->B;
  f.lr = p->fit_lr; f.b1 = p->fit_beta1; f.b2 = p->fit_beta2; f.eps = p->fit_eps;
  f.edge_size = p->fit_coeffs[0]; f.edge_ent = p->fit_coeffs[1]; f.node_size = p->fit_coeffs[2]; f.node_ent = p->fit_coeffs[3];
  return x_launch<k_explain_graphs<true>>(dim3((unsigned)p->B), x_lds_bytes(a.c.npad, a.c.emax) + X_FIT_LDS_EXTRA, stream, k);
}

// the model axis of HCG_EXPLAIN_INTEGRATED: n_models, 0 (what a caller of the one-model form leaves there) meaning 1
inline int x_path_models(const hcg_explain_args* p) { return p->n_models == 0 ? 1 : p->n_models; }

// hcg_explain, mode HCG_EXPLAIN_INTEGRATED, behind the shape check, the flag / NULL checks, the model count and the query
int x_path_launch(hcg_explain_args* p, hipStream_t stream) {
  if (p->path_steps < 1 || p->path_step_first < 0 || p->path_step_count < 0 ||
      (long long)p->path_step_first + p->path_step_count > p->path_steps)
    return HCG_ERR_INVALID_ARG;
  if (p->path_class_index < 0 || p->path_class_index >= p->C) return HCG_ERR_INVALID_ARG;
  if (p->B == 0 || p->path_step_count == 0) return HCG_OK;
  if (!p->path_out_full || !p->path_out_base || !p->path_alpha || !p->path_weight) return HCG_ERR_INVALID_ARG;
  if (!p->graph_ptr || !p->edge_ptr || !p->status || (p->N > 0 && !p->x) || (p->E > 0 && !p->edge_index)) return HCG_ERR_INVALID_ARG;
  for (int l = 0; l < p->n_conv; ++l)
    if (!p->conv_W[l] || !p->conv_b[l]) return HCG_ERR_INVALID_ARG;
  for (int i = 0; i < p->R; ++i)
    if (!p->head_W[i] || !p->head_b[i]) return HCG_ERR_INVALID_ARG;
  if ((p->E > 0 && !p->path_edge_attr) || (p->N > 0 && !p->path_node_attr)) return HCG_ERR_INVALID_ARG;
  if (!p->workspace || p->workspace_bytes < p->workspace_bytes_needed) return HCG_ERR_WORKSPACE;

  XPathArgs k;
  XArgs& a = k.a;
  x_fill_common(a.c, p);
  a.edge_mask = a.node_mask = a.target = a.dout = nullptr;
  a.target_class = nullptr;
  a.out = p->path_out_full;
  a.loss = a.d_edge_mask = a.d_node_mask = a.dx = nullptr;
  a.ws = (float*)p->workspace;
  a.N = (int)p->N;
  a.sigmoid = 0;
  XPath& f = k.f;
  f.alpha = p->path_alpha;
  f.weight = p->path_weight;
  f.node_attr = p->path_node_attr;
  f.edge_attr = p->path_edge_attr;
  f.out_base = p->path_out_base;
  f.step_first = p->path_step_first;
  f.steps = p->path_step_count;
  f.cls = p->path_class_index;
  f.B = (int)p->B;
  const int M = x_path_models(p);                         // (checked by the caller: 1 .. 65535)
  f.ws_model = p->workspace_bytes_needed / (size_t)M / sizeof(float);
  return x_launch<k_explain_graphs<false, true>>(dim3((unsigned)p->B, (unsigned)M), x_lds_bytes(a.c.npad, a.c.emax), stream, k);
}

// ---- HCG_EXPLAIN_MOMENTS: running mean / sum of squared deviations over a model axis ---------------------------------------
// One thread per entry of the (up to two) [count][len] arrays of a call walks the models in ascending order: Welford's
// recurrence in float32, never contracted, k = the 1-based count over the WHOLE ensemble.  The state lives in the caller's
// arrays and each entry has one owner, so the moments are bitwise independent of how the models are split into calls.
// Consecutive threads read consecutive floats of a model's row.
constexpr int XM_T = 256;

struct XMom {
  const float* v0; const float* v1;     // [count][len0], [count][len1]
  float* mean0; float* mean1;
  float* m20; float* m21;
  float* sd0; float* sd1;
  long long len0, len1;
  int total, first, count;
};

__global__ __launch_bounds__(XM_T) void k_model_moments(const XMom a) {
#pragma clang fp contract(off)
  long long i = (long long)blockIdx.x * XM_T + threadIdx.x;
  const bool second = i >= a.len0;
  if (second) i -= a.len0;
  const long long len = second ? a.len1 : a.len0;
  if (i >= len) return;
  const float* v = (second ? a.v1 : a.v0) + i;
  float* const mean_p = (second ? a.mean1 : a.mean0) + i;
  float* const m2_p = (second ? a.m21 : a.m20) + i;
  float mean = 0.f, m2 = 0.f;                             // the call that starts at model 0 starts from 0
  if (a.first > 0) { mean = *mean_p; m2 = *m2_p; }
  for (int j = 0; j < a.count; ++j) {
    const float x = v[(size_t)j * (size_t)len];
    const float k = (float)(a.first + j + 1);
    const float d = x - mean;
    mean += d / k;
    m2 += d * (x - mean);
  }
  *mean_p = mean;
  *m2_p = m2;
  if (a.first + a.count == a.total) (second ? a.sd1 : a.sd0)[i] = sqrtf(m2 / (float)a.total);
}

int x_moments_launch(hcg_explain_args* p, hipStream_t stream) {
  if (p->mom_total < 1 || p->mom_first < 0 || p->mom_count < 0 || (long long)p->mom_first + p->mom_count > p->mom_total)
    return HCG_ERR_INVALID_ARG;
  long long blocks = 0;
  for (int s = 0; s < 2; ++s) {
    if (p->mom_len[s] < 0 || p->mom_len[s] >= (1ll << 31)) return HCG_ERR_INVALID_ARG;
    blocks += p->mom_len[s];
  }
  blocks = hcg_cdiv(blocks, (long long)XM_T);
  p->workspace_bytes_needed = 0;
  if (p->flags & HCG_EXPLAIN_QUERY) return HCG_OK;
  if (p->mom_count == 0 || blocks == 0) return HCG_OK;
  for (int s = 0; s < 2; ++s)
    if (p->mom_len[s] > 0 && (!p->mom_values[s] || !p->mom_mean[s] || !p->mom_m2[s] || !p->mom_std[s])) return HCG_ERR_INVALID_ARG;
  XMom a;
  a.v0 = p->mom_values[0]; a.v1 = p->mom_values[1];
  a.mean0 = p->mom_mean[0]; a.mean1 = p->mom_mean[1];
  a.m20 = p->mom_m2[0]; a.m21 = p->mom_m2[1];
  a.sd0 = p->mom_std[0]; a.sd1 = p->mom_std[1];
  a.len0 = p->mom_len[0]; a.len1 = p->mom_len[1];
  a.total = p->mom_total; a.first = p->mom_first; a.count = p->mom_count;
  hipLaunchKernelGGL(k_model_moments, dim3((unsigned)blocks), dim3(XM_T), 0, stream, a);
  HCG_CHECK_LAUNCH();
  return HCG_OK;
}

}  // namespace

extern "C" int hcg_explain(hcg_explain_args* p, hcg_stream_t stream_) {
  if (!p) return HCG_ERR_INVALID_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  // the class-index form of the upstream gradient belongs to HCG_EXPLAIN_GRAPHS and HCG_EXPLAIN_FIT alone
  if ((p->flags & HCG_EXPLAIN_TARGET_CLASS) && (p->mode == HCG_EXPLAIN_LAYER_EDGE_GRAD || p->mode == HCG_EXPLAIN_ENSEMBLE ||
                                                p->mode == HCG_EXPLAIN_SHAPLEY || p->mode == HCG_EXPLAIN_INTEGRATED ||
                                                p->mode == HCG_EXPLAIN_MOMENTS || p->mode == HCG_EXPLAIN_COALITIONS ||
                                                p->mode == HCG_EXPLAIN_SUBSETS || p->mode == HCG_EXPLAIN_GREEDY))
    return HCG_ERR_INVALID_ARG;
  // groups of features as players belong to HCG_EXPLAIN_SHAPLEY alone
  if ((p->flags & HCG_EXPLAIN_GROUPED) && p->mode != HCG_EXPLAIN_SHAPLEY) return HCG_ERR_INVALID_ARG;
  if (p->mode == HCG_EXPLAIN_LAYER_EDGE_GRAD) {
    if (p->flags & HCG_EXPLAIN_QUERY) { p->workspace_bytes_needed = 0; return HCG_OK; }
    return hcg_edge_weight_grad_launch(p->layer_dout, p->layer_out, p->layer_h, p->rowptr, p->col, p->dinv, p->slope,
                                       p->apply_act, p->dew_csr, p->N, p->E, p->D, stream);
  }
  if (p->mode == HCG_EXPLAIN_ENSEMBLE) return hcg_ensemble_launch(p, stream);
  if (p->mode == HCG_EXPLAIN_SHAPLEY) return hcg_shapley_launch(p, stream);
  if (p->mode == HCG_EXPLAIN_COALITIONS) return hcg_coalitions_launch(p, stream);
  if (p->mode == HCG_EXPLAIN_SUBSETS) return hcg_subsets_launch(p, stream);
  if (p->mode == HCG_EXPLAIN_GREEDY) return hcg_greedy_launch(p, stream);
  if (p->mode == HCG_EXPLAIN_MOMENTS) return x_moments_launch(p, stream);
  const bool fit = p->mode == HCG_EXPLAIN_FIT;
  const bool path = p->mode == HCG_EXPLAIN_INTEGRATED;
  if (p->mode != HCG_EXPLAIN_GRAPHS && !fit && !path) return HCG_ERR_INVALID_ARG;
  if (!x_shapes_ok(p)) return HCG_ERR_UNSUPPORTED;
  // (PATH: the masks and the upstream gradient are the algorithm's own)
  if (path && ((p->flags & HCG_EXPLAIN_SIGMOID) || p->target || p->dout || p->edge_mask || p->node_mask || p->dx)) return HCG_ERR_INVALID_ARG;
  const bool cls = (p->flags & HCG_EXPLAIN_TARGET_CLASS) != 0;
  if (cls && p->C < 2) return HCG_ERR_UNSUPPORTED;          // a cross-entropy needs two classes or more
  // (FIT: the tiles and lists of HCG_EXPLAIN_GRAPHS and two hard counts behind them)
  if (fit) p->lds_bytes = (int32_t)(x_lds_bytes(x_round4(p->max_nodes, 4), x_round4(p->max_edges, 4)) + X_FIT_LDS_EXTRA);
  if (path) p->lds_bytes = (int32_t)x_lds_bytes(x_round4(p->max_nodes, 4), x_round4(p->max_edges, 4));
  // H_l and A_l of every layer, [N][64] f32 each: the backward reads them again
  p->workspace_bytes_needed = hcg_align_up((size_t)2 * p->n_conv * (size_t)(p->N > 0 ? p->N : 1) * XD * sizeof(float), 256);
  if (path) {
    // one workspace slice per model of the launch (grid y)
    const int M = x_path_models(p);
    if (M < 1 || M > 65535) return HCG_ERR_INVALID_ARG;
    p->workspace_bytes_needed *= (size_t)M;
  }
  if (p->flags & HCG_EXPLAIN_QUERY) return HCG_OK;
  if (fit) return x_fit_launch(p, stream);
  if (path) return x_path_launch(p, stream);
  if (p->B == 0) return HCG_OK;
  const bool bwd = p->target || p->dout;                       // (target: the slot in either reading)
  if ((p->target && p->dout) || (cls && !p->target_class)) return HCG_ERR_INVALID_ARG;
  if (!x_common_ok(p) || (p->E > 0 && !p->edge_mask)) return HCG_ERR_INVALID_ARG;
  if (bwd && ((p->E > 0 && !p->d_edge_mask) || (p->node_mask && !p->d_node_mask) || (p->target && !p->loss))) return HCG_ERR_INVALID_ARG;
  if (!p->node_mask && p->d_node_mask) return HCG_ERR_INVALID_ARG;
  if (bwd && (!p->workspace || p->workspace_bytes < p->workspace_bytes_needed)) return HCG_ERR_WORKSPACE;

  XArgs a;
  x_fill_common(a.c, p);
  a.edge_mask = p->edge_mask;
  a.node_mask = p->node_mask;
  a.target = cls ? nullptr : p->target;
  a.dout = p->dout;
  a.target_class = cls ? p->target_class : nullptr;
  a.out = p->out;
  a.loss = p->loss;
  a.d_edge_mask = p->d_edge_mask;
  a.d_node_mask = bwd ? p->d_node_mask : nullptr;
  a.dx = bwd ? p->dx : nullptr;
  a.ws = (float*)p->workspace;
  a.N = (int)p->N;
  a.sigmoid = (p->flags & HCG_EXPLAIN_SIGMOID) ? 1 : 0;
  return x_launch<k_explain_graphs<false>>(dim3((unsigned)p->B), x_lds_bytes(a.c.npad, a.c.emax), stream, a);
}
