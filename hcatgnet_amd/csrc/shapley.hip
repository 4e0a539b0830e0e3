// Shapley value sampling (Captum's ShapleyValueSampling with baselines 0 and one feature per step, as the reference uses it
// through torch_geometric.explain.Explainer on GCN_explain: scripts_experiments/explain_gnn.py) for a BATCH of graphs.
//
// The features of a graph are its n F node-feature entries and its e directed edges (the header states the indexing).  One
// permutation of them costs one masked forward per feature; the graph and the model are the same for all of them.  So the grid
// runs over (graph, permutation): one workgroup of 8 waves builds its graph once, keeps it in LDS and walks its permutation on
// chip -- switch a feature on, evaluate, record the difference -- with no launch and no HBM round trip between evaluations.
// Workgroups never depend on each other, nothing is reduced across them, no float atomics: every sum has one owner and a fixed
// order, so the differences of (graph, permutation) are bitwise the same run to run and whatever else shares the launch.
// Per workgroup:
//   build     once: gcn_norm on chip from the raw COO edges (rules: graph_csr.h) -- in-degree, dinv from the UNMASKED
//             in-degree, the by-destination entry list ((source << 16) | local edge, rows sorted).  Forward only: no
//             by-source list, no workspace of activations.  mval[e] = 0 (off) for an edge with an entry, -1 for one without
//             (an explicit (i, i) edge is part of the unit self loop; an ungrouped edge is ignored): switching such an edge on
//             changes nothing.
//   state     h1 = x~ W1^T [n][64], starting at 0 (everything off).  A node entry (i, f) switched on is the rank-1 update
//             h1[i, :] += x[i, f] W1[:, f] (64 FMAs by one wave); an edge switched on sets mval[e] = 1 and touches no row of
//             h1.  Layer 1's GEMM is therefore never recomputed.
//   evaluate  A1 = leaky(dinv_i (dinv_i h1_i + sum_k m_k dinv_c h1_c) + b1) (h1 -> t0);  per further layer  H = A_prev W^T
//             (t0 -> t1: explain_tile.h x_gemm, the lane's weight row in 64 registers) and the same aggregation (t1 -> t0);
//             [max, mean] pooling;  readout of depth R;  v = out[class_index].
//   walk      the permutation is read a chunk of 256 steps at a time: every thread classifies one step -- a node entry whose x
//             is exactly 0, an edge without an entry or an index outside the graph cannot change the output, its difference
//             (exactly 0) is written at once and no evaluation is spent on it -- the others go through LDS to the serial walk.
// Build, aggregation and pooling are explain_tile.h's, shared with explain.hip and ensemble.hip; the readout loop is this
// file's own (explain_tile.h's header says why).
// What is the same for every evaluation of a workgroup stays in registers where it fits: the second conv layer's weight row
// (models of two conv layers, the reference's: 64 registers; deeper stacks reload the row per layer from L2) and the first
// readout layer's weights (16 registers per thread).
// LDS holds three [npad][64 + 4] f32 tiles (h1, t0, t1; the pooling partials alias t1), the entry list and mask values and
// ~5 KB of structure, sized at launch from the batch's largest graph: 160 KB less 208 bytes at this mode's limit of 184 nodes
// and 1024 directed edges (the reference's largest graph has 184 atoms).
// The differences go to the caller's workspace, one row per permutation of the launch; k_shapley_reduce then adds the rows onto
// the accumulator, p ascending, continuing from what earlier launches left: the mean over all permutations is one fixed-order
// sum however the permutations are split into launches.
// HCG_EXPLAIN_GROUPED (k_shapley_walk<true>): the players are groups of features -- an atom, a bond, a fragment (Captum's
// feature_mask) -- and a background is always on.  The walk is the same: "apply the step to the state" becomes "apply every
// live member of the group" (s_apply: the host lists them, ascending, in global memory), "evaluate" stays one evaluation, and
// the base evaluation follows the background's application.  The chunk classification reads one group id per thread; an empty
// member range is a group that cannot change the output (0 at once, no evaluation); pj / pv carry the queued group ids and
// their first member positions.  Permutation rows, workspace rows and the accumulator have one entry per group.  No LDS is
// added: the members are staged through t1, which is idle between two evaluations.
// HCG_EXPLAIN_COALITIONS (k_coalition_values, below the walk): every subset of a graph's live groups evaluated once, the state
// rebuilt from zero per subset.  Build (s_build), weights in registers (s_load_weights), application (s_apply) and evaluation
// (s_eval) are the walk's: both kernels call the same four functions.
// HCG_EXPLAIN_SUBSETS (k_subset_values, below the coalition kernel): a caller's LIST of subsets of a graph's groups, any number
// of groups, evaluated the same way -- but the set groups are applied in ONE filtered pass over the graph's member list
// (s_apply_subset), the row's bit words staged in pj / pv, where the coalition kernel pays one s_apply per set group.
// HCG_EXPLAIN_GREEDY (k_greedy_round, below the subset kernel): one round of the greedy insertion / deletion order per launch,
// the previous round's winner picked on chip by every workgroup of the graph, the candidates evaluated as k_subset_values rows.
// A model axis (k_shapley_walk, both instantiations, and k_subset_values): n_models = M frozen models of one architecture,
// weights stacked [M, ...], one more grid axis -- walk dim3(B, perm_count, M), subsets dim3(jobs, M).  The model index is
// uniform: s_model shifts the weight pointers of a LOCAL XCommon by m times the layer's size once, at the top of the kernel,
// and s_apply*, s_load_weights and s_eval run on it unchanged.  Every output takes a leading model axis (out / out_base
// [M][B][C], workspace [M][count][row], shap_acc [M][row], table [M][S][B][C]); with M = 1 every offset is zero.  The
// coalition and the greedy kernel take one model (n_models > 1: HCG_ERR_UNSUPPORTED); a loop over a group of models INSIDE
// a workgroup, which would build the graph once per group as ensemble.hip does, is not done.
#include "common.h"
#include "graph_csr.h"
#include "explain_tile.h"

namespace {

constexpr int S_MAX_NODES = 184;
constexpr int S_CHUNK = 256;           // walk steps classified at a time
constexpr int S_NPAD_MIN = 16;         // (the pooling partials, XW * 128 floats, alias t1)

struct SArgs {     // the kernel's argument block (device pointers by value)
  XCommon c;
  const int32_t* perm;                      // [P][row]
  float* out;                               // [B][C] everything on
  float* out_base;                          // [B][C] everything off
  float* ws;                                // [count][row] the differences of this launch's permutations
  long long NF, Etot, row;                  // N F, E, N F + E (GROUPED: row = G, the groups of the batch)
  int first, cls;
};

struct SGArgs : SArgs {   // what HCG_EXPLAIN_GROUPED adds (GROUPED = true only): perm is [P][G], ws [count][G]
  const int32_t* group_ptr;                 // [B + 1] graph g's groups: group_ptr[g] .. group_ptr[g + 1] - 1 of a row
  const int32_t* member_ptr;                // [G + 1] into `members`
  const int32_t* members;                   // live members, local feature indices, ascending within a group
  const int32_t* bg_ptr;                    // [B + 1] into `bg_members`
  const int32_t* bg_members;                // the live background of every graph, ascending
};

struct SLds {
  float* h1;            // [npad][XS]  x~ W1^T of the features switched on so far
  float* t0;            // [npad][XS]
  float* t1;            // [npad][XS]  (pooling partials: its first XW * 128 floats)
  unsigned* ent;        // [emax]  by destination: (source << 16) | local edge
  float* mval;          // [emax]  1 on, 0 off, -1 no entry
  int* rowptr;          // [npad + 4]
  int* cnt;             // [npad]  in-degree, then the fill cursor
  float* dinv;          // [npad]
  float* hv;            // [X_HEAD] readout activations: emb | v1 | v2 | ... | out
  int* pj;              // [S_CHUNK] the chunk's steps: local feature index (GROUPED: local group id), -1 = nothing to evaluate
  float* pv;            // [S_CHUNK] the x value of a node entry (GROUPED: the bits of the group's first position in `members`)
};

__host__ __device__ inline unsigned s_lds_bytes(int npad, int emax) {
  return 3u * npad * XS * 4 + 2u * emax * 4 + (unsigned)(npad + 4) * 4 + 2u * npad * 4 + X_HEAD * 4 + 2 * S_CHUNK * 4;
}

// (integer offsets, as mid.hip's carve: the arrays must stay LDS pointers for the compiler)
__device__ __forceinline__ SLds s_carve(char* base, int npad, int emax) {
  SLds L;
  unsigned off = 0;
  L.h1 = reinterpret_cast<float*>(base + off); off += (unsigned)npad * XS * 4;
  L.t0 = reinterpret_cast<float*>(base + off); off += (unsigned)npad * XS * 4;
  L.t1 = reinterpret_cast<float*>(base + off); off += (unsigned)npad * XS * 4;
  L.ent = reinterpret_cast<unsigned*>(base + off); off += (unsigned)emax * 4;
  L.mval = reinterpret_cast<float*>(base + off); off += (unsigned)emax * 4;
  L.rowptr = reinterpret_cast<int*>(base + off); off += (unsigned)(npad + 4) * 4;
  L.cnt = reinterpret_cast<int*>(base + off); off += (unsigned)npad * 4;
  L.dinv = reinterpret_cast<float*>(base + off); off += (unsigned)npad * 4;
  L.hv = reinterpret_cast<float*>(base + off); off += X_HEAD * 4;
  L.pj = reinterpret_cast<int*>(base + off); off += S_CHUNK * 4;
  L.pv = reinterpret_cast<float*>(base + off);
  return L;
}

__device__ __forceinline__ float s_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// The launch's XCommon with the weight pointers of model m (uniform) of weights stacked [M, ...]: layer sizes 64 F, then
// 64 * 64 (conv), 64 (conv bias), out_i in_i and out_i (readout; in_i = 128 >> i, out_i = C on the last layer).  m = 0
// changes nothing.  A layer the model does not have keeps a pointer nobody reads.
__device__ __forceinline__ XCommon s_model(const XCommon& c, unsigned m) {
  XCommon r = c;
  const size_t mm = m;
#pragma unroll
  for (int l = 0; l < HCG_EXPLAIN_MAX_CONVS; ++l) {
    r.cW[l] = c.cW[l] + mm * (size_t)(XD * (l == 0 ? c.F : XD));
    r.cb[l] = c.cb[l] + mm * XD;
  }
#pragma unroll
  for (int i = 0; i < HCG_HEAD_MAX_LAYERS; ++i) {
    const int in_i = (2 * XD) >> i, out_i = i == c.R - 1 ? c.C : in_i / 2;
    r.hW[i] = c.hW[i] + mm * (size_t)(out_i * in_i);
    r.hb[i] = c.hb[i] + mm * (size_t)out_i;
  }
  return r;
}

// GROUPED: switch the members mem[mb .. me) on (mb, me uniform; all 8 waves).  XT members at a time are staged in t1 (free
// between two evaluations): the thread that loads a member stores an edge's mval = 1 itself and leaves a node entry as
// (node << 6 | f, x) for the node's owner -- wave (node mod 8) -- which applies its entries in list order with the ungrouped
// walk's rank-1 update.  So every element of h1 has one owner and takes its updates in ascending member order, whatever the
// group's size.  An index outside [0, K) is skipped.  The caller places the barrier between this and the evaluation.
// `on(position in mem)` filters the list (s_apply: everything; s_apply_subset: the members of the row's groups): a member that
// is off is staged as nothing (code -1), which skips without reordering.
template <class On>
__device__ __forceinline__ void s_apply_if(const SLds& L, const XCommon& cm, const int32_t* mem, int mb, int me, int nbase, int nF,
                                           int K, int tid, On on) {
  const int lane = tid & 63, wave = tid >> 6, F = cm.F;
  int* const code = reinterpret_cast<int*>(L.t1);        // [XT]
  float* const val = L.t1 + XT;                          // [XT]  (npad >= 16: the tile has 16 * XS >= 2 XT floats)
#pragma nounroll
  for (int c0 = mb; c0 < me; c0 += XT) {
    if (c0 != mb) __syncthreads();                       // (the members staged before have been applied)
    int cd = -1;
    float xv = 0.f;
    if (tid < me - c0 && on(c0 + tid)) {
      const int jj = mem[c0 + tid];
      if (jj >= 0 && jj < nF) {
        const int i = jj / F;
        cd = (i << 6) | (jj - i * F);
        xv = cm.x[(size_t)nbase * F + jj];
      } else if (jj >= nF && jj < K) {
        L.mval[jj - nF] = 1.f;
      }
    }
    code[tid] = cd;
    val[tid] = xv;
    __syncthreads();
    const int cnt = min(XT, me - c0);
#pragma nounroll
    for (int s = 0; s < cnt; s += 64) {
      const int cdl = code[s + lane];
      const float xl = val[s + lane];
      unsigned long long mine = __ballot(cdl >= 0 && ((cdl >> 6) & (XW - 1)) == wave);
#pragma nounroll
      while (mine) {
        const int b = __builtin_ctzll(mine);
        mine &= mine - 1;
        const int cu = __builtin_amdgcn_readlane(cdl, b);
        const float xs = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xl), b));
        const int i = cu >> 6, f = cu & 63;
        L.h1[i * XS + lane] = fmaf(xs, cm.cW[0][lane * F + f], L.h1[i * XS + lane]);
      }
    }
  }
}

__device__ __forceinline__ void s_apply(const SLds& L, const XCommon& cm, const int32_t* mem, int mb, int me, int nbase, int nF,
                                        int K, int tid) {
  s_apply_if(L, cm, mem, mb, me, nbase, nF, K, tid, [](int) { return true; });
}

// HCG_EXPLAIN_SUBSETS: the members mem[mb .. me) -- ALL groups of the graph, group by group -- whose group is set in the row's
// bit words `bits` (LDS, staged by the caller behind a barrier), in one pass.  grp[p] is the local group id of mem[p]; an id
// outside [0, ng) is off.  The list is ordered by group, then by local index, and an off member is skipped in place, so every
// element of h1 takes the updates it takes when the set groups are applied one s_apply each, in the same order.
__device__ __forceinline__ void s_apply_subset(const SLds& L, const XCommon& cm, const int32_t* mem, const int32_t* grp,
                                               const unsigned* bits, int ng, int mb, int me, int nbase, int nF, int K, int tid) {
  s_apply_if(L, cm, mem, mb, me, nbase, nF, K, tid, [&](int p) {
    const int y = grp[p];
    return y >= 0 && y < ng && ((bits[y >> 5] >> (y & 31)) & 1u) != 0;
  });
}

// One evaluation of the state in LDS (h1, mval): conv stack, pooling, readout -> the position of the output row in hv.  `w` is
// the lane's weight row of conv layer 2 (models of two conv layers: loaded once by the caller; deeper stacks reload it here),
// rw0 the thread's 16 weights of readout layer 0 (W[ro][rsub + 8 k], zero for a thread without an output).  Opens on the
// caller's barrier behind the last change of the state, ends behind a barrier; k_shapley_walk and k_coalition_values both
// evaluate through this and nothing else.
__device__ __forceinline__ int s_eval(const SLds& L, const XCommon& cm, const XMasked fmt, float (&w)[XD], const float (&rw0)[16],
                                      int n, int tid) {
  const int lane = tid & 63, wave = tid >> 6, ro = tid >> 3, rsub = tid & 7;
  const int C = cm.C, R = cm.R, n_conv = cm.n_conv;
#pragma nounroll
  for (int l = 0; l < n_conv; ++l) {
    if (l > 0) {
      if (n_conv > 2) x_weight_row(w, reinterpret_cast<const char*>(x_pick(cm.cW, l)), lane, XD);
      x_gemm(L.t0, w, n, wave, [&](int r, float v) { L.t1[r * XS + lane] = v; });
      __syncthreads();
    }
    x_conv_out(l == 0 ? L.h1 : L.t1, L.t0, L.ent, L.rowptr, fmt, L.dinv, x_pick(cm.cb, l), n, tid, cm.slope,
               [](int, int, float4) {});
    __syncthreads();
  }
  // pooling (t0 = A of the last layer; the partials alias t1), readout
  x_pool(L.t0, L.t1, L.hv, n, tid);
  int off = 0;
  for (int i = 0; i < R; ++i) {
    const int in_i = (2 * XD) >> i, out_i = i == R - 1 ? C : in_i / 2;
    float p = 0.f;
    if (i == 0) {
#pragma unroll
      for (int k = 0; k < 16; ++k) p = fmaf(rw0[k], L.hv[rsub + 8 * k], p);
    } else if (ro < out_i) {
      const float* W = x_pick(cm.hW, i) + (size_t)ro * in_i;
      for (int k = rsub; k < in_i; k += 8) p = fmaf(W[k], L.hv[off + k], p);
    }
    p += __shfl_xor(p, 1, 8);
    p += __shfl_xor(p, 2, 8);
    p += __shfl_xor(p, 4, 8);
    if (ro < out_i && rsub == 0) {
      const float y = p + x_pick(cm.hb, i)[ro];
      L.hv[off + in_i + ro] = i == R - 1 ? y : hcg_leaky(y, cm.slope);
    }
    off += in_i;
    __syncthreads();
  }
  return off;
}

// The weights every evaluation of a workgroup reuses, loaded once: the lane's row of conv layer 2 (two conv layers) and the
// thread's share of readout layer 0.
__device__ __forceinline__ void s_load_weights(float (&w)[XD], float (&rw0)[16], const XCommon& cm, int tid) {
  const int lane = tid & 63, ro = tid >> 3, rsub = tid & 7;
  if (cm.n_conv == 2) x_weight_row(w, reinterpret_cast<const char*>(cm.cW[1]), lane, XD);
  const int out0 = cm.R == 1 ? cm.C : XD;
  const float* W = cm.hW[0] + (size_t)(ro < out0 ? ro : 0) * (2 * XD) + rsub;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const float v = W[8 * k];
    rw0[k] = ro < out0 ? v : 0.f;
  }
}

// The graph, once per workgroup (both kernels): the by-destination entry list, dinv, h1 = 0 and mval = 0 for an edge with an
// entry, -1 for one without.  Ends behind a barrier.
__device__ __forceinline__ void s_build(const SLds& L, const XCommon& cm, const XSpan& sp, int tid) {
  const int n = sp.n, ne = sp.ne;
  EdgeRegs<X_EPT, XT> er;
  er.load(XGraph{sp.ebase, sp.ne}, cm.ei, cm.E, tid);
  for (int i = tid; i < cm.npad; i += XT) L.cnt[i] = 0;
  for (int idx = tid; idx < n * XD; idx += XT) L.h1[(idx >> 6) * XS + (idx & 63)] = 0.f;       // everything off
  XEdges q;
  x_edge_pass(q, er, sp, tid, cm.status);
  x_build_rows<XMasked, false>(q, {L.ent, L.rowptr, L.cnt}, {}, L.dinv, n, tid);
#pragma unroll
  for (int j = 0; j < X_EPT; ++j)
    if (tid + j * XT < ne) L.mval[tid + j * XT] = q.live[j] ? 0.f : -1.f;
  __syncthreads();
}

// Everything off: h1 = 0 and mval = 0 for every edge with an entry.  Opens behind a barrier (the evaluation before is done: h1,
// mval and t1 are idle), ends behind one.
__device__ __forceinline__ void s_reset(const SLds& L, int n, int ne, int tid) {
  for (int idx = tid; idx < n * XD; idx += XT) L.h1[(idx >> 6) * XS + (idx & 63)] = 0.f;
#pragma unroll
  for (int j = 0; j < X_EPT; ++j)
    if (tid + j * XT < ne && L.mval[tid + j * XT] > 0.f) L.mval[tid + j * XT] = 0.f;
  __syncthreads();
}

// One row of k_subset_values, which k_greedy_round evaluates its candidates with: everything off, the live background
// bgm[bb .. be), the members mem[mb .. me) whose group is set in `bits` in one filtered pass, one evaluation -> the position of
// the output row in hv.  Opens behind a barrier (or on `bits` written by the thread that reads them: s_reset's barrier stands
// before the filtered pass), ends behind one.
__device__ __forceinline__ int s_row_subset(const SLds& L, const XCommon& cm, const XMasked fmt, float (&w)[XD], const float (&rw0)[16],
                                            const int32_t* bgm, int bb, int be, const int32_t* mem, const int32_t* grp,
                                            const unsigned* bits, int ng, int mb, int me, int nbase, int n, int ne, int tid) {
  const int nF = n * cm.F, K = nF + ne;
  s_reset(L, n, ne, tid);
  s_apply(L, cm, bgm, bb, be, nbase, nF, K, tid);
  __syncthreads();                                         // (the staging of the list before has been read)
  s_apply_subset(L, cm, mem, grp, bits, ng, mb, me, nbase, nF, K, tid);
  __syncthreads();
  return s_eval(L, cm, fmt, w, rw0, n, tid);
}

// The job of a workgroup of the three job kernels, a triple of a.jobs, and its graph's groups; all uniform.
struct SJob {
  int g, first, count;                      // the graph, the first mask / row / id of the run, their number
  int gp, ng;                               // the graph's first group and its number of groups
};

// false: the triple or the graph's group range is outside the arrays (at most `max_groups` groups) -- nothing to do
template <class Args>
__device__ __forceinline__ bool s_job(SJob& j, const Args& a, int max_groups) {
  const int32_t* const job = a.jobs + 3 * ((size_t)a.first + blockIdx.x);
  j.g = __builtin_amdgcn_readfirstlane(job[0]);
  j.first = __builtin_amdgcn_readfirstlane(job[1]);
  j.count = __builtin_amdgcn_readfirstlane(job[2]);
  if (j.g < 0 || j.g >= a.B) return false;
  j.gp = __builtin_amdgcn_readfirstlane(a.group_ptr[j.g]);
  j.ng = __builtin_amdgcn_readfirstlane(a.group_ptr[j.g + 1]) - j.gp;
  return !(j.ng < 0 || j.ng > max_groups || j.gp < 0 || (long long)j.gp + j.ng > a.G);
}

// GROUPED = false: one feature per step (Args = SArgs).  GROUPED = true: HCG_EXPLAIN_GROUPED (Args = SGArgs) -- the players are
// the graph's groups, a step switches on every live member of one group and is evaluated once, and the live background is on
// from the base evaluation on.  The ungrouped instantiation is the kernel as it was before the template.
template <bool GROUPED, class Args>
__global__ __launch_bounds__(XT) void k_shapley_walk(const Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const XCommon cm = s_model(a.c, blockIdx.z);             // grid z: the model
  const SLds L = s_carve(smem, cm.npad, cm.emax);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x;
  const int F = cm.F, C = cm.C;
  const bool p0 = a.first + (int)blockIdx.y == 0;          // permutation 0 of the whole call writes out / out_base
  // the model's slices: ws [M][count][row], out / out_base [M][B][C]
  float* const wsrow = a.ws + ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * (size_t)a.row;
  float* const out = a.out + (size_t)blockIdx.z * gridDim.x * C;
  float* const out_base = a.out_base + (size_t)blockIdx.z * gridDim.x * C;

  XSpan sp;
  if (x_refused(sp, cm, g, tid)) {
    // the graph's rows are zero -- over whatever part of its ranges lies inside the arrays
    const int nbase = sp.nbase, ebase = sp.ebase, n_raw = sp.n_raw, ne_raw = sp.ne_raw;
    if (p0)
      for (int k = tid; k < C; k += XT) { out[(size_t)g * C + k] = 0.f; out_base[(size_t)g * C + k] = 0.f; }
    if constexpr (GROUPED) {
      const long long ge = a.group_ptr[g + 1];
      for (long long k = (long long)a.group_ptr[g] + tid; k < ge; k += XT)
        if (k >= 0 && k < a.row) wsrow[k] = 0.f;
      return;
    }
    for (long long e = tid; e < ne_raw; e += XT) {
      const long long p = (long long)ebase + e;
      if (p >= 0 && p < a.Etot) wsrow[a.NF + p] = 0.f;
    }
    for (long long i = tid; i < (long long)n_raw * F; i += XT) {
      const long long p = (long long)nbase * F + i;
      if (p >= 0 && p < a.NF) wsrow[p] = 0.f;
    }
    return;
  }

  // ---------------------------------------------------------------------------------------------- build (once per workgroup)
  const int nbase = sp.nbase, ebase = sp.ebase, n = sp.n, ne = sp.ne;
  s_build(L, cm, sp, tid);
  const XMasked fmt{L.mval};

  // ---------------------------------------------------------------------------------------------- what every evaluation reuses
  float w[XD];                                            // the lane's weight row of a conv layer >= 2
  float rw0[16];                                          // readout layer 0: W[ro][rsub + 8 k]
  s_load_weights(w, rw0, cm, tid);

  const int nF = n * F, K = nF + ne;                      // the graph's features
  int gp = 0, steps = K;                                  // GROUPED: the graph's first group and its number of groups
  if constexpr (GROUPED) {
    gp = __builtin_amdgcn_readfirstlane(a.group_ptr[g]);
    steps = __builtin_amdgcn_readfirstlane(a.group_ptr[g + 1]) - gp;
  }
  const long long seg = GROUPED ? (long long)gp : (long long)nbase * F + ebase;     // its segment of a permutation row
  const int32_t* const prow = a.perm + (size_t)(a.first + (int)blockIdx.y) * (size_t)a.row;
  int knext = 0, nq = 0, qi = 0;
  bool base = true;
  float vprev = 0.f;
  int off = 0;                                            // position of the output row in hv (set by the readout)

#pragma nounroll
  while (true) {
    int j = 0;
    if (!base) {
      // ------------------------------------------------------------------------------------------ the next step that needs an evaluation
      bool found = false;
      while (!found) {
        if (qi == nq) {
          if (knext >= steps) break;
          const int cnt = min(S_CHUNK, steps - knext);
          __syncthreads();                                 // (the chunk before has been walked)
          if (tid < cnt) {
            long long at = seg + knext + tid;
            at = at < a.row ? at : a.row - 1;
            const int jj = prow[at];
            int code = -1;
            float xv = 0.f;
            if constexpr (GROUPED) {
              // a group without a live member: its difference is 0 by definition, written at once
              if (jj >= 0 && jj < steps && (long long)gp + jj < a.row) {
                const int mb = a.member_ptr[gp + jj];
                if (a.member_ptr[gp + jj + 1] > mb) code = jj; else wsrow[gp + jj] = 0.f;
                xv = __int_as_float(mb);
              }
            } else if (jj >= 0 && jj < nF) {
              const size_t p = (size_t)nbase * F + jj;
              xv = cm.x[p];
              if (xv != 0.f) code = jj; else wsrow[p] = 0.f;
            } else if (jj >= nF && jj < K) {
              if (L.mval[jj - nF] >= 0.f) code = jj; else wsrow[a.NF + ebase + (jj - nF)] = 0.f;
            }
            L.pj[tid] = code;
            L.pv[tid] = xv;
          }
          __syncthreads();
          knext += cnt;
          nq = cnt;
          qi = 0;
          continue;
        }
        j = __builtin_amdgcn_readfirstlane(L.pj[qi]);
        found = j >= 0;
        ++qi;
      }
      if (!found) break;
      if constexpr (GROUPED) {
        const int mb = __builtin_amdgcn_readfirstlane(__float_as_int(L.pv[qi - 1]));
        const int me = __builtin_amdgcn_readfirstlane(a.member_ptr[gp + j + 1]);
        s_apply(L, cm, a.members, mb, me, nbase, nF, K, tid);
      } else if (j < nF) {
        if (wave == 0) {
          const float xv = s_uniform(L.pv[qi - 1]);
          const int i = j / F, f = j - i * F;
          L.h1[i * XS + lane] = fmaf(xv, cm.cW[0][lane * F + f], L.h1[i * XS + lane]);
        }
      } else if (tid == 0) {
        L.mval[j - nF] = 1.f;
      }
      __syncthreads();
    } else if constexpr (GROUPED) {
      // the background is on in every evaluation, the base included
      s_apply(L, cm, a.bg_members, __builtin_amdgcn_readfirstlane(a.bg_ptr[g]), __builtin_amdgcn_readfirstlane(a.bg_ptr[g + 1]),
              nbase, nF, K, tid);
      __syncthreads();
    }

    off = s_eval(L, cm, fmt, w, rw0, n, tid);
    const float v = L.hv[off + a.cls];
    if (base) {
      if (p0 && tid < C) out_base[(size_t)g * C + tid] = L.hv[off + tid];
    } else if (tid == 0) {
      wsrow[GROUPED ? (size_t)(gp + j) : j < nF ? (size_t)nbase * F + j : (size_t)(a.NF + ebase + (j - nF))] = v - vprev;
    }
    vprev = v;
    base = false;
    // (hv is next written behind the barriers of the next evaluation's conv stack)
  }
  // hv still holds the last evaluation: everything on (features that were skipped change nothing; GROUPED: every live
  // feature is in the background or in a group)
  if (p0 && tid < C) out[(size_t)g * C + tid] = L.hv[off + tid];
}

// HCG_EXPLAIN_COALITIONS: the table v(S) over every subset S of a graph's LIVE groups.  One workgroup per job (graph, run of
// consecutive subset masks), the LDS layout and the build of k_shapley_walk<true>.  For every mask m of the run the state is
// rebuilt from zero -- h1 = 0, mval = 0 for every edge with an entry, the live background applied, then the k-th live group for
// every set bit k of m, ascending, all through s_apply -- and evaluated once (s_eval); thread c < C writes output c to row
// live_ptr[g] + m.  Nothing is carried from one mask to the next, so a row is bitwise independent of the run it sits in, of
// the launch and of the rest of the batch; every row has one writer, there is no workspace, no reduce and no atomics.  The
// state of mask 2^(y + 1) - 1 takes the updates the walk's state takes in the identity order up to group y, in that order.
struct CArgs {
  XCommon c;
  float* table;                             // [rows][C]
  const int32_t* jobs;                      // [.][3] graph, first mask, masks
  const long long* live_ptr;                // [B + 1] graph g's rows: live_ptr[g] + mask
  const int32_t* group_ptr;                 // [B + 1] the LIVE groups of graph g (the grouped block's arrays)
  const int32_t* member_ptr;                // [G + 1]
  const int32_t* members;
  const int32_t* bg_ptr;                    // [B + 1]
  const int32_t* bg_members;
  long long rows, G, B;
  int first;                                // first job of this launch
};

constexpr int C_MAX_GROUPS = 16;

__global__ __launch_bounds__(XT) void k_coalition_values(const CArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const XCommon& cm = a.c;
  const SLds L = s_carve(smem, cm.npad, cm.emax);
  const int tid = threadIdx.x;
  const int C = cm.C;
  SJob jb;
  if (!s_job(jb, a, C_MAX_GROUPS)) return;
  const int g = jb.g, m0 = jb.first, mcount = jb.count, gp = jb.gp, ng = jb.ng;
  // the masks of the run that exist and whose rows lie inside the table
  const long long lp = a.live_ptr[g];
  const long long mlo = max(0ll, max((long long)m0, -lp));
  const long long mhi = min(min((long long)m0 + mcount, 1ll << ng), a.rows - lp);

  XSpan sp;
  if (x_refused(sp, cm, g, tid)) {
    for (long long k = mlo * C + tid; k < mhi * C; k += XT) a.table[lp * C + k] = 0.f;
    return;
  }
  const int nbase = sp.nbase, n = sp.n, ne = sp.ne;
  s_build(L, cm, sp, tid);
  const XMasked fmt{L.mval};
  float w[XD];
  float rw0[16];
  s_load_weights(w, rw0, cm, tid);
  const int nF = n * cm.F, K = nF + ne;
  const int bb = __builtin_amdgcn_readfirstlane(a.bg_ptr[g]), be = __builtin_amdgcn_readfirstlane(a.bg_ptr[g + 1]);

#pragma nounroll
  for (long long mm = mlo; mm < mhi; ++mm) {
    const int m = (int)mm;
    s_reset(L, n, ne, tid);
    s_apply(L, cm, a.bg_members, bb, be, nbase, nF, K, tid);
#pragma nounroll
    for (int k = 0; k < ng; ++k)
      if ((m >> k) & 1) {
        __syncthreads();                                   // (the staging of the list before has been read)
        s_apply(L, cm, a.members, __builtin_amdgcn_readfirstlane(a.member_ptr[gp + k]),
                __builtin_amdgcn_readfirstlane(a.member_ptr[gp + k + 1]), nbase, nF, K, tid);
      }
    __syncthreads();
    const int off = s_eval(L, cm, fmt, w, rw0, n, tid);
    if (tid < C) a.table[(lp + mm) * C + tid] = L.hv[off + tid];
    // (hv is next written behind the barriers of the next evaluation's conv stack)
  }
}

// HCG_EXPLAIN_SUBSETS: v(S) for a caller's list of subsets S of a graph's groups (ALL of them listed: a dead group has an
// empty member range, so bit y is the caller's group y), any number of groups up to V_MAX_GROUPS.  One workgroup per job
// (graph, first row, rows), the LDS layout and the build of the two kernels above.  Per row: the graph's bit words of the
// row are staged in pj / pv (512 words, idle here), the state is rebuilt from zero -- h1 = 0, mval = 0 for every edge with an
// entry, the live background through s_apply, the set groups through s_apply_subset: one filtered pass over the graph's
// member list, no global load per group -- and evaluated once (s_eval); thread c < C writes output c to row (s, g) of the
// [S][B][C] table.  Nothing is carried from row to row: a row depends on its bits and its graph alone.  For the same subset
// the state takes the updates k_coalition_values applies, in the same order, so the rows are bitwise that kernel's.
struct VArgs {
  XCommon c;
  float* table;                             // [S][B][C]
  const int32_t* jobs;                      // [.][3] graph, first row, rows
  const unsigned* bits;                     // [S][W]
  const int32_t* word_ptr;                  // [B + 1] graph g's words of a row: word_ptr[g] .., W = word_ptr[B]
  const int32_t* group_ptr;                 // [B + 1] ALL groups of graph g
  const int32_t* member_ptr;                // [G + 1]
  const int32_t* members;
  const int32_t* member_group;              // parallel to `members`: the member's local group id
  const int32_t* bg_ptr;                    // [B + 1]
  const int32_t* bg_members;
  long long S, G, B;
  int first;                                // first job of this launch
};

constexpr int V_MAX_GROUPS = 2 * S_CHUNK * 32;     // the bits pj / pv hold: 16384 (a graph inside the limits has <= 12800 features)

__global__ __launch_bounds__(XT) void k_subset_values(const VArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const XCommon cm = s_model(a.c, blockIdx.y);             // grid y: the model
  const SLds L = s_carve(smem, cm.npad, cm.emax);
  const int tid = threadIdx.x;
  const int C = cm.C;
  float* const table = a.table + (size_t)blockIdx.y * (size_t)a.S * (size_t)a.B * C;      // [M][S][B][C]: the model's slice
  SJob jb;
  if (!s_job(jb, a, V_MAX_GROUPS)) return;
  const int g = jb.g, s0 = jb.first, scount = jb.count, gp = jb.gp, ng = jb.ng;
  const int nw = (ng + 31) >> 5;                           // <= 512 = XT: one word per thread
  const int wp = __builtin_amdgcn_readfirstlane(a.word_ptr[g]);
  const int W = __builtin_amdgcn_readfirstlane(a.word_ptr[a.B]);
  if (wp < 0 || (long long)wp + nw > W) return;
  // the rows of the run that exist
  const long long slo = max(0ll, (long long)s0);
  const long long shi = min((long long)s0 + scount, a.S);

  XSpan sp;
  if (x_refused(sp, cm, g, tid)) {
    for (long long s = slo; s < shi; ++s)
      if (tid < C) table[((size_t)s * (size_t)a.B + g) * C + tid] = 0.f;
    return;
  }
  const int nbase = sp.nbase, n = sp.n, ne = sp.ne;
  s_build(L, cm, sp, tid);
  const XMasked fmt{L.mval};
  float w[XD];
  float rw0[16];
  s_load_weights(w, rw0, cm, tid);
  const int bb = __builtin_amdgcn_readfirstlane(a.bg_ptr[g]), be = __builtin_amdgcn_readfirstlane(a.bg_ptr[g + 1]);
  const int mb = __builtin_amdgcn_readfirstlane(a.member_ptr[gp]), me = __builtin_amdgcn_readfirstlane(a.member_ptr[gp + ng]);
  unsigned* const bits = reinterpret_cast<unsigned*>(L.pj);     // [2 S_CHUNK]: pj and pv lie side by side

#pragma nounroll
  for (long long s = slo; s < shi; ++s) {
    // the row's words (the evaluation before ended behind a barrier: pj / pv are idle), then the row
    if (tid < nw) bits[tid] = a.bits[(size_t)s * (size_t)W + wp + tid];
    const int off = s_row_subset(L, cm, fmt, w, rw0, a.bg_members, bb, be, a.members, a.member_group, bits, ng, mb, me, nbase,
                                 n, ne, tid);
    if (tid < C) table[((size_t)s * (size_t)a.B + g) * C + tid] = L.hv[off + tid];
    // (hv is next written behind the barriers of the next evaluation's conv stack)
  }
}

// HCG_EXPLAIN_GREEDY: one ROUND of the greedy insertion / deletion order of every graph's groups; launch k = a.round of a
// sequence the host enqueues on one stream without reading anything in between.  One workgroup per job (graph, first id, ids),
// the LDS layout, the build and the per-row sequence of k_subset_values.  The graph's on-set lives in pj / pv as bit words:
// the start state (empty, or full for a deletion run) with the picks 0 .. k - 2 flipped, read from the `order` prefix that
// the owners of earlier launches wrote.  For k >= 1 EVERY workgroup of the graph computes pick k - 1 itself from round
// k - 1's candidate values (half (k - 1) & 1 of `cand`, written by launch k - 1; this launch writes the other half): the live
// groups not yet picked, scanned with the total order (greater key, then lower id; NaN = -inf), so the pick does not depend
// on how the scan is split over threads, and no workgroup reads what a sibling writes in the same launch.  Only the owner
// (first id 0) records it: order[gp + k - 1] and the pick's C values.  The owner of launch 0 evaluates the all-on and the
// background-only rows.  Then the job's candidates: flip the bit in LDS, rebuild from zero and evaluate exactly as a
// k_subset_values row, write the C outputs to `cand`, flip the bit back -- bitwise that kernel's row for the same bits.
struct GArgs {
  XCommon c;
  float* values;                            // [G][C] row gp + k: the outputs after pick k
  float* cand;                              // [2][G][C]
  int32_t* order;                           // [G]
  float* out;                               // [B][C] everything on
  float* out_base;                          // [B][C] the background only
  const int32_t* jobs;                      // [.][3] graph, first id, ids
  const int32_t* group_ptr;                 // [B + 1] ALL groups of graph g
  const int32_t* member_ptr;                // [G + 1]
  const int32_t* members;
  const int32_t* member_group;              // parallel to `members`: the member's local group id
  const int32_t* bg_ptr;                    // [B + 1]
  const int32_t* bg_members;
  long long G, B;
  int first;                                // first job of this launch
  int round, cls;
  int deletion;                             // the on-set starts full; a picked group's bit is clear
  float sgn;                                // key = sgn * value[cls]
};

// (key, id) of lane a against lane b's: the greater key, then the lower id
__device__ __forceinline__ void g_better(float& bk, int& by, float ok, int oy) {
  if (ok > bk || (ok == bk && oy < by)) { bk = ok; by = oy; }
}

__global__ __launch_bounds__(XT) void k_greedy_round(const GArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const XCommon& cm = a.c;
  const SLds L = s_carve(smem, cm.npad, cm.emax);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = cm.C;
  // (s_job's decode, written out: through the function this kernel takes a 169th VGPR, which costs it a wave per SIMD)
  const int32_t* const job = a.jobs + 3 * ((size_t)a.first + blockIdx.x);
  const int g = __builtin_amdgcn_readfirstlane(job[0]);
  const int y0 = __builtin_amdgcn_readfirstlane(job[1]);
  const int ycount = __builtin_amdgcn_readfirstlane(job[2]);
  if (g < 0 || g >= a.B) return;
  const int gp = __builtin_amdgcn_readfirstlane(a.group_ptr[g]);
  const int ng = __builtin_amdgcn_readfirstlane(a.group_ptr[g + 1]) - gp;
  if (ng < 0 || ng > V_MAX_GROUPS || gp < 0 || (long long)gp + ng > a.G) return;
  const int nw = (ng + 31) >> 5;                           // <= 512 = XT: one word per thread
  const int k = a.round;
  const bool owner = y0 == 0;
  // the ids of the job that exist
  const int ylo = max(0, y0);
  const int yhi = (int)min((long long)y0 + ycount, (long long)ng);
  float* const cw = a.cand + ((size_t)(k & 1) * (size_t)a.G + gp) * C;                  // this round's candidates
  const float* const cr = a.cand + ((size_t)((k + 1) & 1) * (size_t)a.G + gp) * C;      // the round before's
  const bool record = owner && k >= 1 && k - 1 < ng;       // the owner's row of `values` and entry of `order`
  float* const vrow = a.values + (size_t)(gp + (record ? k - 1 : 0)) * C;

  XSpan sp;
  if (x_refused(sp, cm, g, tid)) {
    for (long long i = (long long)ylo * C + tid; i < (long long)yhi * C; i += XT) cw[i] = 0.f;
    if (owner && k == 0 && tid < C) { a.out[(size_t)g * C + tid] = 0.f; a.out_base[(size_t)g * C + tid] = 0.f; }
    if (record && tid < C) vrow[tid] = 0.f;
    return;
  }
  const bool evaluates = yhi > ylo || (owner && k == 0);   // (a job that only picks needs no graph)
  const int nbase = sp.nbase, n = sp.n, ne = sp.ne;
  float w[XD];
  float rw0[16];
  if (evaluates) {
    s_build(L, cm, sp, tid);
    s_load_weights(w, rw0, cm, tid);
  }
  const XMasked fmt{L.mval};
  const int bb = __builtin_amdgcn_readfirstlane(a.bg_ptr[g]), be = __builtin_amdgcn_readfirstlane(a.bg_ptr[g + 1]);
  const int mb = __builtin_amdgcn_readfirstlane(a.member_ptr[gp]), me = __builtin_amdgcn_readfirstlane(a.member_ptr[gp + ng]);
  unsigned* const bits = reinterpret_cast<unsigned*>(L.pj);     // [2 S_CHUNK]: pj and pv lie side by side

  // the row in `bits`, as k_subset_values evaluates it
  auto row = [&]() {
    return s_row_subset(L, cm, fmt, w, rw0, a.bg_members, bb, be, a.members, a.member_group, bits, ng, mb, me, nbase, n, ne, tid);
  };
  // a word of the state in which every group of the graph is on
  auto full_word = [&](int t) { return t == nw - 1 && (ng & 31) ? (1u << (ng & 31)) - 1u : 0xffffffffu; };

  if (owner && k == 0) {
    // ---------------------------------------------------------------------------------------------- launch 0: both ends
    if (tid < nw) bits[tid] = full_word(tid);
    __syncthreads();
    int off = row();
    if (tid < C) a.out[(size_t)g * C + tid] = L.hv[off + tid];
    if (tid < nw) bits[tid] = 0u;
    __syncthreads();
    off = row();
    if (tid < C) a.out_base[(size_t)g * C + tid] = L.hv[off + tid];
    __syncthreads();                                       // (the filtered pass has read the words)
  }

  // ------------------------------------------------------------------------------------------------ the on-set after picks 0 .. k - 2
  if (tid < nw) bits[tid] = a.deletion ? full_word(tid) : 0u;
  __syncthreads();
  for (int i = tid; i < min(k - 1, ng); i += XT) {
    const int y = a.order[gp + i];
    if (y >= 0 && y < ng) atomicXor(&bits[y >> 5], 1u << (y & 31));        // (integer: the picks are distinct, any order)
  }
  __syncthreads();

  if (k >= 1) {
    // ---------------------------------------------------------------------------------------------- pick k - 1
    float bk = -INFINITY;
    int by = 0x7fffffff;                                   // (no candidate: loses against every candidate, -inf keys included)
    for (int y = tid; y < ng; y += XT) {
      const bool picked = (((bits[y >> 5] >> (y & 31)) & 1u) != 0u) != (a.deletion != 0);
      if (!picked && a.member_ptr[gp + y + 1] > a.member_ptr[gp + y]) {
        float key = a.sgn * cr[(size_t)y * C + a.cls];
        if (!(key == key)) key = -INFINITY;
        g_better(bk, by, key, y);
      }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float ok = __shfl_xor(bk, d);
      const int oy = __shfl_xor(by, d);
      g_better(bk, by, ok, oy);
    }
    float* const rk = L.t1;                                // [XW] (idle between two evaluations)
    int* const ry = reinterpret_cast<int*>(L.t1) + XW;     // [XW]
    if (lane == 0) { rk[wave] = bk; ry[wave] = by; }
    __syncthreads();
    bk = rk[0];
    by = ry[0];
#pragma unroll
    for (int q = 1; q < XW; ++q) g_better(bk, by, rk[q], ry[q]);
    const int pick = __builtin_amdgcn_readfirstlane(by);
    if (pick < ng) {
      if (tid == 0) bits[pick >> 5] ^= 1u << (pick & 31);
      if (record) {
        if (tid == 0) a.order[gp + k - 1] = pick;
        if (tid < C) vrow[tid] = cr[(size_t)pick * C + tid];
      }
    }
    __syncthreads();
  }

  // -------------------------------------------------------------------------------------------------- the job's candidates
#pragma nounroll
  for (int y = ylo; y < yhi; ++y) {
    const unsigned m = 1u << (y & 31);
    const bool picked = ((__builtin_amdgcn_readfirstlane(bits[y >> 5]) & m) != 0u) != (a.deletion != 0);
    const bool live = __builtin_amdgcn_readfirstlane(a.member_ptr[gp + y + 1]) > __builtin_amdgcn_readfirstlane(a.member_ptr[gp + y]);
    if (picked || !live) continue;                         // (uniform: the words are the same for every thread)
    __syncthreads();                                       // (every thread has read the word)
    if (tid == 0) bits[y >> 5] ^= m;
    const int off = row();                                 // (its first barrier stands between the flip and the filtered pass)
    if (tid < C) cw[(size_t)y * C + tid] = L.hv[off + tid];
    if (tid == 0) bits[y >> 5] ^= m;
    __syncthreads();
    // (hv is next written behind the barriers of the next evaluation's conv stack)
  }
}

// acc[i] (+)= sum_p ws[p][i], p ascending; the call that ends at the last permutation divides by their number.  Grid y: the
// model -- its [count][row] slice of the workspace, its row of the accumulator, the same sum.
__global__ __launch_bounds__(256) void k_shapley_reduce(const float* __restrict__ ws, float* __restrict__ acc, long long row,
                                                        int count, int fresh, int last, float n_perm) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= row) return;
  ws += (size_t)blockIdx.y * (size_t)count * (size_t)row;
  acc += (size_t)blockIdx.y * (size_t)row;
  float s = fresh ? 0.f : acc[i];
  for (int p = 0; p < count; ++p) s += ws[(size_t)p * (size_t)row + i];
  acc[i] = last ? s / n_perm : s;
}

// the model axis of HCG_EXPLAIN_SHAPLEY and HCG_EXPLAIN_SUBSETS: n_models, 0 (what a caller of the one-model form leaves
// there) meaning 1, as HCG_EXPLAIN_INTEGRATED reads it
inline int s_models(const hcg_explain_args* p) { return p->n_models == 0 ? 1 : p->n_models; }

// ---- what the four launchers share.  Each calls these where it made the check itself: the order of a launcher's checks, and
// with it the code of every refused block, is what it was (tests/test_host_shapley_launch_codes.py).
// a pointer of another mode is set (`perm` belongs to HCG_EXPLAIN_SHAPLEY alone)
inline bool s_foreign(const hcg_explain_args* p, bool takes_perm) {
  return p->edge_mask || p->node_mask || p->target || p->dout || (!takes_perm && p->perm);
}

// the shapes these kernels take -> the dynamic LDS of one workgroup, or HCG_ERR_UNSUPPORTED
inline int s_lds(const hcg_explain_args* p) {
  if (!x_shapes_ok(p) || p->max_nodes > S_MAX_NODES) return HCG_ERR_UNSUPPORTED;
  const unsigned lds = s_lds_bytes(x_round4(p->max_nodes, S_NPAD_MIN), x_round4(p->max_edges, 4));
  return lds > 160 * 1024 ? HCG_ERR_UNSUPPORTED : (int)lds;
}

// the group lists of a launch: none may be NULL, an empty one included
inline bool s_lists_ok(const hcg_explain_args* p) {
  return p->shap_group_ptr && p->shap_member_ptr && p->shap_members && p->shap_bg_ptr && p->shap_bg_members;
}

// ... into the kernel's block, whichever it is (SGArgs, CArgs, VArgs, GArgs: the same member names)
template <class A>
void s_fill_lists(A& a, const hcg_explain_args* p) {
  a.group_ptr = p->shap_group_ptr;
  a.member_ptr = p->shap_member_ptr;
  a.members = p->shap_members;
  a.bg_ptr = p->shap_bg_ptr;
  a.bg_members = p->shap_bg_members;
  if constexpr (!std::is_same_v<A, SGArgs> && !std::is_same_v<A, CArgs>) a.member_group = p->sub_member_group;
}

}  // namespace

// hcg_explain, mode HCG_EXPLAIN_SHAPLEY (explain.hip dispatches here)
int hcg_shapley_launch(hcg_explain_args* p, hipStream_t stream) {
  if (s_foreign(p, true)) return HCG_ERR_INVALID_ARG;
  const int M = s_models(p);
  if (M < 1 || M > 65535) return HCG_ERR_INVALID_ARG;
  const int lds = s_lds(p);
  if (lds < 0) return lds;
  const bool grouped = (p->flags & HCG_EXPLAIN_GROUPED) != 0;
  const long long NF = (long long)p->N * p->F;
  // (every group has a member, so G <= N F + E)
  if (grouped && (p->shap_n_groups < 0 || p->shap_n_groups > NF + p->E)) return HCG_ERR_INVALID_ARG;
  const long long row = grouped ? (long long)p->shap_n_groups : NF + p->E;   // entries of a permutation and of a workspace row
  const int count = p->perm_count > 0 ? p->perm_count : 1;
  if (row >= (1ll << 31) || count > 65535) return HCG_ERR_UNSUPPORTED;
  p->lds_bytes = lds;
  // one row of differences per permutation of this call and model: M times the one-model figure ([M][count][row], packed)
  p->workspace_bytes_needed = (size_t)M * hcg_align_up((size_t)count * (size_t)(row > 0 ? row : 1) * sizeof(float), 256);
  if (p->flags & HCG_EXPLAIN_QUERY) return HCG_OK;
  if (p->n_perm < 1 || p->perm_count < 1 || p->perm_first < 0 || (long long)p->perm_first + p->perm_count > p->n_perm ||
      p->class_index < 0 || p->class_index >= p->C)
    return HCG_ERR_INVALID_ARG;
  if (p->B == 0) return HCG_OK;
  if (!x_common_ok(p) || !p->out_base || (row > 0 && (!p->perm || !p->shap_acc))) return HCG_ERR_INVALID_ARG;
  if (grouped && !s_lists_ok(p)) return HCG_ERR_INVALID_ARG;
  if (row > 0 && (!p->workspace || p->workspace_bytes < p->workspace_bytes_needed)) return HCG_ERR_WORKSPACE;

  SGArgs a{};
  x_fill_common(a.c, p, S_NPAD_MIN);
  a.perm = p->perm;
  a.out = p->out;
  a.out_base = p->out_base;
  a.ws = (float*)p->workspace;
  a.NF = NF;
  a.Etot = p->E;
  a.row = row;
  a.first = p->perm_first;
  a.cls = p->class_index;
  if (grouped) s_fill_lists(a, p);                          // (the union holds these in a grouped call only: else NULL)
  const dim3 grid((unsigned)p->B, (unsigned)p->perm_count, (unsigned)M);
  const int rc = grouped ? x_launch<k_shapley_walk<true, SGArgs>>(grid, lds, stream, a)
                         : x_launch<k_shapley_walk<false, SArgs>>(grid, lds, stream, static_cast<const SArgs&>(a));
  if (rc != HCG_OK) return rc;
  if (row > 0) {
    hipLaunchKernelGGL(k_shapley_reduce, dim3((unsigned)hcg_cdiv(row, 256), (unsigned)M), dim3(256), 0, stream, (const float*)p->workspace,
                       p->shap_acc, row, p->perm_count, p->perm_first == 0 ? 1 : 0,
                       p->perm_first + p->perm_count == p->n_perm ? 1 : 0, (float)p->n_perm);
    HCG_CHECK_LAUNCH();
  }
  return HCG_OK;
}

// hcg_explain, mode HCG_EXPLAIN_COALITIONS (explain.hip dispatches here)
int hcg_coalitions_launch(hcg_explain_args* p, hipStream_t stream) {
  if (s_foreign(p, false)) return HCG_ERR_INVALID_ARG;
  if (p->n_models > 1) return HCG_ERR_UNSUPPORTED;          // (the kernel has no model axis: never one model silently)
  const int lds = s_lds(p);
  if (lds < 0) return lds;
  if (p->coal_max_live > C_MAX_GROUPS || p->coal_rows >= (1ll << 31)) return HCG_ERR_UNSUPPORTED;
  p->lds_bytes = lds;
  p->workspace_bytes_needed = 0;
  if (p->flags & HCG_EXPLAIN_QUERY) return HCG_OK;
  if (p->coal_max_live < 0 || p->coal_rows < 0 || p->shap_n_groups < 0 || p->coal_job_first < 0 || p->coal_job_count < 0)
    return HCG_ERR_INVALID_ARG;
  if (p->B == 0 || p->coal_job_count == 0) return HCG_OK;
  if (!x_common_ok(p, false) || !p->coal_values || !p->coal_jobs || !p->coal_live_ptr || !s_lists_ok(p)) return HCG_ERR_INVALID_ARG;

  CArgs a;
  x_fill_common(a.c, p, S_NPAD_MIN);
  a.table = p->coal_values;
  a.jobs = p->coal_jobs;
  a.live_ptr = reinterpret_cast<const long long*>(p->coal_live_ptr);
  s_fill_lists(a, p);
  a.rows = p->coal_rows;
  a.G = p->shap_n_groups;
  a.B = p->B;
  a.first = p->coal_job_first;
  return x_launch<k_coalition_values>(dim3((unsigned)p->coal_job_count), lds, stream, a);
}

// hcg_explain, mode HCG_EXPLAIN_SUBSETS (explain.hip dispatches here)
int hcg_subsets_launch(hcg_explain_args* p, hipStream_t stream) {
  if (s_foreign(p, false)) return HCG_ERR_INVALID_ARG;
  const int M = s_models(p);
  if (M < 1 || M > 65535) return HCG_ERR_INVALID_ARG;
  const int lds = s_lds(p);
  if (lds < 0) return lds;
  if (p->sub_max_groups > V_MAX_GROUPS || p->coal_rows >= (1ll << 31)) return HCG_ERR_UNSUPPORTED;
  p->lds_bytes = lds;
  p->workspace_bytes_needed = 0;
  if (p->flags & HCG_EXPLAIN_QUERY) return HCG_OK;
  if (p->sub_max_groups < 0 || p->coal_rows < 0 || p->shap_n_groups < 0 || p->coal_job_first < 0 || p->coal_job_count < 0)
    return HCG_ERR_INVALID_ARG;
  if (p->B == 0 || p->coal_job_count == 0) return HCG_OK;
  if (!x_common_ok(p, false) || !p->coal_values || !p->coal_jobs || !p->sub_bits || !p->sub_word_ptr || !p->sub_member_group ||
      !s_lists_ok(p))
    return HCG_ERR_INVALID_ARG;

  VArgs a;
  x_fill_common(a.c, p, S_NPAD_MIN);
  a.table = p->coal_values;
  a.jobs = p->coal_jobs;
  a.bits = p->sub_bits;
  a.word_ptr = p->sub_word_ptr;
  s_fill_lists(a, p);
  a.S = p->coal_rows;
  a.G = p->shap_n_groups;
  a.B = p->B;
  a.first = p->coal_job_first;
  return x_launch<k_subset_values>(dim3((unsigned)p->coal_job_count, (unsigned)M), lds, stream, a);
}

// hcg_explain, mode HCG_EXPLAIN_GREEDY (explain.hip dispatches here)
int hcg_greedy_launch(hcg_explain_args* p, hipStream_t stream) {
  if (s_foreign(p, false)) return HCG_ERR_INVALID_ARG;
  // (what is wrong whatever the shapes are, by a query too: the column, the round, the flags)
  if (p->class_index < 0 || p->class_index >= p->C || p->greedy_round < 0 ||
      (p->greedy_flags & ~(HCG_GREEDY_DELETION | HCG_GREEDY_NEGATE)))
    return HCG_ERR_INVALID_ARG;
  if (p->n_models > 1) return HCG_ERR_UNSUPPORTED;          // (the pick would need a reduction over the models inside a round)
  const int lds = s_lds(p);
  if (lds < 0) return lds;
  if (p->sub_max_groups > V_MAX_GROUPS) return HCG_ERR_UNSUPPORTED;
  p->lds_bytes = lds;
  p->workspace_bytes_needed = 0;
  if (p->flags & HCG_EXPLAIN_QUERY) return HCG_OK;
  if (p->sub_max_groups < 0 || p->shap_n_groups < 0 || p->shap_n_groups >= (1ll << 31) || p->coal_job_first < 0 ||
      p->coal_job_count < 0)
    return HCG_ERR_INVALID_ARG;
  if (p->B == 0 || p->coal_job_count == 0) return HCG_OK;
  if (!x_common_ok(p) || !p->out_base || !p->coal_values || !p->coal_jobs || !p->greedy_order || !p->greedy_cand ||
      !p->sub_member_group || !s_lists_ok(p))
    return HCG_ERR_INVALID_ARG;

  GArgs a;
  x_fill_common(a.c, p, S_NPAD_MIN);
  a.values = p->coal_values;
  a.cand = p->greedy_cand;
  a.order = p->greedy_order;
  a.out = p->out;
  a.out_base = p->out_base;
  a.jobs = p->coal_jobs;
  s_fill_lists(a, p);
  a.G = p->shap_n_groups;
  a.B = p->B;
  a.first = p->coal_job_first;
  a.round = p->greedy_round;
  a.cls = p->class_index;
  a.deletion = (p->greedy_flags & HCG_GREEDY_DELETION) ? 1 : 0;
  a.sgn = (p->greedy_flags & HCG_GREEDY_NEGATE) ? -1.f : 1.f;
  return x_launch<k_greedy_round>(dim3((unsigned)p->coal_job_count), lds, stream, a);
}
