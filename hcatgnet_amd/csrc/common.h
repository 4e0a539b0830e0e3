// Internal helpers shared by the HIP translation units of libhcatgnet_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/hcatgnet_hip.h"

#define HCG_WAVE 64

static inline int hcg_hip_err(hipError_t e) { return e == hipSuccess ? HCG_OK : (HCG_ERR_HIP_BASE - (int)e); }

// launch + return on error (kernel launch errors are sticky-free: read with hipGetLastError)
#define HCG_CHECK_LAUNCH()                                  \
  do {                                                      \
    hipError_t _e = hipGetLastError();                      \
    if (_e != hipSuccess) return hcg_hip_err(_e);           \
  } while (0)

#define HCG_TRY(expr)                 \
  do {                                \
    int _rc = (expr);                 \
    if (_rc != HCG_OK) return _rc;    \
  } while (0)

static inline size_t hcg_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline int64_t hcg_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// bump allocator over the caller's workspace
struct HcgArena {
  char* base;
  size_t size, off;
  HcgArena(void* p, size_t n) : base((char*)p), size(n), off(0) {}
  template <typename T>
  T* take(size_t count) {
    size_t bytes = hcg_align_up(count * sizeof(T), 256);
    if (off + bytes > size) return nullptr;
    T* r = (T*)(base + off);
    off += bytes;
    return r;
  }
};

// torch.optim.Adam's update of one element (amsgrad / weight_decay / maximize off), shared by every kernel that applies it
// (optim.hip, reduce.hip) and written with explicit roundings: left to the compiler, the fused and the stand-alone update
// contracted these expressions into different fma's, and with eps = 1e-9 (model/networks.py:38) a last-bit difference in a
// moment of a near-zero gradient becomes an lr-sized difference of the parameter.
//   step_size = lr / (1 - b1^t), bc2_sqrt = sqrt(1 - b2^t)
__device__ __forceinline__ float hcg_adam_update(float p, float g, float& m, float& v, float b1, float b2, float eps,
                                                 float step_size, float bc2_sqrt) {
  m = __fmaf_rn(b1, m, __fmul_rn(1.0f - b1, g));
  v = __fmaf_rn(b2, v, __fmul_rn(__fmul_rn(1.0f - b2, g), g));
  const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), bc2_sqrt), eps);
  return __fsub_rn(p, __fmul_rn(step_size, __fdiv_rn(m, denom)));
}

// b^t for an integer t >= 0 by squaring, in double: a few ulp of double, far inside the float the caller rounds to
// (torch computes `1 - beta ** step` in Python doubles); ~20 multiplications instead of a library pow().  Adam's bias
// corrections from a step count held on the device (optim.hip, reduce.hip, explain.hip).
__device__ __forceinline__ double hcg_powi(double b, int t) {
  double r = 1.0;
  while (t > 0) {
    if (t & 1) r *= b;
    b *= b;
    t >>= 1;
  }
  return r;
}

// torch.optim.SGD's update (momentum / weight_decay / maximize off) and torch.optim.RMSprop's (momentum / centered /
// weight_decay / maximize off), explicitly rounded for the same reason as hcg_adam_update
__device__ __forceinline__ float hcg_sgd_update(float p, float g, float lr) { return __fsub_rn(p, __fmul_rn(lr, g)); }

__device__ __forceinline__ float hcg_rmsprop_update(float p, float g, float& v, float alpha, float eps, float lr) {
  v = __fmaf_rn(alpha, v, __fmul_rn(__fmul_rn(1.0f - alpha, g), g));
  return __fsub_rn(p, __fmul_rn(lr, __fdiv_rn(g, __fadd_rn(__fsqrt_rn(v), eps))));
}

__device__ __forceinline__ float hcg_leaky(float v, float slope) { return v > 0.f ? v : v * slope; }
__device__ __forceinline__ float hcg_leaky_grad(float y_out, float slope) { return y_out > 0.f ? 1.f : slope; }

// Cross-entropy of ONE graph (nn.CrossEntropyLoss with default settings on class-index targets): v[0 .. C) holds the
// logits on entry and the error softmax(v)[c] - [c == label] on return (entries >= C: 0); returns the loss term
// logsumexp(v) - v[label] as log(sum exp(v - max)) - (v[label] - max).  Class and label meet by comparing (float)c == label,
// nothing is indexed by the label: a label that equals none of 0 .. C-1 (out of range, negative, not an integer, NaN) leaves
// the NaN the term starts from.  expf / logf, not the fast intrinsics: at most RC values per graph.
template <int RC>
__device__ __forceinline__ float hcg_ce_row(float (&v)[RC], int C, float label) {
  float m = v[0];
#pragma unroll
  for (int c = 1; c < RC; ++c)
    if (c < C) m = fmaxf(m, v[c]);
  float sum = 0.f, picked = __builtin_nanf("");
#pragma unroll
  for (int c = 0; c < RC; ++c) {
    if (c < C) {
      const float sh = v[c] - m;
      if ((float)c == label) picked = sh;
      v[c] = expf(sh);
      sum += v[c];
    }
  }
  const float inv = 1.0f / sum;
#pragma unroll
  for (int c = 0; c < RC; ++c) v[c] = c < C ? v[c] * inv - ((float)c == label ? 1.f : 0.f) : 0.f;
  return logf(sum) - picked;
}

// ---- internal launchers implemented in gemm.hip -------------------------------------------
// C[M,N] = sum_k A(m,k) B(k,n), A(m,k) at A[m*sam + k*sak], B(k,n) at B[k*sbk + n*sbn];
// epilogue: + bias[n] (nullable), LeakyReLU when act.  splits > 1: deterministic split-K through
// `partials` ([splits, M, N] floats).
size_t hcg_gemm_partial_floats(int64_t M, int64_t N, int64_t K, int* splits_out);
int hcg_gemm(const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn,
             float* C, int64_t M, int64_t N, int64_t K, const float* bias, int act, float slope,
             float* partials, size_t partial_floats, hipStream_t stream);
// out[d] = sum_m src[m, d]  (deterministic two-stage); partials >= colsum_partial_floats
size_t hcg_colsum_partial_floats(int64_t M, int64_t D);
int hcg_colsum(const float* src, float* out, int64_t M, int64_t D, float* partials, hipStream_t stream);

// ---- the any-shape layer's edge-multiplier gradient (layer.hip), reached through hcg_explain (explain.hip) ----------
int hcg_edge_weight_grad_launch(const float* dout, const float* out, const float* h, const int32_t* rowptr, const int32_t* col,
                                const float* dinv, float slope, int apply_act, float* dew_csr, int64_t N, int64_t E, int64_t D,
                                hipStream_t stream);

// ---- the ensemble forward (ensemble.hip), reached through hcg_explain, mode HCG_EXPLAIN_ENSEMBLE (explain.hip) ----------
int hcg_ensemble_launch(hcg_explain_args* p, hipStream_t stream);
// ---- Shapley value sampling (shapley.hip), reached through hcg_explain, mode HCG_EXPLAIN_SHAPLEY -------------------------
int hcg_shapley_launch(hcg_explain_args* p, hipStream_t stream);
// mode HCG_EXPLAIN_COALITIONS: the table over every subset of a graph's live groups
int hcg_coalitions_launch(hcg_explain_args* p, hipStream_t stream);
// mode HCG_EXPLAIN_SUBSETS: the values of a list of subsets of a graph's groups
int hcg_subsets_launch(hcg_explain_args* p, hipStream_t stream);
// mode HCG_EXPLAIN_GREEDY: one round of the greedy insertion / deletion order of a graph's groups
int hcg_greedy_launch(hcg_explain_args* p, hipStream_t stream);

// ---- the fit controller (fit.hip), reached through hcg_update_dev (optim.hip): `fit_control` of hcg_update_args ----------
int hcg_fit_control_launch(const hcg_fit_control_args* a, hipStream_t stream);

// ---- an epoch's shuffle and index arrays (shuffle.hip), reached through hcg_collate (collate.hip): `epoch_draw` of
//      hcg_collate_args, not NULL ----------
int hcg_epoch_draw_launch(const hcg_collate_args* c, hipStream_t stream);

// ---- one-graph-per-wave kernels (wave.hip), selected inside the hcg_mid_* entry points (mid.hip) ----------
int hcg_w64_applicable(int64_t F, int64_t D, int64_t max_nodes, int64_t max_edges);
int hcg_w64_bwd_grid(int64_t B);
int hcg_w64_fwd_launch(const float* x, const float* W, const float* b, const int64_t* edge_index, int64_t E,
                       const int32_t* graph_ptr, const int32_t* edge_ptr, int64_t B, int64_t F, float slope, int apply_act,
                       float* out, float* emb, int32_t* status, hipStream_t stream);
int hcg_w64_bwd_launch(const float* dout, const float* demb, const float* emb, const float* out, const float* x,
                       const float* W, const int64_t* edge_index, int64_t E, const int32_t* graph_ptr,
                       const int32_t* edge_ptr, int64_t B, int64_t F, float slope, int apply_act, float* dx,
                       float* partials, int32_t* status, hipStream_t stream);
