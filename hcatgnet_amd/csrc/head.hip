// Regression head as ONE stand-alone launch (SURVEY rows a10, a12 and their part of a11; f2): the form used behind conv
// stacks whose forward is more than one launch (one graph per workgroup / wave, wide layers, size-grouped batches).  The
// small-graph tiles carry the same tile code in the tail of their forward launch instead (fused.hip).
// As separate launches (readout fwd, mse fwd, sqrt, three torch kernels of sqrt's backward, mse bwd, readout bwd) this
// dependent chain of eight tiny kernels cost ~39 us of a 132 us training step: pure launch latency around 67 MFLOP.
// One workgroup per 32-graph tile, forward and backward of a tile back to back; nothing waits for another workgroup
// (head_tile.h: the loss scale is deferred to the step's last launch), so the grid is simply min(tiles, CUs).
#include "common.h"
#include "head_tile.h"
#include "launch.h"

namespace {
using namespace hcg_head;

template <int RD, int RC, bool BACKWARD, int LOSS = LOSS_SQ>
__global__ __launch_bounds__(HC<RD>::NT, 1) void k_head(const float* __restrict__ emb, const float* __restrict__ y,
                                                       const float* __restrict__ W0, const float* __restrict__ b0,
                                                       const float* __restrict__ W1, const float* __restrict__ b1, int B, int C,
                                                       float slope, float* __restrict__ z, float* __restrict__ out,
                                                       float* __restrict__ demb, float* __restrict__ slabs,
                                                       int* __restrict__ step_counter) {
  __shared__ HeadLds<RD> L;
  HeadState<RD, RC> S;
  const int tiles = (B + RT - 1) / RT;
  if (step_counter && blockIdx.x == 0 && threadIdx.x == 0) { step_counter[0] += 1; step_counter[1] += 1; }   // this training step's number, for the update launched later | exchange stamp
  head_begin<RD, RC>(L, S, W0, b0, W1, b1, C);
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int g0 = t * RT, n = B - g0 < RT ? B - g0 : RT;
    head_tile<RD, RC, BACKWARD, LOSS>(L, S, [g0](int row) { return g0 + row; }, n, C, slope, emb, y, W0, z, out, demb);
  }
  head_end<RD, RC, BACKWARD>(L, S, C, slabs + (size_t)blockIdx.x * HC<RD>::SLAB, slabs + (size_t)gridDim.x * HC<RD>::SLAB + blockIdx.x);
}

// D = 64: the stand-alone launch runs the latency-cut 16-row tile code of the forward's tail (head_tile.h: hcg_head16; 8
// waves, weight fragments in registers straight from L2): its per-tile chain is about half the 32-row code's, and without a
// grid-wide exchange nothing ties the grid to one workgroup per 32 graphs -- 16 graphs per tile fill twice the CUs
// (B = 4096: 256 workgroups instead of 128).
template <int RC, bool BACKWARD, int LOSS = LOSS_SQ>
__global__ __launch_bounds__(hcg_head16::NT, 1) void k_head16(const float* __restrict__ emb, const float* __restrict__ y,
                                                             const float* __restrict__ W0, const float* __restrict__ b0,
                                                             const float* __restrict__ W1, const float* __restrict__ b1, int B,
                                                             int C, float slope, float* __restrict__ z, float* __restrict__ out,
                                                             float* __restrict__ demb, float* __restrict__ slabs,
                                                             int* __restrict__ step_counter) {
  namespace h16 = hcg_head16;
  __shared__ h16::Lds L;
  if (step_counter && blockIdx.x == 0 && threadIdx.x == 0) { step_counter[0] += 1; step_counter[1] += 1; }
  h16::Prefetch<RC> P;
  h16::prefetch<RC, LOSS>(P, W0, b0, W1, C);
  h16::State<RC> S;
  h16::begin<RC, LOSS>(S, b1, C);
  constexpr int T16 = h16::RT;
  const int tiles = (B + T16 - 1) / T16;
  bool first = true;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int g0 = t * T16, n = B - g0 < T16 ? B - g0 : T16;
    h16::tile<RC, BACKWARD, LOSS>(L, S, P, [g0](int row) { return g0 + row; }, n, C, slope, nullptr, emb, y, z, out, demb, first);
    first = false;
  }
  __syncthreads();
  h16::end<RC, BACKWARD, LOSS>(L, S, C, slabs + (size_t)blockIdx.x * h16::SLAB, slabs + (size_t)gridDim.x * h16::SLAB + blockIdx.x);
}

// min(tiles of rt graphs, CUs)
int head_grid_rt(int64_t B, int rt) { return hcg_grid((B + rt - 1) / rt, hcg_cu_count()); }
int head_grid(int64_t B, int64_t D = 128) { return head_grid_rt(B, D == 64 ? hcg_head16::RT : RT); }
size_t head_slab(int64_t D) { return D == 128 ? (size_t)HC<128>::SLAB : (size_t)HC<64>::SLAB; }

}  // namespace

extern "C" int hcg_head_supported(int64_t D, int64_t C) { return ((D == 64 || D == 128) && C >= 1 && C <= RCMAX) ? 1 : 0; }

// workspace: [grid][SLAB] gradient slabs | [grid] SSE partials
extern "C" size_t hcg_head_workspace_bytes(int64_t B, int64_t D) {
  if (D != 64 && D != 128) return 0;
  return hcg_align_up((size_t)head_grid(B, D) * (head_slab(D) + 1) * sizeof(float), 256) + 256;
}

extern "C" int hcg_head_fwd_bwd(const float* emb, const float* y, const float* W0, const float* b0, const float* W1,
                                const float* b1, int64_t B, int64_t D, int64_t C, float slope, int flags, float* z,
                                float* out, float* demb, void* workspace, size_t workspace_bytes, int32_t* step_counter,
                                hcg_stream_t stream) {
  if (!hcg_head_supported(D, C)) return HCG_ERR_UNSUPPORTED;
  if (flags & ~(HCG_HEAD_FORWARD_ONLY | HCG_HEAD_LOSS_CE)) return HCG_ERR_INVALID_ARG;
  const bool bwd = !(flags & HCG_HEAD_FORWARD_ONLY), ce = (flags & HCG_HEAD_LOSS_CE) != 0;
  if (ce && C < 2) return HCG_ERR_INVALID_ARG;          // (a softmax over one class has nothing to learn)
  if (B <= 0 || !emb || !y || !W0 || !b0 || !W1 || !b1 || !z || !out || (bwd && !demb) || !workspace) return HCG_ERR_INVALID_ARG;
  if (workspace_bytes < hcg_head_workspace_bytes(B, D)) return HCG_ERR_WORKSPACE;
  const int grid = head_grid(B, D);
  float* slabs = (float*)workspace;
#define LAUNCH_HEAD(RD_, RC_, BW, ...)                                                                                    \
  hipLaunchKernelGGL((k_head<RD_, RC_, BW, ##__VA_ARGS__>), dim3(grid), dim3(HC<RD_>::NT), 0, (hipStream_t)stream, emb, y, W0, \
                     b0, W1, b1, (int)B, (int)C, slope, z, out, demb, slabs, (int*)step_counter)
#define DISPATCH_HEAD(RD_)                                                                            \
  do {                                                                                                \
    if (C == 1) { if (bwd) LAUNCH_HEAD(RD_, 1, true); else LAUNCH_HEAD(RD_, 1, false); }              \
    else        { if (bwd) LAUNCH_HEAD(RD_, RCMAX, true); else LAUNCH_HEAD(RD_, RCMAX, false); }      \
  } while (0)
#define LAUNCH_HEAD16(RC_, BW, ...)                                                                                       \
  hipLaunchKernelGGL((k_head16<RC_, BW, ##__VA_ARGS__>), dim3(grid), dim3(hcg_head16::NT), 0, (hipStream_t)stream, emb, y, W0, \
                     b0, W1, b1, (int)B, (int)C, slope, z, out, demb, slabs, (int*)step_counter)
  if (ce) {       // (two classes or more: the eight-class instantiations)
    if (D == 128) { if (bwd) LAUNCH_HEAD(128, RCMAX, true, LOSS_CE); else LAUNCH_HEAD(128, RCMAX, false, LOSS_CE); }
    else          { if (bwd) LAUNCH_HEAD16(RCMAX, true, LOSS_CE); else LAUNCH_HEAD16(RCMAX, false, LOSS_CE); }
  } else if (D == 128) {
    DISPATCH_HEAD(128);
  } else if (C == 1) {
    if (bwd) LAUNCH_HEAD16(1, true); else LAUNCH_HEAD16(1, false);
  } else {
    if (bwd) LAUNCH_HEAD16(RCMAX, true); else LAUNCH_HEAD16(RCMAX, false);
  }
#undef LAUNCH_HEAD16
#undef DISPATCH_HEAD
#undef LAUNCH_HEAD
  HCG_CHECK_LAUNCH();
  return HCG_OK;
}

extern "C" int hcg_head_reduce_job(const void* workspace, size_t workspace_bytes, int64_t B, int64_t D, int64_t C, float* dW0,
                                   float* db0, float* dW1, float* db1, hcg_reduce_job* job) {
  if (B <= 0 || (D != 64 && D != 128) || C < 1 || C > RCMAX || !job || !workspace) return HCG_ERR_INVALID_ARG;
  if (dW0 && (!db0 || !dW1 || !db1)) return HCG_ERR_INVALID_ARG;
  if (workspace_bytes < hcg_head_workspace_bytes(B, D)) return HCG_ERR_WORKSPACE;
  if (D == 128) head_fill_job<128>((const float*)workspace, head_grid(B, D), (int)C, dW0, db0, dW1, db1, job);
  else head_fill_job<64>((const float*)workspace, head_grid(B, D), (int)C, dW0, db0, dW1, db1, job);
  return HCG_OK;
}

// ======================================================================================================================
// Readout heads of depth R = 1, 3, 4 in ONE launch (reference model/gcn.py:36-45: widths 2D -> D -> D/2 -> ..., LeakyReLU
// behind every hidden layer, a last Linear(w, C) without one), with k_head's contract: forward, squared error, backward on
// the unscaled error, one gradient slab + SSE partial per workgroup, the step counter.  One workgroup per 16-graph tile
// (grid <= CUs, a workgroup loops over tiles beyond that); the tile's activations and errors stay in LDS, the weights come
// from L2.  Plain f32 FMA: a few MFLOP per step, and every layer runs the same three loops.  Each gradient element has one
// owning thread that adds its tile's graphs in order and its tiles in order: no atomics, bitwise repeatable.
// ======================================================================================================================
namespace {
namespace deep {

constexpr int TG = 16;     // graphs per tile
constexpr int NT = 256;    // threads per workgroup

__host__ __device__ constexpr int kin(int D, int i) { return (2 * D) >> i; }                 // input width of layer i
// slab offset of layer i's [dW | db]: the hidden layers before it (out = in / 2)
__host__ __device__ constexpr int seg_off(int D, int i) { return i == 0 ? 0 : seg_off(D, i - 1) + (kin(D, i - 1) / 2) * (kin(D, i - 1) + 1); }
// LDS offset (per graph row) of layer i's input activations
__host__ __device__ constexpr int act_off(int D, int i) { return i == 0 ? 0 : act_off(D, i - 1) + kin(D, i - 1); }
inline int slab_floats(int D, int R, int C) {
  return (int)hcg_align_up((size_t)seg_off(D, R - 1) + (size_t)C * (kin(D, R - 1) + 1), 8);
}

template <int D, int R>
struct Lds {
  float act[TG * act_off(D, R)];     // every layer's input rows, layer after layer (layer 0's = the embedding)
  float d[2][TG * D];                // errors of a layer's outputs / of its input (ping-pong)
  float red[NT];
};

// layer I: x [n, K] -> LeakyReLU(x W^T + b) [n, K/2] into the next layer's input rows; the last layer: out = x W^T + b
// [n, C] to global memory, the error out - y into d[0], the squared error into this thread's partial.  LOSS_CE: the logits
// go into d[0], and behind a barrier thread g < n turns graph g's row into softmax - onehot and adds the graph's loss term
// to its partial (a second pass per row: the error needs all of a row's logits)
template <int D, int R, int I, int LOSS = LOSS_SQ>
__device__ __forceinline__ void fwd_layer(Lds<D, R>& L, const hcg_head_args& a, int n, int g0, float& sse) {
  constexpr int K = kin(D, I);
  constexpr bool LAST = I == R - 1;
  const int C = (int)a.C, O = LAST ? C : K / 2;
  const float* __restrict__ W = a.W[I];
  const float* __restrict__ b = a.b[I];
  const float4* x4 = reinterpret_cast<const float4*>(L.act + TG * act_off(D, I));
  for (int idx = threadIdx.x; idx < n * O; idx += NT) {
    const int g = idx / O, o = idx - g * O;
    const float4* w4 = reinterpret_cast<const float4*>(W + (size_t)o * K);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll 8
    for (int k = 0; k < K / 4; ++k) {
      const float4 w = w4[k], v = x4[g * (K / 4) + k];
      s0 = fmaf(v.x, w.x, s0); s1 = fmaf(v.y, w.y, s1); s2 = fmaf(v.z, w.z, s2); s3 = fmaf(v.w, w.w, s3);
    }
    const float v = ((s0 + s1) + (s2 + s3)) + b[o];
    if constexpr (!LAST) {
      L.act[TG * act_off(D, I + 1) + g * O + o] = hcg_leaky(v, a.slope);
    } else {
      const size_t row = (size_t)(g0 + g) * C + o;
      a.out[row] = v;
      if constexpr (LOSS == LOSS_CE) {
        L.d[0][g * O + o] = v;
      } else {
        const float e = v - a.y[row];
        sse = fmaf(e, e, sse);
        L.d[0][g * O + o] = e;
      }
    }
  }
  if constexpr (LAST && LOSS == LOSS_CE) {
    __syncthreads();
    if ((int)threadIdx.x < n) {
      float* row = L.d[0] + threadIdx.x * C;
      float v[RCMAX];
#pragma unroll
      for (int c = 0; c < RCMAX; ++c) v[c] = row[c < C ? c : 0];
      sse += hcg_ce_row<RCMAX>(v, C, a.y[g0 + threadIdx.x]);
#pragma unroll
      for (int c = 0; c < RCMAX; ++c)
        if (c < C) row[c] = v[c];
    }
  }
}

// layer I's backward from the errors of its outputs (d[P], [n, O]): dW += d^T x, db += sum d (this workgroup's slab; the
// first tile writes, later ones add), dx = d W -- times the LeakyReLU derivative of layer I - 1 into d[P ^ 1], or, for the
// first layer, demb to global memory
// (LOSS: the code does not depend on it, but an instantiation shared by the kernels of both losses changed the register
//  allocation of the regression kernels that inline it)
template <int D, int R, int I, int P, int LOSS = LOSS_SQ>
__device__ __forceinline__ void bwd_layer(Lds<D, R>& L, const hcg_head_args& a, int n, int g0, float* __restrict__ slab,
                                          bool first) {
  constexpr int K = kin(D, I), K4 = K / 4;
  constexpr bool LAST = I == R - 1;
  const int O = LAST ? (int)a.C : K / 2;
  const float* dl = L.d[P];
  const float4* x4 = reinterpret_cast<const float4*>(L.act + TG * act_off(D, I));
  float* __restrict__ dWb = slab + seg_off(D, I);
  for (int idx = threadIdx.x; idx < O * K4; idx += NT) {
    const int o = idx / K4, k4 = idx - o * K4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int g = 0; g < n; ++g) {
      const float e = dl[g * O + o];
      const float4 v = x4[g * K4 + k4];
      s.x = fmaf(e, v.x, s.x); s.y = fmaf(e, v.y, s.y); s.z = fmaf(e, v.z, s.z); s.w = fmaf(e, v.w, s.w);
    }
    float4* dst = reinterpret_cast<float4*>(dWb) + idx;
    if (!first) {
      const float4 p = *dst;
      s = make_float4(p.x + s.x, p.y + s.y, p.z + s.z, p.w + s.w);
    }
    *dst = s;
  }
  for (int o = threadIdx.x; o < O; o += NT) {
    float s = 0.f;
    for (int g = 0; g < n; ++g) s += dl[g * O + o];
    float* dst = dWb + O * K + o;
    *dst = first ? s : *dst + s;
  }
  const float4* W4 = reinterpret_cast<const float4*>(a.W[I]);
  for (int idx = threadIdx.x; idx < n * K4; idx += NT) {
    const int g = idx / K4, k4 = idx - g * K4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int o = 0; o < O; ++o) {
      const float e = dl[g * O + o];
      const float4 w = W4[o * K4 + k4];
      s.x = fmaf(e, w.x, s.x); s.y = fmaf(e, w.y, s.y); s.z = fmaf(e, w.z, s.z); s.w = fmaf(e, w.w, s.w);
    }
    if constexpr (I == 0) {
      reinterpret_cast<float4*>(a.demb + (size_t)(g0 + g) * (2 * D))[k4] = s;
    } else {
      const float4 v = x4[g * K4 + k4];
      const float sl = a.slope;
      s = make_float4(s.x * hcg_leaky_grad(v.x, sl), s.y * hcg_leaky_grad(v.y, sl), s.z * hcg_leaky_grad(v.z, sl),
                      s.w * hcg_leaky_grad(v.w, sl));
      reinterpret_cast<float4*>(L.d[P ^ 1])[g * K4 + k4] = s;
    }
  }
}

template <int D, int R, int LOSS = LOSS_SQ, int I = 0>
__device__ __forceinline__ void forward(Lds<D, R>& L, const hcg_head_args& a, int n, int g0, float& sse) {
  fwd_layer<D, R, I, LOSS>(L, a, n, g0, sse);
  __syncthreads();
  if constexpr (I + 1 < R) forward<D, R, LOSS, I + 1>(L, a, n, g0, sse);
}

template <int D, int R, int LOSS = LOSS_SQ, int I = R - 1>
__device__ __forceinline__ void backward(Lds<D, R>& L, const hcg_head_args& a, int n, int g0, float* slab, bool first) {
  bwd_layer<D, R, I, (R - 1 - I) & 1, LOSS>(L, a, n, g0, slab, first);
  __syncthreads();
  if constexpr (I > 0) backward<D, R, LOSS, I - 1>(L, a, n, g0, slab, first);
}

template <int D, int R, bool BACKWARD, int LOSS = LOSS_SQ>
__global__ __launch_bounds__(NT, 1) void k_head_deep(const hcg_head_args a, int slab) {
  __shared__ Lds<D, R> L;
  if (a.step_counter && blockIdx.x == 0 && threadIdx.x == 0) { a.step_counter[0] += 1; a.step_counter[1] += 1; }
  float* slabs = static_cast<float*>(a.workspace);
  float* own = slabs + (size_t)blockIdx.x * slab;
  const int B = (int)a.B, tiles = (B + TG - 1) / TG;
  float sse = 0.f;
  bool first = true;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int g0 = t * TG, n = B - g0 < TG ? B - g0 : TG;
    const float4* e4 = reinterpret_cast<const float4*>(a.emb + (size_t)g0 * (2 * D));
    for (int idx = threadIdx.x; idx < n * (2 * D / 4); idx += NT) reinterpret_cast<float4*>(L.act)[idx] = e4[idx];
    __syncthreads();
    forward<D, R, LOSS>(L, a, n, g0, sse);
    if constexpr (BACKWARD) backward<D, R, LOSS>(L, a, n, g0, own, first);
    first = false;
  }
  // this workgroup's SSE partial: a fixed tree over the threads' fixed-order partials
  L.red[threadIdx.x] = sse;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) L.red[threadIdx.x] += L.red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) slabs[(size_t)gridDim.x * slab + blockIdx.x] = L.red[0];
}

}  // namespace deep
}  // namespace

static bool deep_supported(int64_t D, int64_t C, int64_t R) {
  return (D == 64 || D == 128) && C >= 1 && C <= RCMAX && (R == 1 || R == 3 || R == 4);
}

// workspace: [grid][slab] gradient slabs | [grid] SSE partials (hcg_general_workspace_bytes, HCG_WS_HEAD_DEEP)
size_t hcg_head_deep_workspace_bytes_impl(int64_t B, int64_t D, int64_t C, int64_t R) {
  if (B <= 0 || !deep_supported(D, C, R)) return 0;
  return hcg_align_up((size_t)head_grid_rt(B, deep::TG) * (deep::slab_floats((int)D, (int)R, (int)C) + 1) * sizeof(float), 256) + 256;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int hcg_head_deep_fwd_bwd(const hcg_head_args* args, hcg_reduce_job* job, hcg_stream_t stream) {
  if (!args) return HCG_ERR_INVALID_ARG;
  const hcg_head_args& a = *args;
  if (!deep_supported(a.D, a.C, a.R)) return HCG_ERR_UNSUPPORTED;
  if (a.flags & ~(HCG_HEAD_FORWARD_ONLY | HCG_HEAD_LOSS_CE)) return HCG_ERR_INVALID_ARG;
  const bool bwd = !(a.flags & HCG_HEAD_FORWARD_ONLY), ce = (a.flags & HCG_HEAD_LOSS_CE) != 0;
  if (ce && a.C < 2) return HCG_ERR_INVALID_ARG;
  if (a.B <= 0 || a.B * a.D * 2 > INT32_MAX || !a.emb || !a.y || !a.out || !a.workspace || !aligned16(a.emb)) return HCG_ERR_INVALID_ARG;
  if (bwd && (!a.demb || !aligned16(a.demb))) return HCG_ERR_INVALID_ARG;
  for (int i = 0; i < a.R; ++i)
    if (!a.W[i] || !a.b[i] || !aligned16(a.W[i]) || (a.grad[0] && !a.grad[i])) return HCG_ERR_INVALID_ARG;
  if (a.workspace_bytes < hcg_head_deep_workspace_bytes_impl(a.B, a.D, a.C, a.R)) return HCG_ERR_WORKSPACE;
  const int grid = head_grid_rt(a.B, deep::TG), slab = deep::slab_floats((int)a.D, (int)a.R, (int)a.C);
  if (job) {      // (the slabs this launch leaves, one segment per layer)
    job->slabs = (const float*)a.workspace;
    job->sse_part = (const float*)a.workspace + (size_t)grid * slab;
    job->nslabs = grid;
    job->slab_floats = slab;
    job->nseg = bwd && a.grad[0] ? a.R : 0;
    job->reserved = 0;
    for (int g = 0; g < HCG_REDUCE_MAX_SEGS; ++g) job->seg[g] = hcg_reduce_seg{0, 0, 1, 1, nullptr};
    for (int i = 0; i < job->nseg; ++i) {
      const int K = deep::kin((int)a.D, i), n = (i == a.R - 1 ? (int)a.C : K / 2) * (K + 1);
      job->seg[i] = hcg_reduce_seg{deep::seg_off((int)a.D, i), n, n, n, a.grad[i]};
    }
  }
#define LAUNCH_DEEP_(D_, R_, BW, LOSS_) \
  hipLaunchKernelGGL((deep::k_head_deep<D_, R_, BW, LOSS_>), dim3(grid), dim3(deep::NT), 0, (hipStream_t)stream, a, slab)
#define LAUNCH_DEEP(D_, R_)                                                                                             \
  do {                                                                                                                  \
    if (ce) { if (bwd) LAUNCH_DEEP_(D_, R_, true, LOSS_CE); else LAUNCH_DEEP_(D_, R_, false, LOSS_CE); }                \
    else if (bwd) LAUNCH_DEEP_(D_, R_, true, LOSS_SQ);                                                                  \
    else LAUNCH_DEEP_(D_, R_, false, LOSS_SQ);                                                                          \
  } while (0)
  if (a.D == 64) {
    if (a.R == 1) LAUNCH_DEEP(64, 1); else if (a.R == 3) LAUNCH_DEEP(64, 3); else LAUNCH_DEEP(64, 4);
  } else {
    if (a.R == 1) LAUNCH_DEEP(128, 1); else if (a.R == 3) LAUNCH_DEEP(128, 3); else LAUNCH_DEEP(128, 4);
  }
#undef LAUNCH_DEEP
#undef LAUNCH_DEEP_
  HCG_CHECK_LAUNCH();
  return HCG_OK;
}
