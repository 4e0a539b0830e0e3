// Host-side pieces shared by the conv launchers (fused.hip, mid.hip, wave.hip, tall.hip) and head.hip: the CU count, the
// dynamic-LDS limit, runtime choice -> template argument, the argument rules every family repeats, reduction-job fillers.
#pragma once
#include <type_traits>
#include <utility>
#include "common.h"

// CUs of the current device, asked once per process (also keeps the query out of a stream capture); 256 (an MI355X) when
// no device answers, so the workspace queries work on a machine without one
inline int hcg_cu_count() {
  static const int cus = [] {
    int dev = 0, v = 0;
    const bool ok = hipGetDevice(&dev) == hipSuccess &&
                    hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0;
    return ok ? v : 256;
  }();
  return cus;
}

// min(want, cap) workgroups, at least one
inline int hcg_grid(int64_t want, int64_t cap) {
  const int64_t g = want < cap ? want : cap;
  return g < 1 ? 1 : (int)g;
}

// columns of a weight-gradient slab row for an input width F <= 128, and the kernels' K padding: 32 or 64 (a wider F is
// contracted in chunks of 64, or refused by the family)
inline int hcg_fpad(int64_t F) { return F <= 32 ? 32 : (F <= 64 ? 64 : 128); }
inline int hcg_kpad(int64_t F) { return F <= 32 ? 32 : 64; }

// dynamic LDS above 64 KB has to be allowed per kernel: once per process (not per launch: the step may be under capture).
// The kernel is a template VALUE parameter: one static per instantiation, not per signature.
template <auto KFN>
hipError_t hcg_allow_lds(size_t bytes) {
  static const hipError_t st = hipFuncSetAttribute((const void*)KFN, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  return st;
}

// one launch: raise the kernel's dynamic-LDS limit to `lds_limit` (0: leave it), launch, report the launch's error
template <auto KFN, class... A>
int hcg_launch(dim3 grid, dim3 blk, size_t lds, size_t lds_limit, hipStream_t stream, A... args) {
  if (lds_limit) {
    const hipError_t e = hcg_allow_lds<KFN>(lds_limit);
    if (e != hipSuccess) return hcg_hip_err(e);
  }
  hipLaunchKernelGGL(KFN, grid, blk, lds, stream, args...);
  return hcg_hip_err(hipGetLastError());
}

// Runtime choice -> compile-time constant: fn(std::integral_constant<int, i>{}) for the i in [0, N) that was asked for.
// A launcher keeps a constexpr table of the forms it instantiates and dispatches the row index; the lambda returns the
// launch's code.
template <class Fn, int... I>
int hcg_with_index_impl(int i, Fn&& fn, std::integer_sequence<int, I...>) {
  int rc = HCG_ERR_INVALID_ARG;
  (void)((i == I ? (rc = fn(std::integral_constant<int, I>{}), true) : false) || ...);
  return rc;
}
template <int N, class Fn>
int hcg_with_index(int i, Fn&& fn) {
  return hcg_with_index_impl(i, fn, std::make_integer_sequence<int, N>{});
}
// ... and fn(c0, c1, ...) with every bool as std::true_type / std::false_type, for the choices that are a plain product
template <class Fn>
int hcg_with_bools(Fn&& fn) {
  return fn();
}
template <class Fn, class... Rest>
int hcg_with_bools(Fn&& fn, bool v, Rest... rest) {
  auto bound = [&](auto c) { return hcg_with_bools([&](auto... cs) { return fn(c, cs...); }, rest...); };
  return v ? bound(std::true_type{}) : bound(std::false_type{});
}

// The forward's forms on graphs of more than 64 nodes (mid.hip, tall.hip): plain, pooled ([max, mean] epilogue), pooled in
// the training's bit form (`out` is not written), first-layer training form (Ahat x and the sign pieces leave as well)
struct hcg_fwd_form_t { bool pool, bits, zs; };
constexpr hcg_fwd_form_t HCG_FWD_FORMS[4] = {{false, false, false}, {true, false, false}, {true, true, false}, {false, false, true}};
inline int hcg_fwd_form(const void* emb, const void* poolbits, const void* xagg) { return poolbits ? 2 : (xagg ? 3 : (emb ? 1 : 0)); }

// ---- argument rules shared by the families ---------------------------------------------------------------------
// a batch without edges still hands the kernels a readable edge_index (no graph has edges: nothing of it is used)
inline void hcg_edge_dummy(const int64_t*& edge_index, int64_t& E, const int32_t* graph_ptr) {
  if (E == 0) { edge_index = reinterpret_cast<const int64_t*>(graph_ptr); E = 1; }
}
// LeakyReLU is evaluated as max(v, slope*v)
inline bool hcg_slope_ok(int apply_act, float slope) { return !apply_act || (slope >= 0.f && slope <= 1.f); }
// whether a backward reads the forward's `out`: for the activation derivative and the pooled-gradient routing
inline bool hcg_bwd_reads_out(bool poolg, int apply_act) { return poolg || (apply_act & 1); }
// the backward's forms: pooled (upstream gradient demb, expanded with emb) needs both; apply_act is bit 0 (leaky'(out)) |
// bit 1 (dx handed down premasked, which needs a dx); `out` where hcg_bwd_reads_out
inline int hcg_bwd_form_check(bool poolg, bool have_demb, bool have_emb, int apply_act, bool have_dx, bool have_out) {
  if (poolg && (!have_demb || !have_emb)) return HCG_ERR_INVALID_ARG;
  if ((apply_act & ~3) || ((apply_act & 2) && !have_dx)) return HCG_ERR_INVALID_ARG;
  if (hcg_bwd_reads_out(poolg, apply_act) && !have_out) return HCG_ERR_INVALID_ARG;
  return HCG_OK;
}

// ---- reduction jobs ----------------------------------------------------------------------------------------------
// `nslabs` slabs of one segment: rows of `row_in` floats, the first `row_out` of each summed into dst
inline void hcg_fill_job(hcg_reduce_job* job, const float* slabs, int nslabs, int count, int row_in, int row_out, float* dst) {
  job->slabs = slabs;
  job->nslabs = nslabs;
  job->slab_floats = count;
  job->nseg = 1;
  job->sse_part = nullptr;
  job->reserved = 0;
  job->seg[0] = hcg_reduce_seg{0, count, row_in, row_out, dst};
}
// slabs of "dW [rows][fpad] | db [rows]" (the tiles, the one-graph-per-workgroup and the one-graph-per-wave kernels)
inline int hcg_dw_db_slab_floats(int rows, int fpad) { return rows * fpad + rows; }
inline void hcg_fill_job_dw_db(hcg_reduce_job* job, const float* slabs, int nslabs, int rows, int fpad, int64_t F, float* dW,
                               float* db) {
  hcg_fill_job(job, slabs, nslabs, rows * fpad, fpad, (int32_t)F, dW);
  job->slab_floats = hcg_dw_db_slab_floats(rows, fpad);
  job->nseg = 2;
  job->seg[1] = hcg_reduce_seg{rows * fpad, rows, 1, 1, db};
}
