// gcn_norm on chip for the per-graph kernel families (mid.hip: one graph per workgroup, wave.hip: one graph per wave,
// tall.hip: the wide-layer route).  Each family rebuilds its graph's normalised adjacency in LDS from the raw COO edges
// with its own thread map and barriers; the rules those builds share live here, once (DESIGN a3):
//   * a graph whose host metadata does not fit the kernel is refused and reported (HCG_STATUS_SHAPE_LIMIT);
//   * dinv = (1 + in-degree)^-1/2;
//   * every CSR row is sorted by id, so the per-node summation order is fixed whatever order the LDS atomics ran in.
// Every piece takes compile-time shape constants and plain arguments only; all of it is inlined into the callers.  A piece
// is shared only where the callers' instructions stay what they were: the edge pass (local ids, (i, i) edges collapsing
// into the unit self loop, HCG_STATUS_EDGE_UNGROUPED) stays in each family's build, and tall.hip's seg_graph keeps its own
// refusal -- as shared code both changed the register allocation of the kernels around them.
#pragma once
#include "common.h"

namespace {

// Host metadata that does not fit the kernel (n outside [0, nmax], ne outside [0, emax]): the graph is refused (n = ne = 0)
// and reported by the thread with t == 0 (t: the thread's index in the graph's workgroup or wave).  The selects stay OUTSIDE
// the reporting thread's branch: assigned inside it, n and ne became per-lane registers and every address derived from them
// a 64-bit vector computation.
__device__ __forceinline__ void graph_refuse(int& n, int& ne, int nmax, int emax, int t, int32_t* status) {
  const bool bad = n < 0 || n > nmax || ne < 0 || ne > emax;
  n = __builtin_amdgcn_readfirstlane(bad ? 0 : n);
  ne = __builtin_amdgcn_readfirstlane(bad ? 0 : ne);
  if (bad && t == 0) atomicOr(status, HCG_STATUS_SHAPE_LIMIT);
}

// A graph's raw edges, EPT per thread (edge t + j * STRIDE in slot j), requested one graph AHEAD of their use: loads only,
// unconditional, clamped index (E >= 1 and `ei` readable are guaranteed by the host wrappers).  Uniform bases + one unsigned
// 32-bit byte offset per slot = the scalar-base form of global_load; the clamps of the graph's edge range are scalar work.
// (The kernels are bound by VALU issue: per-slot 64-bit index arithmetic counts.)
template <int EPT, int STRIDE>
struct EdgeRegs {
  long long s[EPT], d[EPT];
  template <class G>
  __device__ __forceinline__ void load(const G& gi, const int64_t* __restrict__ ei, int64_t E, int t) {
    long long eb = gi.ebase;
    eb = eb < 0 ? 0 : (eb > E - 1 ? E - 1 : eb);
    const long long room = E - eb;
    const int nec = (long long)gi.ne < room ? gi.ne : (int)room;
    const int last = nec > 0 ? nec - 1 : 0;
    const char* sb = reinterpret_cast<const char*>(ei + eb);
    const char* db = reinterpret_cast<const char*>(ei + E + eb);
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
      const int e = t + j * STRIDE;
      const unsigned off = 8u * (unsigned)(e < last ? e : last);
      s[j] = *reinterpret_cast<const long long*>(sb + off);
      d[j] = *reinterpret_cast<const long long*>(db + off);
    }
  }
};

__device__ __forceinline__ float gcn_dinv(int degin) { return 1.0f / sqrtf(1.0f + (float)degin); }

// exclusive scan of the row sizes cnt[0 .. nrows) into rowptr[0 .. nrows] by ONE wave, RPL rows per lane (t = lane of the
// scanning wave, nrows <= 64 RPL)
template <int RPL>
__device__ __forceinline__ void csr_scan_rows(const int* cnt, int* rowptr, int nrows, int t) {
  int v[RPL], tot = 0;
#pragma unroll
  for (int j = 0; j < RPL; ++j) {
    const int i = t * RPL + j;
    v[j] = i < nrows ? cnt[i] : 0;
    tot += v[j];
  }
  int incl = tot;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int x = __shfl_up(incl, off, 64);
    if (t >= off) incl += x;
  }
  int run = incl - tot;
#pragma unroll
  for (int j = 0; j < RPL; ++j) {
    const int i = t * RPL + j;
    if (i < nrows) rowptr[i] = run;
    run += v[j];
  }
  if (t == 63) rowptr[nrows] = incl;
}

// four values in ascending order: a sorting network.  (By value: sorting the caller's variables through references changed
// the register allocation of the mid.hip kernels.)
struct Sorted4 { unsigned a0, a1, a2, a3; };
__device__ __forceinline__ Sorted4 sort4(unsigned a0, unsigned a1, unsigned a2, unsigned a3) {
  unsigned t;
  t = min(a0, a1); a1 = max(a0, a1); a0 = t;
  t = min(a2, a3); a3 = max(a2, a3); a2 = t;
  t = min(a0, a2); a2 = max(a0, a2); a0 = t;
  t = min(a1, a3); a3 = max(a1, a3); a1 = t;
  t = min(a1, a2); a2 = max(a1, a2); a1 = t;
  return {a0, a1, a2, a3};
}

// col[kb .. ke) sorted by id.  Rows of <= 4 entries (every row of a molecular graph) through the register network: no
// dependent LDS chain; longer ones by insertion.
__device__ __forceinline__ void csr_sort_row(unsigned short* col, int kb, int ke) {
  const int len = ke - kb;
  if (len > 1 && len <= 4) {
    const Sorted4 o = sort4(col[kb], col[kb + 1], len > 2 ? col[kb + 2] : 0xffffu, len > 3 ? col[kb + 3] : 0xffffu);
    col[kb] = (unsigned short)o.a0;
    col[kb + 1] = (unsigned short)o.a1;
    if (len > 2) col[kb + 2] = (unsigned short)o.a2;
    if (len > 3) col[kb + 3] = (unsigned short)o.a3;
  } else if (len > 4) {
    for (int a = kb + 1; a < ke; ++a) {
      const unsigned short key = col[a];
      int b = a - 1;
      while (b >= kb && col[b] > key) { col[b + 1] = col[b]; --b; }
      col[b + 1] = key;
    }
  }
}

// acc = t[row] + sum_{k in [kb, ke)} t[col[k]] for this lane's (row, 4 c4 .. 4 c4 + 3) slot of a tile with row stride TS:
// the first four neighbours' rows are requested together (independent LDS reads instead of a chain of dependent ones),
// longer rows loop on
__device__ __forceinline__ void f4_add(float4& a, const float4 v) { a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }

template <int TS>
__device__ __forceinline__ float4 csr_row_sum(const float* t, const unsigned short* col, int row, int kb, int ke, int c4) {
  float4 acc = *reinterpret_cast<const float4*>(t + row * TS + 4 * c4);
  int c[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) c[j] = kb + j < ke ? col[kb + j] : row;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float4 v = *reinterpret_cast<const float4*>(t + c[j] * TS + 4 * c4);
    if (kb + j < ke) f4_add(acc, v);
  }
  for (int k = kb + 4; __any(k < ke); ++k) {
    if (k < ke) f4_add(acc, *reinterpret_cast<const float4*>(t + col[k] * TS + 4 * c4));
  }
  return acc;
}

}  // namespace
