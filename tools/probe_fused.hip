// Dev probe (not product): the two-layer conv backward pair (k_fused_bwd_pair, mode HCG_FUSED_BWD_PAIR of hcg_fused_forward)
// on the C3 shape -- 4096 graphs x 30 atoms x 64 directed edges, F = D = 64, the training form (poolbits) -- beside the two
// single launches, and with -DHCG_STAMP -DHCG_STAMP_BWD the s_memtime stamps of the first workgroup's waves around the
// boundary between the two phases.  Build (stamps):
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -fno-slp-vectorize -DHCG_STAMP -DHCG_STAMP_BWD -o tools/probe_fused tools/probe_fused.hip
// Read the stamp build's SHARES, not its length: its fences forbid overlaps the product kernel has.
#include "../hcatgnet_amd/csrc/fused.hip"
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)
#define RC(x) do { int e = (x); if (e != HCG_OK) { printf("hcg error %d at %d\n", e, __LINE__); return 1; } } while (0)

template <class T>
static T* upload(const std::vector<T>& v) {
  T* d = nullptr;
  if (hipMalloc(&d, v.size() * sizeof(T)) != hipSuccess) return nullptr;
  if (hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
  return d;
}

int main() {
  const int B = 4096, n = 30, F = 64, D = 64, N = B * n;
  std::mt19937 rng(1);
  auto rnd = [&](size_t k, float s) { std::vector<float> v(k); for (auto& f : v) f = s * ((float)(rng() % 2000) / 1000.f - 1.f); return v; };
  std::vector<int> gp(B + 1), ep(B + 1);
  std::vector<long long> src, dst;
  for (int g = 0; g < B; ++g) {   // ring + 2 chords per graph: 32 bonds -> 64 directed edges
    gp[g] = g * n; ep[g] = (int)src.size();
    auto bond = [&](int i, int j) { src.push_back(g * n + i); dst.push_back(g * n + j); src.push_back(g * n + j); dst.push_back(g * n + i); };
    for (int i = 0; i < n; ++i) bond(i, (i + 1) % n);
    bond(0, 15); bond(7, 22);
  }
  gp[B] = N; ep[B] = (int)src.size();
  const int E = (int)src.size();
  std::vector<long long> ei(2 * (size_t)E);
  for (int e = 0; e < E; ++e) { ei[e] = src[e]; ei[E + e] = dst[e]; }
  const size_t bits_bytes = hcg_fused_aux_bytes(HCG_FUSED_POOLBITS, B, 1);
  std::vector<uint32_t> bits(bits_bytes / 4);
  for (auto& w : bits) w = (uint32_t)rng();
  float *x = upload(rnd((size_t)N * F, 1.f)), *out1 = upload(rnd((size_t)N * D, 1.f)), *W1 = upload(rnd(D * F, 0.125f)),
        *W2 = upload(rnd(D * D, 0.125f)), *demb = upload(rnd((size_t)B * 2 * D, 1.f));
  long long* dei = upload(ei);
  int *dgp = upload(gp), *dep = upload(ep);
  uint32_t* dbits = upload(bits);
  if (!x || !out1 || !W1 || !W2 || !demb || !dei || !dgp || !dep || !dbits) { printf("upload failed\n"); return 1; }
  const size_t wsb = hcg_fused_workspace_bytes(B, F, D, 1);
  float *ddx; void *ws1, *ws0; int* dstatus;
  CK(hipMalloc(&ddx, (size_t)N * D * 4)); CK(hipMalloc(&ws1, wsb)); CK(hipMalloc(&ws0, wsb)); CK(hipMalloc(&dstatus, 16));
  CK(hipMemset(dstatus, 0, 16));
  printf("N %d E %d\n", N, E);

  hcg_fused_fwd_args a{};
  a.mode = HCG_FUSED_BWD_PAIR;
  a.x = x; a.W1 = W1; a.out1 = out1; a.W2 = W2;
  a.edge_index = (const int64_t*)dei; a.E = E; a.graph_ptr = dgp; a.edge_ptr = dep;
  a.N = N; a.B = B; a.F = F; a.D = D; a.graphs_per_tile = 1; a.pair_graphs_per_tile_upper = 1; a.slope = 0.01f;
  a.demb = demb; a.poolbits = dbits; a.status = dstatus;
  a.pair_dx = ddx; a.pair_ws_upper = ws1; a.pair_ws_upper_bytes = wsb; a.pair_ws_lower = ws0; a.pair_ws_lower_bytes = wsb;
  a.pair_act_upper = 3; a.pair_act_lower = 0;

  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  float ms;
  for (int it = 0; it < 55; ++it) {
    if (it == 5) { CK(hipDeviceSynchronize()); CK(hipEventRecord(e0, 0)); }
    RC(hcg_fused_layer_bwd(nullptr, demb, nullptr, nullptr, dbits, out1, W2, (const int64_t*)dei, E, dgp, dep, N, B, D, D, 1, 0.01f, 3,
                           ddx, dstatus, ws1, wsb, 0));
    RC(hcg_fused_layer_bwd(ddx, nullptr, nullptr, nullptr, nullptr, x, W1, (const int64_t*)dei, E, dgp, dep, N, B, F, D, 1, 0.01f, 0,
                           nullptr, dstatus, ws0, wsb, 0));
  }
  CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1));
  printf("two launches: %.2f us per pair of launches\n", ms * 1000.f / 50);
#ifdef HCG_STAMP
  unsigned long long* dstamp;
  const size_t nst = 4 * WAVES * 128;
  CK(hipMalloc(&dstamp, nst * 8)); CK(hipMemset(dstamp, 0, nst * 8));
#endif
  for (int it = 0; it < 55; ++it) {
    if (it == 5) { CK(hipDeviceSynchronize()); CK(hipEventRecord(e0, 0)); }
    RC(hcg_fused_forward(&a, 0));
  }
  CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1));
  printf("pair: %.2f us per launch\n", ms * 1000.f / 50);
  int status[4]; CK(hipMemcpy(status, dstatus, 16, hipMemcpyDeviceToHost)); printf("status %d\n", status[0]);
#if defined(HCG_STAMP) && defined(HCG_STAMP_BWD)
  // one more launch, alone on the device, with the stamp buffer set: its stamps are the ones printed
  CK(hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_buf), &dstamp, sizeof(dstamp)));
  RC(hcg_fused_forward(&a, 0));
  CK(hipDeviceSynchronize());
  std::vector<unsigned long long> sb(nst);
  CK(hipMemcpy(sb.data(), dstamp, nst * 8, hipMemcpyDeviceToHost));
  // A = upper layer (stamps 0..63), B = lower layer (64..127); cycles since the workgroup's first stamp
  const int idx[] = {0, 60, 61, 62, 63, 64 + 56, 64 + 0, 64 + 1, 64 + 2, 64 + 3, 64 + 60, 64 + 61, 64 + 63};
  const char* nm[] = {"A.loop", "A.loop-end", "A.loop-barrier", "A.combined", "A.slab", "barrier", "B.begin-issued", "B.count-built",
                      "B.first-MFMA", "B.agg-done", "B.loop-end", "B.loop-barrier", "B.slab"};
  for (int wg = 0; wg < 2; ++wg) {
    const unsigned long long* s0 = sb.data() + (size_t)wg * WAVES * 128;
    unsigned long long base = ~0ull;
    int early = 0, late = 0;
    for (int w = 0; w < WAVES; ++w) {
      base = std::min(base, s0[w * 128]);
      if (s0[w * 128 + 60] < s0[early * 128 + 60]) early = w;
      if (s0[w * 128 + 60] > s0[late * 128 + 60]) late = w;
    }
    printf("workgroup %d: early wave %d, late wave %d (by the end of the upper layer's tile loop)\n", wg, early, late);
    printf("  %-14s", "stamp");
    for (int w = 0; w < WAVES; ++w) printf(" %8s%d", "wave", w);
    printf("\n");
    for (size_t k = 0; k < sizeof(idx) / sizeof(idx[0]); ++k) {
      printf("  %-14s", nm[k]);
      for (int w = 0; w < WAVES; ++w) printf(" %9llu", s0[w * 128 + idx[k]] - base);
      printf("\n");
    }
    // SIMD partners w and w + 4: how much later the younger one leaves each tile loop
    for (int ph = 0; ph < 2; ++ph) {
      printf("  %s partner skew (wave w+4 - wave w) ", ph ? "B.loop-end" : "A.loop-end");
      for (int w = 0; w < WAVES / 2; ++w)
        printf(" %9lld", (long long)s0[(w + 4) * 128 + 64 * ph + 60] - (long long)s0[w * 128 + 64 * ph + 60]);
      printf("\n");
    }
  }
#endif
  return 0;
}
