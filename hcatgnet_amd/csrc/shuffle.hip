// An epoch's shuffle drawn on the device: numpy's `Generator(PCG64).permutation(G)` bit for bit, and the index arrays
// `store.epoch_layout` makes of it, as one launch of one workgroup in front of the epoch's collate (the contract is in
// include/hcatgnet_hip.h: hcg_epoch_draw_args).  With the permutation and the layout made on chip an epoch of a fit needs no
// host data -- no numpy draw, no index upload through pinned rows -- so a control interval of epochs is ONE captured graph
// (hcatgnet_amd/fit.py, form "chunk").  `store.pcg64_permutation` restates the draw in plain Python and is its CPU oracle.
// The swap chain of a Fisher-Yates shuffle is serial by nature (step i reads what step i + 1 wrote): one lane walks it with
// the array in LDS and the generator in registers; the layout behind it is parallel, a wave per batch.
#include "common.h"

namespace {

constexpr int DRAW_THREADS = 1024;
constexpr int DRAW_WAVES = DRAW_THREADS / HCG_WAVE;

typedef unsigned __int128 u128;

struct Pcg {
  u128 state, inc;
  uint32_t has_uint32, uinteger;
};

// pcg64: the 128-bit LCG steps, the output is XSL-RR of the NEW state
__device__ __forceinline__ uint64_t pcg_next64(Pcg& g) {
  const u128 mult = ((u128)0x2360ED051FC65DA4ull << 64) | (u128)0x4385DF649FCCF645ull;
  g.state = g.state * mult + g.inc;
  const uint64_t hi = (uint64_t)(g.state >> 64), lo = (uint64_t)g.state;
  const uint64_t x = hi ^ lo;
  const unsigned rot = (unsigned)(hi >> 58);                // state >> 122
  return (x >> rot) | (x << ((64u - rot) & 63u));
}

// numpy's buffered halves: the low word first, the high word kept for the next call
__device__ __forceinline__ uint32_t pcg_next32(Pcg& g) {
  if (g.has_uint32) {
    g.has_uint32 = 0;
    return g.uinteger;
  }
  const uint64_t w = pcg_next64(g);
  g.has_uint32 = 1;
  g.uinteger = (uint32_t)(w >> 32);
  return (uint32_t)w;
}

__global__ __launch_bounds__(DRAW_THREADS) void k_epoch_draw(hcg_epoch_draw_args a, const int64_t* __restrict__ node_ptr_all,
                                                             const int64_t* __restrict__ edge_ptr_all) {
  __shared__ int32_t s_perm[HCG_EPOCH_DRAW_MAX_GRAPHS];
  const int tid = threadIdx.x, G = (int)a.G;
  if (a.gate) {                                             // (a uniform address: the whole workgroup leaves or stays)
    const int32_t stopped = a.gate->stopped, epoch = a.gate->epoch;
    if (stopped || epoch < 0 || epoch >= a.gate_max_epochs) return;
  }
  for (int i = tid; i < G; i += DRAW_THREADS) s_perm[i] = i;
  __syncthreads();
  if (tid == 0 && G > 1) {
    Pcg g;
    g.state = ((u128)a.rng->state_hi << 64) | (u128)a.rng->state_lo;
    g.inc = ((u128)a.rng->inc_hi << 64) | (u128)a.rng->inc_lo;
    g.has_uint32 = a.rng->has_uint32;
    g.uinteger = a.rng->uinteger;
    for (uint32_t i = (uint32_t)G - 1; i >= 1; --i) {
      uint32_t mask = i;                                    // random_interval(i): the smallest 2^k - 1 >= i
      mask |= mask >> 1;
      mask |= mask >> 2;
      mask |= mask >> 4;
      mask |= mask >> 8;
      mask |= mask >> 16;
      uint32_t j;
      do {
        j = pcg_next32(g) & mask;
      } while (j > i);
      const int32_t t = s_perm[i];
      s_perm[i] = s_perm[j];
      s_perm[j] = t;
    }
    a.rng->state_lo = (uint64_t)g.state;
    a.rng->state_hi = (uint64_t)(g.state >> 64);
    a.rng->has_uint32 = g.has_uint32;
    a.rng->uinteger = g.uinteger;
  }
  __syncthreads();
  // the layout: ids | graph_ptr blocks | edge_ptr blocks.  Only the last batch can be short, so block b starts at b full blocks
  const int bs = a.batch_size, nfull = G / bs, rem = G % bs;
  const int nb = nfull + ((rem && !a.drop_last) ? 1 : 0);
  const int64_t W = ((int64_t)bs + 2) / 2;                  // int64 words of a full batch's block
  const int64_t tot = (int64_t)nfull * W + (nb > nfull ? (rem + 2) / 2 : 0);
  int64_t* __restrict__ ids = a.layout;
  int32_t* __restrict__ p32 = reinterpret_cast<int32_t*>(a.layout + G);
  for (int i = tid; i < G; i += DRAW_THREADS) ids[i] = s_perm[i];
  const int wave = tid / HCG_WAVE, lane = tid % HCG_WAVE;
  for (int b = wave; b < nb; b += DRAW_WAVES) {
    const int i0 = b * bs, B = b < nfull ? bs : rem;
    int32_t* __restrict__ gp = p32 + (int64_t)b * 2 * W;
    int32_t* __restrict__ ep = gp + 2 * tot;
    uint32_t carry_n = 0, carry_e = 0;                      // (unsigned: sums past 2^31 wrap as the host's int32 cast does)
    if (lane == 0) {
      gp[0] = 0;
      ep[0] = 0;
      if ((B & 1) == 0) {                                   // B + 1 pointers in B + 2 int32: the padding word
        gp[B + 1] = 0;
        ep[B + 1] = 0;
      }
    }
    for (int k0 = 0; k0 < B; k0 += HCG_WAVE) {
      const int k = k0 + lane;
      uint32_t n = 0, e = 0;
      if (k < B) {
        const int g = s_perm[i0 + k];
        n = (uint32_t)(node_ptr_all[g + 1] - node_ptr_all[g]);
        e = (uint32_t)(edge_ptr_all[g + 1] - edge_ptr_all[g]);
      }
      for (int d = 1; d < HCG_WAVE; d <<= 1) {              // inclusive scan over the wave
        const uint32_t un = __shfl_up(n, d, HCG_WAVE), ue = __shfl_up(e, d, HCG_WAVE);
        if (lane >= d) {
          n += un;
          e += ue;
        }
      }
      n += carry_n;
      e += carry_e;
      if (k < B) {
        gp[k + 1] = (int32_t)n;
        ep[k + 1] = (int32_t)e;
      }
      carry_n = __shfl(n, HCG_WAVE - 1, HCG_WAVE);
      carry_e = __shfl(e, HCG_WAVE - 1, HCG_WAVE);
    }
  }
}

}  // namespace

// reached through hcg_collate (collate.hip): `epoch_draw` of its argument struct
int hcg_epoch_draw_launch(const hcg_collate_args* c, hipStream_t stream) {
  const hcg_epoch_draw_args* d = c->epoch_draw;
  if (!c->node_ptr_all || !c->edge_ptr_all || !d->rng || !d->layout) return HCG_ERR_INVALID_ARG;
  if (d->G < 1 || d->batch_size < 1 || (d->drop_last != 0 && d->drop_last != 1) || d->reserved != 0) return HCG_ERR_INVALID_ARG;
  if (d->gate && d->gate_max_epochs < 1) return HCG_ERR_INVALID_ARG;
  if (((uintptr_t)d->rng | (uintptr_t)d->layout | (uintptr_t)d->gate | (uintptr_t)c->node_ptr_all | (uintptr_t)c->edge_ptr_all) %
      sizeof(int64_t))
    return HCG_ERR_INVALID_ARG;
  if (d->G > HCG_EPOCH_DRAW_MAX_GRAPHS) return HCG_ERR_UNSUPPORTED;
  hcg_epoch_draw_args a = *d;
  if ((int64_t)a.batch_size > a.G) a.batch_size = (int32_t)a.G + 1;      // (one short batch either way)
  hipLaunchKernelGGL(k_epoch_draw, dim3(1), dim3(DRAW_THREADS), 0, stream, a, c->node_ptr_all, c->edge_ptr_all);
  HCG_CHECK_LAUNCH();
  return HCG_OK;
}
