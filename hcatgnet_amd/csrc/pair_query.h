// Where the two-layer backward pair (mode HCG_FUSED_BWD_PAIR of hcg_fused_forward, fused.hip: k_fused_bwd_pair) applies.
// Host code only, no HIP in it: fused.hip answers its query with this function, and tests/test_host_bwd_pair_boundary.py
// compiles it alone, with and without -DHCG_NO_BWD_PAIR, to hold the answers of both builds without a GPU.
#pragma once
#include <stdint.h>

#include "../../include/hcatgnet_hip.h"

// HCG_OK: the pair may be launched for this block (the launch form still checks its workspaces); otherwise the code of
// include/hcatgnet_hip.h.  `dd` = the width the small-graph tiles are built for.
static inline int hcg_bwd_pair_applies(const hcg_fused_fwd_args* a, int64_t dd) {
  const int64_t N = a->N, B = a->B, F = a->F, D = a->D;
  const int gpt = a->graphs_per_tile;
  if (a->pair_flags & ~HCG_FUSED_PAIR_QUERY) return HCG_ERR_INVALID_ARG;
  if ((a->pair_act_upper & ~3) || (a->pair_act_lower & ~3)) return HCG_ERR_INVALID_ARG;
  if (N < 0 || B < 0 || a->E < 0) return HCG_ERR_INVALID_ARG;
#ifdef HCG_NO_BWD_PAIR
  return HCG_ERR_UNSUPPORTED;      // (A/B builds: the caller then issues the two single launches)
#endif
  // both layers on the small-graph tiles over the same tiles, the upper layer hands dx down premasked, so the lower one
  // runs with its activation bits clear
  if (D != dd || F < 1 || F > 64 || gpt < 1 || a->pair_graphs_per_tile_upper != gpt) return HCG_ERR_UNSUPPORTED;
  if (!(a->pair_act_upper & 2) || a->pair_act_lower != 0 || !a->pair_dx) return HCG_ERR_UNSUPPORTED;
  if ((uintptr_t)a->out1 % 16 != 0 || (uintptr_t)a->pair_dx % 16 != 0) return HCG_ERR_UNSUPPORTED;   // wide rows of the D-wide tensors
  const bool bits = a->poolbits != nullptr;
  const bool poolg = bits || a->pair_dout == nullptr;
  if (bits && (a->pair_dout || a->emb || a->out2)) return HCG_ERR_INVALID_ARG;
  if (poolg && (!a->demb || (!bits && (!a->emb || !a->out2)))) return HCG_ERR_INVALID_ARG;
  if (!poolg && (a->pair_act_upper & 1) && !a->out2) return HCG_ERR_INVALID_ARG;
  if (!a->x || !a->W1 || !a->W2 || !a->out1 || !a->graph_ptr || !a->edge_ptr || !a->status || (a->E > 0 && !a->edge_index))
    return HCG_ERR_INVALID_ARG;
  return HCG_OK;
}
