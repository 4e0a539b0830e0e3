#!/usr/bin/env python3
"""Time grouped Shapley value sampling (atoms, bonds, fragments as players) against today's per-entry call on real-size
graphs (52 and 535 of them) in ONE process, legs alternating, `--permutations` permutations each (default 25, Captum's):

  (a) the per-entry call (`ShapleySampling` without groups): every node-feature entry and every directed edge a player.
  (b) atoms plus bonds: `atom_groups` + `bond_groups` numbered after the atoms.
  (c) atoms, every edge in the background.
  (d) three fragments (contiguous node ranges), edges in the background, walked EXACTLY: all 3! = 6 orders.
  (p) optional, `--parent-lib PATH`: leg (a) on the library built from the parent commit, loaded into this process beside
      this build's (the ungrouped Python path is the same code) -- the ungrouped kernel is expected level with it.

Protocol of tools/bench_shapley.py: warm-up first; then `--windows` rounds of the legs, one call per window,
device-synchronised at both ends; a window's figure is its milliseconds per (graph, permutation); reported: median, p10,
p90 over the windows.  Next to each time: the evaluations per (graph, permutation) DERIVED on the host from the shapes
(live players + the base evaluation), not counted by the kernel.  One JSON line on stdout (and `--out`).

    python tools/bench_shapley_groups.py --out profiles/shapley_groups_bench.json
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import hcatgnet_amd as H  # noqa: E402
from hcatgnet_amd import _lib  # noqa: E402
from hcatgnet_amd._groups import _group_layout  # noqa: E402
from hcatgnet_amd.shapley import (GROUPED_WORKGROUPS_PER_CU, ShapleySampling, all_group_permutations, atom_groups, bond_groups,  # noqa: E402
                                  draw_group_permutations, draw_permutations)
from tools.bench_shapley import commit_hash, make_batch, make_model, stats, timed, REAL  # noqa: E402


def load_other(path):
    """A second build of the library in this process, with the signatures of this one."""
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


class use_lib:
    """Calls inside run on `lib` instead of this build's library."""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        self.mine, _lib._lib = _lib.load(), self.lib

    def __exit__(self, *exc):
        _lib._lib = self.mine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--graphs", type=int, nargs="+", default=[52, 535])
    ap.add_argument("--permutations", type=int, default=25)
    ap.add_argument("--nonzero-share", type=float, default=0.2)
    ap.add_argument("--commit", default=None, help="commit hash for the record (default: git rev-parse HEAD)")
    ap.add_argument("--parent-lib", default=None, help="libhcatgnet_hip.so built from the parent commit: adds leg (p)")
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    model = make_model()
    parent = load_other(a.parent_lib) if a.parent_lib else None
    cases = []
    for B in a.graphs:
        batch = make_batch(B, a.nonzero_share)
        N, F = batch.x.shape
        E = int(batch.edge_index.shape[1])
        n = torch.bincount(batch.batch, minlength=B)
        ag = atom_groups(batch)
        bg = bond_groups(batch, first=n)
        frag = ag * 3 // n[batch.batch]
        gen = lambda: torch.Generator().manual_seed(1)
        P = a.permutations
        perm_a = draw_permutations(batch, int(F), P, gen())
        perm_b = draw_group_permutations(batch, ag, bg, P, gen())
        perm_c = draw_group_permutations(batch, ag, None, P, gen())
        perm_d = all_group_permutations(batch, frag, None)
        sv = {k: ShapleySampling(model) for k in "abcdp"}
        legs = {"a_entries": (lambda: sv["a"](batch, permutations=perm_a), P),
                "b_atoms_bonds": (lambda: sv["b"](batch, group_permutations=perm_b, node_group=ag, edge_group=bg), P),
                "c_atoms": (lambda: sv["c"](batch, group_permutations=perm_c, node_group=ag), P),
                "d_fragments_exact": (lambda: sv["d"](batch, group_permutations=perm_d, node_group=frag), int(perm_d.shape[0]))}
        if parent is not None:
            def on_parent():
                with use_lib(parent):
                    sv["p"](batch, permutations=perm_a)
            legs["p_entries_parent"] = (on_parent, P)
        for k, (fn, _) in legs.items():                  # warm-up: plan, buffers, the LDS attribute of either kernel
            fn()
            fn()
        assert all(sv[k].last_path == "fused" for k in "abcd")
        torch.cuda.synchronize()
        t = {k: [] for k in legs}
        for _ in range(a.windows):
            for k, (fn, Pk) in legs.items():
                t[k].append(1e3 * timed(fn) / (B * Pk))
        # evaluations per (graph, permutation), derived on the host: live players + the base
        live_edges = int((batch.edge_index[0] != batch.edge_index[1]).sum())
        evals = {"a_entries": (int((batch.x != 0).sum()) + live_edges + B) / B,
                 "b_atoms_bonds": (int(_group_layout(batch, int(F), ag, bg).live_group.sum()) + B) / B,
                 "c_atoms": (int(_group_layout(batch, int(F), ag, None).live_group.sum()) + B) / B,
                 "d_fragments_exact": (int(_group_layout(batch, int(F), frag, None).live_group.sum()) + B) / B}
        if parent is not None:
            evals["p_entries_parent"] = evals["a_entries"]
        rec = dict(graphs=B, nodes=int(N), edges=E, max_nodes=int(batch.max_nodes), max_edges=int(batch.max_edges),
                   permutations=P, fragment_orders=int(perm_d.shape[0]), lds_bytes=sv["a"].lds_bytes(batch),
                   samples_per_launch=dict(
                       a_entries=ShapleySampling.default_samples_per_launch(P, B, int(N) * int(F) + E, int(batch.max_nodes) * int(F) + int(batch.max_edges)),
                       **{k: ShapleySampling.default_samples_per_launch(int(q.shape[0]), B, int(q.shape[1]), int(_group_layout(batch, int(F), ng_, eg_).max_groups),
                                                                        GROUPED_WORKGROUPS_PER_CU)
                          for k, q, ng_, eg_ in (("b_atoms_bonds", perm_b, ag, bg), ("c_atoms", perm_c, ag, None), ("d_fragments_exact", perm_d, frag, None))}),
                   groups=dict(b_atoms_bonds=int(perm_b.shape[1]), c_atoms=int(perm_c.shape[1]), d_fragments_exact=int(perm_d.shape[1])))
        med = {}
        for k, v in t.items():
            s = stats(v)
            s["evaluations_per_graph_permutation"] = round(evals[k], 2)
            s["wall_us_per_evaluation"] = round(1e3 * s["median_ms"] / evals[k], 3)     # (of the whole grid, not of one workgroup)
            rec[k + "_ms_per_graph_permutation"] = s
            med[k] = s["median_ms"]
        for k in ("b_atoms_bonds", "c_atoms", "d_fragments_exact"):
            time_ratio, eval_ratio = med[k] / med["a_entries"], evals[k] / evals["a_entries"]
            rec[k + "_over_a"] = dict(time=round(time_ratio, 4), evaluations=round(eval_ratio, 4),
                                      time_over_evaluations=round(time_ratio / eval_ratio, 3))
        # (b) / (a) and (c) / (a) "track" the counts when the time ratio is within 25 % of the evaluation ratio
        rec["b_and_c_track_the_evaluation_counts"] = all(0.75 <= rec[k + "_over_a"]["time_over_evaluations"] <= 1.25
                                                         for k in ("b_atoms_bonds", "c_atoms"))
        if parent is not None:
            sa, sp = rec["a_entries_ms_per_graph_permutation"], rec["p_entries_parent_ms_per_graph_permutation"]
            lo, hi = min(sa["p10_ms"], sp["p10_ms"]), max(sa["p90_ms"], sp["p90_ms"])
            rec["a_vs_parent"] = dict(median_ratio=round(sa["median_ms"] / sp["median_ms"], 4),
                                      both_medians_inside_the_joint_p10_p90=lo <= sa["median_ms"] <= hi and lo <= sp["median_ms"] <= hi,
                                      spreads_overlap=sa["p10_ms"] <= sp["p90_ms"] and sp["p10_ms"] <= sa["p90_ms"])
        cases.append(rec)
        print(json.dumps(rec), file=sys.stderr)
    out = dict(bench="shapley_groups", device=torch.cuda.get_device_name(0), commit=a.commit or commit_hash(),
               parent_commit=a.parent_commit, graph_shape=REAL, nonzero_share=a.nonzero_share, kernel="k_shapley_walk", cases=cases,
               note="one window = one call, host work of the call (group lists: one sort per call) included; ms per (graph, "
                    "permutation); evaluations_per_graph_permutation is DERIVED on the host (live players + one base "
                    "evaluation), not counted by the kernel; (d) runs 6 orders, not `permutations`; not measured: the apply "
                    "step alone, the limit shapes (184 nodes, 1024 edges), more than two conv layers")
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
