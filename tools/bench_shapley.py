#!/usr/bin/env python3
"""Time Shapley value sampling of one frozen model on real-size graphs (52 and 535 of them) in ONE process, legs alternating:

  (a) the batch-synchronous loop (`ShapleySampling.loop`): one forward-only `ExplainStep` call of the whole batch per walk
      step.  It is long, so it runs `--loop-permutations` permutations (default 1) and is scaled per permutation.
  (b) the on-chip walk (`ShapleySampling`, csrc/shapley.hip), `--permutations` permutations (default 25, Captum's), default
      launch split.

The synthetic generator's node features are dense; the reference's are mostly one-hot (about 80 % of the entries of its
golden graphs are exactly 0), so `--nonzero-share` of the entries are kept (default 0.2) -- the record states the share of
walk steps that needed an evaluation.  Warm-up first; then `--windows` rounds of the legs, one call per window,
device-synchronised at both ends; a window's figure is its milliseconds per (graph, permutation); reported: median, p10,
p90 over the windows.  One JSON line on stdout (and `--out`).

    python tools/bench_shapley.py --out profiles/shapley_bench.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_shapley.py --profile-calls 3     # launches per kernel call
"""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import hcatgnet_amd as H  # noqa: E402
from hcatgnet_amd import synth  # noqa: E402
from hcatgnet_amd.shapley import ShapleySampling, draw_permutations  # noqa: E402

REAL = dict(nodes=120, extra_bonds=4, max_degree=4, feat=25, nodes_jitter=64)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(v):
    t = torch.tensor(sorted(v), dtype=torch.float64)
    q = lambda p: float(torch.quantile(t, p))
    return dict(median_ms=round(q(0.5), 5), p10_ms=round(q(0.1), 5), p90_ms=round(q(0.9), 5), windows=len(v))


def make_model():
    torch.manual_seed(0)
    m = H.make_network("GCN", H.default_options(), 25).cuda().eval()
    with torch.no_grad():
        for q in m.parameters():
            if q.dim() == 1:
                q.add_(0.05)
    return m


def make_batch(B, share):
    sb = synth.make_batch(num_graphs=B, **REAL)
    keep = torch.rand(sb.x.shape, generator=torch.Generator().manual_seed(5)) < share
    sb.x = (sb.x * keep).contiguous()
    return sb.as_batch("cuda")


def kernel_resources():
    """VGPRs of k_shapley_walk from tools/kres.py (needs hipcc); None when the compiler is not there."""
    try:
        out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kres.py"), os.path.join(REPO, "hcatgnet_amd", "csrc", "shapley.hip"),
                              "k_shapley_walk", "-fno-slp-vectorize"], capture_output=True, text=True, timeout=300).stdout
        m = re.search(r"vgpr\s+(\d+) agpr\s+(\d+) scratch\s+(\d+)", out)
        return dict(vgprs=int(m.group(1)), agprs=int(m.group(2)), scratch_bytes=int(m.group(3))) if m else None
    except Exception:
        return None


def commit_hash():
    try:
        r = subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True)
        return r.stdout.strip() or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--graphs", type=int, nargs="+", default=[52, 535])
    ap.add_argument("--permutations", type=int, default=25)
    ap.add_argument("--loop-permutations", type=int, default=1)
    ap.add_argument("--nonzero-share", type=float, default=0.2)
    ap.add_argument("--commit", default=None, help="commit hash for the record (default: git rev-parse HEAD)")
    ap.add_argument("--vgprs", type=int, default=None, help="VGPRs of k_shapley_walk (default: ask tools/kres.py)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-calls", type=int, default=0, help="only this many kernel calls on the first batch (for a kernel trace)")
    a = ap.parse_args()

    model = make_model()
    batches = {B: make_batch(B, a.nonzero_share) for B in a.graphs}

    if a.profile_calls:
        b = batches[a.graphs[0]]
        sv = ShapleySampling(model)
        perm = draw_permutations(b, 25, a.permutations, torch.Generator().manual_seed(1))
        torch.cuda.synchronize()
        launches = 0
        for _ in range(a.profile_calls):
            sv(b, permutations=perm)
            spl = sv.default_samples_per_launch(a.permutations, b.num_graphs, perm.shape[1], b.max_nodes * 25 + b.max_edges)
            launches += -(-a.permutations // spl)
        torch.cuda.synchronize()
        print(json.dumps(dict(profiled_kernel_calls=a.profile_calls, launches_of_each_kernel=launches, path=sv.last_path)))
        return

    cases = []
    for B in a.graphs:
        batch = batches[B]
        sv = ShapleySampling(model)
        assert sv.reason(batch) is None, sv.reason(batch)
        perm = draw_permutations(batch, 25, max(a.permutations, a.loop_permutations), torch.Generator().manual_seed(1))
        pa, pb = perm[:a.loop_permutations].contiguous(), perm[:a.permutations].contiguous()
        legs = {"a_loop": (lambda: sv.loop(batch, permutations=pa), a.loop_permutations),
                "b_kernel": (lambda: sv(batch, permutations=pb), a.permutations)}
        sv(batch, permutations=pb[:2].contiguous())           # warm-up: plan, buffers, the LDS attribute
        sv(batch, permutations=pb)
        assert sv.last_path == "fused"
        torch.cuda.synchronize()
        t = {k: [] for k in legs}
        for _ in range(a.windows):
            for k, (fn, P) in legs.items():
                t[k].append(1e3 * timed(fn) / (B * P))
        N, F = batch.x.shape
        E = int(batch.edge_index.shape[1])
        live = int((batch.edge_index[0] != batch.edge_index[1]).sum())
        evals = int((batch.x != 0).sum()) + live + B
        rec = dict(graphs=B, nodes=int(N), edges=E, max_nodes=int(batch.max_nodes), max_edges=int(batch.max_edges),
                   kernel_permutations=a.permutations, loop_permutations=a.loop_permutations,
                   samples_per_launch=sv.default_samples_per_launch(a.permutations, B, N * F + E, int(batch.max_nodes) * int(F) + int(batch.max_edges)),
                   walk_steps_per_permutation=int(N) * int(F) + E, evaluations_per_permutation=evals,
                   evaluated_share=round(evals / (int(N) * int(F) + E), 4),
                   lds_bytes=sv.lds_bytes(batch))
        rec.update({k + "_ms_per_graph_permutation": stats(v) for k, v in t.items()})
        rec["a_over_b_median"] = round(rec["a_loop_ms_per_graph_permutation"]["median_ms"] / rec["b_kernel_ms_per_graph_permutation"]["median_ms"], 2)
        rec["b_p90_below_a_p10"] = rec["b_kernel_ms_per_graph_permutation"]["p90_ms"] < rec["a_loop_ms_per_graph_permutation"]["p10_ms"]
        cases.append(rec)
        print(json.dumps(rec), file=sys.stderr)
    res = dict(vgprs=a.vgprs) if a.vgprs is not None else kernel_resources()
    out = dict(bench="shapley", device=torch.cuda.get_device_name(0), commit=a.commit or commit_hash(), graph_shape=REAL,
               nonzero_share=a.nonzero_share, kernel="k_shapley_walk", kernel_resources=res, cases=cases,
               note="one window = one call; (a) the batch-synchronous loop on forward-only ExplainStep, scaled per permutation; "
                    "(b) the on-chip walk plus its ordered reduce, default launch split; evaluations_per_permutation is DERIVED on "
                    "the host (non-zero entries of x + edges that are no self loop + one base evaluation per graph; the synthetic "
                    "batches have no ungrouped edges), not counted by the kernel")
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
