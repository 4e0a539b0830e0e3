#!/usr/bin/env python3
"""Dev tool: where does the HOST time of one eager step go (cProfile over 300 steps)?

    host_profile.py [CONFIG [key=value ...]]      the synth config (default C2) and keywords of `synth.make_config`, e.g. the
                                                  size-grouped ragged batch: host_profile.py C3 nodes_jitter=6 group_by_size=True
"""
import ast, cProfile, pstats, sys, os, io, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, hcatgnet_amd as H
from hcatgnet_amd import synth, _lib
if os.environ.get("HCG_LIB"):          # a library variant (A/B runs on one box)
    _lib.LIB_PATH = os.path.abspath(os.environ["HCG_LIB"])
cfg, kw = (sys.argv[1:2] or ["C2"])[0], {k: ast.literal_eval(v) for k, v in (a.split("=", 1) for a in sys.argv[2:])}
sb = synth.make_config(cfg, **kw); m = H.make_network("GCN", H.default_options(), sb.x.shape[1]).cuda()
print(f"config {cfg} {kw}: {sb.num_graphs} graphs, {sb.x.shape[0]} nodes, largest {sb.max_nodes}, n_small {sb.n_small}")
x, ei, bv, y = sb.x.cuda(), sb.edge_index.cuda(), sb.batch.cuda(), sb.y.cuda(); y2 = y.unsqueeze(1)
from hcatgnet_amd.train import FusedTrainStep
trainer = FusedTrainStep(m)
def step():      # the product's training step (no autograd)
    trainer(H.Batch(x, ei, bv, sb.num_graphs, y=y, max_nodes=sb.max_nodes, max_edges=sb.max_edges, edges_grouped=True,
                    n_small=sb.n_small))
for _ in range(20): step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(300): step()
t1 = time.perf_counter(); torch.cuda.synchronize(); t2 = time.perf_counter()
print(f"host issue time {1e3*(t1-t0)/300:.3f} ms/step, +drain {1e3*(t2-t0)/300:.3f} ms/step")
pr = cProfile.Profile(); pr.enable()
for _ in range(300): step()
pr.disable(); torch.cuda.synchronize()
s = io.StringIO(); pstats.Stats(pr, stream=s).sort_stats("tottime").print_stats(22); print(s.getvalue()[:4500])
