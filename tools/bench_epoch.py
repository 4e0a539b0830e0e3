#!/usr/bin/env python3
"""Dev tool: one training epoch as the reference runs it (scripts_experiments/train_GNN.py:73-80: 535 training graphs,
batch_size 40, shuffle; utils/utils_model.py:55-70) -- hcatgnet_amd.train.train_network over a DeviceLoader vs the CPU
oracle's loop on the same graphs.  Prints ms per epoch and graphs/s.  `--optimizer Adam | SGD | rmsprop`: the reference's
`--optimizer` (model/networks.py:36-44); the CPU oracle's loop is Adam's and runs only for Adam.  `--readout-layers` /
`--n-convolutions`: the reference's depth options (options/base_options.py:185-197); away from the defaults the per-batch
autograd loop such models took before the fused step covered them is timed too.  `--problem-type classification
--n-classes C`: the reference's `--problem_type` (model/networks.py:30-34) with labels drawn uniformly from 0 .. C-1 -- the
cross-entropy step (train.FusedTrainStep) -- with the same legs."""
import argparse, sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import hcatgnet_amd as H
from hcatgnet_amd import synth
from hcatgnet_amd import train as _train
from hcatgnet_amd.train import train_network, eval_network
from oracle import gcn_oracle
ap = argparse.ArgumentParser()
ap.add_argument("--optimizer", default="Adam", choices=["Adam", "SGD", "rmsprop"])
ap.add_argument("--readout-layers", type=int, default=2)
ap.add_argument("--n-convolutions", type=int, default=2)
ap.add_argument("--problem-type", default="regression", choices=["regression", "classification"])
ap.add_argument("--n-classes", type=int, default=None, help="classification: number of classes (default 3)")
args = ap.parse_args()
OPT = args.optimizer
CLS = args.problem_type == "classification"
if args.n_classes is not None and not CLS:
    ap.error("--n-classes goes with --problem-type classification")
DEPTH = dict(readout_layers=args.readout_layers, n_convolutions=args.n_convolutions)
DEFAULT_DEPTH = DEPTH == dict(readout_layers=2, n_convolutions=2) and not CLS     # (False: the autograd loop is timed too)
if CLS:
    DEPTH.update(problem_type="classification", n_classes=3 if args.n_classes is None else args.n_classes)
G, BS = 535, 40
sb = synth.make_config("REAL", num_graphs=G)
if CLS:
    sb.y = torch.randint(0, DEPTH["n_classes"], (G,), generator=torch.Generator().manual_seed(1)).float()
graphs = sb.as_graph_list()
store = H.DeviceGraphStore(graphs, device="cuda")
loader = H.DeviceLoader(store, batch_size=BS, shuffle=True, seed=0)
model = H.make_network("GCN", H.default_options(optimizer=OPT, **DEPTH), 25).cuda()
print(f"optimizer {OPT}: {type(model.optimizer).__name__}" + ("" if DEFAULT_DEPTH else f", {DEPTH}"))
import gc
for _ in range(3):
    train_network(model, loader, "cuda")
# set-up is over: everything alive now leaves the cyclic collector's sight -- a full collection of a process that holds torch,
# 15 trainers and a captured epoch takes ~85 ms and lands in whichever loop allocates most (the per-batch loop: it measured
# 7.9 ms/epoch instead of 2.3 with the collector walking those objects)
gc.collect(); gc.freeze()
torch.cuda.synchronize(); t0 = time.perf_counter()
EP = 20
for _ in range(EP):
    loss = train_network(model, loader, "cuda")
torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / EP
print(f"MI355X  train_network: {dt * 1e3:8.2f} ms/epoch ({len(loader)} batches of {BS}; {G / dt:10.0f} graphs/s), last epoch loss {loss:.4f}"
      f"  [whole epochs as one hipGraph: {_train.epoch_window_of(model, loader) is not None}]")
_train.EPOCH_WINDOW = False
loader_b = H.DeviceLoader(store, batch_size=BS, shuffle=True, seed=0)
model_b = H.make_network("GCN", H.default_options(optimizer=OPT, **DEPTH), 25).cuda()      # (its own model: the window's 14 trainers stay out of the way)
for _ in range(3):
    train_network(model_b, loader_b, "cuda")
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(EP):
    train_network(model_b, loader_b, "cuda")
torch.cuda.synchronize(); dtl = (time.perf_counter() - t0) / EP
_train.EPOCH_WINDOW = True
print(f"MI355X  train_network: {dtl * 1e3:8.2f} ms/epoch with the per-batch loop (round 2's form)")
if not DEFAULT_DEPTH:
    # the per-batch autograd loop: what train_network ran for such a model while the fused step refused it
    real_reason = _train.FusedTrainStep.reason
    _train.FusedTrainStep.reason = lambda self, batch=None: "timing the autograd loop"
    model_c = H.make_network("GCN", H.default_options(optimizer=OPT, **DEPTH), 25).cuda()
    for _ in range(3):
        train_network(model_c, loader_b, "cuda")
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(EP):
        train_network(model_c, loader_b, "cuda")
    torch.cuda.synchronize(); dta = (time.perf_counter() - t0) / EP
    _train.FusedTrainStep.reason = real_reason
    print(f"MI355X  train_network: {dta * 1e3:8.2f} ms/epoch with the per-batch autograd loop (the form before the fused step)")
t0 = time.perf_counter()
for _ in range(EP):
    eval_network(model, loader, "cuda")
torch.cuda.synchronize(); dte = (time.perf_counter() - t0) / EP
print(f"MI355X  eval_network : {dte * 1e3:8.2f} ms/epoch (shuffling loader: per-batch loop)")
vloader = H.DeviceLoader(store, batch_size=BS)          # the reference's validation / test loaders do not shuffle
for _ in range(3):
    eval_network(model, vloader, "cuda")
t0 = time.perf_counter()
for _ in range(EP):
    eval_network(model, vloader, "cuda")
torch.cuda.synchronize(); dtv = (time.perf_counter() - t0) / EP
print(f"MI355X  eval_network : {dtv * 1e3:8.2f} ms/epoch (fixed loader: batches collated once, one graph launch per call)")
if OPT != "Adam" or not DEFAULT_DEPTH:
    sys.exit(0)
# CPU: the oracle's loop with the host collate (what the reference does through PyG on the CPU)
torch.set_num_threads(min(16, os.cpu_count() or 1))
params = {k: v.detach().cpu().clone() for k, v in H.make_network("GCN", H.default_options(), 25).state_dict().items()}
p, opt = gcn_oracle.make_train_state(params)
cl = H.DataLoader(graphs, batch_size=BS, shuffle=True)
def cpu_epoch():
    for b in cl:
        gcn_oracle.train_step(p, opt, b.x, b.edge_index, b.batch, b.y, b.num_graphs)
cpu_epoch(); t0 = time.perf_counter()
for _ in range(3): cpu_epoch()
dtc = (time.perf_counter() - t0) / 3
print(f"CPU oracle loop ({torch.get_num_threads()} threads): {dtc * 1e3:8.2f} ms/epoch ({G / dtc:10.0f} graphs/s) -> x{dtc / dt:.1f}")
