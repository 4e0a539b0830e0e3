"""The reference's per-batch loops on MI355X (reference utils/utils_model.py:55-111).

`train_network` / `eval_network` / `predict_network` keep the reference's names, arguments and return
values; what changes is how a step is issued:

  reference step (utils/utils_model.py:60-68)          here (`FusedTrainStep`)
  -------------------------------------------          ---------------------------------------------------
  optimizer.zero_grad()                                 -- (every gradient is overwritten, never accumulated)
  out = model(batch)                                    hcg_fused_forward               1 launch: both conv layers, pooling AND
  loss = sqrt(MSELoss(out, y.unsqueeze(1)))                 the readout head (forward, squared error, unscaled backward)
  loss.backward()                                       hcg_fused_layer_bwd x n_conv    (other graph sizes: hcg_mid_* / hcg_tall_*
                                                            per layer + hcg_head_fwd_bwd)
  [data parallel]                                       [one-shot xGMI exchange inside the last launch, or an RCCL all-reduce]
  optimizer.step()                                      hcg_step_tail                   1 launch: slab reductions -> ONE flat
  loss.item()                                               gradient, loss + its deferred scale, Adam, the next batch's plan
                                                        -- (the loss stays on the device; ONE sync per epoch)

No autograd graph is built: the step is a fixed sequence of C-ABI calls, which is also what makes it capturable
into a hipGraph (`FusedTrainStep.capture`).  Graphs up to 32 nodes run through the small-graph tiles (csrc/fused.hip),
graphs up to 192 nodes -- the reference's own reaction graphs -- through the one-graph-per-workgroup kernels
(csrc/mid.hip).  Models / batches neither covers (widths other than 64, explicit edge weights, larger graphs) take
the autograd path with the same arithmetic contract.
"""
from __future__ import annotations

import contextlib
import ctypes
from typing import NamedTuple, Optional

import torch
import torch.distributed

from . import _lib
from . import functional as HF

def _is_cross_entropy(model) -> bool:
    """`--problem_type classification`: the model's loss is an `nn.CrossEntropyLoss` (networks.CrossEntropyLoss)."""
    return isinstance(getattr(model, "loss", None), torch.nn.CrossEntropyLoss)


def _cross_entropy_reason(model) -> Optional[str]:
    """Why the fused step does not take this cross-entropy model (None: it does).  The kernels compute
    `nn.CrossEntropyLoss()(out, y.long())` with default settings over two classes or more."""
    loss = model.loss
    if loss.weight is not None:
        return "cross-entropy with class weights (weight is not None)"
    if loss.reduction != "mean":
        return f"cross-entropy with reduction={loss.reduction!r} (only 'mean')"
    if loss.label_smoothing != 0.0:
        return f"cross-entropy with label_smoothing={loss.label_smoothing}"
    if loss.ignore_index != -100:
        return f"cross-entropy with ignore_index={loss.ignore_index}"
    if model._n_classes < 2:
        return f"cross-entropy with n_classes={model._n_classes} (needs 2 or more)"
    return None


def _head_deep_supported(D: int, C: int, R: int) -> bool:
    """A readout of depth R at width D with C outputs has the one-launch head of csrc/head.hip (k_head_deep)."""
    return _lib.load().hcg_general_workspace_bytes(_lib.HCG_WS_HEAD_DEEP, 1, D, C, R) > 0


class LayerForm(NamedTuple):
    """How one conv layer runs in a step: everything `layer_forms` decides and the step's phases then only read."""
    fam: object             # kernel family (functional.TILES / MID / TALL)
    gpt: int                # graphs per tile (0 off the small-graph tiles)
    stacked: bool           # forward: the two layers of a two-layer stack on the tiles, one launch
    bits: Optional[str]     # pooled layer kept as sign / is-the-column-max bits only: the workspace that holds them
    #                         ("poolbits": tiles, "poolbits_r": as a part; "poolbits_tall": wide-layer route); None = stored
    head: bool              # pooled layer of a stack on the tiles, kept as bits: its forward launch can carry the readout head
    kp: int                 # dense first layer: the forward also leaves Ahat x [N, kp] (32 / 64 / 128) and the sign pieces of
    #                         its output, the whole backward is ONE dense launch (csrc/tall.hip: k_tall_dw<FIRST>); 0 = not
    flags: int              # the backward's flag word: 1 = applies its own activation derivative (0: dout arrives premasked,
    #                         the layer never reads its own output), 2 = hands dx down premasked
    pair: Optional[str]     # "upper" (layer 1) / "lower" (layer 0) of a backward pair candidate: both on the tiles, dx premasked
    jobs: int               # reduction jobs its backward leaves for the step tail (a later part: 0, its slabs join the first's)


class Part(NamedTuple):
    """A graph range of a step's batch.  An ordinary batch is one part; a size-grouped one (`collate(..., group_by_size=True)`)
    is two: graphs [0, n_small) on the small-graph tiles, the others one graph per wave / workgroup (disjoint rows and slabs)."""
    geo: object             # functional.Geometry of the range (node rows stay absolute)
    forms: list             # the LayerForm of every conv layer on it (`step_parts`)
    stream: object          # hipStream_t its launches go to: None = the current stream


def _convs(model):
    """[model.conv1] + list(model.conv_layers) from `_modules`: no `nn.Module.__getattr__` (~0.5 us each, twice per step)."""
    return [model._modules["conv1"], *model._modules["conv_layers"]._modules.values()]


def _layer_shapes(model, convs=None):
    """(in_channels, out_channels, family preference) of every conv layer (`convs`: the caller has listed them already)."""
    return [(c.in_channels, c.out_channels, getattr(c, "family", "auto")) for c in (_convs(model) if convs is None else convs)]


def layer_forms(shapes, N, max_nodes, max_edges, forward_only=False, sw=None, plan=None, part=None):
    """The form of every conv layer of a step -> [LayerForm], or None when a layer has no fused kernel family.  Pure host
    arithmetic on plain values: `shapes` = `_layer_shapes`, the batch's row count and largest graph, `sw` = whoever holds the
    development switches (a step, default the class), `plan` (whose own N and largest graph the caller passes) adds
    `conv_route`'s plan-level checks.  The support check asks with a batch's collate metadata, `_prepare` with its plan: the
    jobs the one predicts are the jobs the other leaves.
    `part`: the forms of a graph range of a size-grouped batch, the part-th of `step_parts` (`max_nodes`: its largest graph).
    A range takes no row-streaming form (family "mid" whatever the convs prefer, no dense first layer: those kernels walk all
    N rows), is no backward pair candidate, carries no head and keeps the tiles' pooled layer as bits whatever POOLBITS says."""
    sw = FusedTrainStep if sw is None else sw
    whole = part is None
    routes = [HF.conv_route(plan, F, D, family if whole else "mid", max_nodes=max_nodes, max_edges=max_edges, rows=N)
              for F, D, family in shapes]
    if (None, 0) in routes:
        return None
    n, fams = len(routes), [fam for fam, _ in routes]
    stacked = n == 2 and fams[0] is HF.TILES and routes[0] == routes[1]
    pair = (whole and sw.BWD_PAIR and sw.PREMASK and not forward_only and n >= 2 and fams[0] is HF.TILES
            and fams[1] is HF.TILES)
    # a layer on the tiles or one graph per workgroup can hand its dx down already multiplied by the activation derivative
    # of the layer below (it holds those rows anyway, for dW): one tensor less per step
    premask = [bool(sw.PREMASK) and l > 0 and fam is not HF.TALL for l, fam in enumerate(fams)]
    forms = []
    for l, ((F, D, _), (fam, gpt)) in enumerate(zip(shapes, routes)):
        last = l == n - 1
        bits = None
        if not whole:
            bits = "poolbits_r" if last and fam is HF.TILES else None
        elif last and sw.POOLBITS and (fam is HF.TILES or (fam is HF.TALL and F <= (64 if D == 64 else 128))):
            bits = "poolbits" if fam is HF.TILES else "poolbits_tall"
        dense = False
        if whole and l == 0 and n >= 2 and sw.XAGG and not forward_only:
            if fam is HF.TALL:
                dense = (F <= 64 or D == 128) and fams[1] is HF.TALL
            elif fam is HF.MID:     # (behind the one-graph-per-workgroup kernels: batches under functional.TALL_MIN_NODES_D64)
                dense = (D == 64 and F <= 64 and sw.XAGG_MID and fams[1] is not HF.TILES
                         and HF.tall_shape_supported(N, F, D, max_nodes, max_edges, any_rows=True))
        kp = (32 if F <= 32 else (64 if F <= 64 else 128)) if dense else 0
        flags = (1 if (last or not premask[l + 1]) else 0) | (2 if premask[l] else 0)
        # jobs: the families' `reduce_jobs` -- the tiles 1; the wide-layer route and the dense first layer dW, db; one graph
        # per workgroup one per 64-column half
        jobs = 1 if fam is HF.TILES else (2 if (fam is HF.TALL or kp) else D // 64)
        forms.append(LayerForm(fam, gpt, stacked, bits, bool(whole and last and stacked and bits), kp, flags,
                               ("lower", "upper")[l] if (pair and l < 2) else None, jobs if part in (None, 0) else 0))
    return forms


def step_parts(shapes, N, B, max_nodes, max_edges, n_small=None, C=1, forward_only=False, sw=None, plan=None):
    """The graph ranges a step runs as its parts -> [(first graph, graphs, [LayerForm])], None when a layer has no fused kernel
    family.  Two for a size-grouped batch (`n_small`: where `Batch.n_small` says the second group starts) of a model the
    grouping covers -- two conv layers of width 64, the one-launch head -- with both groups non-empty, a largest graph over
    32 nodes, every layer of the first group on the tiles and of the second one graph per wave / workgroup; else the batch."""
    sw = FusedTrainStep if sw is None else sw
    # a step keeps the answers by the inputs (it asks twice per step: the support check, then `_prepare` with the plan, whose
    # own checks -- passed -- add nothing); without the memo the eager step's host time was 0.113 against 0.104 ms
    memo = sw._forms_memo if (plan is None or HF._per_graph_plan(plan)) else None
    key = (tuple(shapes), N, B, max_nodes, max_edges, n_small, C, forward_only, sw.POOLBITS, sw.XAGG, sw.XAGG_MID, sw.PREMASK,
           sw.BWD_PAIR, HF.TALL_MIN_NODES_D64)
    if memo is not None and key in memo:
        return memo[key]
    parts = None
    if (n_small is not None and 0 < n_small < B and len(shapes) == 2 and shapes[0][1] == 64 and max_nodes is not None
            and max_nodes > 32 and max_edges is not None and _lib.load().hcg_head_supported(64, C)):
        a = layer_forms(shapes, N, 32, max_edges, forward_only, sw, plan, part=0)
        b = layer_forms(shapes, N, max_nodes, max_edges, forward_only, sw, plan, part=1)
        if a and b and all(f.fam is HF.TILES for f in a) and all(f.fam is HF.MID for f in b):
            parts = [(0, int(n_small), a), (int(n_small), B - int(n_small), b)]
    if parts is None:
        forms = layer_forms(shapes, N, max_nodes, max_edges, forward_only, sw, plan)
        parts = None if forms is None else [(0, B, forms)]
    if memo is not None:
        if len(memo) >= 64:         # (a shuffled epoch's batches differ in N: bounded, not kept for ever)
            memo.clear()
        memo[key] = parts
    return parts


class _Ctx:
    """Everything one step needs, resolved once: shapes, weights, buffers, its parts (`step_parts`: the form of every layer).
    `main`, `side`: the current stream and the later parts' while a size-grouped step is captured; `poolbits`: per part."""
    __slots__ = ("batch", "plan", "x", "y2", "convs", "lins", "N", "F", "B", "D", "C", "n_conv", "dev", "W", "bs",
                 "parts", "main", "side", "bufs", "head_fused", "forward_only", "flat", "gaddr", "step_word", "jobs",
                 "loss_mode", "sse_split", "poolbits", "xagg", "bwd_pair")


class FusedTrainStep:
    """One training step of the reference's loop as THREE enqueued launches on small-graph tiles (conv stack + pooling +
    readout head, the two conv backward layers as one pair launch -- two launches with `BWD_PAIR = False` or where the pair
    does not apply --, the step tail), n_conv + 4 in general -- no autograd, no host sync.

        step = FusedTrainStep(model)            # model: hcatgnet_amd.GCN on the GPU
        loss = step(batch)                      # 0-d device tensor: sqrt(MSE) of this batch, weights already updated

    `rmse=True` is the reference's `torch.sqrt(model.loss(...))`; `optimizer_step=False` stops after the backward
    (gradients in `model.parameters()[i].grad`, views of one flat buffer); `grad_sync` is called with the flat gradient
    between backward and optimiser (data parallel: `DataParallelGCN.attach(step)` sets it).

    The loss scale is DEFERRED: the backward is linear in dloss/dout = scale * (out - y), so the head and every conv
    backward launch run on the unscaled error, the head leaves one partial sum of squared errors per workgroup, and the
    step's last launch (`hcg_step_tail`) derives loss and scale and applies the scale while it reduces the gradient slabs
    -- there is no grid-wide exchange anywhere in the step (csrc/head_tile.h, csrc/reduce.hip).

    `combine` (data parallel, needs rmse): "mean" = every rank's own sqrt(MSE), gradients averaged (DDP convention);
    "sse" = gradients stay those of SSE / 2, [SSE, count] sit behind the flat buffer, `grad_sync` SUMS all of it over the
    ranks and ONE scale 1 / (count * sqrt(SSE / count)) gives the gradient of sqrt(MSE) over the concatenated batch of all
    ranks -- what the reference's step computes on one device (utils/utils_model.py:64-65); the loss returned is then that
    global loss.

    Classification (`--problem_type classification`, a model whose loss is `nn.CrossEntropyLoss` with default settings --
    no class weights, reduction "mean", no label smoothing -- and two classes or more): the reference's training line
    cannot execute for such a model, so the loss is the minimal reading of it, `nn.CrossEntropyLoss()(out, y.long())`
    with `out` [B, C] and `y` [B] holding class indices: the mean over the graphs of the batch, no sqrt, no unsqueeze
    (`rmse` does not apply).  The same split carries it: the head runs its backward on softmax(out) - onehot and leaves a
    partial sum of per-graph terms logsumexp(out) - out[label], the deferred scale is 1 / B (HCG_LOSS_CE).  The head is a
    launch of its own (the one riding in the forward launch is regression-only), `y` may be int64 or float32, a label outside
    0 .. C-1 makes the loss NaN, and `combine="sse"` is refused: it is a property of the squared error.
    """

    # development switches for A/B measurements (tools/ab_env.sh sets them from the environment; never set in product
    # code): POOLBITS = False stores the pooled layer's activations as the plain forms do, PREMASK = False leaves every
    # activation derivative to the layer that owns it, HEAD_IN_FORWARD = False keeps the head a launch of its own
    POOLBITS = True
    XAGG_MID = True                # ... and behind the one-graph-per-workgroup kernels (batches under functional.TALL_MIN_NODES_D64)
    XAGG = True                    # first layer on the wide-layer route: Ahat x + sign pieces from the forward, one dense backward launch
    PREMASK = True
    # conv layers 1 and 0 on the small-graph tiles: their backward as two phases of ONE launch (csrc/fused.hip:
    # k_fused_bwd_pair; bitwise the two launches).  On since its A/B (profiles/bwd_pair_ab.txt): the slowest of 5
    # pair runs of the C3 bench beat the fastest of 5 two-launch runs, 0.0999 against 0.1019 ms/step (means 0.0995 / 0.1024)
    BWD_PAIR = True
    HEAD_IN_FORWARD = True
    OVERLAP_GROUPS = True          # captured size-grouped steps: the two kernel families as two branches of the hipGraph
    _forms_memo = None             # (`step_parts` asked with the class, or a step made without __init__: nothing is kept)

    def __init__(self, model, rmse: bool = True, optimizer_step: bool = True, grad_sync=None, combine: str = "mean"):
        if combine not in ("mean", "sse"):
            raise ValueError(f"combine must be 'mean' or 'sse', got {combine!r}")
        if combine == "sse" and not rmse:
            raise ValueError("combine='sse' reproduces sqrt(MSE) over the concatenated batch: it needs rmse=True")
        if combine == "sse" and _is_cross_entropy(model):
            raise ValueError("combine='sse' reproduces sqrt(MSE) over the concatenated batch: a cross-entropy model takes "
                             "combine='mean'")
        self.model, self.rmse, self.optimizer_step, self.grad_sync = model, rmse, optimizer_step, grad_sync
        self.combine = combine
        if optimizer_step and hasattr(model.optimizer, "enable_capturable"):
            model.optimizer.enable_capturable()     # step count / lr in device memory: same launches eager and captured
        self._bufs = {}
        self._graph = None
        self._capturing_split = False
        self._side_streams = {}
        # pipelined loaders: a pointers-only `BatchPlan` of the NEXT batch (built once with validate=False); the step's last
        # launch re-derives its graph_ptr / edge_ptr from the tensors' current contents, so the next step -- on a batch object
        # that carries that plan (`batch._hcg_plan = plan`) -- starts without a plan launch
        self.next_plan = None
        # data parallel: a `xgmi.OneShotExchange` (set by its `attach`): the gradient exchange then happens INSIDE the step's
        # last launch instead of as an RCCL collective between two launches
        self.exchange = None
        self._last_carried = False              # the last step's tail launch carried reduction + (exchange) + update
        self.exchange_fallback_sync = None      # the collective hook `OneShotExchange.attach` took out of `grad_sync`
        # one-device rehearsals only (two ranks sharing a GPU): called right before the launch that carries the exchange.
        # A rank's polling launch fills every CU, and the OTHER process's conv kernels (488 of a SIMD's 512 VGPRs per
        # workgroup) cannot be placed beside it, so on one device the ranks must meet (synchronize + barrier) before that
        # launch; on one GPU per rank nothing of another process ever runs on the device and this stays None
        self.pre_exchange_hook = None
        # data parallel, RCCL form: True = `capture()` / `StepWindow` record the collective and the update launch too (RCCL
        # collectives survive hipGraph capture: tools/exp_rccl_capture.py), so the whole data-parallel step is ONE graph.
        # Default False: the graph ends after the slab reduction, `replay()` issues collective + update eagerly behind it
        self.capture_exchange = False
        self._pcache = None
        self._pair_ok = {}                      # answers of the backward pair's query (`_pair_applies`)
        self._forms_memo = {}                   # ... and of `step_parts`

    def _trainable(self):
        """The model's parameters in `model.parameters()` order, from a cache: the module walk of `nn.Module.parameters()`
        costs ~20 us and a step needs the list four times (a quarter of the host time of a step at the reference's batch
        size 40).  The cache is checked on every use -- each (module, name) slot still holds the same Parameter object and
        the model's direct children are the same modules -- and rebuilt when not."""
        model, c = self.model, self._pcache
        key = tuple(map(id, model._modules.values()))
        if c is None or c[0] != key or any(m._parameters.get(n) is not q for m, n, q in c[1]):
            entries, seen = [], set()
            for m in model.modules():
                for n, q in m._parameters.items():
                    if q is not None and id(q) not in seen:
                        seen.add(id(q))
                        entries.append((m, n, q))
            c = self._pcache = (key, entries, [q for _, _, q in entries])
        return c[2]

    def reason(self, batch=None) -> Optional[str]:
        """`unsupported_reason(self.model, batch)` with the cached parameter list."""
        return self.unsupported_reason(self.model, batch, self._trainable(), self)

    # ------------------------------------------------------------------ support check (host only)
    @staticmethod
    def unsupported_reason(model, batch=None, _params=None, _step=None) -> Optional[str]:
        """None when `model` takes the fused step on `batch`, else why not.  Without a batch the answer covers the model
        alone, and only for readout depth 2: other depths (1, 3, 4 at widths 64 / 128 with up to 8 classes) are accepted
        per batch, which is how the step and every epoch loop ask."""
        lib = _lib.load()
        R = getattr(model, "readout_layers", None)
        if R != 2 and not (R is not None and _head_deep_supported(model.embedding_dim, model._n_classes, R)):
            return ("readout depth other than 2, or other than 1 / 3 / 4 at widths 64 / 128 with up to 8 classes "
                    f"(readout_layers = {R})")
        if not bool(getattr(model, "use_fused", True)):
            return "fused kernels disabled on the model"
        # every gradient slab of the step is reduced by ONE launch of at most HCG_REDUCE_MAX_JOBS jobs (hcg_step_tail)
        head_jobs = 1 if (R != 2 or lib.hcg_head_supported(model.embedding_dim, model._n_classes)) else 0
        shapes = _layer_shapes(model)
        if FusedTrainStep._conv_jobs(model, shapes=shapes) + head_jobs > _lib.HCG_REDUCE_MAX_JOBS:
            return (f"{model.n_convolutions} conv layers of width {model.embedding_dim}: their gradient reductions and the "
                    f"head's exceed the step tail's {_lib.HCG_REDUCE_MAX_JOBS} jobs")
        # (heads the one-launch kernel does not cover -- widths other than 64 / 128 -- run as five launches of the any-shape
        #  kernels inside the same no-autograd step)
        if _is_cross_entropy(model):
            why = _cross_entropy_reason(model)
            if why is not None:
                return why
        elif type(model.loss).__name__ != "MSELoss":
            return "loss other than MSE or cross-entropy"
        if not all(q.requires_grad for q in (model.parameters() if _params is None else _params)):
            return "frozen parameters (the fused backward writes every gradient)"
        if batch is not None:
            if getattr(batch, "y", None) is None:
                return "batch has no targets"
            mx = getattr(batch, "max_nodes", None)
            if mx is None or not getattr(batch, "edges_grouped", False):
                return "batch lacks collate metadata (max_nodes / grouped edges)"
            jobs = FusedTrainStep._conv_jobs(model, batch, _step, shapes)
            if jobs is None:
                return "graph / layer shape outside the fused kernels (small-graph tiles and one-graph-per-workgroup)"
            if jobs + head_jobs > _lib.HCG_REDUCE_MAX_JOBS:
                return (f"{model.n_convolutions} conv layers on this batch's kernel forms need {jobs} gradient reductions, "
                        f"with the head's over the step tail's {_lib.HCG_REDUCE_MAX_JOBS} jobs")
        elif R != 2:
            return f"readout depth {R} is accepted per batch: ask with the batch (without one, only depth 2 is vouched for)"
        return None

    @staticmethod
    def _conv_jobs(model, batch=None, step=None, shapes=None) -> Optional[int]:
        """Reduction jobs the conv layers' backward leaves for the step tail: the sum over the batch's `step_parts` (asked
        with its collate metadata), the same plan `_backward_layers` executes; None = a layer outside the fused kernels.
        Without a batch: the fewest any batch could need (1 per 64-wide layer, 2 per wider one)."""
        shapes = _layer_shapes(model) if shapes is None else shapes
        if batch is None:
            return sum(1 if D == 64 else 2 for _, D, _ in shapes)
        ns = getattr(batch, "n_small", None)
        # (the arguments `_prepare` will ask with: the two questions of a step are one entry of the step's memo)
        parts = step_parts(shapes, batch.x.shape[0], batch.num_graphs, batch.max_nodes, getattr(batch, "max_edges", None), ns,
                           model._n_classes, sw=step)
        return None if parts is None else sum(f.jobs for _, _, forms in parts for f in forms)

    def _side_stream(self, dev):
        st = self._side_streams.get(dev)
        if st is None:
            st = self._side_streams[dev] = torch.cuda.Stream(device=dev)
        return st

    # ------------------------------------------------------------------ buffers
    def _buffers(self, key, N, B, F, D, C, n_conv, dev, R=2):
        """Step buffers: allocated for the largest (N, B) seen so far and handed out as views -- the variable-size
        batches of a shuffled epoch then reuse one allocation instead of ~12 `torch.empty` per step."""
        lib = _lib.load()
        cap = self._bufs.get("cap")
        sig = (F, D, C, n_conv, dev, R)
        if cap is None or cap["sig"] != sig or cap["N"] < N or cap["B"] < B:
            capN = max(N, int(cap["N"] * 1.25) if cap and cap["sig"] == sig else 0)
            capB = max(B, cap["B"] if cap and cap["sig"] == sig else 0)
            f32 = dict(dtype=torch.float32, device=dev)
            # head slabs: the stand-alone head's (<= one per CU) or the forward tail's (one per workgroup of the tile launch:
            # graphs_per_tile 1 bounds it)
            hb = max(lib.hcg_head_workspace_bytes(capB, D if lib.hcg_head_supported(D, C) else 64),
                     lib.hcg_fused_aux_bytes(_lib.HCG_FUSED_HEAD_WS, capB, 1),
                     lib.hcg_general_workspace_bytes(_lib.HCG_WS_HEAD_DEEP, capB, D, C, R))
            cap = {"sig": sig, "N": capN, "B": capB,
                   "acts": [torch.empty(capN, D, **f32) for _ in range(n_conv)],
                   "dacts": [torch.empty(capN, D, **f32) for _ in range(n_conv - 1)],
                   "emb": torch.empty(capB, 2 * D, **f32), "demb": torch.empty(capB, 2 * D, **f32),
                   "z": torch.empty(capB, D, **f32), "out": torch.empty(capB, C, **f32), "loss": torch.zeros(2, **f32),
                   "ws_head": torch.empty(hb, dtype=torch.uint8, device=dev), "ws": {}}
            self._bufs = {"cap": cap}
            self._graph = None                          # a captured graph holds the old buffers' addresses
        b = self._bufs.get(key)
        if b is None:
            b = {"acts": [t[:N] for t in cap["acts"]], "dacts": [t[:N] for t in cap["dacts"]], "emb": cap["emb"][:B],
                 "demb": cap["demb"][:B], "z": cap["z"][:B], "out": cap["out"][:B], "loss": cap["loss"],
                 "ws_head": cap["ws_head"], "ws_head_bytes": cap["ws_head"].numel(), "ws": cap["ws"]}
            self._bufs = {"cap": cap, key: b}          # views of the current shape (one live shape at a time)
        return b

    def _layer_ws(self, c: _Ctx, l, fams, F):
        """Workspace of layer l's kernels, of family `fams[i]` on part i (gradient slabs; the wide-layer kernels' also holds
        the H / dH round trip, and their forward and backward share it) -> per part (buffer or address, bytes).  The parts'
        slabs share one buffer, back to back: an earlier part's are its launch's slabs exactly (its query less the 256-byte pad)."""
        if len(c.parts) == 1:
            p, fam = c.parts[0], fams[0]
            wsb = fam.workspace_bytes(p.geo, p.forms[l].gpt, F, c.D)
            return [(self._ws(c.bufs, (fam.name, l) if fam.row_streaming else l, wsb, c.dev), wsb)]
        sizes = []
        for i, (p, fam) in enumerate(zip(c.parts, fams)):
            is_last = i == len(fams) - 1
            sizes.append(fam.workspace_bytes(p.geo, p.forms[l].gpt, F, c.D) - (0 if is_last else 256))
        ws, slabs, off = self._ws(c.bufs, ("r", l), sum(sizes), c.dev), [], 0
        for nbytes in sizes:                # (the first part is handed the buffer, the later ones an address inside it)
            slabs.append((ws if off == 0 else ws.data_ptr() + off, nbytes))
            off += nbytes
        return slabs

    def _ws(self, bufs, key, nbytes, dev):
        ws = bufs["ws"].get(key)
        if (ws is None or ws.numel() < nbytes) and nbytes > 0:
            ws = bufs["ws"][key] = torch.empty(int(nbytes * 1.25), dtype=torch.uint8, device=dev)
        return ws

    def _head_buffers(self, bufs, B, D, C, dev):
        """Scratch of the any-shape head (five launches): allocated once per capacity."""
        lib = _lib.load()
        hb = bufs["ws"].get("head_generic")
        if hb is None or hb["B"] < B:
            f32 = dict(dtype=torch.float32, device=dev)
            u8 = dict(dtype=torch.uint8, device=dev)
            hb = {"B": B, "dout": torch.empty(B, C, **f32), "dz": torch.empty(B, D, **f32),
                  "dz_ws1": torch.empty(B, C, **f32), "dz_ws0": torch.empty(B, D, **f32),
                  "ws1": torch.empty(max(lib.hcg_general_workspace_bytes(_lib.HCG_WS_LINEAR, B, D, C, 0), 256), **u8),
                  "ws0": torch.empty(max(lib.hcg_general_workspace_bytes(_lib.HCG_WS_LINEAR, B, 2 * D, D, 0), 256), **u8)}
            bufs["ws"]["head_generic"] = hb
        return hb

    def _flat_grads(self, params, dev):
        """ONE flat gradient buffer in parameter order (+ two floats behind it: [SSE, count] of the data-parallel "sse"
        form); the parameters' `.grad` are (re-)attached as views of it."""
        n = sum(p.numel() for p in params)
        flat = getattr(self, "_flat", None)
        if flat is None or flat.numel() != n or flat.device != dev:
            self._flat_ext = torch.zeros(n + 2, dtype=torch.float32, device=dev)
            flat = self._flat_ext[:n]
            self._flat = flat
            self._graph = None
            off = 0
            for p in params:                      # .grad = view of the flat buffer, parameter order
                p.grad = flat[off:off + p.numel()].view_as(p)
                off += p.numel()
        else:
            off = 0
            for p in params:
                g = p.grad
                if g is None or g.data_ptr() != flat.data_ptr() + 4 * off:
                    p.grad = flat[off:off + p.numel()].view_as(p)
                off += p.numel()
        return flat

    # ------------------------------------------------------------------ the step, piece by piece
    def _prepare(self, batch, forward_only: bool) -> _Ctx:
        model, lib = self.model, _lib.load()
        c = _Ctx()
        c.batch, c.forward_only = batch, forward_only
        x, y = batch.x, batch.y
        _lib.require_gpu(x, y, batch.edge_index)
        c.x = x = HF._f32c(x)
        c.plan = plan = model._plan_for(batch, x, batch.edge_index, batch.batch, None)
        c.convs = convs = _convs(model)
        # readout linears: readout[i] = Sequential(Linear, LeakyReLU) for the hidden layers, the last a bare Linear
        c.lins = [m[0] if isinstance(m, torch.nn.Sequential) else m for m in model.readout]
        c.N, c.F, c.B, c.D, c.C = x.shape[0], x.shape[1], plan.B, model.embedding_dim, model._n_classes
        c.n_conv, c.dev = len(convs), x.device
        ce = _is_cross_entropy(model)
        if ce:
            # one class index per graph, as float32 (what the stores and loaders keep; int64 labels are converted)
            c.y2 = (y if y.dtype == torch.float32 else y.to(torch.float32)).contiguous().reshape(-1)
            if c.y2.shape[0] != c.B:
                raise ValueError(f"classification targets hold {c.y2.shape[0]} class indices for {c.B} graphs")
        else:
            c.y2 = HF._f32c(y).reshape(c.B, -1)
            if c.y2.shape[1] != c.C:
                raise ValueError(f"targets have {c.y2.shape[1]} columns, the model predicts {c.C}")
        parts = step_parts(_layer_shapes(model, convs), plan.N, c.B, plan.max_nodes, plan.max_edges, getattr(batch, "n_small", None),
                           c.C, forward_only, self, plan)
        if parts is None:
            raise _lib.HcgError("FusedTrainStep: graph / layer shape outside the fused kernels")
        # while a size-grouped step is being CAPTURED the later part's launches go to a second stream, forked before each conv
        # phase and joined behind it = two branches of the hipGraph: each family's last workgroups fill the CUs the other has
        # already left (neither fills the chip: ~1.4 tiles per wave / ~0.6 graphs per wave slot at 4096 graphs).  Ragged bench:
        # replay 0.1975 -> 0.188 ms/step; the four event calls cost the host-bound eager step 0.196 -> 0.215: it keeps one stream
        c.main = c.side = side = None
        if len(parts) > 1:
            side = _lib.stream_ptr()            # (asked once for the later parts' launches)
            if self.OVERLAP_GROUPS and torch.cuda.is_current_stream_capturing():
                c.main, c.side = torch.cuda.current_stream(c.dev), self._side_stream(c.dev)
                side = ctypes.c_void_p(c.side.cuda_stream)
        c.parts = [Part(HF.geometry(plan, g0, nB), forms, side if g0 else None) for g0, nB, forms in parts]
        c.bufs = self._buffers((c.N, c.B, c.F, plan.E), c.N, c.B, c.F, c.D, c.C, c.n_conv, c.dev, len(c.lins))
        c.W = [HF._f32c(cv.lin.weight) for cv in convs]
        c.bs = [HF._f32c(cv.bias) for cv in convs]
        c.head_fused = bool(lib.hcg_head_supported(c.D, c.C) if len(c.lins) == 2
                            else _head_deep_supported(c.D, c.C, len(c.lins)))
        c.jobs = HF.JobList()
        c.flat = c.gaddr = c.step_word = None
        c.poolbits = [None] * len(c.parts)
        c.xagg = None
        c.bwd_pair = False
        # how the loss scale reaches the gradients (see the class docstring).  "sse" with a collective between backward and
        # update: the tail leaves the gradients unscaled and [SSE, count] behind the flat buffer; everything else: the tail
        # applies this rank's own scale ("sse" without any exchange IS sqrt(MSE) of the own batch)
        dp_sync = self.grad_sync is not None or self.exchange is not None or self._capturing_split
        c.sse_split = self.combine == "sse" and dp_sync and not forward_only
        c.loss_mode = _lib.HCG_LOSS_SSE if c.sse_split else (_lib.HCG_LOSS_RMSE if self.rmse else _lib.HCG_LOSS_MSE)
        if ce:
            c.loss_mode = _lib.HCG_LOSS_CE              # (`rmse` does not apply; "sse" was refused at construction)
        if not forward_only:
            params = self._trainable()
            c.flat = self._flat_grads(params, c.dev)
            # address of every parameter's slice of the flat gradient buffer (cached per buffer: eight tensor slices per
            # step otherwise)
            ga = getattr(self, "_gaddr", None)
            if ga is None or ga[0] != c.flat.data_ptr() or ga[1] is not params:
                addr, off = {}, 0
                for q in params:
                    addr[id(q)] = c.flat.data_ptr() + 4 * off
                    off += q.numel()
                ga = self._gaddr = (c.flat.data_ptr(), params, addr)
            c.gaddr = ga[2]
            # without a collective between backward and update, the step's last launch applies the update itself; the head
            # advances the step number that launch reads
            opt = model.optimizer
            # (a one-shot exchange rides in that launch only when all its polling workgroups are resident at once: the
            #  64-wide model's slabs need ~540 of ~1800; the 128-wide one's ~2100 -- it keeps the collective, see
            #  hcg_xchg_resident_blocks)
            if (self.optimizer_step and self.grad_sync is None and not self._capturing_split and c.head_fused
                    and hasattr(opt, "fused_update_ready") and (self.exchange is None or c.D == 64)):
                c.step_word = opt.fused_update_ready(c.flat)
            c.bwd_pair = self._pair_applies(c)
        return c

    def _pair_applies(self, c: _Ctx) -> bool:
        """Decided here, before anything is launched: conv layers 1 and 0 a pair candidate of the plan (both on the
        small-graph tiles, layer 1 handing its dx down premasked), and the library agreeing (the query touches no GPU; its
        answer is kept per shape and buffer set)."""
        geo, forms, _ = c.parts[0]
        if not forms[0].pair:
            return False
        acts0, dx, gpt, gpt_up = c.bufs["acts"][0], c.bufs["dacts"][0], forms[0].gpt, forms[1].gpt
        key = (c.F, c.D, gpt, gpt_up, c.x.data_ptr() % 16, acts0.data_ptr() % 16, dx.data_ptr() % 16)
        ok = self._pair_ok.get(key)
        if ok is None:
            # (the upper layer's form does not enter the answer: asked as the not-pooled one)
            ok = self._pair_ok[key] = HF.TILES.backward_pair(geo, gpt, c.x, c.W[0], acts0, c.W[1], 2, gpt_up=gpt_up,
                                                             dout=dx, dx=dx, query=True)
        return ok

    def _g(self, c: _Ctx, prm) -> int:
        return c.gaddr[id(prm)]

    def _tiles_stack(self, c: _Ctx, geo, gpt, **extra):
        """Both conv layers (+ pooling) on the small-graph tiles: one launch."""
        HF.TILES.forward(geo, gpt, c.x, c.W[0], c.bs[0], 1, out=c.bufs["acts"][0], emb=c.bufs["emb"], W2=c.W[1], b2=c.bs[1],
                         **extra)

    def _head_in_forward(self, c: _Ctx) -> bool:
        """The C3 form: both conv layers on small-graph tiles, pooled layer on chip, one-launch head -> everything up to
        the loss is ONE launch."""
        return bool(self.HEAD_IN_FORWARD and c.head_fused
                    and c.loss_mode != _lib.HCG_LOSS_CE      # (the head in the forward launch is regression-only)
                    and len(c.lins) == 2 and c.parts[0].forms[-1].head)

    def _pooled_bits(self, c: _Ctx, i=0):
        """The pooled layer's activations stay on chip: the bits its backward needs of them (sign, is-the-column-max) are all
        that is stored -- two bits per element on the small-graph tiles, one byte per (row, 4 columns) on the wide-layer
        route (csrc/tall.hip: k_gseg_bwd).  -> their workspace on part i, None for a pooled layer in the plain form."""
        geo, top = c.parts[i].geo, c.parts[i].forms[-1]
        if top.bits:
            nbytes = (c.N * (c.D // 4) if top.bits == "poolbits_tall"
                      else _lib.load().hcg_fused_aux_bytes(_lib.HCG_FUSED_POOLBITS, geo.B, top.gpt))
            c.poolbits[i] = self._ws(c.bufs, top.bits, nbytes, c.dev)
        return c.poolbits[i]

    def _forward_with_head(self, c: _Ctx):
        """conv stack + pooling + readout head (forward, squared error, unscaled readout backward): one launch."""
        lib, bufs, geo, gpt = _lib.load(), c.bufs, c.parts[0].geo, c.parts[0].forms[0].gpt
        l0, l1 = c.lins
        self._tiles_stack(
            c, geo, gpt, poolbits=self._pooled_bits(c), y=c.y2, head_W0=HF._f32c(l0.weight), head_b0=HF._f32c(l0.bias),
            head_W1=HF._f32c(l1.weight), head_b1=HF._f32c(l1.bias), C=c.C, z=bufs["z"], head_out=bufs["out"], demb=bufs["demb"],
            head_workspace=bufs["ws_head"], head_workspace_bytes=bufs["ws_head_bytes"], step_counter=c.step_word,
            head_flags=_lib.HCG_HEAD_FORWARD_ONLY if c.forward_only else 0)
        g = (lambda q: self._g(c, q)) if not c.forward_only else (lambda q: None)
        _lib.check(lib.hcg_fused_head_reduce_job(_lib.ptr(bufs["ws_head"]), bufs["ws_head_bytes"], c.B, gpt, c.C, g(l0.weight),
                                                 g(l0.bias), g(l1.weight), g(l1.bias), c.jobs.slot()),
                   "hcg_fused_head_reduce_job")
        c.jobs.n += 1

    def _forward_layers(self, c: _Ctx):
        """The conv stack (+ pooling) of every other shape: per part one launch per layer (stacked pair: one), layer by layer."""
        bufs, acts, top = c.bufs, c.bufs["acts"], c.n_conv - 1
        if c.side is not None:
            c.side.wait_stream(c.main)      # fork: the side stream starts behind everything issued so far
        for l in range(c.n_conv):
            h = c.x if l == 0 else acts[l - 1]
            for i, (geo, forms, stream) in enumerate(c.parts):
                f = forms[l]
                if f.stacked:
                    if l == 0:
                        bits = self._pooled_bits(c, i)
                        self._tiles_stack(c, geo, f.gpt, poolbits=bits, out2=None if bits is not None else acts[1])
                    continue
                kw = dict(out=acts[l])
                if l == top:
                    bits = self._pooled_bits(c, i) if f.bits else None
                    kw = dict(out=None if bits is not None else acts[l], emb=bufs["emb"], poolbits=bits)
                if f.fam.row_streaming:
                    (kw["ws"], kw["wsb"]), = self._layer_ws(c, l, [f.fam], h.shape[1])
                if f.kp:
                    # training form of the FIRST layer: Ahat x [N, kp] and its output's sign pieces leave too, for the dense backward
                    c.xagg = (self._ws(bufs, "xagg", c.N * f.kp * 4, c.dev), self._ws(bufs, "signs", c.N * (c.D // 8), c.dev))
                    kw["xagg"], kw["signs"] = c.xagg
                if stream is not None:
                    kw["stream"] = stream
                f.fam.forward(geo, f.gpt, h, c.W[l], c.bs[l], 1, **kw)
        if c.side is not None:
            c.main.wait_stream(c.side)      # join: what follows waits for the side stream's launches too

    def _head(self, c: _Ctx):
        """The readout head as a launch of its own (one-launch kernel for D = 64 / 128, C <= 8; five launches of the
        any-shape kernels otherwise) -- reference model/gcn.py:70-71, utils/utils_model.py:64-65."""
        if len(c.lins) != 2:
            return self._head_deep(c)
        lib, bufs = _lib.load(), c.bufs
        p, stream, slope = _lib.ptr, _lib.stream_ptr(), HF.LEAKY_SLOPE
        B, D, C, (l0, l1) = c.B, c.D, c.C, c.lins
        W0, b0, W1, b1 = HF._f32c(l0.weight), HF._f32c(l0.bias), HF._f32c(l1.weight), HF._f32c(l1.bias)
        emb, z, out = bufs["emb"], bufs["z"], bufs["out"]
        if c.head_fused:
            rc = lib.hcg_head_fwd_bwd(p(emb), p(c.y2), p(W0), p(b0), p(W1), p(b1), B, D, C, slope,
                                      self._head_flags(c), p(z), p(out), p(bufs["demb"]),
                                      p(bufs["ws_head"]), bufs["ws_head_bytes"], p(c.step_word), stream)
            _lib.check(rc, "hcg_head_fwd_bwd")
            g = (lambda q: self._g(c, q)) if not c.forward_only else (lambda q: None)
            _lib.check(lib.hcg_head_reduce_job(p(bufs["ws_head"]), bufs["ws_head_bytes"], B, D, C, g(l0.weight), g(l0.bias),
                                               g(l1.weight), g(l1.bias), c.jobs.slot()), "hcg_head_reduce_job")
            c.jobs.n += 1
            return
        # any-shape head (widths other than 64 / 128, more than 8 classes): Linear + LeakyReLU, Linear, loss with its
        # (scaled) gradient, two Linear backwards that write straight into the flat gradient buffer
        hb = self._head_buffers(bufs, B, D, C, c.dev)
        tail = self._flat_ext[c.flat.numel():] if c.sse_split else None
        _lib.check(lib.hcg_linear_fwd(p(emb), p(W0), p(b0), p(z), B, 2 * D, D, _lib.HCG_ACT_LEAKY, slope, stream), "hcg_linear_fwd")
        _lib.check(lib.hcg_linear_fwd(p(z), p(W1), p(b1), p(out), B, D, C, _lib.HCG_ACT_NONE, slope, stream), "hcg_linear_fwd")
        if c.loss_mode == _lib.HCG_LOSS_CE:
            _lib.ce_fwd_bwd(out, c.y2, bufs["loss"], None if c.forward_only else hb["dout"])
        else:
            _lib.check(lib.hcg_loss_fwd_bwd(p(out), p(c.y2), B * C, c.loss_mode, p(bufs["loss"]), p(hb["dout"]), p(tail),
                                            stream), "hcg_loss_fwd_bwd")
        if c.forward_only:
            return
        g = lambda q: self._g(c, q)
        _lib.check(lib.hcg_linear_bwd(p(hb["dout"]), p(out), p(z), p(W1), p(hb["dz"]), g(l1.weight), g(l1.bias), p(hb["dz_ws1"]),
                                      B, D, C, _lib.HCG_ACT_NONE, slope, p(hb["ws1"]), hb["ws1"].numel(), stream), "hcg_linear_bwd")
        _lib.check(lib.hcg_linear_bwd(p(hb["dz"]), p(z), p(emb), p(W0), p(bufs["demb"]), g(l0.weight), g(l0.bias), p(hb["dz_ws0"]),
                                      B, 2 * D, D, _lib.HCG_ACT_LEAKY, slope, p(hb["ws0"]), hb["ws0"].numel(), stream), "hcg_linear_bwd")

    @staticmethod
    def _head_flags(c: _Ctx) -> int:
        return ((_lib.HCG_HEAD_FORWARD_ONLY if c.forward_only else 0)
                | (_lib.HCG_HEAD_LOSS_CE if c.loss_mode == _lib.HCG_LOSS_CE else 0))

    def _head_deep(self, c: _Ctx):
        """Readout depth 1, 3 or 4: one launch with the contract of `hcg_head_fwd_bwd` (csrc/head.hip: k_head_deep), its
        slabs ONE reduction job -- each layer's bias gradient sits right behind its weight gradient in the flat buffer."""
        lib, bufs, R = _lib.load(), c.bufs, len(c.lins)
        a = _lib.HeadArgs()
        a.emb, a.y, a.out = bufs["emb"].data_ptr(), c.y2.data_ptr(), bufs["out"].data_ptr()
        wb = [(HF._f32c(lin.weight), HF._f32c(lin.bias)) for lin in c.lins]     # (held until the launch is enqueued)
        for i, (W, b) in enumerate(wb):
            a.W[i], a.b[i] = W.data_ptr(), b.data_ptr()
        a.demb = None if c.forward_only else bufs["demb"].data_ptr()
        a.workspace, a.workspace_bytes = bufs["ws_head"].data_ptr(), bufs["ws_head_bytes"]
        a.step_counter = _lib.ptr(c.step_word)
        if not c.forward_only:
            for i, lin in enumerate(c.lins):
                a.grad[i] = self._g(c, lin.weight)
                if self._g(c, lin.bias) != a.grad[i] + 4 * lin.weight.numel():      # (parameter order keeps them adjacent)
                    raise _lib.HcgError("readout bias gradient not directly behind its weight's in the flat buffer")
        a.B, a.D, a.C, a.R = c.B, c.D, c.C, R
        a.flags, a.slope = self._head_flags(c), HF.LEAKY_SLOPE
        _lib.check(lib.hcg_head_deep_fwd_bwd(ctypes.addressof(a), c.jobs.slot(), _lib.stream_ptr()), "hcg_head_deep_fwd_bwd")
        c.jobs.n += 1

    def _backward_layers(self, c: _Ctx):
        """Conv stack backward, last layer first, each layer in the form the plan gave it on each part (`LayerForm.flags`: who
        applies which activation derivative).  A layer's slabs are ONE reduction job: later parts' descriptors join the first's."""
        bufs, jobs, parts, D = c.bufs, c.jobs, c.parts, c.D
        acts, top = bufs["acts"], c.n_conv - 1
        append = _lib.load().hcg_reduce_job_append if len(parts) > 1 else None

        def reduce(l, fams, slabs):
            F, dW, db = c.W[l].shape[1], self._g(c, c.W[l]), self._g(c, c.bs[l])
            for p, fam, (ws, wsb) in zip(parts, fams, slabs):
                kw = dict(first=True) if p.forms[l].kp else {}
                if p is parts[0]:
                    jobs.n += fam.reduce_jobs(p.geo, p.forms[l].gpt, F, D, ws, wsb, dW, db, jobs.slot(), **kw)
                else:           # (one job per part and layer at the grouping's width: `step_parts`)
                    fam.reduce_jobs(p.geo, p.forms[l].gpt, F, D, ws, wsb, dW, db, jobs.spare, **kw)
                    _lib.check(append(jobs.slot() - HF._JOB_BYTES, jobs.spare), "hcg_reduce_job_append")

        if c.side is not None:
            c.side.wait_stream(c.main)
        for l in reversed(range(c.n_conv)):
            last, inp, slabs = l == top, (c.x if l == 0 else acts[l - 1]), None
            for i, (geo, forms, stream) in enumerate(parts):
                # the gradient comes in from the head (demb) or the layer above (its dx), goes out as dx; of its own output the
                # layer reads nothing where the pooled bits / the dense form's sign pieces stand in, or dout came premasked
                f, bits = forms[l], (c.poolbits[i] if last else None)
                kw = dict(dout=None if last else bufs["dacts"][l], demb=bufs["demb"] if last else None,
                          emb=bufs["emb"] if (last and bits is None) else None,
                          out=acts[l] if (bits is None and not f.kp and (last or f.flags & 1)) else None,
                          dx=bufs["dacts"][l - 1] if l > 0 else None)
                if bits is not None:
                    kw["poolbits"] = bits
                if f.pair == "upper" and c.bwd_pair:
                    # layers 1 and 0 in ONE launch: layer 1's phase, a workgroup barrier, layer 0's phase over the same tiles
                    fams, up, low = [f.fam], self._layer_ws(c, 1, [f.fam], D), self._layer_ws(c, 0, [f.fam], c.F)
                    f.fam.backward_pair(geo, f.gpt, c.x, c.W[0], inp, c.W[1], f.flags, ws_up=up[0][0], wsb_up=up[0][1],
                                        ws=low[0][0], wsb=low[0][1], **kw)
                    reduce(1, fams, up)
                    reduce(0, fams, low)
                    return          # (a pair is the whole batch: one part, nothing to join)
                if slabs is None:
                    # (a dense first layer's backward is ONE launch over the forward's Ahat x: the wide-layer route's launcher)
                    fams = [HF.TALL if p.forms[l].kp else p.forms[l].fam for p in parts]
                    slabs = self._layer_ws(c, l, fams, inp.shape[1])
                if f.kp:
                    kw.update(xagg=c.xagg[0], signs=c.xagg[1])
                    if not f.fam.row_streaming:
                        # the node count is read on the device (graph_ptr[B]): a captured epoch's slot has a CAPACITY of rows
                        kw["nodes_dev"] = geo.graph_ptr + 4 * geo.B
                if stream is not None:
                    kw["stream"] = stream
                fams[i].backward(geo, f.gpt, inp, c.W[l], f.flags, ws=slabs[i][0], wsb=slabs[i][1], **kw)
            reduce(l, fams, slabs)
        if c.side is not None:
            c.main.wait_stream(c.side)

    def _tail(self, c: _Ctx):
        """The step's last launch: slab reductions -> ONE flat gradient, the loss and its scale, (exchange,) update, the next
        batch's plan.  With a collective between backward and update the launch stops at the gradient."""
        opt, bufs = self.model.optimizer, c.bufs
        count = self._loss_count(c)
        self._last_carried = c.step_word is not None
        if c.step_word is not None:
            if self.exchange is not None and self.pre_exchange_hook is not None:
                self.pre_exchange_hook()
            if not opt.step_with_reduction(c.jobs.addr, c.jobs.n, c.flat, next_plan=self.next_plan, exchange=self.exchange,
                                           flat_ext=self._flat_ext, mode=self.combine, loss_buf=bufs["loss"],
                                           loss_mode=c.loss_mode, loss_count=count):
                raise _lib.HcgError("optimizer state changed between head launch and update")
            return
        sse_tail = self._flat_ext[c.flat.numel():] if (c.sse_split and c.head_fused) else None
        _lib.step_tail(c.jobs.addr, c.jobs.n, loss=bufs["loss"], loss_mode=c.loss_mode, loss_count=count, sse_tail=sse_tail)
        if self.next_plan is not None:
            self.next_plan.rebuild()                   # (no fused update to ride in: its own launch)
        if not self._capturing_split:
            self._exchange_and_update(bufs["loss"], c.sse_split)

    @staticmethod
    def _loss_count(c: _Ctx) -> float:
        """Terms of the head's partial sums: B * C squared errors, or B per-graph cross-entropy terms."""
        return float(c.B if c.loss_mode == _lib.HCG_LOSS_CE else c.B * c.C)

    def _finish_forward_only(self, c: _Ctx):
        """Forward-only steps (the reference's eval_network body, utils/utils_model.py:75-78): the loss from the head's SSE
        partials, one tiny launch."""
        if c.head_fused:
            _lib.check(_lib.load().hcg_loss_finalize(c.jobs.addr, self._loss_count(c), c.loss_mode, _lib.ptr(c.bufs["loss"]), None,
                                                     _lib.stream_ptr()), "hcg_loss_finalize")
        self.last_out = c.bufs["out"]
        return c.bufs["loss"][0]

    def evaluate(self, batch, _checked: bool = False):
        """Forward + loss only (the reference's `eval_network` body, utils/utils_model.py:75-78): nothing is reduced or
        updated."""
        return self(batch, _forward_only=True, _checked=_checked)

    def __call__(self, batch, _forward_only: bool = False, _checked: bool = False):
        if not _checked:                 # (the epoch loops below have just asked `reason(batch)` themselves)
            why = self.reason(batch)
            if why is not None:
                raise _lib.HcgError(f"FusedTrainStep does not cover this model/batch: {why}")
        c = self._prepare(batch, _forward_only)
        if self._head_in_forward(c):
            self._forward_with_head(c)
        else:
            self._forward_layers(c)
            self._head(c)                               # over all graphs
        if _forward_only:
            return self._finish_forward_only(c)
        self._backward_layers(c)
        self._tail(c)
        self.last_out = c.bufs["out"]
        return c.bufs["loss"][0]

    def _exchange_and_update(self, loss_buf, sse_split: Optional[bool] = None):
        """Behind the step tail when a collective sits between backward and update: gradient exchange (data parallel), the
        "sse" scale, the optimiser."""
        lib, opt, flat = _lib.load(), self.model.optimizer, self._flat
        sync = self.grad_sync
        if sync is None and self.exchange is not None:
            # a one-shot exchange is attached but this step's update is not the fused launch that carries it (any-shape head,
            # optimiser state not one flat group): the ranks exchange through the collective instead -- never not at all
            sync = self.exchange_fallback_sync
            if sync is None:
                raise _lib.HcgError("a one-shot exchange is attached, this step cannot carry it and no collective fallback is "
                                    "set: the replicas would diverge")
        if sse_split is None:
            sse_split = self.combine == "sse" and sync is not None
        if sse_split:
            ext = self._flat_ext
            if sync is not None:
                sync(ext)                                    # SUM of [gradients | SSE | count] over the ranks
            if self.optimizer_step and hasattr(opt, "step_sse"):
                self._flat_grads(self._trainable(), flat.device)
                opt.step_sse(ext, loss_buf)                  # scale + update, one launch
            else:
                _lib.update_dev(ext, n=flat.numel(), loss=loss_buf)     # the scale and the loss alone
                if self.optimizer_step:
                    opt.step()
            return
        if sync is not None:
            sync(flat)
        if self.optimizer_step:
            # the update reads the parameters' `.grad`: they must be views of THIS trainer's buffer (another trainer on
            # the same model may have re-pointed them since)
            self._flat_grads(self._trainable(), flat.device)
            opt.step()

    # ------------------------------------------------------------------ hipGraph
    def capture(self, batch, prefetch=None, next_plan=None):
        """Capture the step on `batch`'s tensors into a hipGraph; `replay()` re-runs it on whatever those tensors
        hold then (copy the next batch into them, or re-collate in place).  `batch` may be a callable returning the
        batch: whatever it enqueues (a device collate, the plan build of a fresh `Batch`) is captured too.  The optimiser switches to its
        device-side step counter / learning rate (`optim.FusedFlatOptimizer.enable_capturable`); the gradient exchange
        (`grad_sync`) is NOT captured: with one, the graph ends after the slab reduction and `replay()` issues the
        collective and the (single-launch) update eagerly behind it.
        `prefetch`: a callable whose launches are captured on a FORKED branch of the graph (forks at the start of the
        step, joins at its end): work for the NEXT step that does not depend on this one -- the next batch's plan build
        (`BatchPlan.rebuild`), a device collate -- runs beside this step instead of in front of the next.
        `next_plan`: sets `self.next_plan` (see `__init__`) for the captured step."""
        if next_plan is not None:
            self.next_plan = next_plan

        def get():
            if callable(batch):
                return batch()
            # a fixed Batch object: drop its cached plan so that the plan build (graph_ptr / edge_ptr from the int64
            # batch vector and edge_index) is enqueued -- and captured -- every time; replay() then follows whatever
            # graph boundaries the tensors hold.  max_nodes / max_edges of `batch` act as capacities.
            try:
                batch._hcg_plan = None
            except Exception:
                pass
            return batch
        # warm-up (two runs): every buffer allocated, optimiser state re-based
        cap = _Capture(self.model.optimizer if self.optimizer_step else None, True, lambda: (self(get()), self(get())))
        sync = orig_sync = self.grad_sync
        if sync is None and self.exchange is not None and not self._last_carried:
            sync = self.exchange_fallback_sync         # (this step's update cannot carry the one-shot exchange: collective form)
        split = sync is not None and not self.capture_exchange
        try:
            if split or sync is None:
                self.grad_sync = None
            self._capturing_split = split              # with an exchange, the graph ends after the slab reduction
                                                       # (unless `capture_exchange`: collective + update are recorded too)
            fork = torch.cuda.Stream() if prefetch is not None else None
            with cap.recording():
                if fork is not None:
                    main = torch.cuda.current_stream()
                    fork.wait_stream(main)
                    with torch.cuda.stream(fork):
                        prefetch()
                loss = self(get())
                if fork is not None:
                    main.wait_stream(fork)
        finally:
            self.grad_sync, self._capturing_split = orig_sync, False
        self._graph = (cap.graph, loss, split, self._graph_fingerprint())
        return self

    def _graph_fingerprint(self):
        """Addresses a captured graph has baked in and that later calls could replace: step buffers, flat gradient,
        the optimiser's flat parameter / state storages."""
        cap = self._bufs.get("cap")
        fp = [t.data_ptr() for t in cap["acts"] + cap["dacts"]] if cap else []
        if cap:      # kernel workspaces (slabs, pooled bits, the wide-layer kernels' dH buffer): they grow on demand
            fp += [(k if isinstance(k, (str, int)) else str(k), t.data_ptr()) for k, t in sorted(cap["ws"].items(), key=lambda kv: str(kv[0]))
                   if torch.is_tensor(t)]
            fp.append(cap["ws_head"].data_ptr())
        fp.append(self._flat.data_ptr() if getattr(self, "_flat", None) is not None else 0)
        opt = self.model.optimizer
        fl = getattr(opt, "_flat", {}).get(0) if self.optimizer_step else None
        if fl is not None:
            fp += [t.data_ptr() for t in [fl["p"]] + opt.flat_state(fl)]
        fp += [q.data_ptr() for q in self._trainable()]      # (cached walk: this runs on every replay)
        return tuple(fp)

    def replay(self):
        if self._graph is None:
            raise _lib.HcgError("replay(): no captured step (never captured, or its buffers were re-allocated by a larger "
                                "eager batch): call capture() again")
        g_main, loss, split, fp = self._graph
        if not _replayable((self,), (fp,), self.optimizer_step):
            self._graph = None
            raise _lib.HcgError("replay(): parameter / optimiser / step buffers changed since capture() "
                                "(load_state_dict, a larger eager batch): call capture() again")
        g_main.replay()
        if split:                                     # exchange between the captured backward and the update:
            self._exchange_and_update(loss_buf=self._bufs["cap"]["loss"])   # one collective, then ONE eager launch
        elif not self.optimizer_step:
            # gradients-only step: the parameters' `.grad` must be THIS trainer's buffer (another trainer on the same model
            # may have re-pointed them since the capture)
            self._flat_grads(self._trainable(), self._flat.device)
        return loss

    def drop_graph(self):
        self._graph = None

    def captured_loss(self):
        """The loss buffer the captured step writes, or None before any step ran on capture buffers."""
        cap = self._bufs.get("cap")
        return None if cap is None else cap["loss"]


class _Capture:
    """The capture protocol of a step and of a window of steps.  Making one is its first half: `opt`, the optimiser the steps
    update (None: none), must be a fused one and with `enable` switches to its device-side step count / learning rate;
    `warm_up()` runs on a side stream bracketed by the current one; the device is synchronised.  `with recording()`, the
    second, puts the block into `graph`; in between the caller settles what it learnt from the warm-up."""

    def __init__(self, opt, enable, warm_up):
        if opt is not None:
            if not hasattr(opt, "enable_capturable"):
                raise _lib.HcgError("capturing steps with optimizer_step needs a fused optimiser of hcatgnet_amd.optim "
                                    "(FusedAdam, FusedSGD, FusedRMSprop)")
            if enable:
                opt.enable_capturable()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            warm_up()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()

    def recording(self):
        # (a live process group has helper threads that query events: their calls must not fail this capture)
        mode = "thread_local" if (torch.distributed.is_available() and torch.distributed.is_initialized()) else "global"
        return torch.cuda.graph(self.graph, capture_error_mode=mode)


def _replayable(steps, fingerprints, updates) -> bool:
    """Before a replay: False when an address the graph of `steps` has baked in was replaced, else the learning rate is synced."""
    for st, fp in zip(steps, fingerprints):
        if fp != st._graph_fingerprint():
            return False
    if updates:
        steps[0].model.optimizer.sync_lr()
    return True


@contextlib.contextmanager
def _taken_back(opt, extra=(), what="capture"):
    """A capture's warm-up runs every step once: hidden extra epochs.  They are undone: parameters, moments and the step count
    (re-based onto the optimiser's flat storages BEFORE the snapshot) and the `extra` tensors go back to what they were, in
    place (same storages, so the captured addresses stay valid) -- also when the capture fails, since the caller then trains
    on in another form.  The exchange stamp is never taken back.  Yields `restore()`, for the caller of several captures."""
    live = opt.capture_state()
    held = live + list(extra)
    saved = [t.clone() for t in held]

    def restore():
        torch.cuda.synchronize()
        with torch.no_grad():
            for t, u in zip(held, saved):
                t.copy_(u)
        torch.cuda.synchronize()
    try:
        yield restore
    finally:
        restore()
    if not opt.on_storages(live):
        raise _lib.HcgError(f"{what}: the optimiser re-based its state during the capture")


class StepWindow:
    """Several consecutive training steps as ONE hipGraph: `steps[i]` (a `FusedTrainStep`, all on the same model) run on
    `batches[i]` (a Batch, or a callable returning one), in order, the weights carried from step to step exactly as
    separate launches would.  What a window saves is the bubble between two graph launches (~3.7 us on MI355X / ROCm 7.2:
    C3 0.1152 -> 0.1115 ms/step, the reference's batch size 40 0.0713 -> 0.0675; `tools/exp_multistep_graph.py`) -- for a
    loader whose batches are known ahead (a resident dataset visited in a fixed or pre-drawn order), an epoch is one launch.
    Each step must be capturable on its own first (`FusedTrainStep.capture` has run, or would succeed): same launches, same
    device-side step count / learning rate, the next batch's plan inside each step's last launch if `next_plan` is set.
    A step whose gradient exchange is a separate collective (`grad_sync`) cannot sit inside a window.

        for i, st in enumerate(steps): st.capture(batch_fn[i], next_plan=plans[(i + 1) % n])
        window = StepWindow(steps, batch_fn);  losses = window.replay()      # one launch = n steps"""

    def __init__(self, steps, batches, forward_only: bool = False, counts64=None):
        """`forward_only`: the steps' `evaluate` form (plan, conv stack, head: loss only, nothing reduced or updated).
        `counts64` (float64 [len(steps)], graphs per batch): the epoch sum dot(losses, counts) -- `_weighted_loss_sum`, the same
        three operations -- and its copy into a pinned host scalar are recorded behind the last step, so reading an epoch's
        value is one stream synchronisation (`value()`), not four launches and a blocking copy."""
        steps, batches = list(steps), list(batches)
        if not steps or len(steps) != len(batches):
            raise ValueError("StepWindow needs as many batches as steps (at least one)")
        model = steps[0].model
        for st in steps:
            if st.model is not model:
                raise ValueError("the steps of a window train ONE model")
            if st.grad_sync is not None and not st.capture_exchange:
                raise _lib.HcgError("a step with a separate gradient collective (grad_sync) cannot be captured into a window "
                                    "(unless its `capture_exchange` is set: the collective is then recorded with the step)")
        self.steps, self.model, self.forward_only = steps, model, bool(forward_only)
        self.updates = steps[0].optimizer_step and not self.forward_only
        self.batches, self.counts64 = batches, counts64      # (kept alive: the graph reads their storages)
        # warm-up (every step once): every buffer allocated, optimiser state re-based, the sum's kernels loaded
        cap = _Capture(model.optimizer if any(st.optimizer_step for st in steps) else None, self.updates, self.run)
        self.value_host = None
        if counts64 is not None:
            self.value_host = torch.zeros(1, dtype=torch.float64).pin_memory()
            self.value_host.copy_(counts64[:1], non_blocking=True)       # (the copy's path taken before the capture)
            torch.cuda.synchronize()
        self.graph = cap.graph
        with cap.recording():
            self.losses, self.value_dev = self.run()
            if counts64 is not None:
                self.value_host.copy_(self.value_dev.reshape(1), non_blocking=True)
        self._fp = [st._graph_fingerprint() for st in steps]

    def run(self):
        """The steps once, in order, on the current stream (eager, or into a graph that is being recorded) -> their losses and
        dot(losses, counts64), a float64 device scalar (None without `counts64`)."""
        losses = [st(b() if callable(b) else b, _forward_only=self.forward_only) for st, b in zip(self.steps, self.batches)]
        return losses, (None if self.counts64 is None else _weighted_loss_dev(losses, self.counts64))

    def value(self) -> float:
        """dot(losses, counts64) of the last replay (needs `counts64`): waits for the current stream, reads the pinned scalar."""
        torch.cuda.current_stream().synchronize()
        return float(self.value_host[0])

    def replay(self):
        """-> the steps' loss tensors (device scalars, overwritten by the next replay)."""
        if not _replayable(self.steps, self._fp, self.updates):
            raise _lib.HcgError("StepWindow.replay(): parameter / optimiser / step buffers changed since the capture: build it again")
        self.graph.replay()
        return self.losses


class EpochWindow:
    """One training epoch of the reference's loop (utils/utils_model.py:55-70: every batch of a shuffled
    `DataLoader(dataset, batch_size, shuffle=True)`, call_methods.py:41-46, through zero_grad / forward / sqrt(MSE) /
    backward / Adam) as ONE hipGraph launch over a `store.DeviceLoader`.

    What makes an epoch capturable although its batches change shape with every shuffle: the NUMBER of batches and their
    graph counts are fixed (batch_size 40, options/base_options.py:269-274: 13 x 40 + 15 for 535 graphs), and every kernel
    of the fused step takes its sizes from graph_ptr / edge_ptr on the device, not from the launch arguments.  So every batch
    slot owns buffers of a fixed CAPACITY (the batch_size largest graphs of the dataset), the collate launch of slot i reads
    its graph ids and prefix sums from a fixed device buffer, and an epoch is: draw the permutation on the host (a few KB,
    the loader's own generator: the same sequence of permutations as iterating the loader), ONE host-to-device copy of the
    epoch's index arrays, ONE graph launch (collate + 4..6 launches per batch, weights carried from batch to batch), one
    reduction of the per-batch losses.  The per-batch loop of round 2 was host-bound at ~140 us per 77 us of kernels.

    Bitwise the per-batch loop on the same permutations (tests/test_gpu_train_step.py).  Applies when every layer of the
    model runs on a per-graph kernel family at capacity shape (not the dense row-streaming kernels of csrc/tall.hip, which
    walk all N rows of a batch); `build` returns None otherwise and the caller keeps its loop."""

    MAX_BATCHES = 64

    @staticmethod
    def build(model, loader):
        try:
            return EpochWindow(model, loader)
        except (_lib.HcgError, RuntimeError):       # refused, or the capture failed (memory, an unsupported launch)
            return None

    def __init__(self, model, loader):
        import numpy as np
        from .batch import Batch
        from .plan import BatchPlan
        from .store import epoch_layout, fill_collate_slot
        st = loader.store
        G, dev, F = len(st), st.device, st.F
        self.batching = (loader.batch_size, loader.drop_last)
        buf, spans, tot = epoch_layout(st.n_host, st.e_host, *self.batching, np.arange(G))
        if not spans or len(spans) > self.MAX_BATCHES or st.y_all is None:
            raise _lib.HcgError("EpochWindow: no batches, too many batches, or a dataset without targets")
        self.model, self.loader, self.G = model, loader, G
        self.Bs = [B for _, B, _ in spans]
        n_desc, e_desc = np.sort(st.n_host)[::-1], np.sort(st.e_host)[::-1]
        maxn, maxe = int(n_desc[0]), int(e_desc[0])
        self.host = torch.zeros(buf.size, dtype=torch.int64).pin_memory()
        self.dbuf = torch.zeros(buf.size, dtype=torch.int64, device=dev)
        d32 = self.dbuf[G:].view(torch.int32)
        self.batches, slots = [], []
        for i, B, off in spans:
            Ncap, Ecap = int(n_desc[:B].sum()), max(int(e_desc[:B].sum()), 1)
            x = torch.zeros(Ncap, F, dtype=torch.float32, device=dev)
            ei = torch.zeros(2, Ecap, dtype=torch.int64, device=dev)
            bvec = torch.zeros(Ncap, dtype=torch.int64, device=dev)
            y = torch.zeros(B, dtype=torch.float32, device=dev)
            idx = torch.zeros(B, dtype=torch.int64, device=dev) if st.idx_all is not None else None
            ids_d, gp_d, ep_d = self.dbuf[i:i + B], d32[off:off + B + 1], d32[2 * tot + off:2 * tot + off + B + 1]
            batch = Batch(x, ei, bvec, B, y=y, idx=idx, max_nodes=maxn, max_edges=maxe, edges_grouped=True)
            batch._hcg_plan = plan = BatchPlan.from_pointers(ei, bvec, gp_d, ep_d, Ncap, Ecap, B, maxn, maxe)
            shapes = [(Fl, D, "auto") for Fl, D, _ in _layer_shapes(model)]      # (whatever the conv's family preference)
            if any(f.fam.row_streaming for f in layer_forms(shapes, Ncap, maxn, maxe, plan=plan) or ()):
                raise _lib.HcgError("EpochWindow: a layer would run on the dense row-streaming kernels (capacity-padded rows)")
            self.batches.append(batch)
            slots.append(fill_collate_slot(_lib.CollateSlot(), ids_d, gp_d, ep_d, x, ei, bvec, y, idx, B, Ncap, Ecap))
        # ONE collate launch for the whole epoch, in front of its first step (every slot owns its buffers; the launch reads the
        # slot descriptors from a device array): a collate per batch was 14 launches of 40 workgroups, a tenth of the epoch
        arr = (_lib.CollateSlot * len(slots))(*slots)
        self.slots_dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
        src = st.collate_args()
        self.cargs = _lib.CollateArgs.from_buffer_copy(src)
        self.cargs.nslots, self.cargs.slots_dev, self.cargs.max_B = len(slots), _lib.ptr(self.slots_dev), max(self.Bs)
        if len(slots) == 1:
            self.cargs.slot = slots[0]

        def first_batch():
            _lib.check(_lib.load().hcg_collate(ctypes.byref(self.cargs), _lib.stream_ptr()), "hcg_collate")
            return self.batches[0]
        fns = [first_batch] + [(lambda b=b: b) for b in self.batches[1:]]
        self.steps = [FusedTrainStep(model) for _ in self.Bs]
        why = self.steps[0].reason(self.batches[0])
        if why is not None:
            raise _lib.HcgError(f"EpochWindow: {why}")
        self.counts = torch.tensor([float(B) for B in self.Bs], dtype=torch.float64, device=dev)
        self._layout(np.arange(G))
        for q in model.parameters():
            _lib.require_gpu(q)
        with _taken_back(model.optimizer, what="EpochWindow"):      # (the warm-up is a hidden extra epoch)
            self.window = StepWindow(self.steps, fns, counts64=self.counts)

    def _layout(self, order, staging=None):
        """The epoch's index arrays (`store.epoch_layout`) for the graphs in this order -> device, through the window's pinned
        buffer or `staging` (a pinned int64 row like `self.host`, the caller's to keep intact until the copy has run)."""
        from .store import epoch_layout
        st, host = self.loader.store, (self.host if staging is None else staging)
        epoch_layout(st.n_host, st.e_host, *self.batching, order, out=host.numpy())
        self.dbuf.copy_(host, non_blocking=True)

    def draw_order(self):
        """The next permutation of the loader's generator (what iterating the loader would have drawn)."""
        import numpy as np
        ld = self.loader
        return ld.rng.permutation(self.G) if ld.shuffle else np.arange(self.G)

    def launch_epoch(self, order=None, staging=None):
        """Issue the epoch on the current stream (index upload + ONE graph launch), no synchronisation; `finish_epoch` reads
        its value.  One epoch in flight per window (the pinned index buffer is rewritten by the next launch) -- unless every
        epoch in flight has a `staging` row of its own (`_layout`; fit.py keeps a ring of them)."""
        if order is None:
            order = self.draw_order()
        self._layout(order, staging)
        return self.window.replay()

    def finish_epoch(self, losses) -> float:
        """-> sum(loss_i * num_graphs_i) / len(dataset), the reference's `train_network` return value (synchronises)."""
        return self.window.value() / self.G        # (the sync also keeps the pinned index buffer from being rewritten too early)

    def run_epoch(self, order=None) -> float:
        return self.finish_epoch(self.launch_epoch(order))


# ---------------------------------------------------------------------------------------------------------------
# the reference's loops (same names / arguments / return values)
# ---------------------------------------------------------------------------------------------------------------
def _rmse_autograd(model, batch):
    """The batch's loss through autograd, for models / batches outside the fused step: the reference's
    sqrt(MSELoss(out, y.unsqueeze(1))); for a classification model, CrossEntropyLoss(out, y.long()) (no sqrt, no unsqueeze:
    see `FusedTrainStep`)."""
    out = model(batch)
    if _is_cross_entropy(model):
        return model.loss(out, batch.y.long())
    return torch.sqrt(model.loss(out, batch.y.unsqueeze(1)))


class _EpochSum:
    """sum(loss_i * num_graphs_i) of an epoch, on the device, in float64 like the reference's Python-float accumulation
    (`loss.item() * batch.num_graphs`, utils/utils_model.py:68): the per-batch losses are kept (one tiny copy each, no
    sync) and meet in ONE dot product at the end of the epoch -- the same operation the one-graph epoch forms
    (`EpochWindow`, `_build_eval_window`) apply to their loss buffers, so both forms return bitwise the same value."""

    def __init__(self):
        self.vals, self.ns = [], []

    def add(self, loss, num_graphs):
        self.vals.append(loss.detach().clone())
        self.ns.append(float(num_graphs))

    def value(self, denom) -> float:
        if not self.vals:
            return 0.0
        return _weighted_loss_sum(self.vals, torch.tensor(self.ns, dtype=torch.float64, device=self.vals[0].device)) / denom


def _weighted_loss_dev(losses, counts64):
    return torch.dot(torch.stack([v.reshape(()) for v in losses]).double(), counts64)


def _weighted_loss_sum(losses, counts64) -> float:
    """One synchronising read: dot(losses, counts) in float64."""
    return float(_weighted_loss_dev(losses, counts64).item())


def train_network(model, train_loader, device):
    """reference utils/utils_model.py:55-70: one epoch; returns sum(loss * num_graphs) / len(dataset).
    The per-batch `loss.item()` of the reference is replaced by a device-side accumulation and ONE sync."""
    model.train()
    fused = _fused_of(model)
    got = _EPOCH_WINDOWS.launch(model, train_loader)
    if got is not None:
        return got[0].finish_epoch(got[1])
    total = _EpochSum()
    for batch in train_loader:
        batch = batch.to(device)
        if fused.reason(batch) is None:
            loss = fused(batch, _checked=True)
        else:
            model.optimizer.zero_grad()
            loss = _rmse_autograd(model, batch)
            loss.backward()
            model.optimizer.step()
            loss = loss.detach()
        total.add(loss, batch.num_graphs)
    return total.value(len(train_loader.dataset))


EPOCH_WINDOW = True      # train_network over a DeviceLoader: whole epochs as one hipGraph (EpochWindow); False = per-batch loop


class _LoaderWindows:
    """One kind of captured window that a `store.DeviceLoader` keeps for a model: ONE entry (model, key, window or None) on
    its attribute `attr`.  `key(model, loader)`: what the window depends on besides the model, None = the kind does not
    apply; `build(model, loader)` -> window or None."""

    def __init__(self, attr, key, build, launch, draw=None):
        self.attr, self.key, self.build, self._launch, self.draw = attr, key, build, launch, draw

    def of(self, model, loader, build: bool = False):
        """The loader's window for this model, or None: there is none (`build`: make it now) or the kind does not apply.
        The model is compared by identity and held (an `id` can be reused); a None is kept like a window: what could not be
        built is not tried again for the same model and key.  A loader that refuses attributes keeps nothing."""
        key = self.key(model, loader)
        if key is None:
            return None
        ent = getattr(loader, self.attr, None)
        if ent is not None and ent[0] is model and ent[1] == key:
            return ent[2]
        if not build:
            return None
        win = self.build(model, loader)
        try:
            setattr(loader, self.attr, (model, key, win))
        except Exception:
            pass
        return win

    def launch(self, model, loader):
        """Issue the loader's window (built on first use) on the current stream -> (window, `launch(window, drawn)`), or None
        without one.  A launch that raises `HcgError` (parameters / optimiser re-based since the capture) drops the entry and
        is repeated ONCE on a rebuilt window; `draw(window)` runs once per call (an epoch's permutation: a rebuild skips none)."""
        drawn = None
        for attempt in range(2):
            win = self.of(model, loader, build=True)
            if win is None:
                return None
            try:
                if attempt == 0 and self.draw is not None:
                    drawn = self.draw(win)
                return win, self._launch(win, drawn)
            except _lib.HcgError:
                try:
                    setattr(loader, self.attr, None)
                except Exception:
                    return None
        return None


def dist_initialized_multi() -> bool:
    return torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1


def _epoch_window_key(model, loader):
    from .store import DeviceLoader
    if (not (EPOCH_WINDOW and isinstance(loader, DeviceLoader) and hasattr(model.optimizer, "enable_capturable"))
            or dist_initialized_multi()):    # (data parallel epochs keep the per-batch loop: the exchange form is the caller's)
        return None
    return (loader.batch_size, loader.drop_last, len(loader.store))


EVAL_WINDOW_MAX_BATCHES = 64


def _eval_window_key(model, loader):
    from .store import DeviceLoader
    if not (isinstance(loader, DeviceLoader) and not loader.shuffle and 0 < len(loader) <= EVAL_WINDOW_MAX_BATCHES):
        return None
    return (loader.batch_size, loader.drop_last, len(loader.store), bool(getattr(model, "use_fused", True)))


def _build_eval_window(model, loader):
    """A `store.DeviceLoader` that does not shuffle yields the same batches every epoch (the reference's validation / test
    loaders, call_methods.py:41-46): they are collated once, their `evaluate` steps captured as ONE hipGraph
    (`StepWindow(forward_only=True)`) and an `eval_network` call is one graph launch + one reduction instead of
    (collate + 3 launches) per batch.  -> the window, or None (a batch outside the fused step, a failed capture): the loop runs."""
    batches, fused = list(loader), _fused_of(model)
    if not all(fused.reason(b) is None for b in batches):
        return None
    try:
        steps = [FusedTrainStep(model, optimizer_step=False) for _ in batches]
        counts = torch.tensor([float(b.num_graphs) for b in batches], dtype=torch.float64, device=batches[0].x.device)
        return StepWindow(steps, batches, forward_only=True, counts64=counts)
    except (_lib.HcgError, RuntimeError):        # (memory, an unsupported launch)
        return None


_EPOCH_WINDOWS = _LoaderWindows("_hcg_epoch_window", _epoch_window_key, EpochWindow.build, EpochWindow.launch_epoch,
                                EpochWindow.draw_order)
_EVAL_WINDOWS = _LoaderWindows("_hcg_eval_window", _eval_window_key, _build_eval_window, lambda win, _: win.replay())
# (model, loader, build=False) -> the `EpochWindow` train_network / the forward-only `StepWindow` eval_network replays, or None
epoch_window_of, eval_window_of = _EPOCH_WINDOWS.of, _EVAL_WINDOWS.of


def eval_network(model, loader, device):
    """reference utils/utils_model.py:72-79 (forward + sqrt(MSE) per batch; no parameter update)."""
    model.eval()
    fused = _fused_of(model)
    got = _EVAL_WINDOWS.launch(model, loader)
    if got is not None:
        return got[0].value() / len(loader.dataset)
    total = _EpochSum()
    with torch.no_grad():
        for batch in loader:
            batch = batch.to(device)
            if fused.reason(batch) is None:
                loss = fused.evaluate(batch, _checked=True)
            else:
                loss = _rmse_autograd(model, batch)
            total.add(loss, batch.num_graphs)
    return total.value(len(loader.dataset))


def _kept_on(model, attr, make):
    """`model.attr`, made on first use (a model that refuses attributes gets a new one every time)."""
    v = getattr(model, attr, None)
    if v is None:
        v = make()
        try:
            setattr(model, attr, v)
        except Exception:
            pass
    return v


def _fused_of(model):
    return _kept_on(model, "_hcg_train_step", lambda: FusedTrainStep(model))


def _run_stream(model, device):
    """The HIP stream of an independent run (one per model)."""
    return _kept_on(model, "_hcg_run_stream", lambda: torch.cuda.Stream(device=device))


def train_networks(models, train_loaders, device, active=None):
    """One epoch of SEVERAL independent runs at once -> [train_network(model_k, loader_k, device) for every k] (None where
    `active[k]` is false: a run that has stopped early).

    The reference's nested cross-validation trains folds * (folds - 1) = 90 models one after another
    (scripts_experiments/train_GNN.py:48-50), each on ~535 graphs in batches of 40 (options/base_options.py:269-274): a
    batch of 40 graphs occupies 40 of the 256 CUs, so one run cannot fill the GPU whatever its kernels do.  The runs share
    nothing (own model, own optimiser, own loaders), so here every run issues its epoch -- ONE hipGraph (`EpochWindow`) --
    on its own HIP stream and the GPU overlaps them; the host synchronises once per run and epoch, after all of them are in
    flight.  Each run's arithmetic is untouched: bitwise what `train_network` gives that run alone
    (tests/test_gpu_train_step.py::test_concurrent_runs_equal_the_runs_one_by_one).  A run whose epoch does not fit the
    one-graph form (a host loader, a layer on the dense row-streaming kernels) is trained by `train_network` in turn."""
    return _run_networks("train_networks", models, train_loaders, device, active, lambda m: m.train(), _EPOCH_WINDOWS.launch,
                         lambda got, ld: got[0].finish_epoch(got[1]), train_network)


def eval_networks(models, loaders, device, active=None):
    """`eval_network` of several independent runs at once (see `train_networks`): every run's evaluation epoch -- one
    forward-only hipGraph over its fixed loader -- on the run's own stream.  -> [eval_network(model_k, loader_k, device)]."""
    return _run_networks("eval_networks", models, loaders, device, active, lambda m: m.eval(), _EVAL_WINDOWS.launch,
                         lambda got, ld: got[0].value() / len(ld.dataset), eval_network)


def _run_networks(name, models, loaders, device, active, set_mode, launch, finish, single):
    """One epoch of every active run on the run's own stream: `launch(model, loader)` issues it as one graph -> what
    `finish(got, loader)` turns into its value (synchronises), or None: `single(model, loader, device)` runs it in turn."""
    K = len(models)
    if len(loaders) != K or (active is not None and len(active) != K):
        raise ValueError(f"{name}: one loader (and one `active` flag) per model")
    out, flying = [None] * K, []
    cur = torch.cuda.current_stream(device)
    for k, (m, ld) in enumerate(zip(models, loaders)):
        if active is not None and not active[k]:
            continue
        set_mode(m)
        _fused_of(m)
        st = _run_stream(m, device)
        st.wait_stream(cur)                         # (whatever the caller did to this run's model on its own stream)
        with torch.cuda.stream(st):
            got = launch(m, ld)
        if got is None:
            out[k] = single(m, ld, device)
        else:
            flying.append((k, st, got, ld))
    for k, st, got, ld in flying:
        with torch.cuda.stream(st):
            out[k] = finish(got, ld)
        cur.wait_stream(st)
    return out


class _Predictions:
    """What the predict loops collect for M models over one loader, and the reference's result tuples made of it."""

    def __init__(self):
        self.y_pred, self.y_true, self.idx, self.embs = [], [], [], []

    def add(self, batch, out, emb=None):
        """`out` [M, graphs of the batch], `emb` [M, graphs, 2D] or None."""
        self.y_pred.append(out)
        self.y_true.append(batch.y.reshape(-1))
        self.idx.append(batch.idx.reshape(-1) if batch.idx is not None else torch.full((batch.num_graphs,), -1, device=out.device))
        if emb is not None:
            self.embs.append(emb)

    def results(self, return_emb: bool) -> list:
        """-> [(y_pred, y_true, idx[, embeddings DataFrame])], one per model."""
        y_pred = torch.cat(self.y_pred, 1).cpu().numpy()
        y_true = torch.cat(self.y_true).cpu().numpy().ravel()
        idx = torch.cat(self.idx).cpu().numpy().ravel()
        res = [(row.ravel(), y_true, idx) for row in y_pred]
        if return_emb:
            import pandas as pd
            for k, emb in enumerate(torch.cat(self.embs, 1).cpu().numpy()):
                frame = pd.DataFrame(emb)
                frame["ddG_exp"], frame["ddG_pred"], frame["index"] = y_true, res[k][0], idx
                res[k] += (frame,)
        return res


def predict_network(model, loader, return_emb: bool = False, device=None):
    """reference utils/utils_model.py:82-111: -> (y_pred, y_true, idx[, embeddings DataFrame]).
    The reference moves the model to the CPU for this; here it stays on the GPU (`device` defaults to the
    model's) and only the results come back.  The embeddings frame has the reference's columns: `0..2D-1`
    (graph_emb = [max, mean]), `ddG_exp`, `ddG_pred`, `index`."""
    model.eval()
    if device is None:
        device = next(model.parameters()).device
    got = _Predictions()
    with torch.no_grad():
        for batch in loader:
            batch = batch.to(device)
            out, emb = model(batch, True)
            got.add(batch, out.reshape(1, -1), emb[None] if return_emb else None)
    return got.results(return_emb)[0]


def predict_networks(models, loader, return_emb: bool = False, device=None):
    """`[predict_network(model_k, loader, return_emb, device) for model_k in models]` -- the same tuples and frames -- with ONE
    ensemble call per batch of the shared loader instead of one forward per model and batch (reference
    scripts_experiments/predict_test.py:19-103: every model of the nested cross-validation predicts the same set).  The
    ensemble is built from the models' weights at call time (`ensemble.EnsemblePredict`); models or batches outside its
    kernel run model by model inside it."""
    from .ensemble import EnsemblePredict
    models = list(models)
    for m in models:
        m.eval()
    if device is None:
        device = next(models[0].parameters()).device
    ens = EnsemblePredict(models)
    M = len(models)
    got = _Predictions()
    with torch.no_grad():
        for batch in loader:
            batch = batch.to(device)
            r = ens(batch, return_emb=return_emb, stats=False)
            got.add(batch, r.out.reshape(M, -1).clone(), r.emb.clone() if return_emb else None)
    return got.results(return_emb)
