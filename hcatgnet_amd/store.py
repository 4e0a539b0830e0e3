"""DeviceGraphStore / DeviceLoader: the dataset resident in HBM, batches collated ON the GPU.

Replaces, for this path, the reference's per-graph `torch.load` (data/datasets.py:74-78) and PyG
`DataLoader(dataset, batch_size, shuffle)` collate (call_methods.py:41-46): one gather launch per batch
(csrc/collate.hip), and because the host knows every graph's size the batch plan (graph_ptr / edge_ptr)
comes for free -- the batch object carries a ready `BatchPlan`, so the fused path launches no plan kernel.
"""
from __future__ import annotations

from typing import Iterable, Optional, Sequence

import ctypes

import numpy as np
import torch

from . import _lib
from .batch import Batch, Data
from .plan import BatchPlan


def epoch_layout(n_host, e_host, batch_size, drop_last, order, out=None):
    """The index arrays of one epoch over the graphs in `order` (`n_host` / `e_host`: nodes / edges of every graph): [ids of
    every batch | graph_ptr of every batch | edge_ptr of every batch] as int64 words -- the pointers are int32, two per
    word, every batch's block starts on a word: (B + 2) // 2 words hold B + 1.  `out`: an int64 buffer to refill instead.
    -> (buffer, [(i, B, off)]: batch order[i:i + B], its pointers at int32 offsets off and 2 * tot + off behind the ids, tot)."""
    G = len(order)
    Bs = [(i, min(batch_size, G - i)) for i in range(0, G, batch_size) if not (drop_last and G - i < batch_size)]
    tot = sum((B + 2) // 2 for _, B in Bs)
    buf = np.zeros(G + 2 * tot, np.int64) if out is None else out
    buf[:] = 0
    buf[:G] = order
    ptr32 = buf[G:].view(np.int32)
    cn, ce = np.cumsum(n_host[order]), np.cumsum(e_host[order])      # (over the epoch: a batch's prefix sums less its start's)
    spans, off = [], 0
    for i, B in Bs:
        ptr32[off + 1:off + B + 1] = cn[i:i + B] - (cn[i - 1] if i else 0)
        ptr32[2 * tot + off + 1:2 * tot + off + B + 1] = ce[i:i + B] - (ce[i - 1] if i else 0)
        spans.append((i, B, off))
        off += 2 * ((B + 2) // 2)
    return buf, spans, tot


_PCG_MULT, _M128, _M64 = 0x2360ED051FC65DA44385DF649FCCF645, (1 << 128) - 1, (1 << 64) - 1


def pcg64_permutation(state: dict, n: int):
    """`np.random.Generator(PCG64).permutation(n)` in plain Python integers: `state` = the generator's
    `bit_generator.state` dict -> (the permutation as a list, the state dict after the draw; `state` is not modified).
    csrc/shuffle.hip's draw restated (include/hcatgnet_hip.h: hcg_epoch_draw_args) and its CPU oracle: a Fisher-Yates shuffle
    from the top, every index `random_interval(i)` = masked rejection over 32-bit halves of pcg64's XSL-RR output, the high
    half of a 64-bit word kept for the next call."""
    if state.get("bit_generator") != "PCG64":
        raise ValueError(f"pcg64_permutation restates numpy's PCG64, not {state.get('bit_generator')!r}")
    s, inc = int(state["state"]["state"]), int(state["state"]["inc"])
    has, held = int(state["has_uint32"]), int(state["uinteger"])
    a = list(range(int(n)))
    for i in range(len(a) - 1, 0, -1):
        mask = (1 << i.bit_length()) - 1
        while True:
            if has:
                has, v = 0, held
            else:
                s = (s * _PCG_MULT + inc) & _M128
                x, rot = ((s >> 64) ^ s) & _M64, s >> 122
                w = ((x >> rot) | (x << ((64 - rot) & 63))) & _M64
                has, held, v = 1, w >> 32, w & 0xFFFFFFFF
            v &= mask
            if v <= i:
                break
        a[i], a[v] = a[v], a[i]
    return a, {"bit_generator": "PCG64", "state": {"state": s, "inc": inc}, "has_uint32": has, "uinteger": held}


def pcg64_to_struct(state: dict) -> "_lib.Pcg64":
    """numpy's PCG64 state dict -> the device struct's host mirror (hcg_pcg64)."""
    if state.get("bit_generator") != "PCG64":
        raise ValueError(f"the device generator is numpy's PCG64, not {state.get('bit_generator')!r}")
    s, inc, g = int(state["state"]["state"]), int(state["state"]["inc"]), _lib.Pcg64()
    g.state_lo, g.state_hi, g.inc_lo, g.inc_hi = s & _M64, s >> 64, inc & _M64, inc >> 64
    g.has_uint32, g.uinteger = int(state["has_uint32"]), int(state["uinteger"])
    return g


def pcg64_from_struct(g: "_lib.Pcg64") -> dict:
    """... and back: what `bit_generator.state = ` takes."""
    return {"bit_generator": "PCG64", "state": {"state": (int(g.state_hi) << 64) | int(g.state_lo),
                                                "inc": (int(g.inc_hi) << 64) | int(g.inc_lo)},
            "has_uint32": int(g.has_uint32), "uinteger": int(g.uinteger)}


class DeviceGenerator:
    """A `DeviceLoader`'s shuffle generator in device memory: `to_device()` moves `loader.rng`'s PCG64 state up, `draw(layout)`
    issues ONE launch (csrc/shuffle.hip) that draws the next permutation -- bit for bit `loader.rng.permutation(G)` -- and
    fills `layout` as `epoch_layout` would, `to_host()` brings the state back: `loader.rng.bit_generator.state` is then what
    numpy would hold after the same draws.  `reason(loader)`: why a loader has none (its generator is not numpy's PCG64, its
    store exceeds what one draw launch takes), else None."""

    @staticmethod
    def reason(loader) -> Optional[str]:
        rng = getattr(loader, "rng", None)
        if not isinstance(rng, np.random.Generator) or type(rng.bit_generator) is not np.random.PCG64:
            return "the loader's generator is not numpy's PCG64"
        if len(loader.store) > _lib.HCG_EPOCH_DRAW_MAX_GRAPHS:
            return f"more than {_lib.HCG_EPOCH_DRAW_MAX_GRAPHS} graphs (what one draw launch keeps in LDS)"
        return None

    def __init__(self, loader):
        why = self.reason(loader)
        if why is not None:
            raise _lib.HcgError(f"DeviceGenerator: {why}")
        self.loader, self.G = loader, len(loader.store)
        self.nbytes, self._words = ctypes.sizeof(_lib.Pcg64), None
        self.state_dev = torch.zeros(self.nbytes, dtype=torch.uint8, device=loader.store.device)
        self.args = a = _lib.EpochDrawArgs()
        a.rng, a.G, a.batch_size, a.drop_last = self.state_dev.data_ptr(), self.G, loader.batch_size, int(bool(loader.drop_last))

    def layout_words(self) -> int:
        """int64 words of the layout buffer a draw fills (`epoch_layout`'s)."""
        if self._words is None:
            self._words = epoch_layout(self.loader.store.n_host, self.loader.store.e_host, self.args.batch_size,
                                       bool(self.args.drop_last), np.arange(self.G))[0].size
        return self._words

    def to_device(self):
        """`loader.rng`'s state -> the device struct (a copy on the current stream)."""
        host = torch.frombuffer(bytearray(bytes(pcg64_to_struct(self.loader.rng.bit_generator.state))), dtype=torch.uint8)
        self.state_dev.copy_(host)
        return self

    def state(self) -> dict:
        """The device struct as numpy's state dict (synchronises)."""
        return pcg64_from_struct(_lib.Pcg64.from_buffer_copy(self.state_dev.cpu().numpy().tobytes()))

    def to_host(self):
        """The device struct -> `loader.rng` (synchronises)."""
        self.loader.rng.bit_generator.state = self.state()
        return self

    def draw(self, layout, gate=None, max_epochs: int = 0):
        """Enqueue one draw on the current stream: the next permutation and its index arrays into `layout` (int64 device
        buffer of `layout_words()`).  `gate`: the device tensor of a fit's `_lib.FitState` -- a stopped fit, or one whose
        epoch has reached `max_epochs`, draws nothing and leaves generator and layout as they are."""
        if layout.dtype != torch.int64 or layout.numel() < self.layout_words() or not layout.is_contiguous():
            raise ValueError("DeviceGenerator.draw: the layout buffer is int64, contiguous and at least layout_words() long")
        _lib.require_gpu(layout, self.state_dev, gate)
        a = self.args
        a.layout, a.gate, a.gate_max_epochs = layout.data_ptr(), _lib.ptr(gate), int(max_epochs)
        _lib.epoch_draw(self.loader.store.collate_args(), a)

    def order(self, layout):
        """The drawn order a layout buffer holds (synchronises)."""
        return layout[:self.G].cpu().numpy()


def fill_collate_slot(sl, ids, gp, ep, x, ei, bvec, y, idx, B, N, E):
    """Point a `_lib.CollateSlot` at one batch: the index views its gather reads, the tensors it writes."""
    p = _lib.ptr
    sl.ids, sl.graph_ptr, sl.edge_ptr, sl.x_out, sl.edge_index_out, sl.batch_out = p(ids), p(gp), p(ep), p(x), p(ei), p(bvec)
    sl.y_out, sl.idx_out, sl.B, sl.N_out, sl.E_out = p(y), p(idx), B, N, E
    return sl


class DeviceGraphStore:
    def __init__(self, graphs: Sequence[Data], device="cuda"):
        if len(graphs) == 0:
            raise ValueError("empty dataset")
        dev = torch.device(device)
        n = np.array([g.num_nodes for g in graphs], np.int64)
        e = np.array([g.num_edges for g in graphs], np.int64)
        self.num_graphs, self.F = len(graphs), int(graphs[0].x.shape[1])
        self.n_host, self.e_host = n, e
        self.node_ptr_host = np.concatenate([[0], np.cumsum(n)])
        self.edge_ptr_host = np.concatenate([[0], np.cumsum(e)])
        x = torch.cat([g.x.to(torch.float32) for g in graphs], 0)
        ei = torch.cat([g.edge_index for g in graphs], 1) if int(e.sum()) else torch.zeros(2, 0, dtype=torch.int64)
        for g in graphs:
            if g.num_edges and (int(g.edge_index.min()) < 0 or int(g.edge_index.max()) >= g.num_nodes):
                raise ValueError("edge_index of a graph refers to a node outside the graph")
        self.x_all = x.contiguous().to(dev)
        self.src_all = ei[0].to(torch.int32).contiguous().to(dev)
        self.dst_all = ei[1].to(torch.int32).contiguous().to(dev)
        self.node_ptr_all = torch.from_numpy(self.node_ptr_host).to(dev)
        self.edge_ptr_all = torch.from_numpy(self.edge_ptr_host).to(dev)
        ys = [getattr(g, "y", None) for g in graphs]
        self.y_all = torch.cat([torch.as_tensor(v, dtype=torch.float32).reshape(-1)[:1] for v in ys]).to(dev) \
            if all(v is not None for v in ys) else None
        ids = [getattr(g, "idx", None) for g in graphs]
        self.idx_all = torch.tensor([int(v) for v in ids], dtype=torch.int64, device=dev) if all(v is not None for v in ids) else None
        self.device = dev

    def __len__(self):
        return self.num_graphs

    def collate_args(self) -> "_lib.CollateArgs":
        """The dataset half of `hcg_collate`'s argument struct (made once; callers fill the slot half)."""
        a = getattr(self, "_collate_args", None)
        if a is None:
            p = _lib.ptr
            a = _lib.CollateArgs()
            a.x_all, a.src_all, a.dst_all, a.node_ptr_all, a.edge_ptr_all = (p(self.x_all), p(self.src_all), p(self.dst_all),
                                                                            p(self.node_ptr_all), p(self.edge_ptr_all))
            a.y_all, a.idx_all, a.F, a.nslots = p(self.y_all), p(self.idx_all), self.F, 1
            self._collate_args = a
        return a

    def collate(self, graph_ids: Iterable[int], _uploaded=None) -> Batch:
        """Batch of the given graphs (host list / array of indices), gathered on the device.
        `_uploaded` (DeviceLoader): device views (ids, graph_ptr, edge_ptr) of this batch inside ONE upload for the whole
        epoch -- otherwise the three index arrays of the batch go up here, one small copy each."""
        lib = _lib.load()
        ids = np.asarray(list(graph_ids) if not isinstance(graph_ids, np.ndarray) else graph_ids, np.int64)
        if ids.size == 0:
            raise ValueError("cannot collate an empty selection")
        if ids.min() < 0 or ids.max() >= self.num_graphs:
            raise IndexError("graph index out of range")
        B = int(ids.size)
        n, e = self.n_host[ids], self.e_host[ids]
        gp = np.zeros(B + 1, np.int32); gp[1:] = np.cumsum(n)
        ep = np.zeros(B + 1, np.int32); ep[1:] = np.cumsum(e)
        N, E = int(gp[-1]), int(ep[-1])
        dev = self.device
        if _uploaded is not None:
            ids_d, gp_d, ep_d = _uploaded
        else:
            ids_d = torch.from_numpy(ids).to(dev, non_blocking=True)
            gp_d = torch.from_numpy(gp).to(dev, non_blocking=True)
            ep_d = torch.from_numpy(ep).to(dev, non_blocking=True)
        x = torch.empty(N, self.F, dtype=torch.float32, device=dev)
        ei = torch.empty(2, E, dtype=torch.int64, device=dev)
        bvec = torch.empty(N, dtype=torch.int64, device=dev)
        y = torch.empty(B, dtype=torch.float32, device=dev) if self.y_all is not None else None
        idx = torch.empty(B, dtype=torch.int64, device=dev) if self.idx_all is not None else None
        a = self.collate_args()
        fill_collate_slot(a.slot, ids_d, gp_d, ep_d, x, ei, bvec, y, idx, B, N, E)
        _lib.check(lib.hcg_collate(ctypes.byref(a), _lib.stream_ptr()), "hcg_collate")
        batch = Batch(x, ei, bvec, B, y=y, idx=idx, max_nodes=int(n.max()), max_edges=int(e.max()), edges_grouped=True)
        # the plan of the fused path is exactly (graph_ptr, edge_ptr): attach it, nothing left to launch
        batch._hcg_plan = BatchPlan.from_pointers(ei, bvec, gp_d, ep_d, N, E, B, batch.max_nodes, batch.max_edges)
        return batch


class DeviceLoader:
    """`DataLoader(dataset, batch_size, shuffle)` over a DeviceGraphStore: the permutation is drawn on the
    host (a few KB), everything else happens on the GPU."""

    def __init__(self, store: DeviceGraphStore, batch_size: int = 1, shuffle: bool = False, seed: Optional[int] = None,
                 drop_last: bool = False):
        self.store, self.batch_size, self.shuffle, self.drop_last = store, int(batch_size), shuffle, drop_last
        self.rng = np.random.default_rng(seed)
        self.dataset = store       # `len(loader.dataset)` is what the reference's loops divide by (utils_model.py:70)

    def __len__(self):
        n = len(self.store)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        st = self.store
        order = self.rng.permutation(len(st)) if self.shuffle else np.arange(len(st))
        # the epoch's index arrays in ONE upload (`epoch_layout`): a batch then costs its gather launch and no host-to-device
        # copy of its own (three ~10 us copies per step otherwise)
        buf, spans, tot = epoch_layout(st.n_host, st.e_host, self.batch_size, self.drop_last, order)
        dbuf = torch.from_numpy(buf).to(st.device)
        d32 = dbuf[len(order):].view(torch.int32)
        for i, B, off in spans:
            yield st.collate(order[i:i + B], _uploaded=(dbuf[i:i + B], d32[off:off + B + 1],
                                                         d32[2 * tot + off:2 * tot + off + B + 1]))
