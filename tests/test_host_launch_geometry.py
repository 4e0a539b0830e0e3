"""Host tests (no GPU) of what the conv launchers' host code answers: which family takes a shape, how large its workspaces
are, every field of the reduction jobs it describes, and the code of every argument refusal.

Nothing is launched and no pointer is followed: the size queries and the job fillers only compute, and the refused calls
return before their launch.  Pointers are made-up, 256-aligned base addresses (one per buffer, `BASES`); a stored pointer is
recorded as "<buffer>+<byte offset>".  The answers are compared with tests/golden/launch_geometry.json, which was generated
by this file from the library of commit b5f3eea -- the last one whose launchers derived their geometry separately in every
entry point -- on a machine without a GPU, where the CU count falls back to 256, the MI355X's.  On a GPU that reports
another CU count the grids differ by design and the tests skip.

Regenerate (only when an answer is MEANT to change): build the library of the commit to pin, then on a machine without a GPU
    HCG_LIB=<that libhcatgnet_hip.so> HCG_WRITE_LAUNCH_GEOMETRY=<commit> python -m pytest tests/test_host_launch_geometry.py
The generator refuses to write a refusal case that was not refused (a code other than the three argument errors, or 0 where
the case is not an empty batch).

The refusal cases run only where no GPU is visible: a regression there would hand made-up addresses to a kernel.
"""
import ctypes
import itertools
import json
import os

import pytest

from hcatgnet_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_geometry.json")
WRITE = bool(os.environ.get("HCG_WRITE_LAUNCH_GEOMETRY"))
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -2, -3

# one made-up base address per buffer: k << 40, all 256-aligned and far apart
NAMES = ("null", "ws", "dW", "db", "dW0", "db0", "dW1", "db1", "x", "W", "b", "ei", "gp", "ep", "out", "emb", "st", "demb", "dout", "bits",
         "xagg", "sign", "dx", "W2", "b2", "out2", "y", "z", "hout", "hws", "ws2", "ndev")
BASES = {n: k << 40 for k, n in enumerate(NAMES)}
BASES["null"] = None


def _ptr(p):
    """A stored pointer as "<buffer>+<byte offset>" (None: NULL)."""
    if not p:
        return None
    k = p >> 40
    return "%s+%d" % (NAMES[k], p - (k << 40))


def _gpu_cu_count():
    try:
        import torch
        if not torch.cuda.is_available():
            return None
        return torch.cuda.get_device_properties(0).multi_processor_count
    except Exception:
        return None


CUS = _gpu_cu_count()
pytestmark = pytest.mark.skipif(CUS is not None and CUS != 256, reason="the golden grids are those of 256 CUs")


def _job_fields(job, all_segs=False):
    segs = []
    for s in list(job.seg)[:_lib.HCG_REDUCE_MAX_SEGS if all_segs else job.nseg]:
        segs += [s.begin, s.count, s.row_in, s.row_out, _ptr(s.dst)]
    return {"job": [_ptr(job.slabs), _ptr(job.sse_part), job.nslabs, job.slab_floats, job.nseg, job.reserved] + segs}


# ---- the small-graph tiles ----------------------------------------------------------------------------------------------
def tiles_rows():
    """[F, max_nodes, B, N] -> [graphs per tile, workspace bytes, aux bytes (poolbits), aux bytes (head), rc + job of
    hcg_fused_reduce_job, the same for an empty batch (N = 0), rc + job of hcg_fused_head_reduce_job with and without targets]"""
    lib = _lib.load()
    rows = []
    for F, mn in itertools.product((1, 25, 32, 33, 64, 65), (1, 16, 17, 32, 33)):
        gpt = lib.hcg_fused_graphs_per_tile(F, 64, mn)
        if gpt == 0:
            rows.append([F, mn, None, None, 0, lib.hcg_fused_workspace_bytes(2048, F, 64, 0), lib.hcg_fused_aux_bytes(0, 2048, 0),
                         lib.hcg_fused_aux_bytes(1, 2048, 0),
                         lib.hcg_fused_workspace_bytes(2048, F, 64, 2)])     # (and asked with a tile count all the same)
            continue
        # one workgroup, the grid cap and a partial last round, at 256 CUs x 8 waves
        for B in (0, 1, 8 * gpt, 8 * gpt + 1, 2048 * gpt, 2048 * gpt + 1, 2 * 2048 * gpt + 3):
            N = B * mn
            ws = lib.hcg_fused_workspace_bytes(B, F, 64, gpt)
            row = [F, mn, B, N, gpt, ws, lib.hcg_fused_aux_bytes(0, B, gpt), lib.hcg_fused_aux_bytes(1, B, gpt)]
            for n in (N, 0):
                job = _lib.ReduceJob()
                rc = lib.hcg_fused_reduce_job(BASES["ws"], ws, n, B, F, 64, gpt, BASES["dW"], BASES["db"], ctypes.addressof(job))
                row.append([rc] + ([_job_fields(job)] if rc == OK else []))
            hws = lib.hcg_fused_aux_bytes(1, B, gpt)
            for targets in (True, False):
                job = _lib.ReduceJob()
                t = [BASES[k] if targets else None for k in ("dW0", "db0", "dW1", "db1")]
                rc = lib.hcg_fused_head_reduce_job(BASES["hws"], hws, B, gpt, 3, *t, ctypes.addressof(job))
                row.append([rc] + ([_job_fields(job, all_segs=True)] if rc == OK else []))
            rows.append(row)
    return rows


# ---- one graph per workgroup / per wave -----------------------------------------------------------------------------------
MID_D, MID_F = (64, 128, 96), (1, 32, 33, 64, 65, 128, 129)
MID_NODES, MID_EDGES = (64, 65, 128, 129, 224, 225), (0, 256, 257, 1024, 1025)
MID_B = (1, 7, 8, 256, 257, 512, 513)


def mid_rows():
    """[D, F, max_nodes, max_edges, B] -> [hcg_mid_supported, workspace bytes, rc + job of hcg_mid_reduce_job for half 0 and 1]"""
    lib = _lib.load()
    rows = []
    for D, F, mn, me, B in itertools.product(MID_D, MID_F, MID_NODES, MID_EDGES, MID_B):
        sup = lib.hcg_mid_supported(F, D, mn, me)
        ws = lib.hcg_mid_workspace_bytes(B, F, D, mn, me)
        row = [D, F, mn, me, B, sup, ws]
        for half in (0, 1):
            job = _lib.ReduceJob()
            rc = lib.hcg_mid_reduce_job(BASES["ws"], ws, B, F, D, mn, me, half, BASES["dW"], BASES["db"], ctypes.addressof(job))
            row.append([rc] + ([_job_fields(job)] if rc == OK else []))
        rows.append(row)
    return rows


# ---- the wide-layer route ---------------------------------------------------------------------------------------------------
def tall_supported_rows():
    """[D, F, max_nodes, max_edges] -> hcg_tall_supported"""
    lib = _lib.load()
    return [[D, F, mn, me, lib.hcg_tall_supported(F, D, mn, me)] for D, F, mn, me in itertools.product(MID_D, MID_F, MID_NODES, MID_EDGES)]


def tall_rows():
    """[D, F, N, B] -> [workspace bytes, then per first_layer_form 0, 1: rc + the two jobs of hcg_tall_reduce_jobs]"""
    lib = _lib.load()
    rows = []
    for D, F, N, B in itertools.product(MID_D, MID_F, (1, 64, 65, 16384, 16385), MID_B):
        ws = lib.hcg_tall_workspace_bytes(N, B, F, D)
        row = [D, F, N, B, ws]
        for first in (0, 1):
            jobs = (_lib.ReduceJob * 2)()
            rc = lib.hcg_tall_reduce_jobs(BASES["ws"], ws, N, B, F, D, first, BASES["dW"], BASES["db"], ctypes.addressof(jobs))
            row.append([rc] + ([_job_fields(jobs[0]), _job_fields(jobs[1])] if rc == OK else []))
        rows.append(row)
    return rows


# ---- refusals ---------------------------------------------------------------------------------------------------------------
# Per launcher: the arguments of a call that WOULD launch (never made), and one variation per early return of the launcher
# (a third element `True`: the return is HCG_OK without a launch -- a batch without graphs or nodes, a query).  Where two
# checks could both fire, a variation with two faults pins their order.  A value that names a buffer stands for its made-up
# address.  Not covered: the returns behind a launch (hipGetLastError, the LDS limit of hcg_tall_layer_fwd, which follows its
# weight-split launch) and hipFuncSetAttribute's -- no argument reaches them without a device.
def _resolve(v):
    return BASES[v] if isinstance(v, str) else v


def _call(fn_name, order, base, change):
    kw = dict(base)
    kw.update(change)
    return getattr(_lib.load(), fn_name)(*[_resolve(kw[k]) for k in order])


BIG = 1 << 40      # workspace bytes that never fall short
NAN = float("nan")

MID_FWD_ORDER = ("x", "W", "b", "ei", "E", "gp", "ep", "N", "B", "F", "D", "mn", "me", "slope", "act", "out", "emb", "bits", "xagg", "sign",
                 "st", "stream")
MID_FWD_BASE = dict(x="x", W="W", b="b", ei="ei", E=900, gp="gp", ep="ep", N=1000, B=10, F=32, D=64, mn=100, me=300, slope=0.01, act=1,
                    out="out", emb=None, bits=None, xagg=None, sign=None, st="st", stream=None)
MID_FWD_CASES = [
    ("D", dict(D=96)), ("F", dict(F=129)), ("nodes", dict(mn=225)), ("edges", dict(me=1025)),
    ("xagg without signs", dict(xagg="xagg")), ("signs without xagg", dict(sign="sign")),
    ("xagg pooled", dict(xagg="xagg", sign="sign", emb="emb")), ("xagg bits", dict(xagg="xagg", sign="sign", bits="bits")),
    ("xagg D 128", dict(xagg="xagg", sign="sign", D=128)), ("xagg F 65", dict(xagg="xagg", sign="sign", F=65)),
    ("xagg no out", dict(xagg="xagg", sign="sign", out=None)), ("xagg on the wave kernels", dict(xagg="xagg", sign="sign", mn=64, me=256)),
    ("slope 1.5", dict(slope=1.5)), ("slope -0.1", dict(slope=-0.1)), ("slope nan", dict(slope=NAN)),
    ("N < 0", dict(N=-1)), ("B < 0", dict(B=-1)), ("E < 0", dict(E=-1)),
    ("empty B", dict(B=0), True), ("empty N", dict(N=0), True),
    ("no x", dict(x=None)), ("no W", dict(W=None)), ("no b", dict(b=None)), ("no graph_ptr", dict(gp=None)), ("no edge_ptr", dict(ep=None)),
    ("no out", dict(out=None)), ("no status", dict(st=None)), ("no edge_index", dict(ei=None)),
    ("bits without emb", dict(bits="bits")), ("bits F 65", dict(bits="bits", emb="emb", F=65)),
    ("bits on the wave kernels", dict(bits="bits", emb="emb", mn=64, me=256)),
    # order
    ("D, then xagg without signs", dict(D=96, xagg="xagg")), ("xagg without signs, then slope", dict(xagg="xagg", slope=2.0)),
    ("xagg pooled, then slope", dict(xagg="xagg", sign="sign", emb="emb", slope=2.0)), ("slope, then N < 0", dict(slope=2.0, N=-1)),
    ("N < 0, then empty B", dict(N=-1, B=0)), ("empty B before no x", dict(B=0, x=None), True), ("no x, then bits without emb", dict(x=None, bits="bits")),
]

MID_BWD_ORDER = ("dout", "demb", "emb", "out", "x", "W", "ei", "E", "gp", "ep", "N", "B", "F", "D", "mn", "me", "slope", "act", "dx", "st",
                 "ws", "wsb", "stream")
MID_BWD_BASE = dict(dout="dout", demb=None, emb=None, out="out", x="x", W="W", ei="ei", E=900, gp="gp", ep="ep", N=1000, B=10, F=32, D=64,
                    mn=100, me=300, slope=0.01, act=1, dx="dx", st="st", ws="ws", wsb=BIG, stream=None)
MID_BWD_CASES = [
    ("D", dict(D=96)), ("nodes", dict(mn=225)),
    ("N = 0", dict(N=0)), ("B = 0", dict(B=0)), ("E < 0", dict(E=-1)), ("no W", dict(W=None)), ("no workspace", dict(ws=None)),
    ("no x", dict(x=None)), ("no graph_ptr", dict(gp=None)), ("no edge_ptr", dict(ep=None)), ("no status", dict(st=None)),
    ("no edge_index", dict(ei=None)),
    ("pooled without demb", dict(dout=None, emb="emb")), ("pooled without emb", dict(dout=None, demb="demb")),
    ("act bits", dict(act=4)), ("premask without dx", dict(act=3, dx=None)), ("act without out", dict(out=None)),
    ("pooled without out", dict(dout=None, demb="demb", emb="emb", act=0, out=None)),
    ("workspace short", dict(wsb=None)), ("workspace short, wave kernels", dict(wsb=None, mn=64, me=256)),
    # order
    ("D, then no W", dict(D=96, W=None)), ("no W, then act bits", dict(W=None, act=4)), ("act bits, then workspace short", dict(act=4, wsb=None)),
    ("act without out, then workspace short", dict(out=None, wsb=None)),
]

TALL_FWD_ORDER = MID_FWD_ORDER[:-1] + ("ws", "wsb", "stream")
TALL_FWD_BASE = dict(MID_FWD_BASE, D=128, ws="ws", wsb=BIG)
TALL_FWD_CASES = [
    ("D", dict(D=96)), ("F not a multiple of 4", dict(F=33)), ("nodes", dict(mn=225)), ("edges", dict(me=1025)),
    ("D 64 goes to mid: its refusal", dict(D=64, slope=2.0)), ("D 64 up to 64 nodes", dict(D=64, mn=64)),
    ("xagg without signs", dict(xagg="xagg")), ("signs without xagg", dict(sign="sign")),
    ("xagg pooled", dict(xagg="xagg", sign="sign", emb="emb")), ("xagg bits", dict(xagg="xagg", sign="sign", bits="bits")),
    ("xagg no out", dict(xagg="xagg", sign="sign", out=None)), ("bits without emb", dict(bits="bits")),
    ("slope 1.5", dict(slope=1.5)), ("slope nan", dict(slope=NAN)),
    ("N < 0", dict(N=-1)), ("B < 0", dict(B=-1)), ("E < 0", dict(E=-1)),
    ("empty B", dict(B=0), True), ("empty N", dict(N=0), True),
    ("no x", dict(x=None)), ("no W", dict(W=None)), ("no b", dict(b=None)), ("no graph_ptr", dict(gp=None)), ("no edge_ptr", dict(ep=None)),
    ("no out", dict(out=None)), ("no status", dict(st=None)), ("no workspace", dict(ws=None)), ("no edge_index", dict(ei=None)),
    ("workspace short", dict(wsb=None)), ("N too large", dict(N=(1 << 30) + 1)),
    # order
    ("xagg without signs, then bits without emb", dict(xagg="xagg", bits="bits")), ("bits without emb, then slope", dict(bits="bits", slope=2.0)),
    ("slope, then N < 0", dict(slope=2.0, N=-1)), ("no x, then workspace short", dict(x=None, wsb=None)),
    ("workspace short, then N too large", dict(wsb=1 << 20, N=(1 << 30) + 1)),
]

TALL_BWD_ORDER = ("dout", "demb", "emb", "out", "bits", "xagg", "sign", "ndev", "x", "W", "ei", "E", "gp", "ep", "N", "B", "F", "D", "mn", "me",
                  "slope", "act", "dx", "st", "ws", "wsb", "stream")
TALL_BWD_BASE = dict(dout="dout", demb=None, emb=None, out="out", bits=None, xagg=None, sign=None, ndev=None, x="x", W="W", ei="ei", E=900,
                     gp="gp", ep="ep", N=1000, B=10, F=32, D=128, mn=100, me=300, slope=0.01, act=1, dx="dx", st="st", ws="ws", wsb=BIG,
                     stream=None)
TALL_BWD_CASES = [
    ("D", dict(D=96)), ("F not a multiple of 4", dict(F=33)), ("D 64 up to 64 nodes", dict(D=64, mn=64)),
    ("N = 0", dict(N=0)), ("B = 0", dict(B=0)), ("E < 0", dict(E=-1)), ("no W", dict(W=None)), ("no workspace", dict(ws=None)),
    ("no x", dict(x=None)), ("no graph_ptr", dict(gp=None)), ("no edge_ptr", dict(ep=None)), ("no status", dict(st=None)),
    ("no edge_index", dict(ei=None)), ("N too large", dict(N=(1 << 30) + 1)),
    ("bits with dout", dict(bits="bits")), ("xagg without signs", dict(xagg="xagg")), ("signs without xagg", dict(sign="sign")),
    ("first-layer form with dx", dict(xagg="xagg", sign="sign")), ("first-layer form pooled", dict(xagg="xagg", sign="sign", dx=None, dout=None)),
    ("first-layer form, workspace short", dict(xagg="xagg", sign="sign", dx=None, wsb=None)),
    ("pooled without demb", dict(dout=None, emb="emb")), ("pooled without emb or bits", dict(dout=None, demb="demb")),
    ("act bits", dict(act=4)), ("premask without dx", dict(act=3, dx=None)), ("act without out", dict(out=None)),
    ("pooled without out", dict(dout=None, demb="demb", emb="emb", act=0, out=None)),
    ("workspace short", dict(wsb=None)), ("workspace short, D 64", dict(wsb=None, D=64)),
    # order
    ("no W, then N too large", dict(W=None, N=(1 << 30) + 1)), ("N too large, then bits with dout", dict(N=(1 << 30) + 1, bits="bits")),
    ("bits with dout, then xagg without signs", dict(bits="bits", xagg="xagg")),
    ("first-layer form with dx, then workspace short", dict(xagg="xagg", sign="sign", wsb=None)),
    ("act bits, then workspace short", dict(act=4, wsb=None)),
]

FUSED_BWD_ORDER = ("dout", "demb", "emb", "out", "bits", "x", "W", "ei", "E", "gp", "ep", "N", "B", "F", "D", "gpt", "slope", "act", "dx", "st",
                   "ws", "wsb", "stream")
FUSED_BWD_BASE = dict(dout="dout", demb=None, emb=None, out="out", bits=None, x="x", W="W", ei="ei", E=900, gp="gp", ep="ep", N=1000, B=100,
                      F=32, D=64, gpt=2, slope=0.01, act=1, dx="dx", st="st", ws="ws", wsb=BIG, stream=None)
FUSED_BWD_CASES = [
    ("bits with dout", dict(bits="bits", demb="demb")), ("bits with emb", dict(bits="bits", dout=None, out=None, demb="demb", emb="emb")),
    ("bits with out", dict(bits="bits", dout=None, demb="demb")), ("bits without demb", dict(bits="bits", dout=None, out=None)),
    ("D", dict(D=128)), ("F = 0", dict(F=0)), ("F", dict(F=65)), ("graphs per tile", dict(gpt=0)),
    ("N < 0", dict(N=-1)), ("B < 0", dict(B=-1)), ("E < 0", dict(E=-1)), ("no W", dict(W=None)), ("no workspace", dict(ws=None)),
    ("pooled without demb", dict(dout=None, emb="emb")), ("pooled without emb", dict(dout=None, demb="demb")),
    ("act bits", dict(act=4)), ("premask without dx", dict(act=3, dx=None)),
    ("act without out", dict(out=None)), ("pooled without out", dict(dout=None, demb="demb", emb="emb", act=0, out=None)),
    ("no x", dict(x=None)), ("no graph_ptr", dict(gp=None)), ("no edge_ptr", dict(ep=None)), ("no status", dict(st=None)),
    ("no edge_index", dict(ei=None)), ("workspace short", dict(wsb=None)),
    ("empty N", dict(N=0, wsb=0), True), ("empty B", dict(B=0, wsb=0), True), ("empty N without x", dict(N=0, x=None, out=None, wsb=0), True),
    # order
    ("bits with dout, then D", dict(bits="bits", demb="demb", D=128)), ("D, then no W", dict(D=128, W=None)),
    ("no W, then act bits", dict(W=None, act=4)), ("no x, then workspace short", dict(x=None, wsb=None)),
]


def _mid_ws_short(kw):
    lib = _lib.load()
    return lib.hcg_mid_workspace_bytes(kw["B"], kw["F"], kw["D"], kw["mn"], kw["me"]) - 1


def _tall_ws_short(kw):
    return _lib.load().hcg_tall_workspace_bytes(kw["N"], kw["B"], kw["F"], kw["D"]) - 1


def _fused_ws_short(kw):
    return _lib.load().hcg_fused_workspace_bytes(kw["B"], kw["F"], kw["D"], kw["gpt"]) - 256 - 1


LAUNCHERS = [
    ("hcg_mid_layer_fwd", MID_FWD_ORDER, MID_FWD_BASE, MID_FWD_CASES, None),
    ("hcg_mid_layer_bwd", MID_BWD_ORDER, MID_BWD_BASE, MID_BWD_CASES, _mid_ws_short),
    ("hcg_tall_layer_fwd", TALL_FWD_ORDER, TALL_FWD_BASE, TALL_FWD_CASES, _tall_ws_short),
    ("hcg_tall_layer_bwd", TALL_BWD_ORDER, TALL_BWD_BASE, TALL_BWD_CASES, _tall_ws_short),
    ("hcg_fused_layer_bwd", FUSED_BWD_ORDER, FUSED_BWD_BASE, FUSED_BWD_CASES, _fused_ws_short),
]

# hcg_fused_forward takes a block: field -> value, both modes
FWD_BLOCK = dict(x="x", W1="W", b1="b", edge_index="ei", E=900, graph_ptr="gp", edge_ptr="ep", N=1000, B=100, F=32, D=64, graphs_per_tile=2,
                 apply_act=1, slope=0.01, out1="out", status="st", mode=0)
HEAD_BLOCK = dict(FWD_BLOCK, W2="W2", b2="b2", emb="emb", poolbits="bits", y="y", head_W0="dW0", head_b0="db0", head_W1="dW1", head_b1="db1",
                  C=1, z="z", out="hout", demb="demb", head_workspace="hws", head_workspace_bytes=BIG)
FWD_CASES = [
    ("mode", dict(mode=2)), ("D", dict(D=128)), ("F = 0", dict(F=0)), ("F", dict(F=65)), ("graphs per tile", dict(graphs_per_tile=0)),
    ("slope 1.5", dict(slope=1.5)), ("slope -0.1", dict(slope=-0.1)), ("slope nan", dict(slope=NAN)),
    ("N < 0", dict(N=-1)), ("B < 0", dict(B=-1)), ("E < 0", dict(E=-1)), ("empty B", dict(B=0), True), ("empty N", dict(N=0), True),
    ("no x", dict(x=None)), ("no W1", dict(W1=None)), ("no b1", dict(b1=None)), ("no graph_ptr", dict(graph_ptr=None)),
    ("no edge_ptr", dict(edge_ptr=None)), ("no status", dict(status=None)), ("no edge_index", dict(edge_index=None)),
    ("bits without emb", dict(poolbits="bits")), ("stacked without b2", dict(W2="W2", out2="out2")), ("stacked without out1", dict(W2="W2", b2="b2", out2="out2", out1=None)),
    ("stacked without out2", dict(W2="W2", b2="b2")), ("out2 without W2", dict(out2="out2")), ("no out1", dict(out1=None)),
    # order
    ("D, then slope", dict(D=128, slope=2.0)), ("slope, then N < 0", dict(slope=2.0, N=-1)), ("N < 0, then empty B", dict(N=-1, B=0)),
    ("empty B before no x", dict(B=0, x=None), True), ("no x, then bits without emb", dict(x=None, poolbits="bits")),
]
HEAD_CASES = [
    ("empty B", dict(B=0)), ("empty N", dict(N=0)),
    ("head without stack", dict(W2=None, b2=None)), ("head without bits", dict(poolbits=None, out2="out2")), ("head flags", dict(head_flags=2)),
    ("C = 0", dict(C=0)), ("C = 9", dict(C=9)),
    ("no y", dict(y=None)), ("no head_b0", dict(head_b0=None)), ("no head_W1", dict(head_W1=None)), ("no head_b1", dict(head_b1=None)),
    ("no z", dict(z=None)), ("no out", dict(out=None)), ("backward without demb", dict(demb=None)), ("no head workspace", dict(head_workspace=None)),
    ("head workspace short", dict(head_workspace_bytes=None)),
    # order
    ("head flags, then C", dict(head_flags=2, C=0)), ("C, then no y", dict(C=0, y=None)), ("no y, then head workspace short", dict(y=None, head_workspace_bytes=None)),
    ("stacked without out1, then head without bits", dict(out1=None, poolbits=None)),
]
PAIR_BLOCK = dict(x="x", W1="W", W2="W2", edge_index="ei", E=900, graph_ptr="gp", edge_ptr="ep", N=1000, B=100, F=32, D=64, graphs_per_tile=2,
                  slope=0.01, out1="out", out2="out2", status="st", mode=1, pair_dx="dx", pair_dout="dout", pair_ws_upper="ws",
                  pair_ws_upper_bytes=BIG, pair_ws_lower="ws2", pair_ws_lower_bytes=BIG, pair_act_upper=3, pair_act_lower=0,
                  pair_graphs_per_tile_upper=2)
PAIR_CASES = [
    ("the query's refusal", dict(F=65)), ("query", dict(pair_flags=1), True), ("no upper workspace", dict(pair_ws_upper=None)),
    ("no lower workspace", dict(pair_ws_lower=None)), ("upper workspace short", dict(pair_ws_upper_bytes="upper")),
    ("lower workspace short", dict(pair_ws_lower_bytes="lower")), ("empty N", dict(N=0, pair_ws_upper_bytes=0, pair_ws_lower_bytes=0), True),
    ("empty B", dict(B=0, pair_ws_upper_bytes=0, pair_ws_lower_bytes=0), True),
    # order
    ("the query's refusal, then no workspace", dict(F=65, pair_ws_upper=None)), ("query before no workspace", dict(pair_flags=1, pair_ws_upper=None), True),
    ("no workspace, then workspace short", dict(pair_ws_lower=None, pair_ws_upper_bytes="upper")),
]


def _block_call(block, change):
    lib = _lib.load()
    kw = dict(block)
    kw.update(change)
    a = _lib.FusedFwdArgs()
    for k, v in kw.items():
        if v is None and k == "head_workspace_bytes":
            v = lib.hcg_fused_aux_bytes(1, kw["B"], kw["graphs_per_tile"]) - 1
        elif v == "upper":
            v = lib.hcg_fused_workspace_bytes(kw["B"], 64, 64, kw["graphs_per_tile"]) - 256 - 1
        elif v == "lower":
            v = lib.hcg_fused_workspace_bytes(kw["B"], kw["F"], 64, kw["graphs_per_tile"]) - 256 - 1
        setattr(a, k, _resolve(v))
    return lib.hcg_fused_forward(ctypes.addressof(a), None)


def refusal_rows():
    """[launcher, case] -> the code returned.  Never where a GPU is visible: see `refusals`."""
    assert CUS is None, "made-up addresses: only where no GPU could be handed them"
    rows = [["hcg_fused_forward", "no block", _lib.load().hcg_fused_forward(None, None), False]]
    for name, order, base, cases, ws_short in LAUNCHERS:
        for case in cases:
            what, change, empty = case[0], dict(case[1]), len(case) > 2
            if "wsb" in change and change["wsb"] is None:
                change["wsb"] = ws_short(dict(base, **change))
            rows.append([name, what, _call(name, order, base, change), empty])
    for name, block, cases in (("hcg_fused_forward", FWD_BLOCK, FWD_CASES), ("hcg_fused_forward + head", HEAD_BLOCK, HEAD_CASES),
                               ("hcg_fused_forward, backward pair", PAIR_BLOCK, PAIR_CASES)):
        for case in cases:
            rows.append([name, case[0], _block_call(block, case[1]), len(case) > 2])
    return rows


SECTIONS = {"tiles": tiles_rows, "mid": mid_rows, "tall_supported": tall_supported_rows, "tall": tall_rows}     # (not the refusals)
INPUTS = {"tiles": 4, "mid": 5, "tall_supported": 4, "tall": 4}      # leading elements of a row that are its inputs


# ---- the golden file ------------------------------------------------------------------------------------------------------
# It holds every row's answers, written once each: "jobs" = the distinct reduction jobs (a row names one as "#k"), and per
# section "answers" = the distinct answer lists and "rows" = the index of each row's answers, rows in the order the functions
# above produce them (their inputs are not stored).  `_expand` gives back [inputs..., answers...] per row.
def _walk(v, fn):
    v = fn(v)
    return [_walk(x, fn) for x in v] if isinstance(v, list) else v


def _intern(table, v):
    key = json.dumps(v)
    return table.setdefault(key, len(table))


def _pack(sections, refusals):
    jobs, out = {}, {}
    for name, n in INPUTS.items():
        answers = {}
        rows = [_intern(answers, _walk(r[n:], lambda v: "#%d" % _intern(jobs, v["job"]) if isinstance(v, dict) else v))
                for r in sections[name]]
        out[name] = {"answers": [json.loads(k) for k in answers], "rows": rows}
    return dict(jobs=[json.loads(k) for k in jobs], refusals=refusals, **out)


def _expand(packed, inputs):
    job = lambda v: {"job": packed["jobs"][int(v[1:])]} if isinstance(v, str) and v.startswith("#") else v
    out = {"refusals": packed["refusals"], "cu_count": packed["cu_count"]}
    for name, n in INPUTS.items():
        sec = packed[name]
        assert len(sec["rows"]) == len(inputs[name]), name
        out[name] = [i[:n] + _walk(sec["answers"][k], job) for i, k in zip(inputs[name], sec["rows"])]
    return out


def _wrapped(items, width=150):
    """JSON list of `items`, several per line."""
    lines, line = [], ""
    for t in (json.dumps(i, separators=(",", ":")) for i in items):
        if line and len(line) + len(t) > width:
            lines.append(line)
            line = ""
        line += t + ","
    return "[\n  " + "\n  ".join(lines + [line]).rstrip(",") + "\n ]"


def _computed():
    """The rows of every section but the refusals from the loaded library, JSON-round-tripped (tuples -> lists)."""
    return {name: json.loads(json.dumps(fn())) for name, fn in SECTIONS.items()}


def _write_golden(computed):
    assert CUS is None, "generate the golden file on a machine without a GPU (CU fallback 256)"
    refusals = refusal_rows()
    for launcher, what, rc, empty in refusals:
        assert rc in ((OK,) if empty else (INVALID, WORKSPACE, UNSUPPORTED)), (launcher, what, rc)
    packed = _pack(computed, refusals)
    with open(GOLDEN, "w") as f:
        f.write('{"commit": %s,\n "cu_count": 256' % json.dumps(os.environ["HCG_WRITE_LAUNCH_GEOMETRY"]))
        f.write(',\n "jobs": %s,\n "refusals": %s' % (_wrapped(packed["jobs"]), _wrapped(packed["refusals"])))
        for name in INPUTS:
            f.write(',\n "%s": {"answers": %s,\n  "rows": %s}' % (name, _wrapped(packed[name]["answers"]), _wrapped(packed[name]["rows"])))
        f.write("\n}\n")


@pytest.fixture(scope="module")
def computed():
    return _computed()


@pytest.fixture(scope="module")
def refusals():
    """The refusal calls, made only where no GPU is visible: the skip comes BEFORE the first of them, so that a regression in
    a launcher's checks can never hand a made-up address to a kernel."""
    if CUS is not None:
        pytest.skip("made-up addresses: only where no GPU could be handed them")
    return json.loads(json.dumps(refusal_rows()))


@pytest.fixture(scope="module")
def golden(computed):
    if WRITE:
        _write_golden(computed)
    with open(GOLDEN) as f:
        return _expand(json.load(f), computed)


@pytest.mark.parametrize("section", list(SECTIONS))
def test_host_answers_equal_the_golden_file(computed, golden, section):
    got, want = computed[section], golden[section]
    assert len(got) == len(want)
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, "%d of %d rows differ; first: got %r, golden %r" % (len(wrong), len(want), wrong[0][0], wrong[0][1])


def test_rows_sit_on_the_boundaries(golden):
    """The golden file holds what this file asks: every shape edge, each family both taking and refusing shapes."""
    assert golden["cu_count"] == 256
    assert len(golden["mid"]) == len(MID_D) * len(MID_F) * len(MID_NODES) * len(MID_EDGES) * len(MID_B)
    assert {r[5] for r in golden["mid"]} == {0, 1} and {r[4] for r in golden["tall_supported"]} == {0, 1}
    assert len(golden["tall"]) == len(MID_D) * len(MID_F) * 5 * len(MID_B)
    refused = [r for r in golden["tiles"] if r[2] is None]          # F = 65 and 33 nodes: no tiles
    assert len(refused) == 6 + 5 - 1 and len(golden["tiles"]) - len(refused) == 7 * (6 * 5 - len(refused))
    # the tiles reach one workgroup, the 256-CU grid cap and the round behind it; both mid kernel families leave slabs
    assert {r[8][1]["job"][2] for r in golden["tiles"] if r[2]} >= {1, 2, 256}
    assert len({r[7][1]["job"][2] for r in golden["mid"] if r[7][0] == OK}) > 4


def test_refusals_return_the_golden_codes(refusals, golden):
    got, want = refusals, golden["refusals"]
    assert [r[:2] for r in got] == [r[:2] for r in want]
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, wrong
    for launcher, what, rc, empty in want:
        assert rc in ((OK,) if empty else (INVALID, WORKSPACE, UNSUPPORTED)), (launcher, what, rc)
