"""Host side of the backward pair's switch (no GPU): where the pair is refused.

* The support query is one host function (csrc/pair_query.h) that fused.hip calls; compiled here alone, with and without
  -DHCG_NO_BWD_PAIR: the A/B build still refuses everything, the product build answers as the library does.
* `FusedTrainStep._pair_applies` still refuses size-grouped batches, `PREMASK = False` and a first layer off the tile family
  before it asks the library."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

from hcatgnet_amd import _lib
from hcatgnet_amd import functional as HF
from hcatgnet_amd.train import FusedTrainStep, Part, _Ctx, step_parts
from tests.test_host_bwd_pair import _pair_block

OK, INVALID, UNSUPPORTED = 0, -1, -3
CSRC = os.path.dirname(_lib.LIB_PATH)
SHIM = ('#include "%s"\nextern "C" int pair_applies(const hcg_fused_fwd_args* a) { return hcg_bwd_pair_applies(a, 64); }\n'
        % os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", "pair_query.h"))


@pytest.fixture(scope="module")
def queries(tmp_path_factory):
    """-> (product build's query, -DHCG_NO_BWD_PAIR build's query): pair_query.h compiled alone by the host compiler."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    d = tmp_path_factory.mktemp("pair_query")
    (d / "shim.cpp").write_text(SHIM)
    fns = []
    for name, defs in (("on", []), ("off", ["-DHCG_NO_BWD_PAIR"])):
        so = str(d / f"libq_{name}.so")
        subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", *defs, str(d / "shim.cpp"), "-o", so], check=True)
        fn = ctypes.CDLL(so).pair_applies
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p]
        fns.append(lambda a, fn=fn: fn(ctypes.addressof(a)))
    return fns


BLOCKS = [dict(), dict(form="pooled"), dict(form="plain", act_up=2), dict(F=25, B=20, nodes=10, gpt=3), dict(x=0x1004),
          dict(D=96), dict(F=65), dict(gpt=3, gpt_up=1), dict(dx=0), dict(act_up=1), dict(act_lo=1), dict(out1=0x2004),
          dict(act_up=7), dict(pair_flags=3), dict(demb=0), dict(W2=0), dict(N=-1)]


def test_query_refuses_everything_in_a_build_without_the_pair(queries):
    on, off = queries
    assert on(_pair_block()) == OK                       # the flagship shape, as FusedTrainStep asks
    malformed = [dict(act_up=7), dict(pair_flags=3), dict(N=-1)]      # told so before the build's answer, as before
    for kw in BLOCKS:
        assert off(_pair_block(**kw)) == (INVALID if kw in malformed else UNSUPPORTED), kw


def test_the_library_answers_with_the_same_function(queries):
    on, _ = queries
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    for kw in BLOCKS:
        a = _pair_block(**kw)
        assert lib.hcg_fused_forward(ctypes.addressof(a), None) == on(a), kw


def _ctx(F=64, D=64, B=3, nodes=30, routes=None, n_small=None, n_conv=2, step=None):
    """What `_pair_applies` reads of a prepared step, on CPU tensors: the query dereferences none of them.  `routes`: what
    `conv_route` is made to answer for the layers (default: what it does answer, the tiles at one graph per tile)."""
    c = _Ctx()
    N = B * nodes
    c.F, c.D, c.n_conv = F, D, n_conv
    c.x = torch.zeros(N, F)
    c.W = [torch.zeros(D, F), torch.zeros(D, D)]
    c.bufs = {"acts": [torch.zeros(N, D)], "dacts": [torch.zeros(N, D)]}
    keep = [torch.zeros(2, 8, dtype=torch.int64), torch.zeros(B + 1, dtype=torch.int32), torch.zeros(B + 1, dtype=torch.int32),
            torch.zeros(4, dtype=torch.int32)]
    c.batch = keep                                        # (kept alive beside the addresses below)
    geo = HF.Geometry(keep[0].data_ptr(), 8, keep[1].data_ptr(), keep[2].data_ptr(), N, B, nodes, 64, keep[3].data_ptr(), 0)
    if n_small is not None:           # a size-grouped batch: its larger graphs have 40 nodes (the real routes answer)
        parts = step_parts([(F, D, "auto"), (D, D, "auto")][:n_conv], N, B, 40, 90, n_small, sw=step)
        assert len(parts) == 2
    else:
        answers = iter(routes if routes is not None else [(HF.TILES, 1), (HF.TILES, 1)])
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(HF, "conv_route", lambda *a, **kw: next(answers))
            parts = step_parts([(F, D, "auto"), (D, D, "auto")][:n_conv], N, B, nodes, 64, sw=step)
    c.parts = [Part(geo._replace(g0=g0, B=nB), forms, None) for g0, nB, forms in parts]
    return c


def _step(**switches):
    step = object.__new__(FusedTrainStep)                 # only the switches and the answer cache: no model, no GPU
    step._pair_ok = {}
    step.BWD_PAIR = True
    for k, v in switches.items():
        setattr(step, k, v)
    return step


def test_pair_applies_only_where_the_step_can_use_it(monkeypatch):
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    asked = []
    real = HF.TILES.backward_pair
    monkeypatch.setattr(HF.TILES, "backward_pair", lambda *a, **kw: (asked.append(kw.get("query")), real(*a, **kw))[1])
    applies = lambda step, **kw: step._pair_applies(_ctx(step=step, **kw))     # (the context's plan: made for that step)
    assert applies(_step()) is True and asked == [True]                       # the control: the flagship form is accepted
    del asked[:]
    assert applies(_step(), n_small=2) is False                               # size-grouped batch
    assert applies(_step(PREMASK=False)) is False                             # dx would not go down premasked
    assert applies(_step(), routes=[(HF.MID, 0), (HF.TILES, 1)]) is False     # first layer off the tile family
    assert applies(_step(), routes=[(HF.TALL, 0), (HF.TILES, 1)]) is False
    assert applies(_step(), n_conv=1) is False
    assert applies(_step(BWD_PAIR=False)) is False
    assert asked == []                                                        # ... all of them before the library is asked
    assert applies(_step(), routes=[(HF.TILES, 3), (HF.TILES, 1)]) is False and asked == [True]   # the library's refusal
