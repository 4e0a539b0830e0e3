"""Host side of the two-layer backward pair (no GPU): the tail fields of hcg_fused_fwd_args, mode HCG_FUSED_BWD_PAIR of
hcg_fused_forward and its query, which validates and answers without touching a GPU."""
import ctypes
import os

import pytest

from hcatgnet_amd import _lib

OK, INVALID, UNSUPPORTED = 0, -1, -3


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def _pair_block(F=64, D=64, B=4096, nodes=30, gpt=1, gpt_up=None, act_up=3, act_lo=0, dx=0x3000, form="bits", **over):
    """The pair's block as FusedTrainStep fills it; the addresses are stand-ins (16-byte aligned), never dereferenced by
    the query."""
    a = _lib.FusedFwdArgs()
    a.mode, a.pair_flags = _lib.HCG_FUSED_BWD_PAIR, _lib.HCG_FUSED_PAIR_QUERY
    a.x, a.W1, a.out1, a.W2 = 0x1000, 0x1100, 0x2000, 0x2100
    a.edge_index, a.graph_ptr, a.edge_ptr, a.status = 0x4000, 0x4100, 0x4200, 0x4300
    a.N, a.B, a.F, a.D, a.E = B * nodes, B, F, D, B * 64
    a.graphs_per_tile = gpt
    a.pair_graphs_per_tile_upper = gpt if gpt_up is None else gpt_up
    a.slope = 0.01
    a.pair_dx = dx
    a.pair_act_upper, a.pair_act_lower = act_up, act_lo
    if form == "bits":
        a.demb, a.poolbits = 0x5000, 0x5100
    elif form == "pooled":
        a.demb, a.emb, a.out2 = 0x5000, 0x5200, 0x5300
    else:
        a.pair_dout, a.out2 = 0x5400, 0x5300
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _rc(a):
    return _lib.load().hcg_fused_forward(ctypes.addressof(a), None)


def test_block_mirror_matches_the_library():
    lib = _lib.load()
    assert ctypes.sizeof(_lib.FusedFwdArgs) == lib.hcg_struct_bytes(_lib.HCG_STRUCT_FUSED_FWD_ARGS)
    assert lib.hcg_version() == 1
    # the pair's fields sit behind the forward's: the forward fields keep their offsets
    assert _lib.FusedFwdArgs.mode.offset > _lib.FusedFwdArgs.step_counter.offset
    assert _lib.FusedFwdArgs.x.offset == 0


def test_zeroed_block_is_still_the_forward():
    """mode 0 = the forward, with the forward's answers: an all-zero block has D = 0 (unsupported), an empty batch of a
    supported shape is nothing to do, and with graphs it asks for its pointers."""
    a = _lib.FusedFwdArgs()
    assert a.mode == _lib.HCG_FUSED_FORWARD == 0
    assert _rc(a) == UNSUPPORTED
    a.F, a.D, a.graphs_per_tile = 64, 64, 1
    assert _rc(a) == OK
    a.N, a.B = 30, 1
    assert _rc(a) == INVALID
    a.mode = 7
    assert _rc(a) == INVALID


def test_query_accepts_where_the_pair_applies():
    assert _rc(_pair_block()) == OK                                             # the flagship shape: 4096 graphs of 30, F = D = 64
    assert _rc(_pair_block(form="pooled")) == OK
    assert _rc(_pair_block(form="plain", act_up=2)) == OK                       # upper layer of a deeper stack, not pooled
    assert _rc(_pair_block(form="plain", act_up=3)) == OK
    assert _rc(_pair_block(F=25, B=20, nodes=10, gpt=3)) == OK
    assert _rc(_pair_block(F=32, B=2100, gpt=1)) == OK
    assert _rc(_pair_block(x=0x1004)) == OK                                     # an unaligned x is the lower layer's non-VEC path


def test_query_refuses_with_the_documented_codes():
    for kw in (dict(D=96), dict(D=128), dict(F=65), dict(F=0), dict(gpt=3, gpt_up=1), dict(gpt=0), dict(dx=0), dict(act_up=1),
               dict(act_up=0), dict(act_lo=1), dict(out1=0x2004), dict(dx=0x3004)):
        assert _rc(_pair_block(**kw)) == UNSUPPORTED, kw
    for kw in (dict(act_up=7), dict(pair_flags=3), dict(demb=0), dict(x=0), dict(W2=0), dict(status=0), dict(N=-1),
               dict(form="pooled", emb=0), dict(form="plain", out2=0), dict(pair_dout=0x5400)):
        assert _rc(_pair_block(**kw)) == INVALID, kw
    # without the query flag the launch form wants its workspaces before anything is enqueued
    assert _rc(_pair_block(pair_flags=0)) == INVALID


def test_python_query_answers_a_bool():
    assert _lib.HCG_ERR_UNSUPPORTED == UNSUPPORTED
    base = dict(x=0x1000, W1=0x1100, out1=0x2000, W2=0x2100, edge_index=0x4000, graph_ptr=0x4100, edge_ptr=0x4200,
                status=0x4300, N=90, B=3, F=64, D=64, E=10, graphs_per_tile=1, pair_graphs_per_tile_upper=1, slope=0.01,
                pair_dx=0x3000, pair_dout=0x5400, pair_act_upper=2)
    assert _lib.fused_bwd_pair(True, **base) is True
    assert _lib.fused_bwd_pair(True, **dict(base, D=96)) is False
    with pytest.raises(_lib.HcgError):
        _lib.fused_bwd_pair(True, **dict(base, W2=None))
