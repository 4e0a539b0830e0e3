"""The return codes of the four launchers of csrc/shapley.hip (no GPU): HCG_EXPLAIN_SHAPLEY with and without
HCG_EXPLAIN_GROUPED, HCG_EXPLAIN_COALITIONS, HCG_EXPLAIN_SUBSETS and HCG_EXPLAIN_GREEDY, for every way a block can be refused or
answered BEFORE a launch, alone and two at a time, so that the order of the launchers' checks is pinned.

No block of this file is complete and valid.  `_call` builds a block whose every pointer is the address of a live host
buffer (nothing dereferences it) and then applies the case's STOPPER last: the query flag, B = 0, no jobs, or one required
member NULL -- each of which returns before the kernel is launched -- and asserts that the stopper holds on the block it
hands to the library.  The expectations were recorded on the library as it was before the launchers shared their prelude."""
import ctypes
import os
import re

import pytest
import torch

import hcatgnet_amd as H
from hcatgnet_amd import _frozen, _lib

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -2, -3
F, D, C, N_CONV, R = 3, 64, 2, 2, 2
MODES = ("shapley", "grouped", "coalitions", "subsets", "greedy")
KERNEL = dict(shapley=_lib.HCG_EXPLAIN_SHAPLEY, grouped=_lib.HCG_EXPLAIN_SHAPLEY, coalitions=_lib.HCG_EXPLAIN_COALITIONS,
              subsets=_lib.HCG_EXPLAIN_SUBSETS, greedy=_lib.HCG_EXPLAIN_GREEDY)
_ = None                            # a stopper the mode does not have

COMMON = ["graph_ptr", "edge_ptr", "status", "x", "edge_index", "conv_W[0]", "conv_b[0]", "conv_W[1]", "conv_b[1]", "head_W[0]",
          "head_b[0]", "head_W[1]", "head_b[1]"]
LISTS = ["shap_group_ptr", "shap_member_ptr", "shap_members", "shap_bg_ptr", "shap_bg_members"]
# what a launch of the mode needs beside COMMON (B > 0, jobs > 0, a row of more than 0 entries)
REQUIRED = dict(shapley=["out", "out_base", "perm", "shap_acc", "workspace", "workspace_bytes"],
                grouped=["out", "out_base", "perm", "shap_acc", "workspace", "workspace_bytes"] + LISTS,
                coalitions=["coal_values", "coal_jobs", "coal_live_ptr"] + LISTS,
                subsets=["coal_values", "coal_jobs", "sub_bits", "sub_word_ptr", "sub_member_group"] + LISTS,
                greedy=["out", "out_base", "coal_values", "coal_jobs", "greedy_order", "greedy_cand", "sub_member_group"] + LISTS)
FORBIDDEN = ["edge_mask", "node_mask", "target", "dout"]


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


_HOST = (ctypes.c_char * 4096)()    # what every pointer of a block points at
ADDR = ctypes.addressof(_HOST)


def _set(a, name, value):
    m = re.fullmatch(r"(\w+)\[(\d+)\]", name)
    if m:
        getattr(a, m.group(1))[int(m.group(2))] = value
    else:
        setattr(a, name, value)


def _get(a, name):
    m = re.fullmatch(r"(\w+)\[(\d+)\]", name)
    return getattr(a, m.group(1))[int(m.group(2))] if m else getattr(a, name)


def _full(mode):
    """A block of `mode` with every member set that a launch would read: 2 graphs of 5 nodes and 8 edges"""
    x = torch.zeros(5, F)
    batch = H.Batch(x, torch.zeros(2, 8, dtype=torch.int64), torch.zeros(5, dtype=torch.int64), 2, max_nodes=3, max_edges=4,
                    edges_grouped=True)
    a = _lib.ExplainArgs()
    assert _frozen.query(a, KERNEL[mode], (F, D, C, N_CONV, R), batch) is None
    a.flags = _lib.HCG_EXPLAIN_GROUPED if mode == "grouped" else 0
    a.slope = 0.01
    for name in COMMON + REQUIRED[mode]:
        _set(a, name, ADDR)
    a.workspace_bytes = 1 << 30 if "workspace" in REQUIRED[mode] else 0
    a.shap_n_groups = 4
    if mode in ("shapley", "grouped"):
        a.n_perm, a.perm_first, a.perm_count, a.class_index = 2, 0, 2, 1
    else:
        a.coal_job_first, a.coal_job_count, a.coal_rows = 0, 3, 8
        a.coal_max_live, a.sub_max_groups = (2, 0) if mode == "coalitions" else (0, 2)
    if mode == "greedy":
        a.class_index, a.greedy_round, a.greedy_flags = 1, 1, 3
    return a


def _call(mode, stopper, extras):
    a = _full(mode)
    for name, value in extras.items():
        _set(a, name, value)
    # the stopper, last: nothing of `extras` can undo it
    if stopper == "query":
        a.flags |= _lib.HCG_EXPLAIN_QUERY
        assert a.flags & _lib.HCG_EXPLAIN_QUERY
    elif stopper == "B0":
        a.B = 0
        assert a.B == 0
    elif stopper == "nojobs":
        assert mode not in ("shapley", "grouped")
        a.coal_job_count = 0
        assert a.coal_job_count == 0
    else:
        assert stopper.startswith("null:")
        name = stopper[5:]
        assert name in COMMON + REQUIRED[mode]
        _set(a, name, None if name != "workspace_bytes" else 0)
        # (the member is read by this launch: a graph, jobs or permutations, and a row of more than 0 entries)
        assert not _get(a, name) and a.B > 0 and a.N > 0 and a.E > 0 and (a.coal_job_count > 0 or a.perm_count > 0)
        assert mode != "grouped" or a.shap_n_groups > 0
    rc = _lib.load().hcg_explain(ctypes.addressof(a), None)
    assert rc in (OK, INVALID, WORKSPACE, UNSUPPORTED), f"{mode} {stopper} {extras}: {rc} is no code of a refused block"
    return rc


# (stopper, what else is set) -> the codes of (shapley, grouped, coalitions, subsets, greedy)
P8 = ADDR
CASES = [
    # ---- the stoppers alone
    ("query", {}, (0, 0, 0, 0, 0)),
    ("B0", {}, (0, 0, 0, 0, 0)),
    ("nojobs", {}, (_, _, 0, 0, 0)),
    # ---- each forbidden pointer
    ("query", {"edge_mask": P8}, (-1, -1, -1, -1, -1)),
    ("query", {"node_mask": P8}, (-1, -1, -1, -1, -1)),
    ("query", {"target": P8}, (-1, -1, -1, -1, -1)),
    ("query", {"dout": P8}, (-1, -1, -1, -1, -1)),
    ("query", {"perm": P8}, (0, 0, -1, -1, -1)),
    ("B0", {"dout": P8}, (-1, -1, -1, -1, -1)),
    ("nojobs", {"perm": P8}, (_, _, -1, -1, -1)),
    # ---- the model axis
    ("query", {"n_models": 2}, (0, 0, -3, 0, -3)),
    ("query", {"n_models": 65536}, (-1, -1, -3, -1, -3)),
    ("B0", {"n_models": 2}, (0, 0, -3, 0, -3)),
    ("B0", {"n_models": 65536}, (-1, -1, -3, -1, -3)),
    # ---- the shape limits
    ("query", {"max_nodes": 185}, (-3, -3, -3, -3, -3)),
    ("B0", {"max_nodes": 185}, (-3, -3, -3, -3, -3)),
    ("query", {"max_nodes": 184, "max_edges": 1024}, (0, 0, 0, 0, 0)),
    ("query", {"coal_max_live": 17}, (0, 0, -3, 0, 0)),
    ("query", {"coal_max_live": 16}, (0, 0, 0, 0, 0)),
    ("query", {"sub_max_groups": 16385}, (0, 0, 0, -3, -3)),
    ("query", {"sub_max_groups": 16384}, (0, 0, 0, 0, 0)),
    ("query", {"coal_rows": 1 << 31}, (0, 0, -3, -3, 0)),
    # ---- what only a launch refuses
    ("query", {"coal_job_first": -1}, (0, 0, 0, 0, 0)),
    ("B0", {"coal_job_first": -1}, (0, 0, -1, -1, -1)),
    ("nojobs", {"coal_job_first": -1}, (_, _, -1, -1, -1)),
    ("B0", {"coal_job_count": -1}, (0, 0, -1, -1, -1)),
    ("B0", {"sub_max_groups": -1}, (0, 0, 0, -1, -1)),
    ("B0", {"coal_max_live": -1}, (0, 0, -1, 0, 0)),
    ("B0", {"shap_n_groups": -1}, (0, -1, -1, -1, -1)),
    ("query", {"shap_n_groups": -1}, (0, -1, 0, 0, 0)),
    ("B0", {"perm_count": 0}, (-1, -1, 0, 0, 0)),
    ("B0", {"perm_first": 1}, (-1, -1, 0, 0, 0)),
    # ---- the column, the round, the flags
    ("query", {"class_index": C}, (0, 0, 0, 0, -1)),
    ("B0", {"class_index": C}, (-1, -1, 0, 0, -1)),
    ("nojobs", {"class_index": C}, (_, _, 0, 0, -1)),
    ("query", {"greedy_flags": 4}, (0, 0, 0, 0, -1)),
    ("B0", {"greedy_flags": 4}, (0, 0, 0, 0, -1)),
    ("query", {"greedy_round": -1}, (0, 0, 0, 0, -1)),
    # ---- two at once: which check comes first
    ("query", {"dout": P8, "max_nodes": 185}, (-1, -1, -1, -1, -1)),
    ("query", {"dout": P8, "n_models": 2}, (-1, -1, -1, -1, -1)),
    ("query", {"n_models": 65536, "max_nodes": 185}, (-1, -1, -3, -1, -3)),
    ("query", {"class_index": C, "max_nodes": 185}, (-3, -3, -3, -3, -1)),
    ("query", {"greedy_flags": 4, "n_models": 2}, (0, 0, -3, 0, -1)),
    ("query", {"perm": P8, "greedy_flags": 4}, (0, 0, -1, -1, -1)),
    ("query", {"max_nodes": 185, "coal_max_live": 17, "sub_max_groups": 16385}, (-3, -3, -3, -3, -3)),
    ("B0", {"sub_max_groups": 16385, "coal_job_first": -1}, (0, 0, -1, -3, -3)),
    ("B0", {"coal_max_live": 17, "coal_job_first": -1}, (0, 0, -3, -1, -1)),
    ("B0", {"max_nodes": 185, "class_index": C}, (-3, -3, -3, -3, -1)),
    ("B0", {"x": None, "out": None, "coal_values": None, "shap_members": None}, (0, 0, 0, 0, 0)),
    ("nojobs", {"x": None, "coal_jobs": None, "shap_group_ptr": None}, (_, _, 0, 0, 0)),
    ("null:x", {"max_nodes": 185}, (-3, -3, -3, -3, -3)),
    ("null:x", {"coal_job_first": -1}, (-1, -1, -1, -1, -1)),
    ("null:x", {"workspace": None}, (-1, -1, -1, -1, -1)),
    ("null:status", {"workspace_bytes": 0}, (-1, -1, -1, -1, -1)),
    ("null:workspace", {"class_index": C}, (-1, -1, _, _, _)),
    ("null:shap_members", {"workspace_bytes": 0}, (_, -1, -1, -1, -1)),
]
# ---- with B > 0, jobs and a row: each required pointer NULL in turn while all others are set
for _name in COMMON:
    CASES.append((f"null:{_name}", {}, (-1, -1, -1, -1, -1)))
for _name in sorted({n for names in REQUIRED.values() for n in names}):
    CASES.append((f"null:{_name}", {}, tuple((-2 if _name.startswith("workspace") else -1) if _name in REQUIRED[m] else _ for m in MODES)))


def _id(case):
    stopper, extras, _codes = case
    return stopper + "".join(f" {k}={'set' if v == P8 else v}" for k, v in extras.items())


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_the_code_is_what_it_was(case):
    stopper, extras, codes = case
    got = tuple(_ if want is _ else _call(mode, stopper, extras) for mode, want in zip(MODES, codes))
    print(f"\n  {_id(case)}: {dict(zip(MODES, got))}")
    assert got == codes


def test_every_condition_of_the_list_is_covered():
    """each forbidden pointer, n_models of 2 and 65536, 185 nodes, 17 live groups, 16385 groups, a negative first job, the
    column C, flags of 4, the query, B = 0, no jobs, every required pointer, and pairs of them"""
    seen = [(s, set(e)) for s, e, _c in CASES]
    for name in FORBIDDEN + ["perm"]:
        assert any(name in e for _s, e in seen), name
    values = [(k, v) for _s, e, _c in CASES for k, v in e.items()]
    for kv in (("n_models", 2), ("n_models", 65536), ("max_nodes", 185), ("coal_max_live", 17), ("sub_max_groups", 16385),
               ("coal_job_first", -1), ("class_index", C), ("greedy_flags", 4)):
        assert kv in values, kv
    assert {"query", "B0", "nojobs"} <= {s for s, _e in seen}
    for mode in MODES:
        for name in COMMON + REQUIRED[mode]:
            assert any(s == f"null:{name}" and not e and c[MODES.index(mode)] is not _ for s, e, c in CASES), (mode, name)
    assert sum(len(e) + (s.startswith("null:") or s in ("B0", "nojobs")) >= 2 for s, e in seen) >= 2
    # the tiny block's own shape: a launch of it would read every required member
    for mode in MODES:
        a = _full(mode)
        assert a.B == 2 and a.N == 5 and a.E == 8 and int(a.N) * F + int(a.E) > 0 and a.shap_n_groups > 0
        assert all(_get(a, n) for n in COMMON + REQUIRED[mode])
