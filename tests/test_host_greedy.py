"""Host tests of `GreedySelection` (no GPU: CPU tensors take the loop path): the fp64 replay, exact ties, truncation and the
dead groups' placement, the result's shapes at the edges, the argument checks, the host job-list builder against a plain
Python loop, and the HCG_EXPLAIN_GREEDY mode and `greedy_` fields of the ABI.  tests/greedy_ref.py states the reference."""
import ctypes
import os

import pytest
import torch

import hcatgnet_amd as H
from hcatgnet_amd import _lib, greedy
from hcatgnet_amd.greedy import GreedyResult, GreedySelection, greedy_jobs
from hcatgnet_amd.subsets import AttributionCurves
from tests import coalition_ref as CR
from tests import greedy_ref as YR
from tests import shapley_ref as SR
from tests import subsets_ref as UR

PARAM_SEED = 23


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def _batch(c):
    return H.Batch(c.x, c.ei, c.batch, c.B, max_nodes=c.max_nodes, max_edges=c.max_edges, edges_grouped=True)


def _finish(c, **mk):
    c.params = SR.rand_params(c.x.shape[1], 64, seed=PARAM_SEED, **mk)
    c.model = SR.model_from_params(H, c.params)
    c.fw = UR.Forwards(c.params, c.x, c.ei, c.batch, c.B, c.ng, c.eg)
    c.kw = dict(node_group=c.ng, edge_group=c.eg)
    return c


@pytest.fixture(scope="module")
def mixed():
    c = CR.mixed_case()
    c.cls = 1
    return _finish(c, n_conv=2, n_read=2, n_classes=2)


@pytest.fixture(scope="module")
def atoms():
    """atoms as players on 31 and 33 nodes: the on-set ends inside a word and crosses a word boundary"""
    c = UR.sized_case((31, 33))
    c.x = CR.sparse_x(c.x, 0.3)
    c.ng, c.eg, c.cls = H.atom_groups(_batch(c)), None, 0
    return _finish(c, n_conv=2, n_read=2, n_classes=1)


# ------------------------------------------------------------------------------------------------ the loop against fp64
@pytest.mark.parametrize("name", ["atoms", "mixed"])
@pytest.mark.parametrize("mode", ["insertion", "deletion"])
def test_loop_passes_the_fp64_replay(name, mode, request):
    c = request.getfixturevalue(name)
    gs = GreedySelection(c.model)
    assert gs.reason(_batch(c)) == "the batch is on the CPU"
    r = gs(_batch(c), class_index=c.cls, mode=mode, **c.kw)
    assert gs.last_path == "loop" and isinstance(r, GreedyResult)
    YR.replay(r, c.fw, c.cls, mode, tag=name)
    assert YR.same(r, gs.loop(_batch(c), class_index=c.cls, mode=mode, **c.kw))
    if name == "mixed":
        # a full run is a valid order of `AttributionCurves`, and its values are that curve
        cur = AttributionCurves(c.model)(_batch(c), r.order, class_index=c.cls, **c.kw)
        cp, gp = cur.curve_ptr.tolist(), r.group_ptr.tolist()
        for g in range(c.B):
            curve = (cur.insertion if mode == "insertion" else cur.deletion)[cp[g] + 1:cp[g + 1]]
            assert torch.equal(curve, r.values[gp[g]:gp[g + 1]]), g
        r2 = gs(_batch(c), class_index=c.cls, mode=mode, direction=-1, **c.kw)
        YR.replay(r2, c.fw, c.cls, mode, direction=-1, tag=name)
        assert not torch.equal(r2.order, r.order)


def test_exact_ties_go_to_the_lower_group_id(mixed):
    c = mixed
    p = dict(c.params)
    last = [k for k in p if k.startswith("readout") and k.endswith("weight")][-1]
    p[last] = torch.zeros_like(p[last])
    model = SR.model_from_params(H, p)
    live, gp = c.fw.live, c.fw.gptr.tolist()
    want = [y for g in range(c.B) for y in [i for i in range(c.fw.count(g)) if live[g][i]] + [i for i in range(c.fw.count(g)) if not live[g][i]]]
    assert want == [0, 0, 1, 2, 0, 1, 2, 3, 4] and gp == [0, 0, 1, 4, 9]
    for mode in ("insertion", "deletion"):
        for direction in (1, -1):
            r = GreedySelection(model)(_batch(c), class_index=c.cls, mode=mode, direction=direction, **c.kw)
            assert r.order.flatten().tolist() == want, (mode, direction)
            assert bool((r.values == r.out_full[3]).all())              # every value is the bias


def test_steps_truncate_and_dead_groups_follow_a_full_run(mixed):
    c = mixed
    gs = GreedySelection(c.model)
    full = gs(_batch(c), class_index=c.cls, **c.kw)
    assert full.steps.tolist() == [0, 1, 3, 5] and full.order[0, 8] == 4          # graph 3's dead group 4 comes last
    assert torch.equal(full.values[8], full.values[7])
    for steps in (1, 2, 4, 7):
        r = gs(_batch(c), class_index=c.cls, steps=steps, **c.kw)
        YR.replay(r, c.fw, c.cls, "insertion", steps=steps, tag=f"mixed steps {steps}")
        gp = r.group_ptr.tolist()
        for g, L in enumerate([0, 1, 3, 4]):
            k = min(steps, L)
            assert torch.equal(r.order[0, gp[g]:gp[g] + k], full.order[0, gp[g]:gp[g] + k])
            assert torch.equal(r.values[gp[g]:gp[g] + k], full.values[gp[g]:gp[g] + k])
        # graph 3 has 4 live groups of 5: the dead one is appended by a run of 4 rounds or more only
        assert r.steps.tolist() == [0, min(steps, 1), min(steps, 3), 5 if steps >= 4 else steps]


def test_result_shapes_without_graphs_without_groups_and_without_live_groups(mixed):
    c = mixed
    gs = GreedySelection(c.model)
    e = H.Batch(c.x[:0], c.ei[:, :0], c.batch[:0], 0, max_nodes=0, max_edges=0, edges_grouped=True)
    for mode in ("insertion", "deletion"):
        r = gs(e, node_group=c.ng[:0], mode=mode)
        assert tuple(r.order.shape) == (1, 0) and r.order.dtype == torch.int32 and tuple(r.values.shape) == (0, 2)
        assert tuple(r.steps.shape) == (0,) and r.steps.dtype == torch.int64 and r.group_ptr.tolist() == [0]
        assert tuple(r.out_full.shape) == tuple(r.out_base.shape) == (0, 2)
        # a batch whose every feature is background: no group at all
        r = gs(_batch(c), node_group=torch.full_like(c.ng, -1), mode=mode)
        assert tuple(r.order.shape) == (1, 0) and tuple(r.values.shape) == (0, 2) and r.steps.tolist() == [0, 0, 0, 0]
        assert r.group_ptr.tolist() == [0] * 5 and torch.equal(r.out_full, r.out_base) and float(r.out_full.abs().min()) > 0
        # one graph whose only group is dead (L_g = 0): the start value is repeated
        nptr, eptr = SR.pointers(c.batch, c.ei, c.B)
        a, b, ea, eb = int(nptr[3]), int(nptr[4]), int(eptr[3]), int(eptr[4])
        one = H.Batch(c.x[a:b], (c.ei[:, ea:eb] - a).contiguous(), torch.zeros(b - a, dtype=torch.long), 1, max_nodes=b - a,
                      max_edges=eb - ea, edges_grouped=True)
        ng = torch.full((b - a,), -1, dtype=torch.int64)
        ng[1] = 0                                                            # the atom whose row of x is zero
        r = gs(one, node_group=ng, mode=mode)
        assert r.order.tolist() == [[0]] and r.steps.tolist() == [1] and torch.equal(r.out_full, r.out_base)
        assert torch.equal(r.values[0], (r.out_base if mode == "insertion" else r.out_full)[0])


def test_every_value_error(mixed):
    c = mixed
    b = _batch(c)
    gs, ss = GreedySelection(c.model), H.ShapleySampling(c.model)
    for call in (gs, gs.loop):
        for bad in ("insert", "both", None, 1):
            with pytest.raises(ValueError, match="mode must be"):
                call(b, mode=bad, **c.kw)
        for bad in (0, 2, -2, 0.5, True, None, "up"):
            with pytest.raises(ValueError, match="direction must be"):
                call(b, direction=bad, **c.kw)
        for bad in (0, -1):
            with pytest.raises(ValueError, match="steps must be at least 1"):
                call(b, steps=bad, **c.kw)
            with pytest.raises(ValueError, match="ids_per_job must be at least 1"):
                call(b, ids_per_job=bad, **c.kw)
        for bad in (-1, 2):
            with pytest.raises(ValueError, match="class_index"):
                call(b, class_index=bad, **c.kw)
        with pytest.raises(ValueError, match="give node_group, edge_group or both"):
            call(b)
    ok = CR.fragments(c.batch, c.B, 3)
    gap = ok.clone(); gap[ok == 1] = 5
    for gkw in (dict(node_group=gap), dict(node_group=ok.float()), dict(node_group=ok[:-1])):
        with pytest.raises(ValueError) as mine:
            gs(b, **gkw)
        with pytest.raises(ValueError) as theirs:
            ss(b, n_samples=1, **gkw)
        assert str(mine.value) == str(theirs.value)


# ------------------------------------------------------------------------------------------------ the job lists
@pytest.mark.parametrize("counts, lives, steps, ipj", [
    ([5, 0, 3, 9], [4, 0, 3, 9], None, 1),
    ([5, 0, 3, 9], [4, 0, 3, 9], None, 4),
    ([5, 0, 3, 9], [4, 0, 3, 9], 3, 2),
    ([40, 33, 1], [40, 30, 0], 10, 16),
    ([184], [184], None, 7),
    ([2, 2], [0, 0], None, 3),
    ([], [], None, 5),
])
def test_job_lists_against_a_plain_loop(counts, lives, steps, ipj):
    rounds = [c if steps is None else min(steps, c) for c in lives]
    jobs, ptr = greedy_jobs(counts, rounds, ipj)
    ref = YR.jobs_ref(counts, rounds, ipj)
    assert jobs.dtype == torch.int32 and jobs.dim() == 2 and jobs.shape[1] == 3 and jobs.is_contiguous()
    launches = len(ptr) - 1
    print(f"\n  counts {counts} rounds {rounds} ids_per_job {ipj}: {launches} launches, {jobs.shape[0]} jobs")
    assert launches == len(ref) == ((max(rounds) + 1) if counts else 0) and ptr[0] == 0 and ptr[-1] == jobs.shape[0]
    assert default_is_sane()
    for k in range(launches):
        mine = [tuple(t) for t in jobs[ptr[k]:ptr[k + 1]].tolist()]
        assert sorted(mine) == sorted(ref[k]), k
        for g, (G, R) in enumerate(zip(counts, rounds)):
            own = sorted((y, n) for q, y, n in mine if q == g)
            if R > k:
                # exactly one owner, and the ranges tile 0 .. G - 1
                assert [y for y, _ in own].count(0) == 1 and all(1 <= n <= ipj for _, n in own)
                assert [y for y, n in own for y in range(y, y + n)] == list(range(G))
            elif R == k:
                assert own == [(0, 0)]                                   # the job that only picks
            else:
                assert own == []


def default_is_sane():
    d = GreedySelection.default_ids_per_job
    return d(0) == 1 and d(184) == 1 and d(4 * 256 * 3) == 3 and d(535 * 100) == 16 and d(10 ** 9) == 16


# ------------------------------------------------------------------------------------------------ ABI
def _query(nodes=184, edges=390, max_groups=0, flags=None, **ptrs):
    a = _lib.ExplainArgs()
    a.mode = _lib.HCG_EXPLAIN_GREEDY
    a.flags = _lib.HCG_EXPLAIN_QUERY if flags is None else flags
    a.F, a.D, a.C, a.n_conv, a.R = 25, 64, 1, 2, 2
    a.max_nodes, a.max_edges, a.N, a.E, a.B = nodes, edges, nodes, edges, 1
    a.sub_max_groups = max_groups
    for k, v in ptrs.items():
        setattr(a, k, v)
    rc = _lib.load().hcg_explain(ctypes.addressof(a), None)
    return rc, int(a.workspace_bytes_needed), int(a.lds_bytes)


def test_struct_size_mode_and_overlay_offsets():
    assert ctypes.sizeof(_lib.ExplainArgs) == 608 == _lib.load().hcg_struct_bytes(_lib.HCG_STRUCT_EXPLAIN_ARGS)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hcatgnet_hip.h")).read()
    assert _lib.HCG_EXPLAIN_GREEDY == 9 and "#define HCG_EXPLAIN_GREEDY 9" in header
    assert "#define HCG_GREEDY_DELETION 1" in header and "#define HCG_GREEDY_NEGATE 2" in header
    assert (_lib.HCG_GREEDY_DELETION, _lib.HCG_GREEDY_NEGATE) == (1, 2)
    base = _lib.ExplainArgs.fit_edge_logit.offset
    # every earlier member where it was
    assert _lib.ExplainArgs.coal_values.offset == base + 48 and _lib.ExplainArgs.sub_bits.offset == base + 96
    assert _lib.ExplainArgs.sub_reserved.offset == base + 124
    at = base + 128
    for name, ctype in _lib.GREEDY_FIELDS:
        f = getattr(_lib.ExplainArgs, name)
        assert f.offset == at and f.size == ctypes.sizeof(ctype) and name in header, name
        at += f.size
    print(f"\n  the greedy_ fields end at byte {at} of 608")
    assert at == 608
    assert [n for n, _ in _lib.GREEDY_FIELDS] == ["greedy_round", "greedy_flags"]
    # the two pointers share the slot of a field the mode does not read
    assert dict(_lib.GREEDY_SLOTS) == dict(greedy_order="coal_live_ptr", greedy_cand="sub_bits")
    for name, slot in _lib.GREEDY_SLOTS:
        f = getattr(_lib.ExplainArgs, name)
        assert f.offset == getattr(_lib.ExplainArgs, slot).offset and f.size == 8 and name in header


def test_the_offsets_match_the_header_compiled_as_c(tmp_path):
    import shutil
    import subprocess
    cc = next((p for p in (shutil.which(n) for n in ("cc", "gcc", "clang", "c++", "g++", "hipcc")) if p), None)
    if cc is None:
        cc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    names = ["coal_live_ptr", "sub_bits", "sub_reserved"] + [n for n, _ in _lib.GREEDY_FIELDS] + [n for n, _ in _lib.GREEDY_SLOTS]
    src = tmp_path / "offsets.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hcatgnet_hip.h"\nint main(void) { printf("' + " ".join(["%zu"] * (len(names) + 1))
                   + '", ' + ", ".join(f"offsetof(hcg_explain_args, {n})" for n in names) + ", sizeof(hcg_explain_args)); return 0; }\n")
    exe = tmp_path / "offsets"
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.run([cc, "-I", inc, str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    print(f"\n  {dict(zip(names + ['sizeof'], got))}")
    assert got == [getattr(_lib.ExplainArgs, n).offset for n in names] + [608]


def test_query_takes_the_shapley_limits_and_reports_lds():
    from hcatgnet_amd import _frozen
    assert _lib.HCG_EXPLAIN_GREEDY in _frozen._MODES and _frozen._MODES[_lib.HCG_EXPLAIN_GREEDY][1] == 184
    a = _lib.ExplainArgs()
    a.mode, a.flags = _lib.HCG_EXPLAIN_SUBSETS, _lib.HCG_EXPLAIN_QUERY
    a.F, a.D, a.C, a.n_conv, a.R, a.max_nodes, a.max_edges, a.N, a.E, a.B = 25, 64, 1, 2, 2, 184, 390, 184, 390, 1
    assert _lib.load().hcg_explain(ctypes.addressof(a), None) == 0
    rc, ws, lds = _query()
    print(f"\n  greedy query at 184 nodes: rc {rc} workspace {ws} lds {lds} (the subset kernel's {int(a.lds_bytes)})")
    assert rc == 0 and ws == 0 and lds == int(a.lds_bytes) > 0
    assert _query(nodes=184, edges=1024)[2] <= 160 * 1024
    assert _query(nodes=185)[0] == -3 and _query(edges=1025)[0] == -3
    assert greedy.MAX_SUBSET_GROUPS == 16384 and _query(max_groups=16384)[0] == 0 and _query(max_groups=16385)[0] == -3
    for name in ("edge_mask", "node_mask", "target", "dout", "perm"):
        assert _query(**{name: 8})[0] == -1, name
    Q = _lib.HCG_EXPLAIN_QUERY
    assert _query(flags=Q | _lib.HCG_EXPLAIN_GROUPED)[0] == -1 and _query(flags=Q | _lib.HCG_EXPLAIN_TARGET_CLASS)[0] == -1
    gs = GreedySelection(H.make_network("GCN", H.default_options(), 25))
    assert gs.reason() is None and gs.launches is None and gs.last_path is None


def test_a_launch_with_bad_scalars_or_null_arrays_is_refused_before_the_gpu_is_touched():
    assert _query(flags=0, max_groups=-1)[0] == -1 and _query(flags=0, greedy_round=-1)[0] == -1
    assert _query(flags=0, greedy_flags=4)[0] == -1 and _query(flags=0, class_index=1)[0] == -1 and _query(flags=0, class_index=-1)[0] == -1
    assert _query(flags=0, coal_job_count=-1)[0] == -1 and _query(flags=0, coal_job_first=-1)[0] == -1
    assert _query(flags=0, coal_job_count=0, greedy_flags=3)[0] == 0          # nothing to run
    assert _query(flags=0, coal_job_count=1)[0] == -1                         # every array NULL


def test_exports_and_docstrings():
    for name in ("GreedySelection", "GreedyResult"):
        assert getattr(H, name) is not None and name in H.__all__
    assert "GreedySelection" in H.__doc__
    for word in ("insertion", "deletion", "lower group", "NaN", "min(`steps`, L_g)", "dead groups", "launches"):
        assert word in GreedySelection.__doc__, word
    assert issubclass(GreedySelection, H.subsets._frozen.FrozenModel)
