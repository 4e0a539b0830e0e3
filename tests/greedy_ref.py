"""The fp64 reference of `GreedySelection` and the helpers both greedy test files share (tests only).

The reference is a REPLAY, so that near-ties need no screening and no case is left out: for each graph the result's own order
is walked.  At round k, with the on-set the result implies, every candidate's value (the live groups not yet picked, one
flipped each) comes from the fp64 oracle (`subsets_ref.Forwards`).  With scale = max(1, max |v_ref|) over everything
evaluated for the graph and TOL = 1e-5 (tests/shapley_ref.py, the bound of every kernel of this family):
    1. |values[k] - v64(pick_k)| <= TOL scale, elementwise over C
    2. key64(pick_k) >= max_y key64(y) - 2 TOL scale: every float32 key is within TOL scale of its fp64 key and the pick has
       the greatest float32 key, so its fp64 key can trail the best fp64 key by twice that at most
    3. the picks are distinct, live and inside the graph; the dead groups follow, ascending, with the last value repeated
       bitwise; `steps` is right; positions beyond are -1 / 0
    4. out_full / out_base are within TOL scale of the all-on / all-off forwards
Every figure is printed before it is asserted (`pytest -s`)."""
import torch

from tests.shapley_ref import TOL


def rounds_ref(fw, steps):
    """per graph: min(steps, L_g)"""
    return [int(fw.live[g].sum()) if steps is None else min(int(steps), int(fw.live[g].sum())) for g in range(fw.B)]


def jobs_ref(counts, rounds, ipj):
    """The job lists as a plain Python loop: list over the launches of lists of (graph, first id, ids)"""
    launches = []
    for k in range((max(rounds) + 1) if counts else 0):
        jobs = []
        for g, (G, R) in enumerate(zip(counts, rounds)):
            if R > k:
                jobs += [(g, y, min(ipj, G - y)) for y in range(0, G, ipj)]
            elif R == k:
                jobs.append((g, 0, 0))
        launches.append(jobs)
    return launches


def replay(r, fw, cls, mode, direction=1, steps=None, tag=""):
    """`GreedyResult` against the fp64 oracle, graph by graph (see the module docstring)"""
    B = fw.B
    assert r.order.dtype == torch.int32 and r.values.dtype == torch.float32 and r.steps.dtype == torch.int64
    assert r.group_ptr.dtype == torch.int64 and torch.equal(r.group_ptr.cpu(), fw.gptr)
    Gt = int(fw.gptr[-1])
    C = int(r.values.shape[1])
    assert tuple(r.order.shape) == (1, Gt) and tuple(r.values.shape) == (Gt, C) and tuple(r.steps.shape) == (B,)
    assert tuple(r.out_full.shape) == tuple(r.out_base.shape) == (B, C)
    order = r.order.flatten().cpu().tolist()
    values32 = r.values.detach().cpu()
    values, full, base = values32.double(), r.out_full.detach().double().cpu(), r.out_base.detach().double().cpu()
    nsteps = r.steps.cpu().tolist()
    sgn = float(direction) if mode == "insertion" else -float(direction)
    rounds = rounds_ref(fw, steps)
    worst, fails, evaluated = dict(values=0.0, gap=0.0, ends=0.0), [], 0
    for g in range(B):
        a, G = int(fw.gptr[g]), fw.count(g)
        live = [y for y in range(G) if bool(fw.live[g][y])]
        dead = [y for y in range(G) if not bool(fw.live[g][y])]
        R = rounds[g]
        on = set() if mode == "insertion" else set(range(G))
        picks = order[a:a + R]
        # 3. the picks: inside the graph, live, distinct
        assert all(0 <= y < G for y in picks) and set(picks) <= set(live) and len(set(picks)) == R, (tag, g, picks)
        ref_full, ref_base = fw(g, range(G)), fw(g, [])
        seen = [ref_full, ref_base]
        rows = []
        for k, y in enumerate(picks):
            cands = [c for c in live if c not in picks[:k]]
            v64 = {c: fw(g, on ^ {c}) for c in cands}
            seen += list(v64.values())
            evaluated += len(cands)
            rows.append((k, y, v64[y], max(sgn * float(v[cls]) for v in v64.values()), sgn * float(v64[y][cls])))
            on = on ^ {y}
        scale = max(1.0, max(float(v.abs().max()) for v in seen))
        bound = TOL * scale
        for k, y, v, best, mine in rows:
            e_v = float((values[a + k] - v).abs().max())            # 1.
            gap = best - mine                                       # 2.
            worst["values"] = max(worst["values"], e_v / bound)
            worst["gap"] = max(worst["gap"], gap / (2 * bound))
            if e_v > bound or gap > 2 * bound:
                fails.append((g, k, y, e_v, bound, gap, 2 * bound))
        e_e = max(float((full[g] - ref_full).abs().max()), float((base[g] - ref_base).abs().max()))    # 4.
        worst["ends"] = max(worst["ends"], e_e / bound)
        if e_e > bound:
            fails.append((g, "ends", e_e, bound))
        # 3. the tail: the dead groups behind a full run (the last value repeated bitwise), nothing behind a truncated one
        filled = R + (len(dead) if R == len(live) else 0)
        assert nsteps[g] == filled, (tag, g, nsteps[g], filled)
        if R == len(live):
            assert order[a + R:a + G] == dead, (tag, g, order[a + R:a + G], dead)
            last = values32[a + R - 1] if R > 0 else (r.out_base if mode == "insertion" else r.out_full)[g].detach().cpu()
            for j in range(R, G):
                assert torch.equal(values32[a + j], last), (tag, g, j)
        assert order[a + filled:a + G] == [-1] * (G - filled) and float(values32[a + filled:a + G].abs().sum()) == 0.0, (tag, g)
    print(f"    {tag} {mode} direction {direction:+d} steps {steps}: {evaluated} fp64 candidates over {B} graphs; worst figure / bound: "
          + "  ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert not fails, fails


def same(a, b):
    """every field of two `GreedyResult`s bitwise equal"""
    return all(torch.equal(p, q) for p, q in zip(a, b))
