"""CPU-side tests of the device-side fit (hcatgnet_amd/fit.py, csrc/fit.hip): `FitControl` -- the kernel's state machine in
plain Python and its oracle on the GPU -- against torch's own ReduceLROnPlateau and the loop of
examples/train_like_reference.py, the argument struct's size as a C compiler sees the header, argument validation.  No
GPU."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import pytest

import hcatgnet_amd as H
from hcatgnet_amd import _lib
from tests import fit_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def _same(a, b):
    return a == b or (a != a and b != b)


def test_crafted_sequences_do_on_torch_what_they_are_crafted_for():
    """Each crafted property on torch's scheduler alone, so that the comparison below cannot pass vacuously."""
    seqs = fit_ref.crafted()
    cfg, rows = seqs["plateau"]
    st, _ = fit_ref.torch_loop(cfg, rows)
    lrs = [cfg["lr"]] + [s["lr"] for s in st]
    assert sum(a != b for a, b in zip(lrs, lrs[1:])) >= 3                       # reduced at least three times
    assert lrs[-1] == cfg["min_lr"] and cfg["lr"] * cfg["factor"] ** 4 < cfg["min_lr"]     # ... and clamped, not merely small
    cfg, rows = seqs["eps"]
    st, _ = fit_ref.torch_loop(cfg, rows)
    assert all(s["lr"] == cfg["lr"] for s in st) and cfg["patience"] == 0       # a reduction was due on every bad epoch
    assert cfg["lr"] - cfg["lr"] * cfg["factor"] <= cfg["eps"]
    bad = {k: fit_ref.torch_loop(*seqs[k])[0][1]["num_bad_epochs"] for k in ("edge_at", "edge_below", "edge_above")}
    assert bad == {"edge_at": 1, "edge_below": 0, "edge_above": 1}              # `<` at the threshold, not `<=`
    st, _ = fit_ref.torch_loop(*seqs["equal"])
    assert st[-1]["stopped"] and st[-1]["best_epoch"] == 0 and len(st) < len(seqs["equal"][1])
    st, _ = fit_ref.torch_loop(*seqs["nan"])
    assert st[2]["stall"] == 2 and st[2]["lr"] < st[0]["lr"] and st[3]["val_best"] == 0.9       # NaN is never better
    st, _ = fit_ref.torch_loop(*seqs["nan_first"])
    assert st[1]["val_best"] == fit_ref.INF and st[1]["stall"] == 2 and st[2]["best_epoch"] == 2
    st, _ = fit_ref.torch_loop(*seqs["inf"])
    assert st[1]["val_best"] == fit_ref.INF and st[1]["sched_best"] == fit_ref.INF and st[1]["stall"] == 2
    st, _ = fit_ref.torch_loop(*seqs["patience0"])
    assert st[1]["lr"] == 0.005 and st[2]["lr"] == 0.005 and st[3]["lr"] == 0.0025
    st, _ = fit_ref.torch_loop(*seqs["cooldown"])
    assert [s["cooldown_counter"] for s in st[:5]] == [0, 2, 1, 0, 2]
    st, _ = fit_ref.torch_loop(*seqs["stop"])
    assert len(st) == 7 and st[-1]["stopped"] and st[-1]["lr"] < 0.01


@pytest.mark.parametrize("name", sorted(fit_ref.all_sequences()))
def test_fit_control_agrees_with_torch_at_every_step(name):
    """lr, best, num_bad_epochs, cooldown, last_epoch, stall, best_epoch, the snapshot decision after every epoch, and the
    epoch the fit stops at: `FitControl` against torch's scheduler + the example's bookkeeping."""
    from hcatgnet_amd.fit import FitControl
    cfg, rows = fit_ref.all_sequences()[name]
    want, sched = fit_ref.torch_loop(cfg, rows)
    fc = fit_ref.make_control(FitControl, cfg, len(rows))
    got = []
    for row in rows:
        snap = fc.step(*row)
        if snap is None:
            assert fc.stopped and fc.step(*row) is None                          # stays stopped
            continue
        got.append(dict(fc.state(), snapshot=snap))
    assert len(got) == len(want) == fc.epochs_counted == len(fc.log)            # the stop epoch
    for e, (g, w) in enumerate(zip(got, want)):
        for k, v in w.items():
            assert _same(g[k], v), (name, e, k, g[k], v)
        assert g["epoch"] == e + 1 and fc.log[e][3] == w["lr"] and _same(fc.log[e][1], rows[e][1])
    assert fc.sched_best == sched.best and fc.last_epoch == sched.last_epoch


def test_fit_control_ignores_epochs_past_max_epochs():
    from hcatgnet_amd.fit import FitControl
    fc = FitControl(0.01, control_every=1, early_stopping=100, max_epochs=2)
    assert fc.step(1.0, 1.0, 1.0) is True and fc.step(1.0, 2.0, 1.0) is False and fc.step(1.0, 0.1, 1.0) is None
    assert fc.epochs_counted == 2 and fc.val_best == 1.0 and not fc.stopped


def test_fit_control_structs_match_the_header():
    """sizeof(hcg_fit_control_args), sizeof(hcg_fit_state) and sizeof(hcg_update_args) (whose `fit_control` carries the
    launch) as a C compiler sees the header = the ctypes mirrors = what the library was built with; a launch with missing
    pointers or a bad constant is refused on the host."""
    cc = next((p for p in (shutil.which(n) for n in ("cc", "gcc", "clang", "c++", "g++", "hipcc")) if p), None)
    if cc is None:
        cc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write('#include <stdio.h>\n#include "hcatgnet_hip.h"\nint main(void) { printf("%zu %zu %zu", '
                             'sizeof(hcg_fit_control_args), sizeof(hcg_fit_state), sizeof(hcg_update_args)); return 0; }\n')
        subprocess.run([cc, "-I", os.path.join(REPO, "include"), src, "-o", exe], check=True, capture_output=True)
        sizes = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    lib = _lib.load()
    mirrors = [(_lib.FitControlArgs, _lib.HCG_STRUCT_FIT_CONTROL_ARGS), (_lib.FitState, _lib.HCG_STRUCT_FIT_STATE),
               (_lib.UpdateArgs, _lib.HCG_STRUCT_UPDATE_ARGS)]
    for size, (mirror, which) in zip(sizes, mirrors):
        assert ctypes.sizeof(mirror) == size == lib.hcg_struct_bytes(which), mirror
    a, u = _lib.FitControlArgs(), _lib.UpdateArgs()
    u.fit_control = ctypes.addressof(a)
    assert lib.hcg_update_dev(ctypes.addressof(u), None) == -1                   # nothing set
    for i in range(3):
        a.sums[i], a.denom[i] = 0x1000 + 8 * i, 1.0
    a.state, a.lr_dev, a.param, a.best, a.log, a.n = 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 4
    a.max_epochs, a.control_every, a.factor, a.rel_epsilon = 1, 0, 0.5, 1.0
    assert lib.hcg_update_dev(ctypes.addressof(u), None) == -1                   # control_every < 1
    a.control_every, a.denom[1] = 1, 0.0
    assert lib.hcg_update_dev(ctypes.addressof(u), None) == -1                   # a denominator that is not positive
    a.denom[1], a.best = 1.0, a.param
    assert lib.hcg_update_dev(ctypes.addressof(u), None) == -1                   # the best slot is the parameters


SCHEDULES = ((1, 5), (3, 5), (6, 1), (7, 3), (8, 3), (40, 2), (250, 5), (251, 5))


@pytest.mark.parametrize("epochs,every", SCHEDULES)
def test_chunk_end_tiles_the_epochs_on_control_epochs(epochs, every):
    """`chunk_end` walked from 0: the chunks tile 0..epochs, every chunk but possibly the last ends on a control epoch, and
    the launches both forms derive from it are `chunk_launches` (one graph for a full interval, else one per epoch) and
    three per epoch."""
    from hcatgnet_amd.fit import chunk_end, chunk_launches
    at, chunks = 0, []
    while at < epochs:
        end = chunk_end(at, epochs, every)
        assert at < end <= epochs
        chunks.append((at, end))
        at = end
    assert at == epochs and chunks[0] == (0, 1) and chunk_end(epochs, epochs, every) == epochs
    assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
    assert all((end - 1) % every == 0 for _, end in chunks[:-1])
    assert all(end - first == every for first, end in chunks[1:-1])              # (between epoch 0 and the tail: full intervals)
    assert sum(1 if end - first == every else end - first for first, end in chunks) == chunk_launches(epochs, every)
    assert sum(3 * (end - first) for first, end in chunks) == 3 * epochs


def test_the_first_state_is_fit_controls_on_a_stepped_scheduler():
    """`_first_state` -- the one place the controller's `FitState` is initialised, for both device forms -- field by field
    against `FitControl.for_model(...).state()`, on a scheduler that is reducing, cooling down and counting bad epochs."""
    import torch
    from hcatgnet_amd.fit import FitControl, _first_state
    m = H.make_network("GCN", H.default_options(), 25)
    lr0 = m.optimizer.param_groups[0]["lr"]
    m.scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(m.optimizer, mode="min", factor=0.5, patience=1, cooldown=2)
    seen = []
    for val in (None, 1.0, 0.5, 0.7, 0.8, 0.9, 0.95, 0.96):
        if val is not None:
            m.scheduler.step(val)
        init, want = _first_state(m), FitControl.for_model(m, 5, 6, 250).state()
        for k in FitControl.STATE:
            assert getattr(init, k) == want[k], (val, k)
        assert init.lr == m.optimizer.param_groups[0]["lr"] and init.sched_best == m.scheduler.best
        seen.append((init.lr, init.num_bad_epochs, init.cooldown_counter, init.last_epoch))
    assert seen[0] == (lr0, 0, 0, 0) and seen[-1] == (lr0 / 2, 1, 0, 7)        # a fresh scheduler ... one far along
    assert seen[4] == (lr0 / 2, 0, 2, 4) and seen[5][2] == 1                    # the reduction, and the cool-down after it


class _Event:
    def __init__(self, slot, trace):
        self.slot, self.trace = slot, trace

    def record(self):
        self.trace.append(("copy", self.slot))

    def synchronize(self):
        self.trace.append(("read", self.slot))


def _stub_form(launches):
    """A form of `fit._DeviceFit` without a device: its "controller" runs at once on host bytes and stops the fit on epoch
    `stop_epoch`; `_issue` only counts."""
    import torch
    from hcatgnet_amd import fit

    class Block:
        def __init__(self, trace):
            self.state_dev, self.trace = torch.zeros(ctypes.sizeof(_lib.FitState), dtype=torch.uint8), trace

        def pinned(self, lookahead):
            return (torch.zeros(lookahead + 1, self.state_dev.numel(), dtype=torch.uint8),
                    [_Event(s, self.trace) for s in range(lookahead + 1)])

    class Stub(fit._DeviceFit):
        stop_epoch, trace = None, None

        def _resolve(self):
            self.trace, self.chunks = [], []
            self.block = Block(self.trace)

        def _issue(self, first, end):
            self.chunks.append((first, end))
            if first <= self.stop_epoch < end:
                st = _lib.FitState()
                st.stopped = 1
                self.block.state_dev.copy_(torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8))
            return launches(end - first, self.every)
    return Stub


# control epoch c is epoch c * every and ends chunk c.  The host reads control epoch c - lookahead behind chunk c, so a stop
# on control epoch 2 is seen behind chunk 2 + lookahead: 1 + (2 + lookahead) * every epochs and 3 + lookahead state copies
# are out by then, copy k in slot k % (lookahead + 1)
SKELETON = [(0, 7, 3, [0, 0, 0], [0, 0, 0]), (1, 10, 4, [0, 1, 0, 1], [0, 1, 0]), (2, 13, 5, [0, 1, 2, 0, 1], [0, 1, 2])]


@pytest.mark.parametrize("form", ["epoch", "chunk"])
@pytest.mark.parametrize("lookahead,issued,controls,copies,reads", SKELETON)
def test_the_run_skeleton_reads_the_stop_lookahead_intervals_behind(form, lookahead, issued, controls, copies, reads):
    import torch
    from hcatgnet_amd.fit import chunk_launches
    count = {"epoch": lambda n, every: 3 * n, "chunk": lambda n, every: 1 if n == every else n}[form]
    m = H.make_network("GCN", H.default_options(), 25)
    m.scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(m.optimizer, mode="min")
    Stub = _stub_form(count)
    Stub.stop_epoch = 6
    run = Stub(m, None, None, None, 40, 6, 3, lookahead)
    assert (run.issued, run.controls, run.graph_launches, run.done) == (0, 0, 0, False)
    while not run.done:
        run.issue_chunk()
        assert run.check() is run.done
    assert (run.issued, run.controls, run.stop_seen) == (issued, controls, True)
    assert run.chunks == [(0, 1)] + [(a, a + 3) for a in range(1, issued, 3)]
    assert [s for what, s in run.trace if what == "copy"] == copies and [s for what, s in run.trace if what == "read"] == reads
    assert run.graph_launches == (3 * issued if form == "epoch" else chunk_launches(issued, 3)) and run.enqueue_s > 0
    # the epochs run out before the stop is read: 8 epochs, the stop on control epoch 2 = epoch 6, one interval of look-ahead
    Stub.stop_epoch = 6
    run = Stub(m, None, None, None, 8, 6, 3, 1)
    while not run.done:
        run.issue_chunk()
        run.check()
    assert (run.issued, run.controls, run.stop_seen, run.done) == (8, 3, False, True)
    assert run.chunks == [(0, 1), (1, 4), (4, 7), (7, 8)] and [s for what, s in run.trace if what == "copy"] == [0, 1, 0]


def test_both_device_forms_are_the_one_skeleton():
    """`issue_chunk`, `check` and `finish` are the base's alone; each form says only what differs; the controller's first
    state and its argument struct are each made in one place."""
    from hcatgnet_amd import fit
    assert fit._EpochFit.form == "device" and fit._ChunkFit.form == "device-chunk"
    for form in (fit._EpochFit, fit._ChunkFit):
        assert issubclass(form, fit._DeviceFit) and form.__init__ is fit._DeviceFit.__init__
        for shared in ("issue_chunk", "check", "finish", "_resolve"):
            assert shared not in vars(form) and getattr(form, shared) is getattr(fit._DeviceFit, shared)
        assert {"_bind", "_issue", "_settle_generator"} <= set(vars(form))
    src = open(fit.__file__).read()
    assert src.count("init.sched_best") == 1 and src.count("FitControlArgs()") == 1


def test_fit_arguments_are_validated_before_anything_runs():
    from hcatgnet_amd.fit import fit_network, fit_networks
    assert H.fit_network is fit_network and H.fit_networks is fit_networks and H.FitResult._fields[:7] == (
        "log", "epochs_run", "stopped_early", "best_epoch", "best_val", "best_state", "epochs_enqueued")
    m = H.make_network("GCN", H.default_options(), 25)
    for kw in (dict(epochs=0), dict(control_every=0), dict(lookahead=-1)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            fit_network(m, None, None, None, "cpu", **kw)
        with pytest.raises(ValueError, match=next(iter(kw))):
            fit_networks([m], [None], [None], [None], "cpu", **kw)
    with pytest.raises(ValueError, match="per model"):
        fit_networks([m, m], [None, None], [None], [None, None], "cpu")
    with pytest.raises(ValueError, match="per model"):
        fit_networks([m], [None], [None], [None], "cpu", active=[True, False])
