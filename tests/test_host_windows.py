"""Host-side pieces of the graph windows and epoch loops (no GPU): the epoch's index layout, the loader-window cache,
the argument checks of the several-runs loops."""
import numpy as np
import pytest

from hcatgnet_amd import _lib, train
from hcatgnet_amd.store import epoch_layout

N_HOST = np.array([3, 5, 4, 9, 6, 7, 8], np.int64)           # G = 7 graphs
E_HOST = np.array([4, 8, 0, 16, 10, 12, 14], np.int64)       # (one graph without edges)
ORDER = np.array([4, 0, 6, 2, 5, 1, 3], np.int64)
ORDER_2 = np.array([6, 5, 4, 3, 2, 1, 0], np.int64)


def _check_layout(buf, spans, tot, order, bs, drop_last):
    """The layout, restated: batch k is order[k * bs:(k + 1) * bs] (a short last batch unless `drop_last`); behind the G ids,
    its graph_ptr = [0, cumsum(nodes)] as int32 from the next int64 word on, its edge_ptr 2 * tot int32 further."""
    G = len(order)
    n_batches = G // bs if drop_last else -(-G // bs)
    assert len(spans) == n_batches
    assert buf.dtype == np.int64 and buf.size == G + 2 * tot
    assert tot == sum(-(-(min(bs, G - k * bs) + 1) // 2) for k in range(n_batches))     # words of B + 1 int32, rounded up
    ptr32 = buf[G:].view(np.int32)
    # (the ids of graphs that `drop_last` leaves out stay in the ids block, as the loader has always uploaded them)
    assert np.array_equal(buf[:G], order)
    untouched = np.ones(ptr32.size, bool)
    off_want = 0
    for k, (i, B, off) in enumerate(spans):
        assert (i, B, off) == (k * bs, min(bs, G - k * bs), off_want)
        assert off % 2 == 0                                                              # every block starts on a word
        ids = buf[i:i + B]
        assert np.array_equal(ids, order[i:i + B])
        assert np.array_equal(ptr32[off:off + B + 1], np.concatenate([[0], np.cumsum(N_HOST[ids])]))
        assert np.array_equal(ptr32[2 * tot + off:2 * tot + off + B + 1], np.concatenate([[0], np.cumsum(E_HOST[ids])]))
        untouched[off:off + B + 1] = untouched[2 * tot + off:2 * tot + off + B + 1] = False
        off_want += 2 * (-(-(B + 1) // 2))
    assert not ptr32[untouched].any()                                                    # every other word is zero


@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("bs", [3, 4, 8])
def test_epoch_layout_matches_its_restatement(bs, drop_last):
    """Batch sizes 3 and 4: odd and even B + 1 (the word rounding); 8: one short batch, or none at all with `drop_last`.  A
    second call into the same buffer with another permutation leaves no stale word."""
    buf, spans, tot = epoch_layout(N_HOST, E_HOST, bs, drop_last, ORDER)
    _check_layout(buf, spans, tot, ORDER, bs, drop_last)
    if bs == 8 and drop_last:
        assert spans == [] and tot == 0 and buf.size == 7
    again, spans_2, tot_2 = epoch_layout(N_HOST, E_HOST, bs, drop_last, ORDER_2, out=buf)
    assert again is buf and spans_2 == spans and tot_2 == tot
    _check_layout(buf, spans_2, tot_2, ORDER_2, bs, drop_last)
    fresh, _, _ = epoch_layout(N_HOST, E_HOST, bs, drop_last, ORDER_2)
    assert fresh.tobytes() == buf.tobytes()


class _Loader:
    key = "k"


class _SlotsLoader:
    __slots__ = ()
    key = "k"


class _Windows:
    """A `_LoaderWindows` kind over stand-ins, with counting callables.  `stale` launches raise HcgError; `builds_none`:
    the build gives None."""

    def __init__(self, stale=0, builds_none=False):
        self.built = self.launched = self.drawn = 0
        self.stale, self.builds_none = stale, builds_none
        self.kind = train._LoaderWindows("_win", lambda model, loader: loader.key, self.build, self.launch, self.draw)

    def build(self, model, loader):
        self.built += 1
        return None if self.builds_none else ["window", self.built]

    def draw(self, win):
        self.drawn += 1
        return ("order", self.drawn)

    def launch(self, win, drawn):
        self.launched += 1
        if self.launched <= self.stale:
            raise _lib.HcgError("stale")
        return (win[1], drawn)


def test_loader_window_is_built_once_per_model_and_key():
    w, loader, model = _Windows(), _Loader(), object()
    assert w.kind.of(model, loader) is None and w.built == 0                 # a look builds nothing
    win, got = w.kind.launch(model, loader)
    assert (win, got) == (["window", 1], (1, ("order", 1)))
    assert w.kind.launch(model, loader)[0] is win and w.built == 1 and w.launched == 2 and w.drawn == 2
    assert w.kind.of(model, loader) is win
    loader.key = "other"                                                      # another key: built again
    assert w.kind.of(model, loader) is None
    assert w.kind.launch(model, loader)[0] == ["window", 2] and w.built == 2
    other = object()                                                          # another model object: built again
    assert w.kind.of(other, loader) is None
    assert w.kind.launch(other, loader)[0] == ["window", 3] and w.built == 3
    assert w.kind.of(other, loader, build=True) == ["window", 3] and w.built == 3
    loader.key = None                                                         # the kind does not apply: nothing is built
    assert w.kind.launch(other, loader) is None and w.kind.of(other, loader, build=True) is None and w.built == 3


def test_loader_window_keeps_a_failed_build():
    w, loader, model = _Windows(builds_none=True), _Loader(), object()
    assert w.kind.launch(model, loader) is None and w.kind.launch(model, loader) is None
    assert w.kind.of(model, loader, build=True) is None
    assert w.built == 1 and w.launched == 0
    loader.key = "other"
    assert w.kind.launch(model, loader) is None and w.built == 2


def test_loader_window_rebuilds_once_when_its_launch_is_stale():
    w, loader, model = _Windows(stale=1), _Loader(), object()
    win, got = w.kind.launch(model, loader)
    assert (w.built, w.launched, w.drawn) == (2, 2, 1)                        # one rebuild; the permutation drawn once
    assert win == ["window", 2] and got == (2, ("order", 1))
    assert w.kind.of(model, loader) is win
    w = _Windows(stale=2)
    assert w.kind.launch(model, _Loader()) is None
    assert (w.built, w.launched, w.drawn) == (2, 2, 1)


def test_loader_window_on_a_loader_that_refuses_attributes():
    w, loader, model = _Windows(), _SlotsLoader(), object()
    assert w.kind.launch(model, loader) == (["window", 1], (1, ("order", 1)))
    assert w.kind.of(model, loader) is None                                   # nothing was kept
    assert w.kind.launch(model, loader)[0] == ["window", 2]
    w = _Windows(stale=1)
    assert w.kind.launch(model, loader) is None and (w.built, w.launched) == (1, 1)


def test_the_window_accessors_are_the_two_kinds_of_train_network_and_eval_network():
    assert train.epoch_window_of.__self__ is train._EPOCH_WINDOWS and train._EPOCH_WINDOWS.attr == "_hcg_epoch_window"
    assert train.eval_window_of.__self__ is train._EVAL_WINDOWS and train._EVAL_WINDOWS.attr == "_hcg_eval_window"
    assert train.epoch_window_of(object(), _Loader()) is None                 # no DeviceLoader: neither kind applies
    assert train.eval_window_of(object(), _Loader(), build=True) is None


@pytest.mark.parametrize("fn", ["train_networks", "eval_networks"])
def test_several_runs_need_one_loader_and_one_flag_per_model(fn):
    run = getattr(train, fn)
    with pytest.raises(ValueError, match=f"^{fn}: one loader \\(and one `active` flag\\) per model$"):
        run([object()], [], "cuda")
    with pytest.raises(ValueError, match=f"^{fn}: one loader"):
        run([object(), object()], [object(), object()], "cuda", active=[True])
