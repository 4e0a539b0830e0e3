"""CPU-side tests of the chunk form of a fit (hcatgnet_amd/fit.py) and of the shuffle drawn on the device (csrc/shuffle.hip):
`store.pcg64_permutation` -- the kernel's draw in plain Python and its oracle on the GPU -- against numpy's own
`Generator.permutation`, the generator's state to the device struct and back, the new structs' sizes, argument validation of
the draw launch and of `form`.  No GPU."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import hcatgnet_amd as H
from hcatgnet_amd import _lib
from hcatgnet_amd import store as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS, SIZES, DRAWS = (0, 5, 20232023), (1, 2, 3, 40, 41, 535), 4


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def test_the_restated_draw_is_numpys_permutation():
    """Seeds {0, 5, 20232023} x n in {1, 2, 3, 40, 41, 535}, four consecutive draws each: the permutation and the state after
    every draw (has_uint32 and uinteger included) are numpy's.  Some compared draws start with a buffered half."""
    buffered = 0
    for seed in SEEDS:
        for n in SIZES:
            rng = np.random.default_rng(seed)
            state = rng.bit_generator.state
            for d in range(DRAWS):
                buffered += int(state["has_uint32"] == 1 and n > 1)
                arg, before = state, dict(state, state=dict(state["state"]))
                want = rng.permutation(n)
                got, state = S.pcg64_permutation(arg, n)
                assert arg == before                                            # (the argument is not modified)
                assert got == want.tolist(), (seed, n, d)
                assert state == rng.bit_generator.state, (seed, n, d)
    assert buffered >= 1


def test_a_draw_of_one_graph_draws_nothing():
    state = np.random.default_rng(3).bit_generator.state
    got, after = S.pcg64_permutation(state, 1)
    assert got == [0] and after == state


def test_the_state_goes_to_the_device_struct_and_back_without_loss():
    for seed in SEEDS:
        rng = np.random.default_rng(seed)
        for n in (0, 3, 535):               # (a fresh state, one with a buffered half, one far along)
            if n:
                rng.permutation(n)
            state = rng.bit_generator.state
            g = S.pcg64_to_struct(state)
            assert S.pcg64_from_struct(g) == state
            again = S.pcg64_from_struct(_lib.Pcg64.from_buffer_copy(bytes(g)))  # (through the bytes that travel)
            assert again == state
            other = np.random.default_rng(99)
            other.bit_generator.state = again
            assert other.permutation(41).tolist() == np.random.Generator(_with_state(state)).permutation(41).tolist()
    with pytest.raises(ValueError, match="PCG64"):
        S.pcg64_to_struct(np.random.Generator(np.random.Philox(1)).bit_generator.state)
    with pytest.raises(ValueError, match="PCG64"):
        S.pcg64_permutation(np.random.Generator(np.random.Philox(1)).bit_generator.state, 4)


def _with_state(state):
    bg = np.random.PCG64()
    bg.state = state
    return bg


def test_draw_structs_match_the_header():
    """sizeof(hcg_epoch_draw_args), sizeof(hcg_pcg64) and sizeof(hcg_collate_args) (whose `epoch_draw` carries the launch) as
    a C compiler sees the header = the ctypes mirrors = what the library was built with."""
    cc = next((p for p in (shutil.which(n) for n in ("cc", "gcc", "clang", "c++", "g++", "hipcc")) if p), None)
    if cc is None:
        cc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write('#include <stdio.h>\n#include "hcatgnet_hip.h"\nint main(void) { printf("%zu %zu %zu %d", '
                             'sizeof(hcg_epoch_draw_args), sizeof(hcg_pcg64), sizeof(hcg_collate_args), '
                             'HCG_EPOCH_DRAW_MAX_GRAPHS); return 0; }\n')
        subprocess.run([cc, "-I", os.path.join(REPO, "include"), src, "-o", exe], check=True, capture_output=True)
        *sizes, cap = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    lib = _lib.load()
    mirrors = [(_lib.EpochDrawArgs, _lib.HCG_STRUCT_EPOCH_DRAW_ARGS), (_lib.Pcg64, _lib.HCG_STRUCT_PCG64),
               (_lib.CollateArgs, _lib.HCG_STRUCT_COLLATE_ARGS)]
    for size, (mirror, which) in zip(sizes, mirrors):
        assert ctypes.sizeof(mirror) == size == lib.hcg_struct_bytes(which), mirror
    assert ctypes.sizeof(_lib.Pcg64) == 40
    assert cap == _lib.HCG_EPOCH_DRAW_MAX_GRAPHS
    from hcatgnet_amd.train import EpochWindow
    assert cap >= EpochWindow.MAX_BATCHES                     # (64 batches of any size down to one graph fit a launch)


def test_a_malformed_draw_block_is_refused_on_the_host():
    """`hcg_collate` with `epoch_draw` set validates the block before it touches a GPU (stream NULL, made-up addresses)."""
    lib = _lib.load()
    c, d = _lib.CollateArgs(), _lib.EpochDrawArgs()
    c.epoch_draw = ctypes.addressof(d)
    call = lambda: lib.hcg_collate(ctypes.byref(c), None)
    assert call() == -1                                                          # nothing set
    c.node_ptr_all, c.edge_ptr_all = 0x1000, 0x2000
    d.rng, d.layout, d.G, d.batch_size = 0x3000, 0x4000, 40, 0
    assert call() == -1                                                          # batch_size < 1
    d.batch_size, d.G = 40, 0
    assert call() == -1                                                          # no graphs
    d.G, d.drop_last = 40, 2
    assert call() == -1                                                          # drop_last is 0 or 1
    d.drop_last, d.rng = 0, 0
    assert call() == -1                                                          # no generator
    d.rng, d.layout = 0x3000, 0x4004
    assert call() == -1                                                          # a layout that is not 8-byte aligned
    d.layout, d.gate, d.gate_max_epochs = 0x4000, 0x5000, 0
    assert call() == -1                                                          # a gate without max_epochs
    d.gate, d.reserved = 0, 1
    assert call() == -1                                                          # reserved word set
    d.reserved, d.G = 0, _lib.HCG_EPOCH_DRAW_MAX_GRAPHS + 1
    assert call() == _lib.HCG_ERR_UNSUPPORTED                                    # past the cap
    # without the block the struct is a collate as before: refused for its own reasons (no slots)
    c.epoch_draw = None
    assert call() == -1


def test_eligibility_of_a_loader_is_decided_on_the_host():
    class FakeStore:
        def __init__(self, n):
            self.n = n

        def __len__(self):
            return self.n

    class FakeLoader:
        def __init__(self, n, rng):
            self.store, self.rng = FakeStore(n), rng
    assert S.DeviceGenerator.reason(FakeLoader(535, np.random.default_rng(1))) is None
    assert "PCG64" in S.DeviceGenerator.reason(FakeLoader(535, np.random.Generator(np.random.Philox(1))))
    assert "PCG64" in S.DeviceGenerator.reason(FakeLoader(535, np.random.Generator(np.random.PCG64DXSM(1))))
    assert "PCG64" in S.DeviceGenerator.reason(FakeLoader(535, np.random.RandomState(1)))
    assert "graphs" in S.DeviceGenerator.reason(FakeLoader(_lib.HCG_EPOCH_DRAW_MAX_GRAPHS + 1, np.random.default_rng(1)))
    assert S.DeviceGenerator.reason(FakeLoader(_lib.HCG_EPOCH_DRAW_MAX_GRAPHS, np.random.default_rng(1))) is None


def test_form_is_validated_before_anything_runs():
    from hcatgnet_amd.fit import FORMS, fit_network, fit_networks
    assert FORMS == ("epoch", "chunk") and H.FitResult._fields[-1] == "graph_launches"
    assert H.FitResult._field_defaults["graph_launches"] == 0 and H.FitResult._field_defaults["form"] == "device"
    m = H.make_network("GCN", H.default_options(), 25)
    for bad in ("graph", "", None, "Chunk"):
        with pytest.raises(ValueError, match="form"):
            fit_network(m, None, None, None, "cpu", form=bad)
        with pytest.raises(ValueError, match="form"):
            fit_networks([m], [None], [None], [None], "cpu", form=bad)
    for kw in (dict(epochs=0), dict(control_every=0), dict(lookahead=-1)):      # (the other checks hold in the new form too)
        with pytest.raises(ValueError, match=next(iter(kw))):
            fit_network(m, None, None, None, "cpu", form="chunk", **kw)


def test_chunk_schedule_launch_counts():
    """The launches a fit of `epochs` epochs at `control_every` issues in the chunk form: epoch 0, the full intervals, the tail."""
    from hcatgnet_amd.fit import chunk_launches
    assert chunk_launches(250, 5) == 1 + 49 + 4
    assert chunk_launches(251, 5) == 1 + 50
    assert chunk_launches(40, 2) == 1 + 19 + 1
    assert chunk_launches(7, 3) == 1 + 2
    assert chunk_launches(8, 3) == 1 + 2 + 1
    assert chunk_launches(1, 5) == 1 and chunk_launches(3, 5) == 3 and chunk_launches(6, 1) == 6
