"""GPU test of the fused step's per-layer plan (`train.layer_forms`): one `FusedTrainStep` step per route class, at the
smallest shapes that reach it, hands the step tail exactly the reduction jobs the support check predicted from the
batch's collate metadata (`FusedTrainStep._conv_jobs`) plus the head's.  What the forms compute is held by the suites of
the kernels themselves; which launches they issue by tests/test_host_layer_plan.py."""
import pytest
import torch

from hcatgnet_amd import _lib, synth
from hcatgnet_amd.train import FusedTrainStep
from tests.test_gpu_parity import H  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

# (graph sizes, F, D) -> families of the two layers on every part of the step, Ahat x columns of the dense first layer
ROUTES = {"tiles": ((30, 30, 30), 25, 64, ["tiles", "tiles"], 0),
          "size-grouped": ((30, 30, 40, 40), 25, 64, ["tiles", "tiles", "mid", "mid"], 0),
          "mid, dense first layer": ((70, 40), 25, 64, ["mid", "mid"], 32),
          "wide-layer": ((70, 70), 28, 128, ["tall", "tall"], 32)}


@pytest.mark.parametrize("route", list(ROUTES))
def test_the_tail_gets_the_jobs_the_plan_predicted(H, monkeypatch, route):
    sizes, F, D, fams, kp = ROUTES[route]
    graphs = []
    for i, n in enumerate(sizes):
        graphs += synth.make_batch(1, n, extra_bonds=3, max_degree=4, feat=F, seed=synth.BASE_SEED + i).as_graph_list()
    batch = H.collate(graphs, group_by_size=route == "size-grouped").to("cuda")
    torch.manual_seed(0)
    model = H.make_network("GCN", H.default_options(embedding_dim=D), F).cuda()
    step = FusedTrainStep(model)
    assert step.reason(batch) is None
    forms = [f for p in step._prepare(batch, False).parts for f in p.forms]
    assert [f.fam.name for f in forms] == fams and forms[0].kp == kp          # the shapes reach the route class

    # the step's last launch, with or without the optimiser's update riding in it (`optimizer.step_with_reduction` ends
    # there too): note the job count it is handed, then call through
    handed, real_tail = [], _lib.step_tail
    monkeypatch.setattr(_lib, "step_tail", lambda addr, n, *a, **kw: (handed.append(n), real_tail(addr, n, *a, **kw))[1])
    loss = step(batch)
    torch.cuda.synchronize()
    head_jobs = 1 if _lib.load().hcg_head_supported(D, 1) else 0
    assert len(handed) == 1 and handed[0] - head_jobs == FusedTrainStep._conv_jobs(model, batch, step)
    assert handed[0] - head_jobs == sum(f.jobs for f in forms)
    assert torch.isfinite(loss).item()
