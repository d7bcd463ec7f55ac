"""Child process of tests/test_gpu_wide_train.py::test_fit_is_captured_in_a_subprocess: ``Flow.fit`` of the first model of
the reference's image notebook with TORCHFLOWS_AMD_GRAPH=1 against the same fit with =0.  argv[1]: the value of the
``wide_train`` switch ("0": the layer-by-layer route -- nothing may be captured; the eager fit is skipped)."""
import copy
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
wide_train = sys.argv[1] if len(sys.argv) > 1 else "1"
os.environ["TORCHFLOWS_AMD_DEBUG"] = f"wide_train={wide_train}"
from torchflows_amd.flows import Flow  # noqa: E402
from torchflows_amd.bijections.finite.autoregressive.architectures import RealNVP  # noqa: E402

torch.manual_seed(0)
# 2 048 synthetic 28 x 28 images: a smooth blob at a random position on a noisy background
yy, xx = torch.meshgrid(torch.arange(28.0), torch.arange(28.0), indexing="ij")
cy, cx = torch.rand(2048, 1, 1) * 14 + 7, torch.rand(2048, 1, 1) * 14 + 7
x = (torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 18.0) + 0.1 * torch.randn(2048, 28, 28)).reshape(2048, 1, 28, 28).cuda()
flow = Flow(RealNVP((1, 28, 28), n_layers=2)).cuda()
flow.train()
with torch.no_grad():
    flow.log_prob(x)
flow.eval()
with torch.no_grad():
    before = float(flow.log_prob(x).mean())
graph, eager = copy.deepcopy(flow), copy.deepcopy(flow)
os.environ["TORCHFLOWS_AMD_GRAPH"] = "1"
graph.fit(x, n_epochs=3, lr=0.001, batch_size=256, shuffle=False)
out = {"before": before, "graph_stats": graph._fit_stats}
with torch.no_grad():
    out["after_graph"] = float(graph.log_prob(x).mean())
if wide_train != "0":
    os.environ["TORCHFLOWS_AMD_GRAPH"] = "0"
    eager.fit(x, n_epochs=3, lr=0.001, batch_size=256, shuffle=False)
    with torch.no_grad():
        out["after_eager"] = float(eager.log_prob(x).mean())
    out["eager_stats"] = eager._fit_stats
print(json.dumps(out))
