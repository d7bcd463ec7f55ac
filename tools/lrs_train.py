"""Step times of CouplingLRS(64, n_layers=8) training on one MI355X: the fused route (one lean program + one
tfk_rqs_coupling_train_bwd launch with the LRS flag + three tfk_rows_outer per coupling) against this build's
TORCHFLOWS_AMD_DEBUG=train_fused=0 route (layer by layer, GEMM-library calls), alternating, median of the calls.

  fit   the Flow.fit step at batch 1 024 (40 steps per call; the fused route is captured into a hipGraph)
  mle   one maximum-likelihood step (log_prob.mean().backward()) on 2^18 rows

    python tools/lrs_train.py [--calls 7]        ->  one JSON line
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchflows_amd import CouplingLRS, Flow  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.manual_seed(0)
    flow = Flow(CouplingLRS(64, n_layers=8)).cuda()
    data = torch.randn(40 * 1024, 64, device="cuda") * 0.7 + 0.2
    big = torch.randn(1 << 18, 64, device="cuda") * 0.7 + 0.2
    flow.train()
    with torch.no_grad():
        flow.log_prob(data)                                   # data-dependent init

    def fit_step_ms(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f.fit(data, n_epochs=1, lr=1e-4, batch_size=1024, shuffle=False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / 40

    def mle_step_ms(f):
        for p in f.parameters():
            p.grad = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        (-f.log_prob(big).mean()).backward()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    routes = {"fused": "", "train_fused=0": "train_fused=0"}
    times = {leg: {r: [] for r in routes} for leg in ("fit", "mle")}
    for call in range(args.calls + 1):                        # the first call of each route warms up
        for route, env in routes.items():
            os.environ["TORCHFLOWS_AMD_DEBUG"] = env
            f = copy.deepcopy(flow)
            for leg, fn in (("fit", fit_step_ms), ("mle", mle_step_ms)):
                ms = fn(f)
                if call:
                    times[leg][route].append(ms)
    out = {leg: {r: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for r, v in by.items()}
           for leg, by in times.items()}
    print(json.dumps({"model": "CouplingLRS(64, n_layers=8)", "calls": args.calls, **out}))


if __name__ == "__main__":
    main()
