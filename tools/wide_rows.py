"""Per-launch time of ``Flow.log_prob`` and ``Flow.sample`` on event sizes above 256 (public API only, so that it runs on
any commit of this package): RealNVP((1, 28, 28)) at the preset's default 2 layers and at 8, RealNVP(1024, n_layers=8), each
over 2^16 resident rows -- HIP events around every call, the median of 100 after warm-up.

    python tools/wide_rows.py [--rows 65536] [--reps 100] [--tag NAME]

One JSON line per (model, call): us per launch, evals/s, the HBM floor (2 N D + N) * 4 bytes (rows in, rows out, one
log-probability; log_prob, which writes no rows, is held to the same floor) over ``--stream-tbs`` (default 5.5 TB/s, what
the per-layer kernels reach, profiles/), and the fraction of that floor achieved.
"""
import argparse
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn, reps, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)                   # us
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--stream-tbs", type=float, default=5.5)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/wide_rows.py needs a GPU")
    import torchflows_amd as tfa
    warnings.simplefilter("ignore")
    N = args.rows
    models = (("RealNVP((1,28,28))", (1, 28, 28), {}), ("RealNVP((1,28,28), n_layers=8)", (1, 28, 28), dict(n_layers=8)),
              ("RealNVP(1024, n_layers=8)", (1024,), dict(n_layers=8)))
    for name, es, kw in models:
        torch.manual_seed(0)
        flow = tfa.Flow(tfa.RealNVP(es if len(es) > 1 else es[0], **kw))
        flow.train()
        with torch.no_grad():
            flow.log_prob(torch.randn(256, *es))              # ActNorm's data-dependent initialisation (host)
        flow = flow.eval().cuda()
        D = 1
        for v in es:
            D *= v
        x = torch.randn(N, *es, device="cuda")
        floor_us = (2 * N * D + N) * 4 / (args.stream_tbs * 1e12) * 1e6
        with torch.no_grad():
            calls = (("log_prob", lambda: flow.log_prob(x)),
                     ("sample", lambda: flow.sample((N,), return_log_prob=True)))
            for what, fn in calls:
                us = timed(fn, args.reps)
                med = statistics.median(us)
                print(json.dumps(dict(tag=args.tag, model=name, call=what, rows=N, D=D, us_per_launch=round(med, 1),
                                      us_min=round(min(us), 1), us_p90=round(sorted(us)[int(0.9 * len(us))], 1),
                                      evals_per_s=round(N / med * 1e6), hbm_floor_us=round(floor_us, 1),
                                      floor_fraction=round(floor_us / med, 3))), flush=True)


if __name__ == "__main__":
    main()
