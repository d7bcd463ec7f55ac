"""Per-launch time of the deep sigmoidal kernels (csrc/tfk_dsf.hip) and of ``Flow.log_prob`` / ``Flow.sample`` of
``CouplingDeepSF(64, n_layers=8)`` over 2^16 resident rows -- the protocol of tools/wide_rows.py: HIP events around every
call, the median of 100 after warm-up.

    python tools/dsf_rows.py [--rows 65536] [--reps 100] [--aten-reps 5] [--tag NAME]

One JSON line per measurement:
  * ``tfk_dsf_coupling_fwd`` / ``tfk_dsf_coupling_inv`` alone, on the rows and the parameters h the flow's first coupling
    sees (its own conditioner's output): us per launch and, for fwd, the fraction of the HBM floor
    (2 N D + N T P + N) * 4 bytes over ``--stream-tbs`` (default 5.5 TB/s); for inv the mean bisection trip count, counted
    by re-enacting the kernel's rule (midpoint until it stops moving, at most 64 times) with ATen ops on the first
    4 096 rows;
  * ``log_prob`` and ``sample`` of the whole flow on the kernels;
  * the same two calls with the transformer forced onto the ATen composite path (TORCHFLOWS_AMD_DEBUG="dsf=0"): this
    build's own fallback, the only comparison there is -- no earlier release runs these models.
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


def trip_counts(tr, z, h, max_trips=64):
    """Bisection trips per element under the kernel's rule, components last to first (ATen re-enactment)."""
    trips = torch.zeros_like(z)
    start = tr.n_parameters_per_element
    for comp in reversed(tr.components):
        P = comp.n_parameters_per_element
        start -= P
        hc = h[..., start:start + P].reshape(-1, P)
        y = z.reshape(-1)
        lo, hi, mid = torch.full_like(y, -10.0), torch.full_like(y, 10.0), torch.zeros_like(y)
        live = torch.ones_like(y, dtype=torch.bool)
        n = torch.zeros_like(y)
        for _ in range(max_trips):
            below = comp.forward_1d(mid, hc)[0] < y
            lo, hi = torch.where(below, mid, lo), torch.where(below, hi, mid)
            nxt = (lo + hi) / 2
            n += live
            live = live & (nxt != mid)
            mid = nxt                                         # (a settled element keeps reproducing its midpoint)
            if not bool(live.any()):
                break
        trips += n.view_as(z)
        z = mid.view_as(z)
    return trips


def report(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--aten-reps", type=int, default=5)
    ap.add_argument("--stream-tbs", type=float, default=5.5)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/dsf_rows.py needs a GPU")
    import torchflows_amd as tfa
    from torchflows_amd import native
    warnings.simplefilter("ignore")
    N, D = args.rows, 64
    name = "CouplingDeepSF(64, n_layers=8)"
    torch.manual_seed(0)
    flow = tfa.Flow(tfa.CouplingDeepSF(D, n_layers=8))
    flow.train()
    with torch.no_grad():
        flow.log_prob(torch.randn(256, D))                    # ActNorm's data-dependent initialisation (host)
    flow = flow.eval().cuda()
    x = torch.randn(N, D, device="cuda")

    def stats(us):
        return dict(us_per_launch=round(statistics.median(us), 1), us_min=round(min(us), 1),
                    us_p90=round(sorted(us)[int(0.9 * len(us))], 1))

    with torch.no_grad():
        # the transformer launches alone, on the first coupling's own inputs
        layer = next(l for l in flow.bijection.layers if hasattr(l, "coupling"))
        tr, T = layer.transformer, layer.coupling.target_event_size
        C, K = tr.n_components, tr.hidden_dim
        P = 3 * K * C
        h = layer.conditioner_transform(x[:, :layer.coupling.source_event_size].contiguous()).reshape(N, -1).contiguous()
        out, ld = torch.empty_like(x), torch.empty(N, device="cuda")
        floor_us = (2 * N * D + N * T * P + N) * 4 / (args.stream_tbs * 1e12) * 1e6
        s = stats(timed(lambda: native.dsf_coupling(x, h, out, ld, None, T, C, K), args.reps))
        report(tag=args.tag, model=name, call="tfk_dsf_coupling_fwd", rows=N, D=D, T=T, n_components=C, hidden_dim=K, **s,
               hbm_floor_us=round(floor_us, 1), floor_fraction=round(floor_us / s["us_per_launch"], 3))
        z = out.clone()
        s = stats(timed(lambda: native.dsf_coupling(z, h, out, ld, None, T, C, K, inverse=True), args.reps))
        n = min(N, 4096)
        trips = trip_counts(tr, z[:n, D - T:], h[:n].view(n, T, P))
        report(tag=args.tag, model=name, call="tfk_dsf_coupling_inv", rows=N, D=D, T=T, n_components=C, hidden_dim=K, **s,
               mean_trips_per_component=round(float(trips.mean()) / C, 2), max_trips_per_element=int(trips.max()),
               round_trip_max_abs=float((out[:, D - T:] - x[:, D - T:]).abs().max()))
        # the whole flow, on the kernels and with the transformer on the ATen path
        calls = (("log_prob", lambda: flow.log_prob(x)), ("sample", lambda: flow.sample((N,), return_log_prob=True)))
        for path, reps in (("libtfk", args.reps), ("aten fallback of this build (dsf=0)", args.aten_reps)):
            if reps <= 0:
                continue
            prev = os.environ.get("TORCHFLOWS_AMD_DEBUG")
            if path != "libtfk":
                os.environ["TORCHFLOWS_AMD_DEBUG"] = ",".join(v for v in (prev, "dsf=0") if v)
            try:
                for what, fn in calls:
                    before = native.calls
                    fn()
                    launches = native.calls - before
                    s = stats(timed(fn, reps, warmup=2 if path != "libtfk" else 10))
                    report(tag=args.tag, model=name, call=what, path=path, rows=N, D=D, libtfk_launches=launches, **s,
                           evals_per_s=round(N / s["us_per_launch"] * 1e6))
            finally:
                if prev is None:
                    os.environ.pop("TORCHFLOWS_AMD_DEBUG", None)
                else:
                    os.environ["TORCHFLOWS_AMD_DEBUG"] = prev


if __name__ == "__main__":
    main()
