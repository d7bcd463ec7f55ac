"""``Flow.log_prob`` / ``Flow.sample`` of ``CouplingDenseSF(64, n_layers=8)`` and ``CouplingDeepDenseSF(64, n_layers=8)`` over
2^14 resident rows on the dense sigmoidal kernel (csrc/tfk_dense_dsf.hip) against this build's own ATen composite path
(TORCHFLOWS_AMD_DEBUG="dense=0") -- the protocol of tools/dsf_rows.py: HIP events around every call, the median of the
timed calls after warm-up, the two routes ALTERNATING in one process.

    python tools/dense_rows.py [--rows 16384] [--reps 20] [--tag NAME]

One JSON line per measurement:
  * ``tfk_dsf_coupling_fwd`` / ``_inv`` of the first coupling alone, on its own conditioner's predicted block: us per
    launch; for fwd the HBM floor (N n_predicted + 2 N D + N) * 4 bytes over ``--stream-tbs`` (default 5.5 TB/s); for inv
    the mean bisection trips per component, counted by re-enacting the kernel's rule with ATen ops on the first 512 rows;
  * ``log_prob`` and ``sample`` of the whole flow, route ``dense=1`` and ``dense=0``;
  * the training leg (``--train-rows``, default 2^12: the ATen graph keeps the composed (N, 32, 243 / 486) tensor of every
    layer): ``tfk_dsf_coupling_bwd`` of the first coupling alone (its gradient rows restored by a copy inside the timed
    call), then one maximum-likelihood step ``log_prob(x).mean().backward()`` on the reverse-mode kernel against
    ``dense_train=0`` (this build's ATen graph), alternating, with the peak allocated memory of a step of each.
``--legs eval`` / ``--legs train`` runs one of the two halves.
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

from tools.dsf_rows import report, timed  # noqa: E402


def set_route(on: bool):
    os.environ["TORCHFLOWS_AMD_DEBUG"] = "dense=1" if on else "dense=0"


def stats(us):
    return dict(us_per_call=round(statistics.median(us), 1), us_min=round(min(us), 1),
                us_p90=round(sorted(us)[int(0.9 * len(us))], 1))


def train_leg(args, flow, name, layer):
    """The reverse-mode launch of ``layer`` alone, then a maximum-likelihood step of ``flow`` on both routes."""
    from torchflows_amd import native
    from torchflows_amd.bijections.finite.autoregressive.layers_base import _dense_inputs
    N, D = args.train_rows, 64
    x = torch.randn(N, D, device="cuda")
    tr, T, S = layer.transformer, layer.coupling.target_event_size, layer.coupling.source_event_size
    C, L, H = tr.n_components, tr.n_dense_layers, tr.hidden_size
    set_route(True)
    with torch.no_grad():
        pred, desc = _dense_inputs(layer, x[:, :S].contiguous(), None, layer._target_index32)
        g0, g, gld = torch.randn_like(x), torch.empty_like(x), torch.randn(N, device="cuda")
        gh = torch.zeros(sum(native.dense_bwd_floats(N, T, tr.n_parameters_per_element, pred.shape[1])), device="cuda")
        s = stats(timed(lambda: (g.copy_(g0), native.dense_coupling_bwd(x, pred, g, gld, gh, desc, T, C, L, H)), args.reps))
        report(tag=args.tag, model=name, call="tfk_dsf_coupling_bwd", rows=N, T=T, n_predicted=pred.shape[1], **s)
    del gh, pred

    def step():
        flow.zero_grad(set_to_none=True)
        flow.log_prob(x).mean().backward()
    specs = {"dense_train=1": "dense=1,dense_train=1", "dense_train=0": "dense=1,dense_train=0"}
    us, extra = {}, {}
    for route, spec in specs.items():                            # warm-up of both routes, launches and peak memory of a step
        os.environ["TORCHFLOWS_AMD_DEBUG"] = spec
        step()
        step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = native.calls
        step()
        torch.cuda.synchronize()
        extra[route] = dict(libtfk_launches=native.calls - before,
                            peak_allocated_mib=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1))
        us[route] = []
    for _ in range(args.train_reps):                             # alternating: one timed step each
        for route, spec in specs.items():
            os.environ["TORCHFLOWS_AMD_DEBUG"] = spec
            us[route] += timed(step, 1, warmup=0)
    for route in specs:
        report(tag=args.tag, model=name, call="log_prob(x).mean().backward()", route=route, rows=N, **extra[route],
               **stats(us[route]))
    flow.zero_grad(set_to_none=True)


def trip_counts(tr, z, h, max_trips=64):
    """Bisection trips per element under the kernel's rule, components last to first (ATen re-enactment)."""
    comps = getattr(tr, "components", [tr])
    trips = torch.zeros_like(z)
    start = tr.n_parameters_per_element
    for comp in reversed(comps):
        start -= comp.n_parameters_per_element
        hc = [p.contiguous() for p in comp.split_parameters(h[..., start:start + comp.n_parameters_per_element])]
        lo, hi, mid = torch.full_like(z, -10.0), torch.full_like(z, 10.0), torch.zeros_like(z)
        live = torch.ones_like(z, dtype=torch.bool)
        for _ in range(max_trips):
            below = comp.forward_1d(mid, hc)[0] < z
            lo, hi = torch.where(below, mid, lo), torch.where(below, hi, mid)
            nxt = (lo + hi) / 2
            trips += live
            live = live & (nxt != mid)
            mid = nxt
            if not bool(live.any()):
                break
        z = mid
    return trips


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 14)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stream-tbs", type=float, default=5.5)
    ap.add_argument("--tag", default="")
    ap.add_argument("--train-rows", type=int, default=1 << 12)
    ap.add_argument("--train-reps", type=int, default=10)
    ap.add_argument("--legs", default="eval,train")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/dense_rows.py needs a GPU")
    import torchflows_amd as tfa
    from torchflows_amd import native
    from torchflows_amd.bijections.finite.autoregressive.layers_base import _dense_inputs
    warnings.simplefilter("ignore")
    N, D = args.rows, 64

    for ctor in (tfa.CouplingDenseSF, tfa.CouplingDeepDenseSF):
        name = f"{ctor.__name__}(64, n_layers=8)"
        torch.manual_seed(0)
        flow = tfa.Flow(ctor(D, n_layers=8))
        flow.train()
        with torch.no_grad():
            flow.log_prob(torch.randn(256, D))                    # ActNorm's data-dependent initialisation (host)
        flow = flow.eval().cuda()
        x = torch.randn(N, D, device="cuda")
        set_route(True)
        layer = next(l for l in flow.bijection.layers if hasattr(l, "coupling"))
        if "train" in args.legs:
            train_leg(args, flow, name, layer)
        if "eval" not in args.legs:
            continue
        with torch.no_grad():
            tr, T, S = layer.transformer, layer.coupling.target_event_size, layer.coupling.source_event_size
            C, L, H = tr.n_components, tr.n_dense_layers, tr.hidden_size
            pred, desc = _dense_inputs(layer, x[:, :S].contiguous(), None, layer._target_index32)
            out, ld = torch.empty_like(x), torch.empty(N, device="cuda")
            floor_us = (pred.numel() + 2 * N * D + N) * 4 / (args.stream_tbs * 1e12) * 1e6
            s = stats(timed(lambda: native.dense_coupling(x, pred, out, ld, desc, T, C, L, H), args.reps))
            report(tag=args.tag, model=name, call="tfk_dsf_coupling_fwd", rows=N, T=T, n_predicted=pred.shape[1],
                   parameters_per_row=T * tr.n_parameters_per_element, **s, hbm_floor_us=round(floor_us, 1))
            z = out.clone()
            s = stats(timed(lambda: native.dense_coupling(z, pred, out, ld, desc, T, C, L, H, inverse=True), args.reps))
            n = min(N, 512)
            h = layer.conditioner_transform(x[:n, :S].contiguous()).view(n, T, -1)
            trips = trip_counts(tr, z[:n].index_select(1, layer._target_index), h)
            report(tag=args.tag, model=name, call="tfk_dsf_coupling_inv", rows=N, T=T, **s,
                   mean_trips_per_component=round(float(trips.mean()) / C, 2))
            calls = (("log_prob", lambda: flow.log_prob(x)), ("sample", lambda: flow.sample((N,), return_log_prob=True)))
            for what, fn in calls:
                us = {True: [], False: []}
                for route in (True, False):                          # warm-up of both routes
                    set_route(route)
                    before = native.calls
                    fn()
                    launches = native.calls - before
                    us[route] = [launches]
                for _ in range(args.reps):                           # alternating: one timed call each
                    for route in (True, False):
                        set_route(route)
                        us[route] += timed(fn, 1, warmup=0)
                for route in (True, False):
                    report(tag=args.tag, model=name, call=what, route="dense=1" if route else "dense=0", rows=N,
                           libtfk_launches=us[route][0], **stats(us[route][1:]))
    os.environ.pop("TORCHFLOWS_AMD_DEBUG", None)


if __name__ == "__main__":
    main()
