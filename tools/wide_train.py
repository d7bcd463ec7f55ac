"""Training-step times on event sizes above 256 (public API only, so that it runs on any commit of this package):

  * ``Flow.fit`` at batch 1 024, eager (TORCHFLOWS_AMD_GRAPH=0) and captured (=1): seconds of a fit over 8 batches x E epochs
    for E = 4 and E = 12, per-step time = the difference over the 64 extra steps (set-up, the two eager steps and the capture
    cancel), the median of ``--fits`` such pairs;
  * one maximum-likelihood step (log_prob, backward, AdamW) on 2^16 resident rows: HIP events around every step, the median
    of ``--reps`` after warm-up;
  * with ``--kernels`` (builds that have tfk_wide_coupling_train_bwd): the reverse-mode launch alone and the three
    tfk_rows_outer products alone at D = 784, against their algorithmic bytes (x 4D + g 8D + gh_rec 4 * 2hp + 2 * 64) * N and
    4 N (M + 16) per product.

for RealNVP((1, 28, 28)) with 3 and 8 layers and RealNVP(1024, n_layers=8).

    [TORCHFLOWS_AMD_LIB=<libtfk.so of another build>] [TORCHFLOWS_AMD_DEBUG=wide_train=0] \
        python tools/wide_train.py [--root <checkout whose package to import>] [--tag NAME] [--kernels]

``--root`` imports the package from another checkout (a parent commit next to this one: its Python and its library), so
both can be run alternately on one box.  One JSON line per measurement.
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--rows", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--fits", type=int, default=3)
    ap.add_argument("--tag", default="")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--skip-fit", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--models", default="", help="comma-separated indices into the model list (default: all three)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/wide_train.py needs a GPU")
    import torchflows_amd as tfa
    warnings.simplefilter("ignore")

    def emit(**kw):
        print(json.dumps(dict(tag=args.tag, **kw)), flush=True)

    def make(es, kw):
        torch.manual_seed(0)
        flow = tfa.Flow(tfa.RealNVP(es if len(es) > 1 else es[0], **kw))
        flow.train()
        with torch.no_grad():
            flow.log_prob(torch.randn(256, *es))              # ActNorm's data-dependent initialisation (host)
        return flow.eval().cuda()

    models = (("RealNVP((1,28,28), n_layers=3)", (1, 28, 28), dict(n_layers=3)),
              ("RealNVP((1,28,28), n_layers=8)", (1, 28, 28), dict(n_layers=8)),
              ("RealNVP(1024, n_layers=8)", (1024,), dict(n_layers=8)))
    if args.models:
        models = tuple(models[int(i)] for i in args.models.split(","))
    for name, es, kw in models:
        if not args.skip_fit:
            data = torch.randn(8 * 1024, *es, device="cuda")
            for mode in ("0", "1"):
                os.environ["TORCHFLOWS_AMD_GRAPH"] = mode
                per_step, stats = [], None
                make(es, kw).fit(data, n_epochs=4, lr=1e-3, batch_size=1024, shuffle=False)      # lazy state, untimed
                for _ in range(args.fits):
                    secs = {}
                    for epochs in (4, 12):
                        flow = make(es, kw)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        flow.fit(data, n_epochs=epochs, lr=1e-3, batch_size=1024, shuffle=False)
                        torch.cuda.synchronize()
                        secs[epochs] = time.perf_counter() - t0
                        stats = dict(flow._fit_stats)
                    per_step.append((secs[12] - secs[4]) / 64 * 1e3)
                emit(model=name, what="fit_step_ms", graph=mode, batch=1024, median=round(statistics.median(per_step), 4),
                     all=[round(v, 4) for v in per_step], fit_stats=stats)
            os.environ.pop("TORCHFLOWS_AMD_GRAPH", None)
        if args.skip_step:
            continue
        # one maximum-likelihood step on resident rows
        flow = make(es, kw)
        x = torch.randn(args.rows, *es, device="cuda")
        opt = torch.optim.AdamW(flow.parameters(), lr=1e-4)

        def step():
            opt.zero_grad(set_to_none=True)
            loss = -flow.log_prob(x).mean()
            loss.backward()
            opt.step()
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        emit(model=name, what="ml_step_ms", rows=args.rows, median=round(statistics.median(ms), 3), min=round(min(ms), 3),
             p90=round(sorted(ms)[int(0.9 * len(ms))], 3))
        del flow, x, opt

    if args.kernels:
        from torchflows_amd import autograd as ag, native
        D, H, N = 784, 14, args.rows
        dev = torch.device("cuda", torch.cuda.current_device())
        pack = ag._WideTrainPack.get(D, H, dev, False)
        lin1, lin2 = torch.nn.Linear(D // 2, H).cuda(), torch.nn.Linear(H, D).cuda()
        block = pack.pack(lin1, lin2)
        x, g, gld = torch.randn(N, D, device="cuda"), torch.randn(N, D, device="cuda"), torch.randn(N, device="cuda")
        gh, gpre, hid = pack.records(N)
        acc = torch.empty(pack.n_acc, device="cuda")
        lo2, lo3 = pack.GH * 16, (pack.GH + pack.hp) * 16
        g0 = g.clone()

        def kernel():
            native.wide_coupling_train_bwd(x, g, gld, block, gh, gpre, hid)

        def products():
            native.rows_outer(gh, pack.GH, hid, acc[:lo2])
            native.rows_outer(x, pack.hp, gpre, acc[lo2:lo3])
            native.rows_outer(gpre, 16, hid, acc[lo3:])
        bytes_k = (4 * D + 8 * D + 4 * pack.GH + 2 * 64) * N
        bytes_p = sum(4 * N * (M + 16) for M in (pack.GH, pack.hp, 16))
        for what, fn, nbytes in (("wide_bwd_kernel_us", kernel, bytes_k), ("rows_outer_x3_us", products, bytes_p)):
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            us = []
            for _ in range(args.reps):
                g.copy_(g0)                       # (the launch works in place: the same gradient rows every time)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                us.append(a.elapsed_time(b) * 1e3)
            med = statistics.median(us)
            emit(what=what, D=D, rows=N, median=round(med, 1), min=round(min(us), 1), algorithmic_bytes=nbytes,
                 tb_per_s=round(nbytes / med / 1e6, 3))


if __name__ == "__main__":
    main()
