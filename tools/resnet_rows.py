"""Per-launch time of the ResNet coupling kernel (csrc/tfk_glow_resnet.hip, kind 4 of tfk_glow_coupling) and of
``Flow.log_prob`` of ``MultiscaleRealNVP((3, 32, 32), use_resnet=True)`` over 2^14 resident rows -- the protocol of
tools/dsf_rows.py: HIP events around every call, the median of 100 after warm-up.

    python tools/resnet_rows.py [--rows 16384] [--reps 100] [--rounds 3] [--tag NAME]

One JSON line per measurement:
  * the program's first kind-4 launch alone (checkerboard coupling, conditioner image (3, 16, 32), T = 1 536): us per
    launch, the multiply-adds it executes per row (image_program.layer_cost) and the packed-fma floor of the trunk -- its
    multiply-adds at ``--fma-tmacs`` (default 55 TMAC/s, v_pk_fma_f32 as tools/micro/rates.hip measures it) -- with the
    share of it reached;
  * ``log_prob`` of the whole flow as a program and with TORCHFLOWS_AMD_IMAGE_PROGRAM=0 (THIS build's layer-by-layer route:
    the ResNet on ATen / MIOpen) -- the only comparison there is, no earlier release runs these models --, alternating
    ``--rounds`` times in one process, every round reported.
"""
import argparse
import copy
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


def stats(us):
    return dict(us_per_launch=round(statistics.median(us), 1), us_min=round(min(us), 1),
                us_p90=round(sorted(us)[int(0.9 * len(us))], 1))


def report(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 14)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--aten-reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fma-tmacs", type=float, default=55.0)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/resnet_rows.py needs a GPU")
    import torchflows_amd as tfa
    from torchflows_amd import image_program, native
    from torchflows_amd.bijections.finite.multiscale.architectures import MultiscaleRealNVP
    warnings.simplefilter("ignore")
    N, shape = args.rows, (3, 32, 32)
    name = "MultiscaleRealNVP((3, 32, 32), use_resnet=True)"
    torch.manual_seed(0)
    flow = tfa.Flow(MultiscaleRealNVP(shape, use_resnet=True))
    flow.train()
    with torch.no_grad():
        flow.log_prob(torch.randn(64, *shape))                # ActNorm / BatchNorm statistics (host)
    flow = flow.eval().cuda()
    flows = {"1": flow, "0": copy.deepcopy(flow)}             # (a compiled program stays cached on its module: one copy per route)
    x = torch.randn(N, *shape, device="cuda")
    with torch.no_grad():
        prog = image_program.get_program(flow.bijection, 0, x.device)
        step = next(s for s in prog.steps if s.layer.kind == 4)
        rows = x.reshape(N, -1).clone()
        logdet = torch.zeros(N, device="cuda")
        s = stats(timed(lambda: native.glow_coupling(rows, logdet, step.layer), args.reps))
        trunk = sum(2 * hw * hw * 144 * C + (hw // 2) ** 2 * 18 * C * C for C, hw in ((4, 32), (8, 16), (16, 8)))
        floor_us = N * trunk / (args.fma_tmacs * 1e12) * 1e6
        report(tag=args.tag, model=name, call="tfk_glow_coupling kind 4", rows=N, image=step.info["image"], T=step.layer.T,
               slots=step.info["slots"], lds_bytes=step.info["lds_bytes"], **s,
               macs_per_row=image_program.layer_cost(step.layer)["flops"] // 2, trunk_macs_per_row=trunk,
               trunk_packed_fma_floor_us=round(floor_us, 1), floor_fraction=round(floor_us / s["us_per_launch"], 3))
        for rnd in range(args.rounds):
            for path, env, reps in (("program", "1", args.reps), ("layers (IMAGE_PROGRAM=0, ResNet on ATen)", "0", args.aten_reps)):
                os.environ["TORCHFLOWS_AMD_IMAGE_PROGRAM"] = env
                try:
                    before = native.calls
                    flows[env].log_prob(x)
                    launches = native.calls - before
                    s = stats(timed(lambda: flows[env].log_prob(x), reps, warmup=3))
                    report(tag=args.tag, model=name, call="log_prob", path=path, round=rnd, rows=N, libtfk_launches=launches,
                           **s, evals_per_s=round(N / s["us_per_launch"] * 1e6))
                finally:
                    os.environ.pop("TORCHFLOWS_AMD_IMAGE_PROGRAM", None)


if __name__ == "__main__":
    main()
