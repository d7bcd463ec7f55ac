#!/usr/bin/env python
"""Fingerprint of the flow programs the host-side compiler emits, for refactors that must not change a byte of them.

It only calls ``torchflows_amd.fused.compile_chain`` (device ``cpu``: the packers run on the host), so the same file runs
on any two commits; ``diff`` of the two outputs is the check.

    python tools/program_fingerprint.py --out default.json            # the grid under the CURRENT environment
    python tools/program_fingerprint.py --all-settings OUT_DIR        # the grid once per debug setting (a process each,
                                                                      # --jobs of them at a time)
    python tools/program_fingerprint.py --routes tests/golden/program_routes.json

Per case: ``D``, ``D_log``, ``identity_out``, ``pos``, ``pos_in`` and per segment ``mfma``, ``wide``, ``numel``, the op
tuples and the sha256 of the parameter bytes; ``null`` where the compiler declines, ``{"raises": ...}`` where the preset
does not exist at that size.  The sha compares runs on ONE machine: fp64 BLAS may round differently on another CPU, and
with another number of threads, which is why every run of this tool computes with ``THREADS`` threads whatever the
environment says.  So ``--routes`` -- the committed fixture of tests/test_host_program_routes.py -- leaves it out and
keeps one case per (preset family, row-width class, context) plus the chains that cross a budget or format boundary.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PRESETS = ("RealNVP", "NICE", "CouplingRQNSF", "CouplingLRS", "MAF", "IAF", "MaskedAutoregressiveRQNSF",
           "InverseAutoregressiveRQNSF", "MaskedAutoregressiveLRS")
SIZES = (3, 8, 15, 16, 22, 32, 63, 64, 99, 128, 201, 256, 258, 512)
CONTEXT = 5
THREADS = 4               # torch threads of every grid, fixed: the rounding of the fp64 products depends on it
# chains that cross a budget or a format boundary: (preset, D, n_layers, hidden width or None)
BOUNDARY = (("RealNVP", 64, 8, None), ("RealNVP", 64, 14, None), ("RealNVP", 128, 8, None), ("RealNVP", 256, 8, None),
            ("RealNVP", 256, 3, None), ("CouplingRQNSF", 64, 8, None), ("RealNVP", 64, 2, 11), ("CouplingRQNSF", 64, 2, 24))
SETTINGS = (("default", {}), ("lean0", {"TORCHFLOWS_AMD_DEBUG": "lean=0"}),
            ("lean_f16x2_0", {"TORCHFLOWS_AMD_DEBUG": "lean_f16x2=0"}), ("lean_bf16x3_1", {"TORCHFLOWS_AMD_DEBUG": "lean_bf16x3=1"}),
            ("bf16x3_0", {"TORCHFLOWS_AMD_DEBUG": "lean_bf16x3=0,rqs_bf16x3=0"}),
            ("stream_chain0", {"TORCHFLOWS_AMD_DEBUG": "stream_chain=0"}), ("rows16_0", {"TORCHFLOWS_AMD_DEBUG": "rows16=0"}),
            ("odd_lean0", {"TORCHFLOWS_AMD_DEBUG": "odd_lean=0"}), ("fused_pad0", {"TORCHFLOWS_AMD_DEBUG": "fused_pad=0"}),
            ("mfma0", {"TORCHFLOWS_AMD_MFMA": "0"}))


def grid():
    """[(preset, D, context elements or 0, n_layers, hidden width or None)]; both directions of each are compiled."""
    cases = [(p, D, C, 3, None) for p in PRESETS for D in SIZES for C in (0, CONTEXT)]
    return cases + [(p, D, 0, n, h) for p, D, n, h in BOUNDARY]


def case_id(case, direction):
    p, D, C, n, h = case
    return f"{p}-D{D}-ctx{C}-n{n}" + (f"-h{h}" if h else "") + f"-dir{direction}"


def build_flow(case):
    """The preset in eval mode, its ActNorm layers initialised by one train-mode ``log_prob`` on 128 rows."""
    import torch
    import torchflows_amd as tfa
    p, D, C, n, h = case
    torch.manual_seed(1000 + D)
    kw = dict(n_layers=n)
    if C:
        kw["context_shape"] = (C,)
    if h:
        kw["conditioner_kwargs"] = dict(n_hidden=h)
    flow = tfa.Flow(getattr(tfa, p)(D, **kw))
    flow.train()
    with torch.no_grad():
        flow.log_prob(torch.randn(128, D), **(dict(context=torch.randn(128, C)) if C else {}))
    return flow.eval()


def describe(chain, sha: bool):
    """The chain as plain JSON data (float fields of the ops as float32 reprs), None for a declined composition."""
    import numpy as np
    if chain is None:
        return None
    field = lambda v: repr(np.float32(v).item()) if isinstance(v, float) else int(v)
    segs = []
    for seg in chain.segments:
        s = dict(mfma=bool(seg.mfma), wide=bool(seg.wide), numel=int(seg.params.numel()),
                 ops=[[field(v) for v in op] for op in seg.ops])
        if sha:
            s["sha256"] = hashlib.sha256(seg.params.detach().contiguous().numpy().tobytes()).hexdigest()
        segs.append(s)
    return dict(D=int(chain.D), D_log=int(chain.D_log), identity_out=bool(chain.identity_out), pos=chain.pos.tolist(),
                pos_in=None if chain.pos_in is None else chain.pos_in.tolist(), segments=segs)


def fingerprint(case, sha: bool = True):
    """{case id: description} for both directions of one case."""
    import torch
    from torchflows_amd import fused
    try:
        flow = build_flow(case)
    except Exception as e:                                   # (the preset does not exist at this size)
        return {case_id(case, d): {"raises": type(e).__name__} for d in (0, 1)}
    out = {}
    for d in (0, 1):
        try:
            out[case_id(case, d)] = describe(
                fused.compile_chain(flow.bijection, d, torch.device("cpu"), context=bool(case[2])), sha)
        except Exception as e:
            out[case_id(case, d)] = {"raises": type(e).__name__}
    return out


def width_class(desc):
    if desc is None:
        return "declined"
    if "raises" in desc:
        return "raises"
    return "wide" if desc["segments"] and desc["segments"][0]["wide"] else str(desc["D"])


def routes():
    """The committed fixture: the first case of the grid for every (preset, width class, context), and the boundary chains."""
    seen, cases = set(), []
    for case in grid():
        got = fingerprint(case, sha=False)
        for d in (0, 1):
            desc = got[case_id(case, d)]
            key = (case[0], width_class(desc), bool(case[2]))
            boundary = case[3] != 3 or case[4] is not None
            if boundary or (key not in seen and key[1] != "raises"):
                seen.add(key)
                cases.append(dict(id=case_id(case, d), preset=case[0], D=case[1], context=case[2], n_layers=case[3],
                                  n_hidden=case[4], direction=d, expect=desc))
    return cases


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="write the grid's fingerprint under the current environment to this JSON file")
    ap.add_argument("--all-settings", metavar="DIR", help="one JSON file per debug setting, each from a process of its own")
    ap.add_argument("--routes", metavar="FILE", help="write the machine-independent route fixture")
    ap.add_argument("--jobs", type=int, default=2, help="--all-settings: processes at a time (each computes with "
                                                        f"{THREADS} threads)")
    args = ap.parse_args()
    t0 = time.time()
    if not args.all_settings:
        import torch
        torch.set_num_threads(THREADS)
    if args.all_settings:
        os.makedirs(args.all_settings, exist_ok=True)
        bad = []
        for i in range(0, len(SETTINGS), max(1, args.jobs)):
            procs = []
            for name, env in SETTINGS[i:i + max(1, args.jobs)]:
                e = {k: v for k, v in os.environ.items() if k not in ("TORCHFLOWS_AMD_DEBUG", "TORCHFLOWS_AMD_MFMA")}
                e.update(env, OMP_NUM_THREADS=str(THREADS))
                procs.append((name, subprocess.Popen([sys.executable, os.path.abspath(__file__), "--out",
                                                      os.path.join(args.all_settings, name + ".json")], env=e)))
            bad += [name for name, p in procs if p.wait() != 0]
        print(f"{len(SETTINGS)} settings in {time.time() - t0:.1f} s" + (f"; FAILED: {bad}" if bad else ""))
        sys.exit(1 if bad else 0)
    if args.routes:
        cases = routes()
        with open(args.routes, "w") as f:
            json.dump(dict(cases=cases), f, separators=(",", ":"))
            f.write("\n")
        print(f"{len(cases)} route cases in {time.time() - t0:.1f} s -> {args.routes}")
        return
    result = {}
    for case in grid():
        result.update(fingerprint(case))
    text = json.dumps(result, indent=0, sort_keys=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
    n_ok = sum(1 for v in result.values() if v is not None and "raises" not in v)
    print(f"{len(result)} entries, {n_ok} compiled, {time.time() - t0:.1f} s", file=sys.stderr)


if __name__ == "__main__":
    main()
