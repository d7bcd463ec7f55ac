#!/usr/bin/env python
"""Per-call Python time of libtfk's wrappers with the launching entry points stubbed: no GPU work is in the number.

    python tools/abi_host_cost.py [TREE]        # TREE: a checkout whose torchflows_amd is timed (default: this one)

Times ``native.affine_coupling``, ``native.flow_run_mfma`` (plain route), ``native.rows_fma`` and one transformer-kind
route (``autograd._transform_forward`` on an RQ spline): 20 000 calls each, 5 repeats, median / min / max in microseconds
as one JSON line.  Compare two commits in ONE session, each in its own process; the other checkout loads this one's
library through TORCHFLOWS_AMD_LIB.  The stand-in is the recorder of tests/test_gpu_abi_calls.py in its quiet mode; the
tensors live on the HIP device (the wrappers reject host tensors) and are never touched."""
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else ROOT
sys.path[:0] = [TREE, os.path.join(ROOT, "tests")]

import test_gpu_abi_calls as t                                  # noqa: E402
from torchflows_amd import autograd as ag, native               # noqa: E402

assert os.path.abspath(native.__file__).startswith(TREE), native.__file__
native._lib = t.Recorder(native.lib(), quiet=True)
N = 3
x, h, z, ld, st = t.f(N, 4), t.f(N, 2, 2), t.f(N, 4), t.f(N), t.f(4, 2)
x64, z64, loc, log_scale, params = t.f(N, 64), t.f(N, 64), t.f(64), t.f(64), t.f(1024)
ops = [(12, 0, 2, 0), (16, 0, 0, 512)]
spline, h_spline = types.SimpleNamespace(transformer=t._transformer("rqs")), t.f(N, 2, 23)
WORK = {
    "affine_coupling": lambda: native.affine_coupling(x, h, z, ld, None, 2),
    "flow_run_mfma": lambda: native.flow_run_mfma(x64, z64, ld, loc, log_scale, None, ops, params),
    "rows_fma": lambda: native.rows_fma(x, st),
    "transform_forward_rqs": lambda: ag._transform_forward(spline, ag.FORWARD, x, h_spline, z, ld, None, 2, False),
}
out = {"tree": TREE}
for name, fn in WORK.items():
    for _ in range(2000):
        fn()
    reps = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(20000):
            fn()
        reps.append((time.perf_counter() - t0) / 20000 * 1e6)
    out[name] = {"median_us": round(statistics.median(reps), 4), "min_us": round(min(reps), 4), "max_us": round(max(reps), 4)}
print("HOSTCOST " + json.dumps(out))
