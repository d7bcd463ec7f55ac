"""Record ``train_launch_trace.json``: per case of tests/test_train_launch_trace_cpu.py the sequence of libtfk launches of
one training step (forward + backward of ``autograd.run``) with stubbed entry points -- names, operand shapes, flags, op
tuples, parameter-block sizes.  This project's own recorded results; no GPU and no reference needed.  From the repository
root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_train_launch_trace.py

The fixture pins the launch sequence across changes of the host code: it is regenerated only when a change is MEANT to
alter what a step launches, never to make a refactor pass.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # the repository root

import test_train_launch_trace_cpu as T  # noqa: E402


def gen_train_launch_trace():
    from torchflows_amd import native
    real = {name: getattr(native, name) for name in T.ENTRY_POINTS}
    out = {}
    for name in sorted(T.CASES):
        try:
            out[name] = T.record(name, setattr, os.environ.__setitem__)
        finally:
            for k, v in real.items():
                setattr(native, k, v)
            os.environ.pop("TORCHFLOWS_AMD_DEBUG", None)
    with open(T.FIXTURE, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(T.FIXTURE, os.path.getsize(T.FIXTURE), "bytes;", {k: len(v) - 1 for k, v in out.items()})


if __name__ == "__main__":
    gen_train_launch_trace()
