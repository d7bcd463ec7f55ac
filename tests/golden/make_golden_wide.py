"""Generate the fixtures of the wide-row route (event sizes above 256) by RUNNING the real reference, in the key
layout of the other flow fixtures (``make_golden.flow_fixture``: both variants, fp64 re-evaluations).

Run where the reference is importable (it cannot travel to the GPU box), from the repository root:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python tests/golden/make_golden_wide.py

Every array written is data (inputs, parameters, outputs of the reference); no reference source is stored.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_golden import NICE, RealNVP, flow_fixture  # noqa: E402  (imports the reference; defines functions only)


def gen_wide():
    # the first model of the reference's image notebook: D = 784, hidden width 14, planes of 392 padded to 448
    # (8 rows: with 16 the file is 1.2 MB -- the two variants' weights alone are 0.4 MB -- above the largest vector-flow fixture)
    flow_fixture("flow_realnvp_1x28x28.npz", RealNVP, (1, 28, 28), 8, dict(n_layers=3), trace_rows=2)
    # the smallest size the route takes: D % 4 == 2 (rows 8-byte aligned), halves of 129 in planes of 192
    flow_fixture("flow_nice258.npz", NICE, 258, 16, dict(n_layers=2))


if __name__ == "__main__":
    gen_wide()
