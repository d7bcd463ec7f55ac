"""Fixtures of the deep sigmoidal image presets, by RUNNING the real reference (run as make_golden_dsf.py is).
``DeepSigmoidGlow((3, 8, 8))`` holds 2.9 M parameters (11 MiB, stored twice by ``flow_fixture``), far above what a
committed file may weigh, so the flow fixture is the (1, 4, 4), one-block model; of the (3, 8, 8) and (1, 28, 28)
models only the state dicts' key lists and shapes are recorded.  Data only; no reference source is stored."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import Flow, flow_fixture, save  # noqa: E402
from torchflows.bijections.finite.multiscale.architectures import DeepSigmoidGlow, MultiscaleDeepSigmoid  # noqa: E402


def traced(event_shape, **kwargs):
    bij = DeepSigmoidGlow(event_shape, **kwargs)
    bij.layers = [bij]                      # (a plain list: what flow_fixture's per-layer trace iterates)
    return bij


if __name__ == "__main__":
    flow_fixture("flow_dsglow_1x4x4.npz", traced, (1, 4, 4), 16, dict(n_layers=1))
    out = {}
    for tag, ctor, shape in (("dsglow_3x8x8", DeepSigmoidGlow, (3, 8, 8)), ("msdsf_1x28x28", MultiscaleDeepSigmoid, (1, 28, 28))):
        sd = Flow(ctor(shape)).state_dict()
        out[tag + "/keys"] = np.array(list(sd))
        out[tag + "/shapes"] = np.array([tuple(v.shape) + (-1,) * (4 - v.dim()) for v in sd.values()], dtype=np.int64)
    save("image_dsf_keys.npz", **out)
