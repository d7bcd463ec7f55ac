"""Generate the gradient fixture of the wide training route by RUNNING the real reference's autograd (fp32 and fp64) on the
weights and inputs of the committed ``flow_realnvp_1x28x28.npz``, in the key layout of the other ``grads_flow_*`` fixtures
(``make_golden._flow_grads``: w, gx, gx64, g/<name>, g64/<name>, trainable).

Run where the reference is importable (it cannot travel to the GPU box), from the repository root:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python tests/golden/make_golden_wide_train.py

Three couplings of 16.5 k weights each, fp32 + fp64 gradients (both stored as fp32, like every fixture): 0.7 MB, below
the limit for a committed file -- every tensor is kept.  Every array written is data (gradients the reference computed);
no reference source is stored.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_golden import RealNVP, _flow_grads  # noqa: E402  (imports the reference; defines functions only)


def gen_wide_train():
    # the first model of the reference's image notebook: D = 784, hidden width 14 (make_golden_wide.gen_wide's constructor)
    _flow_grads("flow_realnvp_1x28x28.npz", RealNVP, (1, 28, 28), dict(n_layers=3))


if __name__ == "__main__":
    gen_wide_train()
