"""One deep sigmoidal CONVOLUTIONAL coupling at a time: what tests/test_gpu_image_dsf_shapes.py holds
csrc/tfk_glow_dsf.hip to, and what tests/test_host_image_dsf_shapes.py proves about the cases on the host before
anything runs on a GPU.

A case is one coupling of torchflows_amd/bijections/finite/multiscale/base.py (CheckerboardCoupling, ChannelWiseCoupling,
or NormalizedCheckerboardCoupling, whose ActNorm leaves a pending (s, t) map on sources and targets) with
``DeepSigmoid(n_hidden_layers=C, hidden_dim=K)``, seeded, data-initialised by one training-mode pass and put in eval().
The last Linear layer of the ConvNet is then rescaled and recentred over the initialisation images, so that its
pre-activations have mean 0 and spread ``PRE_SPREAD`` over the samples: left alone its outputs are a few 1e-2 and the
bounded parameters of every target of every sample are nearly equal; scaled alone (x 50 on the weight) they saturate at
+-2 around an offset that does not depend on the sample (the 84 constant inputs of that layer), std 8e-3 over the samples
against 1.75 overall.  Either way a kernel that mixed up samples or targets would pass.  ``sensitivity`` measures on the
host what each such mistake costs, for every case.

The references are this package's own ATen path on the host: the module in float64 (a ``.double()`` copy) and in float32
(the floor).  The inverse is asked for ``z_in = fp32(forward64(x))``.  Measures and bars are those of
tests/dsf_reference.py (``bar``, ``normwise``, ``rel``); values are compared on the target columns."""
import copy
import functools
from types import SimpleNamespace

import numpy as np
import torch

from dsf_reference import bar, normwise, rel  # noqa: F401  (the measures, re-exported)

PRE_SPREAD = 4.0            # spread over the samples given to the pre-activations of the ConvNet's last Linear layer
N_INIT = 48                 # images of the data-dependent initialisation
N_ROWS = 37                 # two full row tiles of 16 and one of 5
KEEP_BELOW = 9.99           # inverse x is measured where |x64| is below it (tests/test_gpu_image_dsf.py)
EXCLUDED_CAP = 0.02
SENSITIVITY = 10.0          # every perturbation moves the fp64 result by at least this many bars

SHAPES = {
    # name: (class, event shape, alternate)                                       T   groups
    "checker_1x6x6_T18": ("CheckerboardCoupling", (1, 6, 6), False),            # 18: one full, one of 2 (T % 16 != 0)
    "checker_1x4x4_T8": ("CheckerboardCoupling", (1, 4, 4), False),             # 8 < 16: three of four waves idle
    "channel_4x3x3_T18": ("ChannelWiseCoupling", (4, 3, 3), False),             # 18 contiguous
    "checker_3x8x8_T96": ("CheckerboardCoupling", (3, 8, 8), False),            # 96: six groups, more than waves
    "checker_alt_3x8x8_T96": ("CheckerboardCoupling", (3, 8, 8), True),
    "channel_2x4x4_T16": ("ChannelWiseCoupling", (2, 4, 4), False),             # 16: exactly one group
    "normalized_1x6x6_T18": ("NormalizedCheckerboardCoupling", (1, 6, 6), False),
}
T_OF = {"checker_1x6x6_T18": 18, "checker_1x4x4_T8": 8, "channel_4x3x3_T18": 18, "checker_3x8x8_T96": 96,
        "checker_alt_3x8x8_T96": 96, "channel_2x4x4_T16": 16, "normalized_1x6x6_T18": 18}

SUPPORTED = [(C, K) for C in (1, 2) for K in range(1, 17)] + [(C, K) for C in (3, 4) for K in range(1, 9)]
EVERY = "checker_1x6x6_T18"                                  # group (a)
# group (b): the smallest and largest K on either side of the one-pass switch (K = 4 | 5) and of the AGPRs (10 | 11)
GEOMETRY_CK = [(1, 1), (2, 4), (2, 5), (4, 8), (2, 11), (2, 16)]
GEOMETRY_SHAPES = [s for s in SHAPES if s != EVERY]
GEOMETRY_N = [1, 16, 17, 37]
LAUNCH_SHAPES = ["checker_3x8x8_T96", "checker_1x4x4_T8"]    # group (c)
UNREACHABLE_CK = [(1, 4), (1, 5), (2, 4), (2, 5)]            # group (d), on EVERY

# The record of the sensitivity condition (tests/test_host_image_dsf_shapes.py asserts it case by case).  Every case moves
# z by at least ten bars under the sample and the target roll.  Listed here, per case, are the LOG-DET quantities that
# stay short of ten bars -- s: sample roll, t: target roll, c: components reversed -- because the log-det is measured
# relative to |log-det| ~ 3 K T; each of them still moves by at least ABOVE_THE_BAR bars.  Not listed because it holds for
# no case with C >= 2: z under reversed components (at most 0.7 bars; the conditioner's output enters as
# h / 1000, so the components commute to second order).  No case was dropped for these: that would leave ten cases, all
# of one component, and most kernels without a test.
SHORT_OF_TEN = {
    "checker_1x6x6_T18": {(1, 7): "t", (1, 10): "t", (1, 11): "t", (1, 12): "t", (1, 13): "st", (1, 14): "t", (1, 15): "st", (2, 3): "c", (2, 5): "c", (2, 7): "c", (2, 8): "c", (2, 9): "c", (2, 10): "stc", (2, 11): "tc", (2, 12): "c", (2, 13): "tc", (2, 14): "stc", (2, 15): "tc", (2, 16): "stc", (3, 7): "c"},
    "checker_1x4x4_T8": {(2, 16): "tc"},
    "channel_4x3x3_T18": {(2, 5): "c", (2, 11): "tc", (2, 16): "stc"},
    "checker_3x8x8_T96": {(2, 4): "tc", (2, 5): "tc", (4, 8): "tc", (2, 11): "stc", (2, 16): "stc"},
    "checker_alt_3x8x8_T96": {(2, 4): "stc", (2, 5): "stc", (4, 8): "stc", (2, 11): "stc", (2, 16): "stc"},
    "channel_2x4x4_T16": {(2, 11): "tc", (2, 16): "tc"},
    "normalized_1x6x6_T18": {(4, 8): "c", (2, 11): "c", (2, 16): "stc"},
}
ABOVE_THE_BAR = 1.5         # a launch with that mistake misses its log-det bar by half again, at the least
ORDER_HELD = 2.0            # reversed components move the log-det by two bars: no launch within its bar can hide it


def all_cases():
    """(shape name, C, K) of every case of groups (a), (b), (c), (e); (d) runs on cases of (a)."""
    return [(EVERY, C, K) for C, K in SUPPORTED] + [(s, C, K) for s in GEOMETRY_SHAPES for C, K in GEOMETRY_CK]


def _seed(name, C, K):
    return 9000 + 1000 * list(SHAPES).index(name) + 20 * C + K


def coupling_of(module):
    from torchflows_amd.bijections.finite.autoregressive.layers_base import CouplingBijection
    return module if isinstance(module, CouplingBijection) else module.layers[-1]


@functools.lru_cache(maxsize=None)
def make_case(name, C, K):
    """The module (float32, eval, on the host), its float64 copy and N_ROWS standard-normal images."""
    from torchflows_amd.bijections.finite.autoregressive.transformers.combination.sigmoid import DeepSigmoid
    from torchflows_amd.bijections.finite.multiscale import base as ms
    cls, shape, alternate = SHAPES[name]
    torch.manual_seed(_seed(name, C, K))
    kwargs = dict(transformer_class=DeepSigmoid, transformer_kwargs=dict(n_hidden_layers=C, hidden_dim=K))
    if cls != "NormalizedCheckerboardCoupling":
        kwargs["alternate"] = alternate
    module = getattr(ms, cls)(shape, **kwargs)
    init = torch.randn(N_INIT, *shape)
    module.train()
    with torch.no_grad():
        module.forward(init)                                         # ActNorm init, BatchNorm statistics
    module.eval()
    last = [m for m in coupling_of(module).conditioner_transform.modules() if isinstance(m, torch.nn.Linear)][-1]
    seen = []
    hook = last.register_forward_hook(lambda mod, inp, out: seen.append(inp[0].detach().double()))
    with torch.no_grad():
        module.forward(init)
        hook.remove()
        u = seen[0].reshape(N_INIT, -1)
        W = last.weight.double()
        spread = ((u - u.mean(0)) @ W.T).std(0).mean()               # of the pre-activations over the samples
        W = W * (PRE_SPREAD / spread)
        last.weight.copy_(W.float())
        last.bias.copy_((-(W @ u.mean(0))).float())
    x = torch.randn(N_ROWS, *shape)
    cp = coupling_of(module)
    T = int(cp.coupling.target_event_size)
    assert T == T_OF[name] and cp.transformer.n_components == C and cp.transformer.hidden_dim == K
    return SimpleNamespace(name=name, C=C, K=K, T=T, D=int(np.prod(shape)), shape=shape, module=module,
                           module64=copy.deepcopy(module).double(), x=x,
                           cols=cp._target_index.numpy().copy())


def _both(case, call):
    out = {}
    with torch.no_grad():
        for tag, m, dtype in (("64", case.module64, torch.float64), ("32", case.module, torch.float32)):
            v, ld = call(m, dtype)
            out["v" + tag], out["ld" + tag] = v.reshape(v.shape[0], -1).numpy(), ld.numpy()
    return out


@functools.lru_cache(maxsize=None)
def reference(name, C, K):
    """float64 and float32 forward of x, and both inverses of z_in = fp32(z64), all rows (N_ROWS, D); read only."""
    case = make_case(name, C, K)
    f = _both(case, lambda m, dt: m.forward(case.x.to(dt)))
    z_in = torch.from_numpy(f["v64"]).float().view(N_ROWS, *case.shape)
    i = _both(case, lambda m, dt: m.inverse(z_in.to(dt)))
    ref = SimpleNamespace(z64=f["v64"], ld64=f["ld64"], z32=f["v32"], ld32=f["ld32"], z_in=z_in.reshape(N_ROWS, -1).numpy(),
                          x64=i["v64"], ldi64=i["ld64"], x32=i["v32"], ldi32=i["ld32"])
    for a in vars(ref).values():
        a.setflags(write=False)
    return ref


def keep_mask(case, ref, n):
    """Target elements of the first n rows on which the inverse's x is measured."""
    return np.abs(ref.x64[:n][:, case.cols]) < KEEP_BELOW


def excluded_share(name, C, K):
    case, ref = make_case(name, C, K), reference(name, C, K)
    return 1.0 - float(keep_mask(case, ref, N_ROWS).mean())


def conditioner_output(case, rows, dtype):
    """h (N, T, 3 K C) of the coupling for rows (N, D) that hold the coupling's own input at the source columns."""
    m = case.module64 if dtype == torch.float64 else case.module
    with torch.no_grad():
        v = torch.as_tensor(rows).to(dtype).view(-1, *case.shape)
        return coupling_of(m).partition_and_predict_parameters(v, None)


def coupling_input64(case):
    """What the coupling itself sees of x in the forward direction (behind the ActNorm, if there is one)."""
    v = case.x.double()
    with torch.no_grad():
        if coupling_of(case.module64) is not case.module64:
            for layer in list(case.module64.layers)[:-1]:
                v, _ = layer.forward(v)
    return v


def sensitivity(name, C, K):
    """How far three mistakes a kernel could make move the float64 forward result of the coupling, as (z norm-wise,
    log-det relative) each: the conditioner's output of the neighbouring sample, of the neighbouring target, and (C >= 2)
    the components in reverse order."""
    case = make_case(name, C, K)
    cp = coupling_of(case.module64)
    v = coupling_input64(case)
    with torch.no_grad():
        h = cp.partition_and_predict_parameters(v, None)
        xt = cp.get_transformed_part(v)
        z0, ld0 = cp.transformer.forward(xt, h)
        P = 3 * K
        flat = h.reshape(h.shape[0], -1, C * P)                    # (N, T, 3 K C), targets in the transformer's order
        moved = {"sample": h.roll(1, 0), "target": flat.roll(1, 1).view_as(h)}
        if C >= 2:
            moved["components"] = torch.cat([h[..., c * P:(c + 1) * P] for c in reversed(range(C))], dim=-1)
        out = {}
        for what, hp in moved.items():
            z, ld = cp.transformer.forward(xt, hp)
            out[what] = (normwise(z.numpy(), z0.numpy()), rel(ld.numpy(), ld0.numpy()))
    return out


def held_to(name, C, K):
    """The bars of the forward launch on all N_ROWS rows: (z, log-det)."""
    case, ref = make_case(name, C, K), reference(name, C, K)
    return (bar(normwise(ref.z32[:, case.cols], ref.z64[:, case.cols])), bar(rel(ref.ld32, ref.ld64)))


QUANTITIES = ("sample_z", "sample_ld", "target_z", "target_ld", "components_z", "components_ld")


def moved_in_bars(name, C, K):
    """``sensitivity`` in units of the bar the forward launch is held to, by quantity name (QUANTITIES)."""
    bars = dict(zip(("z", "ld"), held_to(name, C, K)))
    return {f"{what}_{q}": v / bars[q] for what, pair in sensitivity(name, C, K).items() for q, v in zip(("z", "ld"), pair)}


def compile_step(case, d, device):
    """The compiled program of the case in direction d; its single step is the launch under test."""
    from torchflows_amd import image_program
    prog = image_program.compile_program(case.module, d, device)
    assert prog is not None and len(prog.steps) == 1
    return prog, prog.steps[0]
