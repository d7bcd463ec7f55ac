"""The deep sigmoidal image presets on the host: imports under both spellings, and the image-program compiler taking
their couplings (kind "dsf", one launch each) while still declining what has no fused kernel.  No GPU needed."""
import numpy as np
import pytest
import torch

from conftest import load_golden, state_dict_of
from test_host_dsf import bar, normwise, rel


def test_presets_import_by_both_spellings():
    import torchflows
    import torchflows.architectures as A1
    import torchflows.bijections.finite.multiscale as M1
    import torchflows.bijections.finite.multiscale.architectures as MA1
    import torchflows_amd as tfa
    import torchflows_amd.bijections.finite.multiscale.architectures as MA2
    for name in ("MultiscaleDeepSigmoid", "DeepSigmoidGlow"):
        cls = getattr(MA2, name)
        assert all(getattr(m, name) is cls for m in (torchflows, tfa, A1, M1, MA1)), name
    for missing in ("MultiscaleDenseSigmoid", "DenseSigmoidGlow", "MultiscaleDeepDenseSigmoid", "DeepDenseSigmoidGlow"):
        assert not hasattr(MA2, missing)


@pytest.mark.parametrize("d", [0, 1])
def test_program_compiles_for_deep_sigmoid_glow(d, monkeypatch):
    import torchflows_amd as tfa
    from torchflows_amd import image_program, native
    if not native.available():
        pytest.skip("libtfk.so not built")
    torch.manual_seed(0)
    flow = tfa.Flow(tfa.DeepSigmoidGlow((3, 8, 8)))
    flow.train()
    with torch.no_grad():
        flow.log_prob(torch.randn(32, 3, 8, 8))                  # ActNorm init, BatchNorm statistics
    flow.eval()
    cpu = torch.device("cpu")
    prog = image_program.compile_program(flow.bijection, d, cpu)
    assert prog is not None and len(prog.steps) == 19
    kinds = [s.info["kind"] for s in prog.steps]
    assert kinds.count("dsf") == 16 and kinds.count("conv1x1") == 3
    for s in prog.steps:
        if s.info["kind"] == "dsf":
            L = s.layer
            assert (L.kind, L.n_ch, L.hw) == (3, 2, 5) and L.n_params == L.T * 30 and s.inverse == bool(d)
            assert s.keep[7].numel() == (L.T + 15) // 16 * 30 * 256 and s.info["block"] <= 256
    # the level route has no deep sigmoidal stage: the program keeps one launch per coupling
    monkeypatch.setenv("TORCHFLOWS_AMD_GLOW_LEVELS", "1")
    assert image_program.compile_program(flow.bijection, d, cpu).levels is None
    # the comparison switch of the family turns the new kind off as well
    monkeypatch.setenv("TORCHFLOWS_AMD_DEBUG", "dsf=0")
    assert image_program.compile_program(flow.bijection, d, cpu) is None


def test_program_still_declines_splines():
    from torchflows_amd import image_program
    from torchflows_amd.bijections.finite.autoregressive.transformers.spline.rational_quadratic import RationalQuadratic
    from torchflows_amd.bijections.finite.multiscale.base import MultiscaleBijection
    spline = MultiscaleBijection((3, 16, 16), transformer_class=RationalQuadratic, n_blocks=2).eval()
    assert image_program.compile_program(spline, 0, torch.device("cpu")) is None


@pytest.mark.parametrize("tag,arch,shape", [("dsglow_3x8x8", "DeepSigmoidGlow", (3, 8, 8)),
                                            ("msdsf_1x28x28", "MultiscaleDeepSigmoid", (1, 28, 28))])
def test_state_dict_keys_equal_the_reference(tag, arch, shape):
    import torchflows_amd as tfa
    fx = load_golden("image_dsf_keys.npz")
    sd = tfa.Flow(getattr(tfa, arch)(shape)).state_dict()
    assert list(sd) == [str(k) for k in fx[tag + "/keys"]]
    assert [tuple(v.shape) for v in sd.values()] == [tuple(int(d) for d in row if d >= 0) for row in fx[tag + "/shapes"]]


@pytest.mark.parametrize("variant", ["fresh", "init"])
def test_aten_path_reproduces_reference_fixture(variant):
    """flow_dsglow_1x4x4.npz: the reference's DeepSigmoidGlow((1, 4, 4), n_layers=1) -- the (3, 8, 8) model's state dicts
    alone are 22 MiB -- loaded strictly; this package's ATen path against its outputs at test_host_dsf's bar."""
    import torchflows_amd as tfa
    fx = load_golden("flow_dsglow_1x4x4.npz")
    flow = tfa.Flow(tfa.DeepSigmoidGlow((1, 4, 4), n_layers=1))
    sd = {k: torch.from_numpy(v) for k, v in state_dict_of(fx, variant).items()}
    assert list(flow.state_dict()) == list(sd)
    flow.load_state_dict(sd, strict=True)
    flow.eval()
    g = lambda k: fx[f"{variant}/{k}"]
    with torch.no_grad():
        z, ld = flow.bijection.forward(torch.from_numpy(fx["x"]))
        lp = flow.log_prob(torch.from_numpy(fx["x"]))
        xi, ldi = flow.bijection.inverse(torch.from_numpy(fx["z_in"]))
    # The fixture's inverse inputs are standard-normal draws (flow_fixture), not forward images: where the reference's own
    # float64 inverse ends at the bracket's edge the map is flat and x is not determined.  The mask comes from the
    # reference's output alone; its share is 3.5 % (fresh) and 0 (init), held under 5 %.
    keep = np.abs(g("x_inv64")) < 9.99
    assert keep.mean() >= 0.95
    for got, key, dist in ((z, "z", normwise), (ld, "log_det", rel), (lp, "log_prob", rel), (ldi, "log_det_inv", rel)):
        assert dist(got.numpy(), g(key)) < bar(dist(g(key), g(key + "64"))), key
    assert normwise(xi.numpy()[keep], g("x_inv")[keep]) < bar(normwise(g("x_inv")[keep], g("x_inv64")[keep]))
