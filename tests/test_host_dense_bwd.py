"""Host side of the dense sigmoidal family's reverse mode: the probe, the ``dense_train`` switch and the size of the one
block ``tfk_dsf_coupling_bwd`` takes for the family (include/tfk.h).  No GPU needed."""
import pytest
import torch

from conftest import set_debug


@pytest.fixture(scope="module")
def native():
    from torchflows_amd import native as nat
    if not nat.available():
        pytest.skip("libtfk is not built")
    return nat


def dense_layer(bijection):
    return next(l for l in bijection.layers if getattr(getattr(l, "transformer", None), "native_kind", "") == "dense")


def test_probe_answers_without_a_device(native):
    L = native.lib()
    args = (None, None, None, None, None, 0, 1, None, 1)
    assert L.tfk_dsf_coupling_bwd(*args, native.dense_code(1, 0), 1, 0, None) == 0 and native.dense_bwd_supported()
    assert L.tfk_dsf_coupling_bwd(*args, native.dense_code(1, 0), 1, 1, None) != 0          # the inverse direction
    assert L.tfk_dsf_coupling_bwd(*args, native.dense_code(2, 2), 8, 0, None) != 0          # C P = 774 > 512


def test_reverse_mode_follows_dense_train(native, monkeypatch):
    import torchflows_amd as tfa
    from torchflows_amd import autograd
    kind = native.KINDS["dense"]
    bijection = tfa.CouplingDenseSF(6, n_layers=2)
    tr = dense_layer(bijection).transformer
    assert tr.native_kind == "dense" and kind.reverse == "dense_coupling_bwd"
    assert kind.reverse_mode(tr) and autograd.training_plan(bijection, autograd.FORWARD) is not None
    assert autograd.training_plan(bijection, autograd.INVERSE) is None                       # (the bisection)
    set_debug(monkeypatch, dense_train="0")
    assert not kind.reverse_mode(tr) and kind.coupling(tr) and autograd.training_plan(bijection, autograd.FORWARD) is None
    set_debug(monkeypatch, dense_train="1", dense="0")
    assert not kind.reverse_mode(tr) and not kind.coupling(tr)


@pytest.mark.parametrize("arch,N,T,stride", [("CouplingDenseSF", 5, 3, 146), ("MaskedAutoregressiveDenseSF", 5, 6, 1458)])
def test_gh_is_sized_as_the_header_says(native, arch, N, T, stride):
    import torchflows_amd as tfa
    torch.manual_seed(0)
    ct = dense_layer(getattr(tfa, arch)(6, n_layers=2)).conditioner_transform                    # (a MADE hands over its whole output: stride D P)
    assert (T * 243, stride) == (ct.n_transformer_parameters, T * 243 if "Masked" in arch else ct.n_predicted_parameters)
    want = T * 243 * (1 + 256) + N * stride             # [dL/dbase | 256 slices | dL/dpred]
    assert sum(native.dense_bwd_floats(N, T, 243, stride)) == want
    x, desc = torch.zeros(N, 6), torch.zeros(T + 1 + 2 * T * 243, dtype=torch.int32)
    with pytest.raises(native.NativeError, match=f"= {want}$"):
        native.dense_coupling_bwd(x, torch.zeros(N, stride), x.clone(), torch.zeros(N), torch.zeros(want - 1), desc, T, 1, 1, 8)
