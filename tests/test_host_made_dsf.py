"""Host side of the one-launch sequential map of the MADE-based deep sigmoidal layers (csrc/tfk_made_dsf.hip): the
device-free probe behind ``tfk_made_rqs_sequential_lds_bytes`` and what ``_made_pack`` hands the kernel.  No GPU needed."""
import pytest
import torch

from conftest import set_debug


def _layer(name="DeepSigmoidalForwardMaskedAutoregressive", **kw):
    from torchflows_amd.bijections.finite.autoregressive import layers
    torch.manual_seed(0)
    return getattr(layers, name)((6,), **kw).eval()


def test_probe_accepts_what_tfk_dsf_supported_accepts():
    from torchflows_amd import native
    probe = native.lib().tfk_made_rqs_sequential_lds_bytes
    for C in range(0, 6):
        for K in range(0, 19):
            assert (probe(8, 8, native.made_dsf_code(C, K)) <= 160 * 1024) == native.dsf_supported(C, K), (C, K)
    assert probe(8, 32, native.made_dsf_code(2, 4)) > 160 * 1024               # hidden_padded: 8 or 16
    assert probe(1024, 16, native.made_dsf_code(2, 16)) > 160 * 1024           # b2 alone: 393 KB


@pytest.mark.parametrize("D,HP,C,K,G,want", [(64, 8, 2, 5, 8, 13760), (7, 8, 2, 5, 8, 3280), (131, 16, 2, 10, 16, 49680)])
def test_probe_counts_the_documented_layout(D, HP, C, K, G, want):
    """include/tfk.h: 4 (align4(D hp + hp + D P + (64 / G) (D + 1)) + 2 P hp) bytes."""
    from torchflows_amd import native
    P = 3 * K * C
    assert 4 * ((D * HP + HP + D * P + (64 // G) * (D + 1) + 3) // 4 * 4 + 2 * P * HP) == want
    assert native.lib().tfk_made_rqs_sequential_lds_bytes(D, HP, native.made_dsf_code(C, K)) == want


def test_made_pack_of_a_default_layer():
    layer = _layer()
    W1t, b1, W2, b2 = layer._made_pack()
    assert (tuple(W1t.shape), tuple(b1.shape), tuple(W2.shape), tuple(b2.shape)) == ((6, 8), (8,), (6, 24, 8), (6, 24))
    first, last = layer.conditioner_transform.sequential[0], layer.conditioner_transform.sequential[2]
    H = first.out_features
    assert torch.equal(W1t[:, :H], (first.weight * first.mask).t()) and torch.equal(b1[:H], first.bias)
    assert torch.equal(W2[:, :, :H].reshape(6 * 24, H), last.weight * last.mask) and torch.equal(b2.reshape(-1), last.bias)
    assert float(W1t[:, H:].abs().sum()) == 0.0 and float(W2[:, :, H:].abs().sum()) == 0.0


def test_made_pack_declines(monkeypatch):
    assert _layer(context_shape=(3,))._made_pack() is None
    assert _layer("DenseSigmoidalForwardMaskedAutoregressive")._made_pack() is None
    layer = _layer("DeepSigmoidalInverseMaskedAutoregressive")
    monkeypatch.setenv("TORCHFLOWS_AMD_FUSED", "0")
    assert layer._made_pack() is None
    monkeypatch.delenv("TORCHFLOWS_AMD_FUSED")
    set_debug(monkeypatch, made_fused=0)
    assert layer._made_pack() is None
    set_debug(monkeypatch, made_fused=None)
    assert layer._made_pack() is not None
