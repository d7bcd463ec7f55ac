"""Host side of the fused CouplingLRS(64) training route (no GPU): the flagged entry point, ``_LrsTrainPack`` and the
``_LRS`` route of torchflows_amd/autograd.py."""
import math

import numpy as np
import pytest
import torch

from conftest import set_debug

FLAG = 1 << 16


def test_flagged_n_bins_selects_the_lrs_kernel():
    from torchflows_amd import native
    supported = native.lib().tfk_rqs_coupling_train_bwd_supported
    assert supported(64, FLAG | 8) == 1 and supported(64, 8) == 1
    assert [supported(64, FLAG | 4), supported(128, FLAG | 8), supported(64, (1 << 17) | 8)] == [0, 0, 0]
    assert native.LRS_TRAIN_FLAG == FLAG and native.lib().tfk_abi_version() == 29


@pytest.mark.parametrize("H", [1, 5, 15])
def test_forward_block_is_the_inference_packers(H):
    from torchflows_amd import flow_pack
    from torchflows_amd.train_packs import _LrsTrainPack
    torch.manual_seed(H)
    lin1, lin2 = torch.nn.Linear(32, H), torch.nn.Linear(H, 1024)
    pk = _LrsTrainPack(H, "cpu")
    got = pk.forward_blocks(torch.cat(pk.flat_of(lin1, lin2))[None])[0]
    f64 = lambda t: t.detach().double()
    want = flow_pack._pack_lean_rqs(H, 64, f64(lin1.weight), f64(lin1.bias), f64(lin2.weight).view(32, 32, H),
                                    f64(lin2.bias).view(32, 32), torch.ones(32, dtype=torch.float64),
                                    torch.zeros(32, dtype=torch.float64),
                                    float(np.float32(math.log(math.exp(1 - 1e-5) - 1))), bf16x3=True, lrs=True)
    assert got.numel() == pk.N_FWD and torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_backward_gather_follows_the_operand_layout():
    """A1[8][64] | b1[16] | A2[64][steps2][64] | b2[64][16] | A2T[64][4][64] | A1T[2][4][64]; lane = 16 q + i."""
    from torchflows_amd.train_packs import _LrsTrainPack
    H = 15
    torch.manual_seed(1)
    lin1, lin2 = torch.nn.Linear(32, H), torch.nn.Linear(H, 1024)
    pk = _LrsTrainPack(H, "cpu")
    block = pk.pack(lin1, lin2)
    assert block.numel() == 34832 and pk.steps2 == 4
    W1, W2 = lin1.weight.detach(), lin2.weight.detach().view(32, 32, H)
    off_A2 = 8 * 64 + 16
    off_A2T = off_A2 + 64 * 4 * 64 + 64 * 16
    off_A1T = off_A2T + 64 * 4 * 64
    # A2, tile 8 e + c = 8 * 3 + 5, k-step 2, lane (q = 1, i = 4 * 2 + 3): parameter 4 * 5 + 3 of target 8 * 2 + 3, unit 4 * 2 + 1
    assert block[off_A2 + ((29 * 4) + 2) * 64 + 16 + 11] == W2[19, 23, 9]
    # A2T, tile 8 * 6 + 1, row 2, lane (q = 3, i = 6): parameter 4 * 1 + 2 of target 8 * 3 + 6, unit 4 * (6 & 3) + (6 >> 2)
    assert block[off_A2T + ((49 * 4) + 2) * 64 + 48 + 6] == W2[30, 6, 9]
    # A1T, tile 1, row 3, lane (q = 2, i = 13): unit 4 * 3 + 2, source 8 * (13 >> 2) + 4 * 1 + (13 & 3)
    assert block[off_A1T + ((1 * 4) + 3) * 64 + 32 + 13] == W1[14, 29]


def test_lrs_couplings_of_width_64_are_fully_fused(monkeypatch):
    from torchflows_amd import autograd as ag
    from torchflows_amd.bijections.finite.autoregressive.architectures import CouplingLRS

    def routes(D, **kw):
        plan = ag.training_plan(CouplingLRS(D, n_layers=2, **kw), ag.FORWARD)
        packs = ag._plan_packs(plan, D, "cpu", fold=True)
        return ag.fully_fused(plan, D), [r.route for r in packs.records]

    assert routes(64) == (True, [ag._LRS, ag._LRS])
    for D, kw in ((16, {}), (128, {}), (64, dict(conditioner_kwargs=dict(n_hidden=17))), (64, dict(context_shape=(3,)))):
        assert routes(D, **kw) == (False, []), (D, kw)
    set_debug(monkeypatch, train_fused="0")
    assert routes(64) == (False, [])
