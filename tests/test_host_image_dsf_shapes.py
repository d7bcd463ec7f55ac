"""Host-side proofs about the cases of tests/test_gpu_image_dsf_shapes.py (tests/image_dsf_reference.py builds both), from
the references alone: the inverse excludes at most 2 % of any case, the sensitivity condition, and the compiled step has
the shape the kernel expects.  No GPU needed (the built library only for ``compile_program`` on the CPU device).

The sensitivity condition.  Three mistakes a kernel could make (the conditioner's output of the neighbouring sample, of
the neighbouring target, the components in reverse order) are each to move the float64 z (norm-wise) and log-det
(relative) by at least ten bars.  Asserted per case and per quantity:

* z under the sample and the target roll: ten bars, every case;
* every log-det quantity: ten bars, except where ``R.SHORT_OF_TEN`` records the case and the quantity as short of it; a
  recorded one must still move by ``R.ABOVE_THE_BAR`` bars, so that the mistake fails the log-det comparison as well;
* the order of the components is held by the log-det alone: ``R.ORDER_HELD`` bars in every case with C >= 2 but the two
  named in ``test_every_kernel_has_a_case_that_holds_the_component_order``, and for every K in at least one case;
* z under reversed components cannot meet the condition in any case (asserted as such, so that the statement cannot go
  stale): the conditioner's output is bounded to (-2, 2) and enters as da / 1000, db / 1000, dw / 1000, so every component
  is the same map up to 2e-3 and two of them commute to second order.  No case is dropped for it, since every case with
  two or more components would go."""
import numpy as np
import pytest
import torch

import image_dsf_reference as R
from image_dsf_reference import bar, normwise, rel  # noqa: F401

CASES = R.all_cases()
IDS = [f"{s}-C{C}-K{K}" for s, C, K in CASES]


@pytest.mark.parametrize("name,C,K", CASES, ids=IDS)
def test_inverse_excludes_at_most_two_percent(name, C, K):
    share = R.excluded_share(name, C, K)
    case, ref = R.make_case(name, C, K), R.reference(name, C, K)
    f_z = normwise(ref.z32[:, case.cols], ref.z64[:, case.cols])
    keep = R.keep_mask(case, ref, R.N_ROWS)
    f_x = normwise(ref.x32[:, case.cols][keep], ref.x64[:, case.cols][keep])
    print(f"{name} C{C}_K{K}: excluded {share:.2%}; floors z {f_z:.2e}, x {f_x:.2e}, log-det {rel(ref.ld32, ref.ld64):.2e}, "
          f"inverse log-det {rel(ref.ldi32, ref.ldi64):.2e}")
    assert share <= R.EXCLUDED_CAP
    assert np.isfinite(ref.z64).all() and np.isfinite(ref.x64).all()
    # the float64 inverse returns the input (on the kept elements): z_in is reachable
    assert normwise(ref.x64[:, case.cols][keep], case.x.reshape(R.N_ROWS, -1).numpy()[:, case.cols][keep]) < 1e-5


@pytest.mark.parametrize("name,C,K", CASES, ids=IDS)
def test_sensitivity_condition(name, C, K):
    moved = R.moved_in_bars(name, C, K)
    print(f"{name} C{C}_K{K}: " + ", ".join(f"{q} {v:.1f}" for q, v in moved.items()) + " bars")
    assert set(moved) == set(R.QUANTITIES if C >= 2 else R.QUANTITIES[:4])
    short = {dict(s="sample_ld", t="target_ld", c="components_ld")[c] for c in R.SHORT_OF_TEN.get(name, {}).get((C, K), "")}
    for q, v in moved.items():
        if q == "components_z":
            assert v < R.SENSITIVITY, "reversed components now move z by ten bars: hold it to them like the rest"
        elif q in short:
            assert v >= R.ABOVE_THE_BAR, q
        else:
            assert v >= R.SENSITIVITY, q


ORDER_BELOW_TWO = {("checker_3x8x8_T96", 2, 11), ("checker_3x8x8_T96", 2, 16)}           # 1.5 and 1.9 bars


def test_every_kernel_has_a_case_that_holds_the_component_order():
    """Reversed components move the log-det by at least two bars in every case with C >= 2 except the two above (which
    the bars hold by 1.5 and 1.9: a launch would have to spend its own error against the mistake to pass), so for every
    hidden_dim, i.e. every instantiation of the kernel, some case holds the order whatever the launch's own error."""
    held = set()
    for name, C, K in CASES:
        if C >= 2:
            v = R.moved_in_bars(name, C, K)["components_ld"]
            assert v >= R.ORDER_HELD or (name, C, K) in ORDER_BELOW_TWO, (name, C, K, v)
            if v >= R.ORDER_HELD:
                held.add(K)
    assert held == set(range(1, 17))


PROGRAM_CASES = [(s, C, K) for s in R.SHAPES for C, K in R.GEOMETRY_CK]


@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("name,C,K", PROGRAM_CASES, ids=[f"{s}-C{C}-K{K}" for s, C, K in PROGRAM_CASES])
def test_program_shape(name, C, K, d, monkeypatch):
    from torchflows_amd import native
    native.lib()                                          # (a missing library is an error here, not a skip)
    case = R.make_case(name, C, K)
    T = case.T
    prog, step = R.compile_step(case, d, torch.device("cpu"))
    L = step.layer
    assert (L.kind, L.n_ch, L.hw, L.T) == (3, C, K, T) and L.n_params == T * 3 * K * C and step.inverse == bool(d)
    assert step.keep[7].numel() == (T + 15) // 16 * 3 * K * C * 256 and step.keep[8].numel() == (T + 15) // 16 * 3 * K * C * 16
    assert step.keep[2].numel() % 16 == 0 and step.keep[2].numel() >= T          # (the kernel reads whole groups of 16)
    assert step.info["block"] <= 256 and step.info["tile_rows"] == 16
    assert sorted(step.keep[2][:T].tolist()) == sorted(case.cols.tolist())
    # a pending map only behind an ActNorm: forward it sits on sources and targets, inverse it is all left to the flush
    pending = name.startswith("normalized")
    assert (prog.flush is not None) == pending and (prog.ld_const != 0.0) == pending
    identity = torch.tensor([1.0, 0.0]).expand(T, 2)
    assert torch.equal(step.keep[3][:T], identity) != (pending and d == 0)
    monkeypatch.setenv("TORCHFLOWS_AMD_DEBUG", "glow_block=128,glow_grid=2")
    _, small = R.compile_step(case, d, torch.device("cpu"))
    assert small.info["block"] == 128 and small.layer.block == 128 and small.layer.grid == 2
