"""Host-side proofs about the cases of tests/test_gpu_dsf_shapes.py (tests/dsf_reference.py builds both): the helper's
fp64 inverse is the reference's rule, every inverse case excludes at most 10 % of its elements, the parameter-range
cases reach the branches they are for, and the ATen fp32 path alone sits within the bar.  No GPU needed."""
import numpy as np
import pytest
import torch

import dsf_reference as R
from conftest import load_golden
from dsf_reference import bar, normwise, rel
from test_host_dsf import dsf_transformer


def test_inverse64_is_the_reference_rule():
    """``inverse64`` against ``*_xinv64`` of dsf.npz, which the reference's own bisection produced in fp64, on the
    non-clipped elements.  The fixture ended each component's search on the reference's batch-wide ``allclose``, about
    26 trips in, where an element is still a step of 20 * 2^-27 = 1.5e-7 from its root.  So the helper's rule is held
    to the fixture at the reference's stop, where the two must agree to 1e-8 (measured: bit for bit); the fixed 100
    trips then differ from the fixture by that last step (printed; 5.5e-8 norm-wise and 2.8e-7 on the worst element
    at C2_K4, below 2.1e-8 norm-wise for the other three)."""
    fx = load_golden("dsf.npz")
    T = fx["tgt"].size
    for tag in fx["cases"]:
        tr, C, K = dsf_transformer(str(tag), T)
        z_in = fx[f"{tag}_z_in"]
        n = z_in.shape[0]
        keep = ~fx[f"{tag}_clip"]
        want = fx[f"{tag}_xinv64"]
        assert want.dtype == np.float64
        x_stop, _ = R.inverse64(tr, z_in, fx[f"{tag}_h"][:n], reference_stop=True)
        x64, ld64 = R.inverse64(tr, z_in, fx[f"{tag}_h"][:n])
        e_stop, e_x, e_l = normwise(x_stop[keep], want[keep]), normwise(x64[keep], want[keep]), rel(ld64, fx[f"{tag}_ldinv64"])
        worst = float(np.abs(x64 - want)[keep].max())
        print(f"{tag}: inverse64 vs the fixture's fp64 bisection: x {e_stop:.2e} at the reference's stop, {e_x:.2e} after "
              f"100 trips (worst element {worst:.2e}), log-det {e_l:.2e}")
        assert e_stop < 1e-8
        assert e_l < 1e-5
        clip, near = R.walk_d64(tr, fx[f"{tag}_x"][:n][:, fx["tgt"]], fx[f"{tag}_h"][:n])
        assert np.array_equal(clip, fx[f"{tag}_clip"]) and not (clip & ~near).any()


_INVERSE = R.inverse_cases()


@pytest.mark.parametrize("make", [m for _, m in _INVERSE], ids=[i for i, _ in _INVERSE])
def test_inverse_case_excludes_at_most_a_tenth(make):
    case = make()
    clip, near = R.walk_d64(case.tr, R.targets(case), case.h)
    print(f"near share {near.mean():.3%}, clip share {clip.mean():.3%} of {near.size} elements")
    assert near.mean() <= R.NEAR_CAP
    assert not (clip & ~near).any()


@pytest.mark.parametrize("h_scale", R.RANGE_SCALES)
@pytest.mark.parametrize("C,K", R.RANGE_CK)
def test_range_cases_reach_their_branches(C, K, h_scale):
    case = R.case_e(C, K, h_scale)
    clip, _ = R.walk_d64(case.tr, R.targets(case), case.h)
    beyond = R.da_beyond_20(case)
    print(f"C{C}_K{K} h_scale {h_scale:g}: softplus argument > 20 in {beyond:.1%} of da, clipped {clip.mean():.1%}")
    if h_scale == 30000.0:
        assert beyond >= 0.10
    if h_scale >= 3000.0:
        assert clip.any() and not clip.all()
    if h_scale == 0.0:
        assert beyond == 0.0 and not clip.any()
    z64, ld64 = R.forward64(case)
    assert np.isfinite(z64).all() and np.isfinite(ld64).all()


@pytest.mark.parametrize("C,K", [(2, 4), (2, 5), (1, 16), (4, 8), (4, 1), (3, 1)])
def test_aten_fp32_path_meets_the_bar(C, K):
    """floor <= bar(floor), spelled out on the quantities the GPU file measures, and the floor of x itself: with the
    ``near`` rule it stays small where the clip mask alone would let it reach 1e-2."""
    case = R.case_a(C, K)
    z64, ld64 = R.forward64(case)
    z32, ld32 = R.forward32(case)
    f_z, f_l = normwise(z32, z64), rel(ld32, ld64)
    assert f_z <= bar(f_z) and f_l <= bar(f_l)
    p = R.inverse_problem(case)
    keep = ~p.near
    rows = keep.all(axis=1)
    f_x, f_li = normwise(p.x32[keep], p.x64[keep]), rel(p.ld32[rows], p.ld64[rows])
    print(f"C{C}_K{K}: floors z {f_z:.2e}, log-det {f_l:.2e}, x {f_x:.2e} over {keep.mean():.1%} of the elements, "
          f"inverse log-det {f_li:.2e} over {rows.mean():.1%} of the rows")
    assert f_x <= bar(f_x) and f_li <= bar(f_li)
    assert f_x <= 1e-5
    # the fp64 inverse is a fixed point of the fp64 forward on the kept elements
    back = case.tr.forward(torch.from_numpy(p.x64), case.h.double())[0].numpy()
    assert normwise(back[keep], p.z_in.astype(np.float64)[keep]) < 1e-9
