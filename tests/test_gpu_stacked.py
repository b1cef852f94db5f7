"""GPU tests of the fused StackedPoseLifter MLP (csrc/stacked_lifter.hip through the drop-in
common.models.StackedPoseLifter) against the reference's own outputs, tests/golden/stacked_mlp.npz.

Gates:
  * max|y_gpu - y| <= 1e-5 on all five cases: the project's f32 gate of the sequence lifters;
  * for N >= 64 also max|y_gpu - y64| <= 4 max|y - y64|.  On the CPU max|y - y64| is 2e-8 ... 5.5e-8
    for these cases (outputs of 0.03 ... 0.09 rms) and a re-ordered f32 summation lands at
    0.7 ... 1.9 x of it; 4 x leaves twice that spread and stays 40 x below the 1e-5 gate, while a
    dropped product, a 16-bit operand or a wrong pad column misses it by orders of magnitude;
  * a row's result does not depend on the batch it sits in: bit-identical.
"""
import numpy as np
import pytest
import torch

import stacked_common as SC

pytestmark = pytest.mark.gpu

TOL = 1e-5
F64_FACTOR = 4.0


def _model(c):
    from common.models.StackedPoseLifter import StackedPoseLifter
    m = StackedPoseLifter(c["J"], c["F"], c["num_layers"], c["layer_size"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in
                       SC.case_weights(c["J"], c["F"], c["num_layers"], c["layer_size"]).items()})
    return m.cuda().eval()


@pytest.mark.parametrize("i", range(5))
def test_kernel_matches_reference(i):
    cases, y, y64, _ = SC.mlp_golden()
    c = cases[i]
    a, b = SC.case_inputs(c["J"], c["F"], c["N"])
    m = _model(c)
    with torch.no_grad():
        got = m(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    assert got.shape == y[i].shape and got.dtype == torch.float32
    got = got.cpu().numpy()
    err, err64, ref64 = np.abs(got - y[i]).max(), np.abs(got - y64[i]).max(), np.abs(y[i] - y64[i]).max()
    print(f"stacked_mlp case {i} (J {c['J']} layers {c['num_layers']} size {c['layer_size']} N {c['N']}): "
          f"max|gpu - y| {err:.3e}  max|gpu - y64| {err64:.3e}  max|y - y64| {ref64:.3e}")
    assert np.isfinite(got).all()
    assert err <= TOL
    if c["N"] >= 64:
        assert err64 <= F64_FACTOR * ref64


@pytest.mark.parametrize("i", [1, 3])
def test_rows_do_not_depend_on_the_batch(i):
    cases = SC.mlp_golden()[0]
    c = cases[i]
    N = c["N"]
    a, b = SC.case_inputs(c["J"], c["F"], N)
    a, b = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    m = _model(c)
    with torch.no_grad():
        full = m(a, b)
        again = m(a, b)
        assert torch.equal(full, again)
        for r in (0, 63, 64, N - 1):
            alone = m(a[r:r + 1], b[r:r + 1])
            assert torch.equal(alone[0], full[r]), r
        # and across the row tiles (vp3d_stacked_forward halves the 64-row tile while the launch
        # would not fill 256 CUs): 100 rows run on 16-row tiles, ~9,000 on 32, ~16,500 on 64
        assert torch.equal(m(a[:100], b[:100]), full[:100])
        for rows in (9000, 16500):
            reps = -(-rows // N)
            big = m(a.repeat(reps, 1, 1, 1), b.repeat(reps, 1, 1, 1))
            assert torch.equal(big[:N], full) and torch.equal(big[-N:], full), rows


def test_input_layouts():
    cases = SC.mlp_golden()[0]
    c = cases[3]
    N, J, Fe = c["N"], c["J"], c["F"]
    a, b = SC.case_inputs(J, Fe, N)
    a, b = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    m = _model(c)
    with torch.no_grad():
        want = m(a, b)
        assert want.shape == (N, 1, J, Fe)
        assert torch.equal(m(a.view(N, J, Fe), b.view(N, J, Fe)), want)
        assert torch.equal(m(a.view(N, J * Fe), b.view(N, 1, J, Fe)), want)
        # non-contiguous: every other row of a twice-as-long tensor, and a transposed store
        a2 = torch.empty(2 * N, 1, J, Fe, device="cuda")
        a2[::2] = a
        bt = b.view(N, J, Fe).permute(0, 2, 1).contiguous().permute(0, 2, 1)
        assert not a2[::2].is_contiguous() and not bt.is_contiguous()
        assert torch.equal(m(a2[::2], bt), want)


def test_errors():
    from common.models.StackedPoseLifter import StackedPoseLifter
    cases = SC.mlp_golden()[0]
    c = cases[2]
    a, b = SC.case_inputs(c["J"], c["F"], c["N"])
    a, b = torch.from_numpy(a), torch.from_numpy(b)
    m = _model(c)
    with pytest.raises(RuntimeError):
        m(a, b)
    m.train()
    with pytest.raises(NotImplementedError):
        m(a.cuda(), b.cuda())
    m.eval()
    with pytest.raises(AssertionError):
        m(a.cuda()[:, :, :16], b.cuda()[:, :, :16])
    with pytest.raises(AssertionError):
        m(a.cuda(), b.cuda()[:5])
    too_wide = StackedPoseLifter(17, 3, 1, 513).cuda().eval()
    with pytest.raises(AssertionError, match="layer_size must be 1..512"):
        too_wide(a.cuda(), b.cuda())
    # the handle follows the parameters: an in-place change is seen by the next call
    with torch.no_grad():
        y0 = m(a.cuda(), b.cuda())
        m.mlp_layers[0].bias.add_(0.5)
        y1 = m(a.cuda(), b.cuda())
    assert not torch.equal(y0, y1)
    torch.cuda.synchronize()
