"""CPU tests of the split-fp16 representation model (oracle/x3_model.py): the elementwise
bound DESIGN.md §2 states, the range boundary, and the activation-scale family the GPU gates
(test_gpu_x3_numerics.py) are built on.  No GPU."""
import numpy as np
import pytest
import torch

from helpers import make_model
from oracle.temporal_ref import lifter_forward
from oracle.x3_model import (lifter_forward_x3, rescale_activations, split_f16, split_weights,
                             weight_exponent)
from vp3d_amd import synth


def _split_inputs():
    """2^20 f32 values, both signs: log-uniform over [2^-30, 65504], plus every power of two in
    that range, f16 ties (midpoints of neighbouring f16 values, normal and subnormal, and their
    f32 neighbours), and every f16 subnormal with its f32 neighbours."""
    n = 1 << 20
    u = synth.uniform(11, "x3_split", (n,), -30.0, float(np.log2(65504.0)))
    x = np.minimum(np.exp2(u), 65504.0).astype(np.float32)
    extra = [np.exp2(np.arange(-30, 16, dtype=np.float64)).astype(np.float32)]
    # all positive finite f16 values (bit patterns 1 .. 0x7BFF), subnormals included
    h = np.arange(1, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32)
    ties = (0.5 * (h[:-1].astype(np.float64) + h[1:].astype(np.float64))).astype(np.float32)
    sub = h[:1023]
    extra.append(h)
    for v in (ties, sub):
        extra += [v, np.nextafter(v, np.float32(0)), np.nextafter(v, np.float32(np.inf))]
    # hi + (a tie of the lo half): x = hi + half an f16 step of lo's binade
    extra.append((h[1024:4096].astype(np.float64) * (1.0 + 2.0 ** -12 + 2.0 ** -23)).astype(np.float32))
    e = np.concatenate(extra)
    e = e[(e > 0) & (e <= 65504.0)]
    x[1::2] *= -1.0
    x[:2 * e.size] = np.concatenate([e, -e])  # the specials in both signs
    return x


def test_split_elementwise_bound():
    x = _split_inputs()
    assert x.size == 1 << 20 and np.isfinite(x).all()
    assert (x > 0).sum() > 400_000 and (x < 0).sum() > 400_000
    assert np.abs(x).min() <= 2.0 ** -29 and np.abs(x).max() == 65504.0
    xt = torch.from_numpy(x)
    hi, lo = split_f16(xt)
    assert torch.isfinite(hi).all() and torch.isfinite(lo).all()
    x64 = xt.to(torch.float64)
    err = (x64 - hi - lo).abs()
    bound = 2.0 ** -22 * x64.abs() + 2.0 ** -25
    worst = (err / bound).max().item()
    print(f"max |x - hi - lo| / (2^-22 |x| + 2^-25) = {worst:.4f}")
    assert (err <= bound).all(), worst
    # the bound is not slack by more than the two terms it adds: both regimes come close
    assert worst >= 0.5
    # below 2^-3 the error is the absolute floor (half an f16 subnormal step), not relative
    small = x64.abs() < 2.0 ** -3
    assert err[small].max().item() <= 2.0 ** -25
    assert err[small].max().item() >= 0.99 * 2.0 ** -25
    # an f16 value splits exactly with lo = 0
    h = torch.arange(1, 0x7C00, dtype=torch.int16).view(torch.float16)
    hh, hl = split_f16(h)
    assert torch.equal(hh, h.to(torch.float64)) and not hl.any()


def test_split_range_boundary():
    hi, lo = split_f16(torch.tensor([65504.0, -65504.0, 65519.0], dtype=torch.float32))
    assert torch.isfinite(hi).all() and torch.isfinite(lo).all()
    assert hi[0].item() == 65504.0 and hi[1].item() == -65504.0 and lo[0].item() == 0.0
    assert hi[2].item() == 65504.0 and lo[2].item() == 15.0
    hi, _ = split_f16(torch.tensor([65520.0, -65520.0], dtype=torch.float32))
    assert hi[0].item() == float("inf") and hi[1].item() == float("-inf")


def test_weight_split_scale():
    """W 2^e: the largest weight lands in [2^14, 2^15), and the two halves reproduce an f32
    weight to 2^-22 relative of it or half an f16 subnormal step (2^-25) of the scaled value."""
    w = synth.normal(3, "w", (64, 32, 3), 0.02).astype(np.float32)
    for scale in (1.0, 2.0 ** -9, 2.0 ** 7):
        ws = (w * np.float32(scale)).astype(np.float32)
        whi, wlo, e = split_weights(ws)
        assert e == weight_exponent(ws)
        top = np.abs(ws).max() * 2.0 ** e
        assert 2.0 ** 14 <= top < 2.0 ** 15
        v = torch.from_numpy(ws.astype(np.float64)) * 2.0 ** e
        assert ((v - whi - wlo).abs() <= 2.0 ** -22 * v.abs() + 2.0 ** -25).all()
    assert weight_exponent(np.zeros((4, 4, 1), np.float32)) == 0


_FW = (3, 3, 3)
_S = (0, 4, 6, 8, 10)


@pytest.fixture(scope="module")
def small():
    _, sd = make_model(True, _FW, False, 128)
    x = synth.normalized_windows(1, "x4_27", 4, 27)
    ref64 = lifter_forward(sd, x, list(_FW), strided=True, dtype=torch.float64).numpy()
    ref32 = lifter_forward(sd, x, list(_FW), strided=True).numpy()
    return sd, x, ref64, ref32


def test_oracle_invariant_under_activation_rescale(small):
    """The act_s family changes nothing but the hidden activations' scale: the fp32 oracle gives
    the same bits at every s, and the float64 oracle too."""
    sd, x, ref64, ref32 = small
    for s in (0, 4, 8, 10):
        sds = rescale_activations(sd, s)
        assert set(sds) == set(sd)
        y32 = lifter_forward(sds, x, list(_FW), strided=True).numpy()
        assert np.array_equal(y32, ref32), s
        y64 = lifter_forward(sds, x, list(_FW), strided=True, dtype=torch.float64).numpy()
        assert np.array_equal(y64, ref64), s
    # and it does rescale: the expand output of act_8 is 2^-8 of the base one's
    assert np.array_equal(rescale_activations(sd, 8)["expand_bn.bias"], sd["expand_bn.bias"] * np.float32(2.0 ** -8))
    assert np.array_equal(rescale_activations(sd, 0)["shrink.weight"], sd["shrink.weight"])


def _sweep(sd, x, fw, ref64, ref32):
    e_ref32 = np.abs(ref32 - ref64).max()
    errs = {}
    for s in _S:
        y = lifter_forward_x3(rescale_activations(sd, s), x, list(fw), strided=True).numpy()
        assert y.shape == ref64.shape and np.isfinite(y).all()
        errs[s] = np.abs(y - ref64).max()
    print("e_ref32 %.3e; e_model " % e_ref32 + " ".join(f"s={s}: {errs[s]:.3e}" for s in _S))
    assert e_ref32 > 0
    return e_ref32, errs


def test_model_error_sweep(small):
    """The representation's error against float64 on the small model (128 channels, 4 windows):
    no more than the fp32 oracle's own at O(1) activations (s = 0), then growing with every
    step down in scale as the lo halves run into the f16 subnormal floor.

    s = 4 against e_ref32 is asserted on config 4 (test_model_error_sweep_config4), not here:
    measured 8.33e-8 m against e_ref32 = 4.88e-8 m on this model.  The floor is an absolute
    2^-25 per stored activation whatever the layer width, while the fp32 oracle's error grows
    with the length of its sums (K = 384 here, 3,072 in config 4), so where the two cross
    depends on the width: 1.7x over at 128 channels, 0.93x at 1,024."""
    sd, x, ref64, ref32 = small
    e_ref32, errs = _sweep(sd, x, _FW, ref64, ref32)
    assert errs[0] <= e_ref32
    assert errs[4] < errs[6] < errs[8] < errs[10]


def test_model_error_sweep_config4():
    """The same sweep where the fp32 claim is made: config 4 (1,024 channels, (3,3,3,3,3),
    243 frames) on the 24 oracle windows of the GPU tests.  At most e_ref32 at s = 0 and 4,
    strictly increasing from there.  (Measured: e_ref32 2.22e-7 m; model 8.1e-8, 2.05e-7,
    8.9e-7, 4.2e-6, 1.44e-5 m at s = 0, 4, 6, 8, 10.)"""
    fw = (3, 3, 3, 3, 3)
    _, sd = make_model(True, fw, False, 1024)
    x = synth.normalized_windows(1, "x64_243", 24, 243)
    ref64 = lifter_forward(sd, x, list(fw), strided=True, dtype=torch.float64).numpy()
    ref32 = lifter_forward(sd, x, list(fw), strided=True).numpy()
    e_ref32, errs = _sweep(sd, x, fw, ref64, ref32)
    assert errs[0] <= e_ref32 and errs[4] <= e_ref32
    assert errs[4] < errs[6] < errs[8] < errs[10]


def test_model_exact_shrink_flag(small):
    """shrink_f32 takes the shrink's split (rows and weights) out of the model: a different
    result, and the same size of error at O(1) activations."""
    sd, x, ref64, ref32 = small
    y = lifter_forward_x3(sd, x, list(_FW), strided=True).numpy()
    yf = lifter_forward_x3(sd, x, list(_FW), strided=True, shrink_f32=True).numpy()
    assert not np.array_equal(y, yf)
    e_ref32 = np.abs(ref32 - ref64).max()
    assert np.abs(yf - ref64).max() <= e_ref32


def test_model_follows_oracle_geometry():
    """Dilated, causal and dense forms give the oracle's shapes and stay within 4x the fp32
    oracle's own error of float64 (4 = the split's 2^-22 relative bound over f32's 2^-24; a
    wrong slice or dilation is an error of the outputs' own size)."""
    for kw in (dict(strided=False), dict(strided=False, causal=True), dict(strided=False, dense=True),
               dict(strided=True, causal=True)):
        _, sd = make_model(kw["strided"], _FW, kw.get("causal", False), 64, dense=kw.get("dense", False))
        x = synth.normalized_windows(2, "x2_40", 2, 27 if kw["strided"] else 40)
        ref = lifter_forward(sd, x, list(_FW), dtype=torch.float64, **kw).numpy()
        y = lifter_forward_x3(sd, x, list(_FW), **kw).numpy()
        assert y.shape == ref.shape
        e_ref32 = np.abs(lifter_forward(sd, x, list(_FW), **kw).numpy() - ref).max()
        assert np.abs(y - ref).max() <= 4 * e_ref32, kw
