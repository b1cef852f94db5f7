"""The f16x3 activation pre-scale, the parts that need no device (tests/test_gpu_x3_prescale.py
has the rest): choosing exponents from statistics, the oracle-level statement that the rescale
is exact, argument parsing, the refusals, and the C-ABI symbols."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import make_model
from oracle.x3_model import lifter_forward_x3, rescale_activations
from vp3d_amd import _native as N
from vp3d_amd import synth
from vp3d_amd.x3_prescale import (PRESCALE_MAX, chain_layers, check_prescale, choose_prescale, exponent_for,
                                  n_prescale_layers)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FW = (3, 3, 3)  # 5 conv layer outputs: expand, (k-conv, 1x1) x 2


def _stats(absmax):
    return [dict(layer=i, absmax=a, rms=a / 4, small_share=0.0) for i, a in enumerate(absmax)]


def test_layer_bookkeeping():
    assert n_prescale_layers(FW) == 5 and chain_layers(FW) == [0, 2, 4]
    assert n_prescale_layers((3,)) == 1 and chain_layers((3,)) == [0]
    assert n_prescale_layers((3, 3, 3, 3, 3)) == 9


@pytest.mark.parametrize("headroom", [0, 4, 6, 9])
def test_exponent_is_the_largest_under_the_limit(headroom):
    """absmax 2^p < 2^(16 - headroom) holds at the chosen p and fails at p + 1, at powers of two
    (where the bound is met with equality one step later), just under and just over them."""
    limit = 2.0 ** (16 - headroom)
    for k in range(-6, 10):
        for a in (2.0 ** k, float(np.nextafter(np.float32(2.0 ** k), np.float32(0))),
                  float(np.nextafter(np.float32(2.0 ** k), np.float32(np.inf))), 1.37 * 2.0 ** k):
            p = exponent_for(a, headroom)
            assert abs(p) < PRESCALE_MAX, "the case is meant to stay inside the clamp"
            assert a * 2.0 ** p < limit <= a * 2.0 ** (p + 1), (a, p)
    assert exponent_for(1.0, 6) == 9      # 2^9 < 2^10, 2^10 is not
    assert exponent_for(0.999, 6) == 10
    assert exponent_for(1024.0, 6) == -1


def test_exponent_edge_values():
    for a in (0.0, -0.0, float("inf"), float("nan")):
        assert exponent_for(a) == 0
    assert exponent_for(1e-30) == PRESCALE_MAX    # clamped
    assert exponent_for(1e30) == -PRESCALE_MAX


def test_choose_prescale_chain_takes_the_largest_chain_absmax():
    p = choose_prescale(_stats([0.5, 3.0, 7.9, 0.6, 2.0]), FW)
    assert p[0] == p[2] == p[4] == exponent_for(7.9) == 7
    assert p[1] == exponent_for(3.0) == 8 and p[3] == exponent_for(0.6) == 10
    check_prescale(p, FW)
    # tuples starting with absmax are taken too; headroom_bits moves every exponent alike
    q = choose_prescale([(0.5,), (3.0,), (7.9,), (0.6,), (2.0,)], FW, headroom_bits=4)
    assert q == [v + 2 for v in p]
    # a rescale of every activation by 2^-s moves every exponent by exactly s
    for s in (4, 10, 14, -3):
        assert choose_prescale(_stats([a * 2.0 ** -s for a in (0.5, 3.0, 7.9, 0.6, 2.0)]), FW) == [v + s for v in p]


def test_choose_prescale_zero_and_non_finite():
    assert choose_prescale(_stats([0.0] * 5), FW) == [0] * 5
    # a zero chain layer is ignored by the max; a zero k-conv layer gets 0
    p = choose_prescale(_stats([0.0, 0.0, 2.0, 1.0, 0.0]), FW)
    assert p == [exponent_for(2.0), 0, exponent_for(2.0), exponent_for(1.0), exponent_for(2.0)]
    # a non-finite chain layer: the chain gets 0; a non-finite k-conv layer: that layer gets 0
    p = choose_prescale(_stats([1.0, float("nan"), float("inf"), 1.0, 1.0]), FW)
    assert p == [0, 0, 0, exponent_for(1.0), 0]
    with pytest.raises(ValueError, match="5 layers"):
        choose_prescale(_stats([1.0] * 4), FW)


def test_check_prescale_refusals():
    assert check_prescale([3, -2, 3, 7, 3], FW) == [3, -2, 3, 7, 3]
    with pytest.raises(ValueError, match="layer 2"):
        check_prescale([3, 0, 4, 0, 3], FW)
    with pytest.raises(ValueError, match="layer 3 has exponent 25"):
        check_prescale([0, 0, 0, 25, 0], FW)
    with pytest.raises(ValueError, match="expected 5 exponents"):
        check_prescale([0, 0, 0], FW)


def test_module_api_without_a_device():
    """The exponents live on the module as a plain attribute: no state_dict key, kept by
    load_state_dict, refused like the C-ABI refuses them; calibration needs eval mode and a HIP
    tensor."""
    import torch
    m, sd = make_model(True, FW, channels=64)
    keys = list(m.state_dict().keys())
    assert m.f16x3_prescale() == [0] * 5
    m.set_f16x3_prescale([2, 5, 2, -1, 2])
    assert m.f16x3_prescale() == [2, 5, 2, -1, 2]
    assert list(m.state_dict().keys()) == keys
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    assert m.f16x3_prescale() == [2, 5, 2, -1, 2]
    with pytest.raises(ValueError, match="layer 4"):
        m.set_f16x3_prescale([2, 5, 2, -1, 3])
    with pytest.raises(ValueError, match="past"):
        m.set_f16x3_prescale([-25, 0, -25, 0, -25])
    with pytest.raises(ValueError, match="expected 5"):
        m.set_f16x3_prescale([0] * 9)
    assert m.f16x3_prescale() == [2, 5, 2, -1, 2]  # a refused vector changes nothing
    m.set_f16x3_prescale([0] * 5)
    assert m._x3_prescale is None and m.f16x3_prescale() == [0] * 5
    x = torch.zeros(2, 9, 17, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.calibrate_f16x3(x)
    m.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        m.calibrate_f16x3(x)


@pytest.mark.parametrize("s", [4, 10, 14])
def test_oracle_rescale_round_trip_is_exact(s):
    """The oracle-level statement of the GPU invariance case, on the 128-channel fw (3, 5, 3)
    model: the rescale by 2^-s and back returns the state dict bit for bit, so the split-fp16
    model gives the base model's bits -- the pre-scale that undoes a small-activation
    checkpoint loses nothing."""
    fw = (3, 5, 3)
    _, sd = make_model(True, fw, channels=128)
    xs = synth.normalized_windows(1, "x5_45", 5, 45).copy()
    xs[1] = 0.0
    xs[3] *= np.float32(32.0)
    back = rescale_activations(rescale_activations(sd, s), -s)
    for k in sd:
        assert np.array_equal(np.asarray(back[k]), np.asarray(sd[k])), k
    y0 = lifter_forward_x3(sd, xs, list(fw), strided=True).numpy()
    y1 = lifter_forward_x3(back, xs, list(fw), strided=True).numpy()
    assert np.array_equal(y0, y1)


def test_run_arguments_and_refusals():
    import run
    from common.arguments import parse_args
    assert parse_args([]).x3_calibrate == 0
    ok = parse_args(["--evaluate", "synthetic", "--compute-dtype", "f16x3", "--x3-calibrate", "512"])
    assert ok.x3_calibrate == 512 and run.x3_calibrate_refusal(ok) is None
    assert run.x3_calibrate_refusal(parse_args(["--evaluate", "synthetic"])) is None  # off
    for dtype in ("fp32", "bf16", "fp16"):
        with pytest.raises(SystemExit, match="f16x3"):
            run.main(["--evaluate", "synthetic", "--compute-dtype", dtype, "--x3-calibrate", "64"])
    for name in ("Transformer", "LSTM-Coupled", "LSTM-Uncoupled", "StackedPoselifter"):
        args = parse_args(["--evaluate", "synthetic", "--use-model", name, "--compute-dtype", "f16x3",
                           "--x3-calibrate", "64"])
        assert name in run.x3_calibrate_refusal(args)
    with pytest.raises(SystemExit, match="--evaluate"):
        run.main(["--compute-dtype", "f16x3", "--x3-calibrate", "64"])
    with pytest.raises(SystemExit, match=">= 0"):
        run.main(["--evaluate", "synthetic", "--compute-dtype", "f16x3", "--x3-calibrate", "-1"])


def test_capi_symbols_and_null_arguments():
    names = ["vp3d_set_x3_prescale", "vp3d_get_x3_prescale", "vp3d_x3_calibrate", "vp3d_x3_calibrate_windows"]
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vp3d.h")).read(), flags=re.S)
    lib = N.load()
    for n in names:
        assert re.search(r"\b" + n + r"\s*\(", txt), n
        assert n in N.EXPORTS and hasattr(lib, n)
    assert "VP3D_X3_PRESCALE_MAX 24" in txt and N.X3_PRESCALE_MAX == PRESCALE_MAX == 24
    assert ctypes.sizeof(N.vp3d_act_stats) == 24
    p = (ctypes.c_int32 * 3)()
    assert lib.vp3d_set_x3_prescale(None, p, 3) == N.VP3D_ERR_ARG
    assert lib.vp3d_get_x3_prescale(None, p, 3) == N.VP3D_ERR_ARG
    assert lib.vp3d_x3_calibrate(None, None, 1, 1, None, None) == N.VP3D_ERR_ARG
    assert b"handle is NULL" in lib.vp3d_last_error()
