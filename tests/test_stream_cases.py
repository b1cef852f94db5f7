"""The causal-stream oracle (oracle/stream_ref.py) on the shapes of tests/stream_cases.py, on
the CPU: before tests/test_gpu_stream_shapes.py holds the device to 2e-5 m against it, the
reference has to be sound at every one of those shapes.

  * its own arithmetic error -- float32 against float64 evaluation of the same (rounded)
    weights -- is at most 2e-6 m, a tenth of the device gate (measured: <= 7.6e-7 m, on deep6);
  * the edge-padded whole-sequence evaluation really is causal: pose k does not move by a bit
    when every later frame changes, so "pose k of the stream" is well defined;
  * round_weights rounds exactly the conv weights, and rounding is idempotent.
"""
import numpy as np
import pytest
import torch

import stream_cases as sc
from oracle.stream_ref import round_weights, stream_reference

REF_TOL = 2e-6  # metres: float32 oracle vs float64 oracle


def test_case_table_is_consistent():
    assert len(set(sc.CASE_NAMES)) == len(sc.CASES) == 15
    for c in sc.CASES:
        for forms in (c.forms16, c.forms32):
            assert len(forms) == len(sc.MODES) and set(forms) <= {"launches", "persist", "pipe"}
            unset, launches, persist, pipe = forms
            # the dispatch's order of preference (module docstring of stream_cases)
            assert launches == "launches" and pipe == unset
            assert persist in ("persist", "launches") and (unset == "launches") <= (persist == "launches")
        assert "persist" not in c.forms32  # fp32 weights have no LDS-resident form
        assert c.T > 64  # past the frame queue
    assert sc.case("deep6").T > 512  # past its longest ring


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_reference_is_sound(name):
    c = sc.case(name)
    for wdtype in sc.DTYPES:
        y64 = sc.oracle_poses(name, wdtype)
        assert y64.shape == (c.T, c.jout, 3) and np.isfinite(y64).all()
        e = sc.reference_error(name, wdtype)
        print(f"{name} {wdtype}: float32 oracle vs float64 max|d|={e:.3e} m, rms pose {np.sqrt((y64 ** 2).mean()):.3f} m")
        assert e <= REF_TOL
    # the roundings are not no-ops at this shape: each moves the poses, bf16 more than fp16
    d16 = np.abs(sc.oracle_poses(name, "fp16") - sc.oracle_poses(name, "fp32")).max()
    dbf = np.abs(sc.oracle_poses(name, "bf16") - sc.oracle_poses(name, "fp32")).max()
    assert 0.0 < d16 < dbf


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_reference_is_causal(name):
    c = sc.case(name)
    sd = sc.rounded_state(name, "fp32")
    x = sc.case_input(name)
    base = stream_reference(sd, x, c.fw, dense=c.dense)
    np.testing.assert_array_equal(base, sc.oracle_poses(name, "fp32"))
    other = sc.case_input(name, "A", c.T)
    for k in (0, c.T // 2, c.T - 2):
        y = x.copy()
        y[:, k + 1:] = other[:, k + 1:]
        moved = stream_reference(sd, y, c.fw, dense=c.dense)
        np.testing.assert_array_equal(moved[:k + 1], base[:k + 1])
        assert np.abs(moved[k + 1] - base[k + 1]).max() > 1e-4  # the change itself is visible


@pytest.mark.parametrize("name", ["dense", "jout32", "expand1"])
@pytest.mark.parametrize("wdtype", ["fp16", "bf16"])
def test_round_weights_rounds_exactly_the_conv_weights(name, wdtype):
    _, sd = sc.case_model(name)
    r = round_weights(sd, wdtype)
    assert round_weights(sd, "fp32") is sd
    assert list(r) == list(sd)
    to = {"fp16": torch.float16, "bf16": torch.bfloat16}[wdtype]
    n_conv = 0
    for k, v in sd.items():
        if k.endswith("conv.weight") or k == "shrink.weight" or (k.startswith("layers_conv") and k.endswith(".weight")):
            n_conv += 1
            assert v.ndim == 3 and r[k].dtype == np.float32 and r[k].shape == v.shape
            assert (r[k] != v).any(), k
            # representable in the 16-bit type, and the nearest such value
            np.testing.assert_array_equal(torch.from_numpy(r[k]).to(to).float().numpy(), r[k])
            ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(v), 1e-30))) - (10 if wdtype == "fp16" else 7))
            normal = np.abs(v) >= (2.0 ** -14 if wdtype == "fp16" else 2.0 ** -126)
            assert (np.abs(r[k] - v)[normal] <= 0.5 * ulp[normal]).all(), k
        else:
            assert r[k] is v, k
    assert n_conv == 2 * len(sc.case(name).fw)  # expand, two per block, shrink
    again = round_weights(r, wdtype)
    for k in r:
        np.testing.assert_array_equal(again[k], r[k])


def test_round_weights_keeps_tensors_tensors():
    _, sd = sc.case_model("one_width")
    t = {k: torch.from_numpy(v.copy()) for k, v in sd.items()}
    r = round_weights(t, "fp16")
    want = round_weights(sd, "fp16")
    for k in t:
        assert isinstance(r[k], torch.Tensor)
        np.testing.assert_array_equal(r[k].numpy(), want[k])
