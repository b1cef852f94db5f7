"""The weight-stationary f16x3 expand (expand_gemm_x3_ws, VP3D_X3_EXPAND_RING=ws) against the
chunked kernels (=1: three workgroups per CU, =2: two per CU): every form runs the same MFMA
chain per accumulator and the same epilogue, so whole forwards are the same bits.

Config-4 model (1024 channels, 243-frame windows: 81 expand rows per window) on windows of 8
sequences of 1,024 frames.  B is the smallest that reaches each path of the persistent kernel:
  B = 1    81 rows: less than one 128-row group, nearly every workgroup idle
  B = 5    405 rows: 3 full groups and a partial one, fewer groups than row stripes
  B = 300  24,300 rows = 190 groups: unequal trips per stripe, a partial last group
  B = 810  65,610 rows x 4 KB: a split output just over 256 MB, the nontemporal stores
"""
import numpy as np
import pytest
import torch

from helpers import make_model
from oracle.temporal_ref import lifter_forward
from test_gpu_lifter import FP32_COORD_TOL

pytestmark = pytest.mark.gpu

SEQ_LEN, WINDOW, LEAD = 1024, 243, 121
_STATE = {}


def _setup():
    if not _STATE:
        from vp3d_amd.pipeline import SyntheticWindowPool
        model, sd = make_model(True, (3, 3, 3, 3, 3), False, 1024)
        model = model.cuda()
        _STATE.update(sd=sd, lifter=model.native_lifter(torch.device("cuda")), model=model,
                      pool=SyntheticWindowPool(3, device="cuda", n_seq=8, seq_len=SEQ_LEN))
    return _STATE["lifter"], _STATE["pool"], _STATE["sd"]


def _pairs(pool, B):
    """The pool's pair table with its first window moved to a sequence start and (B >= 2) its
    last to a sequence end, so both clamped (non-flat) gather paths run whatever the seed."""
    pairs = pool.global_pairs(B).copy()
    pairs[0, 1] = 3
    if B >= 2:
        pairs[-1, 1] = SEQ_LEN - 2
    first = pairs[:, 1] - LEAD                      # first frame of each window
    at_start, at_end = first < 0, first + WINDOW > SEQ_LEN
    assert at_start.any() and (at_end.any() or B < 2), (at_start.sum(), at_end.sum())
    if B >= 3:  # and unclamped windows beside them: the flat path runs too
        assert not (at_start | at_end).all()
    return pairs


def _forwards(lifter, pool, pairs, monkeypatch, forms=("ws", "1", "2")):
    pd = torch.from_numpy(pairs).cuda()
    ys = {}
    for env in forms:
        monkeypatch.setenv("VP3D_X3_EXPAND_RING", env)
        with torch.no_grad():
            ys[env] = lifter.forward_windows(pool.seqs, pd, WINDOW, LEAD, dtype="f16x3").cpu().numpy()
        lifter.sync_status()  # clean: no range / non-finite fault, no split timeout
    return ys


@pytest.mark.parametrize("B", [1, 5, 300, 810])
def test_x3_expand_ws_bit_identical(B, monkeypatch):
    lifter, pool, _ = _setup()
    if B == 810:
        assert B * 81 * 2 * 1024 * 2 > 256 << 20  # the split expand output: past the nontemporal rule
    ys = _forwards(lifter, pool, _pairs(pool, B), monkeypatch)
    assert ys["ws"].shape == (B, 1, 17, 3) and np.isfinite(ys["ws"]).all()
    assert np.array_equal(ys["ws"], ys["1"]), np.abs(ys["ws"] - ys["1"]).max()
    assert np.array_equal(ys["ws"], ys["2"]), np.abs(ys["ws"] - ys["2"]).max()


def test_x3_expand_ws_plain_rows_and_oracle(monkeypatch):
    """B = 300: the plain-rows form (forward(x) on the pre-gathered windows) under =ws against the
    same forward under =2, and the gathered =ws forward against the CPU oracle at the f16x3 gate
    of test_gpu_lifter.py (the fp32 one)."""
    B = 300
    lifter, pool, sd = _setup()
    pairs = _pairs(pool, B)
    x = pool.seqs.gather(torch.from_numpy(pairs).cuda(), WINDOW, LEAD).reshape(B, WINDOW, 17, 2).contiguous()
    ys = {}
    for env in ("ws", "2"):
        monkeypatch.setenv("VP3D_X3_EXPAND_RING", env)
        with torch.no_grad():
            ys[env] = lifter.forward(x, "f16x3").cpu().numpy()
        lifter.sync_status()
    assert np.isfinite(ys["ws"]).all()
    assert np.array_equal(ys["ws"], ys["2"]), np.abs(ys["ws"] - ys["2"]).max()
    yw = _forwards(lifter, pool, pairs, monkeypatch, forms=("ws",))["ws"]
    assert np.array_equal(yw, ys["ws"])  # gathered on the fly = gathered beforehand
    ref = lifter_forward(sd, x.cpu().numpy(), [3, 3, 3, 3, 3], strided=True).numpy()
    err = np.abs(yw - ref).max()
    print(f"f16x3 ws: max|d|={err:.3e} m")
    assert err <= FP32_COORD_TOL, err
