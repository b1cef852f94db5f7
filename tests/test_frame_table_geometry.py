"""The index mapping of the f16x3 frame tables (vp3d_forward_windows_pool, VP3D_FRAME_TABLES),
restated in float64 torch on the CPU: row j of block b's output in the window starting at frame s
is a function of the sequence and of frame position s + step j alone, so the expand conv and
blocks 1 .. d can be computed once per table row -- one row per frame position, a dilated conv at
stride 1 per sequence over the level below, the residual slice at R_off -- and block d + 1 reads
window b's row j at row base[b] + j step of the deepest table.

Tiny Optimized1f model (8 channels, 243-frame windows) over two sequences of unequal length, starts
before, inside and past each sequence.  The tables are built with the formulas the library uses
(plan_expand_table / plan_frame_tables in csrc/vp3d_capi.cpp, window_bases in
csrc/expand_table.hip) and the result is compared with oracle.temporal_ref.lifter_forward on the
gathered, edge-clamped windows.  Same arithmetic in another association order only where torch's
conv1d differs between its strided and dilated forms: the gate is float64 rounding -- sums of at
most 24 products of O(1) values over 10 layers, so 1e-12 absolute on poses of ~0.1 is three orders
above the rounding and ten below any index slip.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import make_model
from oracle.temporal_ref import lifter_forward

FW = (3, 3, 3, 3, 3)
WINDOW, LEAD = 243, 121
LENS = (70, 301)
JIN, FIN, JOUT, CH = 5, 2, 4, 8
# (sequence, start): before frame 0 by less / more than a window, inside, the last frame, past the end
PAIRS = [(0, 0), (0, -1), (0, -119), (0, -240), (0, -241), (0, -5000), (0, 17), (0, 69), (0, 70), (0, 190), (0, 191),
         (0, 9000), (1, 0), (1, -7), (1, 150), (1, 150), (1, 300), (1, 301), (1, 301 + 121), (1, 301 + 400), (1, -300)]
_STATE = {}


def _setup():
    if not _STATE:
        torch.set_num_threads(2)
        _, sd = make_model(True, FW, False, CH, jin=JIN, fin=FIN, jout=JOUT)
        rng = np.random.RandomState(5)
        seqs = [rng.standard_normal((n, JIN, FIN)) for n in LENS]
        pairs = np.asarray(PAIRS, dtype=np.int64)
        # the gathered windows: frames [start - lead, start - lead + window), edge-clamped per frame
        win = np.stack([seqs[i][np.clip(np.arange(s - LEAD, s - LEAD + WINDOW), 0, LENS[i] - 1)] for i, s in pairs])
        ref = lifter_forward(sd, win, list(FW), strided=True, dtype=torch.float64).numpy()
        ref.setflags(write=False)
        _STATE.update(sd={k: torch.from_numpy(np.asarray(v)).double() for k, v in sd.items()}, seqs=seqs, pairs=pairs,
                      ref=ref)
    return _STATE["sd"], _STATE["seqs"], _STATE["pairs"], _STATE["ref"]


def _bn_relu(h, sd, name):
    return F.relu(F.batch_norm(h, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"],
                               sd[name + ".bias"], False, 0.1, 1e-5))


def _tables_forward(sd, seqs, pairs, depth):
    n_seq, max_len = len(seqs), max(LENS)
    taps = s0 = FW[0]
    rows0 = (WINDOW - taps) // s0 + 1           # 81 expand rows per window
    span = (rows0 - 1) * s0                     # table rows a window steps over
    lo = -(span + max(0, taps - 1 - LEAD))
    t_tab = (max_len - 1 + LEAD - lo + span + 1 + 15) // 16 * 16
    # level 0: row q of sequence i = the expand output of the window start lo + q
    level = []
    for x in seqs:
        fr = np.clip(lo - LEAD + np.arange(t_tab + taps - 1), 0, len(x) - 1)
        h = torch.from_numpy(x[fr]).reshape(1, len(fr), -1).permute(0, 2, 1)
        level.append(_bn_relu(F.conv1d(h, sd["expand_conv.weight"]), sd, "expand_bn"))
    table = torch.cat(level, 0)                 # (n_seq, C, pitch)
    pitch, step = [t_tab], [s0]
    assert table.shape[2] == t_tab
    for b in range(1, depth + 1):
        w, st = FW[b], step[-1]
        # the k-conv once per table row: stride 1, dil = L.dil * step, T_out = T_in - (taps - 1) dil
        k3 = _bn_relu(F.conv1d(table, sd[f"layers_conv.{2 * b - 2}.weight"], dilation=st), sd, f"layers_bn.{2 * b - 2}")
        pout = pitch[-1] - (w - 1) * st
        assert k3.shape[2] == pout
        # the 1x1 row-wise; the residual from the block-input table: R_stride = 1, R_off = res_off * step
        r_off = (w // 2) * st
        table = table[:, :, r_off:r_off + pout] + _bn_relu(F.conv1d(k3, sd[f"layers_conv.{2 * b - 1}.weight"]), sd,
                                                           f"layers_bn.{2 * b - 1}")
        pitch.append(pout)
        step.append(st * w)
    # the flat table and the windows' bases at the deepest pitch (window_bases)
    flat = table.permute(0, 2, 1).reshape(n_seq * pitch[-1], -1)
    start = np.clip(pairs[:, 1], lo, np.asarray(LENS)[pairs[:, 0]] - 1 + LEAD)
    base = pairs[:, 0] * pitch[-1] + start - lo
    rows = rows0 // int(np.prod(FW[1:depth + 1]))  # window rows of block `depth`'s output
    idx = base[:, None] + np.arange(rows)[None, :] * step[-1]
    # no row mixes two sequences
    assert (idx // pitch[-1] == pairs[:, :1]).all() and idx.min() >= 0 and idx.max() < flat.shape[0]
    h = flat[torch.from_numpy(idx)].permute(0, 2, 1)  # (B, C, rows): the per-window block input
    for b in range(depth + 1, len(FW)):
        w = FW[b]
        res = h[:, :, w // 2::w]
        h = _bn_relu(F.conv1d(h, sd[f"layers_conv.{2 * b - 2}.weight"], stride=w), sd, f"layers_bn.{2 * b - 2}")
        h = res + _bn_relu(F.conv1d(h, sd[f"layers_conv.{2 * b - 1}.weight"]), sd, f"layers_bn.{2 * b - 1}")
    h = F.conv1d(h, sd["shrink.weight"], sd["shrink.bias"])
    return h.permute(0, 2, 1).reshape(len(pairs), h.shape[2], -1, 3).numpy(), pitch, step


@pytest.mark.parametrize("depth", [0, 1, 2, 3])
def test_frame_tables_match_the_windowed_forward(depth):
    sd, seqs, pairs, ref = _setup()
    with torch.no_grad():
        y, pitch, step = _tables_forward(sd, seqs, pairs, depth)
    assert step == [3 ** (l + 1) for l in range(depth + 1)]
    assert pitch == [pitch[0] - sum(2 * 3 ** l for l in range(1, l1 + 1)) for l1 in range(depth + 1)]
    assert y.shape == ref.shape == (len(pairs), 1, JOUT, 3)
    err = float(np.abs(y - ref).max())
    print(f"depth {depth}: pitches {pitch}, steps {step}, max |d| = {err:.3e} on poses of rms {ref.std():.3f}")
    assert err <= 1e-12, err
