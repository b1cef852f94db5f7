"""The f16x3 frame tables (vp3d_forward_windows_pool, VP3D_FRAME_TABLES): with the expand table,
blocks 1 .. d computed once per resident frame position and block d + 1 reading the deepest table
through the per-window row bases are the same bits as the per-window path (VP3D_EXPAND_TABLE=0)
at every depth -- every table row comes from the per-row instruction chain (a4's whole / half-N /
quarter-N tiles, never a split-K form) of the window row it replaces.

The set-up of tests/test_gpu_expand_table.py: the 1,024-channel config-4 model over three sequences
of 300 / 517 / 2,048 frames, batches holding both clamps of every sequence and repeated pairs.
Level pitches per sequence: 2,656 (expand table), 2,650 (block 1), 2,632 (block 2), 2,578 (block 3);
the table launches run 124-128 tiles (half-N tiles), the consuming blocks whole tiles, half-N and
quarter-N tails by batch size.
"""
import numpy as np
import pytest
import torch

from test_gpu_expand_table import LEAD, LENS, WINDOW, _pairs, _seqs, _setup, _t_tab

pytestmark = pytest.mark.gpu

_REF = {}


def _forward(lifter, seqs, pairs, monkeypatch, expand=None, depth=None):
    for name, val in (("VP3D_EXPAND_TABLE", expand), ("VP3D_FRAME_TABLES", depth)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))
    with torch.no_grad():
        y = lifter.forward_windows(seqs, torch.from_numpy(pairs).cuda(), WINDOW, LEAD, dtype="f16x3").cpu().numpy()
    took = (lifter.expand_table_mode(), lifter.frame_table_depth())
    lifter.sync_status()  # clean: no window-start, range or split fault
    return y, took


def _old_path(lifter, seqs, pairs, monkeypatch, key):
    """The per-window path's poses of a batch, computed once per key and left unchanged."""
    if key not in _REF:
        y0, took = _forward(lifter, seqs, pairs, monkeypatch, expand="0")
        assert took == (0, 0) and np.isfinite(y0).all()
        y0.setflags(write=False)
        _REF[key] = y0
    return _REF[key]


def _pitches():
    """Rows per sequence of levels 0 .. 3: each block's k-conv (3 taps, dil = step) takes its reach."""
    p = [_t_tab(max(LENS))]
    for step in (3, 9, 27):
        p.append(p[-1] - 2 * step)
    return p


@pytest.mark.parametrize("depth", [0, 1, 2, 3])
@pytest.mark.parametrize("B", [1024, 1021, 1450])
def test_frame_tables_bit_identical(B, depth, monkeypatch):
    lifter, seqs = _setup()
    pairs = _pairs(B)
    y0 = _old_path(lifter, seqs, pairs, monkeypatch, B)
    y, (mode, took) = _forward(lifter, seqs, pairs, monkeypatch, depth=depth)
    clamped = took != depth
    print(f"B={B} VP3D_FRAME_TABLES={depth}: mode {mode}, depth taken {took}" +
          (" (clamped by the kernels' conditions)" if clamped else ""))
    assert 0 <= took <= depth and (mode == 1 or took == 0)
    if B == 1024 and depth in (1, 2):
        assert took == depth
    assert y.shape == (B, 1, 17, 3)
    assert np.array_equal(y, y0), np.abs(y - y0).max()


@pytest.mark.parametrize("depth", [1, 2])
def test_frame_tables_starts_outside_their_sequence(depth, monkeypatch):
    """Starts before frame 0 and past the last frame, by less and by more than a window: level-l
    row q is built from level-0 rows q .. q + reach, which hold the per-frame edge clamp for every
    start the bases can produce."""
    lifter, seqs = _setup()
    B = 1024
    pairs = _pairs(B)
    odd = [(0, -1), (0, -119), (0, -120), (0, -240), (0, -241), (0, -5000), (1, 517), (1, 517 + 120), (1, 517 + 121),
           (1, 517 + 400), (2, 2048 + 9000), (0, 300), (0, 420), (0, 421)]
    pairs[100:100 + len(odd)] = odd
    y0 = _old_path(lifter, seqs, pairs, monkeypatch, "odd")
    y, took = _forward(lifter, seqs, pairs, monkeypatch, depth=depth)
    assert took == (1, depth)
    assert np.array_equal(y, y0), np.abs(y - y0).max()


def test_frame_tables_size_rule(monkeypatch):
    """Unforced, the depth follows the sizes alone: level l is taken when the table block l reads
    has at most half that block's window rows.  Block 1 reads the expand table (3 x 2,656 = 7,968
    rows) and has 27 rows per window: 27 B / 2 reaches 7,968 at B = 591.  Block 2 reads the block-1
    table and has 9 rows per window."""
    lifter, seqs = _setup()
    pitch = _pitches()
    assert len(LENS) * pitch[0] == 7968 and 27 * 590 // 2 < 7968 <= 27 * 591 // 2
    rows1 = len(LENS) * pitch[1]
    b2 = -(-2 * rows1 // 9)  # the first B with 9 B / 2 >= rows1
    assert 9 * (b2 - 1) // 2 < rows1 <= 9 * b2 // 2 and 3 * b2 // 2 < len(LENS) * pitch[2]
    for B, want in ((590, 0), (591, 1), (b2 - 1, 1), (b2, 2)):
        pairs = _pairs(B)
        y, (mode, took) = _forward(lifter, seqs, pairs, monkeypatch)
        print(f"B={B}: mode {mode}, depth {took}")
        assert took == want and (mode == 1 or want == 0)
        y0 = _old_path(lifter, seqs, pairs, monkeypatch, B)
        assert np.array_equal(y, y0), np.abs(y - y0).max()


def test_frame_tables_sequence_outside_pool_faults(monkeypatch):
    """A pair naming a sequence outside the pool still reports the window-start fault at depth 2
    (the bases in front of the block-2 table), and the next clean forward passes."""
    lifter, seqs = _setup()
    B = 1024
    for bad in ((len(LENS), 5), (-1, 5)):
        pairs = _pairs(B)
        pairs[B // 2] = bad
        pd = torch.from_numpy(pairs).cuda()
        monkeypatch.delenv("VP3D_EXPAND_TABLE", raising=False)
        monkeypatch.setenv("VP3D_FRAME_TABLES", "2")
        with torch.no_grad():
            lifter.forward_windows(seqs, pd, WINDOW, LEAD, dtype="f16x3")
            torch.cuda.synchronize()
            assert lifter.frame_table_depth() == 2
            with pytest.raises(RuntimeError, match="expand table"):
                lifter.forward_windows(seqs, pd, WINDOW, LEAD, dtype="f16x3")
        with pytest.raises(RuntimeError, match="expand table"):
            lifter.sync_status()
        lifter.sync_status()  # reported once, then cleared
        pairs = _pairs(B)
        y, took = _forward(lifter, seqs, pairs, monkeypatch, depth=2)
        assert took == (1, 2)
        assert np.array_equal(y, _old_path(lifter, seqs, pairs, monkeypatch, B))


def test_frame_tables_are_rebuilt_every_forward(monkeypatch):
    """No cache across calls: a sequence's frames overwritten in place on the device between two
    depth-2 forwards give the per-window path's poses on the new frames."""
    lifter, _ = _setup()
    seqs = _seqs(LENS, "reb")
    B = 1024
    pairs = _pairs(B)
    ya, took = _forward(lifter, seqs, pairs, monkeypatch, depth=2)
    assert took == (1, 2)
    assert np.array_equal(ya, _old_path(lifter, seqs, pairs, monkeypatch, "reb-before"))
    lo, n = LENS[0], LENS[1]
    seqs.kps[lo:lo + n] = seqs.kps[lo:lo + n].flip(0) * 0.5
    torch.cuda.synchronize()
    yb, took = _forward(lifter, seqs, pairs, monkeypatch, depth=2)
    assert took == (1, 2)
    y0 = _old_path(lifter, seqs, pairs, monkeypatch, "reb-after")
    assert np.array_equal(yb, y0), np.abs(yb - y0).max()
    assert not np.array_equal(yb, ya)
