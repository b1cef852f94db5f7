"""The trimmed layout of the f16x3 expand / frame tables (vp3d_forward_windows_pool,
VP3D_TABLE_TRIM): the table rows of the window starts 0 .. max_len - 1 alone, the starts before
frame 0 and past the last frame served by two edge segments per sequence whose launches are gated
on the batch holding such a start, and the depth rule of the tables -- always the same bits as the
per-window path (VP3D_EXPAND_TABLE=0).

The set-up of tests/test_gpu_expand_table.py: the 1,024-channel config-4 model over three sequences
of 300 / 517 / 2,048 frames (main pitches 2,288 / 2,282 / 2,264 / 2,210 rows per sequence, edge
segments of 480 / 474 / 456 / 402), batches of about 1,024 windows.
"""
import numpy as np
import pytest
import torch

from test_gpu_expand_table import LEAD, LENS, WINDOW, _pairs, _seqs, _setup
from test_gpu_frame_tables import _old_path

pytestmark = pytest.mark.gpu

WIDE, TRIMMED = 1, 2
ODD = [(0, -1), (0, -119), (0, -120), (0, -240), (0, -241), (0, -5000), (1, 517), (1, 517 + 120), (1, 517 + 121),
       (1, 517 + 400), (2, 2048 + 9000), (0, 300), (0, 420), (0, 421)]


def _forward(lifter, seqs, pairs, monkeypatch, trim="1", depth=None):
    """One table forward; returns the poses and (mode, depth, layout, edge gate) -- the gate read
    after the copy back has synchronised."""
    monkeypatch.delenv("VP3D_EXPAND_TABLE", raising=False)
    for name, val in (("VP3D_TABLE_TRIM", trim), ("VP3D_FRAME_TABLES", depth)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))
    with torch.no_grad():
        y = lifter.forward_windows(seqs, torch.from_numpy(pairs).cuda(), WINDOW, LEAD, dtype="f16x3").cpu().numpy()
    layout, edges = lifter.table_layout()
    took = (lifter.expand_table_mode(), lifter.frame_table_depth(), layout, edges)
    lifter.sync_status()  # clean: no window-start, range or split fault
    return y, took


def _odd_pairs(B=1024):
    pairs = _pairs(B)
    pairs[100:100 + len(ODD)] = ODD
    return pairs


@pytest.mark.parametrize("depth", [0, 1, 2, 3])
@pytest.mark.parametrize("B", [1024, 1021, 1450])
def test_trimmed_in_range_bit_identical(B, depth, monkeypatch):
    """Starts inside their sequences: the main region alone, the edge launches gated off."""
    lifter, seqs = _setup()
    pairs = _pairs(B)
    y0 = _old_path(lifter, seqs, pairs, monkeypatch, B)
    y, (mode, took, layout, edges) = _forward(lifter, seqs, pairs, monkeypatch, depth=depth)
    print(f"B={B} VP3D_FRAME_TABLES={depth}: mode {mode}, depth {took}, layout {layout}, edges {edges}")
    # (the forced depth is taken at all three batch sizes, depth 3 included: the level-3 main region
    # is compared here, its edge segments in the tests below)
    assert mode == 1 and took == depth
    assert layout == TRIMMED and not edges
    assert np.array_equal(y, y0), np.abs(y - y0).max()


@pytest.mark.parametrize("depth", [0, 1, 2, 3])
def test_trimmed_starts_outside_their_sequence(depth, monkeypatch):
    """Starts before frame 0 and past the last frame, by less and by more than a window: the gate
    fires and the edge segments hold the per-frame edge clamp."""
    lifter, seqs = _setup()
    pairs = _odd_pairs()
    y0 = _old_path(lifter, seqs, pairs, monkeypatch, "odd")
    y, (mode, took, layout, edges) = _forward(lifter, seqs, pairs, monkeypatch, depth=depth)
    assert mode == 1 and took == depth
    assert layout == TRIMMED and edges
    assert np.array_equal(y, y0), np.abs(y - y0).max()


@pytest.mark.parametrize("name,at,put,fires", [
    ("low", -1, [(0, -1)], True),                                    # one window, the batch's last pair
    ("high", -1, [(2, 2048)], True),
    ("quartet", -4, [(2, -1), (2, 0), (2, 2047), (2, 2048)], True),  # both boundaries of the main region
    ("short", 100, [(0, 300), (0, 420), (1, 2047)], False),          # past a short sequence, below max_len: main
])
def test_trimmed_gate_at_its_smallest(name, at, put, fires, monkeypatch):
    lifter, seqs = _setup()
    B = 1024
    pairs = _pairs(B)
    at = at % B
    pairs[at:at + len(put)] = put
    y0 = _old_path(lifter, seqs, pairs, monkeypatch, "gate-" + name)
    y, (mode, took, layout, edges) = _forward(lifter, seqs, pairs, monkeypatch, depth=2)
    assert (mode, took, layout) == (1, 2, TRIMMED)
    assert edges == fires
    assert np.array_equal(y, y0), np.abs(y - y0).max()


@pytest.mark.parametrize("depth", [1, 3])
def test_trimmed_short_sequence_in_the_high_segment(depth, monkeypatch):
    """A sequence shorter than max_len whose clamped start still reaches the high edge segment: 2,000
    frames beside 2,048, lead 121 -- starts from 2,048 on clamp to at most 2,120 and read the rows of
    the pseudo-window (0, 2048), which holds that sequence's own per-frame clamp to frame 1,999."""
    lifter, _ = _setup()
    lens = (2000, 2048)
    seqs = _seqs(lens, "shorthigh")
    pairs = _pairs(1024, lens)
    put = [(0, 1999), (0, 2047), (0, 2048), (0, 2100), (0, 2120), (0, 2121), (0, 9000), (1, 2048), (1, 2168)]
    pairs[100:100 + len(put)] = put
    y0 = _old_path(lifter, seqs, pairs, monkeypatch, "shorthigh")
    y, (mode, took, layout, edges) = _forward(lifter, seqs, pairs, monkeypatch, depth=depth)
    assert (mode, took, layout, edges) == (1, depth, TRIMMED, True)
    assert np.array_equal(y, y0), np.abs(y - y0).max()
    # the same batch without the starts from max_len on: the main region alone serves (0, 1999 .. 2047)
    pairs[102:100 + len(put)] = (0, 2047)
    y0 = _old_path(lifter, seqs, pairs, monkeypatch, "shorthigh-main")
    y, (mode, took, layout, edges) = _forward(lifter, seqs, pairs, monkeypatch, depth=depth)
    assert (mode, took, layout, edges) == (1, depth, TRIMMED, False)
    assert np.array_equal(y, y0), np.abs(y - y0).max()


def test_layout_follows_the_hint(monkeypatch):
    """Unforced, on one handle with a synchronisation between calls: a batch with starts outside
    runs trimmed with its gate fired and turns the next forward wide; an in-range batch turns the
    one after it trimmed again.  The third call reads no stale edge row, the fourth no stale gate."""
    lifter, seqs = _setup()
    inr, odd = _pairs(1024), _odd_pairs()
    y_in = _old_path(lifter, seqs, inr, monkeypatch, 1024)
    y_odd = _old_path(lifter, seqs, odd, monkeypatch, "odd")
    _forward(lifter, seqs, inr, monkeypatch, trim=None)  # (whatever the handle saw before: an in-range batch last)
    seen = []
    for pairs, want in ((inr, y_in), (odd, y_odd), (inr, y_in), (inr, y_in)):
        y, (mode, took, layout, edges) = _forward(lifter, seqs, pairs, monkeypatch, trim=None)
        assert mode == 1 and took >= 1
        assert np.array_equal(y, want), np.abs(y - want).max()
        seen.append((layout, edges))
    assert seen == [(TRIMMED, False), (TRIMMED, True), (WIDE, False), (TRIMMED, False)], seen


def test_trimmed_tables_are_rebuilt_every_forward(monkeypatch):
    """No cache across calls: frames overwritten in place between two trimmed depth-2 forwards."""
    lifter, _ = _setup()
    seqs = _seqs(LENS, "reb")
    pairs = _pairs(1024)
    ya, took = _forward(lifter, seqs, pairs, monkeypatch, depth=2)
    assert took == (1, 2, TRIMMED, False)
    assert np.array_equal(ya, _old_path(lifter, seqs, pairs, monkeypatch, "reb-before"))
    lo, n = LENS[0], LENS[1]
    seqs.kps[lo:lo + n] = seqs.kps[lo:lo + n].flip(0) * 0.5
    torch.cuda.synchronize()
    yb, took = _forward(lifter, seqs, pairs, monkeypatch, depth=2)
    assert took == (1, 2, TRIMMED, False)
    y0 = _old_path(lifter, seqs, pairs, monkeypatch, "reb-after")
    assert np.array_equal(yb, y0), np.abs(yb - y0).max()
    assert not np.array_equal(yb, ya)


def test_trimmed_sequence_outside_pool_faults(monkeypatch):
    """A pair naming a sequence outside the pool still raises in the trimmed layout, and the next
    clean forward passes."""
    lifter, seqs = _setup()
    B = 1024
    for bad in ((len(LENS), 5), (-1, -7)):
        pairs = _pairs(B)
        pairs[B // 2] = bad
        pd = torch.from_numpy(pairs).cuda()
        monkeypatch.delenv("VP3D_EXPAND_TABLE", raising=False)
        monkeypatch.setenv("VP3D_FRAME_TABLES", "2")
        monkeypatch.setenv("VP3D_TABLE_TRIM", "1")
        with torch.no_grad():
            lifter.forward_windows(seqs, pd, WINDOW, LEAD, dtype="f16x3")
            torch.cuda.synchronize()
            assert lifter.frame_table_depth() == 2 and lifter.table_layout()[0] == TRIMMED
            with pytest.raises(RuntimeError, match="expand table"):
                lifter.forward_windows(seqs, pd, WINDOW, LEAD, dtype="f16x3")
        with pytest.raises(RuntimeError, match="expand table"):
            lifter.sync_status()
        lifter.sync_status()  # reported once, then cleared
        pairs = _pairs(B)
        y, took = _forward(lifter, seqs, pairs, monkeypatch, depth=2)
        assert took == (1, 2, TRIMMED, False)
        assert np.array_equal(y, _old_path(lifter, seqs, pairs, monkeypatch, B))


def test_depth_rule_of_whole_round_tables(monkeypatch):
    """Eight sequences of 2,048 frames: 8 x 2,656 = 21,248 nominal table rows are 332 tiles, at least
    one round, so the measured ratio decides: block 1 (27 rows per window) goes on the table from the
    first B with 21,248 den <= 27 B num.  One B on each side, the same bits on both."""
    lifter, _ = _setup()
    lens = (2048,) * 8
    seqs = _seqs(lens, "rule")
    _, num, den = lifter.table_depth_rule()
    rows0 = len(lens) * 2656
    b1 = -(-rows0 * den // (27 * num))  # the first B that takes level 1
    assert 27 * (b1 - 1) * num < rows0 * den <= 27 * b1 * num
    for B, want in ((b1 - 1, 0), (b1, 1)):
        pairs = _pairs(B, lens)
        y, (mode, took, layout, edges) = _forward(lifter, seqs, pairs, monkeypatch, trim=None)
        print(f"B={B}: mode {mode}, depth {took}, layout {layout}")
        assert took == want and (mode == 1 or want == 0)
        y0 = _old_path(lifter, seqs, pairs, monkeypatch, f"rule-{B}")
        assert np.array_equal(y, y0), np.abs(y - y0).max()


def test_depth_rule_below_one_round_is_the_old_factor(monkeypatch):
    """The 3-sequence pool (7,968 nominal rows, 128 tiles: less than one round) keeps the factor 2:
    27 B / 2 reaches 7,968 at B = 591 (restates tests/test_gpu_frame_tables.py's size rule)."""
    lifter, seqs = _setup()
    factor, _, _ = lifter.table_depth_rule()
    assert factor == 2
    for B, want in ((590, 0), (591, 1)):
        y, (mode, took, layout, edges) = _forward(lifter, seqs, _pairs(B), monkeypatch, trim=None)
        assert took == want and (mode == 1 or want == 0)
        assert np.array_equal(y, _old_path(lifter, seqs, _pairs(B), monkeypatch, B))
