"""The clamp-constant edge rows of the f16x3 frame tables (plan_table_edges in csrc/vp3d_capi.cpp),
restated in integers on the CPU with the model of tests/test_table_trim_geometry.py: a table row
stands for the frames its value is computed from.

A main-region row of level l >= 1 whose frames all clamp to frame 0, or all to the sequence's last
frame, stands for the same frames as its neighbour towards the sequence, so the level's convs
compute rows a_l .. b_l only and the rest are copies of rows a_l and b_l.  For the 243-frame model,
leads 0 / 121 / 242, pools of 300 / 517 / 2,048 and 300 / 2,000 / 2,048 frames, depths 1 .. 3 and
both layouts (trimmed: row 0 = start 0; wide: row 0 = start lo):
  - every row outside a_l .. b_l stands for exactly the frames of the boundary row, in every sequence;
  - in the longest sequence rows a_l + 1 and b_l - 1 do not, so the range is tight;
  - every tap and every residual read of a computed row lies inside the pitch of the level below;
  - 113 / 95 / 41 rows per side at max_len 2,048, lead 121 (the estimate of the gain rests on them).
"""
import numpy as np
import pytest

from test_table_trim_geometry import FW, LENS, LENS_SHORT_HIGH, WINDOW, _layout, _region


def table_pitches(lead, max_len, depth, trimmed):
    """(first, pitch[0 .. depth], step[0 .. depth]) of the main region: plan_table_layout's trimmed
    pitches, or plan_expand_table's wide ones (starts lo .. max_len - 1 + lead)."""
    lo, rows0, pitch, _, step = _layout(lead, max_len, depth)
    if trimmed:
        return 0, pitch, step
    span = (rows0 - 1) * FW[0]
    wide = [(max_len - 1 + lead - lo + span + 1 + 15) // 16 * 16]
    for b in range(1, depth + 1):
        wide.append(wide[-1] - (FW[b] - 1) * step[b - 1])
    return lo, wide, step


def edge_rows(lead, first, max_len, pitch, step):
    """plan_table_edges: [(a_l, b_l)] of levels 0 .. depth (level 0 keeps every row)."""
    out = [(0, pitch[0] - 1)]
    S = FW[0] - 1
    for l in range(1, len(pitch)):
        S += (FW[l] - 1) * step[l - 1]
        a = min(max(lead - first - S, 0), pitch[l] - 1)
        b = min(max(max_len - 1 + lead - first, a), pitch[l] - 1)
        out.append((a, b))
    return out


def test_frame_spans():
    """S_l of the 243-frame model: 2, 8, 26, 80."""
    _, _, step = table_pitches(121, 2048, 3, True)
    S, spans = FW[0] - 1, [FW[0] - 1]
    for l in range(1, 4):
        S += (FW[l] - 1) * step[l - 1]
        spans.append(S)
    assert spans == [2, 8, 26, 80]


@pytest.mark.parametrize("trimmed", [True, False], ids=["trimmed", "wide"])
@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("lead", [0, 121, 242])
@pytest.mark.parametrize("lens", [LENS, LENS_SHORT_HIGH], ids=["lens300_517_2048", "lens300_2000_2048"])
def test_rows_outside_the_range_are_copies(lens, lead, depth, trimmed):
    max_len = max(lens)
    first, pitch, step = table_pitches(lead, max_len, depth, trimmed)
    ab = edge_rows(lead, first, max_len, pitch, step)
    assert ab[0] == (0, pitch[0] - 1)
    for l in range(1, depth + 1):
        a, b = ab[l]
        assert 0 <= a <= b <= pitch[l] - 1
        for n in lens:
            rows = _region(first, n, lead, pitch[:l + 1], step[:l + 1])
            assert rows.shape[0] == pitch[l]
            assert (rows[:a] == rows[a]).all() and (rows[b + 1:] == rows[b]).all()
            if n == max_len:  # tight: one row further in stands for other frames
                assert a + 1 < b - 1
                assert not np.array_equal(rows[a + 1], rows[a])
                assert not np.array_equal(rows[b - 1], rows[b])
        # the computed rows' reads of the level below: taps q + k step, the residual slice among them
        taps = np.arange(a, b + 1)[:, None] + step[l - 1] * np.arange(FW[l])[None, :]
        res = np.arange(a, b + 1) + (FW[l] // 2) * step[l - 1]
        assert taps.min() >= 0 and taps.max() <= pitch[l - 1] - 1
        assert res.min() >= 0 and res.max() <= pitch[l - 1] - 1
    print(f"lead {lead} depth {depth} {'trimmed' if trimmed else 'wide'}: first {first}, pitches {pitch}, rows {ab}")


def test_edge_row_counts():
    """max_len 2,048, lead 121, trimmed pitches 2,288 / 2,282 / 2,264 / 2,210: 113 / 95 / 41 constant
    rows on either side of levels 1 / 2 / 3 -- 9.9 / 8.4 / 3.7 % of the level's rows."""
    first, pitch, step = table_pitches(121, 2048, 3, True)
    assert (first, pitch) == (0, [2288, 2282, 2264, 2210])
    ab = edge_rows(121, first, 2048, pitch, step)
    assert [a for a, _ in ab[1:]] == [113, 95, 41]
    assert [p - 1 - b for (_, b), p in zip(ab[1:], pitch[1:])] == [113, 95, 41]
    share = [round(100 * (p - (b - a + 1)) / p, 1) for (a, b), p in zip(ab[1:], pitch[1:])]
    assert share == [9.9, 8.4, 3.7]
    # one-sided windows: the 240 halo rows all on one side
    for lead in (0, 242):
        first, pitch, step = table_pitches(lead, 2048, 3, True)
        ab = edge_rows(lead, first, 2048, pitch, step)
        print(f"lead {lead}: pitches {pitch}, rows {ab}")
