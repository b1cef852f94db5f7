"""The index mapping of the trimmed f16x3 frame tables (plan_table_layout in csrc/vp3d_capi.cpp,
window_bases_kernel in csrc/expand_table.hip), restated in integers on the CPU.

A table row stands for the frames its value is computed from: a level-0 row for the `taps` frames
of one expand output, a level-l row for the frames of the three level l - 1 rows its k-conv reads
(the residual slice is one of them).  The trimmed layout keeps a main region per sequence for the
window starts 0 .. max_len - 1 and two edge segments per sequence, for the starts lo .. -1 and
max_len .. max_len - 1 + lead, each filled from its own pseudo-window and each self-contained at
every level.  For the 243-frame model over sequences of 300 / 517 / 2,048 frames (and of 300 /
2,000 / 2,048: a sequence shorter than max_len whose clamped starts reach the high edge segment),
every start from -600 to max_len + 600, leads 0 / 121 / 242 and depths 0 .. 3:
  - the region and base the rule assigns make every row a window reads stand for exactly the frames
    the per-frame edge clamp (generators.py:92-100) gives that window row;
  - no main-region row reads outside the main region of the level below, no edge row outside its
    own segment (every read is bounds-checked against its region's pitch while the tables are built);
  - no window's rows leave the region its base lies in.
"""
import numpy as np
import pytest

FW = (3, 3, 3, 3, 3)
WINDOW = 243
LENS = (300, 517, 2048)
# ... and a pool where a sequence shorter than max_len reaches the high edge segment: 2,000 frames with
# lead 121 / 242 clamp starts to 2,120 / 2,241 >= max_len, rows the pseudo-window (i, max_len) holds
# through its own per-frame clamp to frame 1,999
LENS_SHORT_HIGH = (300, 2000, 2048)


def _layout(lead, max_len, depth):
    """plan_expand_table's `lo`, then plan_table_layout's pitches: main / edge rows per sequence
    (segment) of levels 0 .. depth, each level losing its k-conv's reach."""
    taps = s0 = FW[0]
    rows0 = (WINDOW - taps) // s0 + 1
    span = (rows0 - 1) * s0
    lo = -(span + max(0, taps - 1 - lead))
    emax = max(-lo, lead) - 1
    pitch = [(max_len + span + 15) // 16 * 16]
    epitch = [(emax + 1 + span + 15) // 16 * 16]
    step = [s0]
    for b in range(1, depth + 1):
        reach = (FW[b] - 1) * step[-1]
        pitch.append(pitch[-1] - reach)
        epitch.append(epitch[-1] - reach)
        step.append(step[-1] * FW[b])
    return lo, rows0, pitch, epitch, step


def _region(first, n, lead, pitches, steps):
    """The rows of one pseudo-window (first start `first`, sequence of n frames) at the deepest
    level, each as the frames it stands for: level 0 by the per-frame clamp of the fill, level l
    from rows q, q + step, q + 2 step of level l - 1 -- all inside this region."""
    q = np.arange(pitches[0])
    rows = np.clip(first + q[:, None] - lead + np.arange(FW[0])[None, :], 0, n - 1)
    for l in range(1, len(pitches)):
        st, w = steps[l - 1], FW[l]
        q = np.arange(pitches[l])
        taps = q[:, None] + st * np.arange(w)[None, :]
        assert taps.max() < pitches[l - 1] == rows.shape[0]  # (the residual slice q + (w // 2) st is one of them)
        rows = rows[taps].reshape(len(q), -1)
    return rows


@pytest.mark.parametrize("depth", [0, 1, 2, 3])
@pytest.mark.parametrize("lead", [0, 121, 242])
@pytest.mark.parametrize("LENS", [LENS, LENS_SHORT_HIGH], ids=["lens300_517_2048", "lens300_2000_2048"])
def test_trimmed_regions_hold_the_clamped_frames(LENS, lead, depth):
    n_seq, max_len = len(LENS), max(LENS)
    lo, rows0, pitch, epitch, step = _layout(lead, max_len, depth)
    assert lo == (-242 if lead == 0 else -240)
    P, E, st = pitch[depth], epitch[depth], step[depth]
    edge_row0 = n_seq * pitch[0]  # the edge segments: after the level-0 main rows, in every slot
    width = int(np.prod(FW[:depth + 1]))  # frames a level-`depth` row stands for
    rows_d = rows0 // int(np.prod(FW[1:depth + 1]))  # rows of a window at that level
    # the flat table of the deepest level, as the slots hold it
    flat = np.full((edge_row0 + 2 * n_seq * epitch[0], width), -1, dtype=np.int64)
    for i, n in enumerate(LENS):
        flat[i * P:(i + 1) * P] = _region(0, n, lead, pitch, step)
        flat[edge_row0 + 2 * i * E:edge_row0 + (2 * i + 1) * E] = _region(lo, n, lead, epitch, step)
        flat[edge_row0 + (2 * i + 1) * E:edge_row0 + (2 * i + 2) * E] = _region(max_len, n, lead, epitch, step)
    starts = np.arange(-600, max_len + 601)
    j = np.arange(rows_d)
    n_main = n_low = n_high = 0
    for i, n in enumerate(LENS):
        # window_bases_kernel: the existing clamp, then the region and the base
        c = np.clip(starts, lo, n - 1 + lead)
        low, high = c < 0, c >= max_len
        base = np.where(low, edge_row0 + 2 * i * E + (c - lo),
                        np.where(high, edge_row0 + (2 * i + 1) * E + (c - max_len), i * P + c))
        idx = base[:, None] + j[None, :] * st
        # every row of a window inside the region its base lies in
        main = ~(low | high)
        assert (idx[main] // P == i).all()
        seg = (idx[~main] - edge_row0) // E
        assert (seg == (2 * i + high[~main])[:, None]).all() and (idx[~main] >= edge_row0).all()
        # ... and standing for the frames the per-frame edge clamp gives that window row
        want = np.clip(starts[:, None, None] - lead + j[None, :, None] * st + np.arange(width)[None, None, :], 0, n - 1)
        got = flat[idx]
        assert got.min() >= 0
        assert np.array_equal(got, want)
        # starts past a short sequence's end but below max_len are the main region's
        assert main[(starts >= 0) & (starts < max_len)].all()
        n_main, n_low, n_high = n_main + main.sum(), n_low + low.sum(), n_high + high.sum()
    assert n_low == n_seq * 600
    # the high segment serves the sequences with len - 1 + lead >= max_len: every start from max_len on
    # (601 here) -- the longest whenever lead > 0, the 2,000-frame one at leads 121 and 242, the
    # others clamp below max_len
    assert n_high == 601 * sum(n - 1 + lead >= max_len for n in LENS)
    assert n_high == (0 if lead == 0 else 601 * (2 if 2000 in LENS else 1))
    print(f"lead {lead} depth {depth}: lo {lo}, main pitch {P}, edge pitch {E}, step {st}; "
          f"{n_main} main / {n_low} low / {n_high} high starts")


def test_trimmed_row_counts():
    """The rows the issue's estimate rests on: max_len 2,048, lead 121 -- 2,288 / 2,282 / 2,264 /
    2,210 main rows per sequence against the wide 2,656 / 2,650 / 2,632 / 2,578, edge segments of
    480 rows at level 0 (22 % more rows than wide when the gate fires)."""
    lo, _, pitch, epitch, _ = _layout(121, 2048, 3)
    wide = (2048 - 1 + 121 - lo + 240 + 1 + 15) // 16 * 16
    assert (lo, wide) == (-240, 2656)
    assert pitch == [2288, 2282, 2264, 2210] and epitch == [480, 474, 456, 402]
    assert abs((pitch[0] + 2 * epitch[0]) / wide - 1.223) < 1e-3
