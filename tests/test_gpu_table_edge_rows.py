"""The clamp-constant edge rows of the f16x3 frame tables (plan_table_edges in csrc/vp3d_capi.cpp,
VP3D_TABLE_EDGES): each level's convs compute only the main-region rows a_l .. b_l between the runs
of rows whose frames all clamp to the sequence's first / last frame -- the k-conv packed, the 1x1 +
residual out at the table's pitch (conv_gemm_a4's pitched output) -- and a copy kernel fills the
rest from rows a_l and b_l.  A replica is a copy of a row the same instruction chain computed from
the same inputs, so the poses are the same bits as with every row computed (VP3D_TABLE_EDGES=0) and
as on the per-window path (VP3D_EXPAND_TABLE=0).

The set-up of tests/test_gpu_frame_tables.py (1,024-channel config-4 model, sequences of 300 / 517
/ 2,048 frames, B = 1,024).  Every batch holds, for every sequence, the starts 0, 1, 2, len - 2 and
len - 1 -- the windows that read replica rows -- and is otherwise seeded.  The rows reported
(lifter.table_rows) are checked against the integer model of tests/test_table_edge_rows_geometry.py
together with the tile-form rule of conv_gemm_a4_x3_eligible restated below.
"""
import numpy as np
import pytest
import torch

from test_gpu_expand_table import _STATE, LENS, WINDOW, _seqs, _setup
from test_table_edge_rows_geometry import edge_rows, table_pitches

pytestmark = pytest.mark.gpu

B = 1024
TRIMMED, WIDE = 2, 1
ODD = [(0, -1), (0, -119), (0, -120), (0, -240), (0, -241), (0, -5000), (1, 517), (1, 517 + 120), (1, 517 + 121),
       (1, 517 + 400), (2, 2048 + 9000), (0, 300), (0, 420), (0, 421)]
# at lead 242 the nominal (wide) rows of LENS, 3 x 2,784 = 33 M-tiles = 132 tiles, leave the a4 tile
# forms (a last round of more than half the CUs), so plan_frame_tables takes no level whatever the
# edge rows; a longest sequence of 1,990 frames (3 x 2,720 rows = 32 M-tiles) takes them
LENS_242 = (300, 517, 1990)
_REF = {}
_SEQS = {}


def _pool(lens):
    if lens == LENS:
        return _setup()[1]
    if lens not in _SEQS:
        _SEQS[lens] = _seqs(lens, "p%d" % max(lens))
    return _SEQS[lens]


def _pairs(lens=LENS, seed=7, odd=False):
    rng = np.random.RandomState(seed)
    seq = rng.randint(0, len(lens), size=B)
    start = (rng.random_sample(B) * np.asarray(lens)[seq]).astype(np.int64)
    pairs = np.stack([seq, start], axis=-1).astype(np.int32)
    fixed = [(i, s) for i, n in enumerate(lens) for s in (0, 1, 2, n - 2, n - 1)]
    pairs[:len(fixed)] = fixed
    pairs[-len(fixed):] = fixed[::-1]
    if odd:
        pairs[100:100 + len(ODD)] = ODD
    return pairs


def _forward(lifter, seqs, pairs, lead, monkeypatch, expand=None, depth=None, trim=None, edges=None):
    for name, val in (("VP3D_EXPAND_TABLE", expand), ("VP3D_FRAME_TABLES", depth), ("VP3D_TABLE_TRIM", trim),
                      ("VP3D_TABLE_EDGES", edges)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))
    with torch.no_grad():
        y = lifter.forward_windows(seqs, torch.from_numpy(pairs).cuda(), WINDOW, lead, dtype="f16x3").cpu().numpy()
    lifter.sync_status()  # clean: no window-start, range or split fault
    return y


def _per_window(lifter, seqs, pairs, lead, monkeypatch, key):
    """The per-window path's poses of a batch, computed once per key and left unchanged."""
    if key not in _REF:
        y0 = _forward(lifter, seqs, pairs, lead, monkeypatch, expand="0")
        assert lifter.expand_table_mode() == 0 and np.isfinite(y0).all()
        y0.setflags(write=False)
        _REF[key] = y0
    return _REF[key]


def _a4_tile_forms(rows):
    """conv_gemm_a4_x3_eligible for a table launch of `rows` rows of 1,024 channels (no split
    workspace): at least 384 tiles of 256 x 256, or a last round of at most half the CUs (run as
    half-N / quarter-N tiles)."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count & ~7
    ntiles = -(-rows // 256) * 4
    last = ntiles % ncu
    return ntiles >= 384 or (last != 0 and 2 * last <= ncu and last % 4 == 0)


def _expected_rows(lens, lead, depth, layout):
    """[(first_row, rows, pitch)] of levels 0 .. depth: the model's range where the shortened
    launches keep the a4 tile forms, else every row."""
    first, pitch, step = table_pitches(lead, max(lens), depth, layout == TRIMMED)
    out = []
    for (a, b), p in zip(edge_rows(lead, first, max(lens), pitch, step), pitch):
        if (a, b) != (0, p - 1) and not _a4_tile_forms(len(lens) * (b - a + 1)):
            a, b = 0, p - 1
        out.append((a, b - a + 1, p))
    return out


def _reported(lifter):
    return [lifter.table_rows(l) for l in range(lifter.frame_table_depth() + 1)]


def _check(lifter, seqs, pairs, lens, lead, depth, trim, monkeypatch, key, want_depth=None):
    """One batch three ways: per window, every row, between the edge rows.  Returns the new form's poses."""
    y0 = _per_window(lifter, seqs, pairs, lead, monkeypatch, key)
    yf = _forward(lifter, seqs, pairs, lead, monkeypatch, depth=depth, trim=trim, edges="0")
    took_f = (lifter.expand_table_mode(), lifter.frame_table_depth(), lifter.table_layout()[0])
    full = _reported(lifter)
    assert all(a == 0 and r == p for a, r, p in full), full
    y = _forward(lifter, seqs, pairs, lead, monkeypatch, depth=depth, trim=trim, edges="1")
    took = (lifter.expand_table_mode(), lifter.frame_table_depth(), lifter.table_layout()[0])
    got = _reported(lifter)
    print(f"lead {lead} VP3D_FRAME_TABLES={depth} VP3D_TABLE_TRIM={trim}: (mode, depth, layout) {took}, rows {got}")
    assert took == took_f and took[0] == 1 and took[1] <= depth
    assert took[2] == (TRIMMED if trim == 1 else WIDE)
    if want_depth is not None:
        assert took[1] == want_depth
    assert got == _expected_rows(lens, lead, took[1], took[2])
    assert [p for _, _, p in got] == [p for _, _, p in full]
    assert np.array_equal(y, yf), np.abs(y - yf).max()
    assert np.array_equal(y, y0), np.abs(y - y0).max()
    # the default is the new form
    yd = _forward(lifter, seqs, pairs, lead, monkeypatch, depth=depth, trim=trim)
    assert _reported(lifter) == got and np.array_equal(yd, y0)
    return y


@pytest.mark.parametrize("trim", [1, 0], ids=["trimmed", "wide"])
@pytest.mark.parametrize("lead,lens", [(121, LENS), (0, LENS), (242, LENS), (242, LENS_242)],
                         ids=["lead121", "lead0", "lead242", "lead242_len1990"])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_edge_rows_bit_identical(depth, lead, lens, trim, monkeypatch):
    lifter, _ = _setup()
    # (depth 3 may be clamped by the consuming block's conditions, as in tests/test_gpu_frame_tables.py)
    want = 0 if (lead, lens) == (242, LENS) else (depth if depth < 3 else None)
    _check(lifter, _pool(lens), _pairs(lens), lens, lead, depth, trim, monkeypatch, ("in", lead, lens), want_depth=want)
    got = _reported(lifter)
    assert len(got) >= 2 or want == 0
    # rows are skipped on every side the lead leaves a halo on
    assert all(r < p for _, r, p in got[1:]), got
    if lead == 121 and trim == 1:
        assert [(a, p - a - r) for a, r, p in got[1:]] == [(113, 113), (95, 95), (41, 41)][:len(got) - 1]


@pytest.mark.parametrize("trim", [1, 0], ids=["trimmed", "wide"])
def test_edge_rows_with_starts_outside_their_sequence(trim, monkeypatch):
    """Starts before frame 0 and past the last frame: in the trimmed layout the edge gate fires and
    the gated edge segments, which keep every row, serve them; in the wide layout they read the
    main region's replica rows."""
    lifter, seqs = _setup()
    _check(lifter, seqs, _pairs(odd=True), LENS, 121, 2, trim, monkeypatch, ("odd", 121), want_depth=2)
    layout, edges = lifter.table_layout()
    assert edges and layout == (TRIMMED if trim == 1 else WIDE)


def _fresh_lifter():
    from vp3d_amd.lifter import NativeLifter
    _setup()
    m = _STATE["model"]
    return NativeLifter(m.num_joints_in, m.in_features, m.num_joints_out, m.filter_widths, m.causal, m.channels,
                        m.dense, m._variant, dict(m.state_dict()), device=torch.device("cuda"), bn_eps=m.expand_bn.eps)


def test_edge_rows_first_forward_of_a_fresh_handle(monkeypatch):
    """No forward before it has filled any row of the handle's tables: every replica row must come
    from this forward's own copy launches."""
    lifter0, seqs = _setup()
    pairs = _pairs()
    y0 = _per_window(lifter0, seqs, pairs, 121, monkeypatch, ("in", 121, LENS))
    for trim in (1, 0):
        lifter = _fresh_lifter()
        y = _forward(lifter, seqs, pairs, 121, monkeypatch, depth=2, trim=trim, edges="1")
        assert (lifter.expand_table_mode(), lifter.frame_table_depth()) == (1, 2)
        assert _reported(lifter) == _expected_rows(LENS, 121, 2, TRIMMED if trim == 1 else WIDE)
        assert np.array_equal(y, y0), np.abs(y - y0).max()


def test_edge_rows_are_copied_every_forward(monkeypatch):
    """Frames overwritten in place between two forwards (as test_frame_tables_are_rebuilt_every_forward,
    here the 517-frame and the longest sequence, whose first and last frames both change): replica
    rows left over from the earlier forward would give the old poses."""
    lifter, _ = _setup()
    seqs = _seqs(LENS, "edg")
    pairs = _pairs()
    ya = _forward(lifter, seqs, pairs, 121, monkeypatch, depth=2, trim=1, edges="1")
    assert np.array_equal(ya, _per_window(lifter, seqs, pairs, 121, monkeypatch, "edg-before"))
    for i in (1, 2):
        lo, n = sum(LENS[:i]), LENS[i]
        seqs.kps[lo:lo + n] = seqs.kps[lo:lo + n].flip(0) * 0.5
    torch.cuda.synchronize()
    yb = _forward(lifter, seqs, pairs, 121, monkeypatch, depth=2, trim=1, edges="1")
    assert (lifter.frame_table_depth(), lifter.table_layout()[0]) == (2, TRIMMED)
    assert _reported(lifter) == _expected_rows(LENS, 121, 2, TRIMMED)
    y0 = _per_window(lifter, seqs, pairs, 121, monkeypatch, "edg-after")
    assert np.array_equal(yb, y0), np.abs(yb - y0).max()
    # the windows at either end of the changed sequences moved
    ends = [k for k, (i, s) in enumerate(pairs) if i in (1, 2) and (s <= 2 or s >= LENS[i] - 2)]
    assert all(not np.array_equal(yb[k], ya[k]) for k in ends)


FALLBACK_LENS = (300, 517, 2040, 1000, 1500, 2040, 800, 1200)


def test_edge_rows_fall_back_where_the_launch_leaves_the_tile_forms(monkeypatch):
    """Eight sequences, max_len 2,040, lead 121, trimmed: level 1 would compute 2,048 of 2,282 rows
    per sequence = 16,384 rows = 256 tiles, one whole round of 256 CUs with no tail and fewer than
    384 tiles -- not a form conv_gemm_a4_x3_eligible takes -- so level 1 keeps every row (72 M-tiles,
    a half-N tail) while level 2 (2,066 rows, 65 M-tiles) is shortened.  Same poses either way."""
    lifter, _ = _setup()
    seqs = _seqs(FALLBACK_LENS, "fbk")
    pairs = _pairs(FALLBACK_LENS, seed=11)
    _check(lifter, seqs, pairs, FALLBACK_LENS, 121, 2, 1, monkeypatch, "fbk", want_depth=2)
    assert _reported(lifter) == [(0, 2288, 2288), (0, 2282, 2282), (95, 2066, 2264)]
