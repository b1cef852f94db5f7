"""The f16x3 expand table (vp3d_forward_windows_pool): the expand conv computed once per resident
frame and read by block 1 through per-window row bases (VP3D_EXPAND_TABLE=1), the same table with
the windows' rows copied out of it (=copy), and the expand conv per window row (=0) are the same
bits -- every table row comes from the per-row instruction chain of the window row it replaces,
and every consumer reads the same values in the same K order.

Config-4 model (1,024 channels, 17 joints, 243-frame windows: 81 expand rows and 27 block-1 rows
per window) over three sequences of unequal length (300, 517 and 2,048 frames): the table's row
pitch comes from the longest, the edge clamps from each sequence's own length.  Every batch holds
windows starting at frame 0 and at frame len - 1 of every sequence (clamped on either side), the
same pair several times, and is otherwise seeded.  Batch sizes by the block-1 form of
conv_gemm_a4 they reach (tiles = 4 * ceil(27 B / 256) on 256 CUs):
  B = 1,024  432 whole tiles, the partial last round run whole (27 B a multiple of 256)
  B = 1,021  the same with rows past M in the last tile (B prime)
  B = 1,450  612 tiles: a half-N tail
  B = 1,300  552 tiles: a tail of <= a quarter round after whole rounds (quarter-N tiles, or the
             split-K tail where its workspace plan fits: that one keeps its own addressing, so =1
             serves it through the copy)
  B = 64     28 tiles, no whole round: quarter-N tiles; with VP3D_GEMM=q64 the fallback kernel,
             which =1 serves through the copy
"""
import numpy as np
import pytest
import torch

from helpers import make_model

pytestmark = pytest.mark.gpu

LENS = (300, 517, 2048)
WINDOW, LEAD = 243, 121
_STATE = {}


def _seqs(lens, tag):
    from vp3d_amd import synth
    from vp3d_amd.pipeline import DeviceSequences
    kps = [(synth.keypoint_tracks(11, f"{tag}{i}", n) / 1280 * 2 - np.array([1, 720 / 1280])).astype(np.float32)
           for i, n in enumerate(lens)]
    return DeviceSequences(kps, None, None, "cuda")


def _setup():
    if not _STATE:
        model, _ = make_model(True, (3, 3, 3, 3, 3), False, 1024)
        model = model.cuda()
        _STATE.update(model=model, lifter=model.native_lifter(torch.device("cuda")), seqs=_seqs(LENS, "tab"))
    return _STATE["lifter"], _STATE["seqs"]


def _pairs(B, lens=LENS):
    rng = np.random.RandomState(B)
    seq = rng.randint(0, len(lens), size=B)
    start = (rng.random_sample(B) * np.asarray(lens)[seq]).astype(np.int64)
    pairs = np.stack([seq, start], axis=-1).astype(np.int32)
    edge = [(i, s) for i, n in enumerate(lens) for s in (0, n - 1)]
    fixed = edge + [edge[-1]] * 3 + [(1, 200)] * 2  # both clamps of every sequence; repeated pairs
    assert B >= 2 * len(fixed)
    pairs[:len(fixed)] = fixed
    pairs[-len(fixed):] = fixed[::-1]
    assert (pairs[:, 1] >= 0).all() and (pairs[:, 1] < np.asarray(lens)[pairs[:, 0]]).all()
    return pairs


def _forward(lifter, seqs, pairs, monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("VP3D_EXPAND_TABLE", raising=False)
    else:
        monkeypatch.setenv("VP3D_EXPAND_TABLE", mode)
    with torch.no_grad():
        y = lifter.forward_windows(seqs, torch.from_numpy(pairs).cuda(), WINDOW, LEAD, dtype="f16x3").cpu().numpy()
    took = lifter.expand_table_mode()
    lifter.sync_status()  # clean: no window-start, range or split fault
    return y, took


# B -> the path VP3D_EXPAND_TABLE=1 takes (None: whichever the tail plan of the device gives)
@pytest.mark.parametrize("B,gemm,want", [(1024, None, 1), (1021, None, 1), (1450, None, 1), (1300, None, None),
                                         (64, None, None), (64, "q64", 2)])
def test_expand_table_bit_identical(B, gemm, want, monkeypatch):
    lifter, seqs = _setup()
    if gemm:
        monkeypatch.setenv("VP3D_GEMM", gemm)
    pairs = _pairs(B)
    y0, m0 = _forward(lifter, seqs, pairs, monkeypatch, "0")
    y1, m1 = _forward(lifter, seqs, pairs, monkeypatch, "1")
    yc, mc = _forward(lifter, seqs, pairs, monkeypatch, "copy")
    print(f"B={B} gemm={gemm}: modes 0/1/copy -> {m0}/{m1}/{mc}")
    assert y0.shape == (B, 1, 17, 3) and np.isfinite(y0).all()
    assert m0 == 0 and mc == 2 and m1 in (1, 2)
    if want is not None:
        assert m1 == want
    assert np.array_equal(yc, y0), np.abs(yc - y0).max()
    assert np.array_equal(y1, y0), np.abs(y1 - y0).max()


def test_expand_table_starts_outside_their_sequence(monkeypatch):
    """Starts before frame 0 and past the last frame -- by less and by more than a window -- are
    edge-clamped per frame on every path (generators.py:92-100): the table spans the starts that
    differ and the bases clamp the rest onto them, so the three forms stay the same bits."""
    lifter, seqs = _setup()
    B = 1024
    pairs = _pairs(B)
    odd = [(0, -1), (0, -119), (0, -120), (0, -240), (0, -241), (0, -5000), (1, 517), (1, 517 + 120), (1, 517 + 121),
           (1, 517 + 400), (2, 2048 + 9000), (0, 300), (0, 420), (0, 421)]
    pairs[100:100 + len(odd)] = odd
    y0, m0 = _forward(lifter, seqs, pairs, monkeypatch, "0")
    y1, m1 = _forward(lifter, seqs, pairs, monkeypatch, "1")
    yc, mc = _forward(lifter, seqs, pairs, monkeypatch, "copy")
    assert (m0, m1, mc) == (0, 1, 2) and np.isfinite(y0).all()
    assert np.array_equal(yc, y0), np.abs(yc - y0).max()
    assert np.array_equal(y1, y0), np.abs(y1 - y0).max()


def test_expand_table_sequence_outside_pool_faults(monkeypatch):
    """A pair naming a sequence the pool does not hold has no table rows: the table path reads
    valid rows for it and reports a fault at the next call and by sync_status."""
    lifter, seqs = _setup()
    B = 1024
    for bad in ((len(LENS), 5), (-1, 5)):
        pairs = _pairs(B)
        pairs[B // 2] = bad
        pd = torch.from_numpy(pairs).cuda()
        monkeypatch.setenv("VP3D_EXPAND_TABLE", "1")
        with torch.no_grad():
            lifter.forward_windows(seqs, pd, WINDOW, LEAD, dtype="f16x3")
            torch.cuda.synchronize()
            assert lifter.expand_table_mode() == 1
            with pytest.raises(RuntimeError, match="expand table"):
                lifter.forward_windows(seqs, pd, WINDOW, LEAD, dtype="f16x3")
        with pytest.raises(RuntimeError, match="expand table"):
            lifter.sync_status()
        lifter.sync_status()  # reported once, then cleared
        y0, m0 = _forward(lifter, seqs, _pairs(B), monkeypatch, "0")
        assert m0 == 0 and np.isfinite(y0).all()


def _t_tab(max_len):
    """Table rows per sequence: starts -240 .. max_len - 1 + LEAD, then the 240 rows a window steps over."""
    return (max_len - 1 + LEAD + 240 + 240 + 1 + 15) // 16 * 16


def test_expand_table_size_rule(monkeypatch):
    """Unforced, the path follows the sizes alone: table rows (3 sequences x 2,656 = 7,968) against
    half the window rows (81 B / 2) -- B = 196 gives 7,938, B = 197 gives 7,978."""
    lifter, seqs = _setup()
    assert len(LENS) * _t_tab(max(LENS)) == 7968
    ya, ma = _forward(lifter, seqs, _pairs(196), monkeypatch, None)
    yb, mb = _forward(lifter, seqs, _pairs(197), monkeypatch, None)
    assert ma == 0 and mb in (1, 2), (ma, mb)
    y0, _ = _forward(lifter, seqs, _pairs(197), monkeypatch, "0")
    assert np.array_equal(yb, y0)


def test_expand_table_past_2gib_takes_old_path(monkeypatch):
    """Two sequences of 262,144 frames: 2 x 262,752 table rows of 4 KB are past 2 GiB (the 32-bit
    lane offsets of the indirect rows), so the per-window path runs -- also when forced -- although
    the size rule alone (13,000 windows: 526,500 >= 525,504) would take the table."""
    lifter, _ = _setup()
    lens = (262144, 262144)
    seqs = _seqs(lens, "big")
    t_tab = _t_tab(lens[0])
    B = 13000
    assert len(lens) * t_tab * 4096 >= 2 ** 31 - 65536 and len(lens) * t_tab <= B * 81 // 2
    pairs = _pairs(B, lens)
    for mode in (None, "1"):
        y, m = _forward(lifter, seqs, pairs, monkeypatch, mode)
        assert m == 0 and np.isfinite(y).all()
