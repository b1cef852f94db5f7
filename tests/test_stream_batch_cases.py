"""The conditions tests/test_gpu_stream_batch.py relies on, checked with the oracle alone (CPU).

  * The oracle's own arithmetic error on the new inputs (tests/stream_batch_cases.py) -- float32
    against float64 evaluation of the same rounded weights -- is at most TOL_COORD / 20 = 1e-6 m,
    so the 2e-5 m device gate keeps 20 times headroom over the order of f32 sums.
  * The oracle poses of any two sequences that share a batch differ by at least 4e-4 m somewhere
    (the size a wrong tap or a stale slot moves a pose, tests/test_gpu_stream_shapes.py), so
    cross-talk between slots cannot hide under the gate.
  * The schedule of the tracks test lets every slot, before and after its reset, consume enough
    frames that no tap of any layer is still clamped to the stream start, and at least a whole
    receptive field wherever its windows can hold one: resets at step 50 of 90 leave at most 40
    frames per window less the inactive steps, which holds the 27 frames of "jin21" and the 9 of
    "dense" but not the 45 of "expand5" (32 frames at the least there, past its longest layer
    reach of 31).
"""
import itertools

import numpy as np
import pytest
import torch

import stream_batch_cases as bc
import stream_cases as sc
from oracle.stream_ref import stream_reference

REF_TOL = sc.TOL_COORD / 20  # metres: float32 oracle vs float64 oracle
APART = 4e-4                 # metres: two sequences of one batch


@pytest.mark.parametrize("wdtype", bc.WIDE_DTYPES)
@pytest.mark.parametrize("jin", bc.WIDE_JIN)
def test_wide_reference_is_sound_and_slots_are_apart(jin, wdtype):
    y64 = bc.wide_oracle(jin, wdtype)
    assert y64.shape == (65, bc.WIDE_T, 17, 3) and np.isfinite(y64).all()
    e = float(np.abs(bc.wide_oracle(jin, wdtype, torch.float32) - y64).max())
    print(f"wide{jin} {wdtype}: float32 oracle vs float64 max|d|={e:.3e} m")
    assert e <= REF_TOL
    flat = y64.reshape(65, -1)
    apart = min(float(np.abs(flat[a] - flat[b]).max()) for a, b in itertools.combinations(range(65), 2))
    print(f"wide{jin} {wdtype}: closest two sequences {apart:.3e} m apart")
    assert apart >= APART


def test_batched_reference_is_the_stream_reference():
    """batched_reference evaluates the rows of a batch exactly as stream_reference does one."""
    jin = bc.WIDE_JIN[0]
    _, sd = bc.wide_model(jin)
    x = bc.wide_inputs(jin)[3:4]
    one = stream_reference({k: torch.tensor(v) for k, v in sd.items()}, x, bc.WIDE_FW)
    np.testing.assert_allclose(bc.wide_oracle(jin, "fp32")[3], one, rtol=0, atol=1e-12)
    for S in bc.WIDE_S:
        rows = bc.wide_rows(S)
        assert len(rows) == S and len(set(rows)) == S and rows[bc.MARK_AT[S]] == 64


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_case_table_sequences_are_apart(name):
    c = sc.case(name)
    for wdtype in sc.DTYPES:
        a, b = sc.oracle_poses(name, wdtype, "A", c.T), sc.oracle_poses(name, wdtype)
        assert float(np.abs(a - b).max()) >= APART
        # slot 2 runs five steps behind slot 0 on the same sequence
        assert float(np.abs(b[5:] - b[:-5]).max()) >= APART


@pytest.mark.parametrize("name", bc.TRACK_CASES)
def test_track_references_are_sound_and_apart(name):
    for wdtype in bc.TRACK_DTYPES:
        ys = {}
        for s, k, n in bc.track_segments():
            y = bc.track_oracle(name, wdtype, s, k)
            assert y.shape[0] == n and np.isfinite(y).all()
            e = float(np.abs(bc.track_oracle(name, wdtype, s, k, torch.float32) - y).max())
            assert e <= REF_TOL, (s, k, e)
            ys[(s, k)] = y
        for (p, a), (q, b) in itertools.combinations(ys.items(), 2):
            n = min(len(a), len(b))
            assert float(np.abs(a[:n] - b[:n]).max()) >= APART, (p, q)


def test_track_schedule():
    act, seg, idx = bc.track_plan()
    assert act.shape == (bc.TRACK_STEPS, bc.TRACK_S)
    for g in range(bc.TRACK_STEPS):
        for s in range(bc.TRACK_S):
            assert bool(act[g, s]) == (g >= 4 * s and (g + s) % 7 != 3)
    for s in bc.TRACK_RESET_SLOTS:
        assert set(seg[:bc.TRACK_RESET_STEP, s]) <= {-1, 0} and set(seg[bc.TRACK_RESET_STEP:, s]) <= {-1, 1}
        assert idx[bc.TRACK_RESET_STEP:, s].max() < idx[:bc.TRACK_RESET_STEP, s].max() + 5  # restarted at 0
    segs = bc.track_segments()
    assert len(segs) == bc.TRACK_S + len(bc.TRACK_RESET_SLOTS)
    least = min(n for _, _, n in segs)
    assert least == 32
    for name in bc.TRACK_CASES:
        rf, reach = bc.receptive_field(name), bc.longest_layer_reach(name)
        assert least >= reach, (name, least, reach)
        if name != "expand5":  # its 45-frame field does not fit a 40-step window (module docstring)
            assert least >= rf, (name, least, rf)
    assert [bc.receptive_field(n) for n in bc.TRACK_CASES] == [27, 45, 9]
