"""Shared by the batched causal-stream tests (not collected: no test_ prefix): the seeded
per-slot sequences, the activity and reset schedule of the tracks-that-come-and-go test, and
each slot's oracle poses (oracle/stream_ref.py), computed once per run and shared read-only.

Three groups of inputs, all on top of tests/stream_cases.py:

  case table  every shape of stream_cases.CASES in a batch of 3: its sequence B, its sequence A
              (stream_cases.case_input), and B again five steps late.
  wide        (3, 3, 3) at 1024 channels, J_in = 17 and 23 (the trajectory-conditioned input),
              T = 40: the k-convs have K = 3072, six 512-wide LDS chunks, every wave of the
              workgroup with K-steps of its own; batches of 1, 16, 17 and 64 slots.  Slot r
              carries (1 + r % 3) * normalized_windows(seed + r), and one marked sequence takes
              slot MARK_AT[S] of each batch size.
  tracks      "jin21", "expand5" and "dense" in a batch of 5 over 90 global steps: slot s is
              inactive before step 4 s and whenever (g + s) % 7 == 3; slots 1 and 3 are reset at
              step 50 and from then on consume another sequence (the "A" kind: its own seed,
              three times the amplitude).
"""
import functools

import numpy as np
import torch

import stream_cases as sc
from helpers import make_model
from oracle.stream_ref import round_weights, stream_reference
from oracle.temporal_ref import geometry, lifter_forward
from vp3d_amd import synth

# ---- wide ----
WIDE_FW = (3, 3, 3)
WIDE_CHANNELS = 1024
WIDE_T = 40
WIDE_JIN = (17, 23)
WIDE_DTYPES = ("fp32", "fp16")
WIDE_S = (1, 16, 17, 64)
MARK_AT = {1: 0, 16: 0, 17: 16, 64: 63}  # the marked sequence's slot per batch size
_WIDE_SEED = {17: 700, 23: 800}
_MARK = max(WIDE_S)                      # row of the marked sequence in wide_inputs

# ---- tracks ----
TRACK_CASES = ("jin21", "expand5", "dense")
TRACK_DTYPES = ("fp16", "fp32")
TRACK_S = 5
TRACK_STEPS = 90
TRACK_RESET_STEP = 50
TRACK_RESET_SLOTS = (1, 3)


def slot_sequence(seed, name, r, T, jin):
    """Slot r's sequence: (T, jin, 2) float32."""
    x = (1 + r % 3) * synth.normalized_windows(seed + r, f"{name}/slot{r}", 1, T, n_joints=jin)[0]
    return np.ascontiguousarray(x, dtype=np.float32)


def batched_reference(sd, x, fw, dense=False, dtype=torch.float64):
    """stream_reference (oracle/stream_ref.py) of every row of x at once:
    (B, T, J_in, F) -> (B, T, J_out, 3) numpy in `dtype`."""
    x = np.asarray(x)
    pad = sum(geometry(list(fw), True, False, dense)[0])
    xp = np.concatenate([np.repeat(x[:, :1], 2 * pad, axis=1), x], axis=1)
    y = lifter_forward(sd, xp, list(fw), causal=True, dense=dense, dtype=dtype).numpy()
    assert y.shape[:2] == x.shape[:2], (y.shape, x.shape)
    return y


@functools.lru_cache(maxsize=None)
def wide_model(jin):
    """(module on the CPU in eval mode, state_dict as read-only numpy arrays)."""
    m, sd = make_model(False, WIDE_FW, causal=True, channels=WIDE_CHANNELS, jin=jin, seed=_WIDE_SEED[jin])
    for v in sd.values():
        v.setflags(write=False)
    return m, sd


@functools.lru_cache(maxsize=None)
def wide_inputs(jin):
    """(65, T, jin, 2) float32, read-only: rows 0..63 the slot sequences, row 64 the marked one."""
    name = f"wide{jin}"
    rows = [slot_sequence(_WIDE_SEED[jin], name, r, WIDE_T, jin) for r in range(_MARK)]
    rows.append(2.0 * synth.normalized_windows(_WIDE_SEED[jin] + 500, name + "/mark", 1, WIDE_T, n_joints=jin)[0])
    x = np.ascontiguousarray(np.stack(rows), dtype=np.float32)
    x.setflags(write=False)
    return x


def wide_rows(S):
    """Rows of wide_inputs / wide_oracle that the S slots of a batch carry."""
    rows = list(range(S))
    rows[MARK_AT[S]] = _MARK
    return rows


@functools.lru_cache(maxsize=None)
def wide_oracle(jin, wdtype, precision=torch.float64):
    """Oracle poses of every row of wide_inputs on the weights rounded to `wdtype`:
    (65, T, 17, 3) float64 numpy, read-only."""
    _, sd = wide_model(jin)
    rs = {k: torch.tensor(v) for k, v in round_weights(sd, wdtype).items()}
    y = batched_reference(rs, wide_inputs(jin), WIDE_FW, dtype=precision).astype(np.float64)
    y.setflags(write=False)
    return y


# ---- tracks: who consumes what, when ----
def track_active(g, s):
    return g >= 4 * s and (g + s) % 7 != 3


@functools.lru_cache(maxsize=None)
def track_plan():
    """(active, segment, index): three (TRACK_STEPS, TRACK_S) int arrays.  At global step g slot
    s consumes frame index[g, s] of its sequence number segment[g, s] (0 before its reset, 1
    after) when active[g, s], and nothing otherwise (segment / index then -1)."""
    act = np.zeros((TRACK_STEPS, TRACK_S), np.int32)
    seg = np.full((TRACK_STEPS, TRACK_S), -1, np.int32)
    idx = np.full((TRACK_STEPS, TRACK_S), -1, np.int32)
    for s in range(TRACK_S):
        n, cur = 0, 0
        for g in range(TRACK_STEPS):
            if g == TRACK_RESET_STEP and s in TRACK_RESET_SLOTS:
                n, cur = 0, 1
            if track_active(g, s):
                act[g, s], seg[g, s], idx[g, s] = 1, cur, n
                n += 1
    for a in (act, seg, idx):
        a.setflags(write=False)
    return act, seg, idx


def track_segments():
    """[(slot, segment, frames consumed)] of the schedule."""
    act, seg, _ = track_plan()
    return [(s, k, int(((seg[:, s] == k) & (act[:, s] == 1)).sum()))
            for s in range(TRACK_S) for k in ((0, 1) if s in TRACK_RESET_SLOTS else (0,))]


@functools.lru_cache(maxsize=None)
def track_sequence(name, s, segment):
    """(TRACK_STEPS, J_in, 2) float32, read-only: what slot s consumes from in `segment`."""
    c = sc.case(name)
    seed = sc._SEED[name] + 2000
    if segment == 0:
        x = slot_sequence(seed, name + "/track", s, TRACK_STEPS, c.jin)
    else:
        x = 3.0 * synth.normalized_windows(seed + 1000 + s, f"{name}/track/A{s}", 1, TRACK_STEPS, n_joints=c.jin)[0]
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def track_oracle(name, wdtype, s, segment, precision=torch.float64):
    """Oracle poses of exactly the frames slot s consumed in `segment`: (n, J_out, 3)."""
    c = sc.case(name)
    n = dict(((a, b), k) for a, b, k in track_segments())[(s, segment)]
    y = stream_reference(sc.rounded_state(name, wdtype), track_sequence(name, s, segment)[None, :n], c.fw,
                         dense=c.dense, dtype=precision).astype(np.float64)
    y.setflags(write=False)
    return y


def receptive_field(name):
    c = sc.case(name)
    return 1 + 2 * sum(geometry(list(c.fw), True, False, c.dense)[0])


def longest_layer_reach(name):
    """The largest (taps - 1) * dilation + 1 over the case's layers: with that many frames
    consumed no tap of any layer is still clamped to the stream start."""
    c = sc.case(name)
    return 1 + 2 * max(geometry(list(c.fw), True, False, c.dense)[0])
