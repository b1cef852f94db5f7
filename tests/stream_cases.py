"""Shared by the causal-stream shape tests (not collected: no test_ prefix): the case table,
seeded builders of each case's model and input sequences, and the oracle poses
(oracle/stream_ref.py), computed once per run and shared read-only.

Every case names the branch of the host dispatch (csrc/vp3d_capi.cpp: stream_pipe_setup,
stream_persist_setup, vp3d_stream_create) or of a kernel (csrc/stream_pipe.hip,
csrc/stream_persist.hip, csrc/stream_step.hip) it is there for, and pins the form the dispatch
must choose on the 256-CU MI355X.  The forms follow from the setup functions:

  pipe     C in {256, 1024}, a 3-tap expand of Kp <= kPipeExpandK = 128 (Kp = 3 J_in F rounded
           up to 64), every block a dilated 3-tap k-conv, the roles fit the CUs and the LDS
           fits 160 KB; any weight dtype.
  persist  16-bit weights only; a 3-tap expand, at least one block, every block dilated
           (Ktap == C) with at most kStreamMaxTaps = 8 taps, CPW = ceil(C / 256) <= 4 channels
           per workgroup and the outputs fit the G = C / CPW workgroups.
  launches everything else.

VP3D_STREAM_MODE unset or "pipe": pipe, else persist, else launches.  "persist": persist, else
launches.  "launches": launches.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

from helpers import make_model
from oracle.stream_ref import round_weights, stream_reference
from vp3d_amd import synth

MODES = (None, "launches", "persist", "pipe")  # VP3D_STREAM_MODE values, None = unset
DTYPES = ("fp32", "fp16", "bf16")

L, S, P = "launches", "persist", "pipe"

# forms16 / forms32: the form expected with fp16 / bf16 weights and with fp32 weights, in the
# order of MODES (unset, launches, persist, pipe)
Case = namedtuple("Case", "name fw channels jin jout dense T forms16 forms32")

_ALL_L = (L, L, L, L)
_PERSIST16 = (S, L, S, S)          # no pipe; the LDS-resident form for 16-bit weights
_PIPE16 = (P, L, S, P)             # pipe; VP3D_STREAM_MODE=persist still has its own form
_PIPE32 = (P, L, L, P)             # fp32 has no persist form

CASES = [
    # nb == 0: the expand writes xlast directly, the shrink reads a plain vector
    Case("one_width", (3,), 64, 17, 17, False, 100, _ALL_L, _ALL_L),
    # a 1-tap expand (ring of one slot) and a block of dilation 1 (Ktap = 3 C): both persistent
    # forms refuse the expand
    Case("expand1", (1, 3), 64, 17, 17, False, 100, _ALL_L, _ALL_L),
    # persist at CPW = 1, G = 64 workgroups, 51 outputs on 51 of them
    Case("persist_c64", (3, 3), 64, 17, 17, False, 100, _PERSIST16, _ALL_L),
    # the dense ablation: 7 adjacent taps, dilation 1, Ktap = 7 C != C
    Case("dense", (3, 3), 64, 17, 17, True, 100, _ALL_L, _ALL_L),
    # a 5-tap expand (frame ring of 8 slots)
    Case("expand5", (5, 3, 3), 128, 17, 17, False, 100, _ALL_L, _ALL_L),
    # 7 dilated taps in the persist form's scatter ring (dilation 3, ring 32; then dilation 21)
    Case("width7", (3, 7, 3), 128, 17, 17, False, 100, _PERSIST16, _ALL_L),
    # 9 taps > kStreamMaxTaps
    Case("width9", (3, 9), 64, 17, 17, False, 100, _ALL_L, _ALL_L),
    # persist at CPW = 2 on all 256 CUs
    Case("c512", (3, 3, 3), 512, 17, 17, False, 100, _PERSIST16, _ALL_L),
    # 51 outputs > G = 32 workgroups
    Case("c32", (3, 3, 3), 32, 17, 17, False, 100, _ALL_L, _ALL_L),
    # pipe at K = 126 of Kp = 128: two padded LDS elements times two zero weights
    Case("jin21", (3, 3, 3), 256, 21, 17, False, 100, _PIPE16, _PIPE32),
    # K = 132, Kp = 192 > kPipeExpandK: out of the pipe
    Case("jin22", (3, 3, 3), 256, 22, 17, False, 100, _PERSIST16, _ALL_L),
    # the 46-channel trajectory input (K = 138, Kp = 192)
    Case("traj", (3, 3, 3), 256, 23, 17, False, 100, _PERSIST16, _ALL_L),
    # 96 outputs: 6 shrink workgroups in the pipe, no folded shrink when serving
    Case("jout32", (3, 3, 3), 256, 17, 32, False, 100, _PIPE16, _PIPE32),
    # 3 outputs: one shrink workgroup, 3 of its 64 rows valid
    Case("jout1", (3, 3, 3), 256, 17, 1, False, 100, _PIPE16, _PIPE32),
    # dilation 243, ring of 512 slots (T = 560 wraps it); the pipe's LDS is 60,688 bytes
    # (8 waves x 512 slots x 3 rows of partial sums) and its roles take 225 of the 256 CUs
    Case("deep6", (3, 3, 3, 3, 3, 3), 256, 17, 17, False, 560, _PIPE16, _PIPE32),
]
CASE_NAMES = [c.name for c in CASES]
_BY_NAME = {c.name: c for c in CASES}
_SEED = {c.name: 200 + i for i, c in enumerate(CASES)}

# vp3d_stream_create refuses K > 4096 per layer: the 5-tap k-conv at 1024 channels has K = 5120
REFUSED = dict(fw=(3, 5, 3), channels=1024, match="K <= 4096")

# the project's fp32 stream gates (tests/test_gpu_stream.py), applied to every dtype against the
# float64 oracle on that dtype's rounded weights
TOL_COORD = 2e-5   # metres per coordinate
TOL_DMPJPE = 1e-7  # metres


def case(name):
    return _BY_NAME[name]


def expected_form(name, dtype, mode):
    c = _BY_NAME[name]
    return (c.forms32 if dtype == "fp32" else c.forms16)[MODES.index(mode)]


@functools.lru_cache(maxsize=None)
def case_model(name):
    """(module on the CPU in eval mode, state_dict as read-only numpy arrays) of a case."""
    c = _BY_NAME[name]
    m, sd = make_model(False, c.fw, causal=True, channels=c.channels, jin=c.jin, jout=c.jout, dense=c.dense,
                       seed=_SEED[name])
    for v in sd.values():
        v.setflags(write=False)
    return m, sd


@functools.lru_cache(maxsize=None)
def case_input(name, which="B", T=None):
    """(1, T, J_in, 2) float32, read-only.  "B" is the case's sequence (T = the case's length);
    "A" is another one -- its own seed, three times the amplitude -- whose history would show
    in B's poses if a reset or a second stream let it through."""
    c = _BY_NAME[name]
    T = c.T if T is None else T
    if which == "B":
        x = synth.normalized_windows(_SEED[name], name, 1, T, n_joints=c.jin)
    else:
        x = 3.0 * synth.normalized_windows(_SEED[name] + 1000, name + "/A", 1, T, n_joints=c.jin)
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def rounded_state(name, wdtype):
    """The case's state_dict with its conv weights rounded to `wdtype`, as float32 tensors."""
    _, sd = case_model(name)
    return {k: torch.tensor(v) for k, v in round_weights(sd, wdtype).items()}


@functools.lru_cache(maxsize=None)
def oracle_poses(name, wdtype, which="B", T=None, precision=torch.float64):
    """stream_reference of the case's weights rounded to `wdtype`, evaluated in `precision`:
    (T, J_out, 3) float64 numpy, read-only."""
    c = _BY_NAME[name]
    y = stream_reference(rounded_state(name, wdtype), case_input(name, which, T), c.fw, dense=c.dense,
                         dtype=precision).astype(np.float64)
    y.setflags(write=False)
    return y


def reference_error(name, wdtype):
    """max |float32 oracle - float64 oracle| over every coordinate: the yardstick."""
    return float(np.abs(oracle_poses(name, wdtype, precision=torch.float32) - oracle_poses(name, wdtype)).max())


def dmpjpe(out, ref, seed=3):
    """|MPJPE(out, gt) - MPJPE(ref, gt)| in metres against a seeded random ground truth."""
    gt = np.random.default_rng(seed).normal(0.0, 0.2, ref.shape)
    m = lambda p: float(np.linalg.norm(np.asarray(p, dtype=np.float64) - gt, axis=-1).mean())
    return abs(m(out) - m(ref))
