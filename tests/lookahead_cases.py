"""Shared by the look-ahead stream tests (not collected: no test_ prefix): non-causal builds of
the causal-stream fixtures (tests/stream_cases.py, tests/stream_batch_cases.py: same shapes,
seeds, weights and input sequences, causal=False), the non-causal oracle, and a float64 ring
simulation of the arrival-time scheme that csrc/stream_batch.hip's look-ahead form implements.

Oracle of a slot: TemporalModel(causal=False) in eval mode on the sequence edge-padded by P
frames on EACH side (UnchunkedGenerator, generators.py:193-198), P = the sum of the layers'
pads, through oracle.temporal_ref.lifter_forward on the weights rounded to the stream's dtype.
Everything is computed once per run and shared read-only.
"""
import functools

import numpy as np
import torch

import stream_batch_cases as bc
import stream_cases as sc
from helpers import make_model
from oracle.stream_ref import round_weights
from oracle.temporal_ref import geometry, lifter_forward
from vp3d_amd import synth

IDLE, CONSUME, DRAIN = 0, 1, 2

# ---- the real shape: receptive field 243 at 1024 channels ----
REAL_FW = (3, 3, 3, 3, 3)
REAL_CHANNELS = 1024
REAL_T = 130  # P = 121: warm-up, nine steady emissions, a 121-step drain
REAL_SEEDS = (901, 902)
REAL_DTYPES = ("fp32", "fp16")

# ---- short sequences ----
SHORT_CASES = ("jin21", "expand5")
# ---- tracks ----
TRACK_CASES = ("jin21", "dense")


def lookahead(fw, dense=False):
    """P: the sum of the layers' pads, (receptive field - 1) / 2."""
    return sum(geometry(list(fw), False, False, dense)[0])


def edge_pad(x, left, right):
    """(B, T, ...) -> (B, left + T + right, ...): copies of the first / last frame."""
    x = np.asarray(x)
    return np.concatenate([np.repeat(x[:, :1], left, axis=1), x, np.repeat(x[:, -1:], right, axis=1)], axis=1)


def noncausal_reference(sd, x, fw, dense=False, dtype=torch.float64):
    """The oracle of every row of x: (B, T, J_in, F) -> (B, T, J_out, 3) numpy in `dtype`."""
    P = lookahead(fw, dense)
    y = lifter_forward(sd, edge_pad(x, P, P), list(fw), causal=False, dense=dense, dtype=dtype).numpy()
    assert y.shape[:2] == np.asarray(x).shape[:2], (y.shape, np.asarray(x).shape)
    return y


def _frozen(sd):
    for v in sd.values():
        v.setflags(write=False)
    return sd


# ---- the case table, non-causal ----
@functools.lru_cache(maxsize=None)
def case_model(name):
    """(module on the CPU in eval mode, state_dict) of the case built with causal=False: the
    weights of stream_cases.case_model(name), which do not depend on the flag."""
    c = sc.case(name)
    m, sd = make_model(False, c.fw, causal=False, channels=c.channels, jin=c.jin, jout=c.jout, dense=c.dense,
                       seed=sc._SEED[name])
    return m, _frozen(sd)


def case_lookahead(name):
    c = sc.case(name)
    return lookahead(c.fw, c.dense)


@functools.lru_cache(maxsize=None)
def case_oracle(name, wdtype, which="B", T=None, precision=torch.float64):
    """Oracle poses of stream_cases.case_input(name, which, T): (T, J_out, 3) float64, read-only."""
    c = sc.case(name)
    y = noncausal_reference(sc.rounded_state(name, wdtype), sc.case_input(name, which, T), c.fw, c.dense,
                            precision)[0].astype(np.float64)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def sequence_oracle(name, wdtype, key, precision=torch.float64):
    """Oracle poses of a registered sequence (register_sequence): (T, J_out, 3) float64."""
    c = sc.case(name)
    y = noncausal_reference(sc.rounded_state(name, wdtype), _SEQS[key][None], c.fw, c.dense,
                            precision)[0].astype(np.float64)
    y.setflags(write=False)
    return y


_SEQS = {}


def register_sequence(key, x):
    """Keep x (T, J_in, 2) under `key` for sequence_oracle; returns it read-only."""
    if key not in _SEQS:
        x = np.ascontiguousarray(x, dtype=np.float32)
        x.setflags(write=False)
        _SEQS[key] = x
    return _SEQS[key]


# ---- wide ----
@functools.lru_cache(maxsize=None)
def wide_model(jin):
    m, sd = make_model(False, bc.WIDE_FW, causal=False, channels=bc.WIDE_CHANNELS, jin=jin, seed=bc._WIDE_SEED[jin])
    return m, _frozen(sd)


@functools.lru_cache(maxsize=None)
def wide_oracle(jin, wdtype, precision=torch.float64):
    """Oracle poses of every row of stream_batch_cases.wide_inputs: (65, T, 17, 3) float64."""
    _, sd = wide_model(jin)
    rs = {k: torch.tensor(v) for k, v in round_weights(sd, wdtype).items()}
    y = noncausal_reference(rs, bc.wide_inputs(jin), bc.WIDE_FW, dtype=precision).astype(np.float64)
    y.setflags(write=False)
    return y


# ---- real shape ----
@functools.lru_cache(maxsize=None)
def real_model():
    m, sd = make_model(False, REAL_FW, causal=False, channels=REAL_CHANNELS, seed=900)
    return m, _frozen(sd)


@functools.lru_cache(maxsize=None)
def real_inputs():
    """(2, REAL_T, 17, 2) float32, read-only: seeds 901 and 902, the second at three times the amplitude."""
    a = synth.normalized_windows(REAL_SEEDS[0], "lookahead/real0", 1, REAL_T)[0]
    b = 3.0 * synth.normalized_windows(REAL_SEEDS[1], "lookahead/real1", 1, REAL_T)[0]
    x = np.ascontiguousarray(np.stack([a, b]), dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def real_oracle(wdtype, precision=torch.float64):
    _, sd = real_model()
    rs = {k: torch.tensor(v) for k, v in round_weights(sd, wdtype).items()}
    y = noncausal_reference(rs, real_inputs(), REAL_FW, dtype=precision).astype(np.float64)
    y.setflags(write=False)
    return y


# ---- short sequences ----
def short_lengths(name):
    P = case_lookahead(name)
    return (1, 2, P, P + 1, 2 * P + 1)


def short_sequence(name, s):
    """Slot s's sequence of the short-sequence test: (short_lengths(name)[s], J_in, 2)."""
    c = sc.case(name)
    T = short_lengths(name)[s]
    return register_sequence((name, "short", s), bc.slot_sequence(sc._SEED[name] + 3000, name + "/short", s, T, c.jin))


# ---- lift_sequences: seven ragged sequences over three slots ----
LIFT_CASE = "jin21"
LIFT_DTYPES = ("fp16", "fp32")
LIFT_LENGTHS = (17, 1, 60, 2, 33, 14, 45)


def lift_sequence(i):
    """Sequence i of the lift_sequences test: (LIFT_LENGTHS[i], J_in, 2)."""
    c = sc.case(LIFT_CASE)
    return register_sequence((LIFT_CASE, "lift", i), bc.slot_sequence(sc._SEED[LIFT_CASE] + 4000, LIFT_CASE + "/lift", i,
                                                                     LIFT_LENGTHS[i], c.jin))


# ---- tracks: stream_batch_cases' activity schedule, with drains, resets and reuse ----
TRACK_S = bc.TRACK_S
TRACK_STEPS = 125
TRACK_END = {1: 30, 3: 44}  # slots 1 and 3 stop consuming segment 0 at these global steps
TRACK_LAST = 100            # nobody consumes from this global step on: everybody drains


def track_sequence(name, s, segment):
    return register_sequence((name, "track", s, segment), bc.track_sequence(name, s, segment))


@functools.lru_cache(maxsize=None)
def track_plan(name):
    """The schedule as host arrays over (TRACK_STEPS, TRACK_S): codes sent, whether the device
    is expected to take the step, the segment it belongs to, the frame index consumed (-1 if
    none) and the expected pose_frame; `resets` = {global step: [slots reset before it]}.

    Slot s is idle before step 4 s and whenever (g + s) % 7 == 3 (stream_batch_cases).  Slots 1
    and 3 stop consuming at TRACK_END[s], drain (still on that schedule) until their poses are
    out, get one stray CONSUME while drained (ignored), are reset and reused for segment 1
    while the others are mid-stream.  From TRACK_LAST on every slot drains."""
    P = case_lookahead(name)
    codes = np.zeros((TRACK_STEPS, TRACK_S), np.int32)
    takes = np.zeros((TRACK_STEPS, TRACK_S), bool)
    seg = np.full((TRACK_STEPS, TRACK_S), -1, np.int32)
    idx = np.full((TRACK_STEPS, TRACK_S), -1, np.int32)
    pf = np.full((TRACK_STEPS, TRACK_S), -1, np.int32)
    resets = {}
    for s in range(TRACK_S):
        n = t = cur = 0
        stray_sent = False
        for g in range(TRACK_STEPS):
            if not bc.track_active(g, s):
                continue
            seg[g, s] = cur
            end = TRACK_END.get(s) if cur == 0 else None
            draining = g >= TRACK_LAST or (end is not None and g >= end)
            if draining and n > 0 and t - P >= n:  # every pose is out
                if cur == 0 and s in TRACK_END:
                    if not stray_sent:
                        codes[g, s] = CONSUME  # ignored: the slot has drained and is not reset
                        stray_sent = True
                        continue
                    resets.setdefault(g, []).append(s)
                    n = t = 0
                    cur = 1
                    seg[g, s] = cur
                    draining = g >= TRACK_LAST
                else:
                    codes[g, s] = DRAIN  # a no-op
                    continue
            if draining:
                codes[g, s] = DRAIN
                if n == 0:
                    continue  # a drain of a never-fed slot: a no-op
            else:
                codes[g, s] = CONSUME
                idx[g, s] = n
                n += 1
            takes[g, s] = True
            if t >= P:
                pf[g, s] = t - P
            t += 1
    out = dict(codes=codes, takes=takes, seg=seg, idx=idx, pose_frame=pf)
    for a in out.values():
        a.setflags(write=False)
    out["resets"] = resets
    return out


def track_segments(name):
    """[(slot, segment, frames consumed)] of the schedule."""
    p = track_plan(name)
    out = []
    for s in range(TRACK_S):
        for k in (0, 1):
            n = int(((p["seg"][:, s] == k) & (p["idx"][:, s] >= 0)).sum())
            if n:
                out.append((s, k, n))
    return out


def track_oracle(name, wdtype, s, k, precision=torch.float64):
    n = dict(((a, b), c) for a, b, c in track_segments(name))[(s, k)]
    key = (name, "track-consumed", s, k)
    register_sequence(key, track_sequence(name, s, k)[:n])
    return sequence_oracle(name, wdtype, key, precision)


# ---- the scheme, in float64 with rings of the device's sizes ----
def _pow2_at_least(n):
    p = 1
    while p < n:
        p *= 2
    return p


class RingSim:
    """One slot of the look-ahead step in float64 numpy, ring for ring as the device keeps them:
    every tap and the residual read at max(t - back, 0) through a power-of-two ring of
    (taps - 1) dil + 1 slots or more, the residual `pad_b` back, the expand's raw-frame taps
    clamped at the last consumed frame while draining, emission from step P on."""

    def __init__(self, sd, fw, dense=False, eps=1e-5):
        g = lambda k: np.asarray(sd[k], dtype=np.float64)
        pad, _, convs = geometry(list(fw), False, False, dense)
        self.pad, self.P = pad, sum(pad)

        def bn(name):
            scale = g(name + ".weight") / np.sqrt(g(name + ".running_var") + eps)
            return scale, g(name + ".bias") - g(name + ".running_mean") * scale

        self.expand = (g("expand_conv.weight"), fw[0], 1) + bn("expand_bn")
        self.blocks = []
        for i, (k, d, _) in enumerate(convs):
            self.blocks.append(((g(f"layers_conv.{2 * i}.weight"), k, d) + bn(f"layers_bn.{2 * i}"),
                                (g(f"layers_conv.{2 * i + 1}.weight"),) + bn(f"layers_bn.{2 * i + 1}")))
        self.shrink = (g("shrink.weight")[:, :, 0], g("shrink.bias"))
        C, cin = self.expand[0].shape[0], self.expand[0].shape[1]
        self.rings = [np.zeros((_pow2_at_least((fw[0] - 1) + 1), cin))]
        for (kc, _) in self.blocks:
            self.rings.append(np.zeros((_pow2_at_least((kc[1] - 1) * kc[2] + 1), C)))
        self.n = self.t = 0
        self.pose = np.zeros(self.shrink[0].shape[0])

    def reset(self):
        self.n = self.t = 0

    def _conv(self, layer, ring, t, hi=None, newest=None):
        W, taps, dil, scale, shift = layer
        acc = np.zeros(W.shape[0])
        for k in range(taps):
            tt = max(t - (taps - 1 - k) * dil, 0)
            if hi is not None:
                tt = min(tt, hi)
            row = newest if (newest is not None and tt == t) else ring[tt & (len(ring) - 1)]
            acc += W[:, :, k] @ row
        return np.maximum(acc * scale + shift, 0.0)

    def step(self, code, frame=None):
        """-> pose_frame of this step (-1: no pose row written); self.pose is the slot's row."""
        n, t, P = self.n, self.t, self.P
        if code == CONSUME:
            if t != n:
                return -1
        elif code == DRAIN:
            if n == 0 or t - P >= n:
                return -1
        else:
            return -1
        if code == CONSUME:
            frame = np.asarray(frame, dtype=np.float64).reshape(-1)
            h = self._conv(self.expand, self.rings[0], t, hi=t, newest=frame)
            self.rings[0][t & (len(self.rings[0]) - 1)] = frame
        else:
            h = self._conv(self.expand, self.rings[0], t, hi=n - 1)
        for b, (kc, pw) in enumerate(self.blocks, start=1):
            ring = self.rings[b]
            ring[t & (len(ring) - 1)] = h
            y = self._conv(kc, ring, t)
            W1, scale, shift = pw
            res = ring[max(t - self.pad[b], 0) & (len(ring) - 1)]
            h = res + np.maximum((W1[:, :, 0] @ y) * scale + shift, 0.0)
        self.t += 1
        if code == CONSUME:
            self.n += 1
        if t < P:
            return -1
        self.pose = self.shrink[0] @ h + self.shrink[1]
        return t - P

    def lift(self, x):
        """Consume x (T, J_in, F), drain P steps: (T, J_out, 3)."""
        self.reset()
        out = np.zeros((len(x), self.pose.size))
        for g in range(len(x) + self.P):
            k = self.step(CONSUME, x[g]) if g < len(x) else self.step(DRAIN)
            if k >= 0:
                out[k] = self.pose
        return out.reshape(len(x), -1, 3)
