"""ORACLE (test infrastructure only): the causal streaming step's reference.

Pose k of a causal stream equals frame k of the whole-sequence causal evaluation of the
edge-padded sequence: UnchunkedGenerator puts 2*pad copies of frame 0 in front of a causal
sequence (generators.py:193-198 with causal_shift = pad) and TemporalModel(causal=True) maps
it to one pose per frame (oracle/temporal_ref.py).

The 16-bit streams keep f32 activations and round only the weights: upload_weights
(csrc/vp3d_capi.cpp) packs round-to-nearest-even fp16 / bf16 copies of the raw conv weights and
applies BatchNorm as an f32 scale and shift.  ``round_weights`` applies the same rounding to a
state_dict, so a float64 evaluation of the rounded weights is the exact value of what a 16-bit
stream computes, and the rounding itself drops out of the comparison.
"""
from __future__ import annotations

import numpy as np
import torch

from .temporal_ref import geometry, lifter_forward

_ROUND = {"fp16": torch.float16, "bf16": torch.bfloat16}


def round_weights(sd, dtype):
    """`sd` with every 3-D conv weight (the shrink's included) rounded to `dtype` ("fp16" /
    "bf16", round to nearest even) and widened back to float32; every other entry is the same
    object as in `sd`.  "fp32" returns `sd` itself."""
    if dtype == "fp32":
        return sd
    to = _ROUND[dtype]
    out = type(sd)()
    for k, v in sd.items():
        if np.ndim(v) == 3:
            t = v.detach().cpu() if isinstance(v, torch.Tensor) else torch.tensor(np.asarray(v))
            r = t.float().to(to).float()
            out[k] = r if isinstance(v, torch.Tensor) else r.numpy()
        else:
            out[k] = v
    return out


def stream_reference(sd, x, fw, dense=False, dtype=torch.float64):
    """Poses of the causal stream over x: (1, T, J_in, F) -> (T, J_out, 3) numpy in `dtype`."""
    x = np.asarray(x)
    pad = sum(geometry(list(fw), True, False, dense)[0])
    xp = np.concatenate([np.repeat(x[:, :1], 2 * pad, axis=1), x], axis=1)
    y = lifter_forward(sd, xp, list(fw), causal=True, dense=dense, dtype=dtype).numpy()[0]
    assert y.shape[0] == x.shape[1], (y.shape, x.shape)
    return y
