"""Choosing the f16x3 activation pre-scale from calibration statistics (pure Python, no device).

The split-fp16 path stores every activation as hi = f16(a), lo = f16(a - hi); lo is an f16
subnormal for |a| < 2^-3, so small activations lose accuracy.  Layer l's stored
rows may instead hold a * 2^p[l] (include/vp3d.h ``vp3d_set_x3_prescale``); this module picks
the exponents from the per-layer statistics ``NativeLifter.calibrate_x3`` returns.

Layer order: 0 = the expand conv's output, then for block b = 1, 2, ...: 2b - 1 = its k-conv's
output, 2b = its 1x1's output (after the residual add).  The residual add joins layers
0, 2, 4, ... ("the chain"), which therefore share one exponent.
"""
from __future__ import annotations

import math
from typing import List, Sequence

#: the f16 range guard's limit is 65,504 < 2^16
RANGE_BITS = 16
#: |p| bound of vp3d_set_x3_prescale (include/vp3d.h VP3D_X3_PRESCALE_MAX)
PRESCALE_MAX = 24


def n_prescale_layers(filter_widths: Sequence[int]) -> int:
    """Conv layer outputs that carry an exponent: the expand and two per block (not the shrink)."""
    return 1 + 2 * (len(filter_widths) - 1)


def chain_layers(filter_widths: Sequence[int]) -> List[int]:
    """The layers a residual add joins: the expand output and every block's 1x1 output."""
    return list(range(0, n_prescale_layers(filter_widths), 2))


def _absmax(stat) -> float:
    return float(stat["absmax"] if isinstance(stat, dict) else stat[0])


def exponent_for(absmax: float, headroom_bits: int = 6) -> int:
    """The largest p with absmax * 2^p < 2^(16 - headroom_bits), clamped to +-PRESCALE_MAX;
    0 for a zero or non-finite absmax (nothing to scale, or nothing to trust)."""
    if not math.isfinite(absmax) or absmax <= 0.0:
        return 0
    # absmax = m 2^e with m in [0.5, 1): m 2^(e + p) < 2^L exactly when e + p <= L
    _, e = math.frexp(absmax)
    p = RANGE_BITS - int(headroom_bits) - e
    return max(-PRESCALE_MAX, min(PRESCALE_MAX, p))


def choose_prescale(stats, geometry: Sequence[int], headroom_bits: int = 6) -> List[int]:
    """Exponents for ``set_x3_prescale`` from per-layer statistics.

    stats: one entry per conv layer output, each a dict with an ``absmax`` key or a tuple
    starting with it.  geometry: the model's ``filter_widths``.  The chain exponent follows the
    largest absmax over the chain layers, each k-conv output its own; a chain with a non-finite
    absmax, or all zeros, gets 0.  headroom_bits = 6 keeps a x32 input window under the range
    guard with a factor 2 to spare."""
    n = n_prescale_layers(geometry)
    if len(stats) != n:
        raise ValueError(f"expected statistics of {n} layers for filter_widths {list(geometry)}, got {len(stats)}")
    amax = [_absmax(s) for s in stats]
    chain = chain_layers(geometry)
    chain_vals = [amax[l] for l in chain]
    if any(not math.isfinite(v) for v in chain_vals):
        p_chain = 0
    else:
        p_chain = exponent_for(max(chain_vals), headroom_bits)
    out = [exponent_for(a, headroom_bits) for a in amax]
    for l in chain:
        out[l] = p_chain
    return out


def check_prescale(p: Sequence[int], geometry: Sequence[int]) -> List[int]:
    """The checks of vp3d_set_x3_prescale that need no device; returns the exponents as ints."""
    n = n_prescale_layers(geometry)
    p = [int(v) for v in p]
    if len(p) != n:
        raise ValueError(f"f16x3 pre-scale: expected {n} exponents (one per conv layer output, none for the "
                         f"shrink), got {len(p)}")
    for l, v in enumerate(p):
        if abs(v) > PRESCALE_MAX:
            raise ValueError(f"f16x3 pre-scale: layer {l} has exponent {v}, past +-{PRESCALE_MAX}")
    for l in chain_layers(geometry):
        if p[l] != p[0]:
            raise ValueError(f"f16x3 pre-scale: layer {l} (a block's 1x1 output) has exponent {p[l]} but the "
                             f"residual chain (layer 0) has {p[0]}; the layers a residual add joins share one")
    return p
