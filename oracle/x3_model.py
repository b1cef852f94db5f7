"""ORACLE (test infrastructure only): CPU model of the split-fp16 (`f16x3`) representation.

Follows oracle/temporal_ref.py op for op in float64, with what the native f16x3 path does to
its operands (csrc/vp3d_capi.cpp upload_weights, csrc/gemm_common.h epilogue_tp_x3) and
nothing of how it accumulates:

  activations  every stored row (the input, and each layer's output after BN, ReLU and the
               residual add) is hi = f16(a), lo = f16(a - hi); the next conv and the next
               residual read hi + lo.
  weights      W 2^e = hi + lo, both f16, e = 14 - floor(log2(max|W|)) per layer.
  product      hi*Whi + hi*Wlo + lo*Whi = conv(hi + lo, Whi + Wlo) - conv(lo, Wlo), times 2^-e
               (the lo*lo product is dropped).
  BN           scale = g / sqrt(var + eps), shift = b - mean * scale, folded in f32 as the
               host folds them.
  accumulation exact (float64): no MFMA, no f32 partial sums, no sign balancing (an exact sum
               does not care).
  shrink       in split form like every other conv (the default since round 6);
               ``shrink_f32=True`` is the exact shrink over the unsplit rows of the last block
               (VP3D_X3_SHRINK=f32).

So ``lifter_forward_x3(...) - lifter_forward(..., dtype=float64)`` is the part of the f16x3
error that the representation alone gives, at any activation scale; what the native path adds
to it is f32-sized accumulation error.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from .temporal_ref import _t, geometry


def split_f16(a: torch.Tensor):
    """(hi, lo) of the split representation, as float64 tensors: hi = f16(a), lo = f16(a - hi).
    |a| past 65,504 (rounding to f16's infinity from 65,520 on) gives hi = +-inf."""
    a = a.to(torch.float64)
    hi = a.to(torch.float16).to(torch.float64)
    lo = (a - hi).to(torch.float16).to(torch.float64)
    return hi, lo


def weight_exponent(w) -> int:
    """The per-layer power of two of the split weights: max|W 2^e| lies in [2^14, 2^15)."""
    wmax = float(np.abs(np.asarray(w, dtype=np.float32)).max())
    return 14 - int(math.floor(math.log2(wmax))) if wmax > 0.0 else 0


def split_weights(w):
    """(Whi, Wlo, e) of a conv weight: W 2^e = Whi + Wlo + (what two f16 halves cannot hold)."""
    e = weight_exponent(w)
    v = torch.from_numpy(np.ldexp(np.asarray(w, dtype=np.float32), e).astype(np.float32))
    hi, lo = split_f16(v)
    return hi, lo, e


def folded_bn(state, name, eps=1e-5):
    """(scale, shift) of an eval-mode BatchNorm, each step rounded to f32 as upload_weights does."""
    g, b, mu, var = (np.asarray(state[f"{name}.{k}"], dtype=np.float32)
                     for k in ("weight", "bias", "running_mean", "running_var"))
    invstd = np.float32(1.0) / np.sqrt(var + np.float32(eps), dtype=np.float32)
    sc = (invstd * g).astype(np.float32)
    sh = (b - (mu * sc).astype(np.float32)).astype(np.float32)
    return torch.from_numpy(sc.astype(np.float64)), torch.from_numpy(sh.astype(np.float64))


def lifter_forward_x3(state, x, filter_widths, causal=False, strided=False, dense=False,
                      eps=1e-5, shrink_f32=False, num_threads=None):
    """Eval-mode forward of TemporalModel / TemporalModelOptimized1f as the split-fp16
    representation carries it (module docstring).  x: (B, T, J, F).  Returns float64
    (B, T', J_out, 3)."""
    if num_threads is not None:
        torch.set_num_threads(num_threads)
    sd = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v))
          for k, v in state.items() if not k.endswith("num_batches_tracked")}
    xt = _t(x, torch.float64)
    B, T = xt.shape[0], xt.shape[1]
    pad, shift, convs = geometry(filter_widths, causal, strided, dense)
    w0 = filter_widths[0]

    def conv_x3(h, name, **kw):
        """h: stored rows (already hi + lo).  The three kept products, exact, scale undone."""
        whi, wlo, e = split_weights(sd[name])
        _, lo = split_f16(h)
        return (F.conv1d(h, whi + wlo, None, **kw) - F.conv1d(lo, wlo, None, **kw)) * 2.0 ** -e

    def store(a):
        hi, lo = split_f16(a)
        return hi + lo

    def bn_relu(z, name):
        sc, sh = folded_bn(sd, name, eps)
        return F.relu(z * sc[None, :, None] + sh[None, :, None])

    with torch.no_grad():
        h = store(xt.reshape(B, T, -1).permute(0, 2, 1))
        h = store(bn_relu(conv_x3(h, "expand_conv.weight", stride=w0 if strided else 1), "expand_bn"))
        for i, (k, d, s) in enumerate(convs):
            if strided:
                w = filter_widths[i + 1]
                res = h[:, :, shift[i + 1] + w // 2::w]
            else:
                p, c = pad[i + 1], shift[i + 1]
                res = h[:, :, p + c:h.shape[2] - p + c]
            h = store(bn_relu(conv_x3(h, f"layers_conv.{2 * i}.weight", stride=s, dilation=d),
                              f"layers_bn.{2 * i}"))
            h = res + bn_relu(conv_x3(h, f"layers_conv.{2 * i + 1}.weight"), f"layers_bn.{2 * i + 1}")
            if not (shrink_f32 and i == len(convs) - 1):
                h = store(h)
        bias = _t(sd["shrink.bias"], torch.float64)[None, :, None]
        if shrink_f32:
            h = F.conv1d(h, _t(sd["shrink.weight"], torch.float64), None) + bias
        else:
            h = conv_x3(h, "shrink.weight") + bias
        return h.permute(0, 2, 1).reshape(B, h.shape[2], -1, 3)


def rescale_activations(state, s: int):
    """The function-preserving rescale by k = 2^-s: every hidden activation is multiplied by k
    (exactly, in any binary floating-point format short of underflow) and the output is
    unchanged.  expand_bn weight and bias x k; every layers_bn running_mean and bias x k
    (weight and running_var untouched: the normalisation passes k through); shrink.weight / k.
    Returns a new dict of float32 arrays; `state` is left as it is."""
    k = np.float32(2.0 ** -s)
    out = {}
    for key, v in state.items():
        v = np.asarray(v)
        if key in ("expand_bn.weight", "expand_bn.bias"):
            v = v * k
        elif key.startswith("layers_bn.") and key.endswith((".running_mean", ".bias")):
            v = v * k
        elif key == "shrink.weight":
            v = v * (np.float32(1.0) / k)
        out[key] = v.copy()
    return out
