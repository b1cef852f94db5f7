"""Shared by the bf16 mixed-precision training tests (not collected: no test_ prefix): the
bf16-operand oracle, plain and teacher-forced, and the two checks of a bf16 training step.

bf16 mode (vp3d_trainer_set_compute) rounds the operands of every BLOCK conv's
three GEMMs to bf16 and accumulates in f32.  An end-to-end comparison with an oracle that rounds
the same places is not sharp: one value that lies within f32 rounding of a bf16 tie falls the
other way in another implementation and moves everything downstream by 2^-9, so the float32 and
float64 evaluations of such an oracle differ by up to 1e-2 relative in a gradient tensor while the
whole bf16 effect is 3..8e-2.  The teacher-forced oracle takes the device's rounding DECISIONS,
as the suite already takes its ReLU and dropout decisions: inside `bf16_oracle(forced=...)` the
block convs of oracle.train_ref.lifter_train_forward (the `F` that module looks up is replaced by
a shim and put back on exit) run through an autograd Function that

  forward   uses the device's operand rows (vp3d_train_read which = 0; already bf16-exact) as a
            value in place of its own input, and bf16(w) widened; its own input, rounded, is
            compared with the device rows and dropped
  backward  uses the device's gradient rows (which = 1) for gx = conv1d_input(bf16(w), g) and
            gw = conv1d_weight(x_used, g); the incoming oracle gradient, rounded, is compared and
            dropped (the gradient of a rounding is the identity)

The expand conv and the shrink (weight.shape[0] != weight.shape[1]) go to F.conv1d unchanged.
Without `forced` the shim is the plain bf16-operand oracle (its own roundings), which also records
what it rounded: the float32 run of it is the CPU stand-in for the device.
"""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

import train_cases as TC

OPERAND_SHARE_CAP = 2e-3    # share of operand elements that may differ from round_bf16(oracle float64)
STANDIN_SHARE_CAP = 1e-3    # the same share with the float32 oracle standing in for the device
# "Neighbouring bf16 values": where the rows differ they are adjacent on the bf16 grid.  An element
# formed by cancellation (a BatchNorm gradient g - mean(g) - xhat k near zero) carries the f32
# rounding error of its terms, a few 2^-24 of the rows' largest value, whatever its own size: below
# that its value, and so its bf16 cell, is not determined by any f32 evaluation (the float32 and
# float64 oracles themselves are up to 66 cells apart on one or two elements per tensor, all under
# 2e-6 of the largest value and 1e-7 of it apart).  So two rounded values that differ by at most
# 2^-20 of the rows' largest value (sixteen f32 ulps of it) count as neighbours too; they still
# count in the share.
NOISE = 2.0 ** -20

# the table rows of the teacher-forced parity test and the two full-width rows
PARITY_ROWS = ["traj_c72_causal", "w5expand_c200_1f", "c320_dilated", "dense_c136_traj", "causal_1f_c72_traj",
               "w5expand_traj_c64"]
WIDE = {
    "wide_strided_c1024": TC.Case("wide_strided_c1024", True, (3, 3, 3, 3, 3), False, False, 1024, 17, 8, 243, 0.25),
    "wide_dilated_c1024": TC.Case("wide_dilated_c1024", False, (3, 3, 3), False, False, 1024, 17, 3, 61, 0.25),
}
ALL_ROWS = PARITY_ROWS + list(WIDE)


def row(cid):
    return WIDE[cid] if cid in WIDE else TC.case(cid)


def row_state(cid):
    if cid not in WIDE:
        return TC.case_state(cid)
    return _wide_state(cid)


_wide_cache = {}


def _wide_state(cid):
    if cid not in _wide_cache:
        from helpers import make_model
        c = WIDE[cid]
        _, sd = make_model(c.strided, c.fw, causal=c.causal, channels=c.channels, jin=c.jin, dense=c.dense,
                           seed=40 + list(WIDE).index(cid))
        for v in sd.values():
            v.setflags(write=False)
        _wide_cache[cid] = sd
    return _wide_cache[cid]


def row_inputs(cid):
    if cid not in WIDE:
        return TC.case_inputs(cid)
    from vp3d_amd import synth
    c = WIDE[cid]
    x = synth.normalized_windows(6, cid, c.B, c.T, n_joints=c.jin)
    tgt = synth.normal(7, cid + "/target", (c.B, TC.layer_lengths(c)[-1], 17, 3), std=0.2).astype(np.float32)
    return x, tgt


def round_bf16(t):
    """Round to nearest even onto the bf16 grid, keeping the dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


def _ordinal(t):
    """bf16-exact values -> integers that count bf16 values in order (neighbours differ by 1)."""
    bits = (t.to(torch.float32).contiguous().view(torch.int32) >> 16) & 0xFFFF
    mag = bits & 0x7FFF
    return torch.where((bits & 0x8000) != 0, -mag, mag).to(torch.int64)


def compare_operand(kind, layer, mine, forced, report):
    """`mine`: the oracle's own (unrounded) operand; `forced`: the bf16-exact rows used instead."""
    r = round_bf16(mine.detach())
    f = forced.to(mine.dtype)
    diff = r != f
    share = float(diff.double().mean())
    scale = float(f.abs().max())
    # bf16 steps apart, over the elements that differ by more than NOISE x the rows' largest value
    # (every differing element counts in `share`)
    far_apart = diff & ((r - f).abs() > NOISE * scale)
    step = int((_ordinal(r) - _ordinal(f))[far_apart].abs().max()) if far_apart.any() else (1 if diff.any() else 0)
    far = float((mine.detach() - f).abs().max() / max(scale, 1e-30))
    report.append(dict(kind=kind, layer=layer, share=share, step=step, maxnorm=far))


class _BlockConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride, dilation, layer, st):
        forced = st["forced"]
        if forced is None:
            xu = round_bf16(x.detach())
            st["acts"][layer] = xu.clone()
        else:
            xu = forced["acts"][layer].to(x.dtype)
            assert xu.shape == x.shape, (layer, xu.shape, x.shape)
            compare_operand("act", layer, x, xu, st["report"])
        wr = round_bf16(w.detach())
        ctx.save_for_backward(xu, wr)
        ctx.meta = (stride, dilation, layer, st, tuple(w.shape))
        return F.conv1d(xu, wr, None, stride=stride, dilation=dilation)

    @staticmethod
    def backward(ctx, gz):
        xu, wr = ctx.saved_tensors
        stride, dilation, layer, st, wshape = ctx.meta
        forced = st["forced"]
        if forced is None:
            g = round_bf16(gz)
            st["grads"][layer] = g.clone()
        else:
            g = forced["grads"][layer].to(gz.dtype)
            assert g.shape == gz.shape, (layer, g.shape, gz.shape)
            compare_operand("grad", layer, gz, g, st["report"])
        gx = torch.nn.grad.conv1d_input(xu.shape, wr, g, stride=stride, dilation=dilation)
        gw = torch.nn.grad.conv1d_weight(xu, wshape, g, stride=stride, dilation=dilation)
        return gx, gw, None, None, None, None


class _Shim:
    """Stands in for torch.nn.functional inside oracle.train_ref: conv1d of a block conv goes
    through _BlockConv, everything else to torch.nn.functional."""

    def __init__(self, st):
        self._st = st

    def __getattr__(self, name):
        return getattr(F, name)

    def conv1d(self, x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
        st = self._st
        layer = st["calls"]
        st["calls"] += 1
        if w.shape[0] != w.shape[1]:  # expand conv, shrink: the f32 path in every role
            return F.conv1d(x, w, b, stride=stride, padding=padding, dilation=dilation, groups=groups)
        assert b is None and padding == 0 and groups == 1
        return _BlockConv.apply(x, w, stride, dilation, layer, st)


@contextlib.contextmanager
def bf16_oracle(forced=None):
    """Within the block, oracle.train_ref's convolutions of the block convs take bf16 operands.
    forced = dict(acts={layer: (B, C, L) tensor}, grads={layer: ...}): teacher-forced with those
    bf16-exact operands.  Yields the state: ["acts"] / ["grads"] what the plain form rounded,
    ["report"] the comparisons of the forced form (one forward + backward per block: the layer
    index is the count of conv1d calls; reset ["calls"] to 0 to run another)."""
    import oracle.train_ref as TR
    st = dict(forced=forced, acts={}, grads={}, report=[], calls=0)
    saved = TR.F
    TR.F = _Shim(st)
    try:
        yield st
    finally:
        TR.F = saved


def rows_to_cf(rows, B):
    """(B*L, C) channel-last device rows -> (B, C, L) float32 CPU tensor."""
    t = rows.detach().cpu() if isinstance(rows, torch.Tensor) else torch.as_tensor(np.asarray(rows))
    return t.reshape(B, t.shape[0] // B, t.shape[1]).permute(0, 2, 1).contiguous()


def forced_oracles(state, x, tgt, meta, p, masks, relu_masks, forced, momentum=0.1):
    """The teacher-forced oracle in float64 and float32: (o64, o32, report of the float64 run),
    o = (y, loss, grads, running stats) as train_cases._oracle returns them."""
    with bf16_oracle(forced) as st:
        o64 = TC._oracle(state, x, tgt, meta, p=p, masks=masks, dtype=torch.float64, relu_masks=relu_masks,
                         momentum=momentum)
        report = list(st["report"])
    with bf16_oracle(forced):
        o32 = TC._oracle(state, x, tgt, meta, p=p, masks=masks, relu_masks=relu_masks, momentum=momentum)
    return o64, o32, report


def check_operands(tag, report, n_block, cap=OPERAND_SHARE_CAP):
    """Check 1: every block conv's operand rows, in both roles, equal round_bf16(oracle float64
    value) but for a share <= cap of the elements, and those are neighbouring bf16 values."""
    assert len(report) == 2 * n_block, (tag, len(report), n_block)
    worst = 0.0
    for r in report:
        print(f"{tag} layer {r['layer']} {r['kind']}: differ on {r['share']:.2e}, at most {r['step']} bf16 steps, "
              f"max-norm {r['maxnorm']:.2e}")
        assert r["share"] <= cap, (tag, r)
        assert r["step"] <= 1, (tag, r)
        worst = max(worst, r["share"])
    return worst


def check_outputs(tag, got, o64, o32, stats=None):
    """Check 2: y, loss and the running statistics with the forward gates of
    test_gpu_train_shapes.py, every gradient tensor with train_cases._grad_close unchanged."""
    y, loss, grads = got
    y64, l64, g64, _ = o64
    y32, l32, g32, st32 = o32
    e = float(np.abs(np.asarray(y, np.float64) - y32).max())
    print(f"{tag}: poses {e:.2e} m, loss {abs(loss - l32) / abs(l32):.2e}")
    np.testing.assert_allclose(y, y32, atol=1e-5, rtol=0)
    np.testing.assert_allclose(loss, l32, rtol=1e-5)
    assert set(grads) == set(g64)
    worst = 0.0
    for k in grads:
        rel, _ = TC._grad_close(grads[k], g32[k], g64[k], f"{tag} {k}")
        worst = max(worst, rel)
    if stats is not None:
        for k, v in stats.items():
            if "running" in k:
                np.testing.assert_allclose(v, st32[k], rtol=1e-5, atol=1e-6, err_msg=f"{tag} {k}")
    return worst


def n_block_convs(c):
    return 2 * (len(c.fw) - 1)


def standin(cid):
    """The float32 plain bf16-operand oracle as the device (numpy dropout masks, its own ReLU
    decisions), then the teacher-forced oracles fed what it rounded: (stand-in result, o64, o32,
    report)."""
    c = row(cid)
    meta, sd = TC.meta_of(c), row_state(cid)
    x, tgt = row_inputs(cid)
    masks = TC.numpy_masks(c) if c.p > 0 else None
    with bf16_oracle() as st:
        dev = TC._oracle(sd, x, tgt, meta, p=c.p, masks=masks)
        forced = dict(acts=dict(st["acts"]), grads=dict(st["grads"]))
    o64, o32, report = forced_oracles(sd, x, tgt, meta, c.p, masks, None, forced)
    return dev, o64, o32, report
