"""Shared by the training-step tests (not collected: no test_ prefix): the shape table of
tests/test_gpu_train_shapes.py, its seeded weights and inputs, and the oracle and gate helpers
of tests/test_gpu_train.py (oracle/train_ref.py in float32 / float64).

Every row trains the drop-in TemporalModel / TemporalModelOptimized1f for one step (train-mode
forward, mpjpe, backward; csrc/train.hip, csrc/vp3d_train.cpp).  The goldens and dropout cases
of test_gpu_train.py have 32, 64 or 1024 channels, 17 input joints, a 3-tap expand (K = 102,
one k-tile of the weight gradient) and dropout only on plain (3,3,3[,3,3]) models.  What each
row adds (launch_conv_gemm in csrc/conv_gemm.hip; wgrad_f32_kernel / colreduce_kernel in
csrc/train.hip; in the rows of 72, 136 and 200 channels C % 16 != 0, so no f32 conv runs on the
16-byte A loader and the shrink leaves conv_gemm_f32_narrow for the 128x128 kernel on A_PAIRS):

  traj_c72_causal     C = 72: the dilated k-convs (Ktap = 72, taps 3 and 15 rows apart, a 5-tap
                      block) and their data gradients (flipped taps over the zero-padded dZ)
                      on A_SCALAR with taps; 23 input joints: expand weight gradient K = 138
                      (a second k-tile of 10 columns, cin = 46: no 16-byte K loads, groups of
                      four columns straddle taps and the end of K); causal residual slices;
                      dropout with causal and with a width-5 block; lengths 73, 61, 61, 31, 31
  w5expand_c200_1f    strided, 5-tap expand with 17 joints (K = 170); C = 200: the weight
                      gradient's second n-tile has 72 of 128 columns; lengths 9, 3, 3, 1, 1:
                      24 rows per channel in the last block's BatchNorm, M = 24 in its GEMMs
  c320_dilated        C = 320: colreduce_kernel's second channel group (blockIdx.y = 1) has 64
                      of 256 channels, the weight gradient a third, half-full n-tile, the
                      conv GEMMs a third n-tile; C % 16 == 0, so the dilated convs stay on the
                      16-byte loader (the row test_gpu_train_shapes.py reuses across shapes)
  dense_c136_traj     --dense with dropout: contiguous 7- and 19-tap k-convs (K = 952, 2584)
                      on A_PAIRS, dgrad over dZ padded by 6 and 18 rows; 23 joints; C = 136:
                      8 columns in the weight gradient's second n-tile
  causal_1f_c72_traj  strided and causal with dropout 0.1; 48 rows per channel at the end;
                      strided dgrad as one GEMM with N = 216; K = 138 on the strided expand
  no_blocks_c64       fw = (3,): expand, BatchNorm, shrink only; M = 5 x 13 = 65 rows: two
                      reduction chunks, the second of one row, M % 4 = 1 (the reduction's and
                      the weight gradient's row tails)
  w5expand_traj_c64   5-tap expand on 23 joints: K = 230 (second k-tile of 102 columns), a
                      single block, dropout 0.  Four windows: with two, every BatchNorm sees a
                      nearly two-valued batch and the float32 oracle itself is 1.3e-6 .. 2.1e-6 m
                      and up to 6.6e-5 relative (gradients) from the float64 one on every weight
                      seed tried, over the 1e-6 m / 5e-6 that tests/test_train_cases.py asks of a
                      yardstick; with four it is 3.3e-7 m and 1.3e-6

Weights: helpers.make_model(seed = 5 + row index) (trained-like synthetic state, non-trivial
BatchNorm parameters and running statistics); inputs synth.normalized_windows(6, id, B, T, J_in),
targets synth.normal(7, id + "/target", ..., std = 0.2), as test_train_dropout_parity_with_oracle.
Everything derived from a row is computed once (functools.lru_cache) and must be left unchanged.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

from oracle.train_ref import lifter_train_forward, mpjpe as mpjpe_ref
from vp3d_amd import synth

Case = namedtuple("Case", "id strided fw causal dense channels jin B T p")

CASES = [
    Case("traj_c72_causal", False, (3, 5, 3), True, False, 72, 23, 3, 75, 0.25),
    Case("w5expand_c200_1f", True, (5, 3, 3), False, False, 200, 17, 24, 45, 0.25),
    Case("c320_dilated", False, (3, 3, 3), False, False, 320, 17, 5, 61, 0.25),
    Case("dense_c136_traj", False, (3, 3, 3), False, True, 136, 23, 4, 40, 0.25),
    Case("causal_1f_c72_traj", True, (3, 3, 3), True, False, 72, 23, 48, 27, 0.10),
    Case("no_blocks_c64", False, (3,), False, False, 64, 17, 5, 15, 0.25),
    Case("w5expand_traj_c64", False, (5, 3), False, False, 64, 23, 4, 40, 0.0),
]
CASE_IDS = [c.id for c in CASES]
# per-layer output frames (expand, then each block's k-conv and 1x1) the rows are there for
LENGTHS = {
    "traj_c72_causal": [73, 61, 61, 31, 31],
    "w5expand_c200_1f": [9, 3, 3, 1, 1],
    "c320_dilated": [59, 53, 53, 35, 35],
    "dense_c136_traj": [38, 32, 32, 14, 14],
    "causal_1f_c72_traj": [9, 3, 3, 1, 1],
    "no_blocks_c64": [13],
    "w5expand_traj_c64": [36, 26, 26],
}


def case(cid):
    return CASES[CASE_IDS.index(cid)]


def meta_of(c):
    return dict(strided=c.strided, fw=list(c.fw), causal=c.causal, dense=c.dense, channels=c.channels)


def layer_lengths(c, T=None):
    """Output frames of every conv layer but the shrink (the conv length rules of TemporalModel.py)."""
    T = c.T if T is None else T
    w0 = c.fw[0]
    L = (T - w0) // w0 + 1 if c.strided else T - (w0 - 1)
    out, dil = [L], w0
    for w in c.fw[1:]:
        L = (L - w) // w + 1 if c.strided else L - (w - 1) * dil
        out += [L, L]
        dil *= w
    assert min(out) >= 1, (c.id, T, out)
    return out


@functools.lru_cache(maxsize=None)
def case_state(cid):
    """The row's state_dict (numpy, read-only)."""
    from helpers import make_model
    c = case(cid)
    _, sd = make_model(c.strided, c.fw, causal=c.causal, channels=c.channels, jin=c.jin, dense=c.dense,
                       seed=5 + CASE_IDS.index(cid))
    for v in sd.values():
        v.setflags(write=False)
    return sd


@functools.lru_cache(maxsize=None)
def case_inputs(cid, B=None, T=None):
    """(x (B, T, J_in, 2), target (B, T_out, 17, 3)) of a row, optionally at another (B, T)."""
    c = case(cid)
    B, T = c.B if B is None else B, c.T if T is None else T
    tag = cid if (B, T) == (c.B, c.T) else f"{cid}/{B}x{T}"
    x = synth.normalized_windows(6, tag, B, T, n_joints=c.jin)
    tgt = synth.normal(7, tag + "/target", (B, layer_lengths(c, T)[-1], 17, 3), std=0.2).astype(np.float32)
    x.setflags(write=False)
    tgt.setflags(write=False)
    return x, tgt


def numpy_masks(c, seed=11, B=None, T=None):
    """Keep masks drawn on the CPU ((B*L_l, C) uint8 per layer) for oracle-only checks."""
    rng = np.random.default_rng(seed)
    B = c.B if B is None else B
    return [(rng.random((B * L, c.channels)) >= c.p).astype(np.uint8) for L in layer_lengths(c, T)]


# ---- the oracle and the gates of test_gpu_train.py ---------------------------------------
def _model(meta, state, dropout=0.0, channels=None, jin=17):
    from common.models.TemporalModel import TemporalModel, TemporalModelOptimized1f
    c = channels or meta["channels"]
    if meta["strided"]:
        m = TemporalModelOptimized1f(jin, 2, 17, meta["fw"], causal=meta["causal"], channels=c, dropout=dropout)
    else:
        m = TemporalModel(jin, 2, 17, meta["fw"], causal=meta["causal"], channels=c, dropout=dropout,
                          dense=meta["dense"])
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    return m.cuda().train()


def _oracle(state, x, tgt, meta, p=0.0, masks=None, dtype=torch.float32, relu_masks=None, momentum=0.1):
    """Oracle train-mode forward + mpjpe + backward in `dtype`: (y, loss, grads, running stats)."""
    params = {k: torch.tensor(np.array(v), dtype=dtype) for k, v in state.items()
              if not k.endswith("num_batches_tracked")}
    for k, t in params.items():
        if "running" not in k:
            t.requires_grad_(True)
    y = lifter_train_forward(params, torch.tensor(np.asarray(x), dtype=dtype), meta["fw"], causal=meta["causal"],
                             strided=meta["strided"], dense=meta["dense"], p=p, masks=masks,
                             relu_masks=relu_masks, momentum=momentum)
    loss = mpjpe_ref(y, torch.tensor(np.asarray(tgt), dtype=dtype))
    loss.backward()
    grads = {k: t.grad.numpy() for k, t in params.items() if t.requires_grad}
    stats = {k: t.detach().numpy() for k, t in params.items() if "running" in k}
    return y.detach().numpy(), float(loss.detach()), grads, stats


def rel_err(a, ref):
    """||a - ref|| / ||ref|| in float64 (the per-tensor figure of _grad_close)."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(a - ref) / max(np.linalg.norm(ref), 1e-30))


def _grad_close(got, g32, g64, what, tight=None, floor=None):
    """The suite's gradient gate.  `tight` adds a measured bound on the relative error; `floor`
    a measured floor in place of 1e-4 (rel <= max(floor, 4 x the float32 oracle's))."""
    got, g32, g64 = (np.asarray(a, dtype=np.float64) for a in (got, g32, g64))
    nrm = max(np.linalg.norm(g64), 1e-30)
    rel = np.linalg.norm(got - g64) / nrm
    ref_rel = np.linalg.norm(g32 - g64) / nrm
    err = np.abs(got - g64).max()
    print(f"{what}: rel {rel:.2e} (oracle fp32 {ref_rel:.2e}), max|d|/max|g| {err / np.abs(g64).max():.2e}")
    assert rel <= max(1e-4, 4 * ref_rel), f"{what}: relative error {rel:.3e} (oracle fp32 {ref_rel:.3e})"
    assert err <= 2e-3 * np.abs(g64).max() + 1e-30, f"{what}: max|d| {err:.3e}"
    if tight is not None:
        assert rel <= tight, f"{what}: relative error {rel:.3e} over the measured bound {tight:.1e}"
    if floor is not None:
        assert rel <= max(floor, 4 * ref_rel), f"{what}: relative error {rel:.3e} (oracle fp32 {ref_rel:.3e})"
    return float(rel), float(ref_rel)


def _weights_close(got, want, lr, what):
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    assert d.max() <= 2 * lr + 1e-6, f"{what}: {d.max():.3e}"
    assert (d <= 1e-5).mean() >= 0.999, f"{what}: {(d > 1e-5).mean():.4%} of weights off by > 1e-5"


def _masks(m, B, T, kind="dropout"):
    tr = m.native_trainer(torch.device("cuda", torch.cuda.current_device()))
    n_layers = 1 + 2 * (len(m.filter_widths) - 1)
    get = tr.dropout_mask if kind == "dropout" else tr.relu_mask
    return [get(l, m.channels).cpu().numpy() for l in range(n_layers)]


# ---- torch.optim.Adam option sets (tests/test_gpu_train.py part "Adam kernel alone") ------
# (id, optimiser keywords, tensor shapes or None for the 70-tensor list, two groups with a
# gradient missing on the second step)
ADAM_SHAPES = [(1024, 64, 3), (51, 1024, 1), (1024,), (7,), (3000,)]
ADAM_CASES = [
    ("amsgrad_off", dict(amsgrad=False), ADAM_SHAPES, False),
    ("wd_amsgrad", dict(amsgrad=True, weight_decay=1e-4), ADAM_SHAPES, False),
    ("wd_plain", dict(amsgrad=False, weight_decay=1e-4), ADAM_SHAPES, False),
    ("beta1_0p4", dict(amsgrad=True, betas=(0.4, 0.999)), ADAM_SHAPES, False),
    ("seventy_tensors", dict(amsgrad=True), None, False),   # two launches: 64 + 6
    ("steps_diverge", dict(amsgrad=True), ADAM_SHAPES, True),  # by_step splits the launch
]
ADAM_IDS = [a[0] for a in ADAM_CASES]


def adam_problem(aid):
    """(keywords, initial tensors, per-step gradients (None: no gradient), group split) of an
    Adam case, three steps, seeded."""
    _, kw, shapes, diverge = ADAM_CASES[ADAM_IDS.index(aid)]
    rng = np.random.default_rng(100 + ADAM_IDS.index(aid))
    if shapes is None:
        sizes = np.linspace(1, 3000, 70).astype(int)
        shapes = [(int(s),) for s in sizes]
    init = [rng.standard_normal(s).astype(np.float32) * 0.05 for s in shapes]
    steps = []
    for it in range(3):
        gs = [(rng.standard_normal(s) * 10.0 ** rng.integers(-6, 1)).astype(np.float32) for s in shapes]
        if diverge and it == 1:
            gs[1] = None
        steps.append(gs)
    split = 2 if diverge else len(shapes)  # tensors [0, split) in group 0, the rest in group 1
    return kw, init, steps, split


def adam_groups(tensors, split):
    groups = [dict(params=tensors[:split])]
    if split < len(tensors):
        groups.append(dict(params=tensors[split:]))
    return groups
