"""Shared by the CoupledLSTM training tests (not collected: no test_ prefix): a train-mode
oracle, the shape table of tests/test_gpu_lstm_train.py, its seeded weights and inputs, and
the gates of the training tests (tests/train_cases.py).

Oracle.  `lstm_train_forward` is CoupledLSTM.forward in train mode (reference
common/models/CamLSTM.py:98-129) as a plain torch loop over steps and cells: gate order
i, f, g, o, zero initial state, nn.LSTM's inter-layer dropout (every cell's output but the
last's, at every step) by given keep masks, bn_lstm and the head's BatchNorm1d on batch
statistics with the running-stat update, LeakyReLU(0.01) by given sides, the head's dropout by
given masks.  It is differentiable and runs in float32 or float64 on the CPU.

Mask sites, as include/vp3d.h (vp3d_seq_train_mask): 0 .. L-2 the inter-layer LSTM dropouts,
(B, T, H); then one per head layer, (B, width).

Shape table (all with dropout 0.25; csrc/seq_train.hip):

  one_tile_b5       H 128, 2 cells: lstm_train_fwd_kernel<128,32,2>, one tile with 5 of 32
                    windows; the backward's tile has 5 of 16
  tile_rem_b33      B = 33: a second forward tile and a third backward tile of one window; three
                    head layers
  no_recurrence     one cell, T = 1: no recurrent product, no LSTM dropout, B = 2, the smallest
                    batch BatchNorm takes; head 48 -> 24
  three_cells       3 cells: the generic <128,16,4> forms, W_ih of cells 1 and 2, two dropout sites
  h64_odd_head      H 64 (<64,16,4>), head width 75: odd N and K in the head kernels and in the
                    weight-gradient GEMM's scalar loaders
  window_243        the real window length: the loop bounds and the t = 0 row of h(t-1)

Weights as tests/seq_cases.py draws them but WITHOUT the x3 scale of the LSTM matrices: with
saturated gates the gradients through time vanish and a wrong backward would move nothing.
Everything derived from a row is computed once (functools.lru_cache) and must be left unchanged.
"""
import functools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import lstm_train_state
from train_cases import _grad_close, _weights_close, rel_err  # noqa: F401  (the suite's gates)
from vp3d_amd import synth

J_IN, F_IN, J_OUT, F_OUT = 17, 2, 17, 3
P_DROP = 0.25

Case = namedtuple("Case", "id H L head B T")

CASES = [
    Case("one_tile_b5", 128, 2, (128,), 5, 9),
    Case("tile_rem_b33", 128, 2, (128, 128, 128), 33, 3),
    Case("no_recurrence", 128, 1, (48, 24), 2, 1),
    Case("three_cells", 128, 3, (32,), 17, 2),
    Case("h64_odd_head", 64, 1, (75,), 3, 5),
    Case("window_243", 128, 2, (128,), 4, 243),
]
CASE_IDS = [c.id for c in CASES]


def case(cid):
    return CASES[CASE_IDS.index(cid)]


def new_module(c, dropout=P_DROP):
    from common.models.CamLSTM import CoupledLSTM
    return CoupledLSTM(J_IN, F_IN, J_OUT, F_OUT, c.H, c.L, list(c.head), dropout=dropout)


def draw_state(keys, hidden, seed):
    """state_dict (numpy) for the given {key: shape} (lstm_train_state.draw_state, which the
    golden's generator shares)."""
    return lstm_train_state.draw_state(synth, keys, hidden, seed)


@functools.lru_cache(maxsize=None)
def case_state(cid):
    c = case(cid)
    keys = {k: tuple(v.shape) for k, v in new_module(c).state_dict().items()}
    sd = draw_state(keys, c.H, 300 + CASE_IDS.index(cid))
    for v in sd.values():
        v.setflags(write=False)
    return sd


@functools.lru_cache(maxsize=None)
def case_inputs(cid):
    """(x2d (B, T, 17, 2), xcam (B, T, 3, 4), target (B, 1, 17, 3)) of a row."""
    c = case(cid)
    seed = 400 + CASE_IDS.index(cid)
    x2 = synth.normalized_windows(seed, cid, c.B, c.T)
    xc = synth.normal(seed + 1, cid + "/cam", (c.B, c.T, 3, 4), std=0.5).astype(np.float32)
    tgt = synth.normal(seed + 2, cid + "/target", (c.B, 1, J_OUT, F_OUT), std=0.2).astype(np.float32)
    for a in (x2, xc, tgt):
        a.setflags(write=False)
    return x2, xc, tgt


def site_shapes(c):
    return [(c.B, c.T, c.H)] * (c.L - 1) + [(c.B, w) for w in c.head]


def numpy_masks(c, seed=11, p=P_DROP):
    """Keep masks drawn on the CPU, one per site, for oracle-only checks."""
    rng = np.random.default_rng(seed)
    return [(rng.random(s) >= p).astype(np.uint8) for s in site_shapes(c)]


# ---- the reference's two training iterations (tests/golden/make_golden_lstm_train.py) ----
GOLDEN = "train_lstm_h64"


@functools.lru_cache(maxsize=None)
def load_golden():
    """(arrays, meta, initial state): train_lstm_h64.npz (weights, step 0) and train_lstm_h64_s1.npz
    (step 1) as one read-only dict."""
    import json
    import os
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    arrays, meta = {}, None
    for name in (GOLDEN, GOLDEN + "_s1"):
        g = np.load(os.path.join(gold, name + ".npz"), allow_pickle=False)
        meta = json.loads(str(g["meta"]))
        for k in g.files:
            if k != "meta":
                arrays[k] = g[k]
                arrays[k].setflags(write=False)
    return arrays, meta, {k[2:]: v for k, v in arrays.items() if k.startswith("w/")}


def golden_after(arrays, it):
    pre = f"s{it}/after/"
    return {k[len(pre):]: v for k, v in arrays.items() if k.startswith(pre)}


# ---- gradient gate ----------------------------------------------------------------------
def zero_grad_keys(n_head_layers, num_cells=0, T=None):
    """{key: sibling key} of the parameters whose gradient is zero by construction: a per-channel
    constant added in front of a BatchNorm on batch statistics is removed by its mean
    subtraction, so bn_lstm.bias (through the first head Linear) and the bias of every head
    Linear that a BatchNorm follows get no gradient (only the last Linear's bias does).  The
    sibling is the weight that sums the same gradient rows.  With a window of one frame (T = 1)
    every weight_hh multiplies the zero initial state only and gets none either."""
    out = {"bn_lstm.bias": "bn_lstm.weight"} if n_head_layers > 0 else {}
    if T == 1:
        for l in range(num_cells):
            out[f"lstm_layers.weight_hh_l{l}"] = f"lstm_layers.weight_ih_l{l}"
    for j in range(n_head_layers):
        out[f"mlp_layers.{4 * j}.bias"] = f"mlp_layers.{4 * j}.weight"
    return out


def grad_gate(got, g32, g64, key, n_head_layers, what, num_cells=0, T=None):
    """_grad_close (tests/train_cases.py) on every tensor with a gradient.  A relative error
    against a float64 gradient of 1e-17 says nothing, so a structurally zero tensor (zero_grad_keys)
    is gated in absolute terms instead: the float64 oracle's is below 1e-12 of its sibling's, and
    max |got| is within the gate's relative floor, 1e-4, of the sibling's largest element."""
    zeros = zero_grad_keys(n_head_layers, num_cells, T)
    if key not in zeros:
        return _grad_close(got[key], g32[key], g64[key], f"{what} {key}")
    scale = float(np.abs(g64[zeros[key]]).max())
    assert float(np.abs(g64[key]).max()) <= 1e-12 * scale, f"{what} {key}: the float64 oracle's is not zero"
    err = float(np.abs(np.asarray(got[key], np.float64)).max())
    print(f"{what} {key}: structurally zero, max|got| {err:.2e} (sibling max {scale:.2e})")
    assert err <= 1e-4 * scale, f"{what} {key}: {err:.3e} against a structural zero (sibling max {scale:.3e})"
    return None


def weights_gate(got, want, lr, key, n_head_layers, what, num_cells=0, T=None):
    """_weights_close after an Adam step.  Adam divides by the gradient's own magnitude, so a
    structurally zero gradient (rounding noise of either sign) still moves its weight by about
    lr, in a direction no two float32 implementations share: for those tensors only the bound on
    the step itself holds (|d| <= 2 lr)."""
    if key not in zero_grad_keys(n_head_layers, num_cells, T):
        return _weights_close(got, want, lr, f"{what} {key}")
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    assert d.max() <= 2 * lr + 1e-6, f"{what} {key}: {d.max():.3e}"


# ---- the oracle -------------------------------------------------------------------------
def mpjpe(pred, target):
    return torch.mean(torch.norm(pred - target, dim=len(target.shape) - 1))  # common/loss.py:11-17


def lstm_train_forward(params, x2d, xcam, hidden, num_cells, n_head_layers, p=0.0, masks=None, sides=None,
                       momenta=None, eps=1e-5):
    """params: {state_dict key: tensor} of one dtype (running statistics are updated in place).
    masks: per site a keep mask (needed when p > 0); sides: per head layer the LeakyReLU side
    (1 = BN output > 0) or None to take it from the oracle's own BN output."""
    dtype = params["bn_lstm.weight"].dtype
    B, T = x2d.shape[0], x2d.shape[1]
    x = torch.cat([torch.as_tensor(x2d).reshape(B, T, -1), torch.as_tensor(xcam).reshape(B, T, -1)], dim=2).to(dtype)
    momenta = [0.1] * (n_head_layers + 1) if momenta is None else list(momenta)
    scale = 1.0 / (1.0 - p) if p > 0 else 1.0

    def keep(site, v):
        if p <= 0:
            return v
        return v * torch.as_tensor(np.asarray(masks[site]), dtype=dtype).reshape(v.shape) * scale

    seq = [x[:, t] for t in range(T)]
    for l in range(num_cells):
        wi, wh = params[f"lstm_layers.weight_ih_l{l}"], params[f"lstm_layers.weight_hh_l{l}"]
        bi, bh = params[f"lstm_layers.bias_ih_l{l}"], params[f"lstm_layers.bias_hh_l{l}"]
        h = torch.zeros(B, hidden, dtype=dtype)
        c = torch.zeros(B, hidden, dtype=dtype)
        outs = []
        for t in range(T):
            g = F.linear(seq[t], wi, bi) + F.linear(h, wh, bh)
            i, f, gg, o = g.split(hidden, dim=1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
            h = torch.sigmoid(o) * torch.tanh(c)
            outs.append(h)
        if l < num_cells - 1 and p > 0:
            m = torch.as_tensor(np.asarray(masks[l]), dtype=dtype).reshape(B, T, hidden) * scale
            outs = [outs[t] * m[:, t] for t in range(T)]
        seq = outs
    v = F.batch_norm(seq[-1], params["bn_lstm.running_mean"], params["bn_lstm.running_var"],
                     params["bn_lstm.weight"], params["bn_lstm.bias"], True, momenta[0], eps)
    for j in range(n_head_layers):
        pre = f"mlp_layers.{4 * j}"
        bnk = f"mlp_layers.{4 * j + 1}"
        z = F.linear(v, params[pre + ".weight"], params[pre + ".bias"])
        y = F.batch_norm(z, params[bnk + ".running_mean"], params[bnk + ".running_var"], params[bnk + ".weight"],
                         params[bnk + ".bias"], True, momenta[j + 1], eps)
        if sides is not None and sides[j] is not None:
            side = torch.as_tensor(np.asarray(sides[j])).reshape(y.shape).bool()
        else:
            side = y > 0
        y = torch.where(side, y, 0.01 * y)
        v = keep(num_cells - 1 + j, y)
    last = f"mlp_layers.{4 * n_head_layers}"
    out = F.linear(v, params[last + ".weight"], params[last + ".bias"])
    return out.reshape(B, 1, -1, F_OUT)


def oracle_step(state, x2d, xcam, tgt, hidden, num_cells, n_head_layers, p=0.0, masks=None, sides=None,
                dtype=torch.float32, momenta=None):
    """Train-mode forward + mpjpe + backward in `dtype`: (y, loss, grads, running stats), numpy."""
    params = {k: torch.tensor(np.array(v), dtype=dtype) for k, v in state.items()
              if not k.endswith("num_batches_tracked")}
    for k, t in params.items():
        if "running" not in k:
            t.requires_grad_(True)
    y = lstm_train_forward(params, np.asarray(x2d), np.asarray(xcam), hidden, num_cells, n_head_layers, p=p,
                           masks=masks, sides=sides, momenta=momenta)
    loss = mpjpe(y, torch.tensor(np.asarray(tgt), dtype=dtype))
    loss.backward()
    grads = {k: t.grad.numpy() for k, t in params.items() if t.requires_grad}
    stats = {k: t.detach().numpy() for k, t in params.items() if "running" in k}
    return y.detach().numpy(), float(loss.detach()), grads, stats


def case_oracle(cid, masks, sides, dtype):
    c = case(cid)
    x2, xc, tgt = case_inputs(cid)
    return oracle_step(case_state(cid), x2, xc, tgt, c.H, c.L, len(c.head), p=P_DROP, masks=masks, sides=sides,
                       dtype=dtype)
