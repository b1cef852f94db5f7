"""Shared by the trajectory-lifter shape tests (not collected: no test_ prefix): the case
tables, a seeded builder of model state and inputs, and the float64 / float32 oracle outputs
(oracle/seq_lifter_ref.py), computed once per run and shared read-only.

State.  torch's default initialisation leaves every LayerNorm at gamma = 1, beta = 0 and every
attention bias at 0, and makes attention nearly uniform; a wrong gamma index, a dropped bias or
a softmax that mishandles its maximum or key mask would then move nothing.  So every tensor is
drawn from vp3d_amd.synth:
  matrices                    U(+-1/sqrt(fan_in)) (in_proj_weight: torch's xavier bound)
  LayerNorm / BatchNorm gamma U(0.5, 1.5)
  LayerNorm beta, every Linear / attention / LSTM bias   N(0, 0.1)
  BatchNorm beta, mean, var   U(+-0.1), U(+-0.2), U(0.5, 2) (as tests/golden/make_golden.py)
and two scalings make the non-linear parts count: the q and k rows of every in_proj_weight
times 3 (peaked softmax rows; times 6 with one head makes them one-hot, which hides errors
again), the LSTM weight matrices times 3 (saturating gates).
"""
import functools
import math

import numpy as np
import torch

from oracle.seq_lifter_ref import lstm_forward, sliding_windows, transformer_forward
from vp3d_amd import synth

J_IN, F_IN, J_OUT, F_OUT = 17, 2, 17, 3

# (name, (d_model, n_heads, num_layers, dim_feedforward, head_layers), [(mode, W, n)]):
# mode "fwd": n windows of W frames; mode "slide": sliding_window over one sequence of n frames.
# The comments name the dispatch branches of launch_attention / launch_layernorm_rows /
# launch_conv_gemm (csrc/seq_lifter.hip, csrc/conv_gemm.hip) each case is there for.
TRANSFORMER_CASES = [
    # the run.py defaults at an odd frame count (5 x 243 = 1215, and 259): the frame buffer is
    # n_frames x 46 floats, so every workspace buffer behind it starts 8 bytes off a 16-byte
    # boundary unless run() rounds it; mfma<32>, last<32>, LayerNorm vec<32> with all lanes
    # valid, W = 243 (16 key blocks, 3 keys in the last); 17 overlapping windows share P
    ("t1_defaults_odd_frames", (128, 4, 2, 128, (128, 128, 128)), [("fwd", 243, 5), ("slide", 243, 259)]),
    # head dim 16: mfma<16> twice, last<16>; d = 96: LayerNorm vec<32> with 24 valid lanes and
    # K = 96 < Kp = 128 on the 16-byte A loader; W = 17: two key blocks, one valid key in the
    # second; ff = 72 (A_PAIRS, K % 16 = 8), head 80 -> 40 (the narrow kernel at N = 40, K = 80,
    # then K = 40 on A_PAIRS); odd (85) and even (68) frame counts
    ("t2_d96_h6_dh16", (96, 6, 3, 72, (80, 40)), [("fwd", 17, 5), ("fwd", 17, 4)]),
    # head dim 64: the scalar attention_kernel<64>; one layer: last query only (last_only on the
    # scalar kernel); head width 75: N = 75 on the scalar epilogue, then K = lda = 75 on A_SCALAR,
    # the second head buffer at an odd offset (3 x 75 floats): the last LayerNorm writes there
    # and takes the alignment fallback; ff = 200 (A_PAIRS)
    ("t3_dh64_one_layer_odd_head", (64, 1, 1, 200, (75,)), [("fwd", 33, 3)]),
    # the largest window of head dim 64: 2 W dh 4 = 64 KiB of dynamic LDS exactly
    ("t4_dh64_w128", (64, 1, 2, 64, (64,)), [("fwd", 128, 2)]),
    # 20 heads: the last layer on the scalar kernel with last_only (attention_last takes <= 16);
    # d = 320 > 256: the one-wave-per-row LayerNorm (per = 5); W = ATT_WMAX = 256, 16 full key blocks
    ("t5_d320_h20_w256", (320, 20, 2, 128, (128,)), [("fwd", 256, 2)]),
    # 16 heads: attention_last_kernel<32> at 1,024 threads; d = 512: per = 8; W = 100: 7 key
    # blocks (odd), 4 keys in the last
    ("t6_d512_h16", (512, 16, 2, 256, (128,)), [("fwd", 100, 3)]),
    # d = 1024: per = 16 (the LayerNorm's register row full), N = 3072 in the QKV GEMM, ff < d;
    # head dim 64 with 16 heads; W = 40
    ("t7_d1024_h16", (1024, 16, 2, 64, (128,)), [("fwd", 40, 2)]),
    # W = 300 > 256: both attention calls on the scalar kernel (<16>, full and last_only)
    ("t8_w300_scalar", (64, 4, 2, 64, (64,)), [("fwd", 300, 2)]),
    # window family on mfma<16> / last<16>: W = 1 and 15 (one block, clamped query rows), 16 and
    # 48 (W % 16 == 0; 48: an odd block count, the pass's second block all masked), 33 (W % 16
    # != 0, odd count); sliding_window with a single window (L = W = 33)
    ("t9_window_family", (64, 4, 2, 64, (64,)),
     [("fwd", 1, 3), ("fwd", 15, 3), ("fwd", 16, 3), ("fwd", 33, 3), ("fwd", 48, 3), ("slide", 33, 33)]),
]

# (name, (hidden, num_cells, head_layers), [(mode, W, n)]); launch_lstm's branches:
LSTM_CASES = [
    # lstm_kernel<128,32,2> with one cell; one tile, 5 of 32 windows valid
    ("l1_h128_c1", (128, 1, (128,)), [("fwd", 243, 5)]),
    # the run.py defaults: <128,32,2>, two tiles, the second with one window; sliding_window
    # (17 windows sharing the per-frame input projection, an odd frame count)
    ("l2_defaults", (128, 2, (128, 128, 128)), [("fwd", 243, 33), ("slide", 243, 259)]),
    # three cells: lstm_kernel<128,16,4>; bias[2] / wih_t[2] first used; two tiles, one window in
    # the second
    ("l3_h128_c3", (128, 3, (128,)), [("fwd", 243, 17)]),
    # four cells, head width 200 > H (the head buffers' pitch), three tiles
    ("l4_h128_c4", (128, 4, (200,)), [("fwd", 27, 33)]),
    # lstm_kernel<64,16,4> with one cell, one window of one frame; head width 75 (odd N and K)
    ("l5_h64_c1_w1", (64, 1, (75,)), [("fwd", 1, 1)]),
    # H = 64, four cells, head 100 -> 30 (A_PAIRS at K = 100 and 30, N = 30)
    ("l6_h64_c4", (64, 4, (100, 30)), [("fwd", 50, 17)]),
    # H = 64, two cells, W = 2, exactly one full tile
    ("l7_h64_c2_w2", (64, 2, (64,)), [("fwd", 2, 16)]),
]

# one entry per (case, run): (id, kind, case name, cfg, mode, W, n)
RUNS = []
for _kind, _table in (("transformer", TRANSFORMER_CASES), ("lstm", LSTM_CASES)):
    for _name, _cfg, _runs in _table:
        for _mode, _W, _n in _runs:
            RUNS.append((f"{_name}-{_mode}-W{_W}-n{_n}", _kind, _name, _cfg, _mode, _W, _n))
RUN_IDS = [r[0] for r in RUNS]
_SEED = {name: 100 + i for i, (name, _, _) in enumerate(TRANSFORMER_CASES + LSTM_CASES)}


def new_module(kind, cfg):
    """The drop-in module of a case on the CPU, as constructed (torch's default init)."""
    if kind == "transformer":
        from common.models.CamTransformer import CoupledTransformer
        d, heads, layers, ff, head = cfg
        return CoupledTransformer(J_IN, F_IN, J_OUT, F_OUT, d, layers, heads, ff, list(head))
    from common.models.CamLSTM import CoupledLSTM
    hidden, cells, head = cfg
    return CoupledLSTM(J_IN, F_IN, J_OUT, F_OUT, hidden, cells, list(head))


@functools.lru_cache(maxsize=None)
def case_state(kind, name, cfg):
    """state_dict (numpy, read-only) of a case, every tensor but the sinusoid table drawn from
    synth as the module docstring says."""
    seed = _SEED[name]
    keys = {k: tuple(v.shape) for k, v in new_module(kind, cfg).state_dict().items()}
    sd = {}
    for k, shape in keys.items():
        def u(lo, hi):
            return synth.uniform(seed, k, shape, lo, hi).astype(np.float32)
        if k == "positional_encoding.pe" or k.endswith("num_batches_tracked"):
            continue
        bn = k.rsplit(".", 1)[0] + ".running_mean" in keys
        if len(shape) == 2:
            if k.endswith("in_proj_weight"):
                b = math.sqrt(6.0 / (shape[0] + shape[1]))
            elif k.startswith("lstm_layers."):
                b = 1.0 / math.sqrt(cfg[0])
            else:
                b = 1.0 / math.sqrt(shape[1])
            w = u(-b, b)
            if k.endswith("in_proj_weight"):
                w[:2 * shape[1]] *= 3.0
            elif k.startswith("lstm_layers."):
                w *= 3.0
            sd[k] = w
        elif k.endswith("running_mean"):
            sd[k] = u(-0.2, 0.2)
        elif k.endswith("running_var"):
            sd[k] = u(0.5, 2.0)
        elif k.endswith(".weight"):  # LayerNorm / BatchNorm gamma
            sd[k] = u(0.5, 1.5)
        elif bn:  # BatchNorm beta
            sd[k] = u(-0.1, 0.1)
        else:  # LayerNorm beta, Linear / in_proj / out_proj / LSTM biases
            assert "bias" in k, k
            sd[k] = synth.normal(seed, k, shape, std=0.1).astype(np.float32)
    for v in sd.values():
        v.setflags(write=False)
    return sd


def make_module(kind, name, cfg):
    """The drop-in module loaded with case_state, in eval mode, on the CPU."""
    m = new_module(kind, cfg)
    missing = m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in case_state(kind, name, cfg).items()},
                                strict=False)
    assert not missing.unexpected_keys and all(
        k == "positional_encoding.pe" or k.endswith("num_batches_tracked") for k in missing.missing_keys), missing
    return m.eval()


@functools.lru_cache(maxsize=None)
def run_inputs(name, mode, W, n):
    """(x2d, xcam): (n, W, 17, 2), (n, W, 3, 4) for "fwd"; (1, n, ...) for "slide"."""
    seed = _SEED[name]
    tag = f"{name}/{mode}/{W}/{n}"
    B, T = (n, W) if mode == "fwd" else (1, n)
    x2 = synth.normalized_windows(seed + 1, tag, B, T)
    xc = synth.normal(seed + 2, tag + "/cam", (B, T, 3, 4), std=0.5).astype(np.float32)
    x2.setflags(write=False)
    xc.setflags(write=False)
    return x2, xc


def windows(mode, W, x2, xc):
    return (x2, xc) if mode == "fwd" else sliding_windows(x2, xc, W)


@functools.lru_cache(maxsize=None)
def oracle_output(run_id, dtype):
    """The oracle's output of a run at `dtype` as float64 numpy, (windows, 17, 3); read-only."""
    _, kind, name, cfg, mode, W, n = RUNS[RUN_IDS.index(run_id)]
    state = {k: torch.tensor(v) for k, v in case_state(kind, name, cfg).items()}
    w2, wc = windows(mode, W, *(torch.tensor(a) for a in run_inputs(name, mode, W, n)))
    if kind == "transformer":
        y = transformer_forward(state, w2, wc, cfg[1], cfg[2], len(cfg[4]), dtype=dtype)
    else:
        y = lstm_forward(state, w2, wc, cfg[0], cfg[1], len(cfg[2]), dtype=dtype)
    y = y.reshape(-1, J_OUT, F_OUT).to(torch.float64).numpy()
    y.setflags(write=False)
    return y


def reference_error(run_id):
    """e_ref: max |float32 oracle - float64 oracle| over every output coordinate."""
    return float(np.abs(oracle_output(run_id, torch.float32) - oracle_output(run_id, torch.float64)).max())


def torch_modules_forward(kind, m, x2, xc):
    """The case's real nn submodules composed in eval mode on the CPU (the drop-in's own forward
    runs the native kernels only): (B, T, ...) float32 tensors -> (B, 17, 3)."""
    B, T = x2.shape[0], x2.shape[1]
    x = torch.cat([x2.reshape(B, T, -1), xc.reshape(B, T, -1)], dim=2)
    with torch.no_grad():
        if kind == "transformer":
            h = m.input_projection(x) + m.positional_encoding.pe[:, :T]
            h = m.transformer_encoder(m.pre_transformer_norm(h))
            y = m.mlp_layers(h[:, -1])
        else:
            h, _ = m.lstm_layers(x)
            y = m.mlp_layers(m.bn_lstm(h[:, -1]))
    return y.reshape(B, J_OUT, F_OUT)
