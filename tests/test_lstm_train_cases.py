"""The yardsticks of the CoupledLSTM training tests, checked on the CPU: the train-mode oracle of
tests/lstm_train_cases.py against torch's own nn.LSTM / BatchNorm1d autograd and against the
reference's recorded iterations (tests/golden/train_lstm_h64*.npz), the non-vacuity of the shape
table, run.py's refusals and the activation-store size (vp3d_seq_train_bytes)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import lstm_train_cases as LC


def _torch_step(c_H, c_L, head, state, x2, xc, tgt):
    """nn.LSTM + BatchNorm1d + head under autograd in float64 (dropout 0): (y, loss, grads)."""
    lstm = nn.LSTM(46, c_H, c_L, batch_first=True).double()
    bn = nn.BatchNorm1d(c_H).double()
    layers, w = [], c_H
    for h in head:
        layers += [nn.Linear(w, h), nn.BatchNorm1d(h), nn.LeakyReLU(), nn.Dropout(0.0)]
        w = h
    layers.append(nn.Linear(w, LC.J_OUT * LC.F_OUT))
    mlp = nn.Sequential(*layers).double()
    mods = {"lstm_layers": lstm, "bn_lstm": bn, "mlp_layers": mlp}
    for name, m in mods.items():
        m.load_state_dict({k[len(name) + 1:]: torch.tensor(np.array(v), dtype=torch.float64)
                           for k, v in state.items() if k.startswith(name + ".")}, strict=False)
        m.train()
    B, T = x2.shape[:2]
    x = torch.cat([torch.tensor(x2).reshape(B, T, -1), torch.tensor(xc).reshape(B, T, -1)], dim=2).double()
    out, _ = lstm(x)
    y = mlp(bn(out[:, -1])).reshape(B, 1, LC.J_OUT, LC.F_OUT)
    loss = LC.mpjpe(y, torch.tensor(tgt).double())
    loss.backward()
    grads = {f"{name}.{k}": p.grad.numpy() for name, m in mods.items() for k, p in m.named_parameters()}
    return y.detach().numpy(), float(loss), grads


@pytest.mark.parametrize("T", [9, 243])
def test_oracle_matches_torch_autograd(T):
    """Dropout 0, float64: output, loss and every gradient equal torch's to 1e-12 relative."""
    c = LC.Case("torch", 64, 2, (32, 24), 5, T)
    from vp3d_amd import synth
    keys = {k: tuple(v.shape) for k, v in LC.new_module(c).state_dict().items()}
    state = LC.draw_state(keys, c.H, 7)
    x2 = synth.normalized_windows(8, f"torch/{T}", c.B, T)
    xc = synth.normal(9, f"torch/{T}/cam", (c.B, T, 3, 4), std=0.5).astype(np.float32)
    tgt = synth.normal(10, f"torch/{T}/t", (c.B, 1, 17, 3), std=0.2).astype(np.float32)
    y, loss, grads, _ = LC.oracle_step(state, x2, xc, tgt, c.H, c.L, len(c.head), dtype=torch.float64)
    y_t, loss_t, grads_t = _torch_step(c.H, c.L, c.head, state, x2, xc, tgt)
    assert LC.rel_err(y, y_t) <= 1e-12
    assert abs(loss - loss_t) <= 1e-12 * abs(loss_t)
    assert set(grads) == set(grads_t)
    worst = max(LC.rel_err(grads[k], grads_t[k]) for k in grads)
    print(f"T = {T}: largest relative gradient difference {worst:.2e}")
    assert worst <= 1e-12


def test_oracle_reproduces_golden():
    """The reference's two recorded iterations within the project's f32 gates."""
    g, meta, state = LC.load_golden()
    assert meta["dropout"] == 0.0 and meta["amsgrad"] and meta["steps"] == 2
    for it in range(meta["steps"]):
        if it > 0:
            state = LC.golden_after(g, it - 1)
        args = (state, g[f"s{it}/x2d"], g[f"s{it}/xcam"], g[f"s{it}/target"], meta["hidden"], meta["cells"],
                len(meta["head"]))
        y, loss, g32, stats = LC.oracle_step(*args, dtype=torch.float32)
        _, _, g64, _ = LC.oracle_step(*args, dtype=torch.float64)
        np.testing.assert_allclose(y, g[f"s{it}/y"], atol=1e-5, rtol=0)
        np.testing.assert_allclose(loss, float(g[f"s{it}/loss"]), rtol=1e-5)
        rec = {k: g[f"s{it}/grad/{k}"] for k in g64}
        for k in g64:
            LC.grad_gate(rec, g32, g64, k, len(meta["head"]), f"step {it} golden grad")
        for k, v in stats.items():
            np.testing.assert_allclose(v, g[f"s{it}/after/{k}"], rtol=1e-5, atol=1e-6, err_msg=k)


@pytest.mark.parametrize("cid", LC.CASE_IDS)
def test_cases_are_not_vacuous(cid):
    """Every parameter tensor of every row has a float64 gradient of norm > 1e-6 -- but for the
    tensors whose gradient is zero by construction in this architecture (LC.zero_grad_keys: a
    bias in front of a batch-statistics BatchNorm; weight_hh at T = 1), which no choice of weights
    or inputs can move; those are
    checked to BE zero (below 1e-12) instead, and the GPU tests gate them in absolute terms."""
    c = LC.case(cid)
    masks = LC.numpy_masks(c)
    _, _, g64, _ = LC.case_oracle(cid, masks, None, torch.float64)
    norms = {k: float(np.linalg.norm(v)) for k, v in g64.items()}
    zeros = LC.zero_grad_keys(len(c.head), c.L, c.T)
    live = {k: v for k, v in norms.items() if k not in zeros}
    print(cid, "gradient norms", min(live.values()), "..", max(live.values()))
    assert len(norms) == 4 * c.L + 2 + 4 * len(c.head) + 2
    weak = {k: v for k, v in live.items() if not v > 1e-6}
    assert not weak, weak
    assert all(norms[k] < 1e-12 for k in zeros), {k: norms[k] for k in zeros}


@pytest.mark.parametrize("argv,word", [
    (["--stride", "2"], "stride"),
    (["--trajectory"], "trajectory"),
    (["--compute-dtype", "bf16"], "fp32"),
    (["--train-dtype", "bf16"], "fp32"),
])
def test_run_lstm_training_refusals(argv, word):
    """Raised before a device is looked for (so also without one)."""
    import run
    with pytest.raises(SystemExit, match=word):
        run.main(["--use-model", "LSTM-Coupled", *argv])


def test_run_lstm_training_refuses_many_devices(monkeypatch):
    import run
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one device"):
        run.main(["--use-model", "LSTM-Coupled"])


@pytest.mark.parametrize("name", ["Transformer", "LSTM-Uncoupled", "StackedPoselifter"])
def test_run_other_models_still_refuse_training(name):
    import run
    with pytest.raises(SystemExit, match="training"):
        run.main(["--use-model", name])


def test_store_bytes_formula():
    from vp3d_amd import _native as N
    lib = N.load()
    cfg = N.vp3d_seq_cfg()
    cfg.kind = N.SEQ_LSTM
    cfg.num_joints_in, cfg.in_features, cfg.num_joints_out, cfg.out_features = 17, 2, 17, 3
    cfg.n_head_layers = 1
    cfg.head_layers[0] = 128
    for H, L, B, T in [(128, 2, 1024, 243), (64, 1, 3, 5), (128, 4, 33, 1)]:
        cfg.d_model, cfg.num_layers = H, L
        assert lib.vp3d_seq_train_bytes(ctypes.byref(cfg), B, T) == B * T * L * 6 * H * 4
    assert lib.vp3d_seq_train_bytes(ctypes.byref(cfg), 1024, 243) == 1024 * 243 * 4 * 6 * 128 * 4
    assert lib.vp3d_seq_train_bytes(ctypes.byref(cfg), 0, 243) == -1
    cfg.d_model = 96  # not a hidden size the kernels take
    assert lib.vp3d_seq_train_bytes(ctypes.byref(cfg), 4, 4) == -1
    cfg.d_model, cfg.kind = 128, N.SEQ_TRANSFORMER
    assert lib.vp3d_seq_train_bytes(ctypes.byref(cfg), 4, 4) == -1
