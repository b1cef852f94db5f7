#!/usr/bin/env python3
"""Time the CoupledLSTM training step of `run.py --use-model LSTM-Coupled` (1,024 windows of 243
frames, hidden 128, 2 cells, head 128,128,128, dropout 0.25: forward, mpjpe, backward,
Adam(amsgrad)) on the native path, beside stock PyTorch on the same box in the same process.

    python tools/bench_lstm_train.py [--batch 1024] [--steps 20] [--warmup 3]
                                     [--out profiles/lstm_train.json]

native   the drop-in CoupledLSTM with enable_native_training() (csrc/seq_train.hip) and the
         native Adam (vp3d_amd.train.Adam)
torch    the same module's nn.LSTM / BatchNorm1d / head submodules composed as the reference's
         forward (CamLSTM.py:104-129) under torch autograd, with torch.optim.Adam(amsgrad=True)

Each step is timed on its own with device events; the medians are reported.  Then one more pass
of the native step runs with the trainer's role timers on (vp3d_seq_train_profile: events around
every launch group, so this pass is not the timed one): recurrence forward, backward through
time, weight-gradient GEMMs, head and element-wise; the step's remainder (loss, its backward,
Adam, host gaps) is the difference to the timed step.  One JSON line.  Needs a HIP device.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "dynamic-camera-augmented-videopose3d_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

JOINTS, HIDDEN, CELLS, HEAD, FRAMES, DROPOUT = 17, 128, 2, [128, 128, 128], 243, 0.25
F32_PEAK = 157.3e12  # FLOP/s, MI355X f32 vector FMA peak (and the f32 MFMA's)


def recurrence_flop(B, T, H=HIDDEN, L=CELLS):
    """2 x MACs of the products inside the recurrence: h W_hh^T per cell, x W_ih^T per cell above
    the first.  The backward through time has the same count (da W_hh, da W_ih)."""
    return 2.0 * B * T * (2 * L - 1) * H * 4 * H


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lstm_train.py times the MI355X kernels (no CPU timing)")
    from common.loss import mpjpe
    from common.models.CamLSTM import CoupledLSTM
    from vp3d_amd import _native as N
    from vp3d_amd import synth
    from vp3d_amd.train import Adam

    dev = torch.device("cuda", torch.cuda.current_device())
    B, T = args.batch, FRAMES
    torch.manual_seed(0)
    init = CoupledLSTM(JOINTS, 2, JOINTS, 3, HIDDEN, CELLS, HEAD, dropout=DROPOUT).state_dict()
    x2 = torch.from_numpy(synth.normalized_windows(6, "bench_lstm_train", B, T, n_joints=JOINTS)).to(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    xc = (torch.randn((B, T, 3, 4), device=dev, generator=g) * 0.5).contiguous()
    tgt = (torch.randn((B, 1, JOINTS, 3), device=dev, generator=g) * 0.2).contiguous()

    def make():
        m = CoupledLSTM(JOINTS, 2, JOINTS, 3, HIDDEN, CELLS, HEAD, dropout=DROPOUT)
        m.load_state_dict(init)
        return m.cuda().train()

    native = make().enable_native_training()
    stock = make()
    opts = {"native": Adam(native.parameters(), lr=1e-3, amsgrad=True),
            "torch": torch.optim.Adam(stock.parameters(), lr=1e-3, amsgrad=True)}

    def forward(mode):
        if mode == "native":
            return native(x2, xc)
        x = torch.cat([x2.reshape(B, T, -1), xc.reshape(B, T, -1)], dim=2)
        out, _ = stock.lstm_layers(x)
        return stock.mlp_layers(stock.bn_lstm(out[:, -1, :])).reshape(B, 1, JOINTS, 3)

    def step(mode):
        loss = mpjpe(forward(mode), tgt)
        opts[mode].zero_grad(set_to_none=False)
        loss.backward()
        opts[mode].step()
        return loss

    def med(vals):
        s = sorted(vals)
        return 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])

    out = {"bench": "lstm_train", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "build_hash": N.load().vp3d_build_hash().decode(),
           "config": dict(windows=B, frames=T, hidden=HIDDEN, cells=CELLS, head=HEAD, dropout=DROPOUT,
                          steps=args.steps, warmup=args.warmup)}
    tr = native.native_seq_trainer(dev)
    out["activation_store_bytes"] = tr.store_bytes(B, T)
    for mode in ("native", "torch"):
        for _ in range(args.warmup):
            step(mode)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loss = step(mode)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        out[mode] = {"median_ms_per_step": med(ms), "min_ms": min(ms), "max_ms": max(ms),
                     "windows_per_s": B / (med(ms) * 1e-3), "loss_last": float(loss.item())}
        print(f"{mode}: median {med(ms):.2f} ms/step (min {min(ms):.2f}, max {max(ms):.2f})", flush=True)
    out["ratio_torch_over_native"] = out["torch"]["median_ms_per_step"] / out["native"]["median_ms_per_step"]

    tr.profile(True)
    for _ in range(args.steps):
        step("native")
    roles = {k: v / args.steps for k, v in tr.profile(False).items()}
    out["native_roles_ms_per_step"] = roles
    print("native roles, ms/step: " + ", ".join(f"{k} {v:.2f}" for k, v in roles.items()), flush=True)
    flop = recurrence_flop(B, T)
    for role in ("recurrence_forward", "backward_through_time"):
        tf = flop / (roles[role] * 1e-3) / 1e12
        out[role + "_tflops"] = tf
        out[role + "_f32_peak_fraction"] = tf * 1e12 / F32_PEAK
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
