#!/usr/bin/env python3
"""Time the training step in fp32 and in bf16 mixed precision (model.set_train_dtype) in one
process: the step of `bench.py --train` (dilated TemporalModel, 243-frame receptive field, 1,024
channels, dropout 0.25, 1,024 windows, mpjpe, backward, native Adam(amsgrad)).

    python tools/bench_train_dtype.py [--batch 1024] [--steps 10] [--warmup 3] [--pairs 4]
                                      [--out profiles/train_dtype.json]

Two models with the same seeded weights, one per mode, each with its own optimiser.  After a
warm-up of both, `pairs` alternating pairs (fp32, bf16) of `steps` steps are timed with device
events.  Then one more pass per mode runs with the trainer's role timers on
(vp3d_train_profile: events around every launch group, so this pass is not the timed one): the
device time of the forward conv GEMMs, the data-gradient GEMMs, the weight gradients and the
element-wise / per-channel passes; the step's remainder (loss, its backward, Adam, host gaps)
is the difference to the timed step.  One JSON line.  Needs a HIP device.
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

FW = [3, 3, 3, 3, 3]
JOINTS, CHANNELS = 17, 1024
BF16_MFMA_PEAK, F32_MFMA_PEAK = 2516.6e12, 157.3e12  # FLOP/s, MI355X dense matrix peaks


def block_flop_per_window(T, fw=FW, channels=CHANNELS):
    """2 x MACs of one role (forward = dgrad = wgrad) of the block convs on one window."""
    L, dil, total = T - (fw[0] - 1), fw[0], 0
    for w in fw[1:]:
        L -= (w - 1) * dil
        total += 2 * L * channels * channels * (w + 1)
        dil *= w
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_dtype.py times the MI355X kernels (no CPU timing)")
    from common.loss import mpjpe
    from common.models.TemporalModel import TemporalModel
    from vp3d_amd import synth
    from vp3d_amd.train import Adam

    dev = torch.device("cuda", torch.cuda.current_device())
    ref = TemporalModel(JOINTS, 2, JOINTS, FW, channels=CHANNELS, dropout=0.25)
    sd = synth.lifter_state_dict([(k, tuple(v.shape)) for k, v in ref.state_dict().items()], seed=0)
    RF, B = ref.receptive_field(), args.batch
    x = torch.from_numpy(synth.normalized_windows(6, "bench_train_dtype", B, RF, n_joints=JOINTS)).to(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    tgt = (torch.randn((B, 1, JOINTS, 3), device=dev, generator=g) * 0.2).contiguous()

    runs = {}
    for mode in ("fp32", "bf16"):
        m = TemporalModel(JOINTS, 2, JOINTS, FW, channels=CHANNELS, dropout=0.25)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        m.cuda().train().set_train_dtype(mode)
        runs[mode] = (m, Adam(m.parameters(), lr=1e-3, amsgrad=True))

    def step(mode):
        m, opt = runs[mode]
        loss = mpjpe(m(x), tgt)
        opt.zero_grad(set_to_none=False)
        loss.backward()
        opt.step()
        return loss

    def timed(mode, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            loss = step(mode)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n, float(loss.item())

    for mode in runs:
        for _ in range(args.warmup):
            step(mode)
    torch.cuda.synchronize()
    pairs, loss_last = [], {}
    for i in range(args.pairs):
        row = {}
        for mode in ("fp32", "bf16"):
            row[mode], loss_last[mode] = timed(mode, args.steps)
        row["ratio_fp32_over_bf16"] = row["fp32"] / row["bf16"]
        pairs.append(row)
        print(f"pair {i}: fp32 {row['fp32']:.2f} ms/step, bf16 {row['bf16']:.2f} ms/step, "
              f"x{row['ratio_fp32_over_bf16']:.3f}", flush=True)

    roles = {}
    for mode in ("fp32", "bf16"):
        tr = runs[mode][0].native_trainer(dev)
        tr.profile(True)
        for _ in range(args.steps):
            step(mode)
        r = tr.profile(False)
        roles[mode] = {k: v / args.steps for k, v in r.items()}
        print(f"{mode} roles, ms/step: " + ", ".join(f"{k} {v:.2f}" for k, v in roles[mode].items()), flush=True)

    def med(vals):
        s = sorted(vals)
        return 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])

    out = {"bench": "train_dtype", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "config": dict(filter_widths=FW, channels=CHANNELS, windows=B, frames=RF, dropout=0.25,
                          steps_per_sample=args.steps, warmup=args.warmup),
           "pairs_ms_per_step": pairs, "loss_last": loss_last, "roles_ms_per_step": roles}
    for mode in ("fp32", "bf16"):
        ms = med([p[mode] for p in pairs])
        out[mode] = {"median_ms_per_step": ms, "windows_per_s": B / (ms * 1e-3)}
    out["ratio_fp32_over_bf16_median"] = out["fp32"]["median_ms_per_step"] / out["bf16"]["median_ms_per_step"]
    out["bf16_faster_in_every_pair"] = all(p["bf16"] < p["fp32"] for p in pairs)
    flop = block_flop_per_window(RF) * B
    out["bf16_wgrad_tflops_upper"] = flop / (roles["bf16"]["wgrad"] * 1e-3) / 1e12  # the role holds the f32 wgrads too
    out["bf16_wgrad_peak_fraction"] = out["bf16_wgrad_tflops_upper"] * 1e12 / BF16_MFMA_PEAK
    out["bf16_elementwise_share_of_step"] = roles["bf16"]["elementwise"] / out["bf16"]["median_ms_per_step"]
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
