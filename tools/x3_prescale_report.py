#!/usr/bin/env python3
"""The f16x3 activation pre-scale against the float64 oracle, and what calibrating costs.

Config 4 (1,024 channels, fw 3,3,3,3,3, strided) on the 24 edge windows of
tests/test_gpu_x3_numerics.py, for the checkpoint rescaled by 2^-s
(oracle.x3_model.rescale_activations): the native f16x3 error without a pre-scale and after
calibrate_f16x3, in the scaled metres of that test.  Then the time of calibrate_f16x3 at 1,032
windows next to the plain fp32 forward it contains, and the bytes the statistics kernel reads.

    python tools/x3_prescale_report.py [--scales 0,4,6,8,10] [--reps 10] [--calibrate-only]

--calibrate-only runs 3 calibrations and nothing else (for a kernel trace of act_stats_kernel).
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "dynamic-camera-augmented-videopose3d_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from helpers import make_model  # noqa: E402
from oracle.temporal_ref import lifter_forward  # noqa: E402
from oracle.x3_model import rescale_activations  # noqa: E402
from test_gpu_x3_numerics import FW4, RMS_REF, edge_windows  # noqa: E402
from vp3d_amd import _native  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", default="0,4,6,8,10")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--calibrate-only", action="store_true")
    args = ap.parse_args()
    torch.set_num_threads(16)
    model, sd = make_model(True, FW4, False, 1024)
    model = model.cuda()
    xs = edge_windows()
    x = torch.from_numpy(xs).cuda()
    xb = x.repeat(43, 1, 1, 1)

    def load(state):
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})

    def fwd(inp, dtype):
        model.set_compute_dtype(dtype)
        with torch.no_grad():
            y = model(inp)
        model.sync_status()
        return y

    if args.calibrate_only:
        for _ in range(3):
            model.calibrate_f16x3(xb)
        return

    print(f"build {_native.load().vp3d_build_hash().decode()} (vp3d_build_hash)")
    ref64 = lifter_forward(sd, xs, list(FW4), strided=True, dtype=torch.float64).numpy().reshape(24, -1)
    ref32 = lifter_forward(sd, xs, list(FW4), strided=True).numpy().reshape(24, -1)
    scale = np.maximum(1.0, np.sqrt((ref64 ** 2).mean(axis=1)) / RMS_REF)
    err = lambda y: float((np.abs(np.asarray(y, dtype=np.float64).reshape(24, -1) - ref64).max(axis=1) / scale).max())
    print(f"e_ref32 {err(ref32):.3e} scaled m (the fp32 CPU oracle against float64; the same at every s)")
    for s in [int(t) for t in args.scales.split(",")]:
        model.set_f16x3_prescale(None)
        load(rescale_activations(sd, s))
        e_plain = err(fwd(x, "f16x3").cpu().numpy())
        p, stats = model.calibrate_f16x3(x)
        y_cal = fwd(x, "f16x3").cpu().numpy()
        e_f32 = err(fwd(x, "fp32").cpu().numpy())
        print(f"X3PRESCALE s={s:2d}: e_x3 uncalibrated {e_plain:.3e} calibrated {err(y_cal):.3e} e_f32 {e_f32:.3e} "
              f"[scaled m] chain exponent {p[0]} k-conv exponents {p[1::2]} "
              f"largest small_share {max(t['small_share'] for t in stats):.4f} "
              f"expand rms {stats[0]['rms']:.4g}")
    model.set_f16x3_prescale(None)
    load(sd)

    # calibration cost at B = 1,032: host clock around calls that end in a synchronise
    lifter = model.native_lifter()
    rows = [1032 * t for t in (81, 27, 27, 9, 9, 3, 3, 1, 1)]
    nbytes = sum(r * 1024 * 4 for r in rows)

    def timed(fn):
        fn()
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.reps

    t_cal = timed(lambda: model.calibrate_f16x3(xb))
    t_stats = timed(lambda: lifter.calibrate_x3(xb))
    t_f32 = timed(lambda: fwd(xb, "fp32"))
    model.set_f16x3_prescale(None)
    print(f"CALIBRATE B=1032: calibrate_f16x3 {t_cal * 1e3:.3f} ms, calibrate_x3 (fp32 forward + 9 reductions + "
          f"read-back) {t_stats * 1e3:.3f} ms, fp32 forward + sync {t_f32 * 1e3:.3f} ms; the reductions read "
          f"{nbytes / 1e6:.1f} MB (9 layers)")
    print(f"  host-clock difference {max(t_stats - t_f32, 0) * 1e3:.3f} ms: it also holds the accumulators' memset, "
          f"the poses' allocation and the read-back, so {nbytes / max(t_stats - t_f32, 1e-9) / 1e12:.2f} TB/s is a "
          "lower bound on the kernel's rate (the kernel trace has its own time)")


if __name__ == "__main__":
    main()
