#!/usr/bin/env python3
"""Time the look-ahead batched step (vp3d_amd.stream.LookaheadStreamBatch, the look-ahead form of
csrc/stream_batch.hip) on (3, 3, 3, 3, 3) at 1024 channels, non-causal, against the causal
batched step (CausalStreamBatch) on a causal build of the same weights, in one process.

    python tools/bench_stream_lookahead.py [--streams 1,16,64] [--dtypes fp16] [--reps 50]
                                           [--out profiles/stream_lookahead_bench.json]

Per (dtype, S) four forms -- causal eager, causal graph replay, look-ahead eager, look-ahead
graph replay -- are warmed up past the look-ahead (every slot consuming, so the look-ahead step
is in its steady state: every layer runs and a pose row is written), then timed alternately with
device events; a sample is --steps steps, median and min..max of >= 50 samples per step.  A
look-ahead step issues the launches of a causal step, so the figure to read is look-ahead over
causal of the same form.  Needs a HIP device: there is no CPU timing.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "dynamic-camera-augmented-videopose3d_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def _timed(stream, fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n  # microseconds per call


def _stats(t):
    return {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t), "samples": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,16,64")
    ap.add_argument("--dtypes", default="fp16")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=64, help="steps per timed sample")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream_lookahead.py times the MI355X kernels (no CPU timing)")
    if args.reps < 50:
        raise SystemExit("--reps: at least 50 samples")
    from common.models.TemporalModel import TemporalModel
    from vp3d_amd import _native, synth
    from vp3d_amd.stream import CausalStreamBatch, LookaheadStreamBatch

    fw, C, J = (3, 3, 3, 3, 3), 1024, 17
    lifters = {}
    for causal in (True, False):
        m = TemporalModel(J, 2, J, list(fw), causal=causal, channels=C)
        sd = synth.lifter_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed=0)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        m.eval().cuda()
        lifters[causal] = (m, m.native_lifter())
    side = torch.cuda.Stream()
    main_stream = torch.cuda.current_stream()

    results = []
    for dtype in args.dtypes.split(","):
        for S in [int(s) for s in args.streams.split(",")]:
            x = torch.from_numpy(synth.normalized_windows(50, "bench_stream_lookahead", S, 1)[:, 0]).cuda()
            ce, cg = (CausalStreamBatch(lifters[True][1], S, dtype) for _ in range(2))
            le, lg = (LookaheadStreamBatch(lifters[False][1], S, dtype) for _ in range(2))
            out_c = torch.empty((S, J, 3), device="cuda")
            out_l = torch.empty((S, J, 3), device="cuda")
            fin, ain, _ = cg.io_tensors()
            fin.copy_(x.reshape(S, -1))
            ain.fill_(1)
            lin, codes, lout, lframe = lg.io_tensors()
            lin.copy_(x.reshape(S, -1))
            codes.fill_(LookaheadStreamBatch.CONSUME)
            torch.cuda.synchronize()
            cg.capture(side)
            lg.capture(side)
            forms = {
                "causal_eager": (main_stream, lambda: ce.step(x, None, out=out_c)),
                "causal_graph": (side, lambda: cg.replay(side)),
                "lookahead_eager": (main_stream, lambda: le.step(x, None, out=out_l)),
                "lookahead_graph": (side, lambda: lg.replay(side)),
            }
            warm = -(-(le.lookahead + 1) // args.steps) + 2  # past the look-ahead: steady emission
            for _ in range(warm):
                for st, fn in forms.values():
                    _timed(st, fn, args.steps)
            torch.cuda.synchronize()
            # eager and replayed look-ahead steps took the same steps on the same frames
            if int(lframe.min()) < 0 or float((out_l.reshape(S, -1) - lout).abs().max()) != 0.0:
                raise SystemExit(f"{dtype} S={S}: look-ahead graph and eager steps disagree: not timing them")
            times = {k: [] for k in forms}
            for _ in range(args.reps):
                for k, (st, fn) in forms.items():
                    times[k].append(_timed(st, fn, args.steps))
            row = {"dtype": dtype, "streams": S, "lookahead": le.lookahead, "steps_per_sample": args.steps}
            row.update({k: _stats(t) for k, t in times.items()})
            row["eager_lookahead_over_causal"] = row["lookahead_eager"]["median_us"] / row["causal_eager"]["median_us"]
            row["graph_lookahead_over_causal"] = row["lookahead_graph"]["median_us"] / row["causal_graph"]["median_us"]
            results.append(row)
            print(f"{dtype} S={S:2d}: " + "; ".join(
                f"{k} {row[k]['median_us']:.1f} us ({row[k]['min_us']:.1f}..{row[k]['max_us']:.1f})" for k in forms)
                + f"; look-ahead / causal = {row['eager_lookahead_over_causal']:.3f} eager, "
                f"{row['graph_lookahead_over_causal']:.3f} graph", flush=True)
            for o in (ce, cg, le, lg):
                o.close()
    out = {"bench": "stream_lookahead", "config": dict(filter_widths=fw, channels=C, joints=J),
           "build_hash": _native.load().vp3d_build_hash().decode(), "device": torch.cuda.get_device_name(0),
           "torch": torch.__version__, "results": results}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
