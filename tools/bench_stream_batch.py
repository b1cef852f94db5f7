#!/usr/bin/env python3
"""Time the batched causal streaming step (vp3d_amd.stream.CausalStreamBatch,
csrc/stream_batch.hip) on the config-5 model -- (3, 3, 3, 3, 3) at 1024 channels, causal --
against the only other way to advance S streams: S separate CausalStreams of the same lifter at
their default form, each stepped once per round, in the same process.

    python tools/bench_stream_batch.py [--streams 1,4,16,64] [--dtypes fp16,fp32] [--reps 50]
                                       [--out profiles/stream_batch_bench.json]

Per (dtype, S): the three forms -- batched step eager, batched step as a graph replay, the round
of S single steps -- are warmed up, then timed alternately with device events; a sample is
enough steps to last milliseconds (--steps batched steps, or as many rounds as give at least that
many single steps); median and min..max of >= 50 samples, per step / per round.  The figure to
read is the batched step's time over the round's at the same S.  Before timing, one step of
every form on the same frames: the batch's poses against the single streams' (another order of
the f32 sums, so close, not equal).  Needs a HIP device: there is no CPU timing.
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
    ap.add_argument("--streams", default="1,4,16,64")
    ap.add_argument("--dtypes", default="fp16,fp32")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=64, help="batched steps per timed sample")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream_batch.py times the MI355X kernels (no CPU timing)")
    if args.reps < 50:
        raise SystemExit("--reps: at least 50 samples")
    from common.models.TemporalModel import TemporalModel
    from vp3d_amd import _native, synth
    from vp3d_amd.stream import CausalStream, CausalStreamBatch

    fw, C, J = (3, 3, 3, 3, 3), 1024, 17
    m = TemporalModel(J, 2, J, list(fw), causal=True, channels=C)
    sd = synth.lifter_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.eval().cuda()
    lifter = m.native_lifter()
    side = torch.cuda.Stream()
    main_stream = torch.cuda.current_stream()

    results = []
    for dtype in args.dtypes.split(","):
        for S in [int(s) for s in args.streams.split(",")]:
            x = torch.from_numpy(synth.normalized_windows(50, "bench_stream_batch", S, 1)[:, 0]).cuda()  # (S, J, 2)
            eager, graph = CausalStreamBatch(lifter, S, dtype), CausalStreamBatch(lifter, S, dtype)
            singles = [CausalStream(lifter, dtype) for _ in range(S)]
            out_b = torch.empty((S, J, 3), device="cuda")
            out_s = torch.empty((S, J, 3), device="cuda")
            fin, ain, pout = graph.io_tensors()
            fin.copy_(x.reshape(S, -1))
            ain.fill_(1)  # every slot active in the replayed step, as in the eager one
            torch.cuda.synchronize()
            graph.capture(side)

            def step_eager():
                eager.step(x, None, out=out_b)

            def step_graph():
                graph.replay(side)

            def round_singles():
                for s, st in enumerate(singles):
                    st.step(x[s], out=out_s[s])

            # one step of every form on the same frames: the poses agree
            step_eager()
            round_singles()
            with torch.cuda.stream(side):
                step_graph()
            torch.cuda.synchronize()
            diff_single = float((out_b - out_s).abs().max())
            diff_graph = float((out_b.reshape(S, -1) - pout).abs().max())
            if diff_graph != 0.0 or not diff_single <= 2e-5:
                raise SystemExit(f"{dtype} S={S}: the forms disagree (graph vs eager {diff_graph:.3e} m, "
                                 f"batch vs singles {diff_single:.3e} m): not timing them")
            rounds = max(1, -(-args.steps // S))  # rounds per sample: >= --steps single steps
            for _ in range(3):
                _timed(main_stream, step_eager, args.steps)
                _timed(side, step_graph, args.steps)
                _timed(main_stream, round_singles, rounds)
            times = {"batched_eager": [], "batched_graph": [], "singles_round": []}
            for _ in range(args.reps):
                times["batched_eager"].append(_timed(main_stream, step_eager, args.steps))
                times["batched_graph"].append(_timed(side, step_graph, args.steps))
                times["singles_round"].append(_timed(main_stream, round_singles, rounds))
            for st in singles:
                st.check()
            row = {"dtype": dtype, "streams": S, "single_form": singles[0].mode, "steps_per_sample": args.steps,
                   "rounds_per_sample": rounds, "max_abs_diff_batch_vs_singles_m": diff_single,
                   "max_abs_diff_graph_vs_eager_m": diff_graph}
            row.update({k: _stats(t) for k, t in times.items()})
            row["eager_over_singles"] = row["batched_eager"]["median_us"] / row["singles_round"]["median_us"]
            row["graph_over_singles"] = row["batched_graph"]["median_us"] / row["singles_round"]["median_us"]
            results.append(row)
            print(f"{dtype} S={S:2d}: batched step eager {row['batched_eager']['median_us']:8.1f} us "
                  f"({row['batched_eager']['min_us']:.1f}..{row['batched_eager']['max_us']:.1f}), graph "
                  f"{row['batched_graph']['median_us']:8.1f} us ({row['batched_graph']['min_us']:.1f}.."
                  f"{row['batched_graph']['max_us']:.1f}); {S} single steps ({row['single_form']}) "
                  f"{row['singles_round']['median_us']:8.1f} us ({row['singles_round']['min_us']:.1f}.."
                  f"{row['singles_round']['max_us']:.1f}); batched / singles = {row['eager_over_singles']:.3f} eager, "
                  f"{row['graph_over_singles']:.3f} graph; max|batch - singles| {diff_single:.2e} m", flush=True)
            for o in [eager, graph] + singles:
                o.close()
    out = {"bench": "stream_batch", "config": dict(filter_widths=fw, channels=C, joints=J),
           "build_hash": _native.load().vp3d_build_hash().decode(), "device": torch.cuda.get_device_name(0),
           "torch": torch.__version__, "results": results}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
