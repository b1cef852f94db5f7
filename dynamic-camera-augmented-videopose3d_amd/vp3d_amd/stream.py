"""Causal streaming inference (BASELINE config 5): one 2D frame in, one 3D pose out.

Wraps vp3d_stream (include/vp3d.h): a batch of steps is one layer-pipelined persistent
launch (csrc/stream_pipe.hip: every CU owns one layer's channel slice with its weights
resident in VGPRs as f32 -- exact fp32 weights for dtype "fp32", 16-bit weights widened
for "fp16" / "bf16" -- and layer outputs are handed between CUs in-launch); shapes the
pipeline does not cover fall back to stream_persist.hip (16-bit weights in LDS) or to one
GEMV launch per layer (csrc/stream_step.hip).  For a causal dilated TemporalModel
(reference TemporalModel.py:79-138 with causal=True), pose k of the stream equals
frame k of the reference's whole-sequence evaluation of the edge-padded
sequence (UnchunkedGenerator, generators.py:193-198, causal_shift = pad).

CausalStreamBatch advances many such streams in one step (vp3d_mstream,
csrc/stream_batch.hip): one skinny-GEMM launch per layer over all of them.

LookaheadStreamBatch runs the same batched step for a NON-causal TemporalModel (causal=False,
the reference's default), (receptive field - 1) / 2 frames late, with a drain at the end of a
sequence for the reference's right edge padding (vp3d_lstream); lift_sequences schedules whole
ragged sequences over its slots.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native as N


class CausalStream:
    def __init__(self, lifter, dtype: str = "fp16"):
        """lifter: a NativeLifter (``model.native_lifter()``) of a causal TemporalModel."""
        self._lib = N.load()
        self.lifter = lifter
        self.device = lifter.device
        self.dtype = dtype
        self._s = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_stream_create(lifter._h, N.DTYPES[dtype], ctypes.byref(self._s)),
                    "vp3d_stream_create")
        fin, fout, q = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int()
        N.check(self._lib.vp3d_stream_io(self._s, ctypes.byref(fin), ctypes.byref(fout), ctypes.byref(q)))
        self._in_ptr, self._out_ptr, self.queue_len = fin.value, fout.value, q.value
        self.n_in = lifter.cfg.num_joints_in * lifter.cfg.in_features
        self.n_out = lifter.cfg.num_joints_out * 3
        self._graph_stream = None

    def reset(self) -> None:
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_stream_reset(self._s, N.stream_ptr(self.device)))

    def step(self, frame: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """frame: (J_in, F) float32 on the device -> (J_out, 3) float32."""
        if not frame.is_cuda:
            raise RuntimeError("vp3d: stream frames must be HIP device tensors (no CPU fallback)")
        frame = frame.contiguous().float()
        assert frame.numel() == self.n_in
        if out is None:
            out = torch.empty((self.n_out // 3, 3), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_stream_step(self._s, frame.data_ptr(), out.data_ptr(),
                                               N.stream_ptr(self.device)), "vp3d_stream_step")
        return out

    def frames_seen(self) -> int:
        return int(self._lib.vp3d_stream_frames_seen(self._s))

    @property
    def persistent(self) -> bool:
        """True when steps run as one persistent launch per batch (weights resident on
        chip: mode 'pipe' or 'persist'); False for one GEMV launch per layer
        (VP3D_STREAM_MODE=launches, or a shape neither persistent form covers)."""
        return bool(self._lib.vp3d_stream_persistent(self._s))

    @property
    def mode(self) -> str:
        """'pipe' (layer-pipelined persistent launch, stream_pipe.hip), 'persist' (every CU
        runs every layer, weights in LDS, stream_persist.hip) or 'launches' (GEMV per layer)."""
        return {2: "pipe", 1: "persist", 0: "launches"}[int(self._lib.vp3d_stream_mode(self._s))]

    def check(self) -> None:
        """Synchronise and raise if a persistent launch gave up waiting on another CU."""
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_stream_status(self._s), "vp3d_stream_status")

    # ---- serving: the pipelined launch stays resident, frames posted from the host ----
    def serve(self, idle_ms: float = 200.0, stream: torch.cuda.Stream | None = None) -> "Serving":
        """Context manager for real-time use, one frame in flight (config 5's single-frame
        latency): the layer-pipelined launch (mode 'pipe') stays resident with its weights
        in VGPRs; `post(frame)` writes a host frame into pinned memory, `wait(t)` spins on
        pinned memory until pose t is there -- no launch, copy or graph per frame.  The
        launch ends itself after `idle_ms` without a frame."""
        return Serving(self, idle_ms, stream)

    def trace(self):
        """Per-frame device clocks of the layer-pipelined launch (VP3D_STREAM_TRACE=n set
        before the stream was created): returns (clocks, role_first_wg) with clocks of shape
        (workgroups, n, 11) -- [..., 0] input complete, [..., 1 + w] wave w's first output
        stored, 100 MHz ticks, 0 = not recorded; [..., 9], [..., 10] the shader clock counter
        at [..., 0] and [..., 1] -- for the first n frames of the last launch, then clears them."""
        roles, frames = ctypes.c_int32(), ctypes.c_int32()
        N.check(self._lib.vp3d_stream_trace(self._s, None, 0, None, ctypes.byref(roles), ctypes.byref(frames)),
                "vp3d_stream_trace")
        first = np.zeros(roles.value + 1, np.int32)
        N.check(self._lib.vp3d_stream_trace(self._s, None, 0, first.ctypes.data, ctypes.byref(roles),
                                            ctypes.byref(frames)), "vp3d_stream_trace")
        out = np.zeros((int(first[-1]), frames.value, 11), np.uint64)
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_stream_trace(self._s, out.ctypes.data, out.size, first.ctypes.data,
                                                ctypes.byref(roles), ctypes.byref(frames)), "vp3d_stream_trace")
        return out, first

    # ---- hipGraph replay: steps read the device frame queue, write the pose ring ----
    def io_tensors(self):
        """(frame_queue (Q, J_in*F), pose_ring (Q, J_out*3)) views of the device buffers:
        step t reads frame slot t % Q and writes pose slot t % Q."""
        Q = self.queue_len
        fin = _wrap(self._in_ptr, Q * self.n_in, self.device).view(Q, self.n_in)
        fout = _wrap(self._out_ptr, Q * self.n_out, self.device).view(Q, self.n_out)
        return fin, fout

    def capture(self, stream: torch.cuda.Stream, steps: int = 1) -> None:
        """Capture `steps` consecutive steps into one hipGraph."""
        self._graph_stream = stream
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_stream_graph_capture(self._s, stream.cuda_stream, int(steps)),
                    "vp3d_stream_graph_capture")

    def replay(self, stream: torch.cuda.Stream | None = None) -> None:
        s = stream if stream is not None else self._graph_stream
        N.check(self._lib.vp3d_stream_graph_launch(self._s, s.cuda_stream), "vp3d_stream_graph_launch")

    def close(self) -> None:
        if self._s:
            self._lib.vp3d_stream_destroy(self._s)
            self._s = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Serving:
    """A resident serve launch of a CausalStream (vp3d_stream_serve_*)."""

    def __init__(self, st: CausalStream, idle_ms: float, stream):
        self.st, self.idle_ms = st, float(idle_ms)
        self.stream = stream if stream is not None else torch.cuda.Stream(st.device)
        self._pose = np.empty(st.n_out, dtype=np.float32)

    def __enter__(self):
        with torch.cuda.device(self.st.device):
            N.check(self.st._lib.vp3d_stream_serve_begin(self.st._s, self.stream.cuda_stream, self.idle_ms),
                    "vp3d_stream_serve_begin")
        return self

    def post(self, frame) -> int:
        """Post one frame ((J_in, F) host float32); returns its stream index."""
        f = np.ascontiguousarray(np.asarray(frame, dtype=np.float32)).reshape(-1)
        assert f.size == self.st.n_in
        t = ctypes.c_int64()
        N.check(self.st._lib.vp3d_stream_serve_post(self.st._s, f.ctypes.data, ctypes.byref(t)),
                "vp3d_stream_serve_post")
        return int(t.value)

    def wait(self, t: int, timeout_ms: float = 1000.0) -> np.ndarray:
        """Pose (J_out, 3) of frame t (host float32)."""
        out = np.empty(self.st.n_out, dtype=np.float32)
        N.check(self.st._lib.vp3d_stream_serve_wait(self.st._s, int(t), out.ctypes.data, float(timeout_ms)),
                "vp3d_stream_serve_wait")
        return out.reshape(-1, 3)

    def step(self, frame, timeout_ms: float = 1000.0) -> np.ndarray:
        """post + wait in one library call; the pose (J_out, 3).  `last_latency_us` = the
        library's own wall time for it (post start -> pose copied out, no Python overhead)."""
        f = np.ascontiguousarray(np.asarray(frame, dtype=np.float32)).reshape(-1)
        assert f.size == self.st.n_in
        out = np.empty(self.st.n_out, dtype=np.float32)
        lat = ctypes.c_double()
        N.check(self.st._lib.vp3d_stream_serve_step(self.st._s, f.ctypes.data, out.ctypes.data, float(timeout_ms),
                                                    ctypes.byref(lat)), "vp3d_stream_serve_step")
        self.last_latency_us = lat.value
        return out.reshape(-1, 3)

    def __exit__(self, *exc):
        with torch.cuda.device(self.st.device):
            N.check(self.st._lib.vp3d_stream_serve_end(self.st._s, self.stream.cuda_stream), "vp3d_stream_serve_end")
        return False


class CausalStreamBatch:
    """`n_streams` independent causal streams ("slots") of one lifter advanced together.

    Wraps vp3d_mstream (include/vp3d.h): every layer of a step is one skinny GEMM over the
    slots (csrc/stream_batch.hip: exact f32 MFMA, f32 activations, 16-bit weights widened in
    registers), so a step reads the weights once however many slots take part.  Each slot has
    its own position and rings; a slot that is inactive in a step consumes no frame and keeps
    its pose row.  Slot s's k-th active step equals frame k of the reference's whole-sequence
    causal evaluation of the frames that slot consumed, as for a CausalStream -- which stays
    the path for one stream.
    """

    def __init__(self, lifter, n_streams: int, dtype: str = "fp16"):
        """lifter: a NativeLifter (``model.native_lifter()``) of a causal TemporalModel."""
        self._lib = N.load()
        self.lifter = lifter
        self.device = lifter.device
        self.dtype = dtype
        self.n_streams = int(n_streams)
        self._m = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_mstream_create(lifter._h, N.DTYPES[dtype], self.n_streams,
                                                  ctypes.byref(self._m)), "vp3d_mstream_create")
        f, a, p = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        N.check(self._lib.vp3d_mstream_io(self._m, ctypes.byref(f), ctypes.byref(a), ctypes.byref(p)))
        self._io_ptrs = (f.value, a.value, p.value)
        self.j_in, self.in_features = lifter.cfg.num_joints_in, lifter.cfg.in_features
        self.n_in = self.j_in * self.in_features
        self.n_out = lifter.cfg.num_joints_out * 3
        self._graph_stream = None

    def step(self, frames: torch.Tensor, active: torch.Tensor | None = None,
             out: torch.Tensor | None = None) -> torch.Tensor:
        """frames: (S, J_in, F) float32 on the device; active: (S,) device tensor of an integer
        or bool dtype (nonzero = the slot consumes its frame), None = every slot
        -> (S, J_out, 3) float32; the row of an inactive slot is that of its last active step."""
        S = self.n_streams
        if not frames.is_cuda or (active is not None and not active.is_cuda):
            raise RuntimeError("vp3d: stream frames must be HIP device tensors (no CPU fallback)")
        if tuple(frames.shape) != (S, self.j_in, self.in_features):
            raise RuntimeError(f"vp3d: frames must be ({S}, {self.j_in}, {self.in_features}), got {tuple(frames.shape)}")
        frames = frames.contiguous().float()
        a_ptr = None
        if active is not None:
            if tuple(active.shape) != (S,) or active.dtype.is_floating_point or active.dtype.is_complex:
                raise RuntimeError(f"vp3d: active must be an integer or bool tensor of shape ({S},)")
            active = (active != 0).to(torch.int32).contiguous()
            a_ptr = active.data_ptr()
        if out is None:
            out = torch.empty((S, self.n_out // 3, 3), dtype=torch.float32, device=self.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.numel() == S * self.n_out
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_mstream_step(self._m, frames.data_ptr(), a_ptr, out.data_ptr(),
                                                N.stream_ptr(self.device)), "vp3d_mstream_step")
        return out

    def reset(self, slot: int | None = None) -> None:
        """Restart one slot (None: every slot): its next frame is frame 0 of a new sequence."""
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_mstream_reset(self._m, -1 if slot is None else int(slot),
                                                 N.stream_ptr(self.device)), "vp3d_mstream_reset")

    def frames_seen(self) -> np.ndarray:
        """Frames consumed so far by each slot: (S,) int64 (synchronises)."""
        out = np.zeros(self.n_streams, dtype=np.int64)
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_mstream_frames_seen(self._m, out.ctypes.data), "vp3d_mstream_frames_seen")
        return out

    # ---- hipGraph replay: one step reading / writing the io buffers ----
    def io_tensors(self):
        """(frames (S, J_in*F) float32, active (S,) int32, poses (S, J_out*3) float32) views of
        the device buffers a replayed step reads and writes."""
        S = self.n_streams
        f, a, p = self._io_ptrs
        return (_wrap(f, S * self.n_in, self.device).view(S, self.n_in),
                _wrap(a, S, self.device, "<i4"),
                _wrap(p, S * self.n_out, self.device).view(S, self.n_out))

    def capture(self, stream: torch.cuda.Stream) -> None:
        """Capture one step into a hipGraph on `stream` (not the default stream)."""
        self._graph_stream = stream
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_mstream_graph_capture(self._m, stream.cuda_stream), "vp3d_mstream_graph_capture")

    def replay(self, stream: torch.cuda.Stream | None = None) -> None:
        s = stream if stream is not None else self._graph_stream
        N.check(self._lib.vp3d_mstream_graph_launch(self._m, s.cuda_stream), "vp3d_mstream_graph_launch")

    def close(self) -> None:
        if self._m:
            self._lib.vp3d_mstream_destroy(self._m)
            self._m = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LookaheadStreamBatch:
    """`n_streams` slots of one NON-causal lifter (the reference's default, TemporalModel.py:79-138
    with causal=False) advanced together, each `lookahead` = (receptive field - 1) / 2 frames late.

    Wraps vp3d_lstream (include/vp3d.h; the look-ahead form of csrc/stream_batch.hip).  Per step a
    slot gets a code: IDLE, CONSUME (its frame) or DRAIN (a step that repeats its last consumed
    frame, the reference's right edge padding, generators.py:193-198).  A step taken with
    `lookahead` or more steps behind it writes the pose of frame t - lookahead into the slot's
    row and reports that frame index in pose_frame (-1: no row written).  After n frames and
    `lookahead` drains a slot has emitted n poses, pose k being frame k of the reference's
    whole-sequence evaluation of those n frames; reset the slot for the next sequence.
    """

    IDLE, CONSUME, DRAIN = 0, 1, 2

    def __init__(self, lifter, n_streams: int, dtype: str = "fp16"):
        """lifter: a NativeLifter (``model.native_lifter()``) of a non-causal TemporalModel."""
        self._lib = N.load()
        self.lifter = lifter
        self.device = lifter.device
        self.dtype = dtype
        self.n_streams = int(n_streams)
        self._l = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            rc = self._lib.vp3d_lstream_create(lifter._h, N.DTYPES[dtype], self.n_streams, ctypes.byref(self._l))
            if rc and lifter.cfg.causal:
                raise RuntimeError("vp3d: vp3d_lstream_create: " + self._lib.vp3d_last_error().decode()
                                   + " (CausalStreamBatch)")
            N.check(rc, "vp3d_lstream_create")
        la = ctypes.c_int32()
        N.check(self._lib.vp3d_lstream_lookahead(self._l, ctypes.byref(la)), "vp3d_lstream_lookahead")
        self.lookahead = int(la.value)
        f, c, p, k = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        N.check(self._lib.vp3d_lstream_io(self._l, ctypes.byref(f), ctypes.byref(c), ctypes.byref(p), ctypes.byref(k)))
        self._io_ptrs = (f.value, c.value, p.value, k.value)
        self.j_in, self.in_features = lifter.cfg.num_joints_in, lifter.cfg.in_features
        self.n_in = self.j_in * self.in_features
        self.n_out = lifter.cfg.num_joints_out * 3
        self._graph_stream = None

    def step(self, frames: torch.Tensor, codes: torch.Tensor | None = None, out: torch.Tensor | None = None):
        """frames: (S, J_in, F) float32 on the device; codes: (S,) device tensor of an integer or
        bool dtype (0 idle, 1 consume, 2 drain), None = every slot consumes
        -> (poses (S, J_out, 3) float32, pose_frame (S,) int32): row s holds the pose of frame
        pose_frame[s] of slot s's sequence if this step wrote it (pose_frame[s] >= 0), else what
        it held before (zeros before the slot's first pose)."""
        S = self.n_streams
        if not frames.is_cuda or (codes is not None and not codes.is_cuda):
            raise RuntimeError("vp3d: stream frames must be HIP device tensors (no CPU fallback)")
        if tuple(frames.shape) != (S, self.j_in, self.in_features):
            raise RuntimeError(f"vp3d: frames must be ({S}, {self.j_in}, {self.in_features}), got {tuple(frames.shape)}")
        frames = frames.contiguous().float()
        c_ptr = None
        if codes is not None:
            if tuple(codes.shape) != (S,) or codes.dtype.is_floating_point or codes.dtype.is_complex:
                raise RuntimeError(f"vp3d: codes must be an integer or bool tensor of shape ({S},)")
            codes = codes.to(torch.int32).contiguous()
            c_ptr = codes.data_ptr()
        if out is None:
            out = torch.empty((S, self.n_out // 3, 3), dtype=torch.float32, device=self.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.numel() == S * self.n_out
        pose_frame = torch.empty(S, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_lstream_step(self._l, frames.data_ptr(), c_ptr, out.data_ptr(),
                                                pose_frame.data_ptr(), N.stream_ptr(self.device)), "vp3d_lstream_step")
        return out, pose_frame

    def reset(self, slot: int | None = None) -> None:
        """Restart one slot (None: every slot): its next frame is frame 0 of a new sequence."""
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_lstream_reset(self._l, -1 if slot is None else int(slot),
                                                 N.stream_ptr(self.device)), "vp3d_lstream_reset")

    def counts(self):
        """(frames consumed, poses emitted) per slot: two (S,) int64 arrays (synchronises)."""
        n = np.zeros(self.n_streams, dtype=np.int64)
        e = np.zeros(self.n_streams, dtype=np.int64)
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_lstream_counts(self._l, n.ctypes.data, e.ctypes.data), "vp3d_lstream_counts")
        return n, e

    # ---- hipGraph replay: one step reading / writing the io buffers ----
    def io_tensors(self):
        """(frames (S, J_in*F) float32, codes (S,) int32, poses (S, J_out*3) float32, pose_frame
        (S,) int32) views of the device buffers a replayed step reads and writes."""
        S = self.n_streams
        f, c, p, k = self._io_ptrs
        return (_wrap(f, S * self.n_in, self.device).view(S, self.n_in),
                _wrap(c, S, self.device, "<i4"),
                _wrap(p, S * self.n_out, self.device).view(S, self.n_out),
                _wrap(k, S, self.device, "<i4"))

    def capture(self, stream: torch.cuda.Stream) -> None:
        """Capture one step into a hipGraph on `stream` (not the default stream)."""
        self._graph_stream = stream
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_lstream_graph_capture(self._l, stream.cuda_stream), "vp3d_lstream_graph_capture")

    def replay(self, stream: torch.cuda.Stream | None = None) -> None:
        s = stream if stream is not None else self._graph_stream
        N.check(self._lib.vp3d_lstream_graph_launch(self._l, s.cuda_stream), "vp3d_lstream_graph_launch")

    def lift_sequences(self, seqs):
        """Lift any number of ragged sequences, each a (T_i, J_in, F) device tensor, over the
        slots: a free slot takes the next sequence, consumes it a frame per step, drains
        `lookahead` steps and is reset for the one after.  Returns a list of (T_i, J_out, 3)
        float32 device tensors, each exactly what stepping that sequence by hand gives.

        Costs one small host-to-device upload (the step codes) per step.  Which frame a pose
        row belongs to is mirrored on the host instead of read back from pose_frame: the
        mirror holds because this method resets every slot on entry and each slot again
        before it takes a new sequence, so no state a caller left in the batch can reach it
        (and whatever the slots held before the call is discarded)."""
        S, P = self.n_streams, self.lookahead
        seqs = list(seqs)
        for x in seqs:
            if not x.is_cuda:
                raise RuntimeError("vp3d: stream frames must be HIP device tensors (no CPU fallback)")
            if x.dim() != 3 or tuple(x.shape[1:]) != (self.j_in, self.in_features):
                raise RuntimeError(f"vp3d: a sequence must be (T, {self.j_in}, {self.in_features}), got {tuple(x.shape)}")
        seqs = [x.contiguous().float() for x in seqs]
        outs = [torch.empty((x.shape[0], self.n_out // 3, 3), dtype=torch.float32, device=self.device) for x in seqs]
        self.reset()
        nxt = 0
        cur = [-1] * S   # the sequence a slot carries, -1 = free
        took = [0] * S   # steps the slot has taken on it
        frames = torch.zeros((S, self.j_in, self.in_features), dtype=torch.float32, device=self.device)
        poses = torch.empty((S, self.n_out // 3, 3), dtype=torch.float32, device=self.device)
        while True:
            codes = [self.IDLE] * S
            for s in range(S):
                if cur[s] < 0:
                    while nxt < len(seqs) and seqs[nxt].shape[0] == 0:
                        nxt += 1
                    if nxt == len(seqs):
                        continue
                    cur[s], took[s], nxt = nxt, 0, nxt + 1
                    self.reset(s)
                x = seqs[cur[s]]
                if took[s] < x.shape[0]:
                    codes[s] = self.CONSUME
                    frames[s].copy_(x[took[s]])
                else:
                    codes[s] = self.DRAIN
            if not any(codes):
                break
            self.step(frames, torch.tensor(codes, dtype=torch.int32).to(self.device, non_blocking=True), out=poses)
            for s in range(S):
                if codes[s] == self.IDLE:
                    continue
                if took[s] >= P:  # this step wrote the pose of frame took - P (the host mirrors pose_frame)
                    outs[cur[s]][took[s] - P].copy_(poses[s])
                took[s] += 1
                if took[s] == seqs[cur[s]].shape[0] + P:
                    cur[s] = -1
        return outs

    def close(self) -> None:
        if self._l:
            self._lib.vp3d_lstream_destroy(self._l)
            self._l = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lift_sequences(lifter, seqs, n_streams: int = 16, dtype: str = "fp16"):
    """LookaheadStreamBatch(lifter, n_streams, dtype).lift_sequences(seqs) on a batch of its own."""
    bt = LookaheadStreamBatch(lifter, n_streams, dtype)
    try:
        return bt.lift_sequences(seqs)
    finally:
        bt.close()


class _DevBuf:
    """Minimal __cuda_array_interface__ exporter for a raw device pointer."""

    def __init__(self, ptr: int, n: int, typestr: str = "<f4"):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False),
                                         "version": 2, "strides": None}


def _wrap(ptr: int, n: int, device, typestr: str = "<f4") -> torch.Tensor:
    with torch.cuda.device(device):
        return torch.as_tensor(_DevBuf(ptr, n, typestr), device=device)
