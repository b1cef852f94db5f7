"""Python owner of a native lifter handle (vp3d_handle in include/vp3d.h).

`NativeLifter` is the thin object the drop-in `common.models.TemporalModel`
classes delegate their eval-mode forward to.  It owns one device copy of the
folded/packed weights and the activation workspace; it never computes anything
itself.
"""
from __future__ import annotations

import ctypes
from typing import Iterable, List, Sequence

import numpy as np
import torch

from . import _native as N


def weight_order(n_widths: int) -> List[str]:
    """state_dict keys in the order vp3d_create expects (include/vp3d.h)."""
    keys = ["expand_conv.weight", "expand_bn.weight", "expand_bn.bias",
            "expand_bn.running_mean", "expand_bn.running_var"]
    for i in range(2 * (n_widths - 1)):
        keys += [f"layers_conv.{i}.weight", f"layers_bn.{i}.weight", f"layers_bn.{i}.bias",
                 f"layers_bn.{i}.running_mean", f"layers_bn.{i}.running_var"]
    keys += ["shrink.weight", "shrink.bias"]
    return keys


def _host_f32(v) -> np.ndarray:
    if isinstance(v, torch.Tensor):
        v = v.detach().to("cpu", torch.float32).contiguous().numpy()
    return np.ascontiguousarray(np.asarray(v, dtype=np.float32))


class NativeLifter:
    """One vp3d_handle on one HIP device."""

    def __init__(self, num_joints_in: int, in_features: int, num_joints_out: int,
                 filter_widths: Sequence[int], causal: bool, channels: int, dense: bool,
                 variant: int, state: dict, device=None, bn_eps: float = 1e-5):
        self._lib = N.load()
        self.n_widths = len(filter_widths)
        self.num_joints_out = num_joints_out
        self.cfg = N.make_cfg(num_joints_in, in_features, num_joints_out, filter_widths, causal,
                              channels, dense, variant, bn_eps)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None
                                   else torch.device(device).index or 0)
        self._h = ctypes.c_void_p()
        arrays, ptrs = self._pack(state)
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_create(ctypes.byref(self.cfg), ptrs, len(arrays),
                                          ctypes.byref(self._h)), "vp3d_create")
        self.n_layers = self._lib.vp3d_layer_count(self._h)

    def _pack(self, state: dict):
        keys = weight_order(self.n_widths)
        missing = [k for k in keys if k not in state]
        if missing:
            raise KeyError(f"missing state_dict keys: {missing}")
        arrays = [_host_f32(state[k]) for k in keys]
        ptrs = (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])
        return arrays, ptrs

    def load_weights(self, state: dict) -> None:
        arrays, ptrs = self._pack(state)
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_load_weights(self._h, ptrs, len(arrays)), "vp3d_load_weights")

    # ---- shapes ----
    def receptive_field(self) -> int:
        return self._lib.vp3d_receptive_field(self._h)

    def total_causal_shift(self) -> int:
        return self._lib.vp3d_total_causal_shift(self._h)

    def out_frames(self, T: int) -> int:
        return self._lib.vp3d_out_frames(self._h, int(T))

    # ---- compute ----
    def reserve(self, B: int, T: int, dtype: str = "fp32") -> None:
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_reserve(self._h, int(B), int(T), N.DTYPES[dtype]), "vp3d_reserve")

    def forward(self, x: torch.Tensor, dtype: str = "fp32", out: torch.Tensor | None = None
                ) -> torch.Tensor:
        """x: (B, T, J_in, F) float32 on this handle's device -> (B, T', J_out, 3) float32."""
        if x.device != self.device:
            raise RuntimeError(f"input on {x.device}, model on {self.device}")
        if x.dtype != torch.float32:
            x = x.float()
        x = x.contiguous()
        B, T = int(x.shape[0]), int(x.shape[1])
        T_out = self.out_frames(T)
        if T_out < 1:
            raise RuntimeError(f"input of {T} frames is invalid for receptive field "
                               f"{self.receptive_field()}")
        if out is None:
            out = torch.empty((B, T_out, self.num_joints_out, 3), dtype=torch.float32,
                              device=self.device)
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_forward(self._h, x.data_ptr(), B, T, out.data_ptr(),
                                           N.DTYPES[dtype], N.stream_ptr(self.device)),
                    "vp3d_forward")
        return out

    def forward_windows(self, seqs, pairs: torch.Tensor, window: int, lead: int,
                        concat_cams: bool = False, dtype: str = "fp32",
                        out: torch.Tensor | None = None) -> torch.Tensor:
        """Forward of windows gathered on the fly from `seqs` (a pipeline.DeviceSequences):
        window b = frames [start_b - lead, start_b - lead + window) of sequence seq_b,
        edge-clamped; with concat_cams the 12 K.E channels follow each frame's keypoints
        (vp3d_forward_windows_pool: ChunkedGenerator batch + camera concat + TemporalModel forward,
        the gather fused into the expand conv on the 16-bit path).

        `seqs` also tells the library how many sequences are resident and how long the longest
        is.  An f16x3 forward without the camera concat whose windows outnumber the resident
        frames (table rows <= half the window rows, table < 2 GiB: large evaluation batches)
        then computes the expand conv once per resident frame into a table that block 1 reads
        through per-window row bases: the same poses, bit for bit.  On that path the f16x3
        range guard sees every resident frame of `seqs`, and a pair naming a sequence outside
        `seqs` is a fault (RuntimeError at the next forward or sync_status); starts outside their
        sequence are edge-clamped as on every path.  VP3D_EXPAND_TABLE=0 keeps the per-window expand; expand_table_mode() tells
        which path the last call took.

        Frame tables: with the expand table, blocks 1 .. d are computed once per resident frame
        position as well, as long as the table a block reads has at most half that block's
        window rows (d <= blocks - 1; the first per-window block reads the deepest table through
        the same row bases): still the same poses, bit for bit.  Where a table's launch is at
        least one round of tiles the rule is the measured one instead of "half": table rows <=
        window rows (table_depth_rule()).  VP3D_FRAME_TABLES=<d> forces a depth (0 = the expand
        table only; clamped to what the kernels' conditions allow); frame_table_depth() tells the
        depth the last call took.

        Trimmed layout: the tables hold the rows of the starts 0 .. max(lengths) - 1 only; starts
        before frame 0 or past the longest sequence stay exact through edge segments whose
        launches run only when the batch holds such a start, and such a batch makes the next
        call compute the wide layout (every start in one region).  The range guard sees the
        table rows computed, at every level: in the trimmed layout the rows of out-of-range
        starts only when the batch holds one.  VP3D_TABLE_TRIM=0|1 forces wide / trimmed;
        table_layout() tells which the last call took and whether its edge gate fired.

        Clamp-constant edge rows: a table row of blocks 1 .. d whose frames all lie at or before
        frame 0, or all at or after frame max(lengths) - 1, equals its neighbour towards the
        sequence, so each level's convs compute only the rows between those runs and a copy kernel
        fills the rest: still the same bits.  VP3D_TABLE_EDGES=0 computes every row;
        table_rows(level) tells the rows the last call computed."""
        def _idx(d):
            d = torch.device(d)
            return (d.type, d.index if d.index is not None else torch.cuda.current_device())
        if _idx(pairs.device) != _idx(self.device) or _idx(seqs.kps.device) != _idx(self.device):
            raise RuntimeError("pairs / sequences must live on the model's device")
        pairs = pairs.contiguous().to(torch.int32)
        B = int(pairs.shape[0])
        T_out = self.out_frames(window)
        if T_out < 1:
            raise RuntimeError(f"window of {window} frames is invalid for receptive field "
                               f"{self.receptive_field()}")
        cams = None
        if concat_cams:
            if seqs.cam is None:
                raise ValueError("no cameras loaded")
            cams = seqs.cam.data_ptr()
        if out is None:
            out = torch.empty((B, T_out, self.num_joints_out, 3), dtype=torch.float32,
                              device=self.device)
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_forward_windows_pool(
                self._h, seqs.kps.data_ptr(), seqs.f2, cams, seqs.seq_off.data_ptr(),
                seqs.seq_len.data_ptr(), int(seqs.n_seq), int(max(seqs.lengths)), pairs.data_ptr(), B,
                int(window), int(lead), out.data_ptr(), N.DTYPES[dtype], N.stream_ptr(self.device)),
                "vp3d_forward_windows")
        return out

    def expand_table_mode(self) -> int:
        """The path the last forward_windows took: 0 = the expand conv per window row, 1 = the
        expand table read by block 1 through indirect rows, 2 = the table with the windows' rows
        copied out (vp3d_expand_table_mode)."""
        return self._lib.vp3d_expand_table_mode(self._h)

    def frame_table_depth(self) -> int:
        """The frame-table depth of the last forward_windows: how many blocks were computed once
        per table row instead of once per window row, 0 = none (vp3d_frame_table_depth)."""
        return self._lib.vp3d_frame_table_depth(self._h)

    def table_layout(self):
        """(layout, edges) of the last forward_windows (vp3d_table_layout): layout 0 = no table,
        1 = wide (every start lo .. max_len - 1 + lead in one region per sequence), 2 = trimmed
        (the starts 0 .. max_len - 1; the others in gated edge segments); edges: whether its batch
        held a start outside 0 .. max_len - 1 after the edge clamp -- in the trimmed layout,
        whether its edge gate fired.  `edges` is valid once the forward has completed:
        synchronise first."""
        e = ctypes.c_int(0)
        layout = self._lib.vp3d_table_layout(self._h, ctypes.byref(e))
        return layout, bool(e.value)

    def table_rows(self, level: int):
        """(first_row, rows, pitch) of table level `level` in the last forward_windows
        (vp3d_table_rows; 0 = the expand table, l = block l's output): per sequence, the convs
        computed rows first_row .. first_row + rows - 1 of the level's `pitch` main-region rows,
        and the rows outside are copies of the first / last of them.  Raises for a level the call
        had no table of."""
        a, r, p = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        N.check(self._lib.vp3d_table_rows(self._h, int(level), ctypes.byref(a), ctypes.byref(r), ctypes.byref(p)),
                "vp3d_table_rows")
        return a.value, r.value, p.value

    def table_depth_rule(self):
        """(factor, num, den) of the tables' size rule (vp3d_table_depth_rule): a table is taken
        at nominal rows <= window rows // factor where its launch is shorter than one round of
        tiles, at nominal rows * den <= window rows * num otherwise."""
        f, n, d = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        self._lib.vp3d_table_depth_rule(ctypes.byref(f), ctypes.byref(n), ctypes.byref(d))
        return f.value, n.value, d.value

    # ---- f16x3 activation pre-scale ----
    def set_x3_prescale(self, p) -> None:
        """One power-of-two exponent per conv layer output (n_layers - 1: the shrink has none):
        layer l's f16x3 stored rows hold a * 2^p[l] (vp3d_set_x3_prescale).  None or all zeros
        clears it.  Raises on a wrong length, |p| > 24 or a vector breaking the residual chain."""
        n = self.n_layers - 1
        vals = [0] * n if p is None else [int(v) for v in p]
        arr = (ctypes.c_int32 * len(vals))(*vals)
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_set_x3_prescale(self._h, arr, len(vals)), "vp3d_set_x3_prescale")

    def x3_prescale(self) -> List[int]:
        n = self.n_layers - 1
        arr = (ctypes.c_int32 * n)()
        N.check(self._lib.vp3d_get_x3_prescale(self._h, arr, n), "vp3d_get_x3_prescale")
        return list(arr)

    def calibrate_x3(self, x: torch.Tensor | None = None, *, seqs=None, pairs: torch.Tensor | None = None,
                     window: int | None = None, lead: int = 0, concat_cams: bool = False) -> List[dict]:
        """Per-layer statistics of the fp32 forward (vp3d_x3_calibrate) on x: (B, T, J_in, F), or
        on the windows `pairs` gathers from `seqs` (as forward_windows).  One dict per conv
        layer output: absmax, rms, small_share (the share of non-zero values under 2^-3)."""
        n = self.n_layers - 1
        stats = (N.vp3d_act_stats * n)()
        if x is not None:
            if x.device != self.device:
                raise RuntimeError(f"input on {x.device}, model on {self.device}")
            x = x.float().contiguous()
            with torch.cuda.device(self.device):
                N.check(self._lib.vp3d_x3_calibrate(self._h, x.data_ptr(), int(x.shape[0]), int(x.shape[1]),
                                                    stats, N.stream_ptr(self.device)), "vp3d_x3_calibrate")
        else:
            if seqs is None or pairs is None or window is None:
                raise ValueError("calibrate_x3 takes x, or seqs + pairs + window")
            if pairs.device != self.device or seqs.kps.device != self.device:
                raise RuntimeError("pairs / sequences must live on the model's device")
            pairs = pairs.contiguous().to(torch.int32)
            cams = None
            if concat_cams:
                if seqs.cam is None:
                    raise ValueError("no cameras loaded")
                cams = seqs.cam.data_ptr()
            with torch.cuda.device(self.device):
                N.check(self._lib.vp3d_x3_calibrate_windows(
                    self._h, seqs.kps.data_ptr(), seqs.f2, cams, seqs.seq_off.data_ptr(),
                    seqs.seq_len.data_ptr(), pairs.data_ptr(), int(pairs.shape[0]), int(window), int(lead),
                    stats, N.stream_ptr(self.device)), "vp3d_x3_calibrate_windows")
        return [dict(layer=i, absmax=s.absmax, rms=s.rms, small_share=s.small_share) for i, s in enumerate(stats)]

    def sync_status(self) -> None:
        """Synchronise the current stream; raise RuntimeError once if a launch of this lifter
        reported a device-side fault, and clear it (vp3d_sync_status).  The fault kinds:
          * split-K timeout -- an owner tile of a split partial round stopped waiting for its
            helper units (its outputs are wrong); refuses EVERY forward until cleared here;
          * f16x3 range / non-finite -- an activation split into f16 halves was past |x| <=
            65,504, or the poses came out non-finite; refuses f16x3 forwards only (run those
            inputs in fp32).
        A forward raises a pending fault of an earlier forward at entry; the last forward of
        a run is only checked by calling this (vp3d_amd.evaluate does, after its loop)."""
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_sync_status(self._h, N.stream_ptr(self.device)), "vp3d_sync_status")

    # ---- profiling ----
    def profile(self, enable: bool) -> None:
        N.check(self._lib.vp3d_profile_enable(self._h, 1 if enable else 0))

    def profile_layers(self, layers=None) -> None:
        """Time only `layers` (indices; None = all) while profiling is enabled."""
        mask = (1 << 64) - 1 if layers is None else sum(1 << int(i) for i in layers)
        N.check(self._lib.vp3d_profile_layers(self._h, mask))

    def profile_reset(self) -> None:
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_profile_reset(self._h))

    def profile_read(self):
        n = self.n_layers
        ms = (ctypes.c_double * n)()
        cnt = (ctypes.c_int64 * n)()
        fl = (ctypes.c_double * n)()
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_profile_read(self._h, ctypes.addressof(ms),
                                                ctypes.addressof(cnt), ctypes.addressof(fl)))
        return [dict(layer=i, ms_total=ms[i], launches=cnt[i], flop=fl[i]) for i in range(n)]

    def close(self) -> None:
        if self._h:
            self._lib.vp3d_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
