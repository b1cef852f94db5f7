"""Python side of the StackedPoseLifter ensemble (reference common/models/StackedPoseLifter.py,
run.py:241-288 build, :714-729 evaluate).

`NativeStackedLifter` owns a native handle (vp3d_stacked, include/vp3d.h): one packed device
copy of the MLP's weights; the whole chain of Linears is one kernel launch.  It computes
nothing itself.  `NativeStackedModule` is the mixin the drop-in
`common.models.StackedPoseLifter` uses to keep that handle in step with its parameters.
`StackedEnsemble` holds the three models of `--use-model StackedPoselifter` and yields the
three predictions of one generator batch to `vp3d_amd.evaluate.evaluate`.
"""
from __future__ import annotations

import ctypes
from typing import Callable, Dict, List

import torch

from . import _native as N
from .seq_lifter import _host_f32


class NativeStackedLifter:
    def __init__(self, num_joints: int, features: int, num_layers: int, layer_size: int, state: dict, device):
        self._h = ctypes.c_void_p()
        self._lib = N.load()
        cfg = N.vp3d_stacked_cfg()
        cfg.num_joints, cfg.features = int(num_joints), int(features)
        cfg.num_layers, cfg.layer_size = int(num_layers), int(layer_size)
        self.cfg = cfg
        self.num_joints, self.features = int(num_joints), int(features)
        self.device = torch.device(device)
        arrays = [_host_f32(v) for v in state.values()]
        ptrs = (ctypes.c_void_p * max(len(arrays), 1))(*[a.ctypes.data for a in arrays])
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_stacked_create(ctypes.byref(cfg), ptrs, len(arrays), ctypes.byref(self._h)),
                    "vp3d_stacked_create")

    def forward(self, y_transformer: torch.Tensor, y_fcn: torch.Tensor) -> torch.Tensor:
        """Two (n, J * F) tensors -> (n, 1, J, F)."""
        rows = []
        for t in (y_transformer, y_fcn):
            if t.device != self.device:
                raise RuntimeError(f"input on {t.device}, model on {self.device}")
            rows.append(t.contiguous().float())
        n = int(rows[0].shape[0])
        y = torch.empty((n, 1, self.num_joints, self.features), device=self.device)
        if n == 0:
            return y
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_stacked_forward(self._h, rows[0].data_ptr(), rows[1].data_ptr(), n, y.data_ptr(),
                                                   N.stream_ptr(self.device)), "vp3d_stacked_forward")
        return y

    def close(self):
        if self._h:
            self._lib.vp3d_stacked_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NativeStackedModule:
    """Mixin for the drop-in StackedPoseLifter: a NativeStackedLifter per device, re-packed
    whenever a parameter was replaced or modified in place (as NativeSeqModule does)."""

    def _native_key(self, device):
        return (str(device),) + tuple((t.data_ptr(), t._version) for t in self.state_dict(keep_vars=True).values())

    def native_lifter(self, device) -> NativeStackedLifter:
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("vp3d: the stacked pose lifter runs on the MI355X kernel only (no CPU fallback)")
        key = self._native_key(device)
        cached = getattr(self, "_native", None)
        if cached is not None and cached[0] == key:
            return cached[1]
        lifter = NativeStackedLifter(self.num_joints, self.features, self.num_layers, self.layer_size,
                                     dict(self.state_dict()), device)
        self._native = (key, lifter)
        return lifter


class StackedEnsemble:
    """The three models of --use-model StackedPoselifter (run.py:241-288) behind one call.

    `predict(inputs_2d, inputs_cam, seq_length)` restates run.py:715-720 for one sequence:
    the transformer's sliding-window prediction, the FCN's prediction, and the MLP on the two,
    each (1, T, J, F).  Quirk Q12: the two predictions are reshaped to (-1, J * F) explicitly, so
    a one-frame sequence works (the reference's .squeeze() drops its frame axis too).

    The three members are callables, so a CPU test can drive the evaluation loop with oracle
    functions: transformer(inputs_2d, inputs_cam, seq_length), fcn(inputs_2d),
    stacked(y_transformer, y_fcn).  nn.Modules are adapted by `from_modules`.

    `evaluate` appends the two per-sequence P-MPJPE differences (run.py:726-729, metres) to
    `fcn_diffs` / `transformer_diffs`: one list per `begin_action` call.
    """

    def __init__(self, transformer: Callable, fcn: Callable, stacked: Callable, sync: Callable | None = None):
        self.transformer, self.fcn, self.stacked = transformer, fcn, stacked
        self._sync = sync
        self.fcn_diffs: Dict[str, List[float]] = {}
        self.transformer_diffs: Dict[str, List[float]] = {}
        self._action = None

    @classmethod
    def from_modules(cls, model_transformer, model_fcn, model_stacked):
        """Quirk Q10: all three run in eval mode (the reference leaves the two sub-models in
        train mode: dropout active, BatchNorm batch statistics)."""
        for m in (model_transformer, model_fcn, model_stacked):
            m.eval()
        return cls(model_transformer.sliding_window, model_fcn, model_stacked,
                   sync=getattr(model_fcn, "sync_status", None))

    def begin_action(self, action):
        self._action = action
        self.fcn_diffs[action] = []
        self.transformer_diffs[action] = []

    def predict(self, inputs_2d, inputs_cam, seq_length):
        y_t = self.transformer(inputs_2d, inputs_cam, seq_length)
        y_f = self.fcn(inputs_2d)
        J, F = y_f.shape[-2], y_f.shape[-1]
        if y_t.shape[-2:] != y_f.shape[-2:] or y_t.numel() != y_f.numel():
            raise AssertionError(f"transformer prediction {tuple(y_t.shape)} and FCN prediction "
                                 f"{tuple(y_f.shape)} differ")
        y = self.stacked(y_t.reshape(-1, J * F), y_f.reshape(-1, J * F))
        return y_t, y_f, y.reshape(y_f.shape)

    def record(self, metrics, y_t, y_f, y):
        """p_mpjpe(fcn, stacked) and p_mpjpe(transformer, stacked) of one sequence (run.py:722-729)."""
        if self._action not in self.fcn_diffs:
            self.begin_action(self._action)
        J, F = y.shape[-2], y.shape[-1]
        flat = [t.reshape(-1, J, F) for t in (y_f, y_t, y)]
        self.fcn_diffs[self._action].append(float(metrics.p_mpjpe(flat[0], flat[2])))
        self.transformer_diffs[self._action].append(float(metrics.p_mpjpe(flat[1], flat[2])))

    def sync_status(self):
        if callable(self._sync):
            self._sync()
