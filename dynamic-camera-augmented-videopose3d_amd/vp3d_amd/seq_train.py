"""Training step of the CoupledLSTM trajectory lifter on the MI355X kernels (opt-in).

The reference trains ``CoupledLSTM`` (common/models/CamLSTM.py:47-129) in train mode inside
run.py's loop (run.py:451-487): ``model(batch_2d, batch_cam)`` with nn.LSTM's inter-layer
dropout, BatchNorm batch statistics and the head's dropout, mpjpe, ``loss.backward()``,
``optim.Adam(..., amsgrad=True).step()`` (run.py:662).

* `NativeSeqTrainer` owns a ``vp3d_seq_trainer`` (include/vp3d.h): the f32 train-mode forward
  and the backward through time run in libvp3d.so; the parameters stay in the module's own
  tensors and are passed by device pointer on every call.
* `SeqTrainStep` is the autograd node ``CoupledLSTM.forward`` uses in train mode once
  ``model.enable_native_training()`` was called, so a reference training loop
  (``loss.backward()``, any torch optimiser, or `vp3d_amd.train.Adam`) runs unchanged.
"""
from __future__ import annotations

import ctypes
from typing import List, Sequence

import torch
from torch.autograd.graph import increment_version

from . import _native as N
from .train import _ptrs


class NativeSeqTrainer:
    """One vp3d_seq_trainer on one HIP device (geometry of one CoupledLSTM configuration)."""

    ROLES = ("recurrence_forward", "backward_through_time", "weight_gradients", "head_elementwise")

    def __init__(self, num_joints_in: int, in_features: int, num_joints_out: int, out_features: int,
                 hidden_size: int, num_cells: int, head_layers: Sequence[int], device, eps: float = 1e-5,
                 kind: int = N.SEQ_LSTM):
        self._lib = N.load()
        cfg = N.vp3d_seq_cfg()
        cfg.kind = kind
        cfg.num_joints_in, cfg.in_features = num_joints_in, in_features
        cfg.num_joints_out, cfg.out_features = num_joints_out, out_features
        cfg.d_model, cfg.num_layers = hidden_size, num_cells
        if not 1 <= len(head_layers) <= N.SEQ_MAX_HEAD:
            raise AssertionError(f"1..{N.SEQ_MAX_HEAD} head layers are supported")
        cfg.n_head_layers = len(head_layers)
        for i, v in enumerate(head_layers):
            cfg.head_layers[i] = int(v)
        cfg.eps = eps
        self.cfg = cfg
        self.head_layers = [int(v) for v in head_layers]
        self.hidden_size, self.num_cells = hidden_size, num_cells
        self.num_joints_out, self.out_features = num_joints_out, out_features
        self.device = torch.device(device)
        self.generation = 0
        self._B = self._T = -1
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_seq_trainer_create(ctypes.byref(cfg), ctypes.byref(self._h)),
                    "vp3d_seq_trainer_create")
        self.n_params = self._lib.vp3d_seq_weight_count(ctypes.byref(cfg))

    def running_stat_indices(self) -> List[int]:
        """Positions of running_mean / running_var in the parameter table (vp3d_seq_weight_count
        order): bn_lstm's after the cells, then each head layer's after its Linear and BN affine."""
        base = 4 * self.num_cells
        out = [base + 2, base + 3]
        for j in range(len(self.head_layers)):
            out += [base + 4 + 6 * j + 4, base + 4 + 6 * j + 5]
        return out

    def store_bytes(self, B: int, T: int) -> int:
        return int(self._lib.vp3d_seq_train_bytes(ctypes.byref(self.cfg), B, T))

    def forward(self, x2d: torch.Tensor, xcam: torch.Tensor, params: Sequence[torch.Tensor], p: float,
                momenta: Sequence[float], seed: int) -> torch.Tensor:
        """Train-mode forward.  params: the state_dict tensors in order, without the
        num_batches_tracked counters (running stats are updated in place).  Returns y
        (B, 1, J_out, out_features)."""
        assert len(params) == self.n_params, (len(params), self.n_params)
        B, T = int(x2d.shape[0]), int(x2d.shape[1])
        if B < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size "
                             f"{[B, self.hidden_size]}")
        y = torch.empty((B, 1, self.num_joints_out, self.out_features), dtype=torch.float32, device=self.device)
        mom = (ctypes.c_double * len(momenta))(*[float(m) for m in momenta])
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_seq_train_forward(self._h, _ptrs(params), len(params), x2d.data_ptr(),
                                                     xcam.data_ptr(), B, T, float(p), mom,
                                                     int(seed) & (2 ** 64 - 1), y.data_ptr(),
                                                     N.stream_ptr(self.device)), "vp3d_seq_train_forward")
        self._B, self._T = B, T
        # the running statistics were written through raw pointers: bump their version counters so
        # caches keyed on them (the eval lifter's packed weights) see the change
        increment_version([params[i] for i in self.running_stat_indices()])
        self.generation += 1
        return y

    def backward(self, params: Sequence[torch.Tensor], dy: torch.Tensor,
                 trainable: Sequence[bool]) -> List[torch.Tensor | None]:
        grads = [torch.empty_like(t) if tr else None for t, tr in zip(params, trainable)]
        dy = dy.contiguous().float()
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_seq_train_backward(self._h, _ptrs(params), len(params), dy.data_ptr(),
                                                      _ptrs(grads), N.stream_ptr(self.device)),
                    "vp3d_seq_train_backward")
        return grads

    def n_sites(self) -> int:
        return self.num_cells - 1 + len(self.head_layers)

    def site_shape(self, site: int) -> tuple:
        if self._B < 0:
            raise RuntimeError("no train-mode forward yet")
        if site < self.num_cells - 1:
            return (self._B, self._T, self.hidden_size)
        return (self._B, self.head_layers[site - (self.num_cells - 1)])

    def mask(self, site: int, which: int = 0) -> torch.Tensor:
        """Test hook, latest forward: the dropout keep mask (which = 0) or the LeakyReLU side
        (which = 1: BN output > 0, head sites) of mask site `site` (uint8)."""
        out = torch.empty(self.site_shape(site), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_seq_train_mask(self._h, site, which, out.numel(), out.data_ptr(),
                                                  N.stream_ptr(self.device)), "vp3d_seq_train_mask")
        return out

    def profile(self, on: bool) -> dict:
        """Measurement: the device milliseconds per role (ROLES) of the steps run since profiling
        was switched on, then switch it on or off (vp3d_seq_train_profile; synchronises)."""
        ms = (ctypes.c_double * 4)()
        with torch.cuda.device(self.device):
            N.check(self._lib.vp3d_seq_train_profile(self._h, 1 if on else 0, ms), "vp3d_seq_train_profile")
        return dict(zip(self.ROLES, [float(v) for v in ms]))

    def close(self) -> None:
        if self._h:
            self._lib.vp3d_seq_trainer_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SeqTrainStep(torch.autograd.Function):
    """y = CoupledLSTM(x2d, xcam) in train mode; the backward yields every parameter's gradient."""

    @staticmethod
    def forward(ctx, trainer: NativeSeqTrainer, p: float, momenta: tuple, seed: int, trainable: tuple,
                x2d: torch.Tensor, xcam: torch.Tensor, *state: torch.Tensor):
        y = trainer.forward(x2d, xcam, state, p, momenta, seed)
        ctx.trainer = trainer
        ctx.generation = trainer.generation
        ctx.trainable = trainable
        # the trained parameters must be the ones the backward sees (the trainer keeps the
        # activations); an optimiser step in between fails torch's saved-tensor check, a second
        # forward is reported by the generation check below (as vp3d_amd.train.TrainStep)
        ctx.save_for_backward(*[t for t, tr in zip(state, trainable) if tr])
        ctx.state = state
        return y

    @staticmethod
    def backward(ctx, dy):
        trainer = ctx.trainer
        if trainer.generation != ctx.generation:
            raise RuntimeError("vp3d: another train-mode forward of this model ran before this backward; "
                               "the native trainer keeps the activations of the latest forward only")
        ctx.saved_tensors  # version check of the trained parameters
        grads = trainer.backward(ctx.state, dy, ctx.trainable)
        return (None, None, None, None, None, None, None, *grads)


def fresh_seed() -> int:
    """A mask seed from torch's CPU generator, so torch.manual_seed reproduces a run."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())
