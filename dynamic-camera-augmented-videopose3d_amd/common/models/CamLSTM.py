"""Drop-in for the reference's ``common/models/CamLSTM.py``.

Same classes, constructor arguments, submodules and state_dict keys as
Bart-Weil/Dynamic-Camera-Augmented-VideoPose3D common/models/CamLSTM.py:

  CamLSTMBase     :11-44    ``sliding_window(inputs_2d, inputs_cam, window_size)``
  CoupledLSTM     :47-129   concat [2D | K.E] -> nn.LSTM (num_cells, zero state) -> last step
                            -> bn_lstm -> MLP head (Linear, BatchNorm1d, LeakyReLU, Dropout)*
  UncoupledLSTM   :132-257  raises NotImplementedError at construction, like the reference

Eval-mode ``forward`` / ``sliding_window`` on HIP tensors run libvp3d.so
(``vp3d_seq_forward`` / ``vp3d_seq_sliding_window``): the layer-0 input projection once per
frame on the f32 MFMA GEMM, the stacked recurrence in one persistent kernel per tile of 16
windows (csrc/seq_lifter.hip ``lstm_kernel``), the eval BatchNorms folded into the head's
GEMM epilogues.  CPU inputs and train mode raise.

Training is opt-in: after ``model.enable_native_training()`` a train-mode ``forward`` on HIP
tensors runs the native training step (``vp3d_seq_train_forward`` / ``vp3d_seq_train_backward``
through the autograd node ``vp3d_amd.seq_train.SeqTrainStep``), so the reference's loop
(run.py:451-487) runs unchanged; without the call train mode raises as before.
"""
import torch
import torch.nn as nn

from vp3d_amd import _native as _N
from vp3d_amd.seq_lifter import NativeSeqLifter, NativeSeqModule
from vp3d_amd.seq_train import NativeSeqTrainer, SeqTrainStep, fresh_seed

__all__ = ["CamLSTMBase", "CoupledLSTM", "UncoupledLSTM"]


class CamLSTMBase(NativeSeqModule, nn.Module):
    """Shared attributes and ``sliding_window`` (CamLSTM.py:11-44)."""

    cam_mat_shape = (3, 4)

    def __init__(self, num_joints_in, in_features, num_joints_out, out_features, hidden_size, num_cells,
                 head_layers, dropout=0.25):
        super().__init__()
        self.num_joints_in = num_joints_in
        self.in_features = in_features
        self.num_joints_out = num_joints_out
        self.out_features = out_features
        self.hidden_size = hidden_size
        self.num_cells = num_cells
        self.head_layers = head_layers
        self.dropout = dropout

    def sliding_window(self, inputs_2d, inputs_cam, window_size):
        _, T, J, _ = inputs_2d.shape
        if T - window_size + 1 <= 0:
            raise ValueError("window_size larger than sequence length")
        self._check_eval(inputs_2d)
        return self.native_lifter(inputs_2d.device).sliding_window(inputs_2d, inputs_cam, window_size)


class CoupledLSTM(CamLSTMBase):
    """Stacked-LSTM lifter over a window of [2D keypoints | camera matrix] frames (CamLSTM.py:47-129)."""

    def __init__(self, num_joints_in, in_features, num_joints_out, out_features, hidden_size, num_cells,
                 head_layers, dropout=0.25):
        super().__init__(num_joints_in, in_features, num_joints_out, out_features, hidden_size, num_cells,
                         head_layers, dropout)
        cin = num_joints_in * in_features + self.cam_mat_shape[0] * self.cam_mat_shape[1]
        self.lstm_layers = nn.LSTM(cin, hidden_size, num_cells, batch_first=True, dropout=dropout)
        self.bn_lstm = nn.BatchNorm1d(hidden_size)
        self.bn_layers = [self.bn_lstm]
        head = []
        width = hidden_size
        for h in head_layers:
            bn = nn.BatchNorm1d(h)
            self.bn_layers.append(bn)
            head += [nn.Linear(width, h), bn, nn.LeakyReLU(), nn.Dropout(dropout)]
            width = h
        head.append(nn.Linear(width, out_features * num_joints_out))
        self.mlp_layers = nn.Sequential(*head)
        self._native_training = False
        self._seq_trainers = {}

    def set_bn_momentum(self, momentum):
        for bn in self.bn_layers:
            bn.momentum = momentum

    def _make_native(self, state, device):
        return NativeSeqLifter(_N.SEQ_LSTM, self.num_joints_in, self.in_features, self.num_joints_out,
                               self.out_features, self.hidden_size, self.num_cells, self.head_layers, state, device,
                               eps=self.bn_lstm.eps)

    def forward(self, input_2d, input_cam):
        assert len(input_2d.shape) == 4 and len(input_cam.shape) == 4
        assert input_2d.shape[-2] == self.num_joints_in
        assert input_2d.shape[-1] == self.in_features
        assert input_cam.shape[-2] == self.cam_mat_shape[0]
        assert input_cam.shape[-1] == self.cam_mat_shape[1]
        if self.training and self._native_training and input_2d.is_cuda:
            return self._train_forward(input_2d, input_cam)
        self._check_eval(input_2d)
        return self.native_lifter(input_2d.device).forward(input_2d, input_cam)

    def enable_native_training(self):
        """Opt in to the native training step: from now on a train-mode ``forward`` on HIP tensors
        runs ``vp3d_amd.seq_train.SeqTrainStep`` (nn.LSTM's inter-layer dropout, BatchNorm batch
        statistics with the running-stat update, the head's LeakyReLU and dropout, and the backward
        through time, in f32 on the device) instead of raising.  Returns self."""
        self._native_training = True
        return self

    def native_seq_trainer(self, device) -> NativeSeqTrainer:
        """The NativeSeqTrainer (train-mode forward/backward engine) for `device`."""
        device = torch.device(device)
        cached = self._seq_trainers.get(str(device))
        if cached is None:
            cached = NativeSeqTrainer(self.num_joints_in, self.in_features, self.num_joints_out, self.out_features,
                                      self.hidden_size, self.num_cells, self.head_layers, device,
                                      eps=self.bn_lstm.eps)
            self._seq_trainers[str(device)] = cached
        return cached

    def _train_forward(self, input_2d, input_cam):
        if input_2d.shape[0] < 2:
            raise ValueError("Expected more than 1 value per channel when training, got input size "
                             f"{[int(input_2d.shape[0]), self.hidden_size]}")
        for bn in self.bn_layers:
            if bn.momentum is None:
                raise ValueError("vp3d: native CoupledLSTM training needs a BatchNorm momentum "
                                 "(momentum=None, the cumulative average, is not built)")
            if not bn.track_running_stats or not bn.affine:
                raise ValueError("vp3d: native CoupledLSTM training needs affine BatchNorms that track "
                                 "running statistics")
        state = self.state_dict(keep_vars=True)
        tensors = [v for k, v in state.items() if not k.endswith("num_batches_tracked")]
        for t in tensors:
            if t.device != input_2d.device or t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError("vp3d: parameters must be contiguous float32 tensors on the input's device")
        if input_cam.device != input_2d.device:
            raise RuntimeError(f"input_cam on {input_cam.device}, input_2d on {input_2d.device}")
        trainable = tuple(isinstance(t, nn.Parameter) and t.requires_grad for t in tensors)
        trainer = self.native_seq_trainer(input_2d.device)
        # BatchNorm1d.forward counts the batch
        for bn in self.bn_layers:
            bn.num_batches_tracked.add_(1)
        momenta = tuple(float(bn.momentum) for bn in self.bn_layers)
        p = float(self.dropout)
        seed = fresh_seed() if p > 0 else 0
        return SeqTrainStep.apply(trainer, p, momenta, seed, trainable, input_2d.contiguous().float(),
                                  input_cam.contiguous().float(), *tensors)


class UncoupledLSTM(CamLSTMBase):
    """Not implemented on the reference's main branch either (CamLSTM.py:150)."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("UncoupledLSTM data pipeline not implemented on main branch, "
                                  "use uncoupled-lstm branch instead")
