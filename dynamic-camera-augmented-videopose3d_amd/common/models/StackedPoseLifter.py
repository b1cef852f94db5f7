"""Drop-in for the reference's ``common/models/StackedPoseLifter.py``.

Same class, constructor arguments, attributes, ``mlp_layers`` ModuleList and state_dict keys
(``mlp_layers.{0, 3, 6, ...}.{weight, bias}``) as
Bart-Weil/Dynamic-Camera-Augmented-VideoPose3D common/models/StackedPoseLifter.py:4-56: the MLP
that fuses the CoupledTransformer prediction and the TemporalModel prediction of a frame,

  Linear(2 J F, layer_size), ReLU, Dropout, num_layers x [Linear(layer_size, layer_size), ReLU,
  Dropout], Linear(layer_size, J F)

The nn modules only hold the parameters.  Eval-mode ``forward`` on HIP tensors runs
libvp3d.so (``vp3d_stacked_forward``, csrc/stacked_lifter.hip): the whole chain in one launch on
the exact-f32 MFMA, activations in LDS.  CPU inputs raise; train mode raises (training the
ensemble is not on the MI355X path).
"""
import torch
import torch.nn as nn

from vp3d_amd.stacked import NativeStackedModule

__all__ = ["StackedPoseLifter"]


class StackedPoseLifter(NativeStackedModule, nn.Module):

    def __init__(self, num_joints: int, features: int, num_layers: int, layer_size: int, dropout: float = 0.25):
        super().__init__()
        self.num_joints = num_joints
        self.features = features
        self.num_layers = num_layers
        self.layer_size = layer_size

        mlp_layers = [nn.Linear(num_joints * features * 2, layer_size), nn.ReLU(inplace=True), nn.Dropout(dropout)]
        for _ in range(num_layers):
            mlp_layers += [nn.Linear(layer_size, layer_size), nn.ReLU(inplace=True), nn.Dropout(dropout)]
        mlp_layers.append(nn.Linear(layer_size, num_joints * features))
        self.mlp_layers = nn.ModuleList(mlp_layers)
        self.dropout = nn.Dropout(dropout)

    def forward(self, input_3d_transformer: torch.Tensor, input_3d_FCN: torch.Tensor):
        """(B, 1, J, features) or (B, J, features) or (B, J * features), twice -> (B, 1, J, features)
        (StackedPoseLifter.py:37-56; transformer first in the concatenation, :49)."""
        width = self.num_joints * self.features
        rows = []
        for t in (input_3d_transformer, input_3d_FCN):
            assert t.dim() >= 2 and t.numel() == t.shape[0] * width, \
                f"Unexpected input shape {tuple(t.shape)} for {self.num_joints} joints x {self.features} features"
            if t.dim() > 2:
                assert t.shape[-2] == self.num_joints and t.shape[-1] == self.features, \
                    f"Unexpected input shape {tuple(t.shape)} for {self.num_joints} joints x {self.features} features"
            rows.append(t.reshape(t.shape[0], width))
        assert rows[0].shape[0] == rows[1].shape[0], "Batch sizes of the two predictions differ"
        if not (rows[0].is_cuda and rows[1].is_cuda):
            raise RuntimeError("vp3d: the stacked pose lifter runs on the MI355X kernel only (no CPU fallback); "
                               "call model.cuda() and pass CUDA tensors")
        if self.training:
            raise NotImplementedError("vp3d: training the stacked pose lifter is not on the MI355X path "
                                      "(the eval-mode forward is); call model.eval()")
        return self.native_lifter(rows[0].device).forward(rows[0], rows[1])
