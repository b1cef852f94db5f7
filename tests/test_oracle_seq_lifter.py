"""Oracle of the trajectory lifters (oracle/seq_lifter_ref.py) against the reference's own
eval-mode CoupledTransformer / CoupledLSTM outputs (tests/golden/cam_*.npz): forward on
243-frame windows and sliding_window over a padded sequence; and, over every case of
tests/seq_cases.py (the shapes and seeded non-trivial weights of tests/test_gpu_seq_shapes.py),
against torch's own nn.Linear / nn.LayerNorm / nn.TransformerEncoder / nn.LSTM modules on the CPU."""
import json
import os

import numpy as np
import pytest
import torch

import seq_cases as SC
from oracle.seq_lifter_ref import lstm_forward, sliding_windows, transformer_forward

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def load(name):
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(g["meta"]))
    return g, meta, {k[2:]: g[k] for k in g.files if k.startswith("w/")}


def _run(kind, state, meta, x2d, xcam):
    if kind == "transformer":
        return transformer_forward(state, x2d, xcam, meta["n_heads"], meta["num_layers"], len(meta["head_layers"]))
    return lstm_forward(state, x2d, xcam, meta["hidden_size"], meta["num_cells"], len(meta["head_layers"]))


@pytest.mark.parametrize("name,kind", [("cam_transformer", "transformer"), ("cam_lstm", "lstm")])
def test_oracle_matches_reference(name, kind):
    torch.set_num_threads(8)
    g, meta, state = load(name)
    y = _run(kind, state, meta, g["x2d"], g["xcam"]).numpy()
    np.testing.assert_allclose(y, g["y"], atol=2e-6, rtol=0)
    w2, wc = sliding_windows(g["seq2d"], g["seqcam"], meta["window"])
    ys = _run(kind, state, meta, w2, wc).numpy().reshape(g["yseq"].shape)
    np.testing.assert_allclose(ys, g["yseq"], atol=2e-6, rtol=0)


@pytest.mark.parametrize("run_id", SC.RUN_IDS)
def test_oracle_matches_torch_modules_on_shape_cases(run_id):
    """The float32 oracle within 1e-5 of the drop-in's real nn submodules composed in eval mode;
    and its own error against float64 (e_ref, the yardstick of the GPU gate) below 3e-6, so that
    no case's gate `e_gpu <= c * e_ref` goes slack (largest seen: see the printed values)."""
    torch.set_num_threads(8)
    _, kind, name, cfg, mode, W, n = SC.RUNS[SC.RUN_IDS.index(run_id)]
    w2, wc = SC.windows(mode, W, *(torch.tensor(a) for a in SC.run_inputs(name, mode, W, n)))
    y_torch = SC.torch_modules_forward(kind, SC.make_module(kind, name, cfg), w2, wc).double().numpy()
    y32 = SC.oracle_output(run_id, torch.float32)
    e_torch = float(np.abs(y32 - y_torch).max())
    e_ref = SC.reference_error(run_id)
    rms = float(np.sqrt(np.mean(SC.oracle_output(run_id, torch.float64) ** 2)))
    print(f"{run_id}: |oracle32 - torch| {e_torch:.3e}  e_ref {e_ref:.3e}  output rms {rms:.3f}")
    assert y_torch.shape == y32.shape
    assert e_torch <= 1e-5
    assert 0.0 < e_ref < 3e-6
