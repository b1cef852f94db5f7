"""run.py --use-model StackedPoselifter --evaluate on the MI355X, end to end (reference
run.py:241-288 build, :411-417 checkpoint, :714-729 evaluate, :985-987 the diff lines): three
run.py-style checkpoints written with torch.save from the fixture weights and read back by the
weights-only loader, device generator, native transformer sliding window, native FCN (fp32),
the fused MLP kernel and the native metrics, against tests/golden/run_eval_stacked.npz.
"""
import re

import numpy as np
import pytest
import torch

import stacked_common as SC

pytestmark = pytest.mark.gpu


def test_run_main_stacked_matches_reference(tmp_path, capsys):
    import run
    from common.models.CamTransformer import PositionalEncoding
    from common.models.TemporalModel import TemporalModel
    from vp3d_amd import synth
    gold = SC.run_eval_golden()
    meta = gold["meta"]
    fcn = TemporalModel(17, 2, 17, meta["fw"], channels=meta["channels"])
    fcn_sd = synth.lifter_state_dict([(k, tuple(v.shape)) for k, v in fcn.state_dict().items()], seed=meta["seed"])
    tsd = {k: torch.from_numpy(np.asarray(v)) for k, v in SC.transformer_state().items()}
    tsd["positional_encoding.pe"] = PositionalEncoding(128).pe
    weights = tmp_path / "elsewhere"  # the sub-models' paths are used as given, not joined with -c
    weights.mkdir()
    ckpt = tmp_path / "ckpt"
    ckpt.mkdir()
    torch.save({"epoch": 5, "model_pos": tsd}, weights / "transformer.bin")
    torch.save({"epoch": 7, "model_pos": {k: torch.from_numpy(v) for k, v in fcn_sd.items()}}, weights / "fcn.bin")
    torch.save({"epoch": 2, "model_pos": {k: torch.from_numpy(v) for k, v in gold["mlp"].items()}},
               ckpt / "stacked.bin")
    res = run.main(SC.run_argv(meta) + ["--evaluate", "stacked.bin", "-c", str(ckpt),
                                        "--transformer-weights", str(weights / "transformer.bin"),
                                        "--fcn-weights", str(weights / "fcn.bin")])
    out = capsys.readouterr().out
    print(out)
    SC.check_run_result(res, gold)
    # the two printed lines carry the same values (metres under the reference's 'mm' label)
    last = gold["actions"][-1]
    for label, key in (("FCN Diff", "fcn_diffs"), ("Transformer Diff", "transformer_diffs")):
        m = re.search(label + r"\s+\(P-MPJPE\): (\S+) mm", out)
        assert m, out
        assert abs(float(m.group(1)) - np.mean(gold[key][last])) * 1000 <= 1e-3


def test_run_main_stacked_synthetic_default(capsys):
    """--evaluate synthetic at the default sizes: 1024-channel FCN in the default compute dtype,
    the default transformer, the 256 x 3 MLP."""
    import run
    res = run.main(["--use-model", "StackedPoselifter", "--evaluate", "synthetic", "--synthetic-frames", "120"])
    out = capsys.readouterr().out
    for line in ("Protocol #1   (MPJPE) action-wise average:", "Protocol #2 (P-MPJPE) action-wise average:",
                 "Protocol #3 (N-MPJPE) action-wise average:", "Velocity      (MPJVE) action-wise average:",
                 "PMCC (MPJPE and cam velocity):", "FCN Diff                        (P-MPJPE):",
                 "Transformer Diff                (P-MPJPE):"):
        assert line in out, line
    assert len(res["per_action"]) == 3
    for k, v in res["per_action"].items():
        assert np.isfinite(np.asarray(v)).all(), (k, v)
        assert np.isfinite(res["ensemble_diffs"]["fcn"][k]).all()
        assert np.isfinite(res["ensemble_diffs"]["transformer"][k]).all()
    assert np.isfinite(list(res["ensemble_diffs"]["printed"].values())).all()
    torch.cuda.synchronize()
