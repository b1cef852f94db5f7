"""run.py --use-model LSTM-Coupled without --evaluate on the MI355X: the reference's epoch loop
(run.py:424-590; model(batch_2d, batch_cam) :470-471, windows of 243 frames with pad 121
:337-338) through the opt-in native training step, on the synthetic dataset as
tests/test_gpu_run_train.py drives the FCN: both epochs log, the training loss falls, the
checkpoint has the reference's format and loads into a fresh CoupledLSTM, --evaluate runs on it,
and --resume from epoch 1 reaches the uninterrupted run's epoch-2 weights bit for bit."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _argv(tmp, epochs=2, extra=()):
    return ["--use-model", "LSTM-Coupled", "-e", str(epochs), "-b", "32", "-lr", "0.001",
            "--synthetic-subjects", "3", "--synthetic-actions", "2", "--synthetic-frames", "60",
            "--subjects-train", "S1,S2", "--subjects-test", "S3", "-c", str(tmp), "--checkpoint-frequency", "1",
            "--seed", "3", *extra]


def _weights(path):
    from vp3d_amd.checkpoint import load_checkpoint
    return load_checkpoint(str(path))


def test_run_trains_checkpoints_resumes_and_evaluates(tmp_path, capsys):
    import run
    from common.models.CamLSTM import CoupledLSTM
    full_dir, res_dir = tmp_path / "full", tmp_path / "resumed"
    full = run.main(_argv(full_dir))
    out = capsys.readouterr().out
    assert "[1] time" in out and "[2] time" in out
    assert len(full["train"]) == 2 and len(full["valid"]) == 2
    assert full["train"][1] < full["train"][0], full["train"]
    ck1, ck2 = _weights(full_dir / "epoch_1.bin"), _weights(full_dir / "epoch_2.bin")
    assert set(ck2) == {"epoch", "lr", "random_state", "optimizer", "model_pos"}  # run.py:563-569
    assert ck2["epoch"] == 2
    fresh = CoupledLSTM(17, 2, 17, 3, 128, 2, [128, 128, 128])
    fresh.load_state_dict(ck2["model_pos"])
    assert int(fresh.bn_lstm.num_batches_tracked) == 2 * int(ck1["model_pos"]["bn_lstm.num_batches_tracked"])
    # --evaluate on the checkpoint (run.py:403-417, :712-713)
    res = run.main(_argv(full_dir, extra=("--evaluate", "epoch_2.bin")))
    assert res["summary"]["p1"] > 0 and res["summary"]["p1"] == res["summary"]["p1"]
    # --resume: epoch 2 from epoch_1.bin in another directory
    os.makedirs(res_dir)
    torch.save(ck1, res_dir / "epoch_1.bin")
    resumed = run.main(_argv(res_dir, extra=("-r", "epoch_1.bin")))
    assert len(resumed["train"]) == 1
    assert resumed["train"][0] == full["train"][1]
    r2 = _weights(res_dir / "epoch_2.bin")["model_pos"]
    for k, v in ck2["model_pos"].items():
        assert torch.equal(v, r2[k]), k
