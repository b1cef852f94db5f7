"""bf16 mixed-precision training (model.set_train_dtype('bf16'); vp3d_trainer_set_compute,
csrc/train_bf16.hip, csrc/vp3d_train.cpp) against the teacher-forced bf16-operand oracle of
tests/bf16_train_cases.py, which takes the device's rounding decisions (vp3d_train_read) as the
suite already takes its ReLU and dropout decisions.  tests/test_bf16_train_cases.py checks the
yardstick on the CPU for every input used here.

Per step: check 1, the operand rows of every block conv in both roles equal
round_bf16(oracle float64 value) but for a share <= 2e-3 of neighbouring bf16 values; check 2, y,
loss, running statistics and every gradient tensor with the gates of test_gpu_train_shapes.py
(train_cases._grad_close unchanged).  A missing or misplaced rounding moves a block conv's weight
gradient by >= 3e-2, against a gate floor of 1e-4.
"""
import os

import numpy as np
import pytest
import torch

import bf16_train_cases as BT
import train_cases as TC
from train_cases import _masks, _model

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _loss(y, tgt):
    return torch.mean(torch.norm(y - torch.tensor(tgt).cuda(), dim=-1))


def _snapshot(m):
    return {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}


def _train_step(m, x, tgt, seed=1234):
    torch.manual_seed(seed)  # the module draws its dropout seed from torch's generator
    for prm in m.parameters():
        prm.grad = None
    y = m(torch.tensor(x).cuda())
    loss = _loss(y, tgt)
    loss.backward()
    return (y.detach().cpu().numpy(), loss.item(),
            {k: prm.grad.cpu().numpy() for k, prm in m.named_parameters()})


def _bf16_model(cid, capture=True):
    c = BT.row(cid)
    m = _model(TC.meta_of(c), BT.row_state(cid), dropout=c.p, jin=c.jin)
    m.set_train_dtype("bf16")
    if capture:
        m.native_trainer(_dev()).capture(True)
    return m


def _check_forced(tag, m, c, state, x, tgt, got):
    """Checks 1 and 2 for the step `got` = (y, loss, grads) that module `m` just ran from `state`."""
    tr = m.native_trainer(_dev())
    assert tr.compute == "bf16"
    B, T = x.shape[0], x.shape[1]
    p = float(m.drop.p)
    masks = _masks(m, B, T) if p > 0 else None
    rm = _masks(m, B, T, "relu")
    nl = 2 * len(c.fw)
    forced = dict(acts={l: BT.rows_to_cf(tr.read(l, 0), B) for l in range(1, nl - 1)},
                  grads={l: BT.rows_to_cf(tr.read(l, 1), B) for l in range(1, nl - 1)})
    for kind in forced:
        for l, a in forced[kind].items():
            assert torch.equal(BT.round_bf16(a), a), f"{tag} {kind} {l}: rows are not bf16 values"
            assert float(a.abs().max()) > 0, f"{tag} {kind} {l}: rows are all zero"
    o64, o32, report = BT.forced_oracles(state, x, tgt, TC.meta_of(c), p, masks, rm, forced)
    BT.check_operands(tag, report, BT.n_block_convs(c))
    stats = {k: v.cpu().numpy() for k, v in m.state_dict().items()}
    BT.check_outputs(tag, got, o64, o32, stats)


@pytest.mark.parametrize("cid", BT.ALL_ROWS)
def test_teacher_forced_parity(cid):
    c = BT.row(cid)
    sd = BT.row_state(cid)
    x, tgt = BT.row_inputs(cid)
    m = _bf16_model(cid)
    got = _train_step(m, x, tgt)
    _check_forced(cid, m, c, sd, x, tgt, got)
    # the shrink stays f32: its gradient rows are dy
    tr = m.native_trainer(_dev())
    assert tr.read(2 * len(c.fw) - 1, 1).shape == (c.B * TC.layer_lengths(c)[-1], 51)


def test_no_block_conv_is_the_f32_step():
    """fw = (3,): no block conv, so bf16 mode gives the f32 mode's bits."""
    cid = "no_blocks_c64"
    c = TC.case(cid)
    x, tgt = TC.case_inputs(cid)
    ref = _train_step(_model(TC.meta_of(c), TC.case_state(cid), dropout=c.p, jin=c.jin), x, tgt)
    m = _model(TC.meta_of(c), TC.case_state(cid), dropout=c.p, jin=c.jin).set_train_dtype("bf16")
    got = _train_step(m, x, tgt)
    assert m.native_trainer(_dev()).compute == "bf16"
    np.testing.assert_array_equal(got[0], ref[0])
    assert got[1] == ref[1]
    for k in ref[2]:
        np.testing.assert_array_equal(got[2][k], ref[2][k], err_msg=k)


def test_default_untouched_after_a_bf16_step():
    """bf16 and back to fp32: the fp32 step of that model gives the bits of a fresh model's, and
    the bf16 step in between differs from it; vp3d_trainer_compute reports each setting."""
    cid = "c320_dilated"
    c = TC.case(cid)
    x, tgt = TC.case_inputs(cid)
    fresh = _model(TC.meta_of(c), TC.case_state(cid), dropout=c.p, jin=c.jin)
    assert fresh.train_dtype == "fp32"
    ref = _train_step(fresh, x, tgt)
    assert fresh.native_trainer(_dev()).compute == "fp32"
    m = _model(TC.meta_of(c), TC.case_state(cid), dropout=c.p, jin=c.jin)
    m.set_train_dtype("bf16")
    mid = _train_step(m, x, tgt)
    assert m.native_trainer(_dev()).compute == "bf16"
    assert not np.array_equal(mid[0], ref[0])
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in TC.case_state(cid).items()})
    m.set_train_dtype("fp32")
    got = _train_step(m, x, tgt)
    assert m.native_trainer(_dev()).compute == "fp32"
    np.testing.assert_array_equal(got[0], ref[0])
    assert got[1] == ref[1]
    for k in ref[2]:
        np.testing.assert_array_equal(got[2][k], ref[2][k], err_msg=k)
    for k, v in fresh.state_dict().items():
        np.testing.assert_array_equal(m.state_dict()[k].cpu().numpy(), v.cpu().numpy(), err_msg=k)


def test_weights_follow_the_optimiser():
    """forward, backward, native Adam step, forward again: the second step passes the checks
    against the oracle holding the UPDATED parameters (a stale bf16 weight pack fails check 2)."""
    from vp3d_amd.train import Adam
    cid = "c320_dilated"
    c = TC.case(cid)
    x, tgt = TC.case_inputs(cid)
    m = _bf16_model(cid)
    opt = Adam(m.parameters(), lr=1e-2, amsgrad=True)
    first = _train_step(m, x, tgt)
    opt.step()
    state = _snapshot(m)
    moved = TC.rel_err(state["layers_conv.0.weight"], TC.case_state(cid)["layers_conv.0.weight"])
    assert moved > 0.05, moved  # far beyond a bf16 ulp: the packs must be rebuilt
    got = _train_step(m, x, tgt, seed=77)
    assert not np.array_equal(got[0], first[0])
    _check_forced(cid + "-after-adam", m, c, state, x, tgt, got)


def test_bf16_step_is_deterministic():
    cid = "traj_c72_causal"
    x, tgt = BT.row_inputs(cid)
    a = _train_step(_bf16_model(cid, capture=False), x, tgt)
    b = _train_step(_bf16_model(cid), x, tgt)  # capture on: a copy, not another result
    np.testing.assert_array_equal(a[0], b[0])
    assert a[1] == b[1]
    for k in a[2]:
        np.testing.assert_array_equal(a[2][k], b[2][k], err_msg=k)


def test_error_paths():
    from common.models.TemporalModel import TemporalModel
    cid = "w5expand_traj_c64"
    c = TC.case(cid)
    x, tgt = TC.case_inputs(cid)
    m = _model(TC.meta_of(c), TC.case_state(cid), dropout=c.p, jin=c.jin)
    for bad in ("fp16", "f16x3", "float32"):
        with pytest.raises(ValueError, match="training dtype"):
            m.set_train_dtype(bad)
    assert m.train_dtype == "fp32"
    tr = m.native_trainer(_dev())
    with pytest.raises(ValueError):
        tr.set_compute("fp16")
    # 68 channels: refused with the message, before a trainer exists
    m68 = TemporalModel(17, 2, 17, [3, 3], channels=68, dropout=0.0).cuda().train().set_train_dtype("bf16")
    with pytest.raises(ValueError, match="channels % 8 == 0"):
        m68(torch.zeros(2, 9, 17, 2, device="cuda"))
    assert m68._trainer is None
    # read(l, 1) without capture; read before any forward
    with pytest.raises(RuntimeError, match="forward"):
        tr.read(1, 0)
    m.set_train_dtype("bf16")
    xt = torch.tensor(x).cuda()
    y = m(xt)
    loss = _loss(y, tgt)
    assert tr.read(1, 0).shape == (c.B * TC.layer_lengths(c)[0], c.channels)
    # the expand conv stays f32: its rows are x itself (read while the caller still holds x)
    np.testing.assert_array_equal(tr.read(0, 0).cpu().numpy(), x.reshape(c.B * c.T, -1))
    with pytest.raises(RuntimeError, match="capture"):
        tr.read(1, 1)
    # the mode changed between a forward and its backward
    tr.set_compute("fp32")
    with pytest.raises(RuntimeError, match="compute dtype changed"):
        loss.backward(retain_graph=True)
    tr.set_compute("bf16")
    loss.backward()
    with pytest.raises(RuntimeError, match="capture"):
        tr.read(1, 1)  # that backward ran without capture
    assert all(torch.isfinite(prm.grad).all() for prm in m.parameters())


def _argv(tmp, epochs=2, extra=()):
    # the synthetic split of tests/test_gpu_run_train.py
    return ["-e", str(epochs), "-b", "256", "-lr", "0.001", "-lrd", "0.95", "--fcn-architecture", "3,3,3",
            "-ch", "64", "--fcn-dropout", "0", "--synthetic-subjects", "3", "--synthetic-actions", "2",
            "--synthetic-frames", "150", "--subjects-train", "S1,S2", "--subjects-test", "S3",
            "-c", str(tmp), "--checkpoint-frequency", "1", "--seed", "3", *extra]


def _oracle_epochs(args_argv, bf16):
    """The two epochs on the CPU: the plain oracle loop, or the same under the (not teacher-forced)
    bf16-operand shim."""
    import contextlib

    import run
    from common.arguments import parse_args
    from oracle import camera_ref, generators_ref
    from oracle.train_ref import reference_epochs
    from vp3d_amd import synth
    from common.models.TemporalModel import TemporalModel
    args = parse_args(args_argv)
    data = run.synthetic_dataset(args, normalize=camera_ref.normalize_screen_coordinates)
    cams, p3d, p2d = run.fetch(data, ["S1", "S2"])
    cams_t, p3d_t, p2d_t = run.fetch(data, ["S3"])
    m = TemporalModel(17, 2, 17, [3, 3, 3], channels=64)
    sd = synth.lifter_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed=3)
    pad, n_pairs = 13, sum(p.shape[0] for p in p2d)
    rs = np.random.RandomState(1234)

    def train_batches():
        for bi, (bc, b3, b2) in enumerate(generators_ref.chunked_batches(cams, p3d, p2d, 256, 1, pad, 0, random=rs)):
            n = min(256, n_pairs - bi * 256)
            yield bc[:n], b3[:n], b2[:n]

    def test_sequences():
        return generators_ref.unchunked_sequences(cams_t, p3d_t, p2d_t, pad, 0)

    with (BT.bf16_oracle() if bf16 else contextlib.nullcontext()):
        return reference_epochs(sd, [3, 3, 3], train_batches, test_sequences, 2, lr=1e-3, lr_decay=0.95)


def test_run_train_bf16(tmp_path):
    """run.py --train-dtype bf16, two epochs: completes with finite losses that are not the fp32
    run's bits, within 4 x the difference the bf16-operand oracle shows against the plain oracle
    on the CPU (both figures: DESIGN.md §8), and its checkpoint resumes in an fp32 run."""
    import run
    d32, d16 = tmp_path / "fp32", tmp_path / "bf16"
    r32 = run.main(_argv(d32))
    r16 = run.main(_argv(d16, extra=("--train-dtype", "bf16")))
    assert len(r16["train"]) == 2 and len(r16["valid"]) == 2
    assert np.isfinite(r16["train"]).all() and np.isfinite(r16["valid"]).all()
    assert list(r16["train"]) != list(r32["train"])  # the mode is engaged
    o_plain = _oracle_epochs(_argv(d32), False)
    o_bf16 = _oracle_epochs(_argv(d32), True)
    for name, i in (("train", 0), ("valid", 1)):
        cpu = np.abs(np.array(o_bf16[i]) - np.array(o_plain[i]))
        gpu = np.abs(np.array(r16[name]) - np.array(r32[name]))
        print(f"{name}: |bf16 - fp32| per epoch, device {gpu}, oracle {cpu}; losses fp32 {r32[name]} bf16 {r16[name]}")
        assert (gpu <= 4 * cpu).all(), (name, gpu, cpu)
    assert os.path.exists(os.path.join(d16, "epoch_2.bin"))
    resumed = run.main(_argv(d16, epochs=2, extra=("-r", "epoch_1.bin")))  # an fp32 run from the bf16 checkpoint
    assert len(resumed["train"]) == 1 and np.isfinite(resumed["train"]).all()
    np.testing.assert_allclose(resumed["train"][0], r16["train"][1], rtol=1e-2)
