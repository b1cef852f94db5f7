"""The native training step (csrc/train.hip, csrc/vp3d_train.cpp, vp3d_amd/train.py through the
drop-in TemporalModel in train mode) across the shapes of tests/train_cases.py, against the
float64 oracle (oracle/train_ref.py) fed the trainer's own dropout masks and ReLU decisions.
tests/test_train_cases.py checks on the CPU that the float32 oracle is a sound yardstick on
every row and that what a row is there for moves its result far beyond the gates.

Gates (the suite's own, tests/test_gpu_train.py):
  poses              1e-5 m against the float32 oracle
  loss               1e-5 relative
  gradients          _grad_close: per tensor ||g - g64|| <= max(1e-4, 4 x the float32 oracle's)
                     ||g64||, every element within 2e-3 of the largest
  running statistics rtol 1e-5, atol 1e-6
  kept fraction      binomial, 4 sigma around 1 - p
and measured ones.  Over the seven table rows the largest relative error of a gradient tensor is
2.35e-6 (expand_conv.weight of w5expand_traj_c64, whose float32 oracle is at 1.99e-6; the other
rows 4.5e-7 .. 1.5e-6), 0.6 .. 2.4 times the float32 oracle's own, poses 7.8e-8 .. 9.7e-7 m.
GRAD_REL_MEASURED = 3 x 2.35e-6 = 7.1e-6, 14 times under the 1e-4 floor, bounds every tensor of
a table row, and stands in for the 1e-4 floor (max(7.1e-6, 4 x the float32 oracle's)) in every
other step of this file: the one- and two-window steps of test_one_module_across_shapes
normalise over a nearly two-valued batch, where the float32 oracle itself is up to 4.9e-5 from
the float64 one and the kernels 4.7e-5 (ratio at most 2.6 anywhere).  profiles/train_shapes.txt
holds every tensor's error and its ratio to the float32 oracle's, for every step.

Seeded defects.  Each of these, seeded one at a time, passes every training test that existed
before this file (tests/test_gpu_train.py, tests/test_gpu_run_train.py) and fails here:
  the tap of the f32 conv's scalar loader `dil - 1` rows on instead of `dil` (load_a_scalar)
      traj_c72_causal (poses off by 0.26 m), test_bn_cumulative_average
  the second k-tile of the weight gradient's scalar K path reading the neighbouring input
  channel (wgrad_f32_kernel, k0 > 0)
      every row with K > 128: traj_c72_causal, w5expand_c200_1f, dense_c136_traj,
      causal_1f_c72_traj, w5expand_traj_c64 (expand_conv.weight off by 0.32 .. 0.88 relative),
      and the tests that reuse them
  colreduce_kernel's channel-group count rounded down, so a partial last group is not reduced
      c320_dilated, test_one_module_across_shapes, test_one_value_per_channel_raises[c320]
  the residual slice's window pitch taken from the shape the arena was sized for, not the
  batch's (vp3d_train_forward after reserve() kept the arena)
      test_one_module_across_shapes (both p, at the (2, 40) step), test_bn_cumulative_average
  the decayed gradient of adam_kernel as a separate multiply and add (the form before this file)
      tests/test_gpu_train.py::test_adam_options_bitexact_vs_torch[wd_amsgrad, wd_plain]:
      0.85 % of exp_avg off by an ulp after the first step
"""
import numpy as np
import pytest
import torch

import train_cases as TC
from train_cases import _grad_close, _masks, _model, _oracle

pytestmark = pytest.mark.gpu

GRAD_REL_MEASURED = 7.1e-6  # 3 x 2.35e-6 (profiles/train_shapes.txt)


def _loss(y, tgt):
    return torch.mean(torch.norm(y - torch.tensor(tgt).cuda(), dim=-1))


def _snapshot(m):
    return {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}


def _train_step(m, x, tgt, seed=1234):
    """One train-mode forward + mpjpe + backward: (y, loss, gradients by name)."""
    torch.manual_seed(seed)  # the module draws its dropout seed from torch's generator
    for prm in m.parameters():
        prm.grad = None
    y = m(torch.tensor(x).cuda())
    loss = _loss(y, tgt)
    loss.backward()
    return (y.detach().cpu().numpy(), loss.item(),
            {k: prm.grad.cpu().numpy() for k, prm in m.named_parameters()})


def _check_step(tag, m, c, state, x, tgt, y, loss, grads, momentum=0.1, table_row=False):
    """The gates of the module docstring for one step of module `m`, which held `state` before
    it.  Returns the float32 oracle's running statistics (the state the next step starts from)."""
    meta, p = TC.meta_of(c), float(m.drop.p)
    B, T = x.shape[0], x.shape[1]
    masks = None
    if p > 0:
        masks = _masks(m, B, T)
        n = sum(mk.size for mk in masks)
        keep = sum(float(mk.sum()) for mk in masks) / n
        assert abs(keep - (1 - p)) < max(0.005, 4 * np.sqrt(p * (1 - p) / n)), (keep, n)
    rm = _masks(m, B, T, "relu")
    assert [mk.shape[0] for mk in rm] == [B * L for L in TC.layer_lengths(c, T)]
    y32, l32, _, st32 = _oracle(state, x, tgt, meta, p=p, masks=masks, momentum=momentum)
    _, _, g64, _ = _oracle(state, x, tgt, meta, p=p, masks=masks, dtype=torch.float64, relu_masks=rm)
    _, _, g32, _ = _oracle(state, x, tgt, meta, p=p, masks=masks, relu_masks=rm)
    e = float(np.abs(y - y32).max())
    print(f"{tag}: poses {e:.2e} m, loss {abs(loss - l32) / abs(l32):.2e}")
    np.testing.assert_allclose(y, y32, atol=1e-5, rtol=0)
    np.testing.assert_allclose(loss, l32, rtol=1e-5)
    assert set(grads) == set(g64)
    for k in grads:
        rel, ref = _grad_close(grads[k], g32[k], g64[k], f"{tag} {k}", floor=GRAD_REL_MEASURED,
                               tight=GRAD_REL_MEASURED if table_row else None)
        print(f"{tag} {k}: ratio {rel / max(ref, 1e-30):.2f}")
    for k, v in m.state_dict().items():
        if "running" in k:
            np.testing.assert_allclose(v.cpu().numpy(), st32[k], rtol=1e-5, atol=1e-6, err_msg=f"{tag} {k}")
    return st32


@pytest.mark.parametrize("cid", TC.CASE_IDS)
def test_table_row_vs_float64_oracle(cid):
    c = TC.case(cid)
    sd = TC.case_state(cid)
    x, tgt = TC.case_inputs(cid)
    m = _model(TC.meta_of(c), sd, dropout=c.p, jin=c.jin)
    y, loss, grads = _train_step(m, x, tgt)
    _check_step(cid, m, c, sd, x, tgt, y, loss, grads, table_row=True)
    for k, v in m.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1


RESHAPES = [(5, 61), (2, 40), (5, 61), (7, 90), (1, 61)]  # fits, fits, regrow, fits


@pytest.mark.parametrize("p", [0.0, 0.25])
def test_one_module_across_shapes(p):
    """One trainer whose arena is kept (the shape fits) or reallocated (it does not): each step
    passes the gates and equals, bit for bit, the step of a fresh module with the same weights
    and running statistics at that shape (no atomics; the reduction and weight-gradient splits
    depend on the shape alone; the dropout mask on the seed, the layer and the element)."""
    cid = "c320_dilated"
    c = TC.case(cid)
    m = _model(TC.meta_of(c), TC.case_state(cid), dropout=p, jin=c.jin)
    trainer = None
    for it, (B, T) in enumerate(RESHAPES):
        x, tgt = TC.case_inputs(cid, B, T)
        state = _snapshot(m)
        y, loss, grads = _train_step(m, x, tgt, seed=100 + it)
        if trainer is None:
            trainer = m.native_trainer(torch.device("cuda", torch.cuda.current_device()))
        assert m.native_trainer(torch.device("cuda", torch.cuda.current_device())) is trainer
        tag = f"{cid}-p{p}-step{it}-{B}x{T}"
        _check_step(tag, m, c, state, x, tgt, y, loss, grads)
        fresh = _model(TC.meta_of(c), state, dropout=p, jin=c.jin)
        yf, lf, gf = _train_step(fresh, x, tgt, seed=100 + it)
        np.testing.assert_array_equal(y, yf, err_msg=tag)
        assert loss == lf
        for k in grads:
            np.testing.assert_array_equal(grads[k], gf[k], err_msg=f"{tag} {k}")
        for k, v in fresh.state_dict().items():
            np.testing.assert_array_equal(m.state_dict()[k].cpu().numpy(), v.cpu().numpy(), err_msg=f"{tag} {k}")


def test_bn_cumulative_average():
    """momentum=None: the running statistics are the cumulative average of the batch statistics
    (factor 1, 1/2, 1/3 over three different batches) and num_batches_tracked counts them."""
    cid = "traj_c72_causal"
    c = TC.case(cid)
    m = _model(TC.meta_of(c), TC.case_state(cid), dropout=0.0, jin=c.jin)
    m.set_bn_momentum(None)
    for it, (B, T) in enumerate([(3, 75), (4, 60), (3, 50)]):
        x, tgt = TC.case_inputs(cid, B, T)
        state = _snapshot(m)
        y, loss, grads = _train_step(m, x, tgt)
        _check_step(f"{cid}-cumulative-step{it}", m, c, state, x, tgt, y, loss, grads, momentum=1.0 / (it + 1))
    for k, v in m.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 3, k


def test_bn_decayed_momentum():
    """set_bn_momentum with a decayed value, as run.py sets it each epoch."""
    cid = "causal_1f_c72_traj"
    c = TC.case(cid)
    sd = TC.case_state(cid)
    x, tgt = TC.case_inputs(cid)
    m = _model(TC.meta_of(c), sd, dropout=c.p, jin=c.jin)
    m.set_bn_momentum(0.0316)
    y, loss, grads = _train_step(m, x, tgt)
    _check_step(f"{cid}-momentum0.0316", m, c, sd, x, tgt, y, loss, grads, momentum=0.0316)


@pytest.mark.parametrize("cid,T_one", [("w5expand_c200_1f", 45), ("c320_dilated", 27)])
def test_one_value_per_channel_raises(cid, T_one):
    """One window whose last block has one frame: BatchNorm cannot train on one value per
    channel.  The reference raises ValueError (F.batch_norm); so does the drop-in, before
    num_batches_tracked or a running statistic changes, and the module then trains as before."""
    c = TC.case(cid)
    sd = TC.case_state(cid)
    m = _model(TC.meta_of(c), sd, dropout=c.p, jin=c.jin)
    assert TC.layer_lengths(c, T_one)[-1] == 1
    x1, _ = TC.case_inputs(cid, 1, T_one)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m(torch.tensor(x1).cuda())
    for k, v in m.state_dict().items():
        np.testing.assert_array_equal(v.cpu().numpy(), sd[k], err_msg=k)
    x, tgt = TC.case_inputs(cid)
    y, loss, grads = _train_step(m, x, tgt)
    _check_step(f"{cid}-after-refusal", m, c, sd, x, tgt, y, loss, grads)
    for k, v in m.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1


def test_frozen_parameter_is_refused():
    """A parameter with requires_grad False: the native backward has no partial form, so it
    raises (never returns gradients); with the flag restored the module trains as before."""
    cid = "no_blocks_c64"
    c = TC.case(cid)
    sd = TC.case_state(cid)
    x, tgt = TC.case_inputs(cid)
    m = _model(TC.meta_of(c), sd, dropout=c.p, jin=c.jin)
    m.expand_bn.weight.requires_grad_(False)
    for prm in m.parameters():
        prm.grad = None
    loss = _loss(m(torch.tensor(x).cuda()), tgt)
    with pytest.raises(RuntimeError, match="NULL"):
        loss.backward()
    assert all(prm.grad is None for prm in m.parameters())
    m.expand_bn.weight.requires_grad_(True)
    state = _snapshot(m)  # the refused step's forward updated the running statistics
    y, loss, grads = _train_step(m, x, tgt)
    _check_step(f"{cid}-after-frozen", m, c, state, x, tgt, y, loss, grads)


def test_channels_not_multiple_of_8_refused():
    """validate_cfg admits channels % 8 == 0 only: 36 is refused when the trainer is built."""
    from common.models.TemporalModel import TemporalModel
    m = TemporalModel(17, 2, 17, [3, 3], channels=36, dropout=0.0).cuda().train()
    with pytest.raises(AssertionError, match="invalid lifter configuration"):
        m(torch.zeros(2, 9, 17, 2, device="cuda"))
    assert m._trainer is None
