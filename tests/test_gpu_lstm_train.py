"""CoupledLSTM training on the MI355X (csrc/seq_train.hip, csrc/vp3d_seq_train.cpp,
vp3d_amd/seq_train.py): the drop-in model with enable_native_training() against the reference's
recorded iterations and against the float32 / float64 train-mode oracle of
tests/lstm_train_cases.py, fed the masks and LeakyReLU sides the device drew.

Gates, the project's (tests/train_cases.py): y within 1e-5 m, loss 1e-5 relative, every gradient
through _grad_close (relative error <= max(1e-4, 4 x the float32 oracle's); a structurally zero
gradient in absolute terms, lstm_train_cases.grad_gate), running statistics rtol 1e-5 /
atol 1e-6, weights through _weights_close."""
import ctypes

import numpy as np
import pytest
import torch

import lstm_train_cases as LC

pytestmark = pytest.mark.gpu


def _model(c, state, dropout):
    m = LC.new_module(c, dropout=dropout)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()}, strict=False)
    return m.cuda().train().enable_native_training()


def _step(m, x2, xc, tgt):
    y = m(torch.from_numpy(np.array(x2)).cuda(), torch.from_numpy(np.array(xc)).cuda())
    loss = torch.mean(torch.norm(y - torch.from_numpy(np.array(tgt)).cuda(), dim=-1))  # common/loss.py:11-17
    m.zero_grad()
    loss.backward()
    return y, loss


def _grads(m):
    return {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}


def test_train_steps_match_reference():
    """Two reference iterations: forward, mpjpe, backward, Adam(amsgrad) -- the drop-in model in
    train mode with the native Adam (teacher-forced weights from step 1 on)."""
    from vp3d_amd.train import Adam
    g, meta, state = LC.load_golden()
    c = LC.Case("golden", meta["hidden"], meta["cells"], tuple(meta["head"]), meta["B"], meta["T"])
    m = _model(c, state, 0.0)
    opt = Adam(m.parameters(), lr=meta["lr"], amsgrad=meta["amsgrad"])
    for it in range(meta["steps"]):
        if it > 0:
            state = LC.golden_after(g, it - 1)
            m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
        y, loss = _step(m, g[f"s{it}/x2d"], g[f"s{it}/xcam"], g[f"s{it}/target"])
        np.testing.assert_allclose(y.detach().cpu().numpy(), g[f"s{it}/y"], atol=1e-5, rtol=0)
        np.testing.assert_allclose(loss.item(), float(g[f"s{it}/loss"]), rtol=1e-5)
        _, _, g64, _ = LC.oracle_step(state, g[f"s{it}/x2d"], g[f"s{it}/xcam"], g[f"s{it}/target"], c.H, c.L,
                                      len(c.head), dtype=torch.float64)
        rec = {k: g[f"s{it}/grad/{k}"] for k in g64}
        got = _grads(m)
        assert set(got) == set(g64)
        for k in g64:
            LC.grad_gate(got, rec, g64, k, len(c.head), f"step {it} grad", c.L, c.T)
        opt.step()
        for k, v in m.state_dict().items():
            if k.endswith("num_batches_tracked"):
                assert int(v) == it + 1
            elif "running" in k:
                np.testing.assert_allclose(v.cpu().numpy(), g[f"s{it}/after/{k}"], rtol=1e-5, atol=1e-6, err_msg=k)
            else:
                LC.weights_gate(v.cpu().numpy(), g[f"s{it}/after/{k}"], meta["lr"], k, len(c.head), f"step {it}",
                                c.L, c.T)


@pytest.mark.parametrize("cid", LC.CASE_IDS)
def test_shape_table_matches_oracle(cid):
    """Dropout 0.25: the oracle fed the masks and LeakyReLU sides the trainer drew gives the same
    output, loss, gradients and running statistics."""
    c = LC.case(cid)
    x2, xc, tgt = LC.case_inputs(cid)
    torch.manual_seed(1234)  # the module draws its mask seed from torch's generator
    m = _model(c, LC.case_state(cid), LC.P_DROP)
    y, loss = _step(m, x2, xc, tgt)
    tr = m.native_seq_trainer(torch.device("cuda", torch.cuda.current_device()))
    assert tr.n_sites() == c.L - 1 + len(c.head)
    masks = [tr.mask(s, 0).cpu().numpy() for s in range(tr.n_sites())]
    sides = [tr.mask(c.L - 1 + j, 1).cpu().numpy() for j in range(len(c.head))]
    assert [mk.shape for mk in masks] == LC.site_shapes(c)
    y32, loss32, g32, st32 = LC.case_oracle(cid, masks, sides, torch.float32)
    y64, loss64, g64, _ = LC.case_oracle(cid, masks, sides, torch.float64)
    np.testing.assert_allclose(y.detach().cpu().numpy(), y64, atol=1e-5, rtol=0)
    np.testing.assert_allclose(loss.item(), loss64, rtol=1e-5)
    got = _grads(m)
    assert set(got) == set(g64)
    for k in g64:
        LC.grad_gate(got, g32, g64, k, len(c.head), f"{cid} grad", c.L, c.T)
    for k, v in m.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1
        elif "running" in k:
            np.testing.assert_allclose(v.cpu().numpy(), st32[k], rtol=1e-5, atol=1e-6, err_msg=k)


def _trainer(H=128, L=2, head=(128,)):
    from vp3d_amd.seq_train import NativeSeqTrainer
    return NativeSeqTrainer(17, 2, 17, 3, H, L, list(head), torch.device("cuda", torch.cuda.current_device()))


def _trainer_forward(tr, state, B, T, p, seed):
    from vp3d_amd import synth
    params = [torch.from_numpy(np.array(v)).cuda() for v in state.values()]
    x2 = torch.from_numpy(synth.normalized_windows(3, "mask", B, T)).cuda()
    xc = torch.from_numpy(synth.normal(4, "mask/cam", (B, T, 3, 4), std=0.5).astype(np.float32)).cuda()
    return tr.forward(x2, xc, params, p, [0.1] * (len(tr.head_layers) + 1), seed)


def test_mask_statistics():
    """p = 0.25 on a (64, 27, 128) site: the keep rate within 4 binomial standard deviations of
    0.75, two seeds differ, the same seed repeats."""
    c = LC.case("one_tile_b5")
    tr = _trainer()
    B, T, p = 64, 27, 0.25
    masks = []
    for seed in (5, 6, 5):
        _trainer_forward(tr, LC.case_state(c.id), B, T, p, seed)
        masks.append(tr.mask(0, 0).cpu().numpy())
    assert masks[0].shape == (B, T, 128)
    n = masks[0].size
    sd = np.sqrt(0.75 * 0.25 / n)
    for mk in masks[:2]:
        assert set(np.unique(mk)) <= {0, 1}
        assert abs(mk.mean() - 0.75) <= 4 * sd, (mk.mean(), sd)
    assert (masks[0] != masks[1]).mean() > 0.25
    assert np.array_equal(masks[0], masks[2])
    tr.close()


def test_determinism():
    """The same inputs, weights and seed twice: bit-identical y and gradients."""
    cid = "tile_rem_b33"
    c = LC.case(cid)
    x2, xc, tgt = LC.case_inputs(cid)
    runs = []
    for _ in range(2):
        torch.manual_seed(77)
        m = _model(c, LC.case_state(cid), LC.P_DROP)
        y, _ = _step(m, x2, xc, tgt)
        runs.append((y.detach().cpu().numpy(), _grads(m)))
    assert np.array_equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert np.array_equal(runs[0][1][k], runs[1][1][k]), k


def test_stock_torch_adam_and_eval_cache():
    """One step with torch.optim.Adam works, and the eval lifter's weight cache sees the new
    weights: the eval forward changes and equals a fresh model's loaded from the new state_dict."""
    cid = "one_tile_b5"
    c = LC.case(cid)
    x2, xc, tgt = LC.case_inputs(cid)
    torch.manual_seed(5)
    m = _model(c, LC.case_state(cid), LC.P_DROP)
    a, b = torch.from_numpy(np.array(x2)).cuda(), torch.from_numpy(np.array(xc)).cuda()
    with torch.no_grad():
        before = m.eval()(a, b).cpu().numpy()
    m.train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, amsgrad=True)
    w0 = {k: v.detach().clone() for k, v in m.named_parameters()}
    _step(m, x2, xc, tgt)
    opt.step()
    moved = [k for k, v in m.named_parameters() if not torch.equal(v, w0[k])]
    assert len(moved) >= len(w0) - len(LC.zero_grad_keys(len(c.head), c.L, c.T))
    with torch.no_grad():
        after = m.eval()(a, b).cpu().numpy()
    assert not np.array_equal(before, after)
    fresh = LC.new_module(c)
    fresh.load_state_dict(m.state_dict())
    with torch.no_grad():
        want = fresh.cuda().eval()(a, b).cpu().numpy()
    np.testing.assert_allclose(after, want, rtol=0, atol=0)


def test_native_adam_bumps_the_eval_cache():
    from vp3d_amd.train import Adam
    cid = "h64_odd_head"
    c = LC.case(cid)
    x2, xc, tgt = LC.case_inputs(cid)
    m = _model(c, LC.case_state(cid), 0.0)
    a, b = torch.from_numpy(np.array(x2)).cuda(), torch.from_numpy(np.array(xc)).cuda()
    with torch.no_grad():
        before = m.eval()(a, b).cpu().numpy()
    m.train()
    opt = Adam(m.parameters(), lr=1e-3, amsgrad=True)
    _step(m, x2, xc, tgt)
    opt.step()
    with torch.no_grad():
        after = m.eval()(a, b).cpu().numpy()
    fresh = LC.new_module(c)
    fresh.load_state_dict(m.state_dict())
    with torch.no_grad():
        want = fresh.cuda().eval()(a, b).cpu().numpy()
    assert not np.array_equal(before, after)
    np.testing.assert_allclose(after, want, rtol=0, atol=0)


def test_errors():
    cid = "one_tile_b5"
    c = LC.case(cid)
    x2, xc, tgt = LC.case_inputs(cid)
    a, b = torch.from_numpy(np.array(x2)).cuda(), torch.from_numpy(np.array(xc)).cuda()
    m = _model(c, LC.case_state(cid), LC.P_DROP)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        m(a[:1], b[:1])
    # a backward after a second forward
    y1 = m(a, b)
    m(a, b)
    with pytest.raises(RuntimeError, match="another train-mode forward"):
        y1.sum().backward()
    # momentum=None (the cumulative average) is not built
    m.bn_lstm.momentum = None
    with pytest.raises(ValueError, match="momentum"):
        m(a, b)
    m.bn_lstm.momentum = 0.1
    # without the switch the train-mode call raises as before
    plain = LC.new_module(c).cuda().train()
    with pytest.raises(NotImplementedError):
        plain(a, b)


def test_frozen_parameter_gets_no_gradient():
    cid = "one_tile_b5"
    c = LC.case(cid)
    x2, xc, tgt = LC.case_inputs(cid)
    grads = []
    for frozen in (False, True):
        torch.manual_seed(9)
        m = _model(c, LC.case_state(cid), LC.P_DROP)
        if frozen:
            m.lstm_layers.weight_hh_l0.requires_grad_(False)
            m.mlp_layers[0].bias.requires_grad_(False)
        _step(m, x2, xc, tgt)
        grads.append({k: (None if p.grad is None else p.grad.cpu().numpy()) for k, p in m.named_parameters()})
    assert grads[1]["lstm_layers.weight_hh_l0"] is None and grads[1]["mlp_layers.0.bias"] is None
    for k, v in grads[0].items():
        if grads[1][k] is not None:
            assert np.array_equal(v, grads[1][k]), k


def test_trainer_create_refuses_the_transformer_and_bad_arguments():
    from vp3d_amd import _native as N
    from vp3d_amd.seq_train import NativeSeqTrainer
    dev = torch.device("cuda", torch.cuda.current_device())
    with pytest.raises(N.NativeError, match="vp3d error 2"):
        NativeSeqTrainer(17, 2, 17, 3, 128, 2, [128], dev, kind=N.SEQ_TRANSFORMER)
    tr = _trainer()
    state = LC.case_state("one_tile_b5")
    with pytest.raises(N.NativeError, match="dropout"):
        _trainer_forward(tr, state, 4, 3, 1.0, 0)
    lib = N.load()
    none = ctypes.c_void_p()
    assert lib.vp3d_seq_train_backward(tr._h, None, 0, none, None, none) == N.VP3D_ERR_STATE  # no forward yet
    _trainer_forward(tr, state, 4, 3, 0.25, 1)
    with pytest.raises(N.NativeError, match="n must be"):
        out = torch.empty(7, dtype=torch.uint8, device="cuda")
        N.check(lib.vp3d_seq_train_mask(tr._h, 0, 0, 7, out.data_ptr(), N.stream_ptr(dev)))
    tr.close()
