"""CPU self-check of the training-step shape table (tests/train_cases.py): the conditions
tests/test_gpu_train_shapes.py leans on, from the oracle alone (dropout masks drawn with numpy).

  * the float32 oracle is a usable yardstick on every row: poses within 1e-6 m of the float64
    oracle (a tenth of the 1e-5 m gate), every gradient tensor within 5e-6 relative (a twentieth
    of the 1e-4 floor of the gradient gate), with no ReLU decisions shared between the two;
  * what a row is there for changes its result by far more than the gates: causal, dense, the
    six trajectory joints, the BatchNorm momentum;
  * torch.optim.Adam on the CPU, the reference side of the Adam kernel test, gives finite
    results on every option set of train_cases.ADAM_CASES;
  * the partial sums the trainer's arena reserves for its column reductions bound what a
    reduction over any smaller batch writes (host arithmetic of libvp3d.so).
"""
import functools

import numpy as np
import pytest
import torch

import train_cases as TC

POSE_TOL = 1e-6   # m: a tenth of the GPU test's 1e-5 m
GRAD_TOL = 5e-6   # relative, per tensor: a twentieth of the gradient gate's 1e-4 floor
POSE_MOVE = 1e-3  # m: 100 gates
GRAD_MOVE = 5e-3  # relative: 50 gate floors


@functools.lru_cache(maxsize=None)
def _run(cid, dtype=torch.float32, causal=None, momentum=0.1):
    c = TC.case(cid)
    meta = TC.meta_of(c)
    if causal is not None:
        meta["causal"] = causal
    x, tgt = TC.case_inputs(cid)
    masks = TC.numpy_masks(c) if c.p > 0 else None
    return TC._oracle(TC.case_state(cid), x, tgt, meta, p=c.p, masks=masks, dtype=dtype, momentum=momentum)


@pytest.mark.parametrize("cid", TC.CASE_IDS)
def test_table_row_is_what_it_says(cid):
    c = TC.case(cid)
    assert TC.layer_lengths(c) == TC.LENGTHS[cid]
    assert c.channels % 8 == 0
    y, _, grads, _ = _run(cid)
    assert y.shape == (c.B, TC.LENGTHS[cid][-1], 17, 3)
    K = c.fw[0] * c.jin * 2
    assert grads["expand_conv.weight"].shape == (c.channels, c.jin * 2, c.fw[0])
    if cid in ("traj_c72_causal", "causal_1f_c72_traj"):
        assert K == 138 and c.channels % 16 == 8
    if cid == "w5expand_traj_c64":
        assert K == 230
    if cid == "w5expand_c200_1f":
        assert K == 170 and 128 < c.channels < 256 and c.B * TC.LENGTHS[cid][-1] == 24
    if cid == "c320_dilated":
        assert 256 < c.channels < 512 and c.channels % 128 != 0 and c.channels % 16 == 0
    if cid == "no_blocks_c64":
        M = c.B * TC.LENGTHS[cid][0]
        assert M == 65 and M % 4 == 1 and M - 64 == 1  # reduction chunks hold at least 64 rows


@pytest.mark.parametrize("cid", TC.CASE_IDS)
def test_float32_oracle_against_float64(cid):
    y32, l32, g32, st32 = _run(cid)
    y64, l64, g64, st64 = _run(cid, torch.float64)
    e = float(np.abs(y32.astype(np.float64) - y64).max())
    print(f"{cid}: poses {e:.2e} m, loss {abs(l32 - l64) / l64:.2e}")
    assert e <= POSE_TOL
    assert abs(l32 - l64) <= 1e-6 * abs(l64)
    for k in g64:
        r = TC.rel_err(g32[k], g64[k])
        print(f"{cid} {k}: {r:.2e}")
        assert r <= GRAD_TOL, (k, r)
    for k in st64:
        np.testing.assert_allclose(st32[k], st64[k], rtol=1e-6, atol=1e-7, err_msg=k)


@pytest.mark.parametrize("cid", [c.id for c in TC.CASES if c.causal])
def test_causal_matters(cid):
    y, _, g, _ = _run(cid)
    y_nc, _, g_nc, _ = _run(cid, causal=False)
    move = float(np.abs(y - y_nc).max())
    rels = {k: TC.rel_err(g_nc[k], g[k]) for k in g}
    print(f"{cid}: poses move {move:.2e} m, gradients at least {min(rels.values()):.2e}")
    assert move >= POSE_MOVE
    assert min(rels.values()) >= GRAD_MOVE, rels


def _dilated_twin(sd, fw):
    """The dilated model that keeps only the dense k-convs' taps on the dilation grid."""
    out, dil = dict(sd), fw[0]
    for i, w in enumerate(fw[1:]):
        k = f"layers_conv.{2 * i}.weight"
        out[k] = np.ascontiguousarray(sd[k][:, :, ::dil])
        assert out[k].shape[2] == w
        dil *= w
    return out


@pytest.mark.parametrize("cid", [c.id for c in TC.CASES if c.dense])
def test_dense_matters(cid):
    """Against the dilated model holding the same weights on the dilation grid (the taps
    --dense adds set to zero): poses and every gradient tensor move (a dense k-conv's gradient
    compared on the grid taps)."""
    c = TC.case(cid)
    x, tgt = TC.case_inputs(cid)
    y, _, g, _ = _run(cid)
    meta = dict(TC.meta_of(c), dense=False)
    y_d, _, g_d, _ = TC._oracle(_dilated_twin(TC.case_state(cid), c.fw), x, tgt, meta, p=c.p,
                                masks=TC.numpy_masks(c))
    move = float(np.abs(y - y_d).max())
    rels, dil = {}, c.fw[0]
    for k in g:
        a = g[k]
        if a.shape != g_d[k].shape:
            a = a[:, :, ::dil]
            dil *= a.shape[2]
        rels[k] = TC.rel_err(g_d[k], a)
    print(f"{cid}: poses move {move:.2e} m, gradients at least {min(rels.values()):.2e}")
    assert move >= POSE_MOVE
    assert min(rels.values()) >= GRAD_MOVE, rels


@pytest.mark.parametrize("cid", [c.id for c in TC.CASES if c.jin == 23])
def test_trajectory_joints_matter(cid):
    """Without the last six input joints (the expand weight cut to the first 34 input
    channels) the expand gradient of the remaining channels moves."""
    c = TC.case(cid)
    x, tgt = TC.case_inputs(cid)
    _, _, g, _ = _run(cid)
    sd = dict(TC.case_state(cid))
    sd["expand_conv.weight"] = np.ascontiguousarray(sd["expand_conv.weight"][:, :34])
    _, _, g17, _ = TC._oracle(sd, x[:, :, :17], tgt, TC.meta_of(c), p=c.p,
                              masks=TC.numpy_masks(c) if c.p > 0 else None)
    r = TC.rel_err(g17["expand_conv.weight"], g["expand_conv.weight"][:, :34])
    # and the six joints' own gradient is no rounding-level tail of the tensor
    share = np.linalg.norm(g["expand_conv.weight"][:, 34:]) / np.linalg.norm(g["expand_conv.weight"])
    print(f"{cid}: expand gradient moves {r:.2e}, joints 17..22 hold {share:.2e} of its norm")
    assert r >= GRAD_MOVE
    assert share >= GRAD_MOVE


def test_momentum_matters():
    """Momentum 0.1 against 1/3 (the third step of momentum=None) moves a running statistic."""
    _, _, _, a = _run("c320_dilated")
    _, _, _, b = _run("c320_dilated", momentum=1.0 / 3.0)
    move = max(float(np.abs(a[k] - b[k]).max()) for k in a)
    print(f"running statistics move {move:.2e}")
    assert move >= 1e-2


@pytest.mark.parametrize("aid", TC.ADAM_IDS)
def test_torch_adam_reference_is_finite(aid):
    """The reference side of test_adam_options_bitexact_vs_torch: three CPU steps of
    torch.optim.Adam per option set leave finite parameters and moments, and the step counts
    the case is there for."""
    kw, init, steps, split = TC.adam_problem(aid)
    ps = [torch.tensor(a, requires_grad=True) for a in init]
    opt = torch.optim.Adam(TC.adam_groups(ps, split), lr=1e-3, **kw)
    for gs in steps:
        for p, g in zip(ps, gs):
            p.grad = None if g is None else torch.tensor(g)
        opt.step()
    st = opt.state_dict()["state"]
    assert len(st) == len(ps)
    for i, p in enumerate(ps):
        assert torch.isfinite(p).all()
        assert not np.array_equal(p.detach().numpy(), init[i])
        keys = ["exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if kw.get("amsgrad") else [])
        assert ("max_exp_avg_sq" in st[i]) == bool(kw.get("amsgrad"))
        for k in keys:
            assert torch.isfinite(st[i][k]).all() and float(st[i][k].abs().max()) > 0
    counts = sorted({float(s["step"]) for s in st.values()})
    assert counts == ([2.0, 3.0] if aid == "steps_diverge" else [3.0])
    if aid == "seventy_tensors":
        assert len(ps) == 70 and min(p.numel() for p in ps) == 1 and max(p.numel() for p in ps) == 3000


def _reduce_rows(M, C):
    """Python copy of reduce_rows (csrc/train.hip): enough chunks to fill the chip, >= 64 rows each."""
    cgroups = (C + 255) // 256
    chunks = (2048 + cgroups - 1) // cgroups
    return max(64, (M + chunks - 1) // chunks)


@pytest.mark.parametrize("C", [51, 64, 256, 320, 1024])
def test_reduction_arena_bound_covers_every_smaller_batch(C):
    """The trainer sizes its reduction partials once, for the largest (B, T), and keeps the arena
    for smaller batches.  The chunk count a reduction launches is not monotone in the row count
    (C <= 256: 2,048 chunks of 64 rows at 131,072 rows, 2,017 of 65 at 131,073), so the reserved
    count must bound every row count up to the one it was sized for.  Host arithmetic of
    libvp3d.so (vp3d_train_reduce_doubles), swept around the 64-row knee of every width."""
    from vp3d_amd import _native as N
    lib = N.load()
    cgroups = (C + 255) // 256
    knee = 64 * ((2048 + cgroups - 1) // cgroups)
    Ms = sorted({1, 2, 63, 64, 65, 127, 128, 129, 1000, 4097, 3 * knee, 10 * knee + 7}
                | set(range(knee - 130, knee + 131)) | set(range(2 * knee - 3, 2 * knee + 4)))
    launched = {}
    for M in Ms:
        launched[M] = lib.vp3d_train_reduce_doubles(M, C, 0)
        rows = _reduce_rows(M, C)
        assert launched[M] == ((M + rows - 1) // rows) * 2 * C, M
    assert launched[knee] > launched[knee + 1]  # the non-monotone step the bound is there for
    worst = 0
    for M in Ms:
        worst = max(worst, launched[M])
        reserved = lib.vp3d_train_reduce_doubles(M, C, 1)
        assert reserved >= worst, (M, reserved, worst)
        assert reserved <= 2 * C * ((2048 + cgroups - 1) // cgroups)
    assert lib.vp3d_train_reduce_doubles(-1, C, 1) == -1 and lib.vp3d_train_reduce_doubles(5, 0, 0) == -1
