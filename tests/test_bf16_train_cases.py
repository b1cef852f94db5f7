"""CPU self-check of the bf16 training tests' yardstick (tests/bf16_train_cases.py), from the
oracle alone:

  * with the float32 plain bf16-operand oracle standing in for the device, the teacher-forced
    float64 oracle agrees with its operand rows but for a share <= 1e-3 of the elements, all
    neighbouring bf16 values, on every input tests/test_gpu_train_bf16.py uses -- the condition
    under which that test's cap of 2e-3 checks the device's rounding and not the oracle's;
  * the stand-in then passes the output gates with room, and the bf16 effect itself (against the
    plain float64 oracle) is far beyond them, so a missing rounding cannot pass;
  * truncation instead of rounding disagrees on about half the elements;
  * the shim leaves oracle.train_ref as it found it;
  * --train-dtype parses and is refused with --evaluate.
"""
import numpy as np
import pytest
import torch

import bf16_train_cases as BT
import train_cases as TC


@pytest.mark.parametrize("cid", BT.ALL_ROWS)
def test_standin_device_passes_the_operand_condition(cid):
    c = BT.row(cid)
    dev, o64, o32, report = BT.standin(cid)
    worst = BT.check_operands(cid, report, BT.n_block_convs(c), cap=BT.STANDIN_SHARE_CAP)
    print(f"{cid}: worst share {worst:.2e}")
    y, loss, grads, stats = dev
    rel = BT.check_outputs(cid, (y, loss, grads), o64, o32, stats)
    print(f"{cid}: worst gradient tensor {rel:.2e}")
    if cid in BT.WIDE:
        return
    # the bf16 effect: every block conv's weight gradient moves by >= 1e-2 against the plain
    # float64 oracle (measured >= 3e-2), two orders over the gradient gate's 1e-4 floor
    x, tgt = BT.row_inputs(cid)
    masks = TC.numpy_masks(c) if c.p > 0 else None
    _, _, g_plain, _ = TC._oracle(BT.row_state(cid), x, tgt, TC.meta_of(c), p=c.p, masks=masks, dtype=torch.float64)
    for k in g_plain:
        if k.startswith("layers_conv"):
            move = TC.rel_err(o64[2][k], g_plain[k])
            print(f"{cid} {k}: bf16 effect {move:.2e}")
            assert move >= 1e-2, (k, move)


def test_truncation_fails_the_operand_condition():
    """An operand truncated to bf16 instead of rounded differs from round_bf16 on about half the
    elements: check 1 sees it."""
    cid = "w5expand_traj_c64"
    c = BT.row(cid)
    x, tgt = BT.row_inputs(cid)
    with BT.bf16_oracle() as st:
        TC._oracle(BT.row_state(cid), x, tgt, TC.meta_of(c), p=c.p)
        acts = dict(st["acts"])
    torch.manual_seed(0)
    report = []
    for l, a in acts.items():
        raw = a * (1 + torch.rand_like(a) * 2.0 ** -6)  # spread over a few bf16 cells
        trunc = (raw.contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32)
        BT.compare_operand("act", l, raw, trunc, report)
        BT.compare_operand("grad", l, raw, trunc, report)
        nonzero = float((a != 0).double().mean())
        assert report[-1]["share"] > 0.4 * nonzero > 0.1, (report[-1], nonzero)
        assert report[-1]["step"] == 1
    with pytest.raises(AssertionError):
        BT.check_operands("truncated", report, len(acts))


def test_shim_restores_the_oracle():
    import torch.nn.functional as F

    import oracle.train_ref as TR
    assert TR.F is F
    with BT.bf16_oracle() as st:
        assert TR.F is not F and TR.F.relu is F.relu
        assert st["calls"] == 0
    assert TR.F is F
    with pytest.raises(RuntimeError):
        with BT.bf16_oracle():
            raise RuntimeError("inside")
    assert TR.F is F


def test_round_bf16_and_ordinals():
    t = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8, 0.0])
    r = BT.round_bf16(t)
    assert r.tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, -1.0, 0.0]  # ties to even
    a = torch.tensor([1.0, -1.0, 2.0 ** -126])
    b = torch.tensor([1.0 + 2.0 ** -7, -1.0 - 2.0 ** -7, 2.0 ** -126 * (1 + 2.0 ** -7)])
    assert (BT._ordinal(b) - BT._ordinal(a)).abs().tolist() == [1, 1, 1]


def test_train_dtype_argument():
    from common.arguments import parse_args
    assert parse_args([]).train_dtype == "fp32"
    assert parse_args(["--train-dtype", "bf16"]).train_dtype == "bf16"
    assert parse_args(["--train-dtype", "bf16", "--compute-dtype", "f16x3"]).compute_dtype == "f16x3"
    with pytest.raises(SystemExit):
        parse_args(["--train-dtype", "fp16"])
    with pytest.raises(SystemExit):
        parse_args(["--train-dtype", "bf16", "--evaluate", "synthetic"])
    assert parse_args(["--evaluate", "synthetic"]).train_dtype == "fp32"
