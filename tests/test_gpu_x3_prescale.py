"""The calibrated power-of-two activation pre-scale of the f16x3 path, on the device.

The split-fp16 path stores every activation as hi = f16(a), lo = f16(a - hi); below |a| = 2^-3
lo is an f16 subnormal, so a checkpoint with small hidden activations
(oracle.x3_model.rescale_activations(sd, s): every hidden activation x 2^-s, the function
unchanged) loses accuracy without a fault.  With a pre-scale, layer l's stored rows hold
a * 2^p[l]: folded into the f16x3 epilogue vectors on the host, exact, no kernel changed.

Shapes (the ones of tests/test_gpu_x3_numerics.py, whose inputs, weight families and gates are
imported, not edited):
  A  config 4 (1,024 channels, fw 3,3,3,3,3, strided) at the 24 edge windows: the small kernels
  B  the same tiled to B = 1,032: block 1 on a4, the later blocks on their tail plans
  C  128 channels, fw 3,5,3, B = 5: the pack path, K = 640
  D  the dilated TemporalModel on one 25,000-frame sequence: a4 dilated + split-K tails
  E  the 23-"joint" trajectory model through forward_windows with cameras, 8 windows

Everything that is asserted bit for bit follows from the fold being powers of two only; the
tolerance between forced kernel forms (5e-6 m) is the one tests/test_gpu_lifter.py uses between
forms that sum in different orders (test_dilated_seq_split_tail, test_x3_split_shrink).  Those
tests set it on poses of 0.11 m rms; where the edge windows are compared (the x 32 window's poses
are 3.4 m rms) it is applied in the scaled metres of test_gpu_x3_numerics -- a window's error
over max(1, rms / 0.11).  Measured on MI355X: q64, the packed expand and the half-N tails give
the default dispatch's bits at B = 24; the exact-f32 shrink differs from the split shrink by
8.1e-6 m raw on the x 32 window, 3.8e-7 scaled m.
"""
import numpy as np
import pytest
import torch

from helpers import make_model
from oracle.temporal_ref import lifter_forward
from oracle.x3_model import lifter_forward_x3, rescale_activations
from test_gpu_x3_numerics import (FP32_COORD_TOL, FP32_MPJPE_TOL, FW4, R3, RMS_REF, _check, edge_windows,
                                  family_state)
from vp3d_amd import synth
from vp3d_amd.x3_prescale import chain_layers, choose_prescale, exponent_for

pytestmark = pytest.mark.gpu

FORM_TOL = 5e-6  # m, between forms that sum in different orders (module docstring)
FWC = (3, 5, 3)
_MODELS = {}
_CACHE = {}


def _model(kind):
    """One module per kind, kept on the device; every test leaves it without a pre-scale."""
    if kind not in _MODELS:
        if kind == "c4":
            m, sd = make_model(True, FW4, False, 1024)
        elif kind == "c128":
            m, sd = make_model(True, FWC, False, 128)
        elif kind == "seq":
            m, sd = make_model(False, FW4, False, 1024)
        elif kind == "traj":
            m, sd = make_model(True, jin=23, channels=1024, seed=0)
        _MODELS[kind] = (m.cuda(), sd)
    m, sd = _MODELS[kind]
    m.set_f16x3_prescale(None)
    return m, sd


def _load(model, sd):
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})


def _fwd(model, x, dtype="f16x3"):
    model.set_compute_dtype(dtype)
    with torch.no_grad():
        y = model(x)
    model.sync_status()  # the range guard and the split-K watchdog stay silent
    return y.cpu().numpy()


def _inputs(shape):
    """(model kind, filter widths, device input, slice of the output that is compared)."""
    if shape not in _CACHE:
        if shape == "A":
            x = edge_windows()
        elif shape == "B":
            x = np.tile(edge_windows(), (43, 1, 1, 1))
            assert x.shape[0] == 1032
        elif shape == "C":
            x = synth.normalized_windows(1, "x5_45", 5, 45).copy()
            x[1] = 0.0
            x[3] *= np.float32(32.0)
        elif shape == "D":
            x = synth.normalized_windows(1, "x1_25000", 1, 25000).copy()
            x[0, 100:140] = 0.0
            x[0, 24800:24840:2] = 1.0
            x[0, 24801:24840:2] = -1.0
        _CACHE[shape] = torch.from_numpy(x).cuda()
    kind = {"A": "c4", "B": "c4", "C": "c128", "D": "seq"}[shape]
    return kind, _CACHE[shape]


def _sel(shape, y):
    """D is compared on its first and last 64 poses (the last ones come from the tail rows)."""
    return np.concatenate([y[0, :64], y[0, -64:]]) if shape == "D" else y


# ---- 1. invariance ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["A", "B", "C", "D"])
def test_calibrated_forward_is_invariant_to_the_activation_scale(shape):
    """calibrate_f16x3 on rescale_activations(sd, s), then the f16x3 forward: the bits of the
    same on the base checkpoint, the chosen exponents moved by exactly s, no fault."""
    kind, x = _inputs(shape)
    model, sd = _model(kind)
    _load(model, sd)
    p0, stats0 = model.calibrate_f16x3(x)
    assert model.f16x3_prescale() == p0 and model.native_lifter().x3_prescale() == p0
    assert any(p0), p0
    y0 = _sel(shape, _fwd(model, x))
    assert np.isfinite(y0).all()
    print(f"X3PRE {shape} base exponents {p0} absmax {[round(s['absmax'], 3) for s in stats0]} "
          f"small_share {[round(s['small_share'], 4) for s in stats0]}")
    try:
        for s in (4, 10, 14):
            model.set_f16x3_prescale(None)
            _load(model, rescale_activations(sd, s))
            ps, stats = model.calibrate_f16x3(x)
            print(f"X3PRE {shape} s={s} exponents {ps}")
            assert ps == [v + s for v in p0], (s, ps, p0)
            for a, b in zip(stats, stats0):  # the fp32 activations are exactly 2^-s times the base ones
                assert a["absmax"] == b["absmax"] * 2.0 ** -s and a["small_share"] >= b["small_share"]
            ys = _sel(shape, _fwd(model, x))
            assert np.array_equal(ys, y0), (s, np.abs(ys - y0).max())
    finally:
        model.set_f16x3_prescale(None)


# ---- 2. equivalence to the oracle's rescale -----------------------------------------------------
@pytest.mark.parametrize("p", [-2, 3])
@pytest.mark.parametrize("shape", ["A", "C"])
def test_uniform_prescale_equals_the_rescaled_checkpoint(shape, p):
    """set_f16x3_prescale([p] * n) on sd = no pre-scale on rescale_activations(sd, -p), bit for bit."""
    kind, x = _inputs(shape)
    model, sd = _model(kind)
    n = len(model.f16x3_prescale())
    _load(model, rescale_activations(sd, -p))
    want = _fwd(model, x)
    _load(model, sd)
    model.set_f16x3_prescale([p] * n)
    try:
        got = _fwd(model, x)
    finally:
        model.set_f16x3_prescale(None)
    assert np.array_equal(got, want), np.abs(got - want).max()
    assert not np.array_equal(got, _fwd(model, x))  # the stored rows did move


# ---- 3. accuracy ----------------------------------------------------------------------------------
def _refs(family, sd_s, p_chain=None):
    """ref64 and ref32 of the family on the 24 edge windows and, with p_chain, the split model of
    the checkpoint rescaled by it -- computed once each and left unchanged."""
    xs = edge_windows()
    flat = lambda t: t.numpy().reshape((-1,) + tuple(t.shape[2:]))
    if ("refs", family) not in _CACHE:
        _CACHE[("refs", family)] = (flat(lifter_forward(sd_s, xs, list(FW4), strided=True, dtype=torch.float64)),
                                    flat(lifter_forward(sd_s, xs, list(FW4), strided=True)))
    if p_chain is None:
        return _CACHE[("refs", family)]
    if ("mod", family, p_chain) not in _CACHE:
        _CACHE[("mod", family, p_chain)] = flat(
            lifter_forward_x3(rescale_activations(sd_s, -p_chain), xs, list(FW4), strided=True))
    return _CACHE[("refs", family)] + (_CACHE[("mod", family, p_chain)],)


@pytest.mark.parametrize("shape", ["A", "B"])
@pytest.mark.parametrize("family", ["act_10", "act_14"])
def test_calibrated_small_activation_checkpoints_meet_the_gates(family, shape):
    """act_10 and act_14, calibrated, pass gates 1 and 2 of test_gpu_x3_numerics._check (act_10
    is exempt from gate 1 there; not here).  e_model is the split model of the checkpoint
    rescaled by the chain exponent, so the chain exponent is set on every layer for this case.
    Uncalibrated, act_14 is past gate 1 (the representation alone gives 2.5e-4 m)."""
    kind, x = _inputs(shape)
    model, sd = _model(kind)
    sd_s = family_state(sd, family)
    _load(model, sd_s)
    reps = x.shape[0] // 24
    tile = lambda a: np.broadcast_to(a, (reps,) + a.shape).reshape((-1,) + a.shape[1:])
    if family == "act_14":
        raw = _fwd(model, x).reshape(-1, 17, 3)
        r64 = tile(_refs(family, sd_s)[0])
        rms = np.sqrt((r64.reshape(len(r64), -1) ** 2).mean(axis=1))
        e_raw = (np.abs(raw - r64).reshape(len(r64), -1).max(axis=1) / np.maximum(1.0, rms / RMS_REF)).max()
        print(f"X3PRE {shape}/{family} uncalibrated e_x3 {e_raw:.3e} scaled m")
        assert e_raw > FP32_COORD_TOL, e_raw
    p, _ = model.calibrate_f16x3(x)
    p_chain = p[0]
    model.set_f16x3_prescale([p_chain] * len(p))
    try:
        ref64, ref32, mod = _refs(family, sd_s, p_chain)
        y_x3 = _fwd(model, x).reshape(-1, 17, 3)
        y_f32 = _fwd(model, x, "fp32").reshape(-1, 17, 3)
    finally:
        model.set_f16x3_prescale(None)
    assert R3 == 4.0 and FP32_MPJPE_TOL == 1e-7
    _check(f"prescale/{shape}/{family}/p{p_chain}", tile(ref64), tile(ref32), tile(mod), y_x3, y_f32, gate1_x3=True)


# ---- 4. zero is today ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["A", "B", "C", "D"])
def test_zero_prescale_is_the_unscaled_forward(shape):
    """All-zero exponents set, then cleared: the bits from before any call.  The fp32, bf16 and
    fp16 outputs do not move when a non-zero pre-scale is set."""
    kind, x = _inputs(shape)
    model, sd = _model(kind)
    _load(model, sd)
    n = len(model.f16x3_prescale())
    before = {d: _fwd(model, x, d) for d in ("f16x3", "fp32", "bf16", "fp16")}
    model.set_f16x3_prescale([0] * n)
    assert model.native_lifter().x3_prescale() == [0] * n
    assert np.array_equal(_fwd(model, x), before["f16x3"])
    nz = [3 if l in chain_layers(model.filter_widths) else -2 for l in range(n)]
    model.set_f16x3_prescale(nz)
    try:
        assert model.native_lifter().x3_prescale() == nz
        for d in ("fp32", "bf16", "fp16"):
            assert np.array_equal(_fwd(model, x, d), before[d]), d
        scaled = _fwd(model, x)
        assert np.abs(scaled - before["f16x3"]).max() <= FORM_TOL  # (another rounding of the same values)
    finally:
        model.set_f16x3_prescale(None)
    assert np.array_equal(_fwd(model, x), before["f16x3"])


def _traj_setup():
    from vp3d_amd.pipeline import SyntheticWindowPool
    model, sd = _model("traj")
    dev = torch.device("cuda", torch.cuda.current_device())
    if "traj" not in _CACHE:
        pool = SyntheticWindowPool(1000, dev, cameras=True)
        _CACHE["traj"] = (pool, torch.from_numpy(pool.global_pairs(8)).to(dev))
    pool, pairs = _CACHE["traj"]
    return model, sd, pool, pairs, dev


def test_zero_prescale_trajectory_windows():
    """E: forward_windows with the camera concat (bf16 is refused there).  Zero is today; a
    uniform p equals the rescaled checkpoint; the windows twin of the calibration sees the values
    the gathered batch has."""
    model, sd, pool, pairs, dev = _traj_setup()
    _load(model, sd)
    lifter = model.native_lifter(dev)

    def fw(dtype="f16x3"):
        with torch.no_grad():
            y = lifter.forward_windows(pool.seqs, pairs, 243, 121, concat_cams=True, dtype=dtype)
        lifter.sync_status()
        return y.cpu().numpy()

    before = {d: fw(d) for d in ("f16x3", "fp32", "fp16")}
    n = len(model.f16x3_prescale())
    model.set_f16x3_prescale([0] * n)
    assert np.array_equal(fw(), before["f16x3"])
    try:
        model.set_f16x3_prescale([3] * n)
        assert model.native_lifter(dev) is lifter and lifter.x3_prescale() == [3] * n
        got = fw()
        for d in ("fp32", "fp16"):
            assert np.array_equal(fw(d), before[d]), d
    finally:
        model.set_f16x3_prescale(None)
    assert np.array_equal(fw(), before["f16x3"])
    _load(model, rescale_activations(sd, -3))
    assert model.native_lifter(dev) is lifter
    assert np.array_equal(fw(), got)
    _load(model, sd)
    lifter = model.native_lifter(dev)
    x = pool.seqs.gather(pairs, 243, 121, "2d", concat_cams=True).view(8, 243, 23, 2)
    sw = lifter.calibrate_x3(seqs=pool.seqs, pairs=pairs, window=243, lead=121, concat_cams=True)
    sx = lifter.calibrate_x3(x)
    assert len(sw) == n
    for a, b in zip(sw, sx):
        assert a["absmax"] == b["absmax"] and a["small_share"] == b["small_share"]
        assert abs(a["rms"] - b["rms"]) <= 1e-12 * b["rms"]


# ---- 5. forced forms ---------------------------------------------------------------------------------
def _forced(model, x, monkeypatch, env):
    for k in ("VP3D_GEMM", "VP3D_X3_EXPAND", "VP3D_X3_EXPAND_RING", "VP3D_A4_TAIL", "VP3D_X3_SHRINK",
              "VP3D_A4_HN", "VP3D_A4_SPLIT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return _fwd(model, x)


def test_forced_forms_take_the_folded_vectors(monkeypatch):
    """A, exponents (3 on the chain, 5 on the k-convs): every forced form against the default
    dispatch.  The exact-f32 shrink (VP3D_X3_SHRINK=f32: the last 1x1 stores f32 rows at the
    chain's scale) has its own 2^-p_chain scale vector."""
    kind, x = _inputs("A")
    model, sd = _model(kind)
    _load(model, sd)
    n = len(model.f16x3_prescale())
    plain = _forced(model, x, monkeypatch, {})
    # scaled metres as in test_gpu_x3_numerics: the x 32 window's poses are 3.4 m rms, 31 times the
    # 0.11 m outputs FORM_TOL was set on
    rms = np.sqrt((plain.astype(np.float64).reshape(24, -1) ** 2).mean(axis=1))
    scale = np.maximum(1.0, rms / RMS_REF)
    err = lambda a, b: float((np.abs(a.astype(np.float64) - b).reshape(24, -1).max(axis=1) / scale).max())
    model.set_f16x3_prescale([3 if l % 2 == 0 else 5 for l in range(n)])
    try:
        base = _forced(model, x, monkeypatch, {})
        assert err(base, plain) <= FORM_TOL
        for env in ({"VP3D_GEMM": "q64"}, {"VP3D_X3_EXPAND": "pack"}, {"VP3D_A4_TAIL": "hn"},
                    {"VP3D_X3_SHRINK": "f32"}):
            y = _forced(model, x, monkeypatch, env)
            d = err(y, base)
            print(f"X3PRE forced {env}: max|d| vs default {d:.3e} scaled m, raw {np.abs(y - base).max():.3e} m")
            assert np.isfinite(y).all() and d <= FORM_TOL, (env, d)
        # the exact-f32 shrink over pre-scaled f32 rows, held to case 2's identity: a uniform p
        # equals the checkpoint rescaled by -p under the same form, bit for bit
        model.set_f16x3_prescale([3] * n)
        got = _forced(model, x, monkeypatch, {"VP3D_X3_SHRINK": "f32"})
        model.set_f16x3_prescale(None)
        _load(model, rescale_activations(sd, -3))
        want = _forced(model, x, monkeypatch, {"VP3D_X3_SHRINK": "f32"})
        assert np.array_equal(got, want), np.abs(got - want).max()
    finally:
        model.set_f16x3_prescale(None)


def test_forced_expand_rings_bit_identical(monkeypatch):
    """B = 1,032 (where the weight-stationary expand applies): the RING = 1 / 2 / ws expand forms
    give one set of bits with a pre-scale as they do without (tests/test_gpu_expand_ws.py), and
    the half-N tails the bits of q64 (tests/test_gpu_lifter.py test_a4_half_n_tail_bit_identical)."""
    kind, x = _inputs("B")
    model, sd = _model(kind)
    _load(model, sd)
    n = len(model.f16x3_prescale())
    model.set_f16x3_prescale([3 if l % 2 == 0 else 5 for l in range(n)])
    try:
        ys = {r: _forced(model, x, monkeypatch, {"VP3D_X3_EXPAND_RING": r}) for r in ("ws", "1", "2")}
        assert np.array_equal(ys["ws"], ys["1"]), np.abs(ys["ws"] - ys["1"]).max()
        assert np.array_equal(ys["ws"], ys["2"]), np.abs(ys["ws"] - ys["2"]).max()
        whole = _forced(model, x, monkeypatch, {"VP3D_A4_HN": "0", "VP3D_A4_SPLIT": "0"})
        q64 = _forced(model, x, monkeypatch, {"VP3D_GEMM": "q64"})
        hn = _forced(model, x, monkeypatch, {"VP3D_A4_TAIL": "hn"})
        assert np.array_equal(whole, q64), np.abs(whole - q64).max()
        assert np.abs(hn - q64).max() <= FORM_TOL and np.abs(ys["ws"] - q64).max() <= FORM_TOL
    finally:
        model.set_f16x3_prescale(None)


# ---- 6. overflow still raises ------------------------------------------------------------------------
def test_too_large_a_prescale_raises_the_range_fault():
    """A chain exponent of +8 on the 24 edge windows (the x 32 window) puts a stored value past
    65,504: the host-visible fault word, raised at sync_status with the advice to re-calibrate.
    Cleared, the handle gives the unscaled bits again."""
    kind, x = _inputs("A")
    model, sd = _model(kind)
    _load(model, sd)
    n = len(model.f16x3_prescale())
    before = _fwd(model, x)
    model.set_f16x3_prescale([8] * n)
    try:
        model.set_compute_dtype("f16x3")
        with torch.no_grad():
            model(x)
        with pytest.raises(RuntimeError, match="re-calibrate with more headroom or clear the pre-scale"):
            model.sync_status()
    finally:
        model.set_f16x3_prescale(None)
    model.sync_status()  # cleared by the raise
    assert np.array_equal(_fwd(model, x), before)


# ---- 7. the statistics kernel -----------------------------------------------------------------------
def _expand_only_model(sd_c, zero_shift=False):
    """The expand conv of shape C (128 channels, 34 inputs, width 3) followed by a shrink that is
    the identity on the 128 channels (43 x 3 = 129 outputs, the last one zero): the native fp32
    forward then returns the expand layer's output rows themselves (a sum of one value and
    zeros is exact in any order)."""
    from common.models.TemporalModel import TemporalModelOptimized1f
    m = TemporalModelOptimized1f(17, 2, 43, [3], channels=128)
    sd = {k: np.array(v, copy=True) for k, v in sd_c.items() if k.startswith("expand_")}
    if zero_shift:
        sd["expand_bn.bias"][:] = 0.0
        sd["expand_bn.running_mean"][:] = 0.0
    w = np.zeros((129, 128, 1), np.float32)
    w[np.arange(128), np.arange(128), 0] = 1.0
    sd["shrink.weight"], sd["shrink.bias"] = w, np.zeros(129, np.float32)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.eval().cuda()


def test_stats_kernel_against_the_fp32_layer_output():
    """absmax bit-equal to torch.amax(abs), rms within 1e-6 relative and small_share exact, on
    the fp32 path's expand output of shape C (read back through an identity shrink; the forward
    has no per-layer hooks for the deeper layers, whose statistics are checked for consistency
    in the invariance case: exact 2^-s scaling of every absmax)."""
    kind, x = _inputs("C")
    model_c, sd_c = _model(kind)
    _load(model_c, sd_c)
    m = _expand_only_model(sd_c)
    rows = _fwd(m, x, "fp32").reshape(5, 15, 129)[..., :128].astype(np.float32)
    a = torch.from_numpy(rows)
    stats = m.native_lifter().calibrate_x3(x)
    assert len(stats) == 1
    s = stats[0]
    assert np.float32(s["absmax"]) == torch.amax(a.abs()).item() and s["absmax"] == float(np.float32(s["absmax"]))
    rms = float(np.sqrt(np.mean(rows.astype(np.float64) ** 2)))
    assert abs(s["rms"] - rms) <= 1e-6 * rms, (s["rms"], rms)
    small = int(((rows != 0) & (np.abs(rows) < 0.125)).sum())
    assert 0 < small < rows.size
    assert s["small_share"] == small / rows.size, (s["small_share"], small, rows.size)
    # the same layer inside the whole shape C model: the same numbers
    full = model_c.native_lifter().calibrate_x3(x)
    assert len(full) == 5 and all(np.isfinite(t["absmax"]) and t["absmax"] > 0 for t in full)
    assert full[0]["absmax"] == s["absmax"] and full[0]["small_share"] == s["small_share"]
    assert abs(full[0]["rms"] - s["rms"]) <= 1e-12 * s["rms"]


def test_stats_kernel_all_zero_batch():
    """Zero keypoints through a layer without a shift: absmax 0, rms 0, no small values, and the
    exponent 0."""
    kind, x = _inputs("C")
    _, sd_c = _model(kind)
    m = _expand_only_model(sd_c, zero_shift=True)
    p, stats = m.calibrate_f16x3(torch.zeros_like(x))
    assert stats[0]["absmax"] == 0.0 and stats[0]["rms"] == 0.0 and stats[0]["small_share"] == 0.0
    assert p == [0] and m.f16x3_prescale() == [0] and exponent_for(0.0) == 0
    assert choose_prescale(stats, [3]) == [0]


# ---- 8. refusals -----------------------------------------------------------------------------------
def test_refusals():
    kind, x = _inputs("C")
    model, sd = _model(kind)
    _load(model, sd)
    lifter = model.native_lifter()
    with pytest.raises(RuntimeError, match=r"layer 2 .*residual chain"):
        lifter.set_x3_prescale([3, 0, 4, 0, 3])
    with pytest.raises(RuntimeError, match=r"layer 3 has exponent 25"):
        lifter.set_x3_prescale([0, 0, 0, 25, 0])
    with pytest.raises(RuntimeError, match=r"layer 0 has exponent -25"):
        lifter.set_x3_prescale([-25, 0, -25, 0, -25])
    with pytest.raises(RuntimeError, match=r"expected 5 exponents"):
        lifter.set_x3_prescale([0, 0, 0])
    assert lifter.x3_prescale() == [0] * 5
    with pytest.raises(ValueError, match="layer 4"):
        model.set_f16x3_prescale([1, 0, 1, 0, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.calibrate_f16x3(x.cpu())
    model.train()
    try:
        with pytest.raises(RuntimeError, match="eval mode"):
            model.calibrate_f16x3(x)
    finally:
        model.eval()
    assert model.f16x3_prescale() == [0] * 5


# ---- 9. weights reloaded ---------------------------------------------------------------------------
def test_prescale_survives_a_weight_reload():
    """load_state_dict of another family after the exponents were set: the handle is reloaded
    and still applies them (case 2's identity on the new weights)."""
    kind, x = _inputs("C")
    model, sd = _model(kind)
    wide = family_state(sd, "wide")
    _load(model, rescale_activations(wide, -3))
    want = _fwd(model, x)
    _load(model, sd)
    model.set_f16x3_prescale([3] * 5)
    try:
        _fwd(model, x)
        _load(model, wide)
        got = _fwd(model, x)
        assert model.native_lifter().x3_prescale() == [3] * 5
    finally:
        model.set_f16x3_prescale(None)
    assert np.array_equal(got, want), np.abs(got - want).max()


# ---- 10. run.py --------------------------------------------------------------------------------------
def test_run_evaluate_with_x3_calibrate(capsys):
    """--evaluate synthetic --compute-dtype f16x3 --x3-calibrate 512 on the split of
    tests/test_run_eval.py: Protocol #1 within its 1e-4 mm of the run without the flag, and the
    INFO line."""
    import run
    from test_run_eval import _argv, _golden
    _, _, meta = _golden()
    argv = _argv(meta) + ["--compute-dtype", "f16x3"]
    plain = run.main(argv)
    capsys.readouterr()
    cal = run.main(argv + ["--x3-calibrate", "512"])
    out = capsys.readouterr().out
    info = [ln for ln in out.splitlines() if ln.startswith("INFO: f16x3 pre-scale calibrated")]
    assert len(info) == 1 and "chain exponent" in info[0] and "largest small_share" in info[0], out
    print(info[0])
    for k, v in plain["per_action"].items():
        assert abs(cal["per_action"][k][0] - v[0]) <= 1e-4, (k, cal["per_action"][k][0], v[0])
