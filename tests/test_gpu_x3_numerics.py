"""The split-fp16 (`f16x3`) and fp32 lifters against the float64 oracle, on weights and inputs
shaped like trained ones.

Every case compares, on the same windows,

  ref64    oracle.temporal_ref.lifter_forward(dtype=float64)
  e_ref32  the fp32 CPU oracle's error against ref64 (the reference's own fp32 error)
  e_model  oracle.x3_model.lifter_forward_x3 against ref64 (what the split representation
           alone costs, exact accumulation)
  e_x3, e_f32  the native f16x3 / fp32 outputs against ref64

Errors are in scaled metres: a window's max |y - ref64| divided by max(1, rms_window / 0.11),
rms_window being ref64's (0.11 m is the output rms the 1e-5 m gate was set on, helpers.py), then
the max over the compared windows.  For outputs of up to 0.11 m rms that is plain metres; a
window whose outputs are 1.5 m rms (inputs x 32, or a shrink without attenuation) is held to
the same relative error instead of swamping the others.

Gate 1 (relative north star): every window within FP32_COORD_TOL, the pooled dMPJPE within
  FP32_MPJPE_TOL, both in scaled metres.  fp32: every family.  f16x3: every family but act_10
  (the representation alone gives 1.4e-5 m there: e_model below).
Gate 2 (tight): e_f32 <= R32 e_ref32 and e_x3 <= e_model + R3 e_ref32 -- f16x3 is held to its
  modelled representation error plus fp32-sized accumulation error at every activation scale,
  act_10 included.
Gate 3 (edges): the all-zero and the one-frame windows give finite poses, and the all-zero
  window's pose does not depend on its batch (a batch of one gives the same bits).

Weight families (pure transforms of the seed-0 synthetic state dict, `family_state`):
  base, signs (negative / zero / 1e-6 BN gammas), wide (log-uniform gammas and variances, large
  means), outlier (one weight per conv x 256: the per-layer 2^e), act_s (the exact rescale of
  every hidden activation by 2^-s, oracle.x3_model.rescale_activations).
Inputs: 24 windows, six of them edges (`edge_windows`).

R32 and R3 (gate 2) come from the measurement below: each is twice the largest value seen
over all cases, rounded up to one significant figure (the factor 2 for the batch-to-batch spread
of a max statistic over ~50 k coordinates).  Both measurements are under 4 (the ratio of the
split's 2^-22 representation bound to f32's 2^-24), past which they would not be gated but
reported as a finding.
  r32 = e_f32 / e_ref32:              largest 3.19 (dilated/seq25000/wide)  -> R32 = 7
  r3  = (e_x3 - e_model) / e_ref32:   largest 1.95 (strided/default/outlier) -> R3 = 4
The native fp32 path's own error is 2.2-3.2x the CPU oracle's on the 1,024-channel models (its
sums run in another order, on the f32 MFMA), 0.9-1.7x on the small ones; f16x3 is at or under
the native fp32 error down to act_4 and follows the model from act_6 on.

Measured on MI355X, 2026-10-19, build 9f79e036d70a4a9c (vp3d_build_hash), scaled metres
(profiles/x3_numerics_f64_oracle.txt has the whole lines, raw errors and window rms included):
  case                                   e_ref32   e_model      e_x3     e_f32   r32    r3
  strided/default/base                 1.791e-07 6.830e-08 3.447e-07 4.531e-07  2.53  1.54
  strided/default/signs                1.929e-07 5.446e-08 3.070e-07 4.832e-07  2.51  1.31
  strided/default/wide                 2.153e-07 7.143e-08 3.903e-07 4.636e-07  2.15  1.48
  strided/default/outlier              2.025e-07 7.052e-08 4.662e-07 5.507e-07  2.72  1.95
  strided/default/act_4                1.791e-07 1.946e-07 3.692e-07 4.531e-07  2.53  0.97
  strided/default/act_6                1.791e-07 7.539e-07 1.030e-06 4.531e-07  2.53  1.54
  strided/default/act_8                1.791e-07 3.740e-06 3.264e-06 4.531e-07  2.53 -2.65
  strided/default/act_10               1.791e-07 1.211e-05 1.092e-05 4.531e-07  2.53 -6.61
  strided/VP3D_GEMM=q64/base           1.791e-07 6.830e-08 3.447e-07 4.531e-07  2.53  1.54
  strided/VP3D_GEMM=q64/wide           2.153e-07 7.143e-08 3.903e-07 4.636e-07  2.15  1.48
  strided/VP3D_GEMM=q64/act_6          1.791e-07 7.539e-07 1.030e-06 4.531e-07  2.53  1.54
  strided/VP3D_X3_EXPAND=pack/base     1.791e-07 6.830e-08 3.447e-07 4.531e-07  2.53  1.54
  strided/VP3D_X3_EXPAND=pack/wide     2.153e-07 7.143e-08 3.903e-07 4.636e-07  2.15  1.48
  strided/VP3D_X3_EXPAND=pack/act_6    1.791e-07 7.539e-07 1.030e-06 4.531e-07  2.53  1.54
  strided/VP3D_X3_SHRINK=f32/base      1.791e-07 5.263e-08 3.998e-07 4.531e-07  2.53  1.94
  strided/VP3D_X3_SHRINK=f32/wide      2.153e-07 5.939e-08 4.608e-07 4.636e-07  2.15  1.86
  strided/VP3D_X3_SHRINK=f32/act_6     1.791e-07 7.943e-07 1.011e-06 4.531e-07  2.53  1.21
  strided/c128_fw353/base              6.206e-08 4.894e-08 6.729e-08 1.045e-07  1.68  0.30
  strided/c128_fw353/wide              1.114e-07 5.406e-08 1.308e-07 1.330e-07  1.19  0.69
  strided/c128_fw353/act_6             6.206e-08 3.656e-07 4.679e-07 1.045e-07  1.68  1.65
  dilated/seq25000/base                2.070e-07 7.018e-08 3.770e-07 5.572e-07  2.69  1.48
  dilated/seq25000/wide                2.340e-07 8.680e-08 4.436e-07 7.456e-07  3.19  1.52
  dilated/seq25000/act_6               2.070e-07 1.043e-06 1.153e-06 5.572e-07  2.69  0.53
  head/c256_fw33/base                  1.977e-07 6.337e-08 1.682e-07 1.971e-07  1.00  0.53
  head/c256_fw33/signs                 1.615e-07 7.474e-08 1.833e-07 1.991e-07  1.23  0.67
  head/c256_fw333/base                 1.930e-07 7.222e-08 1.977e-07 2.249e-07  1.17  0.65
  head/c256_fw333/signs                2.714e-07 8.676e-08 1.944e-07 2.437e-07  0.90  0.40
"""
import numpy as np
import pytest
import torch

from helpers import make_model, mpjpe_np
from oracle.temporal_ref import lifter_forward
from oracle.x3_model import lifter_forward_x3, rescale_activations
from vp3d_amd import synth

pytestmark = pytest.mark.gpu

FP32_COORD_TOL = 1e-5  # the north-star gates (test_gpu_lifter.py), on outputs of RMS_REF rms
FP32_MPJPE_TOL = 1e-7
RMS_REF = 0.11
# Gate 2's factors: twice the largest value measured over all cases (3.19, 1.95), rounded up to
# one significant figure (module docstring)
R32 = 7.0
R3 = 4.0

FW4 = (3, 3, 3, 3, 3)
FAMILIES = ("base", "signs", "wide", "outlier", "act_4", "act_6", "act_8", "act_10")
# edge windows: index in the batch of 24
W_ZERO, W_REPEAT, W_ALT, W_TINY, W_BIG, W_GAP = 3, 7, 11, 15, 19, 23


def edge_windows():
    """synth.normalized_windows(1, "x64_243", 24, 243) with six windows overwritten: all zeros
    (missed detections), one frame repeated, frames alternating +1 / -1, the window x 2^-10,
    the window x 32, and frames 100-139 zeroed with one f32 subnormal and one -0.0 in them."""
    x = synth.normalized_windows(1, "x64_243", 24, 243).copy()
    x[W_ZERO] = 0.0
    x[W_REPEAT] = x[W_REPEAT, 17:18]
    x[W_ALT, 0::2] = 1.0
    x[W_ALT, 1::2] = -1.0
    x[W_TINY] *= np.float32(2.0 ** -10)
    x[W_BIG] *= np.float32(32.0)
    x[W_GAP, 100:140] = 0.0
    x[W_GAP, 110, 3, 0] = np.float32(1e-40)
    x[W_GAP, 111, 5, 1] = np.float32(-0.0)
    assert x.dtype == np.float32 and x[W_GAP, 110, 3, 0] > 0 and np.signbit(x[W_GAP, 111, 5, 1])
    return x


def _bn_names(sd):
    return [k[:-len(".running_var")] for k in sd if k.endswith(".running_var")]


def family_state(sd, family):
    """The family's state dict (float32 numpy arrays) from the synthetic one; `sd` is not
    modified.  Random draws are synth's counter hash (seed 7), the same on every machine."""
    if family.startswith("act_"):
        return rescale_activations(sd, int(family[4:]))
    out = {k: np.array(v, copy=True) for k, v in sd.items()}
    if family == "base":
        return out
    if family == "signs":
        for bn in _bn_names(sd):
            g = out[bn + ".weight"]
            g[0::2] *= -1.0  # (the sign-balanced split weights negate the odd channels)
            g[5::97] = 0.0
            g[7::101] = 1e-6
        return out
    if family == "wide":
        for bn in _bn_names(sd):
            n = (out[bn + ".weight"].shape[0],)
            mag = np.exp(synth.uniform(7, bn + "/g", n, np.log(0.05), np.log(3.0)))
            sgn = np.where(synth.uniform(7, bn + "/s", n) < 0.5, -1.0, 1.0)
            out[bn + ".weight"] = (mag * sgn).astype(np.float32)
            out[bn + ".running_var"] = np.exp(synth.uniform(7, bn + "/v", n, np.log(0.2), np.log(20.0))).astype(np.float32)
            out[bn + ".running_mean"] = synth.uniform(7, bn + "/m", n, -1.0, 1.0).astype(np.float32)
            out[bn + ".bias"] = synth.uniform(7, bn + "/b", n, -0.5, 0.5).astype(np.float32)
        return out
    if family == "outlier":
        for k, v in out.items():
            if v.ndim == 3:  # every conv, the shrink included
                i = int(synth.bits(7, k + "/outlier", 1)[0] % np.uint64(v.size))
                v.reshape(-1)[i] *= 256.0
        return out
    raise KeyError(family)


# ---- references (CPU), computed once per (model, family, inputs) and left unchanged ----------
_MODELS = {}
_REFS = {}


def _model(strided, fw, channels, shrink_gain=0.05):
    key = (strided, tuple(fw), channels, shrink_gain)
    if key not in _MODELS:
        m, sd = make_model(strided, fw, False, channels, shrink_gain=shrink_gain)
        _MODELS[key] = (m.cuda(), sd)
    return _MODELS[key]


def _load(model, sd):
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})


def _refs(key, sd, xs, fw, strided, shrink_f32=False):
    """ref64, ref32 and the model's output on each window set of `xs` (a list), concatenated."""
    key = key + (shrink_f32,)
    if key not in _REFS:
        r64 = [lifter_forward(sd, x, list(fw), strided=strided, dtype=torch.float64).numpy() for x in xs]
        r32 = [lifter_forward(sd, x, list(fw), strided=strided).numpy() for x in xs]
        mod = [lifter_forward_x3(sd, x, list(fw), strided=strided, shrink_f32=shrink_f32).numpy() for x in xs]
        cat = (lambda a: np.concatenate([v.reshape((-1,) + v.shape[2:]) for v in a]))
        _REFS[key] = tuple(cat(a) for a in (r64, r32, mod))
        for a in _REFS[key]:
            a.setflags(write=False)
    return _REFS[key]


def _native(model, x, dtype):
    model.set_compute_dtype(dtype)
    with torch.no_grad():
        y = model(x)
    model.sync_status()  # raises on a range / split-K fault: the guard must stay silent here
    return y.cpu().numpy().astype(np.float64)


def _scaled_err(y, ref64, scale):
    """Per-window max |y - ref64| / scale: y, ref64 (W, J, 3), scale (W,)."""
    return np.abs(y - ref64).reshape(len(scale), -1).max(axis=1) / scale


def _check(case, ref64, ref32, mod, y_x3, y_f32, gate1_x3=True):
    """All gates on outputs flattened to (windows or frames, J, 3)."""
    W = ref64.shape[0]
    rms = np.sqrt((ref64.reshape(W, -1) ** 2).mean(axis=1))
    scale = np.maximum(1.0, rms / RMS_REF)
    gt = synth.gt_poses(3, "gt", W, ref64.shape[1])
    e = {n: _scaled_err(v, ref64, scale) for n, v in
         (("ref32", ref32), ("model", mod), ("x3", y_x3), ("f32", y_f32))}
    e_ref32, e_model, e_x3, e_f32 = (float(e[n].max()) for n in ("ref32", "model", "x3", "f32"))

    def d_mpjpe(y):  # pooled over the windows, each window's share over its scale
        per = [(mpjpe_np(y[w], gt[w]) - mpjpe_np(ref64[w], gt[w])) / scale[w] for w in range(W)]
        return abs(float(np.mean(per)))

    dm_x3, dm_f32 = d_mpjpe(y_x3), d_mpjpe(y_f32)
    r32 = e_f32 / e_ref32
    r3 = (e_x3 - e_model) / e_ref32
    raw = lambda v: float(np.abs(v - ref64).max())
    print(f"X3NUM {case}: e_ref32 {e_ref32:.3e} e_model {e_model:.3e} e_x3 {e_x3:.3e} e_f32 {e_f32:.3e} "
          f"[scaled m] r32 {r32:.2f} r3 {r3:.2f} dMPJPE x3 {dm_x3:.2e} f32 {dm_f32:.2e} "
          f"rms {rms.min():.3g}..{rms.max():.3g} raw max|d| ref32 {raw(ref32):.3e} model {raw(mod):.3e} "
          f"x3 {raw(y_x3):.3e} f32 {raw(y_f32):.3e}")
    assert np.isfinite(y_x3).all() and np.isfinite(y_f32).all()
    assert e_ref32 > 0
    # gate 1
    assert (e["f32"] <= FP32_COORD_TOL).all(), (case, "fp32", e_f32)
    assert dm_f32 <= FP32_MPJPE_TOL, (case, "fp32", dm_f32)
    if gate1_x3:
        assert (e["x3"] <= FP32_COORD_TOL).all(), (case, "f16x3", e_x3)
        assert dm_x3 <= FP32_MPJPE_TOL, (case, "f16x3", dm_x3)
    # gate 2
    assert e_f32 <= R32 * e_ref32, (case, e_f32, e_ref32, r32)
    assert e_x3 <= e_model + R3 * e_ref32, (case, e_x3, e_model, e_ref32, r3)


# act_10 on f16x3: the split representation alone (exact accumulation, e_model) gives 1.4e-5 m
# on these windows, past the 1e-5 m north-star gate; gate 2 still holds it to the model
_NO_GATE1_X3 = ("act_10",)


@pytest.mark.parametrize("family", FAMILIES)
def test_strided_default_dispatch(family):
    """Config 4 at B = 1,032 (the 24 windows tiled 43 times): block 1 has 27,864 rows = 109
    row tiles x 4 = 436 tiles of 256 x 256, the smallest tiling past the 384 tiles from which
    the default dispatch runs it on the one-wave-per-SIMD a4 kernel; the later blocks take
    their tail plans.  Every one of the 1,032 poses is checked against its oracle value, and
    the 43 tiles against each other bit for bit."""
    model, sd0 = _model(True, FW4, 1024)
    sd = family_state(sd0, family)
    xs = edge_windows()
    ref64, ref32, mod = _refs(("c4", family), sd, [xs], FW4, True)
    _load(model, sd)
    reps = 43
    x = torch.from_numpy(xs).cuda().repeat(reps, 1, 1, 1)
    assert x.shape[0] == 1032
    ys = {}
    for dtype in ("f16x3", "fp32"):
        y = _native(model, x, dtype)
        assert y.shape == (1032, 1, 17, 3)
        ys[dtype] = y.reshape((reps,) + ref64.shape)
        for r in range(1, reps):
            assert np.array_equal(ys[dtype][r], ys[dtype][0]), (dtype, r)
    tile = lambda a: np.broadcast_to(a, (reps,) + a.shape).reshape((-1,) + a.shape[1:])
    _check(f"strided/default/{family}", tile(ref64), tile(ref32), tile(mod),
           ys["f16x3"].reshape(tile(ref64).shape), ys["fp32"].reshape(tile(ref64).shape),
           gate1_x3=family not in _NO_GATE1_X3)
    # gate 3: the edge windows are finite on their own (not only through a max over the batch) ...
    for w in (W_ZERO, W_REPEAT):
        assert np.isfinite(ys["f16x3"][:, w]).all(), w
    if family == "base":
        # ... and the all-zero window alone in a batch gives the same bits as in any position
        alone = _native(model, torch.from_numpy(xs[W_ZERO:W_ZERO + 1]).cuda(), "f16x3")
        assert alone.shape == (1, 1, 17, 3)
        assert np.array_equal(alone[0, 0], ys["f16x3"][0, W_ZERO]), np.abs(alone[0, 0] - ys["f16x3"][0, W_ZERO]).max()
        assert np.array_equal(alone[0, 0], ys["f16x3"][reps - 1, W_ZERO])


@pytest.mark.parametrize("family", ["base", "wide", "act_6"])
@pytest.mark.parametrize("env", ["VP3D_GEMM=q64", "VP3D_X3_EXPAND=pack", "VP3D_X3_SHRINK=f32"])
def test_strided_forced_kernels(env, family, monkeypatch):
    """Config 4 at B = 24 with the block convs forced onto q64, the expand onto the packed-rows
    path, and the shrink onto the exact-f32 GEMM (the model then with its exact shrink)."""
    k, v = env.split("=")
    monkeypatch.setenv(k, v)
    shrink_f32 = env == "VP3D_X3_SHRINK=f32"
    model, sd0 = _model(True, FW4, 1024)
    sd = family_state(sd0, family)
    xs = edge_windows()
    ref64, ref32, mod = _refs(("c4", family), sd, [xs], FW4, True, shrink_f32)
    _load(model, sd)
    x = torch.from_numpy(xs).cuda()
    y_x3 = _native(model, x, "f16x3").reshape(ref64.shape)
    y_f32 = _native(model, x, "fp32").reshape(ref64.shape)
    _check(f"strided/{env}/{family}", ref64, ref32, mod, y_x3, y_f32)
    for w in (W_ZERO, W_REPEAT):
        assert np.isfinite(y_x3[w]).all(), w


@pytest.mark.parametrize("family", ["base", "wide", "act_6"])
def test_strided_small_pack_path(family):
    """128 channels, fw = (3, 5, 3), B = 5 (45 frames): a width-5 block conv (K = 640) and the
    plans of shapes too small for the 256-wide kernels.  One window all zeros, one x 32."""
    fw = (3, 5, 3)
    model, sd0 = _model(True, fw, 128)
    sd = family_state(sd0, family)
    xs = synth.normalized_windows(1, "x5_45", 5, 45).copy()
    xs[1] = 0.0
    xs[3] *= np.float32(32.0)
    ref64, ref32, mod = _refs(("s128", family), sd, [xs], fw, True)
    _load(model, sd)
    x = torch.from_numpy(xs).cuda()
    y_x3 = _native(model, x, "f16x3").reshape(ref64.shape)
    y_f32 = _native(model, x, "fp32").reshape(ref64.shape)
    _check(f"strided/c128_fw353/{family}", ref64, ref32, mod, y_x3, y_f32)
    assert np.isfinite(y_x3[1]).all()


@pytest.mark.parametrize("family", ["base", "wide", "act_6"])
def test_dilated_sequence(family):
    """TemporalModel on one sequence of 25,000 frames: every block layer has >= 384 tiles (the
    dilated convs on a4) plus a partial round (the split-K tail kernels).  Against the oracle
    on the first and the last 64 poses (the last ones come from the tail rows); frames 100-139
    (in the first slice) are zeroed and frames 24,800-24,839 (in the last) alternate +1 / -1."""
    model, sd0 = _model(False, FW4, 1024)
    sd = family_state(sd0, family)
    T, P = 25000, 64
    xs = synth.normalized_windows(1, "x1_25000", 1, T).copy()
    xs[0, 100:140] = 0.0
    xs[0, 24800:24840:2] = 1.0
    xs[0, 24801:24840:2] = -1.0
    n_out = T - 242
    los = (0, n_out - P)
    ref64, ref32, mod = _refs(("seq", family), sd, [xs[:, lo:lo + P + 242] for lo in los], FW4, False)
    _load(model, sd)
    x = torch.from_numpy(xs).cuda()
    sl = lambda y: np.concatenate([y[0, lo:lo + P] for lo in los])
    y_x3 = _native(model, x, "f16x3")
    y_f32 = _native(model, x, "fp32")
    assert y_x3.shape == (1, n_out, 17, 3)
    assert np.isfinite(y_x3).all() and np.isfinite(y_f32).all()
    _check(f"dilated/seq25000/{family}", ref64, ref32, mod, sl(y_x3), sl(y_f32))


@pytest.mark.parametrize("family", ["base", "signs"])
@pytest.mark.parametrize("fw", [(3, 3), (3, 3, 3)])
def test_unattenuated_head(fw, family):
    """shrink_gain = 1.0 (the default 0.05 attenuates the conv stack's error 20-fold before any
    gate sees it), 256 channels, B = 64, one and two blocks: a single layer's error reaches
    the output undiluted."""
    model, sd0 = _model(True, fw, 256, shrink_gain=1.0)
    sd = family_state(sd0, family)
    T = int(np.prod(fw))
    xs = synth.normalized_windows(1, f"x64_{T}", 64, T).copy()
    xs[5] = 0.0
    xs[9] = xs[9, 1:2]
    ref64, ref32, mod = _refs(("head", fw, family), sd, [xs], fw, True)
    _load(model, sd)
    x = torch.from_numpy(xs).cuda()
    y_x3 = _native(model, x, "f16x3").reshape(ref64.shape)
    y_f32 = _native(model, x, "fp32").reshape(ref64.shape)
    _check(f"head/c256_fw{''.join(map(str, fw))}/{family}", ref64, ref32, mod, y_x3, y_f32)
    for w in (5, 9):
        assert np.isfinite(y_x3[w]).all(), w
