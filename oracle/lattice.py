"""ORACLE (test infrastructure only): exact-lattice weights and inputs for the lifter.

Every input, weight, folded BN constant and stored activation of a `lattice_state` model on
`lattice_windows` inputs is a small integer times a power of two:

  inputs        multiples of 1/8 in [-1, 1] (camera rows of the trajectory form too)
  expand conv   sparse +-8 (products are integers); every 8th channel carries 256 and 128 on two
                K indices and the BN shift -257, whose bf16 form is hi = -256, lo = -1 (the
                only shift with a non-zero lo column of the BN-folded expand weights)
  block convs   sparse +-1, every K index (tap x input channel) used, signs alternating
  BN            gamma 1, running_mean 0, running_var float32(0.99999) -- 1.0f / sqrt(var +
                1e-5f) is exactly 1 in f32 -- beta an integer chosen per channel on a
                calibration batch so that activations neither die nor pass the cap
  shrink        +-1/256, bias in multiples of 1/64: poses on the lattice 2^-8 m

So every 16-bit product and every f32 partial sum is exact in any summation order and every
store is exact in bf16 (integers <= 256): bf16, fp16, f16x3 (all lo halves zero) and fp32 must
return `lattice_forward`'s float64 result bit for bit on every kernel form.  `check_exact`
asserts these premises on a case; a test calls it before trusting the case.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from .temporal_ref import _t, geometry
from .x3_model import folded_bn, split_weights

VAR_ONE = np.float32(0.99999)  # 1.0f / sqrt(VAR_ONE + 1e-5f) == 1.0f
ACT_LIMIT = 256.0              # integers up to here are exact in bf16 (8 significant bits)
SUM_LIMIT = 2.0 ** 20          # cap of sum |a w| in lattice units (f32 holds 2^24)
OUT_UNIT = 2.0 ** -8           # the poses' lattice (metres)
LO_SHIFT = -257.0              # bf16: hi -256 + lo -1; exact in fp16 and f32
DEFECTS = ("zero_k", "tap_shift", "res_row", "shift_lo")  # (the fifth, pairs one frame off: lattice_gather)


def keys_shapes(jin, fw, channels, jout=17, fin=2, dense=False):
    """(name, shape) of every state_dict entry of TemporalModel / TemporalModelOptimized1f."""
    _, _, convs = geometry(list(fw), False, not dense, dense)
    ks = [("expand_conv.weight", (channels, jin * fin, fw[0]))]
    bn = lambda n: [(f"{n}.weight", (channels,)), (f"{n}.bias", (channels,)), (f"{n}.running_mean", (channels,)),
                    (f"{n}.running_var", (channels,)), (f"{n}.num_batches_tracked", ())]
    ks += bn("expand_bn")
    for i, (k, _, _) in enumerate(convs):
        ks.append((f"layers_conv.{2 * i}.weight", (channels, channels, k)))
        ks.append((f"layers_conv.{2 * i + 1}.weight", (channels, channels, 1)))
    for i in range(2 * len(convs)):
        ks += bn(f"layers_bn.{i}")
    ks += [("shrink.weight", (jout * 3, channels, 1)), ("shrink.bias", (jout * 3,))]
    return ks


def lattice_windows(seed, B, T, jin=17, fin=2):
    """(B, T, jin, fin) float32, multiples of 1/8 in [-1, 1] (jin = 23: the 6 camera pairs of the
    trajectory form are rows like any other)."""
    rng = np.random.RandomState(seed)
    return (rng.randint(-8, 9, size=(B, T, jin, fin)) / 8.0).astype(np.float32)


def lattice_gather(seqs, pairs, window, lead, cams=None, frame_off=0):
    """Window b = frames [start_b - lead, start_b - lead + window) of sequence seq_b, edge-clamped,
    (with `cams`: the 12 camera channels after each frame's keypoints) as vp3d_forward_windows
    gathers them.  seqs / cams: lists of (T_i, F) arrays.  frame_off: the seeded defect (every
    pair read that many frames off).  Returns (B, window, F [+ 12])."""
    out = []
    for s, st in np.asarray(pairs):
        n = seqs[s].shape[0]
        idx = np.clip(np.arange(window) + int(st) - lead + frame_off, 0, n - 1)
        rows = seqs[s].reshape(n, -1)[idx]
        if cams is not None:
            rows = np.concatenate([rows, cams[s].reshape(n, -1)[idx]], axis=1)
        out.append(rows)
    return np.stack(out).astype(np.float32)


def _sparse(rng, cout, cin, taps, value, nnz_min, rows=None):
    """(cout, cin, taps) with +-value on a dealt permutation of the K = taps * cin indices: every
    K index lands in some row of `rows` (default all), each row gets the same count (>= nnz_min),
    signs alternating within a row from a random start."""
    K = cin * taps
    rows = np.arange(cout) if rows is None else np.asarray(rows)
    nnz = max(nnz_min, -(-K // len(rows)))
    slots = np.concatenate([rng.permutation(K), rng.randint(0, K, size=nnz * len(rows) - K)])
    w = np.zeros((cout, K), dtype=np.float32)
    first = rng.randint(0, 2, size=len(rows))
    for j in range(nnz):
        idx = slots[j * len(rows):(j + 1) * len(rows)]
        w[rows, idx] = value * np.where((first + j) % 2 == 0, 1.0, -1.0)
    # K index = tap * cin + channel
    return np.ascontiguousarray(w.reshape(cout, taps, cin).transpose(0, 2, 1))


def _res_slice(h, i, filter_widths, pad, shift, strided, row_off=0):
    """The residual rows of block i (0-based) out of the block input h (B, C, L)."""
    L = h.shape[2]
    if strided:
        w = filter_widths[i + 1]
        idx = torch.arange(shift[i + 1] + w // 2, L, w)
    else:
        p, c = pad[i + 1], shift[i + 1]
        idx = torch.arange(p + c, L - p + c)
    if row_off and int(idx[-1]) + row_off > L - 1:
        row_off = -row_off  # (the seeded defect, at the block input's last row: one row earlier)
    return h[:, :, idx + row_off]


def _conv(h, w, stride=1, dilation=1, tap_shift=None):
    """conv1d in float64; tap_shift = k: tap k reads one frame later (edge-clamped)."""
    z = F.conv1d(h, w, None, stride=stride, dilation=dilation)
    if tap_shift is not None:
        n = z.shape[2]
        base = tap_shift * dilation + stride * torch.arange(n)
        wk = w[:, :, tap_shift:tap_shift + 1]
        z = z - F.conv1d(h[:, :, base], wk) + F.conv1d(h[:, :, torch.clamp(base + 1, 0, h.shape[2] - 1)], wk)
    return z


def most_read_k(w):
    """The K index (tap * cin + channel) of a (cout, cin, taps) weight that most output channels read."""
    nz = np.asarray(w) != 0
    return int(nz.sum(axis=0).T.reshape(-1).argmax())


def _round_trip(h, dt):
    return bool((h.to(dt).to(torch.float64) == h).all())


def _stat(stats, name, h, a=None, w=None, unit=1.0, **kw):
    """One record per stored activation h; a, w: the conv that made it (for sum |a w|)."""
    if stats is None:
        return
    rec = dict(layer=name, max=float(h.abs().max()), nonzero=float((h != 0).double().mean()),
               bf16_exact=_round_trip(h, torch.bfloat16), f16_exact=_round_trip(h, torch.float16), unit=unit)
    if a is not None:
        rec["abs_sum_units"] = float(F.conv1d(a.abs(), w.abs(), None, **kw).max()) / unit
    stats.append(rec)


def lattice_forward(state, x, filter_widths, causal=False, strided=False, dense=False, eps=1e-5, stats=None,
                    defect=None):
    """float64 poses (B, T', J_out, 3) as a numpy array.  BN folded as upload_weights folds it
    (oracle.x3_model.folded_bn: scale and shift rounded to f32 step by step), everything else
    float64 -- exact on lattice data.  stats: a list that receives one dict per stored activation
    (the input, every layer's output after the residual add, the poses): max, nonzero share,
    bf16 / f16 round-trip exactness and the conv's max sum |a w| in lattice units.
    defect: a seeded defect of this CPU model only -- (kind, layer[, index]) with kind in
      zero_k     weight K index `index` (tap * cin + channel; None: the one most output channels
                 read) of conv `layer` zeroed in every output channel
      tap_shift  tap `index` of conv `layer` reads one frame later
      res_row    the residual slice of 1x1 conv `layer` starts one row later (where that passes
                 the block input's end, one row earlier)
      shift_lo   the expand's shift keeps only its bf16 hi half (layer 0)
    with `layer` the conv's position (0 expand, 1.. the block convs, last the shrink)."""
    sd = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v))
          for k, v in state.items() if not k.endswith("num_batches_tracked")}
    fw = list(filter_widths)
    xt = _t(x, torch.float64)
    B, T = xt.shape[0], xt.shape[1]
    pad, shift, convs = geometry(fw, causal, strided, dense)
    kind, dl, di = (tuple(defect) + (None, None))[:3] if defect else (None, None, None)
    assert kind is None or kind in DEFECTS, kind

    def weight(name, li):
        w = _t(sd[name], torch.float64).clone()
        if kind == "zero_k" and dl == li:
            cin = w.shape[1]
            k = di if di is not None else most_read_k(w)
            w[:, k % cin, k // cin] = 0.0
        return w

    def tap(li):
        return di if kind == "tap_shift" and dl == li else None

    def bn_relu(z, name, li):
        sc, sh = folded_bn(sd, name, eps)
        if kind == "shift_lo" and dl == li:
            sh = sh.to(torch.bfloat16).to(torch.float64)
        return F.relu(z * sc[None, :, None] + sh[None, :, None])

    with torch.no_grad():
        h = xt.reshape(B, T, -1).permute(0, 2, 1).contiguous()
        _stat(stats, "input", h, unit=0.125)
        w = weight("expand_conv.weight", 0)
        kw = dict(stride=fw[0] if strided else 1)
        a, h = h, bn_relu(_conv(h, w, tap_shift=tap(0), **kw), "expand_bn", 0)
        _stat(stats, "expand", h, a, w, **kw)
        for i, (k, d, s) in enumerate(convs):
            l1, l2 = 1 + 2 * i, 2 + 2 * i
            res = _res_slice(h, i, fw, pad, shift, strided, 1 if kind == "res_row" and dl == l2 else 0)
            w = weight(f"layers_conv.{2 * i}.weight", l1)
            kw = dict(stride=s, dilation=d)
            a, h = h, bn_relu(_conv(h, w, tap_shift=tap(l1), **kw), f"layers_bn.{2 * i}", l1)
            _stat(stats, f"block{i + 1}.k{k}", h, a, w, **kw)
            w = weight(f"layers_conv.{2 * i + 1}.weight", l2)
            a, h = h, res + bn_relu(_conv(h, w, tap_shift=tap(l2)), f"layers_bn.{2 * i + 1}", l2)
            _stat(stats, f"block{i + 1}.1x1", h, a, w)
        w = weight("shrink.weight", 1 + 2 * len(convs))
        a, h = h, F.conv1d(h, w, None) + _t(sd["shrink.bias"], torch.float64)[None, :, None]
        _stat(stats, "shrink", h, a, w, unit=OUT_UNIT)
        return h.permute(0, 2, 1).reshape(B, h.shape[2], -1, 3).numpy()


def lattice_emulate(state, x, filter_widths, dt, causal=False, strided=False, dense=False, eps=1e-5):
    """The native 16-bit arithmetic restated in torch (after tools/bf16_error_study.emulate, any
    geometry): input, weights and every stored activation rounded to `dt`, f32 accumulation
    (torch's CPU conv1d, whatever order its threads sum in), the BN fold in f32.  float32 poses."""
    r = lambda t: t.to(dt).float()
    sd = {k: _t(v, torch.float32) for k, v in state.items() if not k.endswith("num_batches_tracked")}
    fw = list(filter_widths)
    pad, shift, convs = geometry(fw, causal, strided, dense)

    def fold(name):
        sc = (1.0 / torch.sqrt(sd[name + ".running_var"] + np.float32(eps))) * sd[name + ".weight"]
        return sc[None, :, None], (sd[name + ".bias"] - sd[name + ".running_mean"] * sc)[None, :, None]

    xt = _t(x, torch.float32)
    B, T = xt.shape[0], xt.shape[1]
    with torch.no_grad():
        h = r(xt.reshape(B, T, -1).permute(0, 2, 1).contiguous())
        sc, sh = fold("expand_bn")
        h = r(F.relu(F.conv1d(h, r(sd["expand_conv.weight"]), None, stride=fw[0] if strided else 1) * sc + sh))
        for i, (k, d, s) in enumerate(convs):
            res = _res_slice(h, i, fw, pad, shift, strided)
            sc, sh = fold(f"layers_bn.{2 * i}")
            h = r(F.relu(F.conv1d(h, r(sd[f"layers_conv.{2 * i}.weight"]), None, stride=s, dilation=d) * sc + sh))
            sc, sh = fold(f"layers_bn.{2 * i + 1}")
            h = r(res + F.relu(F.conv1d(h, r(sd[f"layers_conv.{2 * i + 1}.weight"]), None) * sc + sh))
        h = F.conv1d(h, r(sd["shrink.weight"]), sd["shrink.bias"])
        return h.permute(0, 2, 1).reshape(B, h.shape[2], -1, 3).numpy()


def lattice_state(keys_shapes, seed, filter_widths, causal=False, strided=False, dense=False, calib=None,
                  cap=None):
    """A state_dict (float32 arrays) of the kind the module docstring describes, for the model
    whose entries are `keys_shapes` (any filter widths, dense, causal, channel and joint counts).
    The integer BN biases are set layer by layer on a calibration batch: one minus the floor of
    the channel's median pre-activation (half of a k-conv's outputs alive, 40 % of a 1x1's), lowered where
    needed so that no stored activation of the batch passes `cap`.  calib: (B, T, J, 2) lattice
    inputs, usually the very windows the case runs (cap 240: the bound then holds on them by
    construction); None: 8 windows of lattice_windows (cap 160, the margin to 256 being for other
    inputs -- the tails are long).  check_exact decides per case either way."""
    shapes = {k: tuple(s) for k, s in keys_shapes}
    rng = np.random.RandomState(seed)
    fw = list(filter_widths)
    pad, shift, convs = geometry(fw, causal, strided, dense)
    C, cin, _ = shapes["expand_conv.weight"]
    rf = 1 + 2 * sum(geometry(fw, False, False)[0])
    assert cin % 2 == 0, "rows are (joints, 2) pairs"
    if cap is None:
        cap = 160.0 if calib is None else 240.0
    xs = calib
    if xs is None:
        xs = lattice_windows(seed + 7919, 8 if strided else 2, rf if strided else rf + 48, jin=cin // 2)
    xs = np.asarray(xs, dtype=np.float32)
    sd = {}

    def put_bn(name, beta):
        sd[name + ".weight"] = np.ones(C, np.float32)
        sd[name + ".bias"] = beta.astype(np.float32)
        sd[name + ".running_mean"] = np.zeros(C, np.float32)
        sd[name + ".running_var"] = np.full(C, VAR_ONE, np.float32)
        if name + ".num_batches_tracked" in shapes:
            sd[name + ".num_batches_tracked"] = np.zeros((), np.int64)

    def beta_for(z, q, res=None):
        """z: (B, C, L) pre-activations.  1 - floor(quantile q): everything from the quantile up is
        alive (a single sample too); lowered to keep res + relu(z + b) <= cap."""
        zc = z.permute(1, 0, 2).reshape(C, -1)
        b = 1.0 - torch.floor(torch.quantile(zc, q, dim=1))
        room = cap - zc if res is None else cap - res.permute(1, 0, 2).reshape(C, -1) - zc
        return torch.minimum(b, torch.floor(room.min(dim=1).values)).numpy()

    with torch.no_grad():
        h = _t(xs, torch.float64).reshape(xs.shape[0], xs.shape[1], -1).permute(0, 2, 1).contiguous()
        lo_rows = np.arange(3, C, 8)
        plain = np.setdiff1d(np.arange(C), lo_rows)
        w = _sparse(rng, C, cin, fw[0], 8.0, 3, rows=plain)
        K = cin * fw[0]
        wk = w.transpose(0, 2, 1).reshape(C, K)
        # (B, K, L): the expand's im2col rows, to place the lo rows' two weights where they fire
        cols = F.unfold(h[:, :, None, :], (1, fw[0]), stride=(1, fw[0] if strided else 1))
        cols = cols.reshape(h.shape[0], cin, fw[0], -1).permute(0, 2, 1, 3).reshape(h.shape[0], K, -1)
        for o in lo_rows:
            best = None
            for _ in range(8):  # of 8 random placements the one alive most often on the batch
                k2 = rng.choice(K, size=2, replace=False)
                v2 = np.array([256.0, 128.0]) * rng.choice([-1.0, 1.0], size=2)
                alive = int((cols[:, k2[0]] * v2[0] + cols[:, k2[1]] * v2[1] + LO_SHIFT > 0).sum())
                if best is None or alive > best[0]:
                    best = (alive, k2, v2)
            wk[o, best[1]] = best[2]
        w = np.ascontiguousarray(wk.reshape(C, fw[0], cin).transpose(0, 2, 1))
        sd["expand_conv.weight"] = w
        z = F.conv1d(h, _t(w, torch.float64), None, stride=fw[0] if strided else 1)
        beta = beta_for(z, 0.5)
        beta[lo_rows] = LO_SHIFT
        put_bn("expand_bn", beta)
        h = F.relu(z + _t(beta, torch.float64)[None, :, None])
        for i, (k, d, s) in enumerate(convs):
            res = _res_slice(h, i, fw, pad, shift, strided)
            w = _sparse(rng, C, C, k, 1.0, 3)
            sd[f"layers_conv.{2 * i}.weight"] = w
            z = F.conv1d(h, _t(w, torch.float64), None, stride=s, dilation=d)
            beta = beta_for(z, 0.5)
            put_bn(f"layers_bn.{2 * i}", beta)
            h = F.relu(z + _t(beta, torch.float64)[None, :, None])
            w = _sparse(rng, C, C, 1, 1.0, 2)
            sd[f"layers_conv.{2 * i + 1}.weight"] = w
            z = F.conv1d(h, _t(w, torch.float64), None)
            beta = beta_for(z, 0.6, res)
            put_bn(f"layers_bn.{2 * i + 1}", beta)
            h = res + F.relu(z + _t(beta, torch.float64)[None, :, None])
    n_out = shapes["shrink.weight"][0]
    sd["shrink.weight"] = _sparse(rng, n_out, C, 1, 1.0 / 256.0, min(40, C))
    sd["shrink.bias"] = (rng.randint(-64, 65, size=n_out) / 64.0).astype(np.float32)
    assert set(sd) == set(shapes), set(shapes) ^ set(sd)
    return sd


def _is_pow2(v):
    m, _ = np.frexp(np.asarray(v, dtype=np.float64))
    return bool(np.all(m == 0.5))


def _multiple(v, unit):
    q = np.asarray(v, dtype=np.float64) / unit
    return bool(np.all(q == np.round(q)))


def check_exact(state, x, filter_widths, causal=False, strided=False, dense=False, eps=1e-5, x3_prescale=None):
    """Assert the premises under which every dtype must return lattice_forward's bits on this
    case (module docstring); returns (poses float64, per-layer stats).
      (a) every folded BN scale is a power of two, every folded shift an integer, the shrink
          bias a multiple of the output lattice;
      (b) every stored activation (the input, each layer's output after the residual) is
          unchanged by a round trip through bfloat16 (and float16);
      (c) every conv's sum |a w| (plus |shift|) is <= 2^20 of its lattice units;
      (d) every weight, and the BN-folded expand weight, is exact in bf16 and fp16, and
          W 2^e (oracle.x3_model.weight_exponent's e) has a zero lo half;
      (e) every K index of every conv is used and >= 25 % of each stored activation is non-zero.
    x3_prescale: the f16x3 exponents p (one per conv layer output); a 2^p must stay exact in f16."""
    sd = {k: np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v)
          for k, v in state.items() if not k.endswith("num_batches_tracked")}
    n_conv = sum(1 for k in sd if k.startswith("layers_conv."))
    bns = ["expand_bn"] + [f"layers_bn.{i}" for i in range(n_conv)]
    ws = ["expand_conv.weight"] + [f"layers_conv.{i}.weight" for i in range(n_conv)] + ["shrink.weight"]
    shifts = []
    for name in bns:  # (a)
        sc, sh = folded_bn(sd, name, eps)
        assert _is_pow2(sc.numpy()), name
        assert _multiple(sh.numpy(), 1.0), name
        shifts.append(float(sh.abs().max()))
    assert _multiple(sd["shrink.bias"], OUT_UNIT)
    shifts.append(float(np.abs(sd["shrink.bias"]).max()) / OUT_UNIT)
    sc0 = folded_bn(sd, "expand_bn", eps)[0].numpy()
    for name in ws:  # (d), (e)
        w = np.asarray(sd[name], dtype=np.float32)
        wt = torch.from_numpy(w)
        forms = [wt] if name != "expand_conv.weight" else [wt, wt * torch.from_numpy(sc0.astype(np.float32))[:, None, None]]
        for f in forms:
            assert torch.equal(f.to(torch.bfloat16).float(), f), name
            assert torch.equal(f.to(torch.float16).float(), f), name
        hi, lo, _ = split_weights(w)
        assert float(lo.abs().max()) == 0.0 and bool(torch.isfinite(hi).all()), name
        assert bool((np.abs(w).max(axis=0) > 0).all()), f"{name}: a K index is unused"
    stats = []
    y = lattice_forward(sd, x, filter_widths, causal, strided, dense, eps, stats=stats)
    for j, rec in enumerate(stats):
        stored = rec["layer"] != "shrink"
        if stored:  # (b), (e)
            assert rec["bf16_exact"] and rec["f16_exact"], rec
            assert rec["max"] <= ACT_LIMIT, rec
            assert rec["nonzero"] >= 0.25, rec
        if "abs_sum_units" in rec:  # (c)
            assert rec["abs_sum_units"] + shifts[j - 1] <= SUM_LIMIT, rec
    assert _multiple(y, OUT_UNIT)
    assert np.array_equal(y.astype(np.float32).astype(np.float64), y)
    if x3_prescale is not None:
        check_prescale_exact(stats, x3_prescale)
    return y, stats


def check_prescale_exact(stats, p):
    """The f16x3 activation pre-scale p (one exponent per conv layer output) keeps a case exact:
    the stored rows a 2^p are integers <= 256 times a power of two inside f16's normal range."""
    assert len(p) == len(stats) - 2, (len(p), len(stats))
    for e, rec in zip(p, stats[1:-1]):
        assert rec["max"] * 2.0 ** e <= 2.0 ** 15 and 2.0 ** e >= 2.0 ** -14, (e, rec)


def format_stats(stats):
    return "\n".join(f"  {r['layer']:<12s} max {r['max']:8.4f}  nonzero {100 * r['nonzero']:5.1f} %"
                     + (f"  max sum|a w| {r['abs_sum_units']:8.0f} units" if "abs_sum_units" in r else "")
                     for r in stats)
