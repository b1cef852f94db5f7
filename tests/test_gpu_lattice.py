"""Every lifter dtype and kernel form, bit for bit, on exact-lattice data (oracle/lattice.py).

On a lattice_state model with lattice_windows inputs no product, partial sum or store rounds, in
any dtype or summation order, so bf16, fp16, f16x3 and fp32 must all return the float64 poses of
oracle.lattice.lattice_forward exactly: every assertion here is np.array_equal, and a dropped
K-tile, a tap or residual row off by one, or a shift column from the wrong slot moves poses by
whole lattice units (tests/test_lattice.py seeds such defects into the CPU model).  H16_TOL
(tests/helpers.py) is left to measure the representation error on trained-like weights.

The float64 reference of a case is computed once on its distinct windows (tests/lattice_cases.py)
and tiled: strided windows are independent, and a sequence of period 82 gives poses of period
82; neither 41, 25 nor 82 divides the 256-row tile, so every tile sees another phase.  Which
kernel each layer of each case takes: profiles/lattice_exact.txt.
"""
import numpy as np
import pytest
import torch

import lattice_cases as LC
from helpers import make_model
from oracle import lattice as L

pytestmark = pytest.mark.gpu

KNOBS = ("VP3D_GEMM", "VP3D_A4_WALK", "VP3D_A4_SPLIT", "VP3D_A4_HN", "VP3D_A4_TAIL", "VP3D_EXPAND_SPLIT",
         "VP3D_X3_EXPAND", "VP3D_X3_SHRINK", "VP3D_X3_EXPAND_RING", "VP3D_F32_NARROW")
_MODELS = {}


def _model(case, sd, key=None):
    """The drop-in model of a case with its lattice state, on the GPU (one upload per case)."""
    key = key or case["name"]
    if key not in _MODELS:
        jin = sd["expand_conv.weight"].shape[1] // 2
        m, _ = make_model(case["strided"], case["fw"], case["causal"], case["channels"], jin=jin,
                          jout=case["jout"], dense=case["dense"])
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
        _MODELS[key] = m.eval().cuda()
    return _MODELS[key]


def _full(case, x, y):
    """(device input of the run's size, expected float32 poses): the oracle batch tiled."""
    if case["period"]:
        P, T = case["period"], case["T"]
        one = torch.from_numpy(x[:, :P]).cuda()
        xd = one.repeat(1, -(-T // P), 1, 1)[:, :T].contiguous()
        n_out = T - (x.shape[1] - P)
        assert y.shape[1] == P
        want = np.tile(y, (1, -(-n_out // P), 1, 1))[:, :n_out]
    else:
        B, reps = case["B"], -(-case["B"] // x.shape[0])
        xd = torch.from_numpy(x).cuda().repeat(reps, 1, 1, 1)[:B].contiguous()
        want = np.tile(y, (reps, 1, 1, 1))[:B]
    return xd, want.astype(np.float32)


def _same(got, want, what):
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = got != want
    if bad.any():
        where = np.argwhere(bad)
        d = np.abs(got.astype(np.float64) - want)
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} poses differ from the float64 lattice result, max "
                    f"{np.nanmax(d):.3e} m = {np.nanmax(d) / L.OUT_UNIT:.2f} lattice units; first at {where[0].tolist()}, "
                    f"last at {where[-1].tolist()}, finite {bool(np.isfinite(got).all())}")
    assert np.array_equal(got, want)


def _guarded(fn):
    """fn()'s poses as a numpy array.  A device fault ends the session: nothing more is launched
    on a device whose context has faulted."""
    try:
        return fn().cpu().numpy()
    except RuntimeError as e:
        if any(w in str(e).lower() for w in ("illegal memory", "hip error", "hardware exception", "unspecified launch")):
            pytest.exit(f"device fault, no further GPU tests: {e}", returncode=3)
        raise


def _forward(model, xd, dtype):
    """The model's native forward into a NaN-filled output: poses a form did not write cannot pass
    as the previous form's (the allocator hands the same block back)."""
    def run():
        lifter = model.native_lifter(torch.device("cuda"))
        out = torch.full((xd.shape[0], lifter.out_frames(xd.shape[1]), model.num_joints_out, 3), float("nan"),
                         device="cuda")
        lifter.forward(xd, dtype, out=out)
        lifter.sync_status()  # (an f16x3 range or split-K fault of this forward raises here)
        return out
    return _guarded(run)


def _env(monkeypatch, form):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in form.items():
        monkeypatch.setenv(k, v)


def _fid(form):
    return "default" if not form else "+".join(f"{k[5:].lower()}={v}" for k, v in form.items())


# ---- small shapes, default dispatch, every dtype ------------------------------------------------

_SMALL = [(c, dt) for c in LC.SMALL for dt in c["dtypes"]]


@pytest.mark.parametrize("case,dtype", _SMALL, ids=[f"{c['name']}-{dt}" for c, dt in _SMALL])
def test_small_shapes(case, dtype, monkeypatch):
    _env(monkeypatch, {})
    sd, x, y, _ = LC.build(case)
    xd, want = _full(case, x, y)
    _same(_forward(_model(case, sd), xd, dtype), want, f"{case['name']} {dtype}")


# ---- the 256 x 256 kernels at fill, every form ----------------------------------------------------

_H16_FORMS = [{}, {"VP3D_GEMM": "q64"}, {"VP3D_GEMM": "8p"}, {"VP3D_GEMM": "big"}, {"VP3D_GEMM": "h16"},
              {"VP3D_A4_WALK": "0"}, {"VP3D_A4_WALK": "2"}, {"VP3D_A4_SPLIT": "0"}, {"VP3D_A4_SPLIT": "2"},
              {"VP3D_A4_HN": "0", "VP3D_A4_SPLIT": "0"}, {"VP3D_A4_TAIL": "hn"}, {"VP3D_EXPAND_SPLIT": "0"}]
_X3_FORMS = [{}, {"VP3D_GEMM": "q64"}, {"VP3D_A4_WALK": "2"}, {"VP3D_A4_SPLIT": "0"}, {"VP3D_A4_SPLIT": "2"},
             {"VP3D_A4_HN": "0", "VP3D_A4_SPLIT": "0"}, {"VP3D_A4_TAIL": "hn"}, {"VP3D_EXPAND_SPLIT": "0"},
             {"VP3D_X3_EXPAND": "pack"}, {"VP3D_X3_SHRINK": "f32"}, {"VP3D_X3_SHRINK": "f32", "VP3D_F32_NARROW": "0"},
             {"VP3D_X3_EXPAND_RING": "2"}]
_F32_FORMS = [{}, {"VP3D_F32_NARROW": "0"}]
_HN_FORMS = [{}, {"VP3D_GEMM": "q64"}, {"VP3D_A4_HN": "0", "VP3D_A4_SPLIT": "0"}, {"VP3D_A4_SPLIT": "2"}]
_SEQ_H16 = [{}, {"VP3D_GEMM": "q64"}, {"VP3D_GEMM": "8p"}, {"VP3D_GEMM": "big"}, {"VP3D_GEMM": "h16"},
            {"VP3D_A4_TAIL": "hn"}, {"VP3D_A4_SPLIT": "0"}]
_SEQ_X3 = [{}, {"VP3D_GEMM": "q64"}, {"VP3D_A4_TAIL": "hn"}, {"VP3D_A4_SPLIT": "0"}, {"VP3D_X3_SHRINK": "f32"}]


def _interleave(**forms):
    """[(dtype, form)] with the dtypes taking turns: consecutive runs of a case never share a
    dtype, so activations a form failed to write are the previous run's in another encoding (the
    workspace is reused), not this run's right answer."""
    n = max(len(f) for f in forms.values())
    return [(dt, f[i]) for i in range(n) for dt, f in forms.items() if i < len(f)]


_FILL = _interleave(bf16=_H16_FORMS, f16x3=_X3_FORMS, fp16=_H16_FORMS, fp32=_F32_FORMS)
_FILL_HN = _interleave(bf16=_HN_FORMS, f16x3=_HN_FORMS, fp16=_HN_FORMS)
# the sequence: a4 is the default there (>= 384 tiles); the walk / half-N knobs act on the strided
# 1x1 layers and the partial rounds of the strided shapes
_SEQ = _interleave(bf16=_SEQ_H16, f16x3=_SEQ_X3, fp16=_SEQ_H16, fp32=[{}])
_DEV = {}


def _fill_run(case, dtype, form, monkeypatch):
    _env(monkeypatch, form)
    sd, x, y, _ = LC.build(case)
    key = (case["name"], case["B"])
    if key not in _DEV:
        _DEV.clear()  # one fill input resident at a time
        _DEV[key] = _full(case, x, y)
    xd, want = _DEV[key]
    _same(_forward(_model(case, sd), xd, dtype), want, f"{case['name']} B={case['B']} {dtype} {_fid(form)}")


@pytest.mark.parametrize("dtype,form", _FILL, ids=[f"{dt}-{_fid(f)}" for dt, f in _FILL])
def test_fill_strided_forms(dtype, form, monkeypatch):
    """B = 2050 windows of 243 frames at 1024 channels, the 41 oracle windows tiled 50 times."""
    _fill_run(LC.FILL_STRIDED, dtype, form, monkeypatch)


@pytest.mark.parametrize("dtype,form", _FILL_HN, ids=[f"{dt}-{_fid(f)}" for dt, f in _FILL_HN])
def test_fill_strided_partial_round_forms(dtype, form, monkeypatch):
    """B = 8192 windows (the shape of test_a4_half_n_tail_bit_identical and
    test_a4_split_k_last_round): every block leaves 128 tiles past its whole rounds, run as
    half-N tiles by default, as whole tiles, as 2 split-K units each, or on q64."""
    _fill_run(LC.FILL_STRIDED_HN, dtype, form, monkeypatch)


@pytest.mark.parametrize("dtype,form", _SEQ, ids=[f"{dt}-{_fid(f)}" for dt, f in _SEQ])
def test_fill_sequence_forms(dtype, form, monkeypatch):
    """One dilated sequence of 34,042 frames at 1024 channels, input of period 82."""
    _fill_run(LC.FILL_SEQ, dtype, form, monkeypatch)


# ---- forward_windows: the gather fused into the expand conv ---------------------------------------

_GATHER = [(c, cams, dt) for c in LC.GATHER for cams, dts in ((False, ("bf16", "fp16", "f16x3", "fp32")),
                                                              (True, ("fp16", "f16x3", "fp32"))) for dt in dts]


def _gather_case(case, cams):
    from vp3d_amd.pipeline import DeviceSequences
    seqs, cam, pairs, window, lead = LC.gather_source(case, cams)
    x = L.lattice_gather(seqs, pairs, window, lead, cam).reshape(len(pairs), window, -1, 2)
    key = f"{case['name']}_cams{int(cams)}"
    sd, _, y, _ = LC.build(case, x, key=key)
    ds = DeviceSequences([s.reshape(-1, 17, 2) for s in seqs], device="cuda")
    if cams:
        ds.cam = torch.from_numpy(np.concatenate(cam)).cuda()  # the per-frame K.E table, lattice rows
    return _model(case, sd, key), ds, torch.from_numpy(pairs).cuda(), window, lead, y.astype(np.float32)


def _gather_run(case, cams, dtype, form, monkeypatch):
    _env(monkeypatch, form)
    model, ds, pairs, window, lead, want = _gather_case(case, cams)
    lifter = model.native_lifter(torch.device("cuda"))

    def run():
        out = torch.full((len(pairs), 1, model.num_joints_out, 3), float("nan"), device="cuda")
        lifter.forward_windows(ds, pairs, window, lead, concat_cams=cams, dtype=dtype, out=out)
        lifter.sync_status()
        return out
    _same(_guarded(run), want, f"{case['name']} cams={cams} {dtype} {_fid(form)}")


@pytest.mark.parametrize("case,cams,dtype", _GATHER,
                         ids=[f"{c['name']}-{'cams' if k else 'nocams'}-{dt}" for c, k, dt in _GATHER])
def test_forward_windows(case, cams, dtype, monkeypatch):
    """Windows gathered on the fly (sequences of 19 and 57 frames under a 243-frame window, starts
    on every sequence's first and last frame: both ends overhang) against the oracle on the same
    windows gathered on the CPU."""
    _gather_run(case, cams, dtype, {}, monkeypatch)


_GATHER_FORMS = _interleave(bf16=[{"VP3D_EXPAND_SPLIT": "0"}],
                            f16x3=[{"VP3D_X3_EXPAND_RING": "2"}, {"VP3D_X3_EXPAND": "pack"}, {"VP3D_EXPAND_SPLIT": "0"}],
                            fp16=[{"VP3D_EXPAND_SPLIT": "0"}])


@pytest.mark.parametrize("dtype,form", _GATHER_FORMS, ids=[f"{dt}-{_fid(f)}" for dt, f in _GATHER_FORMS])
@pytest.mark.parametrize("case", LC.GATHER, ids=[c["name"] for c in LC.GATHER])
def test_forward_windows_expand_forms(case, dtype, form, monkeypatch):
    """The gathered expand's other forms (whole row blocks, the two-per-CU ring, pack + GEMM)."""
    _gather_run(case, False, dtype, form, monkeypatch)


@pytest.mark.parametrize("case", LC.GATHER, ids=[c["name"] for c in LC.GATHER])
def test_forward_windows_bf16_refused_with_cameras(case):
    model, ds, pairs, window, lead, _ = _gather_case(case, True)
    lifter = model.native_lifter(torch.device("cuda"))
    with pytest.raises(RuntimeError, match="bf16 is refused"):
        lifter.forward_windows(ds, pairs, window, lead, concat_cams=True, dtype="bf16")


# ---- f16x3 with a non-zero activation pre-scale ---------------------------------------------------

_PRESCALE = [c for c in LC.SMALL if c["name"] in ("s243_c1024_b300", "s243_causal_c64_b5", "d243_c1024_b1_t600")]


@pytest.mark.parametrize("chain,ks", [(2, (-1, 3, 0, 5)), (-3, (4, -2, 1, -4))], ids=["chain+2", "chain-3"])
@pytest.mark.parametrize("case", _PRESCALE, ids=[c["name"] for c in _PRESCALE])
def test_f16x3_prescale_same_bits(case, chain, ks, monkeypatch):
    """Stored rows a 2^p with a an integer <= 256 stay exact in f16 for these exponents
    (check_prescale_exact), so the pre-scaled forward returns the same bits; cleared afterwards."""
    _env(monkeypatch, {})
    sd, x, y, stats = LC.build(case)
    p = [chain]
    for k in ks:
        p += [k, chain]
    L.check_prescale_exact(stats, p)
    model = _model(case, sd)
    xd, want = _full(case, x, y)
    model.set_f16x3_prescale(p)
    try:
        assert model.native_lifter(torch.device("cuda")).x3_prescale() == p
        _same(_forward(model, xd, "f16x3"), want, f"{case['name']} f16x3 prescale {p}")
    finally:
        model.set_f16x3_prescale(None)


# ---- the gate bites: a weight zeroed on the device side shows as the CPU model says ---------------

@pytest.mark.parametrize("dtype", LC.DTYPES)
def test_zeroed_k_index_moves_the_poses(dtype, monkeypatch):
    """Control of the comparison itself.  The K index most channels of block 1's k-conv read is
    zeroed in the weights the model uploads: the poses equal the CPU model's seeded zero_k
    defect bit for bit, and differ from the sound reference on more than 1 % of the poses."""
    _env(monkeypatch, {})
    case = next(c for c in LC.SMALL if c["name"] == "s243_causal_c64_b5")
    sd, x, y, _ = LC.build(case)
    w = np.array(sd["layers_conv.0.weight"])
    k = L.most_read_k(w)
    w[:, k % w.shape[1], k // w.shape[1]] = 0.0
    geom = dict(causal=case["causal"], strided=case["strided"], dense=case["dense"])
    y_bad = L.lattice_forward(sd, x, case["fw"], defect=("zero_k", 1), **geom)
    assert (np.abs(y_bad - y) >= L.OUT_UNIT).mean() > 0.01
    model = _model(case, dict(sd, **{"layers_conv.0.weight": w}), key=case["name"] + "_zeroed")
    xd, want = _full(case, x, y_bad)
    _same(_forward(model, xd, dtype), want, f"{case['name']} zeroed K index {k} {dtype}")
