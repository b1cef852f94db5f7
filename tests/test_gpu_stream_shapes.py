"""The causal streaming step on the shapes of tests/stream_cases.py: every branch of the host
dispatch (csrc/vp3d_capi.cpp: stream_pipe_setup, stream_persist_setup, vp3d_stream_create) and
the three device forms behind it (stream_pipe.hip, stream_persist.hip, stream_step.hip), against
the float64 oracle of oracle/stream_ref.py.

Gate (stream_cases.TOL_COORD, TOL_DMPJPE): 2e-5 m per coordinate and |dMPJPE| <= 1e-7 m, the
project's fp32 stream gates, for fp32, fp16 AND bf16 weights.  The streams keep f32 activations
and round only the weights, so the oracle is evaluated on the same rounded weights
(round_weights) and the rounding is not part of the difference; what is left is the order of the
f32 sums.  The float32 CPU oracle itself lies within 8.3e-7 m of the float64 one on these cases
(tests/test_stream_cases.py), so the coordinate gate keeps about 25 times headroom, while a
wrong tap, a stale ring slot or a zeroed input moves the poses by 4e-4 m or more.  Measured on
an MI355X (profiles/stream_shapes.txt): at most 2.7e-7 m and 1.5e-5 mm, over every case, dtype
and form.

Beyond the per-shape comparison: a reset onto ANOTHER sequence (stale history would show; after
replaying the same sequence it cannot), two streams of one lifter interleaved, the serve form
without the folded shrink, and graph replay in the two fallback forms.
"""
import numpy as np
import pytest
import torch

import stream_cases as sc
from helpers import make_model
from vp3d_amd import synth
from vp3d_amd.stream import CausalStream

pytestmark = pytest.mark.gpu


def _model(name):
    m, _ = sc.case_model(name)
    return m.cuda()


def _frames(name, which="B", T=None):
    return torch.tensor(sc.case_input(name, which, T)[0]).cuda()


def _set_mode(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("VP3D_STREAM_MODE", raising=False)
    else:
        monkeypatch.setenv("VP3D_STREAM_MODE", mode)


def _stream_all(st, xs):
    out = torch.stack([st.step(xs[t]).clone() for t in range(xs.shape[0])]).cpu().numpy()
    st.check()
    return out


def _gate(label, out, name, dtype, which="B", T=None):
    ref = sc.oracle_poses(name, dtype, which, T)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    err = float(np.abs(out - ref).max())
    dm = sc.dmpjpe(out, ref)
    print(f"stream_shape {name} {dtype} {label}: max|d|={err:.3e} m, dMPJPE={dm * 1e3:.3e} mm")
    assert err <= sc.TOL_COORD, (label, err)
    assert dm <= sc.TOL_DMPJPE, (label, dm)


@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_stream_shape_forms(name, dtype, monkeypatch):
    """With VP3D_STREAM_MODE unset, then launches / persist / pipe: the dispatch picks the form
    the case table pins, and all T poses of that form meet the gate."""
    c = sc.case(name)
    m = _model(name)
    xs = _frames(name)
    for mode in sc.MODES:
        _set_mode(monkeypatch, mode)
        st = CausalStream(m.native_lifter(), dtype)
        assert st.mode == sc.expected_form(name, dtype, mode), (mode, st.mode)
        assert st.persistent == (st.mode != "launches")
        out = _stream_all(st, xs)
        _gate(f"mode={mode or 'unset'} form={st.mode}", out, name, dtype)
        assert st.frames_seen() == c.T
        st.close()


def test_stream_refuses_wide_layer():
    """(3, 5, 3) at 1024 channels: the 5-tap k-conv has K = 5120 > the 4096 inputs a GEMV
    stages; no form takes it and creation says so."""
    m, _ = make_model(False, sc.REFUSED["fw"], causal=True, channels=sc.REFUSED["channels"])
    m.cuda()
    for dtype in sc.DTYPES:
        with pytest.raises(RuntimeError, match=sc.REFUSED["match"]):
            CausalStream(m.native_lifter(), dtype)


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("name,mode", [("jin21", "pipe"), ("c512", "persist"), ("width7", "persist"),
                                       ("dense", "launches"), ("one_width", "launches")])
def test_stream_reset_onto_another_sequence(name, mode, dtype, monkeypatch):
    """vp3d_stream_reset clears the position (and the pipe's granules) but neither the rings nor
    the persistent forms' saved state: the t == 0 branches of every kernel must re-seed ALL
    history.  37 frames of sequence A (another seed, three times the amplitude), reset, then B:
    B's poses meet the gate and equal, bit for bit, B on a stream that never saw A."""
    monkeypatch.delenv("VP3D_STREAM_MODE", raising=False)
    assert sc.expected_form(name, "fp16", None) == mode
    form = sc.expected_form(name, dtype, None)  # fp32 has no persist form: launches there
    m = _model(name)
    xa, xb = _frames(name, "A", 37), _frames(name)
    st = CausalStream(m.native_lifter(), dtype)
    assert st.mode == form
    a = _stream_all(st, xa)
    _gate(f"form={form} A before reset", a, name, dtype, "A", 37)
    assert st.frames_seen() == 37
    st.reset()
    assert st.frames_seen() == 0
    b = _stream_all(st, xb)
    _gate(f"form={form} B after reset", b, name, dtype)
    fresh = CausalStream(m.native_lifter(), dtype)
    assert fresh.mode == form
    np.testing.assert_array_equal(b, _stream_all(fresh, xb))


@pytest.mark.parametrize("name,fold", [("jin21", True), ("jout32", False)])
def test_stream_serve_reset_onto_another_sequence(name, fold, monkeypatch):
    """The serve form after a reset onto another sequence, with the shrink folded into the last
    1x1 (jin21) and -- 96 outputs do not fit the fold's 64-granule slots -- with the shrink
    role's all-gather (jout32).  Served poses meet the gate, lie within 1e-6 m of the batch
    form (the fold's other summation order), and without the fold equal it bit for bit."""
    monkeypatch.delenv("VP3D_STREAM_MODE", raising=False)
    monkeypatch.delenv("VP3D_STREAM_FOLD", raising=False)
    c = sc.case(name)
    m = _model(name)
    xa, xb = sc.case_input(name, "A", 37)[0], sc.case_input(name)[0]
    st = CausalStream(m.native_lifter(), "fp16")
    assert st.mode == "pipe"
    with st.serve(idle_ms=500.0) as sv:
        a = np.stack([sv.step(xa[t]) for t in range(37)])
    st.check()
    assert st.frames_seen() == 37
    _gate("serve A before reset", a, name, "fp16", "A", 37)
    st.reset()
    with st.serve(idle_ms=500.0) as sv:
        b = np.stack([sv.step(xb[t]) for t in range(c.T)])
    st.check()
    assert st.frames_seen() == c.T
    _gate(f"serve B after reset fold={int(fold)}", b, name, "fp16")
    batch = _stream_all(CausalStream(m.native_lifter(), "fp16"), _frames(name))
    d = float(np.abs(b - batch).max())
    print(f"stream_shape {name} fp16 serve vs batch: max|d|={d:.3e} m")
    assert d <= 1e-6
    if fold:
        assert d > 0.0  # the fold is really on: another order of the shrink's sum
    else:
        np.testing.assert_array_equal(b, batch)


@pytest.mark.parametrize("name,mode", [("jin21", "pipe"), ("c512", "persist"), ("expand5", "launches")])
def test_two_streams_do_not_share_state(name, mode, monkeypatch):
    """Two streams of ONE lifter stepped alternately (A0, B0, A1, B1, ...): rings, granules,
    saved state and the position are per stream, so each one's poses equal, bit for bit, the
    same sequence streamed alone."""
    monkeypatch.delenv("VP3D_STREAM_MODE", raising=False)
    c = sc.case(name)
    m = _model(name)
    lifter = m.native_lifter()
    xa, xb = _frames(name, "A", c.T), _frames(name)
    sa, sb = CausalStream(lifter, "fp16"), CausalStream(lifter, "fp16")
    assert sa.mode == sb.mode == mode == sc.expected_form(name, "fp16", None)
    assert sa.lifter is sb.lifter
    a, b = [], []
    for t in range(c.T):
        a.append(sa.step(xa[t]).clone())
        b.append(sb.step(xb[t]).clone())
    sa.check()
    sb.check()
    a, b = torch.stack(a).cpu().numpy(), torch.stack(b).cpu().numpy()
    assert sa.frames_seen() == sb.frames_seen() == c.T
    _gate(f"form={mode} A interleaved", a, name, "fp16", "A", c.T)
    _gate(f"form={mode} B interleaved", b, name, "fp16")
    np.testing.assert_array_equal(a, _stream_all(CausalStream(lifter, "fp16"), xa))
    np.testing.assert_array_equal(b, _stream_all(CausalStream(lifter, "fp16"), xb))


@pytest.mark.parametrize("mode", ["persist", "launches"])
def test_stream_graph_replay_fallback_forms(mode, monkeypatch):
    """test_stream_graph_replay_matches_eager (tests/test_gpu_stream.py) in the two fallback
    forms: `persist` captures a memset and one launch of G steps, `launches` G x layers GEMV
    nodes.  Replays fed from the device frame queue equal the eager steps bit for bit."""
    monkeypatch.setenv("VP3D_STREAM_MODE", mode)
    fw, T = (3, 3, 3), 80
    m, sd = make_model(False, fw, causal=True, channels=256)
    x = torch.from_numpy(synth.normalized_windows(12, "graph", 1, T)[0]).cuda().reshape(T, -1)
    m.cuda()
    eager = CausalStream(m.native_lifter(), "fp16")
    assert eager.mode == mode
    want = torch.stack([eager.step(x[t]).clone().reshape(-1) for t in range(T)])
    eager.check()
    for G in (1, 8):
        g = CausalStream(m.native_lifter(), "fp16")
        assert g.mode == mode
        Q = g.queue_len
        assert T % G == 0 and Q % G == 0
        s = torch.cuda.Stream()
        fq, pr = g.io_tensors()
        if mode == "persist":
            with pytest.raises(RuntimeError, match="at most queue_len steps"):
                g.capture(s, steps=Q + 1)
        g.capture(s, steps=G)
        got = []
        with torch.cuda.stream(s):
            for t0 in range(0, T, G):
                for t in range(t0, t0 + G):
                    fq[t % Q].copy_(x[t])
                g.replay(s)
                for t in range(t0, t0 + G):
                    got.append(pr[t % Q].clone())
        torch.cuda.synchronize()
        g.check()
        assert torch.equal(torch.stack(got), want), G
        assert g.frames_seen() == T
