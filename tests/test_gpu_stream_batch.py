"""Batched causal streaming (vp3d_amd.stream.CausalStreamBatch, csrc/stream_batch.hip): many
streams of one lifter advance in one step, each at its own position, against the float64 oracle
of oracle/stream_ref.py on exactly the frames each slot consumed.

Gate (stream_cases.TOL_COORD, TOL_DMPJPE): 2e-5 m per coordinate and |dMPJPE| <= 1e-7 m, the
project's stream gates, for fp32, fp16 and bf16 weights.  The batched step keeps f32 activations
and rounds only the weights (exact f32 MFMA, 16-bit weights widened in registers), so the oracle
is evaluated on the same rounded weights and what is left is the order of the f32 sums: the
float32 oracle lies within 1e-6 m of the float64 one on these inputs while any two sequences of
one batch lie 4e-4 m or more apart (tests/test_stream_batch_cases.py).

Beyond the gate, bit-for-bit: the order of an output's sum depends neither on the number of slots
nor on the slot, so a sequence gives the same poses in any slot of any batch size, behind other
slots' positions, and through a replayed graph.
"""
import numpy as np
import pytest
import torch

import stream_batch_cases as bc
import stream_cases as sc
from helpers import make_model
from oracle.stream_ref import round_weights, stream_reference
from vp3d_amd import synth
from vp3d_amd.stream import CausalStream, CausalStreamBatch

pytestmark = pytest.mark.gpu

LAG = 5  # steps slot 2 of the case-table test stays inactive


def _gate(label, out, ref):
    assert out.shape == ref.shape, (label, out.shape, ref.shape)
    err = float(np.abs(out - ref).max())
    dm = sc.dmpjpe(out, ref)
    print(f"stream_batch {label}: max|d|={err:.3e} m, dMPJPE={dm * 1e3:.3e} mm")
    assert err <= sc.TOL_COORD, (label, err)
    assert dm <= sc.TOL_DMPJPE, (label, dm)


def _run_all(bt, frames, active=None):
    """Step `bt` through frames (T, S, J_in, 2) [with masks active (T, S)]: poses (T, S, J_out, 3)."""
    T = frames.shape[0]
    out = torch.empty((T, bt.n_streams, bt.n_out // 3, 3), dtype=torch.float32, device=frames.device)
    for g in range(T):
        bt.step(frames[g], None if active is None else active[g], out=out[g])
    return out.cpu().numpy()


# ---- (a) every shape of the case table ----
@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_batch_case_table(name, dtype):
    """S = 3 (a partial 16-row tile): slot 0 carries the case's sequence B, slot 1 its sequence
    A, slot 2 B again but inactive for the first LAG steps, so its position lags the others."""
    c = sc.case(name)
    m, _ = sc.case_model(name)
    T = c.T
    xb = torch.tensor(sc.case_input(name)[0]).cuda()
    xa = torch.tensor(sc.case_input(name, "A", T)[0]).cuda()
    late = torch.cat([torch.full_like(xb[:LAG], float("nan")), xb[:T - LAG]])  # never consumed: NaN
    frames = torch.stack([xb, xa, late], dim=1).contiguous()
    active = torch.ones((T, 3), dtype=torch.int32, device="cuda")
    active[:LAG, 2] = 0
    bt = CausalStreamBatch(m.cuda().native_lifter(), 3, dtype)
    out = _run_all(bt, frames, active)
    np.testing.assert_array_equal(bt.frames_seen(), [T, T, T - LAG])
    bt.close()
    _gate(f"{name} {dtype} slot 0 (B)", out[:, 0], sc.oracle_poses(name, dtype))
    _gate(f"{name} {dtype} slot 1 (A)", out[:, 1], sc.oracle_poses(name, dtype, "A", T))
    _gate(f"{name} {dtype} slot 2 (B late)", out[LAG:, 2], sc.oracle_poses(name, dtype)[:T - LAG])
    np.testing.assert_array_equal(out[LAG:, 2], out[:T - LAG, 0])
    assert (out[:LAG, 2] == 0.0).all()  # no pose row before the slot's first frame


# ---- (b) K chunking and tile boundaries at the real width ----
@pytest.mark.parametrize("dtype", bc.WIDE_DTYPES)
@pytest.mark.parametrize("jin", bc.WIDE_JIN)
def test_batch_wide_any_slot_any_batch_size(jin, dtype):
    """(3, 3, 3) at 1024 channels: K = 3072 in the k-convs.  S = 1, 16 (a full tile), 17 (a
    second tile of one row) and 64 (four tiles); every slot meets the gate and the marked
    sequence gives the same bits at slot 0 of 1, slot 0 of 16, slot 16 of 17 and slot 63 of 64."""
    m, _ = bc.wide_model(jin)
    lifter = m.cuda().native_lifter()
    x = torch.tensor(bc.wide_inputs(jin)).cuda()
    ref = bc.wide_oracle(jin, dtype)
    marked = {}
    for S in bc.WIDE_S:
        rows = bc.wide_rows(S)
        bt = CausalStreamBatch(lifter, S, dtype)
        out = _run_all(bt, x[rows].transpose(0, 1).contiguous())
        np.testing.assert_array_equal(bt.frames_seen(), [bc.WIDE_T] * S)
        bt.close()
        for s, r in enumerate(rows):
            if s in (0, 1, 15, 16, 31, 32, 47, 48, 63, bc.MARK_AT[S]):
                _gate(f"wide{jin} {dtype} S={S} slot {s}", out[:, s], ref[r])
        err = float(np.abs(out.transpose(1, 0, 2, 3) - ref[rows]).max())
        print(f"stream_batch wide{jin} {dtype} S={S}: max|d| over every slot {err:.3e} m")
        assert err <= sc.TOL_COORD
        marked[S] = out[:, bc.MARK_AT[S]]
    for S in bc.WIDE_S[1:]:
        np.testing.assert_array_equal(marked[S], marked[1])


# ---- (c) refusals and errors ----
def test_batch_refusals():
    m, _ = sc.case_model("one_width")
    lifter = m.cuda().native_lifter()
    for n in (0, 65):
        with pytest.raises(RuntimeError, match="n_streams"):
            CausalStreamBatch(lifter, n, "fp16")
    with pytest.raises(RuntimeError, match="dtype"):
        CausalStreamBatch(lifter, 2, "f16x3")
    nc, _ = make_model(False, (3, 3), causal=False, channels=64)
    with pytest.raises(RuntimeError):
        CausalStreamBatch(nc.cuda().native_lifter(), 2, "fp16")
    wide, _ = make_model(False, sc.REFUSED["fw"], causal=True, channels=sc.REFUSED["channels"])
    wide.cuda()
    for dtype in sc.DTYPES:
        with pytest.raises(RuntimeError, match=sc.REFUSED["match"]):
            CausalStreamBatch(wide.native_lifter(), 2, dtype)
    bt = CausalStreamBatch(lifter, 2, "fp16")
    good = torch.zeros((2, 17, 2), device="cuda")
    with pytest.raises(RuntimeError, match="device"):
        bt.step(good.cpu())
    with pytest.raises(RuntimeError, match="device"):
        bt.step(good, torch.ones(2, dtype=torch.int32))
    for bad in (torch.zeros((3, 17, 2), device="cuda"), torch.zeros((2, 34), device="cuda"),
                torch.zeros((2, 16, 2), device="cuda")):
        with pytest.raises(RuntimeError, match="frames must be"):
            bt.step(bad)
    with pytest.raises(RuntimeError, match="active must be"):
        bt.step(good, torch.ones(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError):
        bt.reset(2)
    bt.step(good, torch.tensor([True, False], device="cuda"))
    np.testing.assert_array_equal(bt.frames_seen(), [1, 0])
    bt.close()
    with pytest.raises(RuntimeError):
        bt.step(good)
    bt.close()  # idempotent


# ---- (d), (e) tracks that come and go ----
def _track_frames(name):
    """(frames (G, S, J_in, 2) with NaN wherever a slot consumes nothing, active (G, S)) on the device."""
    act, seg, idx = bc.track_plan()
    c = sc.case(name)
    fr = np.full((bc.TRACK_STEPS, bc.TRACK_S, c.jin, 2), np.nan, np.float32)
    for g in range(bc.TRACK_STEPS):
        for s in range(bc.TRACK_S):
            if act[g, s]:
                fr[g, s] = bc.track_sequence(name, s, int(seg[g, s]))[idx[g, s]]
    return torch.tensor(fr).cuda(), torch.tensor(act).cuda()


def _run_tracks(bt, frames, active, graph_stream=None):
    """The schedule of stream_batch_cases through eager steps or, with graph_stream, through
    replays of one captured step fed from io_tensors(): (poses (G, S, J_out, 3), positions (G, S))."""
    G = bc.TRACK_STEPS
    poses = torch.empty((G, bc.TRACK_S, bt.n_out // 3, 3), dtype=torch.float32, device="cuda")
    seen = np.zeros((G, bc.TRACK_S), np.int64)
    if graph_stream is not None:
        fin, ain, pout = bt.io_tensors()
        assert ain.dtype == torch.int32 and fin.shape == (bc.TRACK_S, bt.n_in) and pout.shape == (bc.TRACK_S, bt.n_out)
        bt.capture(graph_stream)
    for g in range(G):
        if graph_stream is None:
            if g == bc.TRACK_RESET_STEP:
                for s in bc.TRACK_RESET_SLOTS:
                    bt.reset(s)
            bt.step(frames[g], active[g], out=poses[g])
        else:
            with torch.cuda.stream(graph_stream):
                if g == bc.TRACK_RESET_STEP:
                    for s in bc.TRACK_RESET_SLOTS:
                        bt.reset(s)
                fin.copy_(frames[g].reshape(bc.TRACK_S, -1))
                ain.copy_(active[g])
                bt.replay(graph_stream)
                poses[g].copy_(pout.view(bc.TRACK_S, -1, 3))
        seen[g] = bt.frames_seen()
    torch.cuda.synchronize()
    return poses.cpu().numpy(), seen


@pytest.mark.parametrize("dtype", bc.TRACK_DTYPES)
@pytest.mark.parametrize("name", bc.TRACK_CASES)
def test_batch_tracks_come_and_go(name, dtype):
    """S = 5 over 90 global steps: slot s inactive before step 4 s and whenever (g + s) % 7 == 3,
    slots 1 and 3 reset at step 50 onto another sequence.  Each slot's poses meet the gate
    against the oracle on exactly the frames it consumed (the frames offered while it is
    inactive are NaN); on inactive steps its pose row and position do not change; and the
    poses equal, bit for bit, the same frames streamed without gaps through a batch of one."""
    act, seg, idx = bc.track_plan()
    m, _ = sc.case_model(name)
    lifter = m.cuda().native_lifter()
    frames, active = _track_frames(name)
    bt = CausalStreamBatch(lifter, bc.TRACK_S, dtype)
    poses, seen = _run_tracks(bt, frames, active)
    bt.close()
    assert np.isfinite(poses).all()
    for s in range(bc.TRACK_S):
        for g in range(bc.TRACK_STEPS):
            if act[g, s]:
                assert seen[g, s] == idx[g, s] + 1, (g, s)
            else:
                reset_now = g == bc.TRACK_RESET_STEP and s in bc.TRACK_RESET_SLOTS
                assert seen[g, s] == (0 if g == 0 or reset_now else seen[g - 1, s]), (g, s)
                np.testing.assert_array_equal(poses[g, s], poses[g - 1, s] if g else np.zeros_like(poses[g, s]))
    one = CausalStreamBatch(lifter, 1, dtype)
    for s, k, n in bc.track_segments():
        got = poses[(seg[:, s] == k) & (act[:, s] == 1), s]
        _gate(f"tracks {name} {dtype} slot {s} segment {k} ({n} frames)", got, bc.track_oracle(name, dtype, s, k))
        one.reset()
        x = torch.tensor(bc.track_sequence(name, s, k)[:n]).cuda()
        np.testing.assert_array_equal(got, _run_all(one, x[:, None])[:, 0])
    one.close()


@pytest.mark.parametrize("name,dtype", [("jin21", "fp16"), ("expand5", "fp32")])
def test_batch_graph_replay_matches_eager(name, dtype):
    """One captured step replayed 90 times, frames and mask written into io_tensors() between
    replays (the schedule of the tracks test, resets included): the poses equal the eager
    steps bit for bit and the positions agree."""
    m, _ = sc.case_model(name)
    lifter = m.cuda().native_lifter()
    frames, active = _track_frames(name)
    eager = CausalStreamBatch(lifter, bc.TRACK_S, dtype)
    want, want_seen = _run_tracks(eager, frames, active)
    eager.close()
    g = CausalStreamBatch(lifter, bc.TRACK_S, dtype)
    with pytest.raises(RuntimeError, match="no captured graph"):
        g.replay(torch.cuda.Stream())
    got, got_seen = _run_tracks(g, frames, active, graph_stream=torch.cuda.Stream())
    g.close()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_seen, want_seen)


# ---- (f) isolation ----
def test_batches_and_a_stream_do_not_share_state():
    """Two batches and one CausalStream of ONE lifter stepped alternately: rings, positions and
    scratch rows are per object, so each equals itself stepped alone, bit for bit."""
    name, dtype, T = "jin21", "fp16", 60
    m, _ = sc.case_model(name)
    lifter = m.cuda().native_lifter()
    xb = torch.tensor(sc.case_input(name)[0][:T]).cuda()
    xa = torch.tensor(sc.case_input(name, "A", T)[0]).cuda()
    f1 = torch.stack([xb, xa, 0.5 * xa], dim=1).contiguous()
    f2 = torch.stack([xa, 2.0 * xb], dim=1).contiguous()

    def make():
        return CausalStreamBatch(lifter, 3, dtype), CausalStreamBatch(lifter, 2, dtype), CausalStream(lifter, dtype)

    b1, b2, st = make()
    o1, o2, o3 = [], [], []
    for t in range(T):
        o1.append(b1.step(f1[t]).clone())
        o3.append(st.step(xb[t]).clone())
        o2.append(b2.step(f2[t]).clone())
    st.check()
    o1, o2, o3 = (torch.stack(o).cpu().numpy() for o in (o1, o2, o3))
    for o in (b1, b2, st):
        o.close()
    b1, b2, st = make()
    np.testing.assert_array_equal(o1, _run_all(b1, f1))
    np.testing.assert_array_equal(o2, _run_all(b2, f2))
    np.testing.assert_array_equal(o3, torch.stack([st.step(xb[t]).clone() for t in range(T)]).cpu().numpy())
    _gate(f"isolation {name} batch 1 slot 0", o1[:, 0], sc.oracle_poses(name, dtype)[:T])
    _gate(f"isolation {name} batch 2 slot 0", o2[:, 0], sc.oracle_poses(name, dtype, "A", T))
    for o in (b1, b2, st):
        o.close()


# ---- (g) weight reload ----
@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_batch_after_weight_reload_uses_new_weights(dtype):
    """The batch shares the handle's device weights: after the module's parameters change,
    native_lifter() re-uploads them in place (vp3d_load_weights), and the next steps of the
    reset batch meet the gate for the NEW weights (every layer's, in the batch's dtype)."""
    fw, T = (3, 3, 3), 40
    m, _ = make_model(False, fw, causal=True, channels=256, seed=5)
    _, sd2 = make_model(False, fw, causal=True, channels=256, seed=6)
    x = np.stack([synth.normalized_windows(40 + s, "batch_reload", 1, T)[0] for s in range(2)], axis=1)
    xs = torch.tensor(x).cuda()
    m.cuda()
    bt = CausalStreamBatch(m.native_lifter(), 2, dtype)
    old = _run_all(bt, xs[:10])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd2.items()})
    assert m.native_lifter() is bt.lifter  # the same handle, weights re-uploaded in place
    bt.reset()
    new = _run_all(bt, xs)
    bt.close()
    assert np.abs(new[:10] - old).max() > 4e-4
    rs = {k: torch.tensor(v) for k, v in round_weights(sd2, dtype).items()}
    for s in range(2):
        _gate(f"reload {dtype} slot {s}", new[:, s], stream_reference(rs, x[None, :, s], fw))
