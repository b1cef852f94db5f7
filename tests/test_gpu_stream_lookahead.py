"""Look-ahead streaming of NON-causal lifters (vp3d_amd.stream.LookaheadStreamBatch, vp3d_lstream,
the look-ahead form of csrc/stream_batch.hip) against the float64 non-causal oracle on exactly
the frames each slot consumed, edge-padded by P on each side (tests/lookahead_cases.py).

Gate (stream_cases.TOL_COORD, TOL_DMPJPE): 2e-5 m per coordinate and |dMPJPE| <= 1e-7 m, the
project's stream gates, for fp32, fp16 and bf16 weights.  The step keeps f32 activations and
rounds only the weights, so the oracle is evaluated on the same rounded weights; the float32
oracle lies within 1e-6 m of the float64 one on these inputs while two sequences of one batch
lie 4e-4 m or more apart (tests/test_stream_lookahead.py).

Beyond the gate: which frame a pose row belongs to (pose_frame) is exact, no-op steps change
nothing, and a sequence gives the same bits in any slot of any batch size, behind other slots'
positions, through a replayed graph and through lift_sequences.
"""
import ctypes

import numpy as np
import pytest
import torch

import lookahead_cases as lc
import stream_batch_cases as bc
import stream_cases as sc
from helpers import make_model
from vp3d_amd import _native as N
from vp3d_amd.stream import CausalStreamBatch, LookaheadStreamBatch, lift_sequences

pytestmark = pytest.mark.gpu

LAG = 5  # steps slot 2 of the case-table test stays idle
I, C, D = lc.IDLE, lc.CONSUME, lc.DRAIN


def _gate(label, out, ref):
    assert out.shape == ref.shape, (label, out.shape, ref.shape)
    err = float(np.abs(out - ref).max())
    dm = sc.dmpjpe(out, ref)
    print(f"stream_lookahead {label}: max|d|={err:.3e} m, dMPJPE={dm * 1e3:.3e} mm")
    assert err <= sc.TOL_COORD, (label, err)
    assert dm <= sc.TOL_DMPJPE, (label, dm)


def _run(bt, frames, codes):
    """Step `bt` through frames (G, S, J_in, 2) with codes (G, S):
    (pose rows (G, S, J_out, 3), pose_frame (G, S)) as numpy."""
    G = codes.shape[0]
    rows = torch.empty((G, bt.n_streams, bt.n_out // 3, 3), dtype=torch.float32, device="cuda")
    pf = torch.empty((G, bt.n_streams), dtype=torch.int32, device="cuda")
    for g in range(G):
        _, k = bt.step(frames[g], codes[g], out=rows[g])
        pf[g] = k
    return rows.cpu().numpy(), pf.cpu().numpy()


def _collect(rows, pf, s, n):
    """Slot s's poses 0..n-1 out of the step rows, each taken where pose_frame names it."""
    out = np.full((n,) + rows.shape[2:], np.nan, np.float32)
    seen = np.zeros(n, int)
    for g in range(rows.shape[0]):
        k = pf[g, s]
        if k >= 0:
            out[k] = rows[g, s]
            seen[k] += 1
    assert (seen == 1).all(), (s, seen)
    return out


def _lift_plan(lengths, P, lead=None):
    """Codes (G, S) of slots that consume lengths[s] frames (after lead[s] idle steps), then drain
    P steps, then idle; and for each step the frame index a slot consumes (-1: none)."""
    S = len(lengths)
    lead = [0] * S if lead is None else lead
    G = max(a + n for a, n in zip(lead, lengths)) + P
    codes = np.zeros((G, S), np.int32)
    idx = np.full((G, S), -1, np.int64)
    for s, (a, n) in enumerate(zip(lead, lengths)):
        codes[a:a + n, s] = C
        idx[a:a + n, s] = np.arange(n)
        codes[a + n:a + n + P, s] = D
    return codes, idx


def _frames(seqs, idx):
    """(G, S, J_in, 2) device frames: NaN wherever a slot consumes nothing."""
    G, S = idx.shape
    fr = np.full((G, S) + seqs[0].shape[1:], np.nan, np.float32)
    for s in range(S):
        on = idx[:, s] >= 0
        fr[on, s] = seqs[s][idx[on, s]]
    return torch.tensor(fr).cuda()


# ---- 4. every shape of the case table ----
@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_lookahead_case_table(name, dtype):
    """S = 3 (a partial 16-row tile): slot 0 carries the case's sequence B, slot 1 its sequence A,
    slot 2 B again but idle (NaN frames) for the first LAG steps; all consume T frames, then
    drain P steps."""
    c = sc.case(name)
    T, P = c.T, lc.case_lookahead(name)
    m, _ = lc.case_model(name)
    xb, xa = sc.case_input(name)[0], sc.case_input(name, "A", T)[0]
    codes, idx = _lift_plan([T, T, T], P, lead=[0, 0, LAG])
    bt = LookaheadStreamBatch(m.cuda().native_lifter(), 3, dtype)
    assert bt.lookahead == P
    rows, pf = _run(bt, _frames([xb, xa, xb], idx), torch.tensor(codes).cuda())
    n, e = bt.counts()
    bt.close()
    np.testing.assert_array_equal(n, [T, T, T])
    np.testing.assert_array_equal(e, [T, T, T])
    trace = [-1] * P + list(range(T))
    for s, lead in enumerate((0, 0, LAG)):
        want = [-1] * lead + trace + [-1] * (LAG - lead)
        np.testing.assert_array_equal(pf[:, s], want)
        assert (rows[:lead + P, s] == 0.0).all()  # no pose row before the slot's first emission
    out = [_collect(rows, pf, s, T) for s in range(3)]
    _gate(f"{name} {dtype} slot 0 (B)", out[0], lc.case_oracle(name, dtype))
    _gate(f"{name} {dtype} slot 1 (A)", out[1], lc.case_oracle(name, dtype, "A", T))
    _gate(f"{name} {dtype} slot 2 (B late)", out[2], lc.case_oracle(name, dtype))
    np.testing.assert_array_equal(out[2], out[0])


# ---- 5. K chunking and tile boundaries at the real width ----
@pytest.mark.parametrize("dtype", bc.WIDE_DTYPES)
@pytest.mark.parametrize("jin", bc.WIDE_JIN)
def test_lookahead_wide_any_slot_any_batch_size(jin, dtype):
    """(3, 3, 3) at 1024 channels, S = 1, 16, 17 and 64: the sampled slots meet the gates, every
    slot max|d|, and the marked sequence gives the same bits at slot 0 of 1, slot 0 of 16,
    slot 16 of 17 and slot 63 of 64."""
    m, _ = lc.wide_model(jin)
    lifter = m.cuda().native_lifter()
    x = bc.wide_inputs(jin)
    ref = lc.wide_oracle(jin, dtype)
    T, P = bc.WIDE_T, lc.lookahead(bc.WIDE_FW)
    marked = {}
    for S in bc.WIDE_S:
        rows_of = bc.wide_rows(S)
        codes, idx = _lift_plan([T] * S, P)
        bt = LookaheadStreamBatch(lifter, S, dtype)
        rows, pf = _run(bt, _frames([x[r] for r in rows_of], idx), torch.tensor(codes).cuda())
        n, e = bt.counts()
        bt.close()
        np.testing.assert_array_equal(n, [T] * S)
        np.testing.assert_array_equal(e, [T] * S)
        np.testing.assert_array_equal(pf, np.repeat(np.array([-1] * P + list(range(T)))[:, None], S, axis=1))
        out = rows[P:]  # every slot emits frame g - P at step g
        for s, r in enumerate(rows_of):
            if s in (0, 1, 15, 16, 31, 32, 47, 48, 63, bc.MARK_AT[S]):
                _gate(f"wide{jin} {dtype} S={S} slot {s}", out[:, s], ref[r])
        err = float(np.abs(out.transpose(1, 0, 2, 3) - ref[rows_of]).max())
        print(f"stream_lookahead wide{jin} {dtype} S={S}: max|d| over every slot {err:.3e} m")
        assert err <= sc.TOL_COORD
        marked[S] = out[:, bc.MARK_AT[S]]
    for S in bc.WIDE_S[1:]:
        np.testing.assert_array_equal(marked[S], marked[1])


# ---- 6. the real shape ----
@pytest.mark.parametrize("dtype", lc.REAL_DTYPES)
def test_lookahead_real_shape(dtype):
    """(3, 3, 3, 3, 3) at 1024 channels, S = 2, T = 130 with P = 121: warm-up, nine steady
    emissions and a 121-step drain."""
    m, _ = lc.real_model()
    x = lc.real_inputs()
    T, P = lc.REAL_T, 121
    codes, idx = _lift_plan([T, T], P)
    bt = LookaheadStreamBatch(m.cuda().native_lifter(), 2, dtype)
    assert bt.lookahead == P
    rows, pf = _run(bt, _frames([x[0], x[1]], idx), torch.tensor(codes).cuda())
    n, e = bt.counts()
    bt.close()
    np.testing.assert_array_equal(n, [T, T])
    np.testing.assert_array_equal(e, [T, T])
    ref = lc.real_oracle(dtype)
    for s in range(2):
        _gate(f"real {dtype} slot {s}", _collect(rows, pf, s, T), ref[s])


# ---- 7. sequences shorter than, equal to and longer than the look-ahead ----
@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("name", lc.SHORT_CASES)
def test_lookahead_short_sequences(name, dtype):
    """Slots 0..4 carry lengths 1, 2, P, P + 1 and 2 P + 1, slot 5 is never fed; each drains when
    its sequence ends.  Then five further drain steps are no-ops everywhere."""
    P = lc.case_lookahead(name)
    lengths = list(lc.short_lengths(name))
    seqs = [lc.short_sequence(name, s) for s in range(5)]
    m, _ = lc.case_model(name)
    codes, idx = _lift_plan(lengths + [0], P)
    codes[:, 5] = D  # a never-fed slot: every drain is a no-op
    idx = np.concatenate([idx, np.full((5, 6), -1)])
    codes = np.concatenate([codes, np.full((5, 6), D, np.int32)])
    bt = LookaheadStreamBatch(m.cuda().native_lifter(), 6, dtype)
    rows, pf = _run(bt, _frames(seqs + [seqs[0]], idx), torch.tensor(codes).cuda())
    n, e = bt.counts()
    bt.close()
    np.testing.assert_array_equal(n, lengths + [0])
    np.testing.assert_array_equal(e, lengths + [0])
    for s, T in enumerate(lengths):
        np.testing.assert_array_equal(pf[:, s], [-1] * P + list(range(T)) + [-1] * (len(pf) - P - T))
        _gate(f"short {name} {dtype} slot {s} ({T} frames)", _collect(rows, pf, s, T),
              lc.sequence_oracle(name, dtype, (name, "short", s)))
        for g in range(P + T, len(pf)):  # no-ops: the row keeps the last pose
            np.testing.assert_array_equal(rows[g, s], rows[P + T - 1, s])
    assert (pf[:, 5] == -1).all() and (rows[:, 5] == 0.0).all()


# ---- 8. tracks that come, drain and go ----
def _track_frames(name):
    p = lc.track_plan(name)
    c = sc.case(name)
    fr = np.full((lc.TRACK_STEPS, lc.TRACK_S, c.jin, 2), np.nan, np.float32)
    for g in range(lc.TRACK_STEPS):
        for s in range(lc.TRACK_S):
            if p["idx"][g, s] >= 0:
                fr[g, s] = lc.track_sequence(name, s, int(p["seg"][g, s]))[p["idx"][g, s]]
    return torch.tensor(fr).cuda(), torch.tensor(p["codes"]).cuda()


def _run_tracks(bt, name, frames, codes, graph_stream=None):
    """The schedule of lookahead_cases.track_plan through eager steps or, with graph_stream,
    through replays of one captured step fed from io_tensors():
    (pose rows, pose_frame, consumed, emitted), each over (TRACK_STEPS, TRACK_S)."""
    resets = lc.track_plan(name)["resets"]
    G, S = lc.TRACK_STEPS, lc.TRACK_S
    rows = torch.empty((G, S, bt.n_out // 3, 3), dtype=torch.float32, device="cuda")
    pf = torch.empty((G, S), dtype=torch.int32, device="cuda")
    cons, emit = np.zeros((G, S), np.int64), np.zeros((G, S), np.int64)
    if graph_stream is not None:
        fin, cin, pout, kout = bt.io_tensors()
        assert cin.dtype == torch.int32 and kout.dtype == torch.int32
        assert fin.shape == (S, bt.n_in) and pout.shape == (S, bt.n_out) and cin.shape == kout.shape == (S,)
        bt.capture(graph_stream)
    for g in range(G):
        if graph_stream is None:
            for s in resets.get(g, ()):
                bt.reset(s)
            _, k = bt.step(frames[g], codes[g], out=rows[g])
            pf[g] = k
        else:
            with torch.cuda.stream(graph_stream):
                for s in resets.get(g, ()):
                    bt.reset(s)
                fin.copy_(frames[g].reshape(S, -1))
                cin.copy_(codes[g])
                bt.replay(graph_stream)
                rows[g].copy_(pout.view(S, -1, 3))
                pf[g].copy_(kout)
        cons[g], emit[g] = bt.counts()
    torch.cuda.synchronize()
    return rows.cpu().numpy(), pf.cpu().numpy(), cons, emit


@pytest.mark.parametrize("dtype", bc.TRACK_DTYPES)
@pytest.mark.parametrize("name", lc.TRACK_CASES)
def test_lookahead_tracks_come_drain_and_go(name, dtype):
    """S = 5 on the (g + s) % 7 != 3 schedule with staggered starts; slots 1 and 3 end their first
    sequence at different steps, drain, ignore a CONSUME sent while drained, are reset and reused
    for another sequence while the others are mid-stream; at the end everybody drains.  pose_frame
    and the counts follow the plan step for step, no-op steps change nothing, and every segment
    meets the gates on exactly the frames it consumed."""
    p = lc.track_plan(name)
    P = lc.case_lookahead(name)
    m, _ = lc.case_model(name)
    frames, codes = _track_frames(name)
    bt = LookaheadStreamBatch(m.cuda().native_lifter(), lc.TRACK_S, dtype)
    rows, pf, cons, emit = _run_tracks(bt, name, frames, codes)
    bt.close()
    assert np.isfinite(rows).all()
    np.testing.assert_array_equal(pf, p["pose_frame"])
    for s in range(lc.TRACK_S):
        n = t = 0
        for g in range(lc.TRACK_STEPS):
            if s in p["resets"].get(g, ()):
                n = t = 0
            if p["takes"][g, s]:
                t += 1
                n += int(p["idx"][g, s] >= 0)
            assert (cons[g, s], emit[g, s]) == (n, max(t - P, 0)), (g, s)
            if pf[g, s] < 0:  # no row written: the previous content stays
                np.testing.assert_array_equal(rows[g, s], rows[g - 1, s] if g else np.zeros_like(rows[g, s]))
    for s, k, n in lc.track_segments(name):
        in_seg = p["seg"][:, s] == k
        got = _collect(rows[in_seg], pf[in_seg], s, n)
        _gate(f"tracks {name} {dtype} slot {s} segment {k} ({n} frames)", got, lc.track_oracle(name, dtype, s, k))


# ---- 9. graph replay ----
@pytest.mark.parametrize("name,dtype", [("jin21", "fp16"), ("dense", "fp32")])
def test_lookahead_graph_replay_matches_eager(name, dtype):
    """One captured step replayed over the tracks schedule (codes 0, 1 and 2, resets included),
    frames and codes written into io_tensors() between replays: pose rows, pose_frame and the
    counts equal the eager steps bit for bit."""
    m, _ = lc.case_model(name)
    lifter = m.cuda().native_lifter()
    frames, codes = _track_frames(name)
    assert set(np.unique(lc.track_plan(name)["codes"])) == {I, C, D}
    eager = LookaheadStreamBatch(lifter, lc.TRACK_S, dtype)
    want = _run_tracks(eager, name, frames, codes)
    eager.close()
    g = LookaheadStreamBatch(lifter, lc.TRACK_S, dtype)
    with pytest.raises(RuntimeError, match="no captured graph"):
        g.replay(torch.cuda.Stream())
    got = _run_tracks(g, name, frames, codes, graph_stream=torch.cuda.Stream())
    g.close()
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


# ---- 10. lift_sequences ----
LIFT_LENGTHS = lc.LIFT_LENGTHS


@pytest.mark.parametrize("dtype", lc.LIFT_DTYPES)
def test_lift_sequences_equals_manual_stepping(dtype):
    """Seven ragged sequences over 3 slots: each meets the gates and equals, bit for bit, the same
    sequence stepped by hand alone in slot 0."""
    name = lc.LIFT_CASE
    c = sc.case(name)
    P = lc.case_lookahead(name)
    m, _ = lc.case_model(name)
    lifter = m.cuda().native_lifter()
    seqs = [lc.lift_sequence(i) for i in range(len(LIFT_LENGTHS))]
    dev = [torch.tensor(x).cuda() for x in seqs]
    bt = LookaheadStreamBatch(lifter, 3, dtype)
    got = bt.lift_sequences(dev)
    n, e = bt.counts()
    assert (n == e).all()
    assert [tuple(y.shape) for y in got] == [(T, c.jout, 3) for T in LIFT_LENGTHS]
    again = lift_sequences(lifter, dev, n_streams=3, dtype=dtype)  # the module-level form, a batch of its own
    for i, T in enumerate(LIFT_LENGTHS):
        y = got[i].cpu().numpy()
        _gate(f"lift {name} {dtype} sequence {i} ({T} frames)", y, lc.sequence_oracle(name, dtype, (name, "lift", i)))
        np.testing.assert_array_equal(again[i].cpu().numpy(), y)
        bt.reset()
        codes, idx = _lift_plan([T, 0, 0], P)
        rows, pf = _run(bt, _frames([seqs[i]] * 3, idx), torch.tensor(codes).cuda())
        np.testing.assert_array_equal(y, _collect(rows, pf, 0, T))
    assert bt.lift_sequences([]) == []
    bt.close()


# ---- 11. refusals and errors ----
def test_lookahead_refusals():
    m, _ = lc.case_model("one_width")
    lifter = m.cuda().native_lifter()
    for n in (0, 65):
        with pytest.raises(RuntimeError, match="n_streams"):
            LookaheadStreamBatch(lifter, n, "fp16")
    with pytest.raises(RuntimeError, match="dtype"):
        LookaheadStreamBatch(lifter, 2, "f16x3")
    causal, _ = sc.case_model("one_width")
    with pytest.raises(RuntimeError, match="look-ahead 0: use vp3d_mstream.*CausalStreamBatch"):
        LookaheadStreamBatch(causal.cuda().native_lifter(), 2, "fp16")
    out = ctypes.c_void_p()  # the C entry itself
    assert N.load().vp3d_lstream_create(causal.native_lifter()._h, N.DTYPES["fp16"], 2, ctypes.byref(out)) == N.VP3D_ERR_ARG
    assert b"look-ahead 0: use vp3d_mstream" in N.load().vp3d_last_error() and out.value is None
    strided, _ = make_model(True, (3, 3), causal=False, channels=64)
    with pytest.raises(RuntimeError, match="strided"):
        LookaheadStreamBatch(strided.cuda().native_lifter(), 2, "fp16")
    wide, _ = make_model(False, sc.REFUSED["fw"], causal=False, channels=sc.REFUSED["channels"])
    wide.cuda()
    for dtype in sc.DTYPES:
        with pytest.raises(RuntimeError, match=sc.REFUSED["match"]):
            LookaheadStreamBatch(wide.native_lifter(), 2, dtype)
    with pytest.raises(RuntimeError):  # unchanged: the causal batch refuses a non-causal lifter
        CausalStreamBatch(lifter, 2, "fp16")
    bt = LookaheadStreamBatch(lifter, 2, "fp16")
    assert bt.lookahead == 1
    good = torch.zeros((2, 17, 2), device="cuda")
    with pytest.raises(RuntimeError, match="device"):
        bt.step(good.cpu())
    with pytest.raises(RuntimeError, match="device"):
        bt.step(good, torch.ones(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="device"):
        bt.lift_sequences([torch.zeros((4, 17, 2))])
    for bad in (torch.zeros((3, 17, 2), device="cuda"), torch.zeros((2, 34), device="cuda"),
                torch.zeros((2, 16, 2), device="cuda")):
        with pytest.raises(RuntimeError, match="frames must be"):
            bt.step(bad)
    with pytest.raises(RuntimeError, match="sequence must be"):
        bt.lift_sequences([torch.zeros((4, 16, 2), device="cuda")])
    with pytest.raises(RuntimeError, match="codes must be"):
        bt.step(good, torch.ones(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="codes must be"):
        bt.step(good, torch.ones(2, dtype=torch.float32, device="cuda"))
    with pytest.raises(RuntimeError):
        bt.reset(2)
    _, k = bt.step(good, torch.tensor([C, 9], device="cuda"))  # any other code is idle
    np.testing.assert_array_equal(k.cpu().numpy(), [-1, -1])
    _, k = bt.step(good)  # codes=None: every slot consumes
    np.testing.assert_array_equal(k.cpu().numpy(), [0, -1])
    n, e = bt.counts()
    np.testing.assert_array_equal(n, [2, 1])
    np.testing.assert_array_equal(e, [1, 0])
    bt.reset(0)
    np.testing.assert_array_equal(bt.counts()[0], [0, 1])
    bt.reset()
    np.testing.assert_array_equal(bt.counts()[0], [0, 0])
    bt.close()
    with pytest.raises(RuntimeError):
        bt.step(good)
    bt.close()  # idempotent
