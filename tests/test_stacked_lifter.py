"""The StackedPoseLifter ensemble without a device (reference common/models/StackedPoseLifter.py,
run.py:241-288, :714-729, :939-940, :985-987): the drop-in module's parameters, the C-ABI's
configuration checks, the in-test restatement of the MLP against the reference's outputs
(tests/golden/stacked_mlp.npz), the evaluation plumbing driven by oracle callables against
tests/golden/run_eval_stacked.npz, and run.py's refusals.
"""
import ctypes

import numpy as np
import pytest
import torch

import stacked_common as SC


def _cases():
    return SC.mlp_golden()[0]


@pytest.mark.parametrize("i", range(5))
def test_dropin_module_matches_reference_state_dict(i):
    from common.models.StackedPoseLifter import StackedPoseLifter
    c = _cases()[i]
    m = StackedPoseLifter(c["J"], c["F"], c["num_layers"], c["layer_size"])
    sd = m.state_dict()
    assert list(sd.keys()) == c["keys"]
    assert [list(v.shape) for v in sd.values()] == c["shapes"]
    assert sum(p.numel() for p in m.parameters()) == c["param_count"]
    assert (m.num_joints, m.features, m.num_layers, m.layer_size) == (c["J"], c["F"], c["num_layers"],
                                                                      c["layer_size"])
    assert isinstance(m.mlp_layers, torch.nn.ModuleList) and isinstance(m.dropout, torch.nn.Dropout)
    # the seeded weights the goldens were made with fit it
    m.load_state_dict({k: torch.from_numpy(v) for k, v in
                       SC.case_weights(c["J"], c["F"], c["num_layers"], c["layer_size"]).items()})


def _cfg(J=17, F=3, L=3, H=256):
    from vp3d_amd import _native as N
    cfg = N.vp3d_stacked_cfg()
    cfg.num_joints, cfg.features, cfg.num_layers, cfg.layer_size = J, F, L, H
    return cfg


def test_weight_count():
    from vp3d_amd import _native as N
    lib = N.load()
    assert lib.vp3d_stacked_weight_count(ctypes.byref(_cfg())) == 10
    assert lib.vp3d_stacked_weight_count(ctypes.byref(_cfg(L=0))) == 4
    assert lib.vp3d_stacked_weight_count(ctypes.byref(_cfg(L=8, H=512))) == 20
    assert lib.vp3d_stacked_weight_count(ctypes.byref(_cfg(H=0))) == -1
    assert lib.vp3d_stacked_weight_count(ctypes.byref(_cfg(H=513))) == -1
    assert lib.vp3d_stacked_weight_count(ctypes.byref(_cfg(L=9))) == -1
    assert lib.vp3d_stacked_weight_count(ctypes.byref(_cfg(L=-1))) == -1
    assert lib.vp3d_stacked_weight_count(ctypes.byref(_cfg(J=0))) == -1
    assert lib.vp3d_abi_version() == 1


@pytest.mark.parametrize("kw,msg", [(dict(H=513), b"layer_size"), (dict(H=0), b"layer_size"),
                                    (dict(L=9), b"num_layers"), (dict(J=400), b"num_joints * features")])
def test_invalid_config_rejected_without_device(kw, msg):
    from vp3d_amd import _native as N
    lib = N.load()
    h = ctypes.c_void_p()
    rc = lib.vp3d_stacked_create(ctypes.byref(_cfg(**kw)), None, 0, ctypes.byref(h))
    assert rc == N.VP3D_ERR_ASSERT and not h
    assert msg in lib.vp3d_last_error()
    with pytest.raises(AssertionError):
        N.check(rc)


def test_null_arguments():
    from vp3d_amd import _native as N
    lib = N.load()
    assert lib.vp3d_stacked_forward(None, None, None, 1, None, None) == N.VP3D_ERR_ARG
    assert lib.vp3d_stacked_destroy(None) == N.VP3D_OK
    assert lib.vp3d_stacked_create(ctypes.byref(_cfg()), None, 0, None) == N.VP3D_ERR_ARG
    h = ctypes.c_void_p()
    assert lib.vp3d_stacked_create(ctypes.byref(_cfg()), None, 10, ctypes.byref(h)) == N.VP3D_ERR_ARG


@pytest.mark.parametrize("i", range(5))
def test_restated_mlp_reproduces_reference(i):
    """The restatement every other test measures against is the reference's network: f32 within
    1e-6 of `y` (bit-identical on the torch build the golden was made with, the rule of
    test_oracle_golden.py), and in float64 within 1e-12 of `y64`."""
    cases, y, y64, meta = SC.mlp_golden()
    c = cases[i]
    sd = SC.case_weights(c["J"], c["F"], c["num_layers"], c["layer_size"])
    a, b = SC.case_inputs(c["J"], c["F"], c["N"])
    torch.set_num_threads(8)
    with torch.no_grad():
        got = SC.mlp_restated(sd, torch.from_numpy(a), torch.from_numpy(b)).numpy().reshape(y[i].shape)
        got64 = SC.mlp_restated(sd, torch.from_numpy(a).double(), torch.from_numpy(b).double()).numpy()
    np.testing.assert_allclose(got, y[i], rtol=0, atol=1e-6)
    if torch.__version__ == meta["torch"]:
        assert np.array_equal(got, y[i])
    np.testing.assert_allclose(got64.reshape(y64[i].shape), y64[i], rtol=0, atol=1e-12)
    assert abs(np.abs(y[i] - y64[i]).max() - c["err_f32_vs_f64"]) < 1e-12


def test_ensemble_single_frame_sequence():
    """Quirk 3: a one-frame sequence goes through (the reference's .squeeze() would drop its
    frame axis)."""
    from vp3d_amd.stacked import StackedEnsemble
    sd = SC.case_weights(17, 3, 0, 64)
    ens = StackedEnsemble(lambda x2, xc, w: torch.ones(1, x2.shape[1] - w + 1, 17, 3),
                          lambda x2: torch.zeros(1, x2.shape[1] - 242, 17, 3),
                          lambda t, f: SC.mlp_restated(sd, t, f))
    y_t, y_f, y = ens.predict(torch.zeros(1, 243, 17, 2), torch.zeros(1, 243, 3, 4), 243)
    assert y.shape == (1, 1, 17, 3) and y_t.shape == y_f.shape == y.shape
    want = SC.mlp_restated(sd, torch.ones(1, 51), torch.zeros(1, 51))
    assert torch.equal(y.reshape(1, 51), want)


def test_run_eval_stacked_plumbing_cpu_oracle():
    import run
    from common.arguments import parse_args
    from oracle import camera_ref, generators_ref
    from oracle.seq_lifter_ref import sliding_windows, transformer_forward
    from oracle.temporal_ref import lifter_forward
    from test_run_eval import OracleMetrics
    from vp3d_amd import synth
    from vp3d_amd.stacked import StackedEnsemble

    torch.set_num_threads(8)
    gold = SC.run_eval_golden()
    meta = gold["meta"]
    args = parse_args(SC.run_argv(meta) + ["--evaluate", "synthetic"])
    data = run.synthetic_dataset(args, normalize=camera_ref.normalize_screen_coordinates)
    from common.models.TemporalModel import TemporalModel
    fcn_sd = synth.lifter_state_dict(
        [(k, tuple(v.shape)) for k, v in TemporalModel(17, 2, 17, meta["fw"], channels=meta["channels"])
         .state_dict().items()], seed=meta["seed"])
    tstate = SC.transformer_state()

    def transformer(x2d, xcam, window):
        w2, wc = sliding_windows(x2d, xcam, window)
        return transformer_forward(tstate, w2, wc, 4, 2, 3).reshape(1, -1, 17, 3)

    ens = StackedEnsemble(transformer, lambda x: lifter_forward(fcn_sd, x, meta["fw"]),
                          lambda t, f: SC.mlp_restated(gold["mlp"], t, f))

    class Gen:
        seq_length = 243

        def __init__(self, cams, p3d, p2d):
            self.args = (cams, p3d, p2d)

        def next_epoch(self):
            cams = self.args[0]
            for cam, (bc, b3, b2) in zip(cams, generators_ref.unchunked_sequences(*self.args, 121, 0)):
                info = {k: cam[k] for k in cam if k.startswith("cam_")}
                yield (torch.from_numpy(bc.astype(np.float32)), torch.from_numpy(b3.astype(np.float32)),
                       torch.from_numpy(b2.astype(np.float32)), info)

    res = run.run_evaluation(data, run.group_actions(data, list(data)), Gen, ens, OracleMetrics())
    assert set(res) >= {"per_action", "summary", "pmcc", "ensemble_diffs"}
    SC.check_run_result(res, gold)


def test_run_stacked_refusals():
    """Training, --trajectory and an FCN of another receptive field are refused with a message;
    a runnable command line without a device ends in the existing 'evaluates on the MI355X' exit."""
    import run
    base = ["--use-model", "StackedPoselifter"]
    with pytest.raises(SystemExit, match="training"):
        run.main(base)
    with pytest.raises(SystemExit, match="--trajectory"):
        run.main(base + ["--evaluate", "synthetic", "--trajectory"])
    with pytest.raises(SystemExit, match="receptive field of 243"):
        run.main(base + ["--evaluate", "synthetic", "--fcn-architecture", "3,3,3"])
    with pytest.raises(SystemExit, match="--transformer-weights and --fcn-weights"):
        run.main(base + ["--evaluate", "stacked.bin"])
    with pytest.raises(SystemExit, match="--fcn-weights"):
        run.main(base + ["--evaluate", "stacked.bin", "--transformer-weights", "t.bin"])
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit, match="evaluates on the MI355X"):
            run.main(base + ["--evaluate", "synthetic"])
