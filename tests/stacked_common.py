"""Shared by the StackedPoseLifter tests (not collected: no test_ prefix): the seeded weights and
inputs of tests/golden/make_golden_stacked.py regenerated from vp3d_amd.synth, the MLP restated
with torch.nn.functional.linear, and the fixture loaders."""
import functools
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from vp3d_amd import synth

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def case_weights(J, Fe, num_layers, layer_size, seed=0):
    """state_dict (numpy f32) of a StackedPoseLifter: Linear i uniform in +-1/sqrt(fan_in)."""
    D = J * Fe
    dims = [(2 * D, layer_size)] + [(layer_size, layer_size)] * num_layers + [(layer_size, D)]
    sd = {}
    for i, (k, n) in enumerate(dims):
        b = 1.0 / np.sqrt(k)
        sd[f"mlp_layers.{3 * i}.weight"] = synth.uniform(seed, f"spl/{i}/w", (n, k), -b, b).astype(np.float32)
        sd[f"mlp_layers.{3 * i}.bias"] = synth.uniform(seed, f"spl/{i}/b", (n,), -b, b).astype(np.float32)
    return sd


def case_inputs(J, Fe, N):
    a = synth.normal(1, "a", (N, 1, J, Fe), std=0.2)
    b = a + synth.normal(2, "b", (N, 1, J, Fe), std=0.03)
    return a.astype(np.float32), b.astype(np.float32)


def mlp_restated(sd, y_transformer, y_fcn):
    """StackedPoseLifter.forward in eval mode (reference StackedPoseLifter.py:46-56) on torch
    tensors of any float dtype: (n, ...) twice -> (n, J * F)."""
    n = y_transformer.shape[0]
    x = torch.cat((y_transformer.reshape(n, -1), y_fcn.reshape(n, -1)), dim=-1)
    n_lin = len(sd) // 2
    for i in range(n_lin):
        w = torch.as_tensor(sd[f"mlp_layers.{3 * i}.weight"]).to(x.dtype)
        b = torch.as_tensor(sd[f"mlp_layers.{3 * i}.bias"]).to(x.dtype)
        x = F.linear(x, w, b)
        if i + 1 < n_lin:
            x = torch.relu(x)
    return x


@functools.lru_cache(maxsize=None)
def mlp_golden():
    """(cases, {i: y}, {i: y64}, meta) of stacked_mlp.npz; loaded once and shared."""
    g = np.load(os.path.join(GOLD, "stacked_mlp.npz"), allow_pickle=False)
    meta = json.loads(str(g["meta"]))
    n = len(meta["cases"])
    y = {i: g[f"y/{i}"] for i in range(n)}
    y64 = {i: g[f"y64/{i}"] for i in range(n)}
    for v in list(y.values()) + list(y64.values()):
        v.setflags(write=False)
    return meta["cases"], y, y64, meta


@functools.lru_cache(maxsize=None)
def run_eval_golden():
    g = np.load(os.path.join(GOLD, "run_eval_stacked.npz"), allow_pickle=False)
    meta = json.loads(str(g["meta"]))
    actions = [str(a) for a in g["actions"]]
    return {"actions": actions, "errors": dict(zip(actions, g["errors"])), "pmcc": g["pmcc"],
            "fcn_diffs": dict(zip(actions, g["fcn_diffs"])),
            "transformer_diffs": dict(zip(actions, g["transformer_diffs"])),
            "mlp": {k[2:]: g[k] for k in g.files if k.startswith("w/")}, "meta": meta}


def transformer_state():
    g = np.load(os.path.join(GOLD, "run_eval_transformer.npz"), allow_pickle=False)
    return {k[2:]: g[k] for k in g.files if k.startswith("w/")}


def run_argv(meta):
    """The seeded synthetic split and the model sizes of run_eval_stacked.npz."""
    return ["--use-model", meta["model"], "--synthetic-subjects", str(meta["subjects"]),
            "--synthetic-actions", str(meta["actions"]), "--synthetic-frames", str(meta["frames"]),
            "--seed", str(meta["seed"]), "--subjects-test", "*", "-ch", str(meta["channels"]),
            "--fcn-architecture", ",".join(map(str, meta["fw"])),
            "--stacked-num-layers", str(meta["stacked_num_layers"]), "--layer-size", str(meta["layer_size"]),
            "--compute-dtype", "fp32"]


def check_run_result(res, gold):
    """Protocol #1 within 1e-4 mm, the other protocols and the per-sequence diffs (x1000) within
    1e-3 mm, PMCC within 1e-4: the tolerances of test_run_eval_seq.py."""
    for k, v in gold["errors"].items():
        got = np.asarray(res["per_action"][k])
        print(k, got, v)
        assert abs(got[0] - v[0]) <= 1e-4, (k, got[0], v[0])
        np.testing.assert_allclose(got[1:], v[1:], rtol=0, atol=1e-3)
    np.testing.assert_allclose([res["pmcc"][k] for k in res["pmcc"]], gold["pmcc"], atol=1e-4)
    d = res["ensemble_diffs"]
    for k in gold["actions"]:
        np.testing.assert_allclose(np.asarray(d["fcn"][k]) * 1000, gold["fcn_diffs"][k] * 1000, rtol=0, atol=1e-3)
        np.testing.assert_allclose(np.asarray(d["transformer"][k]) * 1000, gold["transformer_diffs"][k] * 1000,
                                   rtol=0, atol=1e-3)
    # the printed values: the mean over the last evaluated action's sequences (run.py:939-940, :985-987)
    last = gold["actions"][-1]
    assert abs(d["printed"]["fcn"] - np.mean(gold["fcn_diffs"][last])) * 1000 <= 1e-3
    assert abs(d["printed"]["transformer"] - np.mean(gold["transformer_diffs"][last])) * 1000 <= 1e-3
