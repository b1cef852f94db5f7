#!/usr/bin/env python3
"""Generate the CoupledLSTM training golden by running the REFERENCE itself (read-only import,
as make_golden_stacked.py does; MANIFEST.json is not touched -- the fixture's `meta` carries
the torch version and a sha256 over its arrays).

  train_lstm_h64.npz, train_lstm_h64_s1.npz
                       two reference training iterations (run.py:451-487 with CoupledLSTM,
                       common/models/CamLSTM.py:47-129, in train mode, dropout 0): forward with
                       BatchNorm batch statistics, mpjpe, backward, optim.Adam(amsgrad=True).step()
                       (run.py:662).  hidden 64, 2 cells, head [32, 24], B = 6, T = 9.  Keys as
                       train_*.npz: w/<key>, s{it}/x2d, s{it}/xcam, s{it}/target, s{it}/y,
                       s{it}/loss, s{it}/grad/<key>, s{it}/after/<key>.  The second
                       file holds the s1/ keys (a committed file stays under 1 MiB).

    VP3D_REFERENCE=/path/to/reference python tests/golden/make_golden_lstm_train.py
"""
import hashlib
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
PKG = os.path.join(REPO, "dynamic-camera-augmented-videopose3d_amd")
REF = os.environ.get("VP3D_REFERENCE", "/root/reference")

# `common` must resolve to the reference; vp3d_amd.synth is loaded by file path
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from common import loss as ref_loss  # noqa: E402
from common.models import CamLSTM as ref_lstm  # noqa: E402

_spec = importlib.util.spec_from_file_location("vp3d_synth", os.path.join(PKG, "vp3d_amd", "synth.py"))
synth = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(synth)
_spec = importlib.util.spec_from_file_location("lstm_train_state", os.path.join(REPO, "tests", "lstm_train_state.py"))
_state = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_state)

assert os.path.realpath(ref_lstm.__file__).startswith(os.path.realpath(REF)), ref_lstm.__file__

torch.set_num_threads(8)

NAME = "train_lstm_h64"
HIDDEN, CELLS, HEAD, B, T, STEPS, LR, SEED = 64, 2, [32, 24], 6, 9, 2, 1e-3, 0


def draw_state(keys, hidden, seed):
    """tests/lstm_train_state.py draw_state (the tests' own), loaded by file path."""
    return _state.draw_state(synth, keys, hidden, seed)


def content_sha256(arrays):
    h = hashlib.sha256()
    for k in sorted(arrays):
        v = np.ascontiguousarray(arrays[k])
        h.update(k.encode() + b"\0" + str(v.dtype).encode() + b"\0" + str(v.shape).encode() + b"\0" + v.tobytes())
    return h.hexdigest()


def main():
    m = ref_lstm.CoupledLSTM(17, 2, 17, 3, hidden_size=HIDDEN, num_cells=CELLS, head_layers=HEAD, dropout=0.0)
    keys = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sd = draw_state(keys, HIDDEN, SEED)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    m.train()
    m.set_bn_momentum(0.1)
    opt = torch.optim.Adam(m.parameters(), lr=LR, amsgrad=True)
    arrays = {"w/" + k: v for k, v in sd.items()}
    for it in range(STEPS):
        x2 = synth.normalized_windows(SEED + 10 + it, NAME, B, T)
        xc = synth.normal(SEED + 30 + it, NAME + "/cam", (B, T, 3, 4), std=0.5).astype(np.float32)
        y = m(torch.from_numpy(x2), torch.from_numpy(xc))
        tgt = synth.normal(SEED + 20 + it, NAME + "/target", tuple(y.shape), std=0.2).astype(np.float32)
        loss = ref_loss.mpjpe(y, torch.from_numpy(tgt))
        opt.zero_grad()
        loss.backward()
        arrays[f"s{it}/x2d"] = x2
        arrays[f"s{it}/xcam"] = xc
        arrays[f"s{it}/target"] = tgt
        arrays[f"s{it}/y"] = y.detach().numpy()
        arrays[f"s{it}/loss"] = np.array(loss.item(), dtype=np.float32)
        for k, p in m.named_parameters():
            arrays[f"s{it}/grad/{k}"] = p.grad.numpy().copy()
        opt.step()
        for k, v in m.state_dict().items():
            arrays[f"s{it}/after/{k}"] = v.numpy().copy()
    meta = dict(hidden=HIDDEN, cells=CELLS, head=HEAD, B=B, T=T, steps=STEPS, lr=LR, amsgrad=True, momentum=0.1,
                dropout=0.0, seed=SEED, keys=list(keys), torch=torch.__version__, numpy=np.__version__,
                sha256=content_sha256(arrays))
    # two files: the project takes no new committed file above 1 MiB (the larger fixtures here are
    # older than that rule), and the arrays come to 1.28 MB.  The weights and step 0, then step 1 (tests/lstm_train_cases.py load_golden reads both)
    first = {k: v for k, v in arrays.items() if not k.startswith("s1/")}
    second = {k: v for k, v in arrays.items() if k.startswith("s1/")}
    for name, part in ((NAME, first), (NAME + "_s1", second)):
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, meta=np.array(json.dumps(meta)), **part)
        print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
