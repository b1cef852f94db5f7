"""The seeded CoupledLSTM state of the training tests and of their golden (not collected: no
test_ prefix).  Free of imports from the package, so that tests/golden/make_golden_lstm_train.py,
in whose process `common` is the reference's, can load it by file path with its own copy of
vp3d_amd.synth: one definition, so the golden stays regenerable."""
import math

import numpy as np


def draw_state(synth, keys, hidden, seed):
    """state_dict (numpy) for the given {key: shape}: matrices U(+-1/sqrt(fan_in)) (the LSTM's:
    1/sqrt(hidden)), BatchNorm gamma U(0.5, 1.5), beta U(+-0.1), running mean U(+-0.2), var
    U(0.5, 2), every other bias N(0, 0.1) -- tests/seq_cases.py without the x3 LSTM scale."""
    sd = {}
    for k, shape in keys.items():
        if k.endswith("num_batches_tracked"):
            continue

        def u(lo, hi):
            return synth.uniform(seed, k, shape, lo, hi).astype(np.float32)
        bn = k.rsplit(".", 1)[0] + ".running_mean" in keys
        if len(shape) == 2:
            b = 1.0 / math.sqrt(hidden if k.startswith("lstm_layers.") else shape[1])
            sd[k] = u(-b, b)
        elif k.endswith("running_mean"):
            sd[k] = u(-0.2, 0.2)
        elif k.endswith("running_var"):
            sd[k] = u(0.5, 2.0)
        elif bn and k.endswith(".weight"):
            sd[k] = u(0.5, 1.5)
        elif bn:
            sd[k] = u(-0.1, 0.1)
        else:
            assert "bias" in k, k
            sd[k] = synth.normal(seed, k, shape, std=0.1).astype(np.float32)
    return sd
