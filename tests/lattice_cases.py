"""The exact-lattice cases shared by tests/test_lattice.py (CPU: the premises and the float64
model) and tests/test_gpu_lattice.py (every dtype and kernel form, bit equality).

A case is a model geometry plus its ORACLE batch: the distinct windows the float64 reference is
computed on.  The GPU test tiles them to the run's batch (strided windows are independent; a
periodic sequence gives periodic poses), so the reference costs the same at B = 5 and B = 2050.
The BN biases of a case's state are calibrated on the oracle batch itself (oracle.lattice).
"""
import numpy as np

from oracle import lattice as L

DTYPES = ("bf16", "fp16", "f16x3", "fp32")
H16 = ("bf16", "fp16", "fp32")  # channels % 64 != 0: f16x3 refuses (test_f16x3_unsupported_channels)


def _c(name, fw, strided, channels, B, T=None, causal=False, dense=False, jin=17, jout=17, distinct=None,
       period=None, dtypes=DTYPES, seed=0):
    rf = 1 + 2 * sum(L.geometry(list(fw), False, False)[0])
    return dict(name=name, fw=tuple(fw), strided=strided, channels=channels, B=B, T=T or rf, causal=causal,
                dense=dense, jin=jin, jout=jout, distinct=distinct or B, period=period, dtypes=dtypes, seed=seed)


# Small shapes on the default dispatch.  Which kernel each layer takes: profiles/lattice_exact.txt.
SMALL = [
    _c("s27_c64_b1", (3, 3, 3), True, 64, 1),
    _c("s27_causal_c8_j23_o1_b5", (3, 3, 3), True, 8, 5, causal=True, jin=23, jout=1, dtypes=H16),
    _c("s243_c1024_b300", (3, 3, 3, 3, 3), True, 1024, 300, distinct=25, jout=32),
    _c("s243_causal_c64_b5", (3, 3, 3, 3, 3), True, 64, 5, causal=True, jin=23),
    _c("w5_s75_c64_j23_o32_b5", (5, 5, 3), True, 64, 5, jin=23, jout=32),
    _c("d27_c64_b5_t61", (3, 3, 3), False, 64, 5, T=61),
    _c("d27_causal_c8_b1_t100", (3, 3, 3), False, 8, 1, T=100, causal=True, jout=1, dtypes=H16),
    _c("d243_c1024_b1_t600", (3, 3, 3, 3, 3), False, 1024, 1, T=600),  # 598..358 rows: partial last tiles
    _c("d243_causal_c64_b1_t300", (3, 3, 3, 3, 3), False, 64, 1, T=300, causal=True, jout=32),
    _c("w5_d45_c128_b2_t200", (3, 5, 3), False, 128, 2, T=200),
    _c("dense27_c64_j23_b5_t40", (3, 3, 3), False, 64, 5, T=40, dense=True, jin=23),
    _c("dense27_causal_c64_b1_t50", (3, 3, 3), False, 64, 1, T=50, dense=True, causal=True),
]

# The 256 x 256 kernels at fill.  Strided: the shape of test_gpu_lifter.test_gemm_kernel_override
# (block 1: 217 x 4 tiles, a4 / q64 / 8p / big by VP3D_GEMM; blocks 2-4 under 384 tiles: q64, the
# f16x3 tails).  The sequence is longer than that test's 20,242 frames, whose 80 x 4 tiles stay
# under the 384 that a4 and the LDS-ring kernel ask for: 34,042 frames give every block layer
# 133 x 4 = 532 tiles with a partial last row tile -- two rounds of 256 plus 20, the tail that
# conv_gemm_tail.hip splits over K (f16x3 and the 16-bit dtypes).  B = 8192 (the oracle batch of
# the B = 2050 case, tiled further): 128 tiles past the whole rounds of every block.
FILL_STRIDED = _c("fill_s243_c1024_b2050", (3, 3, 3, 3, 3), True, 1024, 2050, distinct=41)
FILL_STRIDED_HN = dict(FILL_STRIDED, B=8192)  # (same name: the same state, model and reference)
FILL_SEQ = _c("fill_d243_c1024_t34042", (3, 3, 3, 3, 3), False, 1024, 1, T=34042, period=82)

# forward_windows: sequences shorter than a window, windows overhanging both ends
GATHER = [
    _c("g27_c64", (3, 3, 3), True, 64, 37),
    _c("g243_c1024", (3, 3, 3, 3, 3), True, 1024, 24),
]
GATHER_LENS = (19, 400, 243, 57)

ALL = SMALL + [FILL_STRIDED, FILL_SEQ]
_CACHE = {}


def oracle_input(case):
    """The distinct inputs of a case: (distinct, T, jin, 2), or one period + receptive field - 1
    frames of the periodic sequence."""
    if case["period"]:
        rf = 1 + 2 * sum(L.geometry(list(case["fw"]), False, False)[0])
        one = L.lattice_windows(case["seed"] + 1, 1, case["period"], case["jin"])
        reps = -(-(case["period"] + rf - 1) // case["period"])
        return np.tile(one, (1, reps, 1, 1))[:, :case["period"] + rf - 1]
    return L.lattice_windows(case["seed"] + 1, case["distinct"], case["T"], case["jin"])


def gather_source(case, cams):
    """(sequences, camera rows or None, pairs, window, lead) of a forward_windows case: lattice
    rows, starts spread over every sequence from its first to its last frame."""
    rng = np.random.RandomState(case["seed"] + 5)
    seqs = [L.lattice_windows(case["seed"] + 11 + i, 1, n, 17)[0].reshape(n, 34) for i, n in enumerate(GATHER_LENS)]
    cam = [L.lattice_windows(case["seed"] + 31 + i, 1, n, 6)[0].reshape(n, 12) for i, n in enumerate(GATHER_LENS)] \
        if cams else None
    window = case["T"]
    pairs = [(s, st) for s, n in enumerate(GATHER_LENS) for st in (0, n - 1)]
    while len(pairs) < case["B"]:
        s = rng.randint(0, len(GATHER_LENS))
        pairs.append((s, rng.randint(0, GATHER_LENS[s])))
    return seqs, cam, np.asarray(pairs, dtype=np.int32), window, window // 2


def build(case, x=None, key=None):
    """(state, x, float64 poses, stats) of a case, the premises asserted (check_exact); cached.
    x: other oracle inputs than oracle_input's (the gathered windows), cached under `key`."""
    key = key or case["name"]
    if key not in _CACHE:
        x = oracle_input(case) if x is None else x
        ks = L.keys_shapes(x.shape[2], case["fw"], case["channels"], case["jout"], dense=case["dense"])
        sd = L.lattice_state(ks, case["seed"], case["fw"], case["causal"], case["strided"], case["dense"], calib=x)
        y, stats = L.check_exact(sd, x, case["fw"], case["causal"], case["strided"], case["dense"])
        _CACHE[key] = (sd, x, y, stats)
    return _CACHE[key]
