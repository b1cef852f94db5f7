"""The exact-lattice oracle (oracle/lattice.py) on the CPU: for every case the GPU test runs
(tests/lattice_cases.py), at its oracle batch,

  * check_exact's premises hold (powers of two, bf16-exact stored activations, sum |a w| far
    under f32's 2^24, exact weights in every dtype's form, every K index used, live layers);
  * the fold-aware float64 model agrees with the plain float64 reference, which applies BN
    unfolded (var + eps is not exactly 1 in float64);
  * a torch emulation of the 16-bit arithmetic (rounded weights and stored activations, f32
    accumulation) returns the float64 poses bit for bit, at two thread counts;
  * seeded defects of the CPU model (never of a kernel) move more than 1 % of the poses by at
    least one output lattice unit: the bit-equality gate of tests/test_gpu_lattice.py is
    sensitive to each.
The measured figures: profiles/lattice_exact.txt.
"""
import numpy as np
import pytest
import torch

import lattice_cases as LC
from oracle import lattice as L
from oracle.temporal_ref import lifter_forward

# |lattice_forward - lifter_forward(float64)|: the unfolded BN divides by sqrt(float32(0.99999)
# + 1e-5) = 1 + 1.7e-9 in float64 once per layer.  4x the largest measured over the cases
# (2.9e-7 m, g243_c1024 with cameras; profiles/lattice_exact.txt).
UNFOLDED_BN_TOL = 4 * 2.9e-7

CASES = [(c, None) for c in LC.ALL] + [(c, cams) for c in LC.GATHER for cams in (False, True)]
IDS = [c["name"] + ("" if cams is None else ("_cams" if cams else "_nocams")) for c, cams in CASES]


def _built(case, cams):
    if cams is None:
        return case, LC.build(case)
    seqs, cam, pairs, window, lead = LC.gather_source(case, cams)
    x = L.lattice_gather(seqs, pairs, window, lead, cam).reshape(len(pairs), window, -1, 2)
    return case, LC.build(case, x, key=f"{case['name']}_cams{int(cams)}")


def _geom(c):
    return dict(causal=c["causal"], strided=c["strided"], dense=c["dense"])


@pytest.mark.parametrize("case,cams", CASES, ids=IDS)
def test_premises_and_unfolded_reference(case, cams):
    c, (sd, x, y, stats) = _built(case, cams)  # build() asserts check_exact
    ref = lifter_forward(sd, x, list(c["fw"]), dtype=torch.float64, **_geom(c)).numpy()
    d = float(np.abs(ref - y).max())
    print(f"{c['name']}: |folded f64 - unfolded f64| max {d:.3e} m; poses max {np.abs(y).max():.3f} m")
    print(L.format_stats(stats))
    assert d <= UNFOLDED_BN_TOL, d
    assert d > 0.0 or c["channels"] <= 8  # (the plain reference is NOT the bit-exact yardstick)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case,cams", CASES, ids=IDS)
def test_emulated_16bit_arithmetic_is_exact(case, cams, dt):
    c, (sd, x, y, _) = _built(case, cams)
    before = torch.get_num_threads()
    try:
        for n in (1, 3):
            torch.set_num_threads(n)
            e = L.lattice_emulate(sd, x, c["fw"], dt, **_geom(c))
            assert np.array_equal(e, y.astype(np.float32)), (n, np.abs(e - y).max())
    finally:
        torch.set_num_threads(before)


def _defects(c):
    nl = 2 * (len(c["fw"]) - 1)  # block convs; the shrink is conv nl + 1
    # zero_k: the K index (tap x input channel) that most output channels of the layer read
    return [("zero_k", 0), ("zero_k", 1), ("zero_k", nl), ("zero_k", nl + 1),
            ("tap_shift", 0, 0), ("tap_shift", 1, 0), ("tap_shift", nl - 1, 0),
            ("res_row", 2), ("res_row", nl), ("shift_lo", 0)]


@pytest.mark.parametrize("case,cams", CASES, ids=IDS)
def test_seeded_defects_move_the_poses(case, cams):
    """Each defect of the CPU model changes > 1 % of the poses by >= one output lattice unit
    (2^-8 m).  On at most 8 windows spread over the oracle batch (a subset of lattice data is
    lattice data)."""
    c, (sd, x, y, _) = _built(case, cams)
    sel = np.unique(np.linspace(0, x.shape[0] - 1, min(8, x.shape[0])).astype(int))
    x, y = x[sel], y[sel]
    for d in _defects(c):
        yd = L.lattice_forward(sd, x, c["fw"], defect=d, **_geom(c))
        diff = np.abs(yd - y)
        share = float((diff >= L.OUT_UNIT).mean())
        print(f"{c['name']} {d}: {100 * share:5.1f} % of the poses moved, max {diff.max():.3e} m")
        assert share > 0.01, (d, share)


@pytest.mark.parametrize("case", LC.GATHER, ids=[c["name"] for c in LC.GATHER])
@pytest.mark.parametrize("cams", [False, True], ids=["nocams", "cams"])
def test_gather_one_frame_off_moves_the_poses(case, cams):
    c, (sd, x, y, _) = _built(case, cams)
    seqs, cam, pairs, window, lead = LC.gather_source(case, cams)
    xo = L.lattice_gather(seqs, pairs, window, lead, cam, frame_off=1).reshape(x.shape)
    sel = np.unique(np.linspace(0, x.shape[0] - 1, 8).astype(int))
    yd = L.lattice_forward(sd, xo[sel], c["fw"], **_geom(c))
    diff = np.abs(yd - y[sel])
    share = float((diff >= L.OUT_UNIT).mean())
    print(f"{c['name']} gather_off cams={cams}: {100 * share:5.1f} % of the poses moved, max {diff.max():.3e} m")
    assert share > 0.01, share


@pytest.mark.parametrize("fw,strided,T,B", [((3, 3, 3), True, 27, 16), ((3, 3, 3, 3, 3), True, 243, 8),
                                            ((3, 3, 3), False, 80, 2)])
def test_default_calibration_holds_on_other_windows(fw, strided, T, B):
    """Without `calib` the biases are set on the generator's own 8 windows under a lower cap; the
    premises then still hold on windows of another seed (check_exact decides, as for any case)."""
    sd = L.lattice_state(L.keys_shapes(17, fw, 64), 3, fw, strided=strided)
    _, stats = L.check_exact(sd, L.lattice_windows(99, B, T), fw, strided=strided)
    print(L.format_stats(stats))
