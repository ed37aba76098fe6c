"""CPU, NumPy: offmark.resync on cropped leaks that arrive as 4:2:0 planes (build extension, not reference semantics), on the
statement of tests/_planar_resync.py over the oracle.  No device code runs here; tests/test_gpu_planar_resync.py holds the
kernels against the existing planar read-outs of the same sub-planes.

Two facts are pinned here.  A crop at EVEN pixel offsets cuts sub-planes out of the marked planes and reads correctly with both
codecs; a crop at an ODD offset has to resample chroma by half a sample and destroys both marks, which is why the planar calls
score the odd phases 0 and best_phase(even_only=True) leaves them out."""
import numpy as np
import pytest

import _planar_resync as pr
import _resync as rs
import _dct_resync as dr

from offmark import resync

# contrast over the 16 even phases, measured on the recipe (seeds 3000.. and 3500.., crops (10, 20) and (2, 6)):
# DwtDctSvd 1.30-1.33, DCT 1.106-1.115, the unmarked sources <= 1.012, the odd-offset leak 1.017 / 1.005
MARKED_ABOVE = {"svd": 1.2, "dct": 1.06}


def test_cropping_planes_at_even_offsets_is_cropping_the_converted_frame():
    """Fact 1, byte for byte: the conversion replicates chroma over its 2x2 cell."""
    p = pr.marked_planes("svd")[0]
    for cy, cx in (pr.CROP, (2, 6), (0, 0)):
        assert np.array_equal(pr.to_rgb(pr.crop_planes(p, cy, cx)), pr.to_rgb(p)[cy:, cx:])


def test_statement_scores_are_the_rgb_statement_with_the_odd_phases_zeroed():
    p = pr.oracle_leak("svd")[0]
    want, budget = rs.statement_scores(pr.to_rgb(p), scale=pr.SCALE)
    got, got_budget = pr.statement_scores(p, "svd")
    assert np.array_equal(got, np.where(pr.EVEN, want, 0)) and np.array_equal(got_budget, np.where(pr.EVEN, budget, 0))
    p = pr.oracle_leak("dct")[0]
    assert np.array_equal(pr.statement_scores(p, "dct")[0], np.where(pr.EVEN, dr.statement_scores(pr.to_rgb(p)), 0))


@pytest.mark.parametrize("codec", pr.CODECS)
def test_the_recipe_end_to_end_on_the_statement(codec):
    leak, seg = pr.oracle_leak(codec), pr.recipe_segments()
    assert leak[0][0].shape == (pr.LEAK_H, pr.LEAK_W) == (62, 84) and leak[0][1].shape == (31, 42)
    scores = pr.leak_scores(codec)
    assert (scores[:, ~pr.EVEN] == 0).all() and (scores[:, pr.EVEN] > 0).all()
    found = resync.best_phase(scores, pr.LEAK_H, pr.LEAK_W, even_only=True)
    print(f"{codec}: phase {found['phase']} contrast {found['contrast']:.3f}")
    assert found["phase"] == pr.PHASE and found["contrast"] > MARKED_ABOVE[codec]
    assert (found["normalised"][~pr.EVEN] == 0).all()

    class StatementDecoder:                                        # read_cropped_leak_yuv420 on the statement in place of the device
        def sync_scores_planes_yuv420(self, planes, height, width, layout="i420"):
            return scores[:len(planes)]

        def decode_soft_window_planes_yuv420(self, planes, height, width, L, phase, canvas_cols, base=0, layout="i420"):
            return np.stack([pr.statement_window(p, codec, L, phase, canvas_cols, base) for p in leak])

    got = resync.read_cropped_leak_yuv420(StatementDecoder(), pr.pack(leak), pr.LEAK_H, pr.LEAK_W, seg, pr.W, pr.recipe_candidates(),
                                          key=pr.KEY, L=pr.L8)
    print(f"{codec}: base {got['base']} picks {list(got['picks'])} score {got['score']} against runner-up {got['runner_up_score']}")
    assert got["phase"] == pr.PHASE and got["base"] == pr.BASE == (2 * 13 + 3) % 8
    assert list(got["picks"]) == list(pr.CHOSEN) == [1, 0, 1] and not got["ambiguous"]
    first8 = resync.best_phase(scores[:8], pr.LEAK_H, pr.LEAK_W, even_only=True)      # the search reads the first 8 frames
    assert got["contrast"] == first8["contrast"] > MARKED_ABOVE[codec]


@pytest.mark.parametrize("codec", pr.CODECS)
def test_unmarked_sources_carry_no_phase(codec):
    found = resync.best_phase(pr.leak_scores(codec, "unmarked"), pr.LEAK_H, pr.LEAK_W, even_only=True)
    print(f"{codec}: unmarked sources, same crop: best phase {found['phase']}, contrast {found['contrast']:.3f}")
    assert found["contrast"] < 1.03


@pytest.mark.parametrize("codec", pr.CODECS)
def test_an_odd_crop_offset_destroys_the_mark(codec):
    """Fact 2: on planes an odd offset means chroma resampled by half a sample; no phase stands out afterwards."""
    leak = pr.odd_leak(codec)
    h, w = leak[0][0].shape
    assert (h, w) == (60, 82)
    found = resync.best_phase(pr.leak_scores(codec, "odd"), h, w, even_only=True)
    print(f"{codec}: leak through RGB at {pr.ODD_CROP}: best phase {found['phase']}, contrast {found['contrast']:.3f}")
    assert found["contrast"] < 1.05


def test_best_phase_is_unchanged_by_default_and_even_only_never_returns_an_odd_phase():
    scores = np.stack([rs.statement_scores(f)[0] for f in rs.oracle_leak()[:4]])
    old = resync.best_phase(scores, 61, 83)
    new = resync.best_phase(scores, 61, 83, even_only=False)
    assert old["phase"] == new["phase"] == rs.PHASE and old["contrast"] == new["contrast"]
    assert np.array_equal(old["normalised"], new["normalised"]) and (old["normalised"] > 0).all()
    even = resync.best_phase(scores, 61, 83, even_only=True)       # the marked grid of that RGB leak is the odd phase (5, 3)
    assert even["phase"][0] % 2 == 0 and even["phase"][1] % 2 == 0 and even["phase"] != rs.PHASE
    assert (even["normalised"][~pr.EVEN] == 0).all() and np.array_equal(even["normalised"][pr.EVEN], old["normalised"][pr.EVEN])
    rng = np.random.default_rng(1)
    for _ in range(20):
        s = rng.integers(0, 1 << 20, (3, 64))
        s[:, rng.integers(0, 64)] += 1 << 22                       # any phase may hold the largest score
        got = resync.best_phase(s, 72, 104, even_only=True)
        assert got["phase"][0] % 2 == 0 and got["phase"][1] % 2 == 0
        top2 = np.sort(got["normalised"][pr.EVEN])[-2:]
        assert got["contrast"] == top2[1] / top2[0]
    only = resync.best_phase(np.ones(64, np.int64), 8, 8, even_only=True)     # one phase with a unit
    assert only["phase"] == (0, 0) and only["contrast"] == float("inf")
