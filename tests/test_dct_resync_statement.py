"""CPU, NumPy: offmark.resync on the DCT codec (block-grid resync of cropped leaks; build extension, not reference semantics), on the
statement of tests/_dct_resync.py -- the reference's decoder reads each phase's crop with the crop's own masks and frame mean, the
metric is rint(-cos(pi C21 / step) * 2^14).  No device code runs here; tests/test_gpu_dct_resync.py holds the kernels against the
read-out of the same crops."""
import numpy as np

import offmark_oracle as orc
import _dct_resync as dr

from offmark import resync
from offmark.degenerator.de_shuffler import DeShuffler
from offmark.dist.vote import soft_vote


def test_best_phase_recovers_the_crop_summed_and_frame_by_frame():
    scores = dr.oracle_leak_scores()
    found = resync.best_phase(scores, 61, 83)
    others = np.delete(found["normalised"], 8 * dr.PHASE[0] + dr.PHASE[1])
    print(f"phase {found['phase']}: normalised {found['normalised'].max():.3f}, median of the others {np.median(others):.3f}, "
          f"contrast {found['contrast']:.3f}")
    assert found["phase"] == dr.PHASE
    assert found["contrast"] > 1.1                                  # 1.183: C21 is low-frequency, neighbouring phases correlate
    for f in range(scores.shape[0]):
        assert resync.best_phase(scores[f], 61, 83)["phase"] == dr.PHASE, f


def test_unmarked_sources_carry_no_phase():
    scores = np.stack([dr.statement_scores(f) for f in dr.unmarked_leak()])
    found = resync.best_phase(scores, 61, 83)
    print(f"unmarked sources, same crop: best phase {found['phase']}, contrast {found['contrast']:.3f}")
    assert found["contrast"] < 1.05                                 # 1.005


def test_the_recipe_end_to_end_on_the_statement():
    leak = dr.oracle_leak()
    assert leak.shape == (12, 61, 83, 3)
    seg = dr.recipe_segments()
    soft = np.stack([dr.statement_window(f, dr.L8, dr.PHASE, dr.W // 8) for f in leak])
    by_segment = np.stack([soft[seg == s].sum(axis=0) for s in range(dr.S)])
    got = resync.align_segments(by_segment, dr.recipe_candidates(), dr.KEY)
    print(f"alignment base {got['base']} picks {list(got['picks'])} score {got['score']} against runner-up {got['runner_up_score']}")
    assert got["base"] == dr.BASE and list(got["picks"]) == list(dr.CHOSEN) and not got["ambiguous"]

    class StatementDecoder:                                        # read_cropped_leak on the statement in place of the device
        def sync_scores_u8(self, frames):
            return dr.oracle_leak_scores()[:len(frames)]

        def decode_soft_window_u8(self, frames, L, phase, canvas_cols, base=0):
            return np.stack([dr.statement_window(f, L, phase, canvas_cols, base) for f in frames])

    out = resync.read_cropped_leak(StatementDecoder(), leak, seg, dr.W, dr.recipe_candidates(), key=dr.KEY, L=dr.L8)
    assert out["phase"] == dr.PHASE and out["base"] == dr.BASE and list(out["picks"]) == list(dr.CHOSEN) and not out["ambiguous"]
    assert out["score"] == got["score"]


def test_the_plain_read_out_of_the_leak_fails():
    """What the feature buys: the leak cut to a multiple of 8 at phase (0, 0), read by sign."""
    leak, pay, seg = dr.oracle_leak(), dr.recipe_payloads(), dr.recipe_segments()
    plain = np.stack([orc.soft_sums(np.ascontiguousarray(f[:56, :80]), dr.L8, alpha=dr.ALPHA) for f in leak])
    by_sign = soft_vote(plain, DeShuffler(key=dr.KEY).set_shape((dr.L8,)).payload_idx, seg)
    right = sum(int(np.array_equal(by_sign[s], pay[s])) for s in range(dr.S))
    print(f"plain read-out at phase (0, 0): {right}/3 segments by sign")
    assert right < 3
