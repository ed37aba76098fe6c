"""CPU, NumPy: offmark.resync (block-grid resync of cropped DwtDctSvd leaks; build extension, not reference semantics) on the
statement of tests/_resync.py -- the reference's decoder gives s0 per unit, the metric is rint(-sin(2 pi s0 / scale) * 2^14).
No device code runs here; tests/test_gpu_resync.py holds the kernels against the same statement."""
import itertools

import numpy as np
import pytest

import offmark_oracle as orc
import _resync as rs

from offmark import resync
from offmark.fingerprint import payload_for_segment

P8 = np.array([0, 1, 1, 0, 0, 1, 0, 1])


def test_units_per_phase():
    u = resync.units_per_phase(61, 83)
    assert u.shape == (64,) and u.dtype == np.int64
    for py in range(8):
        for px in range(8):
            assert u[8 * py + px] == ((61 - py) // 8) * ((83 - px) // 8)
    assert u[0] == 7 * 10 and u[8 * 5 + 3] == 7 * 10 and u[8 * 6 + 4] == 6 * 9
    one = np.zeros(64, np.int64)
    one[0] = 1
    assert np.array_equal(resync.units_per_phase(8, 8), one)
    u = resync.units_per_phase(8, 40)
    assert np.array_equal(u[:8], [5, 4, 4, 4, 4, 4, 4, 4]) and not u[8:].any()


@pytest.mark.parametrize("dy,dx", [(0, 0), (3, 5), (1, 0), (6, 2)])
def test_best_phase_recovers_the_crop(dy, dx):
    marked = rs.oracle_mark(orc.synthetic_frame(72, 104, 41 + dy + 8 * dx), P8)
    leak = marked[dy:, dx:]
    scores, _ = rs.statement_scores(leak)
    got = resync.best_phase(scores, *leak.shape[:2])
    print(f"crop ({dy}, {dx}): phase {got['phase']}, top {got['normalised'].max():.3f}, contrast {got['contrast']:.3f}")
    assert got["phase"] == ((-dy) % 8, (-dx) % 8)
    assert got["contrast"] > 1.2
    # rows are added: the same frame twice gives the same answer
    twice = resync.best_phase(np.stack([scores, scores]), *leak.shape[:2])
    assert twice["phase"] == got["phase"] and np.allclose(twice["normalised"], got["normalised"])


def test_flat_frame_carries_no_phase():
    scores, _ = rs.statement_scores(np.full((72, 104, 3), 128, np.uint8))
    got = resync.best_phase(scores, 72, 104)
    print(f"flat grey: top {got['normalised'].max():.3f}, contrast {got['contrast']:.4f}")
    assert got["contrast"] < 1.01


def test_phases_without_units_are_excluded():
    scores = np.zeros(64, np.int64)
    scores[:8] = [3 * 16384, 4 * 16384, 0, 0, 0, 0, 0, 0]
    scores[9] = 10 ** 9                                            # a phase an 8x40 frame does not have: ignored
    got = resync.best_phase(scores, 8, 40)
    assert got["phase"] == (0, 1) and got["normalised"][9] == 0 and abs(got["contrast"] - (4 / 4) / (3 / 5)) < 1e-12
    assert resync.best_phase(np.array([5] + [0] * 63), 8, 8)["contrast"] == float("inf")
    with pytest.raises(ValueError):
        resync.best_phase(np.zeros(64), 7, 40)


@pytest.mark.parametrize("S", [2, 3, 4])
def test_rotation_is_unique_for_every_copy_choice(S):
    L, key = 8, 0
    cands = [[payload_for_segment(s + 1, c) for c in range(2)] for s in range(S)]
    for chosen in itertools.product(range(2), repeat=S):
        perfect = np.stack([(2 * resync.shuffled(cands[s][chosen[s]], key).astype(np.int64) - 1) * 16384 for s in range(S)])
        for base in range(L):
            read = np.roll(perfect, -base, axis=1)                 # read[s][q] = perfect[s][(q + base) % L]
            got = resync.align_segments(read, cands, key)
            assert got["base"] == base and list(got["picks"]) == list(chosen) and not got["ambiguous"], (chosen, base, got)
            assert got["score"] == S * L * 16384 and got["runner_up_score"] < got["score"]


def test_a_constructed_tie_is_reported():
    L, key = 8, 0
    perm = resync.shuffled(np.arange(L), key)                      # shuffled(p)[q] = p[perm[q]]
    inv = np.argsort(perm)

    def unshuffled(w):                                             # the payload whose shuffled form is w
        return np.asarray(w)[inv]

    assert np.array_equal(resync.shuffled(unshuffled(P8), key), P8)
    w0, w1 = np.array([1, 1, 0, 1, 0, 0, 0, 1]), np.array([0, 1, 1, 1, 0, 1, 0, 0])
    cands = [[unshuffled(w), unshuffled(np.roll(w, 3))] for w in (w0, w1)]      # per segment: a pattern and its rotation by 3
    read = np.stack([(2 * w.astype(np.int64) - 1) * 16384 for w in (w0, w1)])
    got = resync.align_segments(read, cands, key)
    assert got["ambiguous"] and got["score"] == got["runner_up_score"] == 2 * L * 16384
    assert got["base"] in (0, 3)


def test_the_recipe_end_to_end_on_the_statement():
    leak = rs.oracle_leak()
    assert leak.shape == (12, 61, 83, 3)
    scores = np.stack([rs.statement_scores(f)[0] for f in leak[:8]])
    found = resync.best_phase(scores, 61, 83)
    assert found["phase"] == rs.PHASE
    seg = rs.recipe_segments()
    soft = np.stack([rs.statement_window(f, rs.L8, found["phase"], rs.W // 8) for f in leak])
    by_segment = np.stack([soft[seg == s].sum(axis=0) for s in range(rs.S)])
    got = resync.align_segments(by_segment, rs.recipe_candidates(), rs.KEY)
    print(f"contrast {found['contrast']:.3f}, alignment score {got['score']} against runner-up {got['runner_up_score']}")
    assert got["base"] == rs.BASE and list(got["picks"]) == list(rs.CHOSEN) and not got["ambiguous"]
    assert got["score"] > 1.5 * got["runner_up_score"]             # 13 145 782 against 7 080 502 with float32 LAPACK

    class StatementDecoder:                                        # read_cropped_leak on the statement in place of the device
        def sync_scores_u8(self, frames):
            return np.stack([rs.statement_scores(f)[0] for f in frames])

        def decode_soft_window_u8(self, frames, L, phase, canvas_cols, base=0):
            return np.stack([rs.statement_window(f, L, phase, canvas_cols, base) for f in frames])

    out = resync.read_cropped_leak(StatementDecoder(), leak, seg, rs.W, rs.recipe_candidates(), key=rs.KEY, L=rs.L8, search_frames=2)
    assert out["phase"] == rs.PHASE and out["base"] == rs.BASE and list(out["picks"]) == list(rs.CHOSEN) and not out["ambiguous"]
    assert out["score"] == got["score"]
