"""CPU-only: the statement of the tone calls (tests/_tone.py) and the host side of offmark.tone -- lut_of_histograms, lut_of_sums and
read_toned_leak on the StatementDecoder.

The evidence: tests/_affine_phase.py's leak "A" (the 72 x 104 recipe, oracle-marked, copies [1, 0, 1], rotated by 2 degrees, cropped
to 56 x 90, 12 frames), 4 search frames, its bytes sent through clip(rint(255 * (clip(a x + b, 0, 255) / 255) ** gamma), 0, 255).
Measured with this file (score of the pick, luma rms of the registration, corner_move against the untouched leak's geometry):

  (a, b, gamma)        plain read_registered_leak                 read_toned_leak                          score ratios (toned, |plain|)
  none                 [1, 0, 1]  8 682 833  rms 4.61             [1, 0, 1]  6 467 733  rms 4.59  0.021 px    0.745
  (0.85, 15, 1)        [0, 1, 1]    255 883  rms 10.55  0.246 px  [1, 0, 1]  6 504 355  rms 4.59  0.019 px    0.749  0.030
  (1.10, -8, 1)        [1, 1, 0]   -206 963  rms 7.74   0.141 px  [1, 0, 1]  5 975 349  rms 4.65  0.031 px    0.688  0.024
  (1, 0, 0.85)         [1, 0, 0]    364 639  rms 12.35  0.704 px  [1, 0, 1]  6 506 193  rms 4.59  0.021 px    0.749  0.042
  (1, 0, 1.20)         [1, 1, 1]    258 787  rms 13.55  0.731 px  [1, 0, 1]  6 544 876  rms 4.59  0.023 px    0.754  0.030
  (0.70, 40, 1.10)     [0, 0, 1]   -315 282  rms 17.90  0.650 px  [1, 0, 1]  6 431 272  rms 4.59  0.020 px    0.741  0.036

The first registration (on the histogram-matched leak) lands 0.14 - 0.17 px from the untouched leak's geometry.  The tone fit costs the
untouched leak a quarter of its score (the fitted curve is a step function of 256 means, and the mark is part of what it averages),
which is why read_toned_leak is a separate call and not read_registered_leak's default."""
import functools

import numpy as np
import pytest

import _affine as af
import _affine_phase as ap
import _resync as rs
import _tone as tn

CANVAS = ap.CANVAS


def read(fn, frames):
    return fn(tn.StatementDecoder(), frames, rs.recipe_sources(), rs.recipe_segments(), CANVAS, rs.recipe_candidates(), key=af.KEY, L=af.L8,
              search_frames=ap.SEARCH_FRAMES)


@functools.lru_cache(maxsize=None)
def untouched():
    from offmark import resync
    return read(resync.read_registered_leak, ap.leak("svd", "A"))


def test_a_one_pixel_and_a_two_by_two_case_by_hand():
    one = np.array([[[[7, 200, 7]]]], np.uint8)
    h = tn.histograms(one)
    assert h.shape == (1, 3, 256) and h.sum() == 3 and h[0, 0, 7] == 1 and h[0, 1, 200] == 1 and h[0, 2, 7] == 1
    # the identity geometry: canvas pixel (0, 0) reads leak pixel (0, 0), every other canvas pixel is outside a 1 x 1 leak
    src = np.arange(8 * 8 * 3, dtype=np.uint8).reshape(1, 8, 8, 3) + 50
    s = tn.statement_sums(src, one, [af.IDENTITY])
    assert s.shape == (1, 1, 3, 256, 2) and s[..., 0].sum() == 3
    assert tuple(s[0, 0, 0, 7]) == (1, 50) and tuple(s[0, 0, 1, 200]) == (1, 51) and tuple(s[0, 0, 2, 7]) == (1, 52)
    two = np.array([[[[1, 2, 3], [1, 5, 6]], [[9, 2, 3], [1, 2, 255]]]], np.uint8)
    h = tn.histograms(two)[0]
    assert h.sum() == 12 and h[0, 1] == 3 and h[0, 9] == 1 and h[1, 2] == 3 and h[1, 5] == 1 and h[2, 3] == 2 and h[2, 6] == 1 and h[2, 255] == 1
    s = tn.statement_sums(src, two, [af.IDENTITY])[0, 0]
    # leak (y, x) lands on canvas (y, x): channel 0 has value 1 at (0, 0), (0, 1), (1, 1) and 9 at (1, 0)
    assert s[..., 0].sum() == 12
    assert tuple(s[0, 1]) == (3, int(src[0, 0, 0, 0]) + int(src[0, 0, 1, 0]) + int(src[0, 1, 1, 0])) and tuple(s[0, 9]) == (1, int(src[0, 1, 0, 0]))
    assert tuple(s[2, 255]) == (1, int(src[0, 1, 1, 2])) and tuple(s[1, 5]) == (1, int(src[0, 0, 1, 1]))
    lut = np.stack([np.arange(256), 255 - np.arange(256), np.full(256, 9)]).astype(np.uint8)
    assert np.array_equal(tn.apply_tone(two, lut)[0, 1, 1], [1, 253, 9])


def test_the_counts_add_up_to_the_inside_pixels():
    from offmark import resync
    frames, sources = ap.leak("svd", "A")[:2], rs.recipe_sources()[:2]
    cands = [ap.geometry("A"), resync.affine_of_rotation(CANVAS, (56, 90), 0.0), af.hflip(90), (af.ONE, 0, 30 << 16, 0, af.ONE, 40 << 16), (0,) * 6]
    s = tn.statement_sums(sources, frames, cands)
    for f in range(2):
        for k, g in enumerate(cands):
            inside = int(af.warp(frames[f], g, CANVAS)[1].sum()) if resync._affine_ok(g) else 0
            assert (s[f, k, :, :, 0].sum(axis=1) == inside).all(), (f, k)
            assert (s[f, k, :, :, 1] <= 255 * s[f, k, :, :, 0]).all()
    assert s[:, :4, :, :, 0].any() and not s[:, 4].any()


def test_a_histogram_matched_to_itself_is_the_identity_on_populated_levels():
    from offmark import tone
    h = tn.histograms(ap.leak("svd", "A")[:4]).sum(axis=0)
    lut = tone.lut_of_histograms(h, h)
    assert lut.dtype == np.uint8 and lut.shape == (3, 256)
    for c in range(3):
        have = h[c] > 0
        assert have.sum() > 50 and np.array_equal(lut[c][have], np.arange(256)[have])
        assert (np.diff(lut[c].astype(int)) >= 0).all()
    # products far beyond int64, and an empty side
    big = np.zeros((3, 256), np.int64)
    big[:, 10], big[:, 20] = 1 << 60, 3 << 60
    small = np.zeros((3, 256), np.int64)
    small[:, 100], small[:, 200] = 1 << 40, 3 << 40
    lut = tone.lut_of_histograms(big, small)
    assert (lut[:, 10] == 100).all() and (lut[:, 20] == 200).all() and (lut[:, :10] == 0).all() and (lut[:, 11:20] == 100).all()
    assert np.array_equal(tone.lut_of_histograms(np.zeros((3, 256), np.int64), small), np.tile(np.arange(256, dtype=np.uint8), (3, 1)))
    with pytest.raises(ValueError):
        tone.lut_of_histograms(h[:2], h)


def test_lut_of_sums_is_non_decreasing_and_recovers_a_known_curve():
    from offmark import tone
    # a frame holding all 256 levels in every channel, and sources built from known monotone tables
    leak = np.stack([np.arange(64 * 64) % 256, (np.arange(64 * 64) * 7) % 256, 255 - np.arange(64 * 64) % 256], axis=-1).astype(np.uint8).reshape(1, 64, 64, 3)
    x = np.arange(256, dtype=np.float64)
    known = np.stack([np.clip(np.rint(0.85 * x + 15), 0, 255), np.clip(np.rint(255 * (x / 255) ** 0.85), 0, 255), np.clip(np.rint(1.2 * x - 20), 0, 255)]).astype(np.uint8)
    assert (np.diff(known.astype(int), axis=1) >= 0).all()
    src = tn.apply_tone(leak, known)
    s = tn.statement_sums(src, leak, [af.IDENTITY]).sum(axis=0)[0]
    assert (s[:, :, 0] == 16).all()
    assert np.array_equal(tone.lut_of_sums(s), known)
    # noisy, non-monotone means: the fit is still monotone, pools by weight, and interpolates the gaps
    t = np.zeros((3, 256, 2), np.int64)
    for v, (n, mean) in {10: (4, 50), 20: (1, 40), 30: (1, 30), 40: (2, 100)}.items():
        t[0, v] = (n, n * mean)
    lut = tone.lut_of_sums(t)
    assert (np.diff(lut.astype(int), axis=1) >= 0).all()
    assert lut[0, 10] == lut[0, 20] == lut[0, 30] == 45 and lut[0, 40] == 100 and lut[0, 0] == 45 and lut[0, 255] == 100      # (200 + 40 + 30) / 6 = 45
    assert lut[0, 32] == 56 and np.array_equal(lut[1], np.arange(256))
    real = tn.statement_sums(rs.recipe_sources()[:2], tn.tone_map(ap.leak("svd", "A")[:2], 0.85, 15.0, 1.0), [ap.geometry("A")]).sum(axis=0)[0]
    assert (np.diff(tone.lut_of_sums(real).astype(int), axis=1) >= 0).all()


def test_lut_of_sums_gives_the_identity_for_an_empty_channel():
    from offmark import tone
    t = np.zeros((3, 256, 2), np.int64)
    t[1, 100] = (5, 600)                                       # one populated level: fewer than 2
    t[2, 0], t[2, 255] = (1, 10), (1, 20)
    lut = tone.lut_of_sums(t)
    ident = np.arange(256, dtype=np.uint8)
    assert np.array_equal(lut[0], ident) and np.array_equal(lut[1], ident)
    assert lut[2, 0] == 10 and lut[2, 255] == 20 and lut[2, 128] == 15
    with pytest.raises(ValueError):
        tone.lut_of_sums(t[:, :, 0])


@pytest.mark.parametrize("name", list(tn.TONE_MAPS))
def test_a_tone_mapped_leak_is_misread_plainly_and_read_with_the_tone_fit(name):
    from offmark import resync, tone
    clean = untouched()
    assert list(clean["picks"]) == [1, 0, 1] and clean["score"] > 8_000_000
    leak = tn.tone_map(ap.leak("svd", "A"), *tn.TONE_MAPS[name])
    plain = read(resync.read_registered_leak, leak)
    got = read(tone.read_toned_leak, leak)
    print(f"{name}: plain {[int(p) for p in plain['picks']]} score {plain['score']} rms {plain['registration']['rms']:.2f} | toned "
          f"{[int(p) for p in got['picks']]} score {got['score']} rms {got['registration']['rms']:.2f} "
          f"{resync.corner_move(got['geometry'], clean['geometry'], CANVAS):.3f} px; ratios {got['score'] / clean['score']:.3f} "
          f"{abs(plain['score']) / clean['score']:.4f}")
    assert list(plain["picks"]) != [1, 0, 1]                   # on record: today's route returns another subscriber
    assert abs(plain["score"]) < 0.1 * clean["score"]
    assert list(got["picks"]) == list(af.CHOSEN) == [1, 0, 1] and not got["ambiguous"] and got["registration"]["converged"]
    assert got["score"] > 0.5 * clean["score"]
    t = got["tone"]
    assert set(t) == {"lut0", "lut", "first_registration"} and t["lut"].shape == t["lut0"].shape == (3, 256) and t["lut"].dtype == np.uint8
    assert (np.diff(t["lut"].astype(int), axis=1) >= 0).all() and t["first_registration"]["converged"]


def test_the_untouched_leak_still_reads_through_the_tone_fit():
    from offmark import resync, tone
    got = read(tone.read_toned_leak, ap.leak("svd", "A"))
    assert list(got["picks"]) == [1, 0, 1] and not got["ambiguous"] and got["registration"]["converged"]
    assert resync.corner_move(got["geometry"], untouched()["geometry"], CANVAS) < 0.1


def test_a_decoder_without_the_tone_calls_is_refused():
    import _align as al
    from offmark import tone
    with pytest.raises(ValueError, match="affine"):
        tone.read_toned_leak(al.StatementDecoder(), ap.leak("svd", "A"), rs.recipe_sources(), rs.recipe_segments(), CANVAS, rs.recipe_candidates(),
                             key=af.KEY, L=af.L8, search_frames=ap.SEARCH_FRAMES)
