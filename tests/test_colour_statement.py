"""CPU-only: the statement of the colour calls (tests/_colour.py) and the host side of offmark.colour -- matrix_of_sums, residual_rms
and read_coloured_leak on the StatementDecoder.

The evidence: tests/_affine_phase.py's leak "A" (the 72 x 104 recipe, oracle-marked, copies [1, 0, 1], rotated by 2 degrees, cropped
to 56 x 90, 12 frames), 4 search frames, its pixels sent through clip(rint(a * (M x) + b), 0, 255) with the matrices of
tests/_colour.py (sat, hue about BT.601's chroma plane, the BT.601 / BT.709 mix-ups).  The untouched leak reads [1, 0, 1] at
8 682 833 through read_registered_leak.  Each parametrised case prints the copies and scores of the three routes (plain
read_registered_leak, read_toned_leak, read_coloured_leak), the fit's share of the clean score and its ratio to the better of the other
two; the figures the change was specified against:

  attack                           plain                  toned                  matrix fit             share of clean
  identity                         [1,0,1] 8 682 833      [1,0,1] 6 467 733      [1,0,1] 3 142 640      0.362
  sat 0.8                          [0,0,1]   345 722      [1,0,0]   628 458      [1,0,1] 3 081 887      0.355
  sat 1.25                         [1,1,1]    93 368      [0,0,0]   566 431      [1,0,1] 2 479 384      0.286
  sat 0.6                          [1,1,1]   256 478      [0,1,1]   671 838      [1,0,1] 3 144 967      0.362
  hue +10                          [1,0,1]   451 836      [1,0,1]   406 080      [1,0,1] 2 933 226      0.338
  hue -20                          [1,1,0]   953 332      [1,1,0]   192 721      [1,0,1] 2 721 217      0.313
  601as709                         [0,1,1]   131 337      [0,0,1]    94 389      [1,0,1] 3 256 019      0.375
  709as601                         [1,0,0]   189 998      [0,1,0]   -46 308      [1,0,1] 2 447 611      0.282
  sat 0.8, a 0.85, b 15            [0,1,0]   126 776      [1,0,0]   653 883      [1,0,1] 3 120 583      0.359
  hue 10 . sat 1.2, a 1.10, b -8   [0,1,1]   306 148      [1,1,1]   263 288      [1,0,1] 2 430 780      0.280

The lowest share is 0.280 and the lowest ratio to the other routes 2.85 (hue -20), so the asserted 0.2 and 2 leave a margin of 1.4.
The fit costs the untouched leak 64 % of its score (the tone fit costs 25 %): read_coloured_leak is a call of its own.

NOT handled, on record: a matrix followed by a gamma.  sat 0.8 then gamma 0.85: the matrix fit alone reads [1, 0, 1] at 0.083 of the
clean score; hue 10 then gamma 0.85: 0.105; 601as709 then gamma 1.2: the matrix fit alone misreads, and the fit followed by
read_toned_leak reaches 0.47 there but misreads the hue case.  There is no reliable route yet and none is built."""
import functools

import numpy as np
import pytest

import _affine as af
import _affine_phase as ap
import _colour as co
import _resync as rs

CANVAS = ap.CANVAS
ONE = 65536


def read(fn, frames):
    return fn(co.StatementDecoder(), frames, rs.recipe_sources(), rs.recipe_segments(), CANVAS, rs.recipe_candidates(), key=af.KEY, L=af.L8,
              search_frames=ap.SEARCH_FRAMES)


@functools.lru_cache(maxsize=None)
def untouched():
    from offmark import resync
    return read(resync.read_registered_leak, ap.leak("svd", "A"))


def by_hand(l, s):
    """The 28 sums of a list of (leak pixel, source pixel) pairs, spelled out."""
    out = [0] * 28
    for lp, sp in zip(l, s):
        lp, sp = [int(v) for v in lp], [int(v) for v in sp]
        out[0] += 1
        for c in range(3):
            out[1 + c] += lp[c]
            out[4 + c] += sp[c]
        for n, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            out[7 + n] += lp[i] * lp[j]
            out[13 + n] += sp[i] * sp[j]
        for i in range(3):
            for j in range(3):
                out[19 + 3 * i + j] += lp[i] * sp[j]
    return out


def test_a_one_pixel_and_a_two_by_two_case_by_hand():
    # the identity geometry: canvas pixel (0, 0) reads leak pixel (0, 0), every other canvas pixel is outside a 1 x 1 leak
    src = np.arange(8 * 8 * 3, dtype=np.uint8).reshape(1, 8, 8, 3) + 50            # source pixel (0, 0) = (50, 51, 52)
    one = np.array([[[[7, 200, 9]]]], np.uint8)
    s = co.statement_sums(src, one, [af.IDENTITY])
    assert s.shape == (1, 1, 28) and s.dtype == np.int64
    assert list(s[0, 0]) == [1, 7, 200, 9, 50, 51, 52, 49, 1400, 63, 40000, 1800, 81, 2500, 2550, 2600, 2601, 2652, 2704,
                             350, 357, 364, 10000, 10200, 10400, 450, 459, 468]
    two = np.array([[[[1, 2, 3], [10, 5, 6]], [[9, 2, 254], [100, 20, 30]]]], np.uint8)
    s = co.statement_sums(src, two, [af.IDENTITY])[0, 0]
    pairs_l = [two[0, y, x] for y in range(2) for x in range(2)]
    pairs_s = [src[0, y, x] for y in range(2) for x in range(2)]
    assert list(s) == by_hand(pairs_l, pairs_s)
    assert s[0] == 4 and s[1] == 120 and s[3] == 293 and s[7] == 1 + 100 + 81 + 10000 and s[4] == 50 + 53 + 74 + 77
    assert s[19] == 1 * 50 + 10 * 53 + 9 * 74 + 100 * 77 and s[19 + 3 * 2 + 1] == 3 * 51 + 6 * 54 + 254 * 75 + 30 * 78
    m = np.asarray([[ONE, 0, 0, 0], [0, -ONE, 0, 255 * ONE], [ONE // 2, ONE // 2, 0, 32768]], np.int32)
    assert np.array_equal(co.apply_colour(two, m)[0, 1, 1], [100, 235, 61])      # (100 + 20) / 2 + 0.5 -> 60.5 + 0.5 -> 61


def test_a_pixel_with_a_clipped_byte_contributes_to_nothing():
    src = np.arange(8 * 8 * 3, dtype=np.uint8).reshape(1, 8, 8, 3) + 50
    two = np.array([[[[1, 2, 3], [10, 5, 6]], [[9, 2, 254], [100, 20, 30]]]], np.uint8)
    kept = co.statement_sums(src, two, [af.IDENTITY])[0, 0]
    for ch in range(3):
        for v in (0, 255):
            hit = two.copy()
            hit[0, 1, 1, ch] = v                                # pixel (1, 1) leaves every one of the 28 sums
            s = co.statement_sums(src, hit, [af.IDENTITY])[0, 0]
            assert list(s) == by_hand([two[0, 0, 0], two[0, 0, 1], two[0, 1, 0]], [src[0, 0, 0], src[0, 0, 1], src[0, 1, 0]]), (ch, v)
            assert s[0] == 3 and (s <= kept).all()
    assert not co.statement_sums(src, np.full((1, 2, 2, 3), 255, np.uint8), [af.IDENTITY]).any()
    assert not co.statement_sums(src, np.array([[[[0, 7, 7], [7, 0, 7]], [[7, 7, 0], [255, 7, 7]]]], np.uint8), [af.IDENTITY]).any()
    # the SOURCE's bytes do not decide: 0 and 255 there are counted
    flat = np.zeros((1, 8, 8, 3), np.uint8)
    flat[0, 0, 1] = 255
    s = co.statement_sums(flat, two, [af.IDENTITY])[0, 0]
    assert s[0] == 4 and list(s[4:7]) == [255] * 3


def test_the_count_is_the_inside_pixels_minus_the_excluded_ones():
    from offmark import resync
    frames, sources = np.array(ap.leak("svd", "A")[:2]), rs.recipe_sources()[:2]
    frames[0, 10:20, 10:30, 1] = 255                            # make sure that some pixels are excluded
    frames[1, 30:35, 40:60, 2] = 0
    cands = [ap.geometry("A"), resync.affine_of_rotation(CANVAS, (56, 90), 0.0), af.hflip(90), (af.ONE, 0, 30 << 16, 0, af.ONE, 40 << 16), (0,) * 6]
    s = co.statement_sums(sources, frames, cands)
    excluded_somewhere = False
    for f in range(2):
        for k, g in enumerate(cands):
            if not resync._affine_ok(g):
                assert not s[f, k].any()
                continue
            warped, inside = af.warp(frames[f], g, CANVAS)
            excluded = inside & ((warped == 0) | (warped == 255)).any(axis=2)
            excluded_somewhere |= bool(excluded.any())
            assert s[f, k, 0] == int(inside.sum()) - int(excluded.sum()), (f, k)
            assert (s[f, k, 1:7] <= 255 * s[f, k, 0]).all() and (s[f, k, 1:4] >= s[f, k, 0]).all()
    assert excluded_somewhere and s[:, :4, 0].all() and not s[:, 4].any()


def test_matrix_of_sums_recovers_a_known_matrix_exactly():
    from offmark import colour
    # quarters and halves of 1..254 bytes that stay inside 0..255 and land on integers only when the leak's bytes are multiples of 4
    known = np.asarray([[ONE // 2, ONE // 4, 0, 10 * ONE], [-ONE // 4, ONE // 2, ONE // 4, 70 * ONE], [0, -ONE // 2, ONE // 4, 130 * ONE]], np.int32)
    leak = (np.random.default_rng(5).integers(1, 63, (1, 64, 64, 3)) * 4).astype(np.uint8)
    x = leak.astype(np.int64)
    exact = np.stack([(known[c, :3].astype(np.int64) * x).sum(axis=-1) + known[c, 3] for c in range(3)], axis=-1)
    assert (exact % ONE == 0).all() and (exact >= 0).all() and (exact <= 255 * ONE).all()      # noise free: no rounding, no clipping
    src = (exact // ONE).astype(np.uint8)
    assert np.array_equal(src, co.apply_colour(leak, known))
    s = co.statement_sums(src, leak, [af.IDENTITY]).sum(axis=0)[0]
    assert s[0] == 4096
    m, fitted = colour.matrix_of_sums(s)
    assert fitted and m.dtype == np.int32 and m.shape == (3, 4) and np.array_equal(m, known)
    assert colour.residual_rms(s, m) == 0.0
    assert colour.residual_rms(s, colour.identity()) > 10.0
    # every source channel a copy of the leak's first: a permutation-like matrix comes back as exactly that
    m0, fitted = colour.matrix_of_sums(co.statement_sums(leak[..., [0, 0, 0]], leak, [af.IDENTITY])[0, 0])
    assert fitted and np.array_equal(m0[:, 0], [ONE] * 3) and not m0[:, 1:].any()
    # thirds are not representable in Q16: each entry is the exact fraction rounded once, 65536 / 3 = 21845.33 -> 21845
    l3 = (np.random.default_rng(7).integers(1, 80, (1, 64, 64, 3)) * 3).astype(np.uint8)
    s3 = (l3.astype(np.int64).sum(axis=-1, keepdims=True) // 3).astype(np.uint8)[..., [0, 0, 0]]      # (l0 + l1 + l2) / 3, an integer
    m3, fitted = colour.matrix_of_sums(co.statement_sums(s3, l3, [af.IDENTITY])[0, 0])
    assert fitted and np.array_equal(m3, [[21845, 21845, 21845, 0]] * 3)
    with pytest.raises(ValueError):
        colour.matrix_of_sums(s[:27])
    with pytest.raises(ValueError):
        colour.residual_rms(s, known[:2])


def test_matrix_of_sums_gives_the_identity_where_nothing_can_be_fitted():
    from offmark import colour
    ident = colour.identity()
    assert np.array_equal(ident, co.IDENTITY_MATRIX) and ident.dtype == np.int32
    rng = np.random.default_rng(6)
    src = rng.integers(0, 256, (1, 64, 64, 3), dtype=np.uint8)
    # flat content: one value per channel, the 4 x 4 system has rank 1
    flat = np.empty((1, 64, 64, 3), np.uint8)
    flat[...] = (10, 120, 200)
    m, fitted = colour.matrix_of_sums(co.statement_sums(src, flat, [af.IDENTITY])[0, 0])
    assert not fitted and np.array_equal(m, ident)
    # collinear channels: l_1 = l_0 (grey content), rank 3
    grey = rng.integers(1, 255, (1, 64, 64, 1), dtype=np.uint8)
    grey = np.concatenate([grey, grey, rng.integers(1, 255, (1, 64, 64, 1), dtype=np.uint8)], axis=-1)
    s = co.statement_sums(src, grey, [af.IDENTITY])[0, 0]
    assert s[0] == 4096
    m, fitted = colour.matrix_of_sums(s)
    assert not fitted and np.array_equal(m, ident)
    # a count below 384: 19 x 20 = 380 pixels of perfectly good content; 384 are enough
    noise = rng.integers(1, 255, (1, 20, 20, 3), dtype=np.uint8)
    few = co.statement_sums(noise[:, :19], noise[:, :19], [af.IDENTITY])[0, 0]
    assert few[0] == 380
    m, fitted = colour.matrix_of_sums(few)
    assert not fitted and np.array_equal(m, ident)
    noise = rng.integers(1, 255, (1, 16, 24, 3), dtype=np.uint8)
    enough = co.statement_sums(noise, noise, [af.IDENTITY])[0, 0]
    assert enough[0] == 384
    m, fitted = colour.matrix_of_sums(enough)
    assert fitted and np.array_equal(m, ident)
    assert not colour.matrix_of_sums(np.zeros(28, np.int64))[1]
    # an entry out of the apply range: the source is 40 times the leak's first channel (coefficient 40 > 32 = 2^21 / 2^16)
    small = rng.integers(1, 7, (1, 64, 64, 3), dtype=np.uint8)
    s = co.statement_sums((small[..., [0, 0, 0]] * 40).astype(np.uint8), small, [af.IDENTITY])[0, 0]
    m, fitted = colour.matrix_of_sums(s)
    assert not fitted and np.array_equal(m, ident)
    s = co.statement_sums((small[..., [0, 0, 0]] * 32).astype(np.uint8), small, [af.IDENTITY])[0, 0]
    m, fitted = colour.matrix_of_sums(s)
    assert fitted and np.array_equal(m[:, 0], [32 * ONE] * 3) and not m[:, 1:].any() and co.legal(m)


def test_the_apply_rule_rounds_shifts_and_saturates():
    px = np.array([[[[0, 0, 0], [255, 255, 255], [1, 2, 3], [200, 100, 50]]]], np.uint8)
    big = np.asarray([[co.MAX_COEFF, co.MAX_COEFF, co.MAX_COEFF, co.MAX_OFFSET], [-co.MAX_COEFF, -co.MAX_COEFF, -co.MAX_COEFF, -co.MAX_OFFSET],
                      [-ONE, 0, 0, 32767]], np.int32)
    out = co.apply_colour(px, big)[0, 0]
    assert [list(p) for p in out] == [[255, 0, 0], [255, 0, 0], [255, 0, 0], [255, 0, 0]]       # -1 + 0.99998 + 0.5 floors to 0; below: 0
    half = np.asarray([[ONE, 0, 0, -32768], [ONE, 0, 0, -32769], [0, 0, -ONE, 3 * ONE + 32768]], np.int32)
    assert [list(p) for p in co.apply_colour(px, half)[0, 0]] == [[0, 0, 4], [255, 254, 0], [1, 0, 1], [200, 199, 0]]
    assert co.legal(big) and not co.legal(big + np.asarray([[1, 0, 0, 0]] * 3)) and not co.legal(big + np.asarray([[0, 0, 0, 1]] * 3))
    assert np.array_equal(co.apply_colour(px, co.IDENTITY_MATRIX), px)


@pytest.mark.parametrize("name", list(co.ATTACKS))
def test_a_colour_mapped_leak_is_misread_by_the_other_routes_and_read_with_the_matrix_fit(name):
    from offmark import colour, resync, tone
    clean = untouched()
    assert list(clean["picks"]) == [1, 0, 1] and clean["score"] > 8_000_000
    leak = co.colour_map(ap.leak("svd", "A"), *co.ATTACKS[name])
    plain = read(resync.read_registered_leak, leak)
    toned = read(tone.read_toned_leak, leak)
    got = read(colour.read_coloured_leak, leak)
    c = got["colour"]
    other = max(abs(plain["score"]), abs(toned["score"]))
    print(f"{name}: plain {[int(p) for p in plain['picks']]} {plain['score']} | toned {[int(p) for p in toned['picks']]} {toned['score']} | "
          f"matrix fit {[int(p) for p in got['picks']]} {got['score']} rms {got['registration']['rms']:.2f} "
          f"{resync.corner_move(got['geometry'], clean['geometry'], CANVAS):.3f} px; share of clean {got['score'] / clean['score']:.3f}, "
          f"ratio to the others {got['score'] / other:.2f}; pixels {c['pixels']} residual rms {c['residual_rms']:.2f} "
          f"matrix {(c['matrix'] / 65536.0).round(3).tolist()}")
    # The two comparisons with today's routes hold for the nine leaks whose colours changed.  Under the identity nothing was done to
    # the leak: both other routes read it (the table above: 8 682 833 and 6 467 733) and the fit costs 64 % of the score, so there the
    # comparisons cannot hold and only the fit's own conditions are asserted.
    if name != "identity":                                      # on record: today's routes do not both read the leak with a score that counts
        reads = [list(r["picks"]) == [1, 0, 1] and abs(r["score"]) >= 0.2 * clean["score"] for r in (plain, toned)]
        assert not all(reads)
    assert list(got["picks"]) == list(af.CHOSEN) == [1, 0, 1] and not got["ambiguous"] and got["registration"]["converged"] and c["fitted"]
    assert got["score"] > 0.2 * clean["score"]
    if name != "identity":
        assert got["score"] > 2 * other
    assert set(c) == {"lut0", "matrix", "fitted", "pixels", "residual_rms", "first_registration"}
    assert c["matrix"].shape == (3, 4) and c["matrix"].dtype == np.int32 and co.legal(c["matrix"]) and c["lut0"].shape == (3, 256)
    assert c["pixels"] >= 384 and 0.0 < c["residual_rms"] < 30.0 and c["first_registration"]["converged"]


def test_the_untouched_leak_still_reads_through_the_matrix_fit():
    from offmark import colour, resync
    got = read(colour.read_coloured_leak, ap.leak("svd", "A"))
    assert list(got["picks"]) == [1, 0, 1] and not got["ambiguous"] and got["registration"]["converged"] and got["colour"]["fitted"]
    assert resync.corner_move(got["geometry"], untouched()["geometry"], CANVAS) < 0.19
    m = got["colour"]["matrix"].astype(np.int64)
    assert (np.abs(m[:, :3] - np.eye(3, dtype=np.int64) * ONE) < ONE // 4).all()      # near the identity, not the identity


def test_an_unfitted_matrix_is_applied_as_the_identity_and_nothing_is_raised():
    from offmark import colour, resync
    # a leak whose first channel equals its second: collinear, so nothing is fitted and the call is read_registered_leak's
    grey = np.array(ap.leak("svd", "A"))
    grey[..., 0] = grey[..., 1]
    got = read(colour.read_coloured_leak, grey)
    want = read(resync.read_registered_leak, grey)
    assert not got["colour"]["fitted"] and np.array_equal(got["colour"]["matrix"], colour.identity())
    assert got["geometry"] == want["geometry"] and got["score"] == want["score"] and list(got["picks"]) == list(want["picks"])


def test_a_decoder_without_the_colour_calls_is_refused():
    import _tone as tn
    from offmark import colour
    with pytest.raises(ValueError, match="affine"):
        colour.read_coloured_leak(tn.StatementDecoder(), ap.leak("svd", "A"), rs.recipe_sources(), rs.recipe_segments(), CANVAS, rs.recipe_candidates(),
                                  key=af.KEY, L=af.L8, search_frames=ap.SEARCH_FRAMES)
