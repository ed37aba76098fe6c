"""CPU-only: registration of a leak to its source frames (offmark.resync.register_leak / read_registered_leak; build extensions) over
the NumPy statement of the alignment sums (tests/_align.py), on the rotated-and-cropped leaks of tests/_affine_phase.py and the
rotated-and-scaled leak of tests/_affine.py -- the first 4 frames, from the unrotated centred start, no list of geometries.

Measured on the statement (corner distance = the largest distance in leak pixels between the four canvas corners' samples under the
registered geometry and under the listed truth; |m| = sum |unit metric| per counting unit and frame):
  leak A     corner distance 0.103 px   |m| 12914 registered, 12122 listed truth, 10048 unmarked sources registered the same way
  leak B     corner distance 0.083 px   |m| 12572 / 12153 / 10159
  leak A2    |m| 12984 / 10195 / 10003.  Its listed entry, geometry("A2", 2.0) (+) (1, 2), carries leak A's translation -- A2 is cut at
             other rows and columns -- and lies 2.2 px from the registered geometry, so it holds the ranking only, no distance
  -3 degrees, step 1.10, from the UNROTATED start at scale 1: corner distance 0.016 px, |m| 12706 / 12636 / 10238
The score reaches the unmarked level 0.19 px from the exact translation (offmark/resync.py), the ceiling of every distance bound."""
import functools

import numpy as np
import pytest

import _affine as af
import _affine_phase as ap
import _align as al
import _resync as rs

N = ap.SEARCH_FRAMES
CANVAS = af.CANVAS
CASES = ("A", "A2", "B", "-3deg-step-1.10")
# the statement's measured corner distance to the listed truth (module docstring); None: the listed entry is not that leak's translation
MEASURED_PX = {"A": 0.103, "A2": None, "B": 0.083, "-3deg-step-1.10": 0.016}
CEILING_PX = 0.19


def frames_of(case, codec="svd"):
    return af.leak(codec, case) if case.startswith("-3deg") else ap.leak(codec, case)


def listed_truth(case):
    from offmark import resync
    if case.startswith("-3deg"):
        return resync.affine_of_rotation(CANVAS, CANVAS, *af.ATTACKS[case])
    return resync.shift_affine(ap.geometry(case, 2.0, 1.0, ap.LEAKS[case][2]), 1, 2)


@functools.lru_cache(maxsize=None)
def sources():
    s = rs.recipe_sources()
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def registered(case, codec="svd", start=None, levels=None):
    """register_leak's report from the default start (or ``start``, a tuple of six), shared by the tests."""
    from offmark import resync
    return resync.register_leak(al.StatementDecoder(), sources()[:N], frames_of(case, codec)[:N], CANVAS, start=start, levels=levels)


def per_unit(frames, geom):
    """sum |m| per counting unit and frame over the first N frames at ``geom``."""
    from offmark import resync
    units = int(resync.affine_units(frames.shape[1:3], CANVAS, geom).sum())
    return sum(af.statement_score(f, CANVAS, geom) for f in frames[:N]) / (units * N)


@pytest.mark.parametrize("case", CASES)
def test_a_leak_registers_from_the_unrotated_start_and_reads(case):
    from offmark import resync
    leak = frames_of(case)
    got = resync.read_registered_leak(al.StatementDecoder(), leak, sources(), rs.recipe_segments(), CANVAS, rs.recipe_candidates(), key=af.KEY,
                                      L=af.L8, search_frames=N)
    report = got["registration"]
    assert report == registered(case) and report["converged"] and report["reason"] is None and len(report["iterations"]) == 1
    assert list(got["picks"]) == list(af.CHOSEN) == [1, 0, 1] and got["base"] == 0 and not got["ambiguous"] and got["runner_up_score"] is None
    assert got["geometry"] == report["geometry"] and got["index"] == 0 and got["phase"] == (0, 0)
    assert set(got) >= {"index", "phase", "geometry", "normalised", "contrast", "phase_contrast", "segments", "soft_by_segment", "base", "picks",
                        "score", "runner_up_score", "ambiguous", "registration"}
    assert got["normalised"] == pytest.approx(per_unit(leak, report["geometry"]) / resync.ONE)


@pytest.mark.parametrize("case", CASES)
def test_the_registered_geometry_reads_a_stronger_mark_than_the_listed_truth_and_than_unmarked_sources(case):
    leak, unmarked = frames_of(case), frames_of(case, "none")
    here = per_unit(leak, registered(case)["geometry"])
    truth = per_unit(leak, listed_truth(case))
    none = per_unit(unmarked, registered(case, "none")["geometry"])
    print(f"{case}: |m| per unit and frame {here:.0f} registered, {truth:.0f} listed truth, {none:.0f} unmarked sources registered")
    assert registered(case, "none")["converged"]
    assert here >= truth
    assert here > none


@pytest.mark.parametrize("case", [c for c in CASES if MEASURED_PX[c] is not None])
def test_the_corner_distance_to_the_listed_truth(case):
    from offmark import resync
    d = resync.corner_move(registered(case)["geometry"], listed_truth(case), CANVAS)
    print(f"{case}: {d:.4f} px from the listed truth")
    assert d < min(2 * MEASURED_PX[case], CEILING_PX)


@pytest.mark.parametrize("shift", [(12, 10), (-16, 14)])
def test_the_basin_of_convergence_with_and_without_a_pyramid(shift):
    """One 2x halving brings starts 16-21 px off at the corners home; without it they stay away."""
    from offmark import resync
    home = registered("A")["geometry"]
    start = resync.shift_affine(resync.affine_of_rotation(CANVAS, ap.leak_hw("A"), 0.0), *shift)
    assert resync.corner_move(start, home, CANVAS) > 9.0
    two = registered("A", start=start, levels=2)
    assert two["converged"] and len(two["iterations"]) == 2 and all(0 < k <= 15 for k in two["iterations"])
    assert resync.corner_move(two["geometry"], home, CANVAS) <= 1 / 16
    one = registered("A", start=start, levels=1)
    assert resync.corner_move(one["geometry"], home, CANVAS) > 1 / 16


def test_level_maps_round_trip():
    from offmark import resync
    rng = np.random.default_rng(11)
    geoms = [resync.affine_of_rotation(CANVAS, (57, 91), a, s, (dy, dx)) for a, s, dy, dx in ((2.0, 1.0, 0.0, 0.0), (-3.0, 1.1, 0.5, 0.25), (91.0, 0.7, -3.3, 8.1))]
    geoms += [tuple(int(v) for v in rng.integers(-(1 << 20), 1 << 20, 6)) for _ in range(50)] + [af.hflip(91), af.IDENTITY]
    for g in geoms:
        down = resync.level_down(g)
        back = resync.level_up(down)
        assert down[0::3] == g[0::3] and down[1::3] == g[1::3] and back[0::3] == g[0::3] and back[1::3] == g[1::3]      # the linear part stays
        assert resync.corner_move(g, back, (4096, 4096)) <= 2.0 ** -15
        assert abs(back[2] - g[2]) <= 1 and abs(back[5] - g[5]) <= 1
    assert resync.level_down(af.IDENTITY) == af.IDENTITY and resync.level_up(af.IDENTITY) == af.IDENTITY


def test_a_levels_sums_use_the_level_map():
    """The sums of level 1 are the statement's on the halved frames under level_down of the geometry -- and that geometry samples the
    halved leak where the level map says: level-1 canvas pixel Q reads the level-0 geometry at 2 Q + 1/2, and the level-0 sample p
    is level-1 sample (p - 1/2) / 2, within the two roundings to Q16."""
    from offmark import resync
    g = registered("B")["geometry"]
    down = resync.level_down(g)
    src1, leak1 = al.halve(sources()[:2]), al.halve(ap.leak("svd", "B")[:2])
    assert src1.shape == (2, 36, 52, 3) and leak1.shape == (2, 28, 45, 3)
    for Q in ((0, 0), (35, 51), (17, 3)):
        for axis, (a, b, c) in enumerate((g[0:3], g[3:6])):
            direct = (a * (2 * Q[0] + 0.5) + b * (2 * Q[1] + 0.5) + c - 32768) / 2          # Q16, exact in float64
            mapped = down[3 * axis] * Q[0] + down[3 * axis + 1] * Q[1] + down[3 * axis + 2]
            assert abs(mapped - direct) <= 0.5
    # a direct warp where the answer is exact: a mirrored frame halves to the halved frame mirrored, so the flip of a 90-wide leak
    # must map to the flip of the 45-wide one (offset 44, not the 44.5 that halving the offset alone gives) byte for byte
    leak0 = ap.leak("svd", "A")[0]
    assert leak0.shape[:2] == (56, 90) and resync.level_down(af.hflip(90)) == af.hflip(45) and resync.level_up(af.hflip(45)) == af.hflip(90)
    mirrored, inside = af.warp(leak0, af.hflip(90), (56, 90))
    assert inside.all() and np.array_equal(mirrored, leak0[:, ::-1])
    assert np.array_equal(af.warp(al.halve(leak0[None])[0], resync.level_down(af.hflip(90)), (28, 45))[0], al.halve(mirrored[None])[0])
    want = al.statement_sums(src1, leak1, [down])
    got = al.StatementDecoder().align_sums_u8(src1, leak1, (36, 52), np.asarray([down]))
    assert np.array_equal(got, want) and want[:, 0, 28].min() > 1000
    # one more step at level 1 from there hardly moves: the level-0 fit is the level-1 fit
    nxt = resync.align_step(down, want, (36, 52))
    assert resync.corner_move(down, nxt, (36, 52)) < 0.25


def test_the_sums_of_one_pixel_by_hand():
    """A 9 x 11 canvas under the identity: the sums are those of a direct loop over the interior pixels."""
    rng = np.random.default_rng(5)
    src, leak = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8), rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    T, Yw = al.luma(src), al.luma(leak)
    want = [0] * 29
    for y in range(1, 8):
        for x in range(1, 10):
            gy, gx = int(T[y + 1, x] - T[y - 1, x]), int(T[y, x + 1] - T[y, x - 1])
            yc, xc, e = y - 4, x - 5, int(Yw[y, x] - T[y, x])
            sd = (gy * yc, gy * xc, gy, gx * yc, gx * xc, gx)
            k = 0
            for i in range(6):
                for j in range(i, 6):
                    want[k] += sd[i] * sd[j]
                    k += 1
            for i in range(6):
                want[21 + i] += sd[i] * e
            want[27] += e * e
            want[28] += 1
    assert al.sums(src, leak, af.IDENTITY).tolist() == want and want[28] == 63
    assert not al.sums(src, leak, (0, 0, 0, 0, 0, 0)).any()                      # out of range: 29 zeros


def test_a_flat_source_and_too_few_pixels_do_not_converge_and_raise_nothing():
    from offmark import resync
    dec = al.StatementDecoder()
    leak = ap.leak("svd", "A")[:N]
    flat = np.full((N, *CANVAS, 3), 90, np.uint8)
    got = resync.register_leak(dec, flat, leak, CANVAS)
    assert got["converged"] is False and "positive definite" in got["reason"] and got["iterations"] == [0]
    assert got["geometry"] == resync.affine_of_rotation(CANVAS, leak.shape[1:3], 0.0)
    # a leak of 12 x 16 pixels under the centred start: 192 canvas pixels per frame are inside, one frame
    tiny = np.ascontiguousarray(leak[:1, :12, :16])
    got = resync.register_leak(dec, sources()[:1], tiny, CANVAS)
    assert got["converged"] is False and "fewer than 384" in got["reason"] and got["iterations"] == [0] and got["pixels"] == 192
    with pytest.raises(resync.NoAlignStep):
        resync.align_step(af.IDENTITY, np.zeros(29, np.int64), CANVAS)
    # read_registered_leak hands the report on, and a decoder without the calls is refused
    out = resync.read_registered_leak(dec, np.repeat(tiny, 12, axis=0), sources(), rs.recipe_segments(), CANVAS, rs.recipe_candidates(), key=af.KEY,
                                      L=af.L8, search_frames=1)
    assert out["registration"]["converged"] is False

    class NoAffine:
        def decode_soft_warp_u8(self, *a):
            raise AssertionError

    with pytest.raises(ValueError, match="affine"):
        resync.read_registered_leak(NoAffine(), leak, sources()[:N], rs.recipe_segments()[:N], CANVAS, rs.recipe_candidates())


def test_default_levels():
    from offmark import resync
    assert [resync.default_levels(hw) for hw in ((56, 90), (95, 200), (96, 96), (1001, 1801), (1080, 1920))] == [1, 1, 2, 5, 5]
