"""CPU: the map families of tests/_geometry_edges.py do reach the edges they are named after, and the 32-bit arithmetic the warped
read-out kernels use relative to a tile's first pixel is the int64 rule of include/offmark_hip.h (ofmk_affine) there.

Coverage is a CONDITION on the statement (tests/_affine.py), per map, not a measurement: it is what keeps test_gpu_geometry_edges.py
from passing on units that never count.  The kernels' relative rule is written out again here in NumPy int32, which wraps like the
device's int: for the three tile extents -- 8 px (affine_unit_metric), 39 px (svd_affine_phase_scores_rgb8_kernel), 64 px
(align_sums_rgb8_kernel, align_residuals_rgb8_kernel) -- and the order in which each kernel adds the four coefficients up,
    yb = (int)(p0 >> 16)    q = (p0 & 65535) + r * a.y + c * a.x    sample yb + (q >> 16)    weight (q >> 8) & 255
equals pos >> 16 and (pos >> 8) & 255 of the int64 position at every pixel of every tile that survives the kernel's early-out, |q|
stays below 2^27, and the early-out (the tile's four corner positions) drops no tile that holds a pixel inside the leak."""
import numpy as np
import pytest

import _affine as af
import _geometry_edges as ge
import _warp as wp


def affine_cases():
    """(name, leak_hw, canvas_hw, maps): every affine family on the leak and canvas the GPU tests run it on."""
    out = [("steepest", ge.STEEP_LEAK, ge.CANVAS, ge.steepest(64)), ("uniform", ge.STEEP_LEAK, ge.CANVAS, ge.uniform(64)),
           ("smallest-determinant", ge.ODD_LEAK, ge.CANVAS, ge.smallest_determinant(32)), ("anisotropic", ge.STEEP_LEAK, ge.CANVAS, ge.anisotropic(16)),
           ("boundary", ge.ODD_LEAK, ge.SMALL_CANVAS, ge.boundary(ge.ODD_LEAK)),
           ("far-wide", ge.WIDE_LEAK, ge.LONG_CANVAS, ge.far(ge.WIDE_LEAK)), ("far-tall", ge.TALL_LEAK, ge.LONG_CANVAS, ge.far(ge.TALL_LEAK)),
           ("far-wide-4096", ge.WIDE_LEAK, ge.ALIGN_LONG_CANVAS, ge.far(ge.WIDE_LEAK, ge.ALIGN_LONG_CANVAS, ge.ALIGN_FAR_X)),
           ("far-tall-4096", ge.TALL_LEAK, ge.ALIGN_LONG_CANVAS, ge.far(ge.TALL_LEAK, ge.ALIGN_LONG_CANVAS, ge.ALIGN_FAR_X)),
           ("far-wide-2600", ge.PHASE_WIDE_LEAK, ge.PHASE_LONG_CANVAS, ge.far(ge.PHASE_WIDE_LEAK, ge.PHASE_LONG_CANVAS, ge.PHASE_FAR_X)),
           ("far-tall-2600", ge.PHASE_TALL_LEAK, ge.PHASE_LONG_CANVAS, ge.far(ge.PHASE_TALL_LEAK, ge.PHASE_LONG_CANVAS, ge.PHASE_FAR_X)),
           ("mirror", ge.STEEP_LEAK, ge.CANVAS, [g for pair in ge.mirror_pairs(8) for g in pair])]
    out += [(f"tiny-{h}x{w}", (h, w), ge.SMALL_CANVAS, ge.tiny((h, w))) for h, w in ge.TINY_LEAKS]
    out += [(f"boundary-{h}x{w}", (h, w), ge.SMALL_CANVAS, ge.boundary((h, w))) for h, w in ((1, 83), (61, 2), (3, 3))]
    out += [(f"axis-{n}", leak, canvas, [(ay, 0, by, 0, ax, bx) for ay, by, ax, bx in maps])
            for n, leak, canvas, maps in (("steep", ge.STEEP_LEAK, ge.CANVAS, ge.axis_aligned()), ("odd", ge.ODD_LEAK, ge.CANVAS, ge.axis_aligned(ge.ODD_LEAK)),
                                          ("far", ge.WIDE_LEAK, ge.LONG_CANVAS, ge.axis_aligned_far()))]
    return out


CASES = affine_cases()
IDS = [c[0] for c in CASES]


# ---- 1. the families are what they say ----------------------------------------------------------------------------------------------
def test_every_map_is_in_range_and_the_seed_is_fixed():
    from offmark import resync
    for name, _, _, maps in CASES:
        for g in maps:
            assert len(g) == 6 and ge.in_range(g) and resync._affine_ok(g), (name, g)
    for g in ge.out_of_range():
        assert not ge.in_range(g) and not resync._affine_ok(g), g
    for ay, by, ax, bx in ge.axis_aligned() + ge.axis_aligned_far():
        assert ge.MIN_A <= ay <= ge.MAX_A and ge.MIN_A <= ax <= ge.MAX_A and abs(by) <= ge.MAX_B and abs(bx) <= ge.MAX_B
    ge.steepest.cache_clear()
    again = ge.steepest(64)
    assert again == ge.steepest(64) and again == CASES[0][3]
    signs = {tuple(int(np.sign(g[n])) for n in (0, 1, 3, 4)) for g in ge.steepest(64)}
    assert len({s for s in signs if 0 not in s}) == 16                          # all sign patterns
    at_edge = sum(abs(g[n]) in ge.EDGE_COEFS for g in ge.steepest(64) for n in (0, 1, 3, 4))
    assert at_edge >= 64                                                        # a quarter of the coefficients or more sit at +-2^20 or one below
    for g in ge.smallest_determinant(32) + ge.anisotropic(16):
        assert ge.MIN_DET <= abs(ge.det(g)) < ge.MIN_DET + (1 << 15), g
    assert all(max(abs(g[2]), abs(g[5])) > 1 << 32 for g in ge.far(ge.WIDE_LEAK) + ge.far(ge.TALL_LEAK))


@pytest.mark.parametrize("family", ["steepest", "uniform"])
def test_steep_maps_have_counting_units_and_units_that_do_not_count(family):
    _, leak, canvas, maps = CASES[IDS.index(family)]
    partly = 0
    for g in maps:
        mask = af.units(leak, canvas, g)
        inner = ge.inside(g, leak, canvas)[1:-1, 1:-1]                         # the pixels that contribute to the alignment sums
        assert mask.sum() >= 1 and inner.sum() >= 16, (g, int(mask.sum()), int(inner.sum()))
        partly += not mask.all()
    assert partly >= 0.9 * len(maps), partly


@pytest.mark.parametrize("family", ["far-wide", "far-tall", "far-wide-4096", "far-tall-4096", "far-wide-2600", "far-tall-2600", "axis-far"])
def test_far_maps_count_units_whose_positions_are_in_the_thousands(family):
    _, leak, canvas, maps = CASES[IDS.index(family)]
    axis = 0 if leak[0] > leak[1] else 1
    for g in maps:
        mask = af.units(leak, canvas, g)
        pos = ge.positions(g, canvas)[axis]
        first = (pos[::8, ::8] >> 16)[:mask.shape[0], :mask.shape[1]]            # the position of each unit's first pixel
        assert (mask & (first >= 4096)).sum() >= 1 and not mask.all(), g
        assert max(leak) < 32768 or (mask & (first >= 32768)).sum() >= 1, g     # the long leaks: a counting unit whose Q16 position is past 2^31
        assert abs(int(pos[0, 0])) >> 16 > 25000 and max(abs(g[2]), abs(g[5])) > 1 << 30      # the first tiles are far outside the leak
    assert any(max(abs(g[2]), abs(g[5])) > 1 << 31 for g in maps)               # offsets that fit no int


@pytest.mark.parametrize("leak", [ge.ODD_LEAK, (1, 83), (61, 2), (3, 3)])
def test_boundary_maps_put_canvas_pixels_on_both_sides_of_the_flip(leak):
    canvas = ge.SMALL_CANVAS
    for g, ((y, x), axis, pos, is_in) in zip(ge.boundary(leak), ge.boundary_probes(leak)):
        p = ge.positions(g, canvas)
        assert int(p[axis][y, x]) == pos and pos in [v for v, _ in ge.flip_values(leak[axis])]
        mask = ge.inside(g, leak, canvas)
        around = {bool(mask[y + dy, x + dx]) for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1))}
        assert bool(mask[y, x]) == is_in and (not is_in) in around, (g, y, x)
        # the statement's warp sees the same pixels inside
        assert np.array_equal(af.warp(np.zeros((*leak, 3), np.uint8), g, canvas)[1], mask)


@pytest.mark.parametrize("leak", ge.TINY_LEAKS)
def test_tiny_leaks_fill_units_and_are_read_at_their_last_row_and_column(leak):
    counting = 0
    for g in ge.tiny(leak):
        mask = af.units(leak, ge.SMALL_CANVAS, g)
        counting += bool(mask.any())
        py, px = ge.positions(g, ge.SMALL_CANVAS)
        ok = ge.inside(g, leak, ge.SMALL_CANVAS)
        for pos, side in ((py, leak[0]), (px, leak[1])):                        # the short sides: first and last sample both read
            assert side > 3 or {0, side - 1} <= set((pos >> 16)[ok].tolist()), (g, side)
        assert ok.any() and not ok.all()
    assert counting >= 8, counting


def test_axis_aligned_maps_cover_every_pair_of_scales_and_count_units():
    assert {(g[0], g[2]) for g in ge.axis_aligned()} == {(a, b) for a in ge.AXIS_SCALES for b in ge.AXIS_SCALES}
    for leak in (ge.STEEP_LEAK, ge.ODD_LEAK):
        rects = [wp.units(leak, ge.CANVAS, g) for g in ge.axis_aligned(leak)]
        assert sum(r[1] > r[0] for r in rects) >= (36 if leak == ge.STEEP_LEAK else 16)
    # a magnification where both leak rows repeat over many canvas rows of a taller leak, and the steepest step
    g = ge.axis_aligned()[0]
    assert g[0] == ge.MIN_A and len(set(((g[0] * np.arange(136) + g[1]) >> 16).tolist())) <= 10
    assert ge.axis_aligned()[-1][0] == ge.MAX_A


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_four_corner_unit_rule_is_the_per_pixel_rule(case):
    _, leak, canvas, maps = case
    for g in maps:
        assert np.array_equal(af.corner_units(leak, canvas, g), af.units(leak, canvas, g)), g


def test_mirror_pairs_read_the_same_bytes_in_the_mirrored_leak():
    frame = ge.noise((*ge.STEEP_LEAK, 3), 20)
    for g, m in ge.mirror_pairs(8):
        a, inside_a = af.warp(frame, g, ge.CANVAS)
        b, inside_b = af.warp(np.ascontiguousarray(frame[:, ::-1]), m, ge.CANVAS)
        assert np.array_equal(a, b) and np.array_equal(inside_a, inside_b) and a.any()
        assert af.units(ge.STEEP_LEAK, ge.CANVAS, g).any()


# ---- 2. the kernels' relative rule in int32 -------------------------------------------------------------------------------------------
I32 = np.int32


def steps(n, a):
    """0, a, 2a, ... (n terms) by repeated int32 addition, as a kernel's ``q += a`` per row or column."""
    return np.concatenate([np.zeros(1, I32), np.cumsum(np.full(n - 1, a, I32), dtype=I32)])


def times(n, a):
    """The same by int32 multiplication, as ``dy * a``."""
    return np.arange(n, dtype=I32) * I32(a)


def relative_positions(g, Y0, X0, E, order):
    """What a kernel computes for the E x E pixels of the tiles whose first pixels are (Y0[t], X0[t]): the sample indices and
    weights (iy, fy, ix, fx), int32 [T, E, E], and q itself.  ``order``: how the kernel adds the increments up --
    "unit"   affine_unit_metric: q_row += a.y per canvas row, q += a.x per canvas column
    "phase"  the phase kernel's staging loop and its corner test: q0 + dy * a.y + dx * a.x
    "align"  align_sums / align_residuals: a wavefront starts at q0 + r0 * a.y + c * a.x (r0 = 0, 16, 32, 48) and adds a.y per row"""
    ayy, ayx, by, axy, axx, bx = (int(v) for v in g)
    p0y, p0x = ayy * Y0 + ayx * X0 + by, axy * Y0 + axx * X0 + bx              # int64
    out = []
    for p0, a_row, a_col in ((p0y, ayy, ayx), (p0x, axy, axx)):
        base = (p0 >> 16).astype(I32)                                           # the kernel's (int) cast
        q0 = (p0 & 0xffff).astype(I32)[:, None, None]
        if order == "unit":
            q = q0 + steps(E, a_row)[None, :, None] + steps(E, a_col)[None, None, :]
        elif order == "phase":
            q = q0 + times(E, a_row)[None, :, None] + times(E, a_col)[None, None, :]
        else:
            r0 = (np.arange(E, dtype=I32) // 16) * 16
            q = q0 + (r0 * I32(a_row))[None, :, None] + times(E, a_col)[None, None, :] + np.tile(steps(16, a_row), E // 16)[None, :, None]
        assert q.dtype == I32
        out += [base[:, None, None] + (q >> 16), (q >> 8) & 255, q]
    return out


def tiles_of(canvas, kernel):
    """(Y0, X0, Y1, X1, E, order) of every tile of a kernel: first pixels, the far corner its early-out looks at, extent, order."""
    H, W = canvas
    if kernel == "scores":                                                     # 16 x 16 units; the arithmetic runs per unit
        rows, cols = H // 8, W // 8
        i, j = np.meshgrid(np.arange(0, rows, 16), np.arange(0, cols, 16), indexing="ij")
        i, j = i.reshape(-1), j.reshape(-1)
        return 8 * i, 8 * j, 8 * (np.minimum(i + 16, rows) - 1) + 7, 8 * (np.minimum(j + 16, cols) - 1) + 7, 128, None
    if kernel == "phase":
        oh, ow = 8 * (H // 8), 8 * (W // 8)
        y, x = np.meshgrid(np.arange(0, oh, 32), np.arange(0, ow, 32), indexing="ij")
        y, x = y.reshape(-1), x.reshape(-1)
        return y, x, np.minimum(y + 32, oh) + 6, np.minimum(x + 32, ow) + 6, 39, "phase"
    y, x = np.meshgrid(np.arange(0, H, 64), np.arange(0, W, 64), indexing="ij")
    y, x = y.reshape(-1), x.reshape(-1)
    return y, x, np.minimum(y + 64, H) - 1, np.minimum(x + 64, W) - 1, 64, "align"


def dropped(g, leak, Y0, X0, Y1, X1):
    """The kernels' early-out: the four corner positions all beyond the same edge of the leak (affine_max4 / affine_min4)."""
    ayy, ayx, by, axy, axx, bx = (int(v) for v in g)
    cy = np.stack([(ayy * y + ayx * x + by) >> 16 for y in (Y0, Y1) for x in (X0, X1)])
    cx = np.stack([(axy * y + axx * x + bx) >> 16 for y in (Y0, Y1) for x in (X0, X1)])
    return (cy.max(axis=0) < 0) | (cy.min(axis=0) > leak[0] - 1) | (cx.max(axis=0) < 0) | (cx.min(axis=0) > leak[1] - 1)


def int64_rule(g, Y0, X0, E):
    ayy, ayx, by, axy, axx, bx = (int(v) for v in g)
    y = Y0[:, None, None] + np.arange(E, dtype=np.int64)[None, :, None]
    x = X0[:, None, None] + np.arange(E, dtype=np.int64)[None, None, :]
    return ayy * y + ayx * x + by, axy * y + axx * x + bx


def check_tiles(g, leak, Y0, X0, E, order, bound):
    """Every pixel of the given tiles: the int32 rule equals the int64 rule, and |q| < bound."""
    Y0, X0 = Y0.astype(np.int64), X0.astype(np.int64)
    py, px = int64_rule(g, Y0, X0, E)
    iy, fy, qy, ix, fx, qx = relative_positions(g, Y0, X0, E, order)
    assert np.array_equal(iy, py >> 16) and np.array_equal(fy, (py >> 8) & 255), g
    assert np.array_equal(ix, px >> 16) and np.array_equal(fx, (px >> 8) & 255), g
    for q, p in ((qy, py), (qx, px)):
        true_q = p - ((p[:, :1, :1] >> 16) << 16)
        assert np.array_equal(q, true_q) and np.abs(true_q).max() < bound, (g, int(np.abs(true_q).max()))
    return max(int(np.abs(qy).max()), int(np.abs(qx).max()))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_32_bit_relative_rule_is_the_int64_rule(case):
    name, leak, canvas, maps = case
    worst = {8: 0, 39: 0, 64: 0}
    for g in maps:
        mask = ge.inside(g, leak, (canvas[0] + 8, canvas[1] + 8))              # canvas coordinates are an index space: the phase kernel reads up to 7 px past it
        # the early-outs: a dropped tile holds no pixel inside the leak
        for kernel in ("scores", "phase", "align"):
            Y0, X0, Y1, X1, E, order = tiles_of(canvas, kernel)
            out = dropped(g, leak, Y0, X0, Y1, X1)
            for t in np.flatnonzero(out):
                assert not mask[Y0[t]:Y1[t] + 1, X0[t]:X1[t] + 1].any(), (kernel, g, int(Y0[t]), int(X0[t]))
            if order is not None and (~out).any():
                worst[E] = max(worst[E], check_tiles(g, leak, Y0[~out], X0[~out], E, order, 1 << 27))
        # affine_unit_metric runs on counting units only: 8 x 8 pixels from the unit's first one, |q| < 2^24
        units = af.corner_units(leak, canvas, g)
        if units.any():
            i, j = np.nonzero(units)
            worst[8] = max(worst[8], check_tiles(g, leak, 8 * i, 8 * j, 8, "unit", 1 << 24))
            Y0, X0, Y1, X1, _, _ = tiles_of(canvas, "scores")
            out = dropped(g, leak, Y0, X0, Y1, X1)
            tile = (i // 16) * ((canvas[1] // 8 + 15) // 16) + j // 16
            assert not out[tile].any(), g
    print(f"{name}: largest |q| per extent {worst}")
    if name == "steepest":
        # the bound the kernels' comments state is nearly reached: 65535 + 2 * 63 * 2^20 = 132 186 111 against 2^27 = 134 217 728
        assert worst[64] > 100_000_000 and worst[39] > 60_000_000 and worst[8] > 10_000_000


def test_steep_maps_have_live_pixels_where_q_is_largest():
    """A device test sees only pixels that contribute.  Among the steepest maps some have, in a 64 x 64 tile, a contributing pixel
    and, in a 39 x 39 rectangle, a pixel of a counting unit whose |q| is above 2^26, half the stated bound: a kernel that is wrong
    in the top bit of q's range changes a sum or a score."""
    _, leak, canvas, maps = CASES[IDS.index("steepest")]
    H8, W8 = canvas[0] // 8, canvas[1] // 8
    worst = {39: [], 64: []}
    for g in maps:
        ayy, ayx, by, axy, axx, bx = g
        grown = ge.inside(g, leak, (canvas[0] + 8, canvas[1] + 8))
        live = grown[:canvas[0], :canvas[1]].copy()                            # the pixels that contribute to the alignment sums
        live[[0, -1]] = False
        live[:, [0, -1]] = False

        def largest(y, x, Y0, X0):
            q = [((a_row * Y0 + a_col * X0 + b) & 0xffff) + (y - Y0) * a_row + (x - X0) * a_col for a_row, a_col, b in ((ayy, ayx, by), (axy, axx, bx))]
            return int(np.abs(np.stack(q)).max())

        y, x = np.nonzero(live)
        worst[64].append(largest(y, x, y // 64 * 64, x // 64 * 64))
        most = 0
        for py in range(8):                                                     # the units that count under each of the 64 shifts
            for px in range(8):
                i, j = np.nonzero(grown[py:py + 8 * H8, px:px + 8 * W8].reshape(H8, 8, W8, 8).all(axis=(1, 3)))
                oy, ox = py + 8 * i, px + 8 * j                                 # their origins; q is affine: its extremes are at the unit's corners
                for cy in (0, 7):
                    for cx in (0, 7):
                        most = max(most, largest(oy + cy, ox + cx, oy // 32 * 32, ox // 32 * 32)) if len(i) else most
        worst[39].append(most)
    print(f"largest |q| at a live pixel: 64 px {max(worst[64])}, 39 px {max(worst[39])}")
    assert max(worst[64]) > 120_000_000 and max(worst[39]) > 1 << 26, worst
    # the maps the device's shift search is run on (test_gpu_geometry_edges.py: PHASE_CASES) include such ones
    assert sum(worst[39][k] > 1 << 26 for k in ge.PHASE_STEEPEST) >= 2 and sum(worst[64][k] > 1 << 26 for k in range(16)) >= 4, (worst[39], worst[64][:16])


def test_the_largest_q_of_each_extent_stays_below_the_stated_bounds():
    """The worst case in closed form: a fraction of 65535 and both coefficients at 2^20 with the same sign."""
    for extent, bound in ((8, 1 << 24), (39, 1 << 27), (64, 1 << 27)):
        worst = 65535 + 2 * (extent - 1) * ge.MAX_A
        assert worst < bound, (extent, worst)
        g = (ge.MAX_A, ge.MAX_A, 65535, ge.MAX_A - 1, -ge.MAX_A, 65535)
        order = {8: "unit", 39: "phase", 64: "align"}[extent]
        assert check_tiles(g, (1, 1), np.zeros(1, np.int64), np.zeros(1, np.int64), extent, order, bound) == worst
    assert 65535 + 2 * 63 * ge.MAX_A == 132_186_111
