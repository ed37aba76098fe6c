"""Shared by the geometry-edge tests (test_geometry_edges_statement.py, test_gpu_geometry_edges.py): seeded families of maps at the
edges of what include/offmark_hip.h's ofmk_affine / ofmk_warp admit -- coefficients at +-2^20 (16 leak px per canvas px) in every sign
pattern, determinants at 2^24 (a 16 x magnification), positions exactly where the inside rule flips, offsets near 2^33 -- and the
leaks and canvases they are run on.  NumPy only; the seed is fixed, so every run and both test files see the same maps.

Every map is drawn with the canvas centre pixel (H // 2, W // 2) -- or, every other map, the pixel ``tile_corner`` -- landing on leak
sample (h // 2, w // 2) plus a random sub-pixel fraction, so that canvas pixels contribute; singular draws (|det| < 2^24) are drawn again, so every map passes affine_map_ok.  A
family is a list of 6-tuples (ayy, ayx, by, axy, axx, bx), the axis-aligned ones a list of 4-tuples (ay, by, ax, bx)."""
import functools

import numpy as np

ONE = 65536
MAX_A = 1 << 20                              # |coefficient| bound
MIN_A = 1 << 12                              # ofmk_warp's smallest scale
MIN_DET = 1 << 24
MAX_B = 1 << 48
SEED = 950

STEEP_LEAK, ODD_LEAK = (480, 480), (61, 83)
TINY_LEAKS = ((1, 3), (3, 1), (2, 3), (3, 2), (2, 2), (3, 83), (61, 2), (1, 83))
WIDE_LEAK, TALL_LEAK = (8, 36000), (36000, 8)           # samples past 32768: a Q16 position there no longer fits 32 bits
PHASE_WIDE_LEAK, PHASE_TALL_LEAK = (8, 9000), (9000, 8)  # for the shift search, whose reference takes 64 statement warps per map
CANVAS = (136, 200)                          # 2 x 2 search tiles, 3 x 4 align tiles, 5 x 7 phase rectangles, all with partial edges
SMALL_CANVAS = (72, 104)
LONG_CANVAS, FAR_X = (16, 8200), 8100        # the far family: only units near column 8100 count
ALIGN_LONG_CANVAS, ALIGN_FAR_X = (16, 4096), 4000      # the registration calls take canvases up to 4096
PHASE_LONG_CANVAS, PHASE_FAR_X = (8, 2600), 2500       # |b| above 2^31: still no int, and 64 statement warps of it stay quick
EDGE_COEFS = (MAX_A, MAX_A - 1)
PHASE_STEEPEST = (1, 3, 5, 7, 9, 11, 13, 15)        # the steepest maps the shift search is run on: anchored at tile_corner


def rng_of(*key):
    return np.random.default_rng([SEED, *key])


def noise(shape, *key):
    out = rng_of(*key).integers(0, 256, shape, dtype=np.uint8)
    out.setflags(write=False)
    return out


def det(g):
    ayy, ayx, _, axy, axx, _ = (int(v) for v in g)
    return ayy * axx - ayx * axy


def in_range(g):
    """ofmk_affine's rule, in Python integers."""
    ayy, ayx, by, axy, axx, bx = (int(v) for v in g)
    return all(abs(a) <= MAX_A for a in (ayy, ayx, axy, axx)) and abs(by) <= MAX_B and abs(bx) <= MAX_B and abs(det(g)) >= MIN_DET


def anchored(lin, at, target):
    """The map with linear part lin = (ayy, ayx, axy, axx) whose canvas pixel ``at`` = (y, x) has the Q16 position ``target``."""
    ayy, ayx, axy, axx = (int(v) for v in lin)
    y, x = at
    return ayy, ayx, int(target[0]) - ayy * y - ayx * x, axy, axx, int(target[1]) - axy * y - axx * x


def centred(lin, leak_hw, canvas_hw, rng, at=None):
    """Canvas pixel ``at`` (the canvas centre by default) -> leak centre plus a random sub-pixel fraction."""
    target = [((n // 2) << 16) + int(rng.integers(0, ONE)) for n in leak_hw]
    return anchored(lin, (canvas_hw[0] // 2, canvas_hw[1] // 2) if at is None else at, target)


def tile_corner(canvas_hw):
    """The middle of the canvas unit that ends at row and column 63 (mod 64) nearest the canvas centre: (124, 124) of 136 x 200,
    (60, 60) of 72 x 104.  A steep map has live pixels only around the pixel it is anchored at; anchored here, they sit in the far
    corner of a 64 x 64 tile and of a 32 x 32 rectangle of origins, where |q| is largest -- at the canvas centre of both canvases
    they sit at a tile's first rows, where q is small."""
    return tuple(60 + 64 * ((n // 2) // 64) for n in canvas_hw)


def _drawn(count, leak_hw, canvas_hw, rng, draw, corner=True):
    """``count`` maps from draw(k) -> lin, singular draws drawn again; anchored at the canvas centre and (``corner``) at tile_corner
    in turn, each under every k % 16."""
    out = []
    for k in range(count):
        at = tile_corner(canvas_hw) if corner and (k + k // 16) % 2 else None
        while True:
            g = centred(draw(k), leak_hw, canvas_hw, rng, at)
            if in_range(g):
                break
        out.append(g)
    return out


@functools.lru_cache(maxsize=None)
def steepest(count, leak_hw=STEEP_LEAK, canvas_hw=CANVAS):
    """Each coefficient is 2^20 or 2^20 - 1 (half of the draws) or uniform in [0, 2^20], under the sign pattern k % 16: all 16
    patterns appear from count = 16 on.  (With all four at the edge and an even number of minus signs on each diagonal pair the map
    is singular: such draws are drawn again.)"""
    rng = rng_of(1, count)

    def draw(k):
        return [(-1 if (k >> b) & 1 else 1) * (EDGE_COEFS[int(rng.integers(2))] if rng.random() < 0.5 else int(rng.integers(0, MAX_A + 1)))
                for b in range(4)]

    return _drawn(count, leak_hw, canvas_hw, rng, draw)


@functools.lru_cache(maxsize=None)
def uniform(count, leak_hw=STEEP_LEAK, canvas_hw=CANVAS):
    rng = rng_of(2, count)
    return _drawn(count, leak_hw, canvas_hw, rng, lambda k: [int(v) for v in rng.integers(-MAX_A, MAX_A + 1, 4)])


def _placed(big, small, off, k):
    """(ayy, ayx, axy, axx): k & 1 puts ``big`` on the x axis instead of y; k & 2 swaps the canvas axes (quarter-turn-like: the
    large terms are the off-diagonal ones)."""
    dy, dx = (small, big) if k & 1 else (big, small)
    return [off[0], dy, dx, off[1]] if k & 2 else [dy, off[0], off[1], dx]


@functools.lru_cache(maxsize=None)
def smallest_determinant(count, leak_hw=ODD_LEAK, canvas_hw=CANVAS):
    """One of the two large terms a in +-[2^12, 2^14), the other +-(2^24 // a + 1), the small ones in [-8, 8]: a magnification of
    about 16 in area, 4 to 16 x on one axis; both leak rows and columns repeat over many canvas pixels."""
    rng = rng_of(3, count)

    def draw(k):
        a = int(rng.integers(MIN_A, 1 << 14)) if k >= 4 else MIN_A             # the first four sit at 2^12 exactly
        s = [1 if rng.random() < 0.5 else -1 for _ in range(2)]
        return _placed(s[0] * a, s[1] * (MIN_DET // a + 1), [int(v) for v in rng.integers(-8, 9, 2)], k)

    return _drawn(count, leak_hw, canvas_hw, rng, draw)


@functools.lru_cache(maxsize=None)
def anisotropic(count, leak_hw=STEEP_LEAK, canvas_hw=CANVAS):
    """The pair (+-2^20, +-16), determinant 2^24 up to the small terms: 16 leak px per canvas px on one axis, 4096 canvas px per leak
    px on the other."""
    rng = rng_of(4, count)

    def draw(k):
        s = [1 if rng.random() < 0.5 else -1 for _ in range(2)]
        return _placed(s[0] * MAX_A, s[1] * 16, [int(v) for v in rng.integers(-8, 9, 2)], k)

    return _drawn(count, leak_hw, canvas_hw, rng, draw)


@functools.lru_cache(maxsize=None)
def tiny(leak_hw, canvas_hw=SMALL_CANVAS):
    """16 maps for a leak with a side of 1 to 3 px: large terms +-4096 or +-4097 in all four sign pairs, straight and with the axes
    swapped, small terms in [-8, 8].  16 canvas px per leak px, so units fill, and under the minus signs they run into the leak's
    last row and column from either side."""
    rng = rng_of(5, *leak_hw)

    def draw(k):
        mag = [MIN_A + int(rng.integers(2)) for _ in range(2)]
        return _placed((-1 if k & 4 else 1) * mag[0], (-1 if k & 8 else 1) * mag[1], [int(v) for v in rng.integers(-8, 9, 2)], k)

    return _drawn(16, leak_hw, canvas_hw, rng, draw, corner=False)               # the canvas centre: both ends of the leak are read


# ---- positions exactly where the inside rule flips --------------------------------------------------------------------------------
SIGNED_PERMUTATIONS = tuple([sy * ONE, 0, 0, sx * ONE] for sy in (1, -1) for sx in (1, -1)) + \
    tuple([0, sy * ONE, sx * ONE, 0] for sy in (1, -1) for sx in (1, -1))
PROBES = ((32, 48), (39, 55), (29, 43))      # a unit's first pixel, a unit's last pixel, neither


def flip_values(length):
    """(pos, inside) at the four positions where ``0 <= pos >> 16 <= length - 1`` changes."""
    return (-1, False), (0, True), (((length - 1) << 16) | 0xffff, True), (length << 16, False)


@functools.lru_cache(maxsize=None)
def _boundary(leak_hw):
    maps, probes = [], []
    for n, lin in enumerate(SIGNED_PERMUTATIONS):
        for axis in (0, 1):
            for v, (pos, inside) in enumerate(flip_values(leak_hw[axis])):
                at = PROBES[(n + axis + v) % 3]
                target = [((length // 2) << 16) + 0x8000 for length in leak_hw]      # the other axis: mid-leak, mid-pixel
                target[axis] = pos
                maps.append(anchored(lin, at, target))
                probes.append((at, axis, pos, inside))
    return maps, probes


def boundary(leak_hw):
    """64 maps with |coefficients| = 65536 (the 8 flips and turns): canvas pixel probe = (y, x) has, on one leak axis, exactly
    pos = -1, 0, ((len - 1) << 16) | 0xffff or len << 16, and its canvas neighbours the positions one leak pixel either side."""
    return _boundary(tuple(leak_hw))[0]


def boundary_probes(leak_hw):
    """Parallel to ``boundary``: ((y, x), axis, pos, inside) -- the probe pixel, the leak axis at its edge, the exact position there
    and whether the rule calls it inside."""
    return _boundary(tuple(leak_hw))[1]


# ---- large offsets and large base indices -----------------------------------------------------------------------------------------
def far_sample(leak_hw):
    """The sample on the leak's long axis that column x_star reads: 17 / 18 of the way along (34000 of 36000, 8500 of 9000)."""
    return max(leak_hw) * 17 // 18


@functools.lru_cache(maxsize=None)
def far(leak_hw, canvas_hw=LONG_CANVAS, x_star=FAR_X):
    """8 maps on a long canvas for a leak of 8 x 36000 (or 36000 x 8): the leak's long axis moves +-2^20 or +-(2^20 - 1) per canvas
    column, its short axis half a leak px per canvas row, and the offsets cancel a * x at column x_star, where the canvas reads leak
    sample far_sample(leak) = 34000 on the long axis: |b| is about 2^20 * x_star, only units within some 2200 columns of x_star
    count, and their positions run up to 36000.  The remaining two coefficients are a steep one (the long axis against canvas rows)
    and a small one (the short axis against canvas columns; over x_star columns it still adds up to tens of leak px, which the offset cancels)."""
    rng = rng_of(6, *leak_hw, *canvas_hw)
    wide = leak_hw[1] >= leak_hw[0]
    out = []
    for k in range(8):
        along = (-1 if k & 1 else 1) * EDGE_COEFS[(k >> 1) & 1]                # long leak axis per canvas column
        across = (-1 if k & 4 else 1) * (ONE // 2)                              # short leak axis per canvas row
        steep = int(rng.integers(-MAX_A, MAX_A + 1))                            # long leak axis per canvas row
        small = int(rng.integers(-1024, 1025))                                  # short leak axis per canvas column
        lin = [across, small, steep, along] if wide else [steep, along, across, small]
        short, long_ = (min(leak_hw) // 2 << 16) + int(rng.integers(0, ONE)), (far_sample(leak_hw) << 16) + int(rng.integers(0, ONE))
        g = anchored(lin, (canvas_hw[0] // 2, x_star), (short, long_) if wide else (long_, short))
        assert in_range(g)
        out.append(g)
    return out


# ---- the axis-aligned analogues, for ofmk_warp -------------------------------------------------------------------------------------
AXIS_SCALES = (MIN_A, MIN_A + 1, ONE - 1, ONE + 1, MAX_A - 1, MAX_A)


def centred4(ay, ax, leak_hw, canvas_hw, rng):
    g = centred([ay, 0, 0, ax], leak_hw, canvas_hw, rng)
    return g[0], g[2], g[4], g[5]


@functools.lru_cache(maxsize=None)
def axis_aligned(leak_hw=STEEP_LEAK, canvas_hw=CANVAS):
    """36 maps (ay, by, ax, bx): every pair of the scales 2^12, 2^12 + 1, 2^16 - 1, 2^16 + 1, 2^20 - 1, 2^20."""
    rng = rng_of(7, *leak_hw, *canvas_hw)
    return [centred4(ay, ax, leak_hw, canvas_hw, rng) for ay in AXIS_SCALES for ax in AXIS_SCALES]


@functools.lru_cache(maxsize=None)
def axis_aligned_far(canvas_hw=LONG_CANVAS, x_star=FAR_X):
    """4 maps for the wide far leak: 2^20 or 2^20 - 1 per column with the offset cancelling it at x_star, half a px or 2^12 per row."""
    rng = rng_of(8, *canvas_hw)
    out = []
    for ax in EDGE_COEFS:
        for ay in (ONE // 2, MIN_A):
            g = anchored([ay, 0, 0, ax], (canvas_hw[0] // 2, x_star), ((4 << 16) + int(rng.integers(0, ONE)), (far_sample(WIDE_LEAK) << 16) + int(rng.integers(0, ONE))))
            out.append((g[0], g[2], g[4], g[5]))
    return out


def out_of_range():
    """Maps one step past each bound of ofmk_affine: a coefficient, an offset, the determinant."""
    return [(MAX_A + 1, 0, 0, 0, ONE, 0), (ONE, 0, 0, -MAX_A - 1, ONE, 0), (ONE, 0, MAX_B + 1, 0, ONE, 0), (ONE, 0, 0, 0, ONE, -MAX_B - 1),
            (MIN_A, 0, 0, 0, MIN_A - 1, 0), (MAX_A, MAX_A, 0, MAX_A, MAX_A, 0)]


def out_of_range4():
    return [(MIN_A - 1, 0, ONE, 0), (ONE, 0, MAX_A + 1, 0), (ONE, MAX_B + 1, ONE, 0)]


def interleaved(maps, bad):
    """The maps with the out-of-range ones put between them: (list, indices of the good ones, indices of the bad ones)."""
    out = list(maps)
    for k, b in enumerate(bad):
        out.insert(min(len(out), 1 + k * max(1, len(maps) // len(bad))), b)
    bad_at = [k for k, g in enumerate(out) if any(g is b for b in bad)]
    return out, [k for k in range(len(out)) if k not in bad_at], bad_at


# ---- the cases of the registration calls and of everything else that walks align_kernels.hiph's 64 x 64 tile ---------------------
# (leak, canvas, maps), at most 16 maps each: test_gpu_geometry_edges.py (align_sums, align_residuals), test_gpu_value_edges.py
ALIGN_CASES = {
    "steepest": (STEEP_LEAK, CANVAS, steepest(64)[:16]), "uniform": (STEEP_LEAK, CANVAS, uniform(64)[:15]),
    "smallest-determinant": (ODD_LEAK, CANVAS, smallest_determinant(32)[::2]), "anisotropic": (STEEP_LEAK, CANVAS, anisotropic(16)[:12]),
    "boundary": (ODD_LEAK, SMALL_CANVAS, boundary(ODD_LEAK)[::5]),
    "boundary-1x83": ((1, 83), SMALL_CANVAS, boundary((1, 83))[1::5]), "boundary-61x2": ((61, 2), SMALL_CANVAS, boundary((61, 2))[2::5]),
    "boundary-3x3": ((3, 3), SMALL_CANVAS, boundary((3, 3))[3::5]), "tiny-3x2": ((3, 2), SMALL_CANVAS, tiny((3, 2))[:12]),
    "tiny-1x83": ((1, 83), SMALL_CANVAS, tiny((1, 83))[4:]),
    "far-wide": (WIDE_LEAK, ALIGN_LONG_CANVAS, far(WIDE_LEAK, ALIGN_LONG_CANVAS, ALIGN_FAR_X)),
    "far-tall": (TALL_LEAK, ALIGN_LONG_CANVAS, far(TALL_LEAK, ALIGN_LONG_CANVAS, ALIGN_FAR_X)),
}
RESIDUAL_MAPS = [("steepest", 0), ("steepest", 5), ("uniform", 3), ("smallest-determinant", 1), ("anisotropic", 2), ("boundary", 7), ("boundary-61x2", 9),
                 ("far-wide", 4), ("far-tall", 3)]


# ---- the mirror identity ------------------------------------------------------------------------------------------------------------
def mirrored(g, w):
    """The map that reads, in the leak mirrored left to right, the sample ``g`` reads in the leak: pos_x' = ((w - 1) << 16) - pos_x.
    The bilinear weights mirror exactly only where pos_x is a multiple of 256 (the weight drops the low 8 bits), and the inside rule
    is not symmetric in the leak's last column (pos_x in ((w - 1) << 16, w << 16) is inside, its mirror image is negative): see
    ``mirror_pairs``."""
    ayy, ayx, by, axy, axx, bx = (int(v) for v in g)
    return ayy, ayx, by, -axy, -axx, ((w - 1) << 16) - bx


def positions(g, out_hw, origin=(0, 0)):
    """(pos_y, pos_x), int64 [Hout, Wout]: ofmk_affine's rule."""
    ayy, ayx, by, axy, axx, bx = (int(v) for v in g)
    y = (np.arange(out_hw[0], dtype=np.int64) + origin[0])[:, None]
    x = (np.arange(out_hw[1], dtype=np.int64) + origin[1])[None, :]
    return ayy * y + ayx * x + by, axy * y + axx * x + bx


def inside(g, leak_hw, out_hw, origin=(0, 0)):
    py, px = positions(g, out_hw, origin)
    return (py >= 0) & ((py >> 16) <= leak_hw[0] - 1) & (px >= 0) & ((px >> 16) <= leak_hw[1] - 1)


@functools.lru_cache(maxsize=None)
def mirror_pairs(count, leak_hw=STEEP_LEAK, canvas_hw=CANVAS):
    """``count`` (g, mirrored g): steepest-style maps with every coefficient and offset rounded to a multiple of 256, kept only when no
    canvas pixel falls into the asymmetric last-column fraction, i.e. when both maps call the same canvas pixels inside.  Decided on
    the integer rule alone."""
    rng = rng_of(9, count)
    out = []
    k = 0
    while len(out) < count:
        lin = [(-1 if (k >> b) & 1 else 1) * (MAX_A if rng.random() < 0.5 else int(rng.integers(0, MAX_A + 1)) & ~255) for b in range(4)]
        k += 1
        g = tuple(v & ~255 if n in (2, 5) else v for n, v in enumerate(centred(lin, leak_hw, canvas_hw, rng)))
        m = mirrored(g, leak_hw[1])
        if in_range(g) and np.array_equal(inside(g, leak_hw, canvas_hw), inside(m, leak_hw, canvas_hw)):
            out.append((g, m))
    return out
