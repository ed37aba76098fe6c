"""Shared by the value-edge tests (test_value_edges_statement.py, test_gpu_value_edges.py): the inputs on which the tone, colour and
moment kernels (csrc/tone_kernels.hiph, colour_kernels.hiph, temporal_kernels.hiph's align_moments) meet the logic they add after the
tap -- seeded, read-only, NumPy only.

  edge cases   tests/_geometry_edges.py's twelve ALIGN_CASES with its out-of-range maps interleaved, on three kinds of leak: noise,
               bytes drawn from {0, 1, 254, 255} (under integer taps the warped bytes are those four and colour_sums' clip predicate
               flips from pixel to pixel; under fractional taps they cover everything between) and noise clipped to 1..254 (a bilinear
               mean of such bytes stays in 1..254: colour_sums drops nothing, so its sums are sums over tone_sums' bins).
  structured   content for tone_sums' per-lane runs and its wavefront path.  Under the identity or a whole-pixel shift a lane is a
               canvas column mod 64 and a step a canvas row mod 16: stripes, checkerboards, a staircase of run lengths 1..16, flat tiles
               with one or two differing lanes, leaks 1, 2 and 63 px wide.  Every channel of every frame has its own pattern and its own
               two values, 0 and 255 among them, so a mix-up of the 256 * ch bin base shows.
  histogram    frames whose four-pixel groups run through all eight neighbour-equality patterns (b1 == b0, b2 == b1, b3 == b2) in every
               channel, ABAB among them.
  the cube     all 2^24 RGB triples as one run of pixels.

The statements are tests/_tone.py's, _colour.py's and _toned_clip.py's, unchanged; they are computed once per case and shared."""
import functools

import numpy as np

import _colour as co
import _geometry_edges as ge
import _tone as tn
import _toned_clip as tc

ONE = ge.ONE
N = 2
IDENTITY = (ONE, 0, 0, 0, ONE, 0)
KINDS = ("noise", "extreme", "in-range")
EXTREME_BYTES = (0, 1, 254, 255)
LIBRARY_FRAMES = 12


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


# ---- 1. the edge cases --------------------------------------------------------------------------------------------------------------
def extreme(shape, *key):
    """u8 ``shape``, every byte drawn uniformly from {0, 1, 254, 255}; keyed like ge.noise."""
    return _frozen(np.asarray(EXTREME_BYTES, np.uint8)[ge.rng_of(*key).integers(0, 4, shape)])


def in_range(shape, *key):
    """u8 ``shape``, uniform in 1..254."""
    return _frozen(ge.rng_of(*key).integers(1, 255, shape, dtype=np.uint8))


# A 3 x 2 leak has six bytes per channel and frame and most taps blend two of them: the first draw leaves one of the bins 0, 1, 254, 255
# of a channel empty over the whole case (test_value_edges_statement.py's condition), so that leak is drawn again, with one more key.
REDRAWN = {(3, 2): (4,)}


@functools.lru_cache(maxsize=None)
def leak(kind, hw):
    """u8 [N, h, w, 3].  The noise leak is test_gpu_geometry_edges.py's."""
    shape = (N, *hw, 3)
    return {"noise": lambda: ge.noise(shape, 30, *hw), "extreme": lambda: extreme(shape, 31, *hw, *REDRAWN.get(tuple(hw), ())),
            "in-range": lambda: in_range(shape, 32, *hw)}[kind]()


@functools.lru_cache(maxsize=None)
def sources(canvas):
    return ge.noise((N, *canvas, 3), 40, *canvas)


@functools.lru_cache(maxsize=None)
def library(canvas):
    return ge.noise((LIBRARY_FRAMES, *canvas, 3), 50, *canvas)


@functools.lru_cache(maxsize=None)
def edge_cands(case):
    """(candidates, indices of the in-range ones, indices of the out-of-range ones): the case's maps with two out-of-range maps put
    between them, as test_gpu_geometry_edges.py's align_sums case has them."""
    return ge.interleaved(ge.ALIGN_CASES[case][2], ge.out_of_range()[4:])


@functools.lru_cache(maxsize=None)
def edge_tone(case, kind):
    """int64 [N, K, 3, 256, 2], read-only."""
    leak_hw, canvas, _ = ge.ALIGN_CASES[case]
    return _frozen(tn.statement_sums(sources(canvas), leak(kind, leak_hw), edge_cands(case)[0]))


@functools.lru_cache(maxsize=None)
def edge_colour(case, kind):
    """int64 [N, K, 28], read-only."""
    leak_hw, canvas, _ = ge.ALIGN_CASES[case]
    return _frozen(co.statement_sums(sources(canvas), leak(kind, leak_hw), edge_cands(case)[0]))


# a map of every case for the moments: ge.RESIDUAL_MAPS, and one of each case that list leaves out
MOMENT_MAPS = list(ge.RESIDUAL_MAPS) + [(case, 1) for case in ge.ALIGN_CASES if case not in {c for c, _ in ge.RESIDUAL_MAPS}]
MOMENT_WINDOWS = {1: (0, LIBRARY_FRAMES - 1), 16: (-3, 5)}        # span -> first[]: at span 16 both windows leave the 12 frames


@functools.lru_cache(maxsize=None)
def edge_moments(case, k, kind, span):
    """int64 [N, span, 6], read-only."""
    leak_hw, canvas, maps = ge.ALIGN_CASES[case]
    return _frozen(tc.moments(library(canvas), leak(kind, leak_hw), MOMENT_WINDOWS[span], span, maps[k]))


# ---- 2. structured content ------------------------------------------------------------------------------------------------------------
CANVASES = ((72, 104), (130, 130))           # the smallest with partial last tiles on both axes: 2 x 2 and 3 x 3 tiles of 64 x 64
PALETTE = ((0, 200), (3, 255), (128, 254))   # (even band, odd band) per channel: colour_sums keeps a pixel of (200, 3, 128 or 254) only.
# Channel c has its bands c px later (checkerboards: c down, 2 c right), so the channels change value at different steps and lanes and a
# band's first row or column is kept.
STAIR_PALETTE = ((0, 255), (255, 0), (1, 254))
ROW_PERIODS = (1, 2, 3, 5, 15, 16, 17)       # 15, 16, 17 cross a wavefront's 16-row block
COLUMN_PERIODS = (1, 2, 63, 64, 65)
CHECKER_CELLS = (1, 3, 16)
LANE_COLUMNS = (0, 31, 63, 64)               # a tile's first lane, a middle one, its last, and the next tile's first
FLAT, OTHER, THIRD = (100, 1, 254), (0, 255, 100), (255, 0, 1)
LANE_ROWS, PAIR_ROWS, PAIR_COLUMNS = (5, 20, 37), (7, 23, 50), (10, 40)       # per channel: other wavefronts
THIN_WIDTHS = (1, 2, 63)
THIN_FLAT = ((0, 255, 9), (1, 254, 200))        # two frames: every pixel clipped for colour_sums, and none
SHIFT_X, SHIFT_Y = -(5 << 16), -(3 << 16)


def _two_valued(fn, hw, palette=PALETTE):
    """fn(y, x, c) -> band parity; channel c shows palette[c][parity]."""
    y, x = np.mgrid[:hw[0], :hw[1]]
    return np.stack([np.asarray(palette[c], np.uint8)[fn(y, x, c) % 2] for c in range(3)], axis=-1)


def row_stripes(p, hw):
    return _two_valued(lambda y, x, c: (y - c) // p, hw)


def column_stripes(p, hw):
    return _two_valued(lambda y, x, c: (x - c) // p, hw)


def checkerboard(p, hw):
    return _two_valued(lambda y, x, c: (y - c) // p + (x - 2 * c) // p, hw)


def staircase(hw):
    """Channel 0 is (y // (1 + x % 16)) % 2 * 255: down column x the value changes every 1 + x % 16 rows, so the runs of the 16 lanes
    x % 16 = 0..15 have the lengths 1..16 and end at different rows; channels 1 and 2 the same with the columns moved and reversed."""
    return _two_valued(lambda y, x, c: y // (1 + (x + 5 * c) % 16 if c < 2 else 16 - x % 16), hw, STAIR_PALETTE)


def _flat(hw):
    return np.broadcast_to(np.asarray(FLAT, np.uint8), (*hw, 3)).copy()


def one_lane(hw):
    """[(frame, stated)]: the flat frame with one differing pixel per channel in tile column ``col`` (at rows LANE_ROWS), and with
    that whole column differing; ``stated`` is the bool [h, w, 3] mask of the bytes that differ from flat."""
    out = []
    for col in LANE_COLUMNS:
        for whole in (False, True):
            f, stated = _flat(hw), np.zeros((*hw, 3), bool)
            for c in range(3):
                rows = slice(None) if whole else LANE_ROWS[c]
                f[rows, col, c] = OTHER[c]
                stated[rows, col, c] = True
            out.append((f, stated))
    return out


def two_lanes(hw):
    """[(frame, stated)]: two differing pixels in one row per channel, of the same value and of two values."""
    out = []
    for second in (OTHER, THIRD):
        f, stated = _flat(hw), np.zeros((*hw, 3), bool)
        for c in range(3):
            f[PAIR_ROWS[c], PAIR_COLUMNS[0], c], f[PAIR_ROWS[c], PAIR_COLUMNS[1], c] = OTHER[c], second[c]
            stated[PAIR_ROWS[c], PAIR_COLUMNS, c] = True
        out.append((f, stated))
    return out


FAMILIES = {
    "row-stripes": lambda hw: [row_stripes(p, hw) for p in ROW_PERIODS],
    "column-stripes": lambda hw: [column_stripes(p, hw) for p in COLUMN_PERIODS],
    "checkerboards": lambda hw: [checkerboard(p, hw) for p in CHECKER_CELLS],
    "staircase": lambda hw: [staircase(hw)],
    "one-lane": lambda hw: [f for f, _ in one_lane(hw)],
    "two-lanes": lambda hw: [f for f, _ in two_lanes(hw)],
    **{f"thin-{w}": (lambda hw, w=w: [np.broadcast_to(np.asarray(v, np.uint8), (hw[0], w, 3)) for v in THIN_FLAT]) for w in THIN_WIDTHS},
}


@functools.lru_cache(maxsize=None)
def family(name, canvas):
    """(leak frames u8 [n, h, w, 3], source frames u8 [n, H, W, 3], geometries): every frame of the family on ``canvas``; a thin leak is
    canvas-high and 1, 2 or 63 px wide.  The geometries: the identity (a thin leak: moved 5 px right, so exactly 1, 2 or 63 lanes
    contribute), the same 3 px down (a column's run starts inside a wavefront's 16 rows), and a 2 degree rotation (nothing aligned)."""
    from offmark import resync
    frames = _frozen(np.stack(FAMILIES[name](canvas)))
    hw = frames.shape[1:3]
    base = (ONE, 0, 0, 0, ONE, SHIFT_X if name.startswith("thin") else 0)
    geoms = (base, base[:2] + (SHIFT_Y,) + base[3:], resync.affine_of_rotation(canvas, hw, 2.0))
    return frames, ge.noise((len(frames), *canvas, 3), 41, *canvas, len(frames)), geoms


@functools.lru_cache(maxsize=None)
def family_tone(name, canvas):
    frames, src, geoms = family(name, canvas)
    return _frozen(tn.statement_sums(src, frames, geoms))


@functools.lru_cache(maxsize=None)
def family_colour(name, canvas):
    frames, src, geoms = family(name, canvas)
    return _frozen(co.statement_sums(src, frames, geoms))


def column_runs(channel):
    """The lengths of the runs of equal values down every column of u8 [h, w]: a flat int array."""
    out = []
    for col in np.asarray(channel).T:
        cuts = np.flatnonzero(np.diff(col.astype(np.int16))) + 1
        out.extend(np.diff(np.concatenate([[0], cuts, [len(col)]])))
    return np.asarray(out)


# ---- 3. histogram groups ----------------------------------------------------------------------------------------------------------------
HIST_VALUES = (0, 255, 17, 200)
HIST_SHAPES = ((16, 48), (13, 61), (2, 397), (3, 265), (131, 127))      # h * w % 4 = 0, 1, 2, 3, each the 768 px of the sequence or more; 16637 px: more than a workgroup's 16384


def group_patterns(frame):
    """int [groups, 3]: per full four-pixel group and channel, 4 (b1 == b0) + 2 (b2 == b1) + (b3 == b2)."""
    px = np.asarray(frame).reshape(-1, 3)
    g = px[:len(px) // 4 * 4].reshape(-1, 4, 3)
    eq = g[:, 1:] == g[:, :-1]
    return 4 * eq[:, 0] + 2 * eq[:, 1] + eq[:, 2]


@functools.lru_cache(maxsize=None)
def _group_sequence():
    """u8 [pixels, 3]: for every ordered pair (A, B) of HIST_VALUES and every pattern, a group that starts at A and, where the pattern
    says "differs", steps to the other of A and B (0 0 0 is ABAB) -- then the same with a third value C in the cycle (ABCA).  Channel c
    runs through the patterns 3 c ahead, with the pairs in another order."""
    pairs = [(a, b) for a in HIST_VALUES for b in HIST_VALUES if a != b]
    chans = []
    for c in range(3):
        seq = []
        for cycle in (2, 3):
            for n, (a, b) in enumerate(pairs[4 * c:] + pairs[:4 * c]):
                ring = (a, b) if cycle == 2 else (a, b, next(v for v in HIST_VALUES if v not in (a, b)))
                for pat in range(8):
                    pat = (pat + 3 * c) % 8
                    at = 0
                    seq.append(ring[0])
                    for bit in (4, 2, 1):
                        at += 0 if pat & bit else 1
                        seq.append(ring[at % cycle])
        chans.append(seq)
    return np.asarray(chans, np.uint8).T


@functools.lru_cache(maxsize=None)
def hist_frames(hw):
    """u8 [2, h, w, 3]: the group sequence repeated over the frame; frame 1 starts 37 groups in, its channels rotated."""
    seq, px = _group_sequence(), hw[0] * hw[1]
    a = np.resize(seq, (px, 3))
    b = np.resize(np.roll(seq, -4 * 37, axis=0)[:, [1, 2, 0]], (px, 3))
    return _frozen(np.stack([a, b]).reshape(2, *hw, 3))


# ---- 4. the RGB cube --------------------------------------------------------------------------------------------------------------------
CUBE_HW = (4096, 4096)
PREFIX = ((7, 250, 0), (255, 1, 128), (64, 0, 255))       # the pixels put in front of the cube: triple i then sits in slot (i + k) % 4


@functools.lru_cache(maxsize=1)
def cube():
    """u8 [2^24, 3]: every RGB triple once, triple i = (i >> 16, (i >> 8) & 255, i & 255).  48 MB, read-only."""
    a = np.arange(256, dtype=np.uint8)
    return _frozen(np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3))


def tone_tables():
    """Three u8 [3, 256] tables, none the identity, every channel its own: seeded permutations, an inversion with an offset per channel
    (wrapping), and the evidence's gamma and gain curves."""
    rng = ge.rng_of(60)
    v = np.arange(256)
    return {"permutations": np.stack([rng.permutation(256) for _ in range(3)]).astype(np.uint8),
            "inversions": np.stack([(255 - v + 85 * c) % 256 for c in range(3)]).astype(np.uint8),
            "curves": np.stack([tn.tone_map(v.astype(np.uint8), *tn.TONE_MAPS[k]) for k in ("gamma-0.85", "gain-1.10-8", "gain-0.70+40-gamma-1.10")])}
