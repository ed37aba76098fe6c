"""CPU: the inputs of tests/_value_edges.py hold what they are named after, so that test_gpu_value_edges.py passing means something.

Every item is a CONDITION on the NumPy statements (tests/_tone.py, _colour.py, _toned_clip.py), not a measurement: on every edge map
pixels contribute; on the leak of bytes 0, 1, 254, 255 colour_sums' clip predicate keeps some pixels and drops others under every map,
and all four bytes reach tone_sums' bins in every channel; on the leak in 1..254 nothing is dropped; the structured frames have the
runs, the lone lanes and the bins they are built for; the histogram frames hold all eight group patterns in every channel.  The figures
are printed (pytest -s) and recorded in profiles/value_edges_tests.txt."""
import numpy as np
import pytest

import _geometry_edges as ge
import _tone as tn
import _value_edges as ve

CLIPPED = list(ve.EXTREME_BYTES)


# ---- 1. the edge cases --------------------------------------------------------------------------------------------------------------
def test_the_leaks_are_what_they_say_and_the_seed_is_fixed():
    for hw in {c[0] for c in ge.ALIGN_CASES.values()}:
        x, r = ve.leak("extreme", hw), ve.leak("in-range", hw)
        assert x.shape == r.shape == (ve.N, *hw, 3) and x.dtype == r.dtype == np.uint8
        assert set(np.unique(x)) <= set(CLIPPED) and r.min() >= 1 and r.max() <= 254
        assert np.array_equal(ve.leak("noise", hw), ge.noise((ve.N, *hw, 3), 30, *hw))
        assert not x.flags.writeable and not r.flags.writeable
    big = ve.leak("extreme", ge.STEEP_LEAK)
    assert np.array_equal(big, ve.extreme(big.shape, 31, *ge.STEEP_LEAK)) and abs(np.bincount(big.reshape(-1), minlength=256)[CLIPPED] / big.size - 0.25).max() < 0.01
    assert ve.leak("in-range", ge.STEEP_LEAK).min() == 1 and ve.leak("in-range", ge.STEEP_LEAK).max() == 254
    assert list(ge.ALIGN_CASES) == ["steepest", "uniform", "smallest-determinant", "anisotropic", "boundary", "boundary-1x83", "boundary-61x2", "boundary-3x3",
                                    "tiny-3x2", "tiny-1x83", "far-wide", "far-tall"]


@pytest.mark.parametrize("case", ge.ALIGN_CASES)
def test_every_edge_map_has_pixels_and_the_clip_predicate_flips_under_it(case):
    cands, good, bad = ve.edge_cands(case)
    assert len(bad) == 2 and len(good) == len(ge.ALIGN_CASES[case][2]) and all(ge.in_range(cands[k]) for k in good) and not any(ge.in_range(cands[k]) for k in bad)
    tone = {kind: ve.edge_tone(case, kind) for kind in ve.KINDS}
    colour = {kind: ve.edge_colour(case, kind) for kind in ve.KINDS}
    inside = tone["noise"][:, :, 0, :, 0].sum(axis=2)                          # [N, K]: whatever the leak holds, the same pixels are inside
    for kind in ve.KINDS:
        assert np.array_equal(tone[kind][..., 0].sum(axis=3), np.repeat(inside[:, :, None], 3, axis=2)), kind
        assert not tone[kind][:, bad].any() and not colour[kind][:, bad].any(), kind
    assert (inside[:, good] > 0).all()                                         # every map, both frames
    kept = colour["extreme"][:, :, 0]
    assert ((kept[:, good] > 0) & (kept[:, good] < inside[:, good])).all(), (kept[:, good], inside[:, good])       # some kept, some dropped: every map, both frames
    populated = tone["extreme"][:, good][:, :, :, CLIPPED, 0].sum(axis=(0, 1))           # [3, 4]
    assert (populated > 0).all(), populated                                    # 0, 1, 254 and 255 reach the bins of every channel
    assert np.array_equal(colour["in-range"][:, :, 0], inside)                 # 1..254 in, 1..254 out: nothing dropped
    assert not tone["in-range"][:, :, :, [0, 255], 0].any()
    dropped_noise = inside - colour["noise"][:, :, 0]
    print(f"\n{case}: maps {len(good)} inside {inside[:, good].min()}..{inside[:, good].max()} extreme kept {kept[:, good].min()}..{kept[:, good].max()} "
          f"(of inside: {(kept[:, good] / inside[:, good]).min():.3f}..{(kept[:, good] / inside[:, good]).max():.3f}) noise dropped "
          f"{dropped_noise[:, good].min()}..{dropped_noise[:, good].max()} bins 0/1/254/255 pixels per channel {populated.tolist()}")


@pytest.mark.parametrize("which", ve.MOMENT_MAPS, ids=lambda c: f"{c[0]}-{c[1]}")
def test_the_moment_maps_have_interior_pixels_and_the_windows_leave_the_library(which):
    case, k = which
    for kind in ("noise", "extreme"):
        one, many = ve.edge_moments(case, k, kind, 1), ve.edge_moments(case, k, kind, 16)
        assert (one[:, 0, 0] > 0).all() and (one[:, 0, 1:] > 0).all()
        live = many[:, :, 0] > 0
        assert not live[0, :3].any() and live[0, 3:15].all() and not live[0, 15:].any() and live[1, :7].all() and not live[1, 7:].any()
        assert not many[~live].any()
    print(f"\n{case}-{k}: contributing pixels {ve.edge_moments(case, k, 'noise', 1)[:, 0, 0].tolist()}")


# ---- 2. structured content ------------------------------------------------------------------------------------------------------------
def bins_of(frame):
    """int [3, 256]: the frame's own histogram -- tone_sums' counts under the identity."""
    return tn.histograms(frame[None])[0]


@pytest.mark.parametrize("canvas", ve.CANVASES)
def test_the_stripes_and_checkerboards_have_two_bins_per_channel(canvas):
    H, W = canvas
    assert H % 64 and W % 64 and H % 16 and H > 64 and W > 64                   # partial last tiles both ways, a partial last wavefront
    for name, count in (("row-stripes", len(ve.ROW_PERIODS)), ("column-stripes", len(ve.COLUMN_PERIODS)), ("checkerboards", len(ve.CHECKER_CELLS))):
        frames, src, geoms = ve.family(name, canvas)
        assert frames.shape == (count, H, W, 3) and src.shape == frames.shape and geoms[0] == ve.IDENTITY
        tone, colour = ve.family_tone(name, canvas), ve.family_colour(name, canvas)
        for n, f in enumerate(frames):
            assert np.array_equal(tone[n, 0, :, :, 0], bins_of(f))              # the identity: the sums' counts are the frame's histogram
            for c in range(3):
                assert sorted(np.flatnonzero(tone[n, 0, c, :, 0])) == sorted(ve.PALETTE[c]), (name, n, c)      # two bins, the channel's own
                assert len({f[:, :, c].tobytes() for c in range(3)}) == 3       # three different patterns
            assert 0 < colour[n, 0, 0] < H * W                                  # the predicate keeps some pixels and drops others
            assert (tone[n, 1, :, :, 0].sum(axis=1) == (H - 3) * W).all()       # 3 px down: the first three canvas rows are outside
            assert (0 < tone[n, 2, 0, :, 0].sum() < H * W) and np.count_nonzero(tone[n, 2, 0, :, 0]) > 2      # rotated: blends
    rows, cols = ve.family("row-stripes", canvas)[0], ve.family("column-stripes", canvas)[0]
    assert (rows == rows[:, :, :1]).all() and (cols == cols[:, :1]).all()       # every lane alike; every step alike
    for p, f in zip(ve.ROW_PERIODS, rows):
        runs = ve.column_runs(f[:, :, 0])
        assert runs.max() == p and (runs[runs != p].size <= W)                  # bands of p rows, but for each column's last
    for p, f in zip(ve.COLUMN_PERIODS, cols):
        per_tile = [len(np.unique(f[0, t:t + 64, 0])) for t in (0, 64)]        # the bins a wavefront's 64 lanes flush into at the end
        assert set(ve.column_runs(f[:, :, 0])) == {H} and max(per_tile) == (1 if p == 64 else 2), (p, per_tile)


@pytest.mark.parametrize("canvas", ve.CANVASES)
def test_the_staircase_has_column_runs_of_every_length(canvas):
    (stair,), _, _ = ve.family("staircase", canvas)
    y, x = np.mgrid[:canvas[0], :canvas[1]]
    assert np.array_equal(stair[:, :, 0], (y // (1 + x % 16)) % 2 * 255)
    for c in range(3):
        runs = ve.column_runs(stair[:, :, c])
        assert set(range(1, 17)) <= set(runs) and runs.max() == 16, (c, sorted(set(runs)))
        changes = [np.flatnonzero(np.diff(stair[:16, col, c].astype(int))) for col in range(16)]
        assert {int(rows[0]) for rows in changes if len(rows)} == set(range(15))  # in a wavefront's first block 15 lanes' first runs end at 15 different rows
        print(f"\nstaircase {canvas} channel {c}: run lengths {np.bincount(runs)[1:].tolist()}")
    assert len({stair[:, :, c].tobytes() for c in range(3)}) == 3


@pytest.mark.parametrize("canvas", ve.CANVASES)
def test_the_lone_lanes_differ_from_flat_in_exactly_the_stated_pixels(canvas):
    H, W = canvas
    flat = np.broadcast_to(np.asarray(ve.FLAT, np.uint8), (H, W, 3))
    lanes = ve.one_lane(canvas)
    assert len(lanes) == 2 * len(ve.LANE_COLUMNS) and np.array_equal(np.stack([f for f, _ in lanes]), ve.family("one-lane", canvas)[0])
    for n, (f, stated) in enumerate(lanes):
        col, whole = ve.LANE_COLUMNS[n // 2], n % 2
        assert np.array_equal(f != flat, stated) and stated.sum() == (3 * H if whole else 3)
        assert np.array_equal(np.unique(np.argwhere(stated)[:, 1]), [col])      # one canvas column: one lane of one tile column
        assert [int(f[ve.LANE_ROWS[c], col, c]) for c in range(3)] == list(ve.OTHER)
    pairs = ve.two_lanes(canvas)
    for n, (f, stated) in enumerate(pairs):
        assert np.array_equal(f != flat, stated) and stated.sum() == 6
        for c in range(3):
            at = np.argwhere(stated[:, :, c])
            assert at.tolist() == [[ve.PAIR_ROWS[c], ve.PAIR_COLUMNS[0]], [ve.PAIR_ROWS[c], ve.PAIR_COLUMNS[1]]]      # one row, two lanes of one wavefront
            a, b = (int(f[ve.PAIR_ROWS[c], col, c]) for col in ve.PAIR_COLUMNS)
            assert (a == b) == (n == 0) and ve.FLAT[c] not in (a, b)            # into one bin, then into two
    assert max(ve.PAIR_COLUMNS) < 64 and {0, 255} <= set(ve.FLAT + ve.OTHER + ve.THIRD)


@pytest.mark.parametrize("canvas", ve.CANVASES)
def test_the_thin_leaks_put_their_columns_into_one_bin(canvas):
    H, W = canvas
    for w in ve.THIN_WIDTHS:
        frames, _, geoms = ve.family(f"thin-{w}", canvas)
        assert frames.shape == (2, H, w, 3) and geoms[0] == (ve.ONE, 0, 0, 0, ve.ONE, -(5 << 16)) and geoms[1][2] == -(3 << 16)
        tone, colour = ve.family_tone(f"thin-{w}", canvas), ve.family_colour(f"thin-{w}", canvas)
        for n, flat in enumerate(ve.THIN_FLAT):
            for c in range(3):
                assert np.flatnonzero(tone[n, 0, c, :, 0]).tolist() == [flat[c]] and tone[n, 0, c, flat[c], 0] == H * w      # canvas columns 5 .. 5 + w - 1
                assert tone[n, 1, c, flat[c], 0] == (H - 3) * w
            assert 0 < tone[n, 2, 0, :, 0].sum() and colour[n, :, 0].tolist() == [0, 0, 0] if n == 0 else tone[n, :, 0, :, 0].sum(axis=1).tolist()
        print(f"\nthin-{w} on {canvas}: contributing pixels {tone[0, :, 0, :, 0].sum(axis=1).tolist()} (shifted right, then down, rotated)")


# ---- 3. the histogram frames ------------------------------------------------------------------------------------------------------------
def test_the_histogram_frames_hold_every_group_pattern_in_every_channel():
    assert sorted(h * w % 4 for h, w in ve.HIST_SHAPES[:4]) == [0, 1, 2, 3] and max(h * w for h, w in ve.HIST_SHAPES) > 16384
    for hw in ve.HIST_SHAPES:
        frames = ve.hist_frames(hw)
        assert frames.shape == (2, *hw, 3) and set(np.unique(frames)) == set(ve.HIST_VALUES)
        for f in frames:
            pat = ve.group_patterns(f)
            groups = f.reshape(-1, 3)[:len(pat) * 4].reshape(-1, 4, 3)
            for c in range(3):
                assert set(pat[:, c]) == set(range(8)), (hw, c)
                none = groups[pat[:, c] == 0][:, :, c]                          # no two neighbours equal:
                assert (none[:, 2] == none[:, 0]).any() and (none[:, 2] != none[:, 0]).any()      # ABAB, where b2 == b0 may not merge, and ABCA
            assert (pat[:, 0] != pat[:, 1]).any() and (pat[:, 1] != pat[:, 2]).any()             # the channels differ within a group
    print(f"\nhistogram frames: {[f'{h}x{w}={h * w}' for h, w in ve.HIST_SHAPES]}, groups per pattern in channel 0 of the largest: "
          f"{np.bincount(ve.group_patterns(ve.hist_frames(ve.HIST_SHAPES[-1])[0])[:, 0]).tolist()}")


# ---- 4. the cube --------------------------------------------------------------------------------------------------------------------------
def test_the_cube_holds_every_triple_once():
    cube = ve.cube()
    assert cube.shape == (1 << 24, 3) and cube.dtype == np.uint8 and ve.CUBE_HW[0] * ve.CUBE_HW[1] == 1 << 24
    index = (cube[:, 0].astype(np.int32) << 16) | (cube[:, 1].astype(np.int32) << 8) | cube[:, 2]
    assert np.array_equal(index, np.arange(1 << 24, dtype=np.int32))
    for name, lut in ve.tone_tables().items():
        assert lut.shape == (3, 256) and lut.dtype == np.uint8 and (lut != np.arange(256)).any(axis=1).all(), name
        assert not np.array_equal(lut[0], lut[1]) and not np.array_equal(lut[1], lut[2]), name
