"""CPU-only: the resync calls behave alike on RGB frames and on 4:2:0 planes, for both codecs.
(a) the four window entry points refuse a bad window argument with one code and one message; only the planar two know the
    even-phase rule;
(b) a DCT score call names its OWN sizing function when the workspace is too small;
(c) the three read_*_leak recipes of offmark.resync, driven by a NumPy stub decoder whose soft sums are built from known payloads,
    return the constructed phase, base and picks under one set of keys.
Every refusal comes before any HIP call, so these run without a GPU (the pointer values below are never dereferenced)."""
import ctypes as C

import numpy as np
import pytest

E_ARG, E_WORKSPACE = -1, -2
H, W, N, L = 62, 84, 3, 8
IN, OUT, WS = 0x10001, 0x20000, 0x30000          # WS: 256-byte aligned
BIG = 1 << 40                                    # a workspace size that is never too small
PY, PX, CANVAS_COLS = 6, 4, 13                   # the window: (62 - 6) // 8 = 7 rows of (84 - 4) // 8 = 10 units


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from offmark import _hip
    return _hip.load()


def scales3(v):
    return None if v is None else (C.c_double * 3)(*v)


def outcome(lib, rc):
    return rc, lib.ofmk_last_error().decode()


def svd_window_rgb(lib, h=H, w=W, py=PY, px=PX, canvas_cols=CANVAS_COLS, base=0, scales=(0, 15, 0), ws=WS):
    return outcome(lib, lib.ofmk_svd_detect_soft_window_rgb8(IN, N, h, w, py, px, canvas_cols, base, L, scales3(scales), 4, OUT, None, None))


def svd_window_yuv420(lib, h=H, w=W, py=PY, px=PX, canvas_cols=CANVAS_COLS, base=0, scales=(0, 15, 0), ws=WS):
    return outcome(lib, lib.ofmk_svd_detect_soft_window_yuv420(IN, 0, N, h, w, py, px, canvas_cols, base, L, scales3(scales), 4, OUT, None,
                                                               None))


def dct_window_rgb(lib, h=H, w=W, py=PY, px=PX, canvas_cols=CANVAS_COLS, base=0, scales=None, ws=WS):
    return outcome(lib, lib.ofmk_detect_soft_window_rgb8(IN, N, h, w, py, px, canvas_cols, base, L, 20.0, OUT, 0, ws, BIG, None, None))


def dct_window_yuv420(lib, h=H, w=W, py=PY, px=PX, canvas_cols=CANVAS_COLS, base=0, scales=None, ws=WS):
    return outcome(lib, lib.ofmk_detect_soft_window_yuv420(IN, 1, N, h, w, py, px, canvas_cols, base, L, 20.0, OUT, 0, ws, BIG, None, None))


WINDOW_CALLS = [svd_window_rgb, svd_window_yuv420, dct_window_rgb, dct_window_yuv420]
BAD_WINDOWS = {
    "py = 8": dict(py=8),
    "px = -1": dict(px=-1),
    "no full unit": dict(h=12),                                        # (12 - 6) // 8 = 0 rows
    "canvas_cols below the units per row": dict(canvas_cols=9),
    "base = -1": dict(base=-1),
    "base + rows * canvas_cols = 2^31": dict(base=(1 << 31) - 7 * CANVAS_COLS),
}


@pytest.mark.parametrize("case", list(BAD_WINDOWS))
def test_the_four_window_calls_refuse_a_bad_window_alike(lib, case):
    got = [call(lib, **BAD_WINDOWS[case]) for call in WINDOW_CALLS]
    assert got[0][0] == E_ARG and got[0][1] != ""
    assert all(g == got[0] for g in got), got


def test_the_messages_of_the_window_checks_differ_from_each_other(lib):
    texts = {svd_window_rgb(lib, **kw)[1] for kw in BAD_WINDOWS.values()}
    assert len(texts) == 5, texts                                      # py = 8 and px = -1 share the phase-range message


@pytest.mark.parametrize("odd", [dict(py=1), dict(px=3)])
def test_only_planes_have_the_even_phase_rule(lib, odd):
    planar = [svd_window_yuv420(lib, **odd), dct_window_yuv420(lib, **odd)]
    assert planar[0] == planar[1] and planar[0][0] == E_ARG and "even" in planar[0][1], planar
    # interleaved frames take the odd phase and go on to the check that follows the window's: the scales, the workspace
    rc, text = svd_window_rgb(lib, scales=None, **odd)
    assert rc == E_ARG and "scales is null" in text, text
    rc, text = dct_window_rgb(lib, ws=None, **odd)
    assert rc == E_ARG and "workspace is null" in text, text


def test_a_short_sync_workspace_names_the_calls_own_sizing_function(lib):
    need = lib.ofmk_sync_workspace_bytes(1, H, W)
    assert need > 0
    rc, text = outcome(lib, lib.ofmk_sync_scores_rgb8(IN, N, H, W, 20.0, OUT, 0, WS, need - 1, None, None))
    assert rc == E_WORKSPACE and "ofmk_sync_workspace_bytes(1, H, W)" in text, text
    need = lib.ofmk_sync_workspace_bytes_yuv420(1, H, W)
    assert need > 0
    rc, text = outcome(lib, lib.ofmk_sync_scores_yuv420(IN, 0, N, H, W, 20.0, OUT, 0, WS, need - 1, None, None))
    assert rc == E_WORKSPACE and "ofmk_sync_workspace_bytes_yuv420(1, H, W)" in text, text


# ---- (c) the read_*_leak recipes over a stub decoder ---------------------------------------------------------------------------
ONE = 1 << 14
KEY, UNITS, BASE = 0, 5, 3                        # every frame reads UNITS units per position; the crop rotated positions by BASE
LABELS = [4, 4, 9, 9, 17, 17]                     # three segments of two frames
CANDIDATES = [[[0, 1, 1, 0, 0, 1, 0, 1], [1, 1, 0, 1, 0, 0, 0, 1]],
              [[1, 0, 0, 0, 1, 1, 1, 0], [0, 0, 1, 0, 1, 1, 0, 1]],
              [[0, 1, 0, 0, 1, 0, 1, 1], [1, 1, 1, 0, 0, 1, 0, 0]]]
PICKS = [1, 0, 1]
LH, LW = 61, 83                                   # the RGB leak; planes are 62 x 84
PHASE_RGB, PHASE_PLANES = (5, 3), (2, 6)


def carried(payload):
    """+-1 per position 0..L-1 of the marked frames, by the generator itself"""
    from offmark.generator.shuffler import Shuffler
    p = np.asarray(payload)
    return 2 * np.asarray(Shuffler(key=KEY).generate_wm(p, (p.size,))).reshape(-1).astype(np.int64) - 1


def soft_per_frame(base):
    """int64 [n, L]: each frame reads its segment's payload at +-2^14 per unit, at positions rotated back by ``base``"""
    rows = [np.roll(carried(CANDIDATES[s][PICKS[s]]), -base) * ONE * UNITS for s in range(3) for _ in range(2)]
    return np.stack(rows)


def phase_scores(n, h, w, phase, even_only):
    """int64 [n, 64]: the phase's units all at 2^14, every other phase that takes part at 0.7 of that"""
    out = np.zeros((n, 64), np.int64)
    for py in range(8):
        for px in range(8):
            if even_only and (py % 2 or px % 2):
                continue
            units = max((h - py) // 8, 0) * max((w - px) // 8, 0)
            out[:, 8 * py + px] = units * ONE if (py, px) == phase else units * ONE * 7 // 10
    return out


class StubDecoder:
    def __init__(self):
        self.calls = []

    def sync_scores_u8(self, frames):
        self.calls.append("sync_scores_u8")
        return phase_scores(frames.shape[0], frames.shape[1], frames.shape[2], PHASE_RGB, False)

    def decode_soft_window_u8(self, frames, L, phase, canvas_cols, base=0):
        self.calls.append(("decode_soft_window_u8", tuple(phase), canvas_cols, base))
        return soft_per_frame(BASE)

    def sync_scores_planes_yuv420(self, planes, height, width, layout="i420"):
        self.calls.append("sync_scores_planes_yuv420")
        return phase_scores(planes.shape[0], height, width, PHASE_PLANES, True)

    def decode_soft_window_planes_yuv420(self, planes, height, width, L, phase, canvas_cols, base=0, layout="i420"):
        self.calls.append(("decode_soft_window_planes_yuv420", tuple(phase), canvas_cols, base))
        return soft_per_frame(BASE)

    def decode_soft_warp_u8(self, frames, canvas_hw, geom, L):
        self.calls.append(("decode_soft_warp_u8", tuple(canvas_hw), tuple(geom)))
        return soft_per_frame(0)                  # canvas coordinates: no rotation is left


FRAMES = np.zeros((6, LH, LW, 3), np.uint8)
PLANES = np.zeros((6, 62 * 84 * 3 // 2), np.uint8)
GEOM = (1 << 16, 0, 1 << 16, 0)
CROPPED_KEYS = {"phase", "contrast", "normalised", "segments", "soft_by_segment", "base", "picks", "score", "runner_up_score", "ambiguous"}
RESCALED_KEYS = (CROPPED_KEYS - {"phase"}) | {"geometry", "index"}


def check_alignment(out, base):
    assert out["segments"] == [4, 9, 17]
    assert out["base"] == base and out["picks"].tolist() == PICKS
    assert out["score"] == 3 * 2 * L * ONE * UNITS                    # every position of every frame agrees with its payload
    expect = np.stack([2 * np.roll(carried(CANDIDATES[s][PICKS[s]]), -base) * ONE * UNITS for s in range(3)])
    assert out["soft_by_segment"].dtype == np.int64 and np.array_equal(out["soft_by_segment"], expect)


def test_read_cropped_leak_returns_the_constructed_phase_base_and_picks():
    from offmark import resync
    dec = StubDecoder()
    out = resync.read_cropped_leak(dec, FRAMES, LABELS, 8 * CANVAS_COLS, CANDIDATES, key=KEY, L=L)
    assert set(out) == CROPPED_KEYS
    assert out["phase"] == PHASE_RGB and out["contrast"] == pytest.approx(1 / 0.7, rel=1e-3)
    assert out["normalised"][8 * 5 + 3] == 1.0
    assert dec.calls == ["sync_scores_u8", ("decode_soft_window_u8", PHASE_RGB, CANVAS_COLS, 0)]
    check_alignment(out, BASE)
    as_dict = resync.read_cropped_leak(dec, FRAMES, LABELS, 8 * CANVAS_COLS, dict(zip([4, 9, 17], CANDIDATES)), key=KEY, L=L)
    check_alignment(as_dict, BASE)


def test_read_cropped_leak_yuv420_returns_the_same_keys_and_the_constructed_values():
    from offmark import resync
    dec = StubDecoder()
    out = resync.read_cropped_leak_yuv420(dec, PLANES, 62, 84, LABELS, 8 * CANVAS_COLS, CANDIDATES, key=KEY, L=L, layout="nv12")
    assert set(out) == CROPPED_KEYS
    assert out["phase"] == PHASE_PLANES and out["contrast"] == pytest.approx(1 / 0.7, rel=1e-3)
    odd = [8 * py + px for py in range(8) for px in range(8) if py % 2 or px % 2]
    assert out["normalised"][8 * 2 + 6] == 1.0 and not out["normalised"][odd].any()
    assert dec.calls == ["sync_scores_planes_yuv420", ("decode_soft_window_planes_yuv420", PHASE_PLANES, CANVAS_COLS, 0)]
    check_alignment(out, BASE)


def test_read_rescaled_leak_at_one_geometry_returns_its_documented_keys():
    from offmark import resync
    dec = StubDecoder()
    out = resync.read_rescaled_leak(dec, FRAMES, LABELS, (72, 104), CANDIDATES, [GEOM], key=KEY, L=L)
    assert set(out) == RESCALED_KEYS
    assert out["geometry"] == GEOM and out["index"] == 0 and out["contrast"] is None and out["normalised"] is None
    assert out["runner_up_score"] is None
    assert dec.calls == [("decode_soft_warp_u8", (72, 104), GEOM)]
    check_alignment(out, 0)


def test_a_segment_list_of_the_wrong_length_is_refused_alike():
    from offmark import resync
    texts = []
    for labels in (LABELS[:-1], LABELS + [17]):
        for read in (lambda s: resync.read_cropped_leak(StubDecoder(), FRAMES, s, 8 * CANVAS_COLS, CANDIDATES, key=KEY, L=L),
                     lambda s: resync.read_cropped_leak_yuv420(StubDecoder(), PLANES, 62, 84, s, 8 * CANVAS_COLS, CANDIDATES, key=KEY, L=L),
                     lambda s: resync.read_rescaled_leak(StubDecoder(), FRAMES, s, (72, 104), CANDIDATES, [GEOM], key=KEY, L=L)):
            with pytest.raises(ValueError) as err:
                read(labels)
            texts.append(str(err.value))
    assert set(texts) == {"segment_of_frame needs one entry per frame"}
