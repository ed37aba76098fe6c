"""CPU: the NumPy statement of the DwtDctSvd soft read-out (tests/_svd_soft.py; a build extension, not reference semantics)
agrees with the reference's hard decision where that is defined, and is worth having: on a noise level at which the
reference's per-frame hard decision with a mode vote over whole patterns loses segments, adding the soft sums over a segment's
frames recovers all of them."""
import numpy as np
import pytest

import offmark_oracle as orc
import _svd_soft as ss

P8 = np.array([0, 1, 1, 0, 0, 1, 0, 1])


@pytest.mark.parametrize("H,W,blk,seed", [(64, 96, 4, 1001), (36, 52, 4, 1002), (240, 320, 4, 1003), (64, 96, 8, 1004), (240, 320, 8, 1005)])
def test_sign_is_the_oracle_decoders_bit_on_determined_blocks(H, W, blk, seed):
    wm = orc.shuffle_generate(P8, (1, H * W // 64), 0)
    enc = orc.DwtDctSvdEncoderOracle(scales=(0, 15, 0), blk=blk)
    enc.read_wm(wm)
    marked = orc.mark_frame(orc.synthetic_frame(H, W, seed), enc)
    st = ss.statement(marked, blk=blk)
    ok = ss.determined(st["s0"])
    assert ok.mean() > 0.9 and st["m"].size == ((H // 4 * 2) // blk) * ((W // 4 * 2) // blk)
    assert np.array_equal(st["m"][ok] > 0, st["bits"][ok] == 1)
    assert np.array_equal(st["m"][ok] < 0, st["bits"][ok] == 0)
    assert np.abs(st["m"]).max() <= 16384


def test_metric_landmarks():
    """-2^14 where the encoder puts a 0, +2^14 where it puts a 1, 0 on the thresholds."""
    s0 = np.array([3.75, 11.25, 0.0, 7.5, 15.0, 15 * 7 + 3.75, 15 * 7 + 11.25])
    m = np.rint(-np.sin(2 * np.pi * s0 / 15.0) * 16384).astype(np.int64)
    assert m.tolist() == [-16384, 16384, 0, 0, 0, -16384, 16384]


def test_noise_recipe_hard_vote_loses_segments_soft_sums_recover_all():
    r = ss.noise_recipe()
    hard = ss.hard_recovered(r["hard"], r["payloads"])
    soft = ss.soft_recovered(r["soft"], r["payloads"])
    totals = np.abs(r["soft"].sum(axis=1))                       # [segments, L]
    worst = r["budget"].sum(axis=1).max()
    print(f"hard vote {hard}/16, soft {soft}/16; smallest |segment total| {totals.min()}, worst summed budget {worst}")
    assert hard == 12 and soft == 16
    # a device result within budget of the statement at every position cannot flip a position of a segment total
    assert totals.min() == 43176 and worst == 1196
