"""CPU: the statement behind test_gpu_mask_leaves.py (tests/_mask_leaves.py) held against the oracle -- the named-leaf trees
equal texture_from_features / luminance_from_dc value for value, the infeasible leaves stay empty, tau is what the module says,
the zoo covers every leaf and both sides of every threshold, the per-block mask override restates mark_frame / check_frame --
and the census of the leaves the earlier fixtures reach (ml.write_report: OFFMARK_MASK_LEAVES_OUT=<directory>; the committed copy is
profiles/mask_leaves_tests.txt)."""
import numpy as np

import _mask_leaves as ml
import offmark_oracle as orc

P8 = np.array([0, 1, 1, 0, 0, 1, 0, 1])


def test_named_texture_leaves_equal_the_oracle_value_for_value():
    p = ml.pool()
    ref = orc.texture_from_features(p.ft.a00, p.ft.dcl, p.ft.eh, p.ft.e)
    assert np.array_equal(p.label.value, ref)
    # each leaf holds the value its name says
    for i, name in enumerate(ml.TEX_LEAVES):
        v = ref[p.label.leaf == i]
        if name in ml.TEX_INFEASIBLE:
            assert v.size == 0
            continue
        assert v.size >= 500, (name, v.size)                        # every feasible leaf, richly
        if name.endswith("_1125"):
            assert (v == 1.125).all()
        elif name.endswith("_125"):
            assert (v == 1.25).all()
        elif name.endswith("ramp"):
            assert np.array_equal(v, ml.ramp_value(p.ft.eh[p.label.leaf == i])) and (v > 1).all()
        else:
            assert (v == 1).all()
    # the big arm's constants decide differently from the small arm's on many blocks: what no earlier fixture held
    swapped = dict(ml.PARAMS, A2=ml.PARAMS["A1"], B2=ml.PARAMS["B1"])
    other = ml.tex_label(p.ft.a00, p.ft.dcl, p.ft.eh, p.ft.e, swapped, want_decisive=False).value
    assert ((other != ref) & p.stab.stable).sum() >= 1000
    # the tree is also held on the fixtures' blocks, flat frames and all
    for name, (a00, dcl, eh, e) in ml.fixture_features().items():
        assert np.array_equal(ml.tex_label(a00, dcl, eh, e, want_decisive=False).value, orc.texture_from_features(a00, dcl, eh, e)), name


def test_infeasible_leaves_follow_from_the_inequalities():
    """The module's argument, on random float64 features far beyond what pixels can produce: eh > 900 and cond imply l + e > 400."""
    rng = np.random.default_rng(5)
    n = 400_000
    a00 = rng.uniform(0, 2040, n)
    l, e, h = (np.exp(rng.uniform(np.log(1e-3), np.log(5000), n)) for _ in range(3))
    lab = ml.tex_label(a00, a00 + l, e + h, e, want_decisive=False)
    big_cond = np.isin(lab.leaf, (1, 2, 3, 4, 5, 6))
    assert big_cond.sum() > 10_000
    assert not np.isin(lab.leaf, (1, 3, 5)).any()
    assert (l + e)[big_cond].min() > 900 / (1 + 1 / 1.1) - 1e-9


def test_named_luminance_leaves_equal_the_oracle():
    z = ml.zoo()
    for fl in z.labels:
        ref, mean = orc.luminance_from_dc(fl.ft.ydc)
        assert np.array_equal(fl.lum_value, ref) and max(fl.mean, 90) == mean
        for i, name in enumerate(ml.LUM_LEAVES):
            v = ref[fl.lum_leaf == i]
            assert v.size >= ml.MIN_LEAF
            assert ((v > 1) & (v < 2)).all() if name == "above" else (v == {"lt15": 1.25, "lt25": 1.125, "one": 1.0}[name]).all()


def test_tau_is_ten_times_the_oracles_own_level():
    p = ml.pool()
    assert p.tau == 10 * p.level == 10 * ml.feature_level(p.ft)
    # float32 sums of up to 64 terms of size <= 2040: a few ulp of 10^3; far below every threshold's 1e-3 neighbourhood
    assert 1e-4 < p.level < 2e-3 and p.tau < ml.NEAR * ml.PARAMS["ACT"] / 4
    unstable = int((~p.stab.stable).sum())
    assert 0 < unstable <= p.stab.stable.size // 100
    assert sorted(p.stab.admitted) == np.flatnonzero(~p.stab.stable).tolist()
    for i, adm in p.stab.admitted.items():
        assert ml.in_admitted(float(p.label.value[i]), adm, 0.0)
    # every stable block's value is the same at all 81 perturbations by construction of the leaf, up to the ramp's slope
    print(f"pool: {p.stab.stable.size} blocks, oracle feature level {p.level:.3g}, tau {p.tau:.3g}, {unstable} tau-unstable")


def test_zoo_covers_every_leaf_and_both_sides_of_every_threshold():
    z = ml.zoo()                                                     # asserts the coverage conditions itself
    lines = [f"tau = {z.tau:.6g} = 10 x {z.level:.6g} (largest |float32 feature - float64 feature| of a00, dcl, eh, e over the "
             f"{ml.pool().rgb.shape[0]} pool blocks); {int((~ml.pool().stab.stable).sum())} pool blocks tau-unstable",
             f"{'row (tau-stable blocks)':<34} {'clamped frame':>14} {'unclamped frame':>16}"]
    rows = [ml.zoo_rows(fl) for fl in z.labels]
    strip = lambda k: k.replace("lum:clamped:", "lum:").replace("lum:unclamped:", "lum:")      # noqa: E731
    r0, r1 = ({strip(k): v for k, v in r.items()} for r in rows)
    for k in r0:
        lines.append(f"{k:<34} {r0[k]:>14} {r1[k]:>16}")
    for frame, fl, r in zip(z.frames, z.labels, rows):
        assert frame.shape == (128, 128, 3) and frame.dtype == np.uint8
        ml.assert_zoo_rows(r)
        lines.append(f"frame mean of the block means: {fl.mean:.4f} ({'clamped at 90' if fl.clamped else 'above 90'})")
    assert z.labels[0].clamped and not z.labels[1].clamped
    # the deliberately unstable blocks are unstable for the reason given: their mean is 15 / 25 / the frame mean within rounding
    for fl in z.labels:
        m, ls = fl.m.reshape(-1), fl.lum_stab.stable
        for t in (15.0, 25.0, max(fl.mean, 90.0)):
            hit = np.abs(m - t) <= 2e-3
            assert hit.any() and not ls[hit].any()
            assert all(len(fl.lum_stab.admitted[i]) >= 2 for i in np.flatnonzero(hit))
    ml.write_report("mask_leaves_zoo.txt", lines)


def test_stored_zoo_is_the_generators_output():
    """tests/golden/mask_leaves_zoo.npy / mask_leaves_tau.npy (what the GPU tests load) are zoo()'s frames and the measured tau."""
    z, s = ml.zoo(), ml.stored_zoo()
    assert all(np.array_equal(a, b) for a, b in zip(z.frames, s.frames))
    assert (z.tau, z.level) == (s.tau, s.level)


def test_mask_override_restates_the_oracles_mark_and_read():
    z = ml.zoo()
    wm = orc.shuffle_generate(P8, (1, 256), 0)
    for frame in z.frames:
        for alpha in (20.0, 0.05):
            enc = orc.DctEncoderOracle(alpha=alpha)
            enc.read_wm(wm)
            ref = orc.mark_frame(frame, enc)
            got, dbg = ml.oracle_mark(frame, wm, alpha)
            assert np.array_equal(got, ref) and np.array_equal(dbg["mask"], enc.debug["mask"])
            same, _ = ml.oracle_mark(frame, wm, alpha, np.where(np.arange(256).reshape(16, 16) % 3 == 0, enc.debug["mask"], np.nan))
            assert np.array_equal(same, ref)
            k = int(np.flatnonzero(wm[0])[3])                       # a block that carries a 1: its coefficient is an odd multiple of the step
            other, _ = ml.oracle_mark(frame, wm, alpha, np.where(np.arange(256).reshape(16, 16) == k, 1.7, np.nan))
            diff = (other != ref).any(-1).reshape(16, 8, 16, 8).any((1, 3))
            assert diff.sum() == (alpha == 20.0) and diff.reshape(-1)[k] == (alpha == 20.0)     # that block alone (at 0.05 the change is below a pixel level)
            bits, _ = ml.oracle_read(ref, alpha)
            assert np.array_equal(bits, orc.check_frame(ref, orc.DctDecoderOracle(alpha=alpha)).reshape(-1))


def test_census_of_the_leaves_the_earlier_fixtures_reach():
    """What the suite's DCT fixtures held before the zoo: blocks per leaf, and the nearest block to each threshold.  Recorded, and
    the finding that motivated the zoo is asserted: no fixture block ever met the big arm's ratio clauses."""
    fx = ml.fixture_features()
    feats = [np.concatenate([f[k] for f in fx.values()]) for k in range(4)]
    lab = ml.tex_label(*feats)
    n = lab.leaf.size
    lines = [f"{len(fx)} fixtures, {n} blocks", f"{'texture leaf':<22} {'blocks':>8} {'fixtures':>9}"]
    per_fixture = {name: ml.tex_label(*f, want_decisive=False).leaf for name, f in fx.items()}
    count = {}
    for i, name in enumerate(ml.TEX_LEAVES):
        count[name] = int((lab.leaf == i).sum())
        lines.append(f"{name:<22} {count[name]:>8} {sum(int((v == i).any()) for v in per_fixture.values()):>9}")
    lines.append(f"{'comparison':<22} {'nearest decisive block, relative':>34} {'decisive blocks within 1e-3':>30}")
    for k, (label, _, _) in enumerate(ml.COMPARISONS):
        rel = np.abs(lab.rel[k][lab.decisive[k] & np.isfinite(lab.rel[k])])
        lines.append(f"{label:<22} {(rel.min() if rel.size else np.inf):>34.3g} {int((rel <= ml.NEAR).sum()):>30}")
    assert count["big_first_125"] == 0 and count["big_second_125"] == 0
    assert sum(count.values()) == n and all(count[nm] == 0 for nm in ml.TEX_INFEASIBLE)
    ml.write_report("mask_leaves_census.txt", lines)
