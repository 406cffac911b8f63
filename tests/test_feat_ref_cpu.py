"""tests/feat_ref.py checked on its own, without a GPU: on every input set tests/test_gpu_feat.py uses, the fp32 emulation of each
kernel stays within the derived cap of the float64 reference (so a kernel that does what its source says meets the cap), and
seeded mutants of the emulation - the ways such kernels go wrong - break the cap or the exact check."""
import pytest
import torch

from tests import feat_ref as R


def _ratio(got, ref, cap):
    """Worst |got - ref| / cap; an element with cap 0 must be exact (ratio 0) or counts as inf."""
    err = (got.double() - ref).abs()
    r = torch.where(cap > 0, err / torch.where(cap > 0, cap, torch.ones_like(cap)), torch.where(err > 0, float("inf"), 0.0).double())
    return float(r.max()) if r.numel() else 0.0


def test_stem_emulation_within_cap_and_mutant_rejected():
    worst, zeros = 0.0, 0
    for n, C in R.STEM_CASES:
        case = R.stem_case(n, C)
        ref, cap = R.stem_reference(case)
        worst = max(worst, _ratio(R.stem_emulate(case), ref, cap))
        zeros += int((ref == 0).sum())
        if n > 1:
            assert _ratio(R.stem_emulate(case, relu=False), ref, cap) > 1.0          # mutant: no ReLU
    print(f"FEAT_RATIO_CPU stem {worst:.3f}")
    assert worst <= 1.0 and zeros > 100                                              # ReLU zeros occur


@pytest.mark.parametrize("Fc,kw", R.INTERP_CASES)
def test_interp_emulation_within_cap(Fc, kw):
    case = R.interp_case(Fc, kw)
    ref, cap = R.interp_reference(case)
    r = _ratio(R.interp_emulate(case), ref, cap)
    print(f"FEAT_RATIO_CPU interp Fc={Fc} kw={kw} {r:.3f}")
    assert r <= 1.0
    d = case["deg"].long().clamp(max=kw)
    assert set(d.tolist()) == set(range(kw + 1))                                     # every degree occurs, 0 included
    assert bool((ref[d == 0] == 0).all()) and bool((cap[d == 0] == 0).all())
    assert int(case["on0"].sum()) > 10 and (kw < 2 or (int(case["on1"].sum()) > 10 and int(case["both"].sum()) > 10))


@pytest.mark.parametrize("Fc,kw", R.INTERP_CASES + [(24, 1)])
def test_interp_inputs_hold_no_nearly_coincident_pair(Fc, kw):
    """Input condition of the interpolation tests: a pair is exactly coincident or clearly apart (no d2 in (0, 1e-12)), so the
    fp32 kernels and the float64 reference take the same side of the 1e-16 floor."""
    d2 = R.interp_d2_f64(R.interp_case(Fc, kw))
    d2 = d2[torch.isfinite(d2)]
    assert not bool(((d2 > 0) & (d2 < 1e-12)).any()) and bool((d2 == 0).any())


@pytest.mark.parametrize("mutant", ["clamp", "inv_d", "stale_den"])
def test_interp_mutants_break_the_cap(mutant):
    case = R.interp_case(24, 2)
    ref, cap = R.interp_reference(case)
    kwargs = {"clamp": dict(clamp=False), "inv_d": dict(inv_d=True), "stale_den": dict(stale_den=True)}[mutant]
    got = R.interp_emulate(case, **kwargs)
    bad = ~((got.double() - ref).abs() <= cap)                                        # (a NaN is a miss)
    assert bool(bad.any())
    if mutant == "clamp":                                                            # it is the coincident rows that go wrong
        assert bool(bad[case["on0"] | case["on1"] | case["both"]].any())


@pytest.mark.parametrize("kw", [1, 2])
def test_interp_weights_emulation_within_cap(kw):
    case = R.interp_case(24, kw)
    n0, n1, a, cap = R.interp_weights_reference(case)
    got = R.interp_weights_emulate(case).double()
    rel = (got - a).abs() / torch.where(a > 0, a, torch.ones_like(a))
    r = float((rel / cap.clamp(min=R.U)[:, None]).max())
    print(f"FEAT_RATIO_CPU interp_weights kw={kw} {r:.3f}")
    assert r <= 1.0
    d = case["deg"].long().clamp(max=kw)
    assert bool((got[d == 1] == torch.tensor([1.0, 0.0], dtype=torch.float64)).all()) and bool((got[d == 0] == 0).all())


def test_rowdot_emulation_within_cap():
    worst = 0.0
    for F, ldx, m in R.ROWDOT_CASES:
        case = R.rowdot_case(F, ldx, m)
        ref, cap = R.rowdot_reference(case)
        worst = max(worst, _ratio(R.rowdot_emulate(case), ref, cap))
    print(f"FEAT_RATIO_CPU rowdot {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("prec", [0, 1, 2])
def test_h_conversion_layout_round_trip_and_mutants(prec):
    """h_planes is the inverse of tests/h_util._from_h, its value is v to the format's precision, and the two mutants (hi plane
    rounded to nearest, a non-zero pad column) give other bits."""
    from tests.h_util import _from_h
    g = torch.Generator().manual_seed(prec)
    v = torch.cat([torch.randn(50, 36, generator=g), R.concat_case(4, 50, "tiny")["x"], R.concat_case(4, 50, "huge")["x"]], 1).float()
    ldh = 128
    raw = R.h_planes(v, prec, ldh, hcols=64, fill=3.0)
    val = _from_h(raw, prec, ldh)
    assert bool((val[:, 44:64] == 0).all()) and bool((val[:, 64:] == (6.0 if prec == 0 else 3.0)).all())
    rel = {0: 2.0 ** -21, 1: 2.0 ** -11, 2: 2.0 ** -8}[prec]
    body = v[:, :40].double()
    assert float(((val[:, :40] - body).abs() - rel * body.abs() - (2.0 ** -25 if prec != 2 else 0.0)).max()) <= 0.0
    if prec == 1:
        assert bool((val[:, 40:44].abs() == 65504.0).all())
    if prec == 0:
        hi = raw.view(50, ldh // 32, 2, 32)[:, :, 0].reshape(50, ldh)[:, :44].float()
        assert bool((hi.abs() <= v.abs()).all())                                      # toward zero, saturating
        assert bool((hi[:, 40:].abs() == 65504.0).all())
        assert not R.same_bits(raw, R.h_planes(v, prec, ldh, hcols=64, fill=3.0, hi="rne"))          # mutant: hi to nearest
    assert not R.same_bits(raw, R.h_planes(v, prec, ldh, hcols=64, fill=3.0, pad_value=2.0 ** -20))  # mutant: non-zero pad
    assert R.same_bits(raw, R.h_planes(v, prec, ldh, hcols=64, fill=3.0))


def test_segment_max_reference_and_empty_segment_mutant():
    for F in R.SEG_F:
        for pad in (0, 3):
            case = R.segment_case(F, pad)
            ref = R.segment_max_reference(case)
            assert R.segment_max_matches(ref.float(), ref)
            assert not R.segment_max_matches(R.segment_max_reference(case, empty=-float("inf")).float(), ref)   # mutant: -inf for empty
            assert bool((ref[[0, 6, 8]] == 0).all()) and bool((ref[:, 0][[1, 2, 3, 4, 5, 7]] < 0).all())       # all-negative column
            if F >= 3:
                assert bool((ref[[3, 4], 1] == -float("inf")).all()) and float(ref[5, 2]) == float("inf")
                assert bool(torch.isfinite(ref[7, 1]))
            assert float(ref[7, F - 1]) == (1000.0 if F > 1 else -0.5)                # the maximum sits in the last row
            assert not bool(torch.isnan(ref).any())


def test_exact_references_are_what_they_say():
    for stride, refl, n in R.PACK_CASES:
        case = R.pack_case(stride, refl, n)
        xyzr, batch = R.pack_reference(case)
        p = case["ptr"].long()
        assert batch.shape == (n,) and bool(((p[batch.long()] <= torch.arange(n)) & (torch.arange(n) < p[batch.long() + 1])).all())
        assert bool((xyzr[:, 3] == (case["refl"] if refl else 0.0)).all())
    lv = R.level_case()
    ref, src = R.level_reference(lv), lv["src"][lv["idx"][:lv["m"]].long()]
    v0 = lv["batch"][:lv["m"]] == 0
    assert int(v0.sum()) == 140 and bool((ref[v0, :3] != src[v0, :3]).any())          # 0.37: the round trip is no identity
    assert bool((ref[~v0] == src[~v0]).all())                                         # 3.0: (x / 3) * 3 == x, always
    assert bool((ref[:, 3] == src[:, 3]).all())
    case = R.concat_case(60, 300)
    out = R.concat_reference(case, 72)
    assert bool((out[:, 63:] == 0).all()) and bool((out[:, 60:63] == case["xyzr"][:, :3]).all())
