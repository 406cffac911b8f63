"""tests/sa_conv_ref.py on its own (no GPU): the reference agrees with the oracle's message-passing PointNetConv, the
emulations stay inside the hard cap, and the criteria of tests/test_gpu_sa_conv.py are sharp - a dropped neighbour slot, 32
missing k and a lost a_lo term are all far outside them."""
import pytest
import torch

from oracle import net as onet
from tests import sa_conv_ref as R

SHAPES = [(64, 128, 32), (36, 100, 16), (384, 512, 32)]     # (C1, C2, kw)
_cache = {}


def _case(C1, C2, kw):
    """One case and its reference per shape, shared by every test of the module (never modified)."""
    key = (C1, C2, kw)
    if key not in _cache:
        case = R.make_case(48, 150, C1, C2, kw, B=2, seed=100 + C1, deg="mix")
        _cache[key] = (case, {p: R.reference(case, p) for p in R.PRECS}, {p: R.emulate(case, p) for p in R.PRECS})
    return _cache[key]


def _oracle(case):
    """The case in the oracle's edge-list form, through oracle.net._pointnet_conv (fp32): x = P with an identity first block
    of layer 1, so that layer 1 = P[j] + g W1r; BatchNorm with mean 0 and variance 1 - eps carries (bn_s, bn_t)."""
    C1, kw = case["C1"], case["kw"]
    batch_src = torch.repeat_interleave(torch.arange(case["B"]), case["ptr_src"].diff())
    pos = case["xyzr"].clone()
    pos[:, :3] = pos[:, :3] / case["sf"][batch_src].unsqueeze(-1)            # model.py:122, as oracle.net._sa does it
    own = case["idx"].long()
    d = case["deg"].long().clamp(max=kw)
    valid = torch.arange(kw)[None, :] < d[:, None]
    j = case["nbr"].long()
    j = torch.where(j < 0, own[:, None].expand(-1, kw), j)
    dst = torch.arange(case["M"])[:, None].expand(-1, kw)[valid]
    src = j[valid]
    p = "c"
    sd = {f"{p}.local_nn.0.0.weight": torch.cat([torch.eye(C1), case["W1r"].t()], 1), f"{p}.local_nn.0.0.bias": torch.zeros(C1),
          f"{p}.local_nn.1.0.weight": case["W2"], f"{p}.local_nn.1.0.bias": case["b2"],
          f"{p}.local_nn.1.2.weight": case["bn_s"], f"{p}.local_nn.1.2.bias": case["bn_t"],
          f"{p}.local_nn.1.2.running_mean": torch.zeros(case["C2"]),
          f"{p}.local_nn.1.2.running_var": torch.full((case["C2"],), 1.0 - onet.BN_EPS)}
    return onet._pointnet_conv(sd, p, case["P"], pos, pos[own], src, dst)


@pytest.mark.parametrize("kwargs", [dict(M=48, n_src=150, C1=64, C2=128, kw=32, B=2, seed=1, deg="mix"),
                                    dict(M=33, n_src=100, C1=36, C2=100, kw=16, B=3, seed=2, deg="neg")])
def test_reference_matches_the_oracle(kwargs):
    case = R.make_case(**kwargs)
    ref, _ = R.reference(case)
    got = _oracle(case).double()
    scale = max(1.0, float(ref.abs().max()))
    err = float((got - ref).abs().max())
    print(f"oracle vs reference: max err {err:.3e}, scale {scale:.3f}")
    assert err <= 2e-5 * scale
    none = ~R.rows_with_neighbours(case)
    assert bool(none.any()) and float(ref[none].abs().max()) == 0.0


def test_make_case_is_what_the_issue_describes():
    case = R.make_case(64, 200, 64, 128, 32, B=3, seed=5, deg="over")
    again = R.make_case(64, 200, 64, 128, 32, B=3, seed=5, deg="over")
    assert all(torch.equal(case[k], again[k]) for k in case if torch.is_tensor(case[k]))
    assert int((case["bn_s"] == 0).sum()) == 1 and 0.15 < float((case["bn_s"] < 0).float().mean()) < 0.45
    assert float(case["sf"].min()) >= 1.0 and float(case["sf"].max()) <= 3.0 and case["sf"].unique().numel() == 3
    assert int(case["deg"].max()) == 32 + 5
    b = case["batch_dst"].long()
    lo, hi = case["ptr_src"][:-1][b], case["ptr_src"][1:][b]
    assert bool(((case["idx"] >= lo) & (case["idx"] < hi)).all())
    assert bool(((case["nbr"] >= lo[:, None]) & (case["nbr"] < hi[:, None])).all())
    assert case["ptr_dst"].diff().unique().numel() == 3                      # unequal voxels
    Pp, ldp = R.padded_P(case, "fp16")
    assert ldp == 64 and Pp.shape == (201, 64) and bool((Pp[200] == 1.0).all())
    Pp, ldp = R.padded_P(R.make_case(9, 40, 36, 100, 16, seed=1), "f16x3")
    assert ldp == 64 and float(Pp[:40, 36:].abs().max()) == 0.0
    neg = R.make_case(64, 200, 64, 128, 32, seed=5, deg="neg")
    assert bool((neg["nbr"] < 0).any())
    own = R.make_case(64, 200, 64, 128, 32, B=2, seed=5, deg="self")
    sel = own["batch_dst"] == 0
    assert bool((own["nbr"][sel] == own["idx"][sel][:, None]).all())


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("C1,C2,kw", SHAPES)
def test_emulation_is_inside_the_cap(prec, C1, C2, kw):
    case, refs, emus = _case(C1, C2, kw)
    ref, cap = refs[prec]
    ratio = float(((emus[prec] - ref).abs() / cap.clamp(min=1e-300)).max())
    print(f"{prec} {C1}x{C2} kw {kw}: worst |emulate - reference| / cap = {ratio:.3f}")
    assert bool(((emus[prec] - ref).abs() <= cap).all())
    if prec == "f16x3":
        rtz = R.emulate(case, prec, a_hi="rtz")
        assert bool(((rtz - ref).abs() <= cap).all())
    none = ~R.rows_with_neighbours(case)
    assert bool(none.any()) and float(emus[prec][none].abs().max()) == 0.0


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("C1,C2,kw", SHAPES)
def test_a_dropped_slot_and_missing_k_exceed_the_cap(prec, C1, C2, kw):
    case, refs, _ = _case(C1, C2, kw)
    ref, cap = refs[prec]
    affected = R.rows_with_neighbours(case)
    dropped = R.emulate(case, prec, drop_last_slot=True)
    hit = ((dropped - ref).abs() > cap).any(dim=1)[affected]
    print(f"{prec} {C1}x{C2} kw {kw}: last slot dropped: {100 * float(hit.float().mean()):.0f} % of {int(affected.sum())} targets over the cap")
    assert float(hit.float().mean()) > 0.5
    short = R.emulate(case, prec, zero_last_k=32)
    hit = ((short - ref).abs() > cap).any(dim=1)[affected]
    assert bool(hit.all())


@pytest.mark.parametrize("C1,C2,kw", SHAPES)
def test_a_lost_lo_term_is_far_outside_the_rms_margin(C1, C2, kw):
    case, refs, emus = _case(C1, C2, kw)
    ref, _ = refs["f16x3"]
    rows = R.rows_with_neighbours(case)
    full = R.rms((emus["f16x3"] - ref)[rows])
    lost = R.rms((R.emulate(case, "f16x3", drop_a_lo=True) - ref)[rows])
    print(f"f16x3 {C1}x{C2} kw {kw}: RMS error {full:.3e}, without a_lo {lost:.3e} ({lost / full:.0f} x)")
    assert lost > 100 * full
