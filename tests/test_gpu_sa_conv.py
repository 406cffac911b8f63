"""The fused PointNetConv kernels (p2w_sa_conv_h, p2w_sa_conv_h_rows, p2w_sa_conv) called directly with real data and held
against tests/sa_conv_ref.py.  Every comparison makes the same three assertions (``_check``):
  hard cap   |got - reference| <= cap for every element (a worst-case bound from the number formats),
  RMS margin RMS(got - reference) <= m * RMS(emulate - reference) over the targets with neighbours, m = 2 for fp16 / bf16 (the
             emulation reproduces their operand rounding exactly; the margin is for accumulation order), m = 4 for f16x3 / fp32
             (split_pair's round-toward-zero hi, fused multiply-adds and accumulation order are each about as large as the
             emulated error itself),
  rows without neighbours are exactly 0.
Each comparison prints a line "SA_RATIO <case> <precision> <RMS ratio> <worst cap ratio>" (pytest -s); docs/LAB_NOTES.md holds the
table measured on the MI355X."""
import pytest
import torch

from tests import sa_conv_ref as R
from tests.h_util import _from_h, _pack_h

pytestmark = pytest.mark.gpu

ITEM_256, ITEM_128, PACK8 = 1, 2, 4
RANGE_WORDS, RANGE_SLOTS = 1024, 16
MARGIN = {"f16x3": 4.0, "fp32": 4.0, "fp16": 2.0, "bf16": 2.0}
H_CONV = {0: 2e-6, 1: 1e-3, 2: 8e-3}        # fp32 -> H conversion limits (x scale), as in test_gemm_h_epilogue
PRECS = [0, 1, 2]

A1, A2, A3 = (37, 150, 64, 128, 32), (37, 150, 192, 256, 32), (37, 150, 384, 512, 32)
B1, B2 = (6500, 400, 8, 16, 8), (2100, 400, 36, 100, 16)
WIDTH_EDGES = [(9, 40, 4, 8, 32), (9, 40, 36, 100, 16), (9, 40, 512, 1024, 32), (33, 100, 100, 130, 7), (5, 20, 64, 260, 1)]
D_SHAPE = (64, 200, 64, 128, 32)
# degree policies at D_SHAPE: (policy, voxels)
POLICIES = [("zero", 1), ("full", 1), ("over", 1), ("uniform", 1), ("set", 1), ("neg", 1), ("self", 2), ("mix", 3)]

_cases, _refs = {}, {}


def _case(shape, B=1, deg="mix"):
    """Cases are built once per module and never modified."""
    key = (shape, B, deg)
    if key not in _cases:
        M, n_src, C1, C2, kw = shape
        _cases[key] = R.make_case(M, n_src, C1, C2, kw, B=B, seed=sum(shape) + 7 * B + len(deg), deg=deg)
    return _cases[key]


def _ref(case, prec):
    """(reference, cap, emulation) of a case for a precision name, computed once."""
    key = (id(case), prec)
    if key not in _refs:
        ref, cap = R.reference(case, prec)
        _refs[key] = (ref, cap, R.emulate(case, prec))
    return _refs[key]


def _tag(case, extra=""):
    return f"{case['M']}x{case['n_src']}x{case['C1']}x{case['C2']}k{case['kw']}B{case['B']}{case['policy']}{extra}"


def _check(case, prec, got, tag=""):
    """The three assertions on got [M, C2] (float64, CPU)."""
    ref, cap, emu = _ref(case, prec)
    rows = R.rows_with_neighbours(case)
    assert bool(torch.isfinite(got).all()), "an output element was not written (sentinel left) or is not finite"
    err = (got - ref).abs()
    e_got, e_emu = R.rms((got - ref)[rows]), R.rms((emu - ref)[rows])
    worst = float((err[rows] / cap[rows].clamp(min=1e-300)).max()) if bool(rows.any()) else 0.0
    print(f"SA_RATIO {_tag(case, tag)} {prec} {e_got / e_emu if e_emu else 0.0:.3f} {worst:.4f}")
    assert bool((err <= cap).all()), (worst, int((err > cap).sum()))
    assert e_got <= MARGIN[prec] * e_emu, (e_got, e_emu)
    assert float(got[~rows].abs().max() if bool((~rows).any()) else 0.0) == 0.0


def _run(case, prec, flags=0, want_out=True, want_h=True, ldo=None, ldh=None, ws=None, perm=None, rows_api=False, range_words=None,
         out_rows=None, P_dev=None, xyzr_dev=None, bn_t=None):
    """One call of p2w_sa_conv_h (or p2w_sa_conv_h_rows when perm / range_words / rows_api ask for it) on `case`.
    Outputs are allocated filled with NaN; the workspace is sized by p2w_sa_conv_h_ws_bytes.  perm: P's rows are stored permuted,
    src_row = perm.  P_dev / xyzr_dev: existing (larger) device allocations to place P and the records in.
    After the call P's row n_src must be all zero.
    Returns dict(out [rows, ldo] fp32 CPU | None, h [rows, ldh] float64 decoded | None, h_raw, ldo, ldh)."""
    from pointstowood_amd._lib import check, lib, ptr, stream
    L = lib()
    name = R.PREC_NAME[prec]
    gran, planes = R.K_GRAN[name], (2 if prec == 0 else 1)
    M, n_src, C1, C2, kw = (case[k] for k in ("M", "n_src", "C1", "C2", "kw"))
    Pp, ldp = R.padded_P(case, name)
    if perm is not None:
        src = Pp[:n_src].clone()
        Pp[perm.long()] = src                       # row perm[j] holds source point j
    if P_dev is not None:
        assert P_dev.shape[0] >= n_src + 1 and P_dev.shape[1] == ldp
        P_dev[:n_src + 1].copy_(Pp)
    else:
        P_dev = Pp.cuda()
    if xyzr_dev is not None:
        assert xyzr_dev.shape[0] >= n_src
        xyzr_dev[:n_src].copy_(case["xyzr"])
    else:
        xyzr_dev = case["xyzr"].cuda()
    w1r4 = torch.zeros(4, ldp)
    w1r4[:, :C1] = case["W1r"]
    W2h, wscale, Kp = _pack_h(case["W2"], prec)
    assert Kp == ldp
    d = lambda t: t.cuda().contiguous()
    w1r4, idx, bd, sf, nbr, deg, b2, s = map(d, (w1r4, case["idx"], case["batch_dst"], case["sf"], case["nbr"], case["deg"],
                                                 case["b2"], case["bn_s"]))
    t = d(case["bn_t"] if bn_t is None else bn_t)
    rows = out_rows or M
    ldo = ldo or C2
    ldh = ldh or R.round_up(C2, gran)
    out = torch.full((rows, ldo), float("nan"), device="cuda") if want_out else None
    hdt = torch.bfloat16 if prec == 2 else torch.float16
    out_h = torch.full((rows, planes * ldh), float("nan"), dtype=hdt, device="cuda") if want_h else None
    if ws is None:
        ws = torch.zeros(int(L.p2w_sa_conv_h_ws_bytes(M, flags)), dtype=torch.uint8, device="cuda")
    assert ws.numel() >= int(L.p2w_sa_conv_h_ws_bytes(M, flags))
    src_row = d(perm.to(torch.int32)) if perm is not None else None
    args = (prec, ptr(P_dev), ldp, n_src, ptr(xyzr_dev), ptr(idx), ptr(bd), ptr(sf), ptr(nbr), ptr(deg), kw, M, ptr(w1r4), ptr(W2h),
            wscale, C1, C2, ptr(b2), ptr(s), ptr(t), ptr(out), ldo if want_out else 0, ptr(out_h), ldh if want_h else 0, ptr(ws),
            ws.numel(), flags)
    if perm is not None or range_words is not None or rows_api:
        check(L.p2w_sa_conv_h_rows(*args, ptr(src_row), ptr(range_words), stream()), "p2w_sa_conv_h_rows")
    else:
        check(L.p2w_sa_conv_h(*args, stream()), "p2w_sa_conv_h")
    torch.cuda.synchronize()
    zero_row = P_dev[n_src].cpu()
    assert float(zero_row.abs().max()) == 0.0, "the call must zero P's row n_src"
    return dict(out=out.cpu() if want_out else None, h=_from_h(out_h, prec, ldh) if want_h else None,
                h_raw=out_h.cpu() if want_h else None, ldo=ldo, ldh=ldh)


def _check_both(case, prec, r, tag=""):
    """fp32 output against the reference; the H output agrees with it within the conversion limits and has zero pad columns."""
    M, C2 = case["M"], case["C2"]
    name = R.PREC_NAME[prec]
    _check(case, name, r["out"][:M, :C2].double(), tag)
    scale = max(1.0, float(_ref(case, name)[0].abs().max()))
    assert float((r["h"][:M, :C2] - r["out"][:M, :C2].double()).abs().max()) <= H_CONV[prec] * scale
    assert float(r["h"][:M, C2:].abs().max() if r["ldh"] > C2 else 0.0) == 0.0


# ---- a. work-item shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape,flags", [(A1, 0), (A1, ITEM_256), (A2, 0), (A2, ITEM_128), (A3, 0)])
def test_work_item_shapes(shape, flags, prec):
    """M = 37 with two column tiles gives 20 items on 16 workgroups: XCD chunking, workgroups that return early, and the
    pipeline's carry-over between two items; both item shapes on the side the library would not pick."""
    case = _case(shape)
    _check_both(case, prec, _run(case, prec, flags), f"/flags{flags}")


# ---- b. several items per workgroup with a one-slab K loop -------------------------------------------------------------
@pytest.mark.parametrize("shape,prec", [(B1, 0), (B2, 0), (B2, 1), (B2, 2)])
def test_several_items_per_workgroup_one_slab(shape, prec):
    case = _case(shape)
    _check_both(case, prec, _run(case, prec))


# ---- c. width edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", WIDTH_EDGES)
def test_width_edges(shape, prec):
    """C2 that is no multiple of 16, C2 = 1024, C1pad = 512, kw < 16 down to 1."""
    case = _case(shape)
    _check_both(case, prec, _run(case, prec))


# ---- d + e. degree policies, with and without P2W_SA_PACK8 ------------------------------------------------------------
def _packed_and_plain(case, prec):
    plain, packed = _run(case, prec, 0), _run(case, prec, PACK8)
    _check_both(case, prec, plain)
    _check_both(case, prec, packed, "/pack8")
    assert torch.equal(plain["out"].view(torch.int32), packed["out"].view(torch.int32))
    assert torch.equal(plain["h_raw"].view(torch.int16), packed["h_raw"].view(torch.int16))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("policy,B", POLICIES)
def test_degree_policies_plain_and_packed(policy, B, prec):
    """All 0, all kw, deg > kw (clamped), uniform, the 8 / 9 boundary of the packing, -1 in valid slots, dmax = 0, three unequal
    voxels: each against the reference, and packed == plain bit for bit ("zero" and "full" leave one packing class empty)."""
    _packed_and_plain(_case(D_SHAPE, B, policy), prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape,policy", [((1, 100, 64, 128, 32), "small"), ((3, 100, 64, 128, 32), "large"), ((4, 100, 64, 128, 32), "small"),
                                          ((5, 100, 64, 128, 32), "set"), ((2100, 400, 36, 100, 16), "set")])
def test_pack8_sizes(shape, policy, prec):
    """M = 1, 3, 4, 5 (less than, exactly and just over one shared tile) and 2100; all-small, all-large and mixed."""
    _packed_and_plain(_case(shape, 1, policy), prec)


# ---- f. p2w_sa_conv_h_rows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", [A2, B2])
def test_permuted_p_rows_give_the_same_bits(shape, prec):
    case = _case(shape)
    perm = torch.randperm(case["n_src"], generator=torch.Generator().manual_seed(11))
    ident, rows = _run(case, prec), _run(case, prec, perm=perm)
    assert not torch.equal(perm, torch.arange(case["n_src"]))
    assert torch.equal(ident["out"].view(torch.int32), rows["out"].view(torch.int32))
    assert torch.equal(ident["h_raw"].view(torch.int16), rows["h_raw"].view(torch.int16))
    _check_both(case, prec, rows, "/rows")


# ---- g. outputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", [A1, (33, 100, 100, 130, 7), (9, 40, 36, 100, 16)])
def test_output_combinations_and_wider_rows(shape, prec):
    """out only, out_h only, both; ldo = C2 + 4 keeps its sentinel columns; with ldh two K slabs wider than round_up(C2) the
    columns [C2, round_up(C2, K granularity)) are zero, those from round_up(C2, 256) on keep the sentinel, anything between is
    zero or sentinel (include/p2w.h: the launch writes zeros up to the end of its last column tile)."""
    case = _case(shape)
    M, C2 = case["M"], case["C2"]
    gran = R.K_GRAN[R.PREC_NAME[prec]]
    ldo, ldh = C2 + 4, R.round_up(C2, gran) + 2 * gran
    both = _run(case, prec, ldo=ldo, ldh=ldh)
    only_f = _run(case, prec, want_h=False, ldo=ldo)
    only_h = _run(case, prec, want_out=False, ldh=ldh)
    _check_both(case, prec, dict(both, h=both["h"][:, :R.round_up(C2, gran)], ldh=R.round_up(C2, gran)), "/wide")
    assert torch.equal(both["out"][:, :C2].view(torch.int32), only_f["out"][:, :C2].view(torch.int32))
    assert torch.equal(both["h_raw"].view(torch.int16), only_h["h_raw"].view(torch.int16))
    for r in (both, only_f):
        assert bool(torch.isnan(r["out"][:, C2:]).all())
    for r in (both, only_h):
        h = r["h"]                                                   # decoded: NaN wherever a plane still holds the sentinel
        assert float(h[:, C2:R.round_up(C2, gran)].abs().max() if R.round_up(C2, gran) > C2 else 0.0) == 0.0
        assert bool(torch.isnan(h[:, R.round_up(C2, 256):]).all())
        mid = h[:, R.round_up(C2, gran):min(ldh, R.round_up(C2, 256))]
        assert bool((torch.isnan(mid) | (mid == 0)).all())


# ---- h. stale workspace -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("flags", [0, PACK8])
def test_workspace_left_over_from_a_larger_call(flags, prec):
    """The engine takes its workspace from torch.empty: it holds another call's descriptors in every real run.  A call at M = 300,
    then M = 37 in the same workspace: rows 0..36 equal a call on a zeroed workspace bit for bit, rows 37.. keep the sentinel.
    P / xyzr allocations and the output buffer have the first call's size, so nothing left over can point outside a buffer."""
    from pointstowood_amd._lib import lib
    big, small = _case((300, 200, 64, 128, 32), 1, "set"), _case(A1, 1, "set")
    name = R.PREC_NAME[prec]
    ldp = R.round_up(64, R.K_GRAN[name])
    ws = torch.zeros(int(lib().p2w_sa_conv_h_ws_bytes(300, flags)), dtype=torch.uint8, device="cuda")
    P_dev = torch.zeros(201, ldp, device="cuda")
    xyzr_dev = torch.zeros(200, 4, device="cuda")
    first = _run(big, prec, flags, ws=ws, P_dev=P_dev, xyzr_dev=xyzr_dev)
    _check_both(big, prec, first, f"/flags{flags}")
    assert bool(ws.any())
    second = _run(small, prec, flags, ws=ws, P_dev=P_dev, xyzr_dev=xyzr_dev, out_rows=300)
    clean = _run(small, prec, flags, out_rows=300)
    assert torch.equal(second["out"][:37].view(torch.int32), clean["out"][:37].view(torch.int32))
    assert torch.equal(second["h_raw"][:37].view(torch.int16), clean["h_raw"][:37].view(torch.int16))
    assert bool(torch.isnan(second["out"][37:]).all()) and bool(torch.isnan(second["h_raw"][37:].float()).all())
    _check_both(small, prec, dict(second, out=second["out"][:37], h=second["h"][:37]), f"/stale{flags}")


# ---- i. range report ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_range_report(prec):
    case = _case(A1)
    words = lambda: torch.zeros(RANGE_WORDS, dtype=torch.int32, device="cuda")
    report = lambda w: (bool(w.view(RANGE_SLOTS, 64)[:, 0].any()), bool(w.view(RANGE_SLOTS, 64)[:, 1].any()))   # (over, seen)
    w = words()
    watched, plain = _run(case, prec, range_words=w), _run(case, prec, rows_api=True)
    assert report(w) == (False, True)
    assert torch.equal(watched["out"].view(torch.int32), plain["out"].view(torch.int32))
    assert torch.equal(watched["h_raw"].view(torch.int16), plain["h_raw"].view(torch.int16))
    assert int(w.view(RANGE_SLOTS, 64)[:, 2:].abs().sum()) == 0            # only the word pairs are written
    hot = case["bn_t"].clone()
    hot[5] = 1e5
    w = words()
    _run(case, prec, range_words=w, bn_t=hot)
    assert report(w) == (True, True)
    nan_t = case["bn_t"].clone()
    nan_t[5] = float("nan")                                               # a NaN output is OVER too (include/p2w.h)
    w = words()
    _run(case, prec, range_words=w, bn_t=nan_t)
    assert report(w)[0]


# ---- j. the fp32 path ----------------------------------------------------------------------------------------------------
def _run_fp32(case):
    from pointstowood_amd import _lib
    from pointstowood_amd._lib import check, lib, ptr, stream
    M, n_src, C1, C2, kw = (case[k] for k in ("M", "n_src", "C1", "C2", "kw"))
    Pp, ldp = R.padded_P(case, "fp32")
    Np, Kp = _lib.packed_dims(C2, C1)
    assert Kp == ldp
    w1r4, W2p = torch.zeros(4, Kp), torch.zeros(Np, Kp)
    w1r4[:, :C1] = case["W1r"]
    W2p[:C2, :C1] = case["W2"]
    d = lambda t: t.cuda().contiguous()
    P, xyzr, w1r4, W2p, idx, bd, sf, nbr, deg, b2, s, t = map(d, (Pp, case["xyzr"], w1r4, W2p, case["idx"], case["batch_dst"], case["sf"],
                                                                 case["nbr"], case["deg"], case["b2"], case["bn_s"], case["bn_t"]))
    out = torch.full((M, C2 + 4), float("nan"), device="cuda")
    check(lib().p2w_sa_conv(ptr(P), ldp, ptr(xyzr), ptr(idx), ptr(bd), ptr(sf), ptr(nbr), ptr(deg), kw, M, ptr(w1r4), ptr(W2p), C1, C2,
                            ptr(b2), ptr(s), ptr(t), ptr(out), C2 + 4, stream()), "p2w_sa_conv")
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool(torch.isnan(out[:, C2:]).all())
    return out[:, :C2].double()


@pytest.mark.parametrize("shape,B,policy", [(A1, 1, "mix"), (A2, 1, "mix"), (A3, 1, "mix")] + [(s, 1, "mix") for s in WIDTH_EDGES] +
                         [(D_SHAPE, B, p) for p, B in POLICIES])
def test_fp32_path(shape, B, policy):
    """p2w_sa_conv on the shapes of (a), the width edges of (c) and the degree policies of (d)."""
    case = _case(shape, B, policy)
    _check(case, "fp32", _run_fp32(case))


# ---- k. determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_two_calls_give_equal_bits(prec):
    case = _case(A2)
    a, b = _run(case, prec), _run(case, prec)
    assert torch.equal(a["out"].view(torch.int32), b["out"].view(torch.int32))
    assert torch.equal(a["h_raw"].view(torch.int16), b["h_raw"].view(torch.int16))
