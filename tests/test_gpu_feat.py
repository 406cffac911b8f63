"""The small feature and geometry kernels, each called through the C ABI and held against tests/feat_ref.py: the fp32 results
within the caps derived there from the float64 reference, the H planes bit for bit the exact conversion of the fp32 result, the
exact operators bit for bit.  Every output is prefilled with a sentinel (NaN, or 3.0 where the call must leave it alone).
Each comparison with a cap prints ``FEAT_RATIO <kernel> <case> <precision> <worst err / cap>`` (docs/LAB_NOTES.md holds the table)."""
import pytest
import torch

from tests import feat_ref as R
from tests.h_util import _from_h

pytestmark = pytest.mark.gpu

PLANES = {0: 2, 1: 1, 2: 1}
HDT = {0: torch.float16, 1: torch.float16, 2: torch.bfloat16}


def _abi():
    from pointstowood_amd._lib import check, lib, ptr, stream
    return lib(), check, ptr, stream


def _dev(t):
    return None if t is None else t.cuda().contiguous()


def _h_sentinel(rows, prec, ldh, fill=3.0):
    return torch.full((rows, PLANES[prec] * ldh), fill, dtype=HDT[prec], device="cuda")


def _ratio(got, ref, cap):
    """Worst |got - ref| / cap (cap 0: the element must be exact); NaN counts as inf."""
    err = (got.double() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    safe = torch.where(cap > 0, cap, torch.ones_like(cap))
    r = torch.where(cap > 0, err / safe, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


def _report(kernel, case, prec, ratio):
    print(f"FEAT_RATIO {kernel} {case} {prec} {ratio:.3f}")


def _wide(prec, pad):
    """A row pitch wider than the slab pad (f16x3 rows come in blocks of 32 columns, the others need a multiple of 8)."""
    return pad + (32 if prec == 0 else 8)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("n,C", R.STEM_CASES)
def test_stem_all_entry_points(n, C, prec):
    """p2w_stem, p2w_stem_h2 (fp32 only / H only / both; ldh = the slab pad and wider) and p2w_stem_h2_indexed on records from
    p2w_index_records with a random permutation (fp32 row .w, H row i)."""
    L, check, ptr, stream = _abi()
    case = R.stem_case(n, C)
    ref, cap = R.stem_reference(case)
    x, w, b = _dev(case["xyzr"]), _dev(case["w"]), _dev(case["b"])
    out0 = torch.full((n * C + 8,), float("nan"), device="cuda")
    out0[n * C:] = 3.0
    check(L.p2w_stem(ptr(x), n, ptr(w), ptr(b), C, ptr(out0), stream()))
    assert bool((out0[n * C:] == 3.0).all())
    o0 = out0[:n * C].view(n, C).cpu()
    ratio = _ratio(o0, ref, cap)
    if prec == 0:                                                                    # (p2w_stem has no precision: one table row)
        _report("stem", f"n={n},C={C}", "fp32", ratio)
    assert ratio <= 1.0
    assert n == 1 or bool((o0 == 0).any())                                           # ReLU zeros occur
    pad = R.round_up(C, R.K_ALIGN[prec])
    g = torch.Generator().manual_seed(n + C)
    perm = torch.randperm(n, generator=g).to(torch.int32)
    rec = torch.full((n, 4), float("nan"), device="cuda")
    dperm, dptr = _dev(perm), _dev(torch.tensor([0, n], dtype=torch.int32))
    check(L.p2w_index_records(ptr(x), ptr(dperm), ptr(dptr), 1, n, ptr(rec), stream()))
    for ldh in (pad, _wide(prec, pad)):
        hcols = R.hcols_of(prec, C, ldh)
        want_h = R.h_planes(o0, prec, ldh, hcols=hcols, fill=3.0)
        want_hp = R.h_planes(o0[perm.long()], prec, ldh, hcols=hcols, fill=3.0)
        for f32, h in ((True, False), (False, True), (True, True)):
            for indexed in (False, True):
                o = torch.full((n * C + 8,), float("nan"), device="cuda") if f32 else None
                if f32:
                    o[n * C:] = 3.0
                oh = _h_sentinel(n + 1, prec, ldh) if h else None
                fn = L.p2w_stem_h2_indexed if indexed else L.p2w_stem_h2
                check(fn(prec, ptr(rec if indexed else x), n, ptr(w), ptr(b), C, ptr(o), ptr(oh), ldh, None, stream()))
                tag = (n, C, prec, ldh, f32, h, indexed)
                if f32:
                    assert R.same_bits(o[:n * C].view(n, C).cpu(), o0), tag          # the same kernel arithmetic: the same bits
                    assert bool((o[n * C:] == 3.0).all()), tag
                if h:
                    assert R.same_bits(oh[:n].cpu(), want_hp if indexed else want_h), tag
                    assert bool((oh[n:] == 3.0).all()), tag                          # nothing behind the last row


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Fs", [0, R.INTERP_FS])
@pytest.mark.parametrize("Fc,kw", R.INTERP_CASES)
def test_interp_concat_fp32_and_h(Fc, kw, Fs):
    """p2w_interp_concat within the cap element by element (degrees 0 .. kw and beyond, coincident neighbours, the two-chunk fast
    path and its tail, skip copy exact, zero fill to ldo) and p2w_interp_concat_h2 = the exact conversion of the fp32 twin's
    output (pad zero, columns beyond the pad untouched; Fs = 0: skip = NULL into wider rows)."""
    L, check, ptr, stream = _abi()
    case = R.interp_case(Fc, kw)
    ref, cap = R.interp_reference(case)
    m = case["m"]
    xc, pc, pf, nbr, deg = (_dev(case[k]) for k in ("xc", "xyzr_c", "xyzr_f", "nbr", "deg"))
    skip = _dev(case["skip"]) if Fs else None
    W = Fc + Fs
    outs = []
    for ldo in (W, W + 8):
        out = torch.full((m + 1, ldo), float("nan"), device="cuda")
        out[m:] = 3.0
        check(L.p2w_interp_concat(ptr(xc), Fc, ptr(pc), ptr(pf), ptr(nbr), ptr(deg), kw, ptr(skip), Fs, m, ptr(out), ldo, stream()))
        o = out.cpu()
        assert bool((o[m:] == 3.0).all())
        assert bool((o[:m, W:] == 0).all())                                          # rows are zero-filled up to ldo
        if Fs:
            assert R.same_bits(o[:m, Fc:W].contiguous(), case["skip"])               # the skip copy is exact
        outs.append(o[:m, :W].contiguous())
    assert R.same_bits(outs[0], outs[1])
    ratio = _ratio(outs[0][:, :Fc], ref, cap)
    _report("interp_concat", f"Fc={Fc},kw={kw},Fs={Fs}", "fp32", ratio)
    assert ratio <= 1.0
    d = case["deg"].long().clamp(max=kw)
    assert bool((outs[0][d == 0, :Fc] == 0).all())
    for prec in (0, 1, 2):
        pad = R.round_up(W, R.K_ALIGN[prec])
        for ldh in (pad, _wide(prec, pad), pad + 64):
            oh = _h_sentinel(m + 1, prec, ldh)
            check(L.p2w_interp_concat_h2(prec, ptr(xc), Fc, ptr(pc), ptr(pf), ptr(nbr), ptr(deg), kw, ptr(skip), Fs, m, ptr(oh), ldh,
                                         stream()))
            want = R.h_planes(outs[0], prec, ldh, hcols=R.hcols_of(prec, W, ldh), fill=3.0)
            assert R.same_bits(oh[:m].cpu(), want), (Fc, kw, Fs, prec, ldh)
            assert bool((oh[m:] == 3.0).all())


@pytest.mark.parametrize("kw", [1, 2])
def test_interp_weights_values(kw):
    """The records of p2w_interp_weights on their own: n0, n1 exact, a_s within (2 d + 12) u relative of float64, one-neighbour
    rows exactly {n0, n0, 1, 0}, rows without a neighbour a0 = a1 = 0; kw = 3 is refused."""
    L, check, ptr, stream = _abi()
    case = R.interp_case(24, kw)
    m = case["m"]
    n0, n1, a, cap = R.interp_weights_reference(case)
    pc, pf, nbr, deg = (_dev(case[k]) for k in ("xyzr_c", "xyzr_f", "nbr", "deg"))
    rec = torch.full((m + 1, 4), -7, dtype=torch.int32, device="cuda")
    check(L.p2w_interp_weights(ptr(pc), ptr(pf), ptr(nbr), ptr(deg), kw, m, ptr(rec), stream()))
    r = rec.cpu()
    assert bool((r[m] == -7).all())
    got = r[:m, 2:].contiguous().view(torch.float32).double()
    d = case["deg"].long().clamp(max=kw)
    has = d > 0
    assert torch.equal(r[:m, 0][has].long(), n0[has]) and torch.equal(r[:m, 1][has].long(), n1[has])
    rel = (got - a).abs() / torch.where(a > 0, a, torch.ones_like(a))
    ratio = float((rel / cap.clamp(min=R.U)[:, None]).max())
    _report("interp_weights", f"kw={kw}", "fp32", ratio)
    assert ratio <= 1.0
    assert bool((got[d == 1] == torch.tensor([1.0, 0.0], dtype=torch.float64)).all()) and bool((got[d == 0] == 0).all())
    assert int((d == 0).sum()) > 10 and int((d == 1).sum()) > 10
    nbr3 = torch.zeros((m, 3), dtype=torch.int32, device="cuda")
    assert L.p2w_interp_weights(ptr(pc), ptr(pf), ptr(nbr3), ptr(deg), 3, m, ptr(rec), stream()) == -5      # P2W_EUNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,m,kind", [(F, m, "randn") for F, m in R.CONCAT_CASES] + [(60, 300, "tiny"), (60, 300, "huge")],
                         ids=lambda v: str(v))
def test_concat_xyz_fp32_and_h_exact(F, m, kind):
    """p2w_concat_xyz and p2w_concat_xyz_h2, exact: [x | xyz | zeros], the record's .w nowhere; H = the exact conversion, also
    where the f16x3 lo plane and the single fp16 plane are subnormal ("tiny") and beyond 65504 ("huge")."""
    L, check, ptr, stream = _abi()
    case = R.concat_case(F, m, kind)
    x, p = _dev(case["x"]), _dev(case["xyzr"])
    for ldo in (F + 4, F + 12):
        out = torch.full((m + 1, ldo), float("nan"), device="cuda")
        out[m:] = 3.0
        check(L.p2w_concat_xyz(ptr(x), F, ptr(p), m, ptr(out), ldo, stream()))
        o = out.cpu()
        assert R.same_bits(o[:m].contiguous(), R.concat_reference(case, ldo)), (F, m, ldo)
        assert bool((o[:m, F + 3] == 0).all()) and bool((o[m:] == 3.0).all())        # .w = 7.0 does not leak
    for prec in (0, 1, 2):
        base = R.round_up(F + 4, 32 if prec == 0 else 8)
        for ldh in (base, base + 32):
            oh = _h_sentinel(m + 1, prec, ldh)
            check(L.p2w_concat_xyz_h2(prec, ptr(x), F, ptr(p), m, ptr(oh), ldh, stream()))
            want = R.h_planes(R.concat_reference(case, ldh), prec, ldh)               # the whole row is written: zero tail
            assert R.same_bits(oh[:m].cpu(), want), (F, m, kind, prec, ldh)
            assert bool((oh[m:] == 3.0).all())
            if kind == "huge":
                assert bool(torch.isfinite(_from_h(oh[:m], prec, ldh)).all())


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("F", R.SEG_F)
def test_segment_max_exact(F, pad):
    """p2w_segment_max bit-equal to the float64 reference: segments shorter than the 16-way row split, empty ones (= 0), F % 64
    != 0, ldx > F (NaN in the pad columns), all-negative columns, -inf / +inf, a maximum in the segment's last row."""
    L, check, ptr, stream = _abi()
    cases = [R.segment_case(F, pad)]
    if F in (1, 65):
        cases.append(R.segment_case(F, pad, lengths=[(7 * i) % 41 for i in range(700)]))
    for case in cases:
        x, p = _dev(case["x"]), _dev(case["ptr"])
        B = case["B"]
        out = torch.full((B * F + 8,), float("nan"), device="cuda")
        out[B * F:] = 3.0
        check(L.p2w_segment_max(ptr(x), case["ldx"], F, ptr(p), B, ptr(out), stream()))
        o = out.cpu()
        assert bool((o[B * F:] == 3.0).all())
        assert R.segment_max_matches(o[:B * F].view(B, F), R.segment_max_reference(case)), (F, pad, B)


def test_rowdot_within_cap():
    """p2w_rowdot at F below, at and above one 256-column sweep, ldx = F and wider, one row, a partial and many workgroups."""
    L, check, ptr, stream = _abi()
    for F, ldx, m in R.ROWDOT_CASES:
        case = R.rowdot_case(F, ldx, m)
        ref, cap = R.rowdot_reference(case)
        x, w = _dev(case["x"]), _dev(case["w"])
        out = torch.full((m + 4,), float("nan"), device="cuda")
        out[m:] = 3.0
        check(L.p2w_rowdot(ptr(x), ldx, F, ptr(w), case["b"], m, ptr(out), stream()))
        o = out.cpu()
        assert bool((o[m:] == 3.0).all())
        ratio = _ratio(o[:m], ref, cap)
        _report("rowdot", f"F={F},ldx={ldx},m={m}", "fp32", ratio)
        assert ratio <= 1.0, (F, ldx, m)


@pytest.mark.parametrize("stride,refl,n", R.PACK_CASES)
def test_pack_xyzr_exact(stride, refl, n):
    L, check, ptr, stream = _abi()
    case = R.pack_case(stride, refl, n)
    want_x, want_b = R.pack_reference(case)
    pos, r, p = _dev(case["pos"]), _dev(case["refl"]), _dev(case["ptr"])
    xyzr = torch.full((n + 1, 4), 3.0, device="cuda")
    batch = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
    check(L.p2w_pack_xyzr(ptr(pos), stride, ptr(r), ptr(p), case["B"], n, ptr(xyzr), ptr(batch), stream()))
    assert R.same_bits(xyzr[:n].cpu(), want_x) and torch.equal(batch[:n].cpu(), want_b)
    assert bool((xyzr[n:] == 3.0).all()) and int(batch[n]) == -7


def test_level_gather_exact():
    """p2w_level_gather: ((p / sf_b) * sf_b, refl) of src[idx[i]], bit-equal to the CPU's fp32 arithmetic; rows from ptr[B] on stay
    untouched (m_bound > ptr[B])."""
    L, check, ptr, stream = _abi()
    case = R.level_case()
    want = R.level_reference(case)
    m, bound = case["m"], case["bound"]
    src, idx, batch, p, sf = (_dev(case[k]) for k in ("src", "idx", "batch", "ptr", "sf"))
    dst = torch.full((bound, 4), 3.0, device="cuda")
    check(L.p2w_level_gather(ptr(src), ptr(idx), ptr(batch), ptr(p), case["B"], bound, ptr(sf), ptr(dst), stream()))
    d = dst.cpu()
    assert R.same_bits(d[:m].contiguous(), want)
    assert bool((d[m:] == 3.0).all())
    plain = case["src"][case["idx"][:m].long()]
    v0 = case["batch"][:m] == 0
    assert bool((d[:m][v0, :3] != plain[v0, :3]).any())                               # sf = 0.37: the round trip is not an identity
    assert bool((d[:m][~v0] == plain[~v0]).all())                                     # sf = 3.0: it provably is (tests/feat_ref.py)


@pytest.mark.parametrize("m", [1, 1000])
def test_fill_batch_nbr_exact(m):
    L, check, ptr, stream = _abi()
    batch = torch.randint(0, 50, (m,), generator=torch.Generator().manual_seed(m), dtype=torch.int32)
    db = _dev(batch)
    nbr = torch.full((m + 1,), -7, dtype=torch.int32, device="cuda")
    deg = torch.full((m + 1,), -7, dtype=torch.int32, device="cuda")
    check(L.p2w_fill_batch_nbr(ptr(db), m, ptr(nbr), ptr(deg), stream()))
    assert torch.equal(nbr[:m].cpu(), batch) and bool((deg[:m] == 1).all()) and int(nbr[m]) == -7 and int(deg[m]) == -7
