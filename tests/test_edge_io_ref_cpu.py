"""What of the 16-bit route of edge_layer1 (include/p2w.h: p2w_edge_l1_io / p2w_edge_l1_bwd_io) can be checked without a GPU: the
planted table of tests/edge_io_ref.py against torch's conversions on the CPU, that the table separates a recomputed mask from one read
back from the stored 16-bit H1, and the refusals of the two entry points, which return before a launch."""
import numpy as np

from tests import edge_io_ref as R

EINVAL, ENULL, EALIGN, EWORKSPACE, EUNSUPPORTED = -1, -2, -3, -4, -5
F32, F16, BF16 = 0, 1, 2
A = 0x10000            # a 16-byte aligned address that is never followed: every call below is refused before a launch


def test_table_patterns_are_torchs_conversions():
    """Every fp32 entry of the table stores as the float16 / bfloat16 pattern written beside it; the entries the route's design rests
    on are spelled out once more by value."""
    assert np.array_equal(R.store_bits(R.TABLE32, "f16"), R.TABLE_F16)
    assert np.array_equal(R.store_bits(R.TABLE32, "bf16"), R.TABLE_BF16)
    f = lambda v, k: int(R.store_bits(np.array([v], dtype=np.float32), k)[0])      # noqa: E731
    b = lambda u, k: int(R.store_bits(np.array([u], dtype=np.uint32).view(np.float32), k)[0])      # noqa: E731
    for v in (2.0 ** -25, 2.0 ** -26, 1e-30, 1e-40):
        assert f(v, "f16") == 0x0000, v
    assert f(np.nextafter(np.float32(2.0 ** -25), np.float32(1)), "f16") == 0x0001 and f(2.0 ** -24, "f16") == 0x0001
    assert f(65519.996, "f16") == 0x7BFF and f(65520.0, "f16") == 0x7C00
    assert f(1e-44, "bf16") == 0x0000 and f(1e-40, "bf16") == 0x0001
    assert b(0x7F7F8000, "bf16") == 0x7F80 and b(0x7F7F7FFF, "bf16") == 0x7F7F
    assert bool((R.TABLE32 > 0).all())
    extra = R.PLANTED32[len(R.TABLE):]
    assert np.signbit(extra[0]) and extra[0] == 0 and extra[1] < 0 and np.isnan(extra[2]) and np.isposinf(extra[3])


def test_table_separates_the_recomputed_mask_from_the_stored_one():
    """On the planted case the fp32 h of the planted columns is P itself.  float16: at least four planted values are > 0 in fp32 and
    store as zero; bfloat16: at least one.  The two restatements of the backward differ in gP exactly at those elements - the
    recomputed mask passes the gradient on, the stored one drops it - and agree everywhere else."""
    c = R.planted_case(8)
    g = np.random.default_rng(5)
    geo = g.random((c["E"], 4), dtype=np.float32)
    gH = (g.random((c["E"], 8), dtype=np.float32) + 0.5)                   # no zero gradient: a dropped element shows
    args = (gH, c["P"].numpy(), geo, c["src"].numpy(), c["Wg"].numpy(), c["n_src"])
    h = R.h_fp32(*args[1:])
    j = c["src"].numpy().astype(np.int64)
    for col in c["cols"]:
        want = c["P"].numpy()[j, col]
        want = np.where(want > 0, want, np.float32(0))
        assert np.array_equal(h[:, col].view(np.uint32) & 0x7FFFFFFF, want.view(np.uint32) & 0x7FFFFFFF)       # h = relu(P[j, c]) exactly
    ref = R.backward(*args)
    for kind, least in (("f16", 4), ("bf16", 1)):
        lost = (h > 0) & (R.stored(h, kind) == 0)                         # [E, C1]
        assert int(lost[:, list(c["cols"])].sum()) >= 2 * least and not lost[:, [0, 3, 4, 5, 6, 7]].any()
        bad = R.backward(*args, mask_from=kind)
        lost_rows = np.zeros_like(lost)
        lost_rows[j] = lost                                                # by source: every source has exactly one edge
        assert np.array_equal(ref[0] != bad[0], lost_rows)
        by_source = np.zeros_like(ref[0])
        by_source[j] = gH
        assert np.array_equal(ref[0][lost_rows], by_source[lost_rows])     # the recomputed mask carries the gradient there
        assert bool((bad[0][lost_rows] == 0).all())
        assert not np.array_equal(ref[2], bad[2])                          # gWg loses the same terms
    # an edge whose source is outside [0, n_src) enters nothing, whatever its gradient
    src = c["src"].numpy().copy()
    src[3] = c["n_src"] + 2
    gH2 = gH.copy()
    gH2[3] = np.inf
    out = R.backward(gH2, c["P"].numpy(), geo, src, c["Wg"].numpy(), c["n_src"])
    assert all(bool(np.isfinite(t).all()) for t in out)


def test_io_entry_points_refuse_before_a_launch():
    """Unknown dtype codes (3 and -1) give P2W_EUNSUPPORTED ahead of every other check; with a known code the namesakes' refusals:
    sizes and pitches (-1), null pointers (-2), pitches and pointers that the 4-column lanes cannot take - 16 bytes for fp32, 8 for a
    16-bit H1 / gH - (-3), a workspace that is too small (-4).  No GPU is needed: nothing is launched."""
    from pointstowood_amd._lib import lib
    L = lib()
    n, M, E, C1 = 12, 5, 14, 8
    need = int(L.p2w_edge_l1_bwd_ws_bytes(E, n, C1))
    assert need > 0

    def fwd(th, P=A, ldp=C1, rs=A, rd=A, csr=A, src=A, Wg=A, n_=n, M_=M, E_=E, C1_=C1, geo=A, H1=A, ldh=C1):
        return L.p2w_edge_l1_io(P, ldp, rs, rd, csr, src, Wg, n_, M_, E_, C1_, geo, H1, th, ldh, None)

    def bwd(tg, gH=A, ldg=C1, P=A, ldp=C1, geo=A, src=A, Wg=A, n_=n, E_=E, C1_=C1, gP=A, ldgp=C1, gR=A, gWg=A, ws=A, wsb=need):
        return L.p2w_edge_l1_bwd_io(gH, tg, ldg, P, ldp, geo, src, Wg, n_, E_, C1_, gP, ldgp, gR, gWg, ws, wsb, None)

    for code in (3, -1):
        assert fwd(code) == EUNSUPPORTED and bwd(code) == EUNSUPPORTED
        assert fwd(code, H1=None) == EUNSUPPORTED and fwd(code, C1_=0) == EUNSUPPORTED and fwd(code, ldh=C1 + 1) == EUNSUPPORTED
        assert bwd(code, gH=None) == EUNSUPPORTED and bwd(code, ldg=1) == EUNSUPPORTED and bwd(code, wsb=0) == EUNSUPPORTED
    for t in (F32, F16, BF16):
        for name in ("P", "rs", "rd", "csr", "src", "Wg", "geo", "H1"):
            assert fwd(t, **{name: None}) == ENULL, (t, name)
        for name in ("gH", "P", "geo", "src", "Wg", "gP", "gR", "gWg", "ws"):
            assert bwd(t, **{name: None}) == ENULL, (t, name)
        assert fwd(t, ldp=C1 - 4) == EINVAL and fwd(t, ldh=4) == EINVAL and fwd(t, C1_=0) == EINVAL
        assert fwd(t, n_=-1) == EINVAL and fwd(t, M_=-1) == EINVAL and fwd(t, E_=-1) == EINVAL and fwd(t, M_=0) == EINVAL and fwd(t, n_=0) == EINVAL
        assert fwd(t, M_=0, E_=0) == 0 and fwd(t, E_=0) == 0                                 # nothing to do: nothing launched
        assert fwd(t, ldp=C1 + 2) == EALIGN and fwd(t, ldh=C1 + 1) == EALIGN
        assert fwd(t, P=A + 4) == EALIGN and fwd(t, Wg=A + 8) == EALIGN and fwd(t, rs=A + 4) == EALIGN and fwd(t, rd=A + 8) == EALIGN
        assert fwd(t, geo=A + 4) == EALIGN and fwd(t, H1=A + 4) == EALIGN and fwd(t, H1=A + 2) == EALIGN
        assert bwd(t, ldg=4) == EINVAL and bwd(t, ldp=C1 - 4) == EINVAL and bwd(t, ldgp=4) == EINVAL and bwd(t, C1_=0) == EINVAL
        assert bwd(t, n_=-1) == EINVAL and bwd(t, E_=-1) == EINVAL and bwd(t, n_=0) == EINVAL
        assert bwd(t, ldg=C1 + 2) == EALIGN and bwd(t, ldp=C1 + 1) == EALIGN and bwd(t, ldgp=C1 + 3) == EALIGN
        assert bwd(t, gH=A + 4) == EALIGN and bwd(t, P=A + 8) == EALIGN and bwd(t, Wg=A + 4) == EALIGN and bwd(t, gP=A + 4) == EALIGN
        assert bwd(t, gWg=A + 4) == EALIGN and bwd(t, geo=A + 4) == EALIGN and bwd(t, ws=A + 8) == EALIGN
        assert bwd(t, wsb=need - 1) == EWORKSPACE and bwd(t, wsb=0) == EWORKSPACE
    # the 4-column lanes of a 16-bit tensor take an 8-byte aligned base, those of an fp32 tensor need 16; C1 = 6 asks for neither
    assert fwd(F32, H1=A + 8) == EALIGN and bwd(F32, gH=A + 8) == EALIGN
    for t in (F16, BF16):
        assert bwd(t, gH=A + 8, wsb=0) == EWORKSPACE                       # past the alignment checks
    assert bwd(F32, C1_=6, ldg=7, ldp=6, ldgp=9, gH=A + 4, P=A + 4, gP=A + 4, gWg=A + 4, Wg=A + 4, wsb=0) == EWORKSPACE
    assert bwd(F16, C1_=6, ldg=7, ldp=6, ldgp=9, gH=A + 2, wsb=0) == EWORKSPACE
