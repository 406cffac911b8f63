"""The H GEMM family (p2w_gemm_h2, p2w_gemm_h2_sk, p2w_gemm_h2_rowdot) and p2w_gemm called directly and held per element against
tests/gemm_ref.py: every compile-time epilogue class of gemm_epilogue_dispatch16 on every tile form, with interior tiles (the
specialised path) and row- and column-edge tiles (the guarded path) side by side in one launch.

Outputs are allocated 3 rows longer and one K slab wider than the launch writes and filled with NaN.  ``_check`` asserts
  (a) written exactly once: rows < M, columns < N finite; H pad columns up to the slab boundary zero; every other word still NaN,
  (b) cap: |got - reference| <= cap per element on the fp32 output (H-only classes: the decoded H output against the cap + the
      conversion's half ulp),
  (c) accumulation accuracy, raw-accumulator class "128" only: block_rms(got - ref) <= M_RMS * max(block_rms(emulate - ref),
      rms_floor) for every counted 16 x 32 block,
  (e) H conversion pinned: where a launch writes both outputs the H planes equal feat_ref.h_planes(fp32 output) bit for bit,
and the tests add
  (d) specialised vs generic: the same launch with P2W_GEMM_GENERIC_EPI gives the same bits, fp32 and H,
  (f) determinism: a second launch gives the same bits.
Each checked launch prints "GEMM_RATIO <case> <form> <prec> <worst block ratio> <worst cap ratio>" (pytest -s); docs/LAB_NOTES.md holds
the table measured on the MI355X, from which M_RMS is set."""
import ctypes as C

import pytest
import torch

from tests import feat_ref as F
from tests import gemm_ref as R
from tests.h_util import _pack_h, _to_h

pytestmark = pytest.mark.gpu

TILE_128, TILE_256, GENERIC, ORDER_ROWS, ORDER_COLS, RESIDUAL_H, STREAMK, TILE_64, NO_TILE_64 = 1, 2, 4, 8, 16, 32, 64, 1 << 24, 1 << 25
# ("sk": the library prefers the 64 x 128 tile for N <= 192 and K <= 1024 and then plans no split, P2W_GEMM_STREAMK or not: the form
# rules that tile out, so that the forced split-K tail is what runs)
FORM_FLAGS = {"t64": TILE_64, "t128": TILE_128, "t256": TILE_256, "sk": STREAMK | NO_TILE_64, "lib": 0, "dot128": TILE_128,
              "dot256": TILE_256}
# (c): margin on the block RMS against the emulation's.  Twice the worst block ratio measured on the MI355X, rounded up, no lower
# than 2 (docs/LAB_NOTES.md, "GEMM family against fp64").
M_RMS = {0: 5.0, 1: 3.0, 2: 6.0}
PRECS = [0, 1, 2]
NAMES = list(R.EPI_CLASSES)

_cases, _devs = {}, {}


def _case(M, N, K, prec, epi):
    """Cases are built once per module and never modified."""
    key = (M, N, K, prec, epi)
    if key not in _cases:
        if len(_cases) > 40 or M * N > 2_000_000:       # (bounded: a large case is not kept beside the next one)
            _cases.clear()
            _devs.clear()
        _cases[key] = R.make_case(M, N, K, prec, epi, seed=1)
    return _cases[key]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


NAN_BITS = {torch.float32: 0x7FC00000, torch.float16: 0x7E00, torch.bfloat16: 0x7FC0}


def _nan(shape, dtype):
    """The sentinel, on the device: NaN of one fixed bit pattern."""
    return torch.full(shape, NAN_BITS[dtype], dtype=torch.int32 if dtype == torch.float32 else torch.int16, device="cuda").view(dtype)


def _untouched(t, written_rows, written_cols):
    """Every word of t outside [written_rows, written_cols] still holds the sentinel."""
    b = _bits(t).clone()
    if torch.is_tensor(written_cols):
        written_cols = written_cols.to(t.device)
    b[:written_rows, written_cols] = NAN_BITS[t.dtype]
    return bool((b == NAN_BITS[t.dtype]).all())


def _same(a, b):
    return (a is None and b is None) or (a.shape == b.shape and torch.equal(_bits(a), _bits(b)))


def _dev(case):
    """Device operands of a case (the H forms come from the device's own conversion), its operands as the kernel sees them, the
    reference, the cap and the emulation: once per case."""
    key = id(case)
    if key in _devs:
        return _devs[key]
    from pointstowood_amd._lib import check, lib, ptr, stream
    prec, e = case["prec"], R.EPI_CLASSES[case["epi"]]
    d = {}
    dW, wscale, Kp = _pack_h(case["W"], prec)
    w_cpu, ws_cpu, kp_cpu = R.pack_w(case["W"], prec)
    assert _same(dW.cpu(), w_cpu) and wscale == ws_cpu and Kp == kp_cpu == case["Kpad"]
    d.update(W=dW, wscale=wscale, A=_to_h(case["A"], prec, case["ldh_a"]))
    for k in ("bias", "sc0", "sh0", "sc1", "sh1"):
        d[k] = None if case[k] is None else case[k].cuda()
    r_planes = None
    if e.residual == "f32":
        d["R"] = case["R"].cuda()
    elif e.residual == "h":
        d["R"] = _to_h(case["R"], prec, case["ldr"])
        r_planes = d["R"].cpu()
    elif e.residual == "interp":
        ic = case["interp"]
        d["R"] = case["Z"].cuda()
        d["geo"] = [ic[k].cuda() for k in ("xyzr_c", "xyzr_f", "nbr", "deg")]
        d["rec"] = torch.empty((case["M"], 4), dtype=torch.int32, device="cuda")
        check(lib().p2w_interp_weights(*[ptr(t) for t in d["geo"]], 2, case["M"], ptr(d["rec"]), stream()))
    if "dot" in e.outputs:
        d["dotw"] = case["dotw"].cuda()
    ops = R.operands(case, a_planes=d["A"].cpu(), r_planes=r_planes, w_planes=w_cpu)
    ref, cap = R.reference(case, ops)
    d.update(ops=ops, ref=ref, cap=cap, emu=None)
    _devs[key] = d
    return d


def _run(case, form, flags=0, add_f32=False, ldo=None, odd_ldr=False, bias_shift=False, n=None, ws_bytes=None):
    """One launch of `case` on tile form `form` (+ `flags`).  add_f32: an fp32 output beside the class's own.  ldo / odd_ldr /
    bias_shift: a given fp32 pitch, an fp32 residual re-pitched to an odd ldr, the bias vector moved 4 bytes past an 8-byte
    boundary (all three send the launch to the guarded epilogue).  n: launch with the first n < N output columns only.
    ws_bytes: a smaller split-K workspace.  Returns dict(f32, h, dot: device tensors or None; ldo, ldh, hcols, N)."""
    from pointstowood_amd._lib import Epilogue, check, lib, ptr, stream
    L = lib()
    prec, e, M, K = case["prec"], R.EPI_CLASSES[case["epi"]], case["M"], case["K"]
    N = case["N"] if n is None else n
    d = _dev(case)
    ka, planes = R.K_ALIGN[prec], (2 if prec == 0 else 1)
    want_f32, want_h = ("f32" in e.outputs) or add_f32, "h" in e.outputs
    hcols = R.round_up(N, ka)
    ldh = hcols + ka
    ldo = (R.round_up(N, 2) + ka) if ldo is None else ldo
    f32 = _nan((M + 3, ldo), torch.float32) if want_f32 else None
    h = _nan((M + 3, planes * ldh), R.H_DTYPE[prec]) if want_h else None
    res, ldr = d.get("R"), case.get("ldr", 0)
    if odd_ldr:
        assert e.residual == "f32"
        ldr = case["N"] + 1
        res = torch.zeros((M, ldr), device="cuda")
        res[:, :case["N"]] = d["R"][:, :case["N"]]
    bias = d["bias"]
    if bias_shift:
        buf = torch.zeros(case["N"] + 1, device="cuda")
        buf[1:] = d["bias"]
        bias = buf[1:]
        assert bias.data_ptr() % 8 == 4
    interp = e.residual == "interp"
    ep = Epilogue(ptr(bias), ptr(d["sc0"]), ptr(d["sh0"]), ptr(d["sc1"]), ptr(d["sh1"]), ptr(res), ldr, *e.relu, None,
                  ptr(d["rec"]) if interp else None, case["interp"]["n_c"] if interp else 0)
    flags |= FORM_FLAGS[form] | (RESIDUAL_H if e.residual == "h" else 0)
    out = dict(f32=f32, h=h, dot=None, ldo=ldo, ldh=ldh, hcols=hcols, N=N, keep=(res, bias))
    if "dot" in e.outputs:
        need = int(L.p2w_gemm_h2_rowdot_ws_bytes(M, N))
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
        out["dot"] = _nan((M + 3,), torch.float32)
        check(L.p2w_gemm_h2_rowdot(prec, ptr(d["A"]), case["ldh_a"], ptr(d["W"]), d["wscale"], M, N, K, C.byref(ep), ptr(d["dotw"]),
                                   R.DOT_B, ptr(out["dot"]), ptr(ws), need, flags, stream()))
    elif form in ("sk", "lib"):
        ws = _sk_ws()
        check(L.p2w_gemm_h2_sk(prec, ptr(d["A"]), case["ldh_a"], ptr(d["W"]), d["wscale"], M, N, K, C.byref(ep), ptr(f32), ldo, ptr(h), ldh,
                               ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, flags, stream()))
    else:
        check(L.p2w_gemm_h2(prec, ptr(d["A"]), case["ldh_a"], ptr(d["W"]), d["wscale"], M, N, K, C.byref(ep), ptr(f32), ldo, ptr(h), ldh,
                            flags, stream()))
    torch.cuda.synchronize()
    return out


_ws = []


def _sk_ws():
    if not _ws:
        from pointstowood_amd._lib import lib
        _ws.append(torch.empty(int(lib().p2w_gemm_h2_sk_ws_bytes()), dtype=torch.uint8, device="cuda"))
    return _ws[0]


def _raw_cols(prec, ldh, lo, hi):
    """Positions within a raw H row of the columns lo .. hi - 1 (f16x3: both planes of the [hi(32) | lo(32)] blocks)."""
    c = torch.arange(lo, hi)
    if prec != 0:
        return c
    p = 64 * (c // 32) + c % 32
    return torch.cat([p, p + 32])


def _decode(h, prec, ldh):
    hi, lo = R.decode_planes(h, prec, ldh)
    return hi if lo is None else hi + lo


def _assert_same_launch(a, b, what):
    assert _same(a["f32"], b["f32"]), f"{what}: fp32 outputs differ"
    assert _same(a["h"], b["h"]), f"{what}: H outputs differ"
    assert _same(a["dot"], b["dot"]), f"{what}: row-dot outputs differ"


def _check(case, got, form, rms=False, pin=True, tag=""):
    """Assertions (a), (b), (c) with rms = True, (e) with pin = True where both outputs exist.  Prints GEMM_RATIO."""
    prec, M, N = case["prec"], case["M"], got["N"]
    d = _dev(case)
    ref, cap = d["ref"], d["cap"]
    if ref.dim() == 2 and N != case["N"]:
        ref, cap = ref[:, :N], cap[:, :N]
    name = f"{case['epi']}:{M}x{N}x{case['K']}{tag}"
    worst_cap, worst_blk = 0.0, 0.0
    if got["dot"] is not None:
        assert _untouched(got["dot"][None, :], 1, slice(0, M)), "(a) row-dot output"
        v = got["dot"].cpu()
        assert bool(torch.isfinite(v[:M]).all()), "(a) row-dot output"
        err = (v[:M].double() - ref).abs()
        worst_cap = float((err / cap).max())
        assert bool((err <= cap).all()), ("(b)", name, form, worst_cap)
    f32 = None
    if got["f32"] is not None:
        assert _untouched(got["f32"], M, slice(0, N)), "(a) fp32 words outside [M, N] were written"
        f32 = got["f32"][:M, :N].cpu()
        assert bool(torch.isfinite(f32).all()), "(a) an fp32 element was not written or is not finite"
        err = (f32.double() - ref).abs()
        worst_cap = float((err / cap.clamp(min=1e-300)).max())
        assert bool((err <= cap).all()), ("(b)", name, form, worst_cap, int((err > cap).sum()))
        if rms:
            if d["emu"] is None:
                d["emu"] = R.emulate(case, d["ops"]).v
            b_got, counted = R.block_rms(f32.double() - ref)
            b_emu = torch.maximum(R.block_rms(d["emu"][:, :N] - ref)[0], R.rms_floor(ref))
            ratio = torch.where(counted, b_got / b_emu, torch.zeros_like(b_got))
            worst_blk = float(ratio.max())
    if got["h"] is not None:
        ldh, hcols = got["ldh"], got["hcols"]
        own, pad = _raw_cols(prec, ldh, 0, N).cuda(), _raw_cols(prec, ldh, N, hcols).cuda()
        assert bool(torch.isfinite(got["h"][:M][:, own]).all()), "(a) an H element was not written or is not finite"
        assert bool((_bits(got["h"][:M][:, pad]) == 0).all()), "(a) H pad columns up to the slab boundary are not zero"
        assert _untouched(got["h"], M, _raw_cols(prec, ldh, 0, hcols)), "(a) H words outside the launch's columns and rows were written"
        raw = got["h"][:M].cpu()
        if f32 is None:
            err = (_decode(raw, prec, ldh)[:, :N] - ref).abs()
            hc = R.h_cap(case, ref, cap)
            worst_cap = float((err / hc).max())
            assert bool((err <= hc).all()), ("(b) H", name, form, worst_cap, int((err > hc).sum()))
        elif pin:
            cols = _raw_cols(prec, ldh, 0, hcols)
            want = F.h_planes(f32, prec, ldh, hcols=hcols)
            assert _same(raw[:, cols], want[:, cols]), "(e) the H planes are not the pinned conversion of the fp32 output"
    print(f"GEMM_RATIO {name} {form} {R.PREC_NAME[prec]} {worst_blk:.3f} {worst_cap:.4f}")
    if rms:
        assert worst_blk <= M_RMS[prec], ("(c)", name, form, worst_blk)


def _h_only_twice(case, form, first, flags=0):
    """(e) for an H-only class: the same epilogue with an fp32 output added leaves the same H bits, and those are pinned to it."""
    both = _run(case, form, flags, add_f32=True)
    assert _same(first["h"], both["h"]), "the H output changes when an fp32 output is added"
    _check(case, both, form, tag="+f32")


# ----------------------------------------------------------------------------------------------------------------------------
# 1. classes x forms x precisions
# ----------------------------------------------------------------------------------------------------------------------------
SHAPE_1 = {"t64": (150, 192, 100), "t128": (300, 192, 100), "t256": (600, 320, 100), "sk": (300, 192, 256)}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("form", list(SHAPE_1))
@pytest.mark.parametrize("epi", [n for n in NAMES if n != "513"])
def test_every_class_on_every_form(epi, form, prec):
    """(a), (b), (d), (e) for every epilogue class: interior tiles take the specialised code, edge tiles the guarded one."""
    M, N, K = SHAPE_1[form]
    case = _case(M, N, K, prec, epi)
    got = _run(case, form)
    _check(case, got, form)
    _assert_same_launch(got, _run(case, form, GENERIC), "specialised vs generic epilogue")
    if epi in R.H_ONLY:
        _h_only_twice(case, form, got)
    if epi == "2400" and form in ("t64", "t256"):     # the interpolated residual lives in the 128 x 128 kernel: the tile flag is ignored
        _assert_same_launch(got, _run(case, "t128"), "2400 falls back to the 128 x 128 tile")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("form,M,N", [("dot128", 300, 192), ("dot256", 600, 512)])
def test_rowdot_class(form, M, N, prec):
    case = _case(M, N, 100, prec, "513")
    got = _run(case, form)
    _check(case, got, form)
    _assert_same_launch(got, _run(case, form, GENERIC), "specialised vs generic epilogue")
    _assert_same_launch(got, _run(case, form), "second launch")


# ----------------------------------------------------------------------------------------------------------------------------
# 2. K sweep
# ----------------------------------------------------------------------------------------------------------------------------
K_SWEEP = [("t128", K) for K in (4, 32, 36, 64, 96, 100, 516, 1024, 2048)] + [(f, K) for f in ("t64", "t256", "sk") for K in (32, 516)]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("form,K", K_SWEEP)
def test_k_sweep(form, K, prec):
    """(a) - (c): one, two and three slabs per precision, a ragged last slab, the long layers."""
    M, N, _ = SHAPE_1[form]
    for epi in ("128", "287", "1504"):
        case = _case(M, N, K, prec, epi)
        _check(case, _run(case, form), form, rms=epi == "128")


# ----------------------------------------------------------------------------------------------------------------------------
# 3. the persistent walk at the tile boundary
# ----------------------------------------------------------------------------------------------------------------------------
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


WALK = {"t64": (64, 3, 128), "t128": (128, 2, 128), "t256": (256, 1, 256)}        # tile rows, workgroups per CU, N (one column tile)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("nslab", [1, 2, 3])
@pytest.mark.parametrize("form,epi", [(f, c) for f in WALK for c in ("128", "387", "287", "residual", "2400") if c != "2400" or f == "t128"])
def test_persistent_walk(form, epi, nslab, prec):
    """Every workgroup walks at least three tiles of the fewest slabs: the counted wait behind a specialised epilogue is what the
    next tile's first barrier relies on (with one slab the next tile's prefetch is issued inside the tile's only slab).  (a), (b),
    (d), (f) per class ("residual": 1504 in f16x3, the fp32-residual 480 in the single-plane modes; 2400 on its own kernel, the 128 x
    128 one), (c) on the raw accumulators; the other tile order must give the same bits as the one that was checked."""
    bm, per_cu, N = WALK[form]
    M = (3 * per_cu * _cus() + 5) * bm - 3                     # 3 x slots + 5 tiles, the last one cut by M
    K = nslab * (32 if prec == 0 else 64)
    if epi == "residual":
        epi = "1504" if prec == 0 else "480"
    case = _case(M, N, K, prec, epi)
    got = _run(case, form, ORDER_ROWS)
    _check(case, got, form, rms=epi == "128", pin=False, tag=f":{nslab}slab")
    _assert_same_launch(got, _run(case, form, ORDER_ROWS), "second launch")
    _assert_same_launch(got, _run(case, form, ORDER_ROWS | GENERIC), "specialised vs generic epilogue")
    _assert_same_launch(got, _run(case, form, ORDER_COLS), "columns order vs rows order")
    _assert_same_launch(got, _run(case, form, ORDER_COLS | GENERIC), "columns order, generic epilogue")


# ----------------------------------------------------------------------------------------------------------------------------
# 4. tile orders and grids
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("order", [ORDER_ROWS, ORDER_COLS])
@pytest.mark.parametrize("ntiles", [1, 2, 3, 4, 8, 9])
def test_tile_orders_and_grids(ntiles, order, prec):
    """Every tile is visited exactly once ((a)) in both orders: 3 column tiles take the rows order whatever is asked, 9 leave the
    last XCD slice with an empty slot."""
    case = _case(128 * 11 + 7, 128 * ntiles - 2, 64, prec, "131")
    _check(case, _run(case, "t128", order), "t128", tag=f":order{order}")


# ----------------------------------------------------------------------------------------------------------------------------
# 5. split-K plans
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("nslab", [2, 3, 7, 33])
@pytest.mark.parametrize("M", [5, 300, 2100])
def test_split_k_plans(M, nslab, prec):
    """Uneven piece boundaries j nslab / S (and S = nslab), with the full workspace and with one of exactly two pieces (N = 128: one
    column tile, so that two pieces are a plan).  (a), (b), (d), (f); against p2w_gemm_h2 the bound of test_gemm_h_stream_k_tail."""
    K = nslab * (32 if prec == 0 else 64)
    rel = {0: 2.0 ** -21, 1: 2.0 ** -11, 2: 2.0 ** -8}[prec]
    for N, ws_bytes in ((192, None), (128, 2 * 128 * 128 * 4)):
        for epi in ("287", "1376", "1504", "2400"):
            case = _case(M, N, K, prec, epi)
            got = _run(case, "sk", ws_bytes=ws_bytes)
            _check(case, got, "sk", tag=f":{nslab}slab:ws{'2' if ws_bytes else 'full'}")
            _assert_same_launch(got, _run(case, "sk", ws_bytes=ws_bytes), "second launch")
            _assert_same_launch(got, _run(case, "sk", GENERIC, ws_bytes=ws_bytes), "specialised vs generic epilogue")
            plain = _run(case, "t128")
            scale = max(1.0, float(_dev(case)["ref"].abs().max()))
            bound = 4e-6 * scale * (K / 512) ** 0.5 + 1e-7          # the K range summed in pieces: last fp32 bits only
            if got["f32"] is not None:
                assert float((got["f32"][:M, :N] - plain["f32"][:M, :N]).abs().max()) <= bound
            else:                                                   # (H only: + the two conversions' half ulps)
                a, b = (_decode(t["h"][:M].cpu(), prec, got["ldh"])[:, :N] for t in (got, plain))
                assert float((a - b).abs().max()) <= bound + 2 * rel * scale


# ----------------------------------------------------------------------------------------------------------------------------
# 6. fallbacks to the guarded path
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("form", ["t64", "t128"])
@pytest.mark.parametrize("epi", ["287", "224"])
def test_fallbacks_to_the_guarded_path(epi, form, prec):
    """A misaligned bias vector, an odd fp32 pitch, an odd residual pitch and an odd N each send an otherwise interior-eligible
    launch (M = 256, N = 128) to the guarded epilogue: within the cap, and the bits of the aligned launch."""
    case = _case(256, 130, 100, prec, epi)
    wide = _run(case, form)
    _check(case, wide, form)                                        # N = 130: one column pair in the edge tile
    ok = _run(case, form, n=128)
    _check(case, ok, form)
    first = lambda t, k: None if t[k] is None else t[k][:256, :128 if k == "f32" else (256 if prec == 0 else 128)]
    for what, kw in (("bias 4 bytes past an 8-byte boundary", dict(bias_shift=True)), ("N = 129", dict(n=129)), ("N = 130", {}),
                     ("odd ldo", dict(ldo=128 + 65)), ("odd ldr", dict(odd_ldr=True))):
        if (what == "odd ldo" and "f32" not in R.EPI_CLASSES[epi].outputs) or (what == "odd ldr" and R.EPI_CLASSES[epi].residual != "f32"):
            continue
        got = _run(case, form, n=kw.pop("n", 130 if what == "N = 130" else 128), **kw)
        _check(case, got, form, tag=":" + what.replace(" ", "_"))
        for k in ("f32", "h"):       # (columns 0 .. 127: one [hi | lo] block layout for every N here, the same row prefix)
            if got[k] is not None:
                assert torch.equal(_bits(first(got, k)), _bits(first(ok, k))), (what, k)


# ----------------------------------------------------------------------------------------------------------------------------
# 7. the network's layers at reduced M, tile, order and plan chosen by the library
# ----------------------------------------------------------------------------------------------------------------------------
# (the level-3 shapes; the plan depends on the shape alone, so one class per shape where two share it and the fp64 reference is long)
LEVEL3 = [(n, k, c) for n, k, c in R.LAYERS_C32 if (n, k) in ((2048, 512), (2048, 2048), (512, 2048), (512, 515), (768, 512), (512, 768))
          and (n, k, c) != (2048, 2048, "257")]


def _layer(M, N, K, epi, prec):
    case = _case(M, N, K, prec, epi)
    form = "dot128" if epi == "513" else "lib"
    got = _run(case, form)
    _check(case, got, form)
    if epi in R.H_ONLY:
        _h_only_twice(case, form, got)


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("N,K,epi", R.LAYERS_C32)
def test_layers_c32(N, K, epi, prec):
    _layer(300, N, K, epi, prec)


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("N,K,epi", LEVEL3)
def test_layers_c32_level3_rows(N, K, epi, prec):
    """17 506 rows: the planner takes its own split-K and 64 x 128 decisions."""
    _layer(17506, N, K, epi, prec)


# ----------------------------------------------------------------------------------------------------------------------------
# 8. the fp32 engine
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", ["all_on", "224", "none"])
@pytest.mark.parametrize("M,N,K", [(1, 4, 4), (129, 8, 36), (1000, 192, 128), (4097, 512, 2048), (300, 640, 768), (77, 100, 516)])
def test_fp32_engine(M, N, K, epi):
    """p2w_gemm through the same (a) and (b): reference from the fp32 operands, u = 2^-24 per product and per addition."""
    from pointstowood_amd import _lib
    from pointstowood_amd._lib import Epilogue, check, lib, ptr, stream
    case = R.make_case(M, N, K, "fp32", epi, seed=1)
    e = R.EPI_CLASSES[epi]
    ref, cap = R.reference(case)
    Np, Kp = _lib.packed_dims(N, K)
    assert Kp == case["Kpad"]
    Wp = torch.zeros(Np, Kp)
    Wp[:N, :K] = case["W"]
    dev = lambda t: None if t is None else t.cuda().contiguous()
    dA, dW = dev(case["A"]), dev(Wp)
    vec = {k: dev(case[k]) for k in ("bias", "sc0", "sh0", "sc1", "sh1")}
    dR = dev(case["R"]) if e.residual else None
    ldo = N + 32
    out = _nan((M + 3, ldo), torch.float32)
    ep = Epilogue(ptr(vec["bias"]), ptr(vec["sc0"]), ptr(vec["sh0"]), ptr(vec["sc1"]), ptr(vec["sh1"]), ptr(dR), case.get("ldr", 0), *e.relu)
    check(lib().p2w_gemm(ptr(dA), case["A"].shape[1], ptr(dW), M, N, K, C.byref(ep), ptr(out), ldo, stream()))
    got = out[:M, :N].cpu()
    assert bool(torch.isfinite(got).all()) and _untouched(out, M, slice(0, N))
    err = (got.double() - ref).abs()
    worst = float((err / cap.clamp(min=1e-300)).max())
    print(f"GEMM_RATIO {epi}:{M}x{N}x{K} p2w_gemm fp32 0.000 {worst:.4f}")
    assert bool((err <= cap).all()), (worst, int((err > cap).sum()))
