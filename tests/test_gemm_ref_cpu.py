"""tests/gemm_ref.py on its own (no GPU): the emulation stays inside the hard cap for every class, precision and K of
tests/test_gpu_gemm.py's matrix, the criteria of that file are sharp - every mutant of the emulation leaves the cap or the
block-RMS margin - and the class list and the layer table agree with the kernel source, the engine and the checkpoint layout.

Why there are two criteria.  The hard cap is a worst-case bound, linear in K; the kernel's real error grows like sqrt(K).  A fault
the size of an operand's low part - the a_lo w_hi term of f16x3 lost, entirely or in the last K slab only - stays INSIDE the cap at
long K (measured here at 256 x 256: worst |error| / cap 0.2 - 0.6 for the whole term at K = 1024), so the cap alone does not catch
it.  The RMS of the error over a 16 x 32 block does: the mutants raise it by two to three orders of magnitude (figures printed by
test_a_lost_lo_term_is_far_outside_the_rms_margin), against a margin of a few times the emulation's own."""
import os
import re

import pytest
import torch

from tests import gemm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (4, 32, 36, 64, 96, 100, 516, 1024, 2048)              # the K sweep of tests/test_gpu_gemm.py
M_CPU, N_CPU = 150, 192
_cache = {}


def _case(epi, prec, K, M=M_CPU, N=N_CPU):
    """One case with its operands, reference and emulation, shared by the tests of this module (never modified)."""
    key = (epi, prec, K, M, N)
    if key not in _cache:
        case = R.make_case(M, N, K, prec, epi, seed=3)
        ops = R.operands(case)
        _cache[key] = (case, ops, R.reference(case, ops), R.emulate(case, ops))
    return _cache[key]


@pytest.mark.parametrize("prec", R.PRECS)
def test_emulation_is_inside_the_cap(prec):
    """Every class at K = 100, and the three sweep classes at every K of the sweep."""
    worst = 0.0
    todo = [(epi, 100) for epi in R.EPI_CLASSES] + [(epi, K) for epi in ("128", "287", "1504") for K in KS if K != 100]
    for epi, K in todo:
        case, ops, (ref, cap), emu = _case(epi, prec, K)
        ratio = float(((emu.v - ref).abs() / cap.clamp(min=1e-300)).max())
        worst = max(worst, ratio)
        assert bool(((emu.v - ref).abs() <= cap).all()), (epi, K, ratio)
        if emu.h is not None:       # the H output decodes to within the conversion's half ulp of it
            dec = sum(p.double() for p in emu.h)
            assert bool(((dec - ref).abs() <= R.h_cap(case, ref, cap)).all()), (epi, K)
    print(f"{R.PREC_NAME[prec]}: worst |emulate - reference| / cap over {len(todo)} cases = {worst:.3f}")


def test_fp32_engine_emulation_is_inside_the_cap():
    for epi in ("all_on", "224", "none"):
        case = R.make_case(77, 100, 516, "fp32", epi, seed=3)
        ref, cap = R.reference(case)
        emu = R.emulate(case)
        ratio = float(((emu.v - ref).abs() / cap.clamp(min=1e-300)).max())
        print(f"fp32 {epi}: worst |emulate - reference| / cap = {ratio:.3f}")
        assert ratio <= 1.0


def _frac_over(v, ref, cap):
    return float(((v - ref).abs() > cap).double().mean())


@pytest.mark.parametrize("prec", R.PRECS)
def test_gross_mutants_exceed_the_cap(prec):
    """A ReLU skipped, the neighbouring column's parameters, the next row's residual and 32 missing k in one 16 x 32 block put more
    than half of the affected elements (rows, for the row-dot class) outside the CAP."""
    name = R.PREC_NAME[prec]
    for i in range(4):      # skip_relu on the all-on chain: elements whose value at that ReLU is negative are the affected ones
        case, ops, (ref, cap), emu = _case("all_on", prec, 100)
        mut = R.emulate(case, ops, skip_relu=i).v
        changed = mut != emu.v
        assert float(changed.double().mean()) > 0.05
        frac = float((((mut - ref).abs() > cap) & changed).double().sum() / changed.double().sum())
        print(f"{name} skip_relu={i}: {100 * frac:.0f} % of {int(changed.sum())} affected elements over the cap")
        assert frac > 0.5
    for epi in ("131", "287", "1504", "513"):
        case, ops, (ref, cap), _ = _case(epi, prec, 100)
        frac = _frac_over(R.emulate(case, ops, neighbour_column_params=True).v, ref, cap)
        print(f"{name} {epi} neighbour_column_params: {100 * frac:.0f} % over the cap")
        assert frac > 0.5
    for epi in ("224", "480", "1504", "2400"):
        case, ops, (ref, cap), _ = _case(epi, prec, 100)
        frac = _frac_over(R.emulate(case, ops, next_row_residual=True).v, ref, cap)
        print(f"{name} {epi} next_row_residual: {100 * frac:.0f} % over the cap")
        assert frac > 0.5
    for K in (100, 1024):
        for epi, blk in (("128", (2, 3)), ("287", (0, 0))):
            case, ops, (ref, cap), emu = _case(epi, prec, K)
            mut = R.emulate(case, ops, zero_k=(case["Kpad"] - 64, case["Kpad"]) if K > 64 else (0, 32), zero_block=blk).v
            rs, cs = slice(16 * blk[0], 16 * blk[0] + 16), slice(32 * blk[1], 32 * blk[1] + 32)
            outside = mut.clone()
            outside[rs, cs] = emu.v[rs, cs]
            assert torch.equal(outside, emu.v)                               # only that block differs
            changed = (mut != emu.v)[rs, cs]                                 # (a ReLU hides the elements it zeroes either way)
            assert float(changed.double().mean()) > 0.1
            frac = float(((((mut - ref).abs() > cap)[rs, cs]) & changed).double().sum() / changed.double().sum())
            print(f"{name} {epi} K {K} zero_k in block {blk}: {100 * frac:.0f} % of {int(changed.sum())} affected elements over the cap")
            assert frac > 0.5


@pytest.mark.parametrize("K", [516, 100, 1024, 36])
def test_a_lost_lo_term_is_far_outside_the_rms_margin(K):
    """f16x3 without a_lo w_hi - everywhere, or in the last K slab only - at 256 x 256 on the raw-accumulator class: the affected
    blocks' RMS error rises by more than 50 x the unmutated emulation's (the GPU test allows a single-digit factor), while the
    worst |error| / cap stays below 1 at long K: the cap alone does not catch it."""
    case, ops, (ref, cap), emu = _case("128", 0, K, M=256, N=256)
    base, counted = R.block_rms(emu.v - ref)
    base = torch.maximum(base, R.rms_floor(ref))
    assert bool(counted.all())
    last = (case["Kpad"] - 32)
    for label, mut in (("whole term", R.emulate(case, ops, drop_a_lo=True).v), ("last slab", R.emulate(case, ops, drop_a_lo_from_k=last).v)):
        got, _ = R.block_rms(mut - ref)
        ratio = float((got / base).min())
        cap_ratio = float(((mut - ref).abs() / cap).max())
        print(f"f16x3 K {K} a_lo lost, {label}: block RMS x {ratio:.0f} (least affected block), worst |err| / cap {cap_ratio:.2f}")
        assert ratio > 50


@pytest.mark.parametrize("prec", R.PRECS)
def test_h_truncate_changes_bits(prec):
    for epi in ("287", "1504"):
        case, ops, _, emu = _case(epi, prec, 100)
        mut = R.emulate(case, ops, h_truncate=True)
        assert torch.equal(mut.v, emu.v)
        plane = -1                                                           # the plane the kernel rounds to nearest
        diff = float((mut.h[plane].view(torch.int16) != emu.h[plane].view(torch.int16)).double().mean())
        print(f"{R.PREC_NAME[prec]} {epi} h_truncate: {100 * diff:.0f} % of the H words differ")
        assert diff > 0.05


def test_block_rms_counts_cut_blocks_of_64_elements():
    err = torch.ones(20, 40)
    err[16:, 32:] = 3.0
    rms, counted = R.block_rms(err)
    assert rms.shape == (2, 2) and torch.equal(rms, torch.tensor([[1.0, 1.0], [1.0, 3.0]], dtype=torch.float64))
    assert counted.tolist() == [[True, True], [True, False]]                 # 4 x 32 = 128 and 16 x 8 = 128 count, 4 x 8 = 32 does not


def test_ef_of_and_the_class_list_match_the_kernel():
    """ef_of reproduces every class number, and the numbers gemm_epilogue_dispatch16 specialises are exactly EPI_CLASSES' (a class
    added to the kernel must enter the matrix of tests/test_gpu_gemm.py)."""
    for name, e in R.EPI_CLASSES.items():
        assert R.ef_of_class(e) == e.ef, name
        if name not in ("all_on", "none"):
            assert name == str(e.ef)
    assert R.ef_of(relu0=1, sc0=1, relu1=1, sc1=1, relu2=1, out_h=1) == 287
    assert R.ef_of(residual="interp", relu_final=1, out_h=1) == 2400 and R.ef_of(relu0=1, dot=1) == 513
    src = open(os.path.join(ROOT, "pointstowood_amd", "csrc", "p2w_hgemm.h")).read()
    found = {int(m) for m in re.findall(r"P2W_EPI_CASE\((\d+)\)", src)}
    found |= {int(m) for m in re.findall(r"case (\d+):", src)} | {int(m) for m in re.findall(r"ef == (\d+)", src)}
    assert {128, 2400, 513} <= found
    assert found == set(R.SPECIALISED), sorted(found ^ set(R.SPECIALISED))
    assert len(R.SPECIALISED) == 14 and 511 not in found and 384 not in found


def test_layers_c32_agree_with_the_checkpoint_layout():
    from pointstowood_amd.synthetic_weights import synth_state_dict
    C = 32
    sd = synth_state_dict(1, C)
    shape = lambda k: tuple(sd[k].shape[:2])
    want = set()
    f_in = C
    for l in (1, 2, 3):
        p = f"sa{l}_module"
        C1, k1 = shape(p + ".conv.local_nn.0.0.weight")
        assert k1 == f_in + 4
        want.add((C1, f_in))                                                  # the hoisted layer 1: the feature columns only
        r = p + ".residual_block"
        want |= {shape(r + ".expand.0.weight"), shape(r + ".conv.0.pointwise_conv.weight"), shape(r + ".conv.3.pointwise_conv.weight"),
                 shape(r + ".project.0.weight")}
        f_in = shape(p + ".conv.local_nn.1.0.weight")[0]
    want |= {shape("sa4_module.NN.0.0.weight"), shape("sa4_module.NN.1.0.weight")}
    Fc = shape("sa4_module.NN.1.0.weight")[0]
    for l in (4, 3, 2, 1):
        n0, k0 = shape(f"fp{l}_module.NN.0.0.weight")
        want |= {(n0, k0), (n0, Fc), (n0, k0 - Fc), shape(f"fp{l}_module.NN.1.0.weight")}      # whole, and split W_i | W_s
        Fc = shape(f"fp{l}_module.NN.1.0.weight")[0]
    want.add(shape("conv1.weight"))
    assert {(n, k) for n, k, _ in R.LAYERS_C32} == want
    assert len(set(R.LAYERS_C32)) == len(R.LAYERS_C32)
    assert all(c in R.EPI_CLASSES for _, _, c in R.LAYERS_C32)
    assert {c for _, _, c in R.LAYERS_C32} == {"128", "263", "287", "257", "1376", "1504", "131", "259", "2400", "513"}
