"""Host-side helpers for tests of the H family (16-bit MFMA operands, include/p2w.h): weight packing, H tensors in and out,
and the per-precision GEMM error bound.  Shared by tests/test_gpu_ops.py and tests/test_gpu_sa_conv.py."""
import numpy as np
import torch


def _pack_h(W, prec):
    """Host-side H weights of W [N, K] for precision code `prec` (0 f16x3, 1 fp16, 2 bf16): (tensor on the GPU, 2^-e, K_pad)."""
    from pointstowood_amd import _lib
    N, K = W.shape
    Np, Kp = _lib.packed_dims(N, K, prec)
    Wp = torch.zeros(Np, Kp, dtype=torch.float64)
    Wp[:N, :K] = W.double()
    e = int(np.floor(np.log2(1024.0 / float(Wp.abs().max()))))
    Ws = Wp * 2.0 ** e
    if prec == 0:     # H layout: blocks of 32 k stored as [hi(32) | lo(32)]
        hi = Ws.float().half()
        lo = (Ws - hi.double()).float().half()
        w = torch.stack([hi.view(Np, Kp // 32, 32), lo.view(Np, Kp // 32, 32)], dim=2).reshape(Np, 2 * Kp)
    else:
        w = Ws.float().to(torch.float16 if prec == 1 else torch.bfloat16)
    return w.contiguous().cuda(), 2.0 ** -e, Kp


def _to_h(x, prec, ldh):
    """H form of an fp32 [m, F] tensor, produced ON THE DEVICE by p2w_concat_xyz_h2 with zero positions (so the
    kernels' own fp32 -> 16-bit conversion is what gets tested)."""
    from pointstowood_amd._lib import check, lib, ptr, stream
    m, F = x.shape
    assert F % 4 == 0 and ldh >= F + 4
    planes = 2 if prec == 0 else 1
    out = torch.full((m, planes * ldh), float("nan"), dtype=torch.bfloat16 if prec == 2 else torch.float16, device="cuda")
    zeros = torch.zeros((m, 4), device="cuda")
    check(lib().p2w_concat_xyz_h2(prec, ptr(x.cuda().contiguous()), F, ptr(zeros), m, ptr(out), ldh, stream()))
    return out


def _from_h(t, prec, ldh):
    """Values [m, ldh] (float64, on the CPU) of an H tensor: f16x3 rows are blocks of 32 columns stored [hi(32) | lo(32)]."""
    v = t.cpu().double()
    if prec != 0:
        return v[:, :ldh]
    b = v.view(v.shape[0], ldh // 32, 2, 32)
    return (b[:, :, 0] + b[:, :, 1]).reshape(v.shape[0], ldh)


# relative error bound of a K-term dot product per precision (operand rounding 2^-22 / 2^-11 / 2^-8, fp32 accumulate)
H_TOL = {0: 4e-5, 1: 3e-3, 2: 2.5e-2}
