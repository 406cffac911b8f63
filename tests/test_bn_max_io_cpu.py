"""What of relu_bn_max's float16 / bfloat16 route (include/p2w.h: p2w_relu_bn_max_io / _bwd_io; train.py --fused_bn_max) can be checked
without a GPU: the refusals of the two entry points that return before a launch, the command-line flag, how the flag reaches the
model, and the rounding that tests/test_gpu_bn_max_io.py compares dz against."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENULL, EALIGN, EWORKSPACE, EUNSUPPORTED = -1, -2, -3, -4, -5
F32, F16, BF16 = 0, 1, 2
A = 0x10000            # a 16-byte aligned address that is never followed: every call below is refused before a launch


def test_io_entry_points_refuse_before_a_launch():
    """Unknown dtype codes (3 and -1) give P2W_EUNSUPPORTED ahead of every other check; with a known code the namesake's refusals come
    back in its order: sizes (-1), null pointers (-2), a workspace off 16 bytes (-3), a workspace that is too small (-4)."""
    from pointstowood_amd._lib import lib
    L = lib()
    E, M, C2 = 14, 5, 8
    need = int(L.p2w_relu_bn_max_ws_bytes(E, M, C2))
    assert need > 0

    def fwd(tz, z=A, ldz=C2, csr=A, gamma=A, beta=A, rm=A, rv=A, mom=0.1, eps=1e-5, E_=E, M_=M, C2_=C2, out=A, ext=A, arg=A, mean=A, invstd=A,
            ws=A, wsb=need):
        return L.p2w_relu_bn_max_io(z, tz, ldz, csr, gamma, beta, rm, rv, mom, eps, E_, M_, C2_, out, ext, arg, mean, invstd, ws, wsb, None)

    def bwd(tz, g=A, z=A, ldz=C2, csr=A, arg=A, ext=A, mean=A, invstd=A, gamma=A, E_=E, M_=M, C2_=C2, dz=A, lddz=C2, dgamma=A, dbeta=A, ws=A,
            wsb=need):
        return L.p2w_relu_bn_max_bwd_io(g, z, tz, ldz, csr, arg, ext, mean, invstd, gamma, E_, M_, C2_, dz, lddz, dgamma, dbeta, ws, wsb, None)

    for code in (3, -1):
        assert fwd(code) == EUNSUPPORTED and bwd(code) == EUNSUPPORTED
        assert fwd(code, z=None) == EUNSUPPORTED and fwd(code, E_=1) == EUNSUPPORTED and fwd(code, ws=A + 4) == EUNSUPPORTED
        assert fwd(code, wsb=0) == EUNSUPPORTED and bwd(code, dz=None) == EUNSUPPORTED and bwd(code, lddz=1) == EUNSUPPORTED
        assert bwd(code, wsb=0) == EUNSUPPORTED
    for tz in (F32, F16, BF16):
        for name in ("z", "csr", "gamma", "beta", "rm", "rv", "out", "ext", "arg", "mean", "invstd", "ws"):
            assert fwd(tz, **{name: None}) == ENULL, (tz, name)
        for name in ("g", "z", "csr", "arg", "ext", "mean", "invstd", "gamma", "dz", "dgamma", "dbeta", "ws"):
            assert bwd(tz, **{name: None}) == ENULL, (tz, name)
        assert fwd(tz, E_=1) == EINVAL and fwd(tz, M_=0) == EINVAL and fwd(tz, C2_=0) == EINVAL and fwd(tz, ldz=C2 - 1) == EINVAL
        assert fwd(tz, eps=-1.0) == EINVAL and fwd(tz, mom=1.5) == EINVAL and fwd(tz, eps=float("nan")) == EINVAL
        assert fwd(tz, E_=1, z=None) == EINVAL                                   # sizes before pointers, as in the namesake
        assert bwd(tz, E_=1) == EINVAL and bwd(tz, M_=-3) == EINVAL and bwd(tz, C2_=0) == EINVAL and bwd(tz, ldz=C2 - 4) == EINVAL
        assert bwd(tz, lddz=4) == EINVAL
        assert fwd(tz, ws=A + 4) == EALIGN and bwd(tz, ws=A + 8) == EALIGN
        assert fwd(tz, wsb=need - 1) == EWORKSPACE and fwd(tz, wsb=0) == EWORKSPACE and bwd(tz, wsb=need - 1) == EWORKSPACE


def _parser():
    sys.path.insert(0, ROOT)
    try:
        import importlib.util
        spec = importlib.util.spec_from_file_location("p2w_train_cli", os.path.join(ROOT, "train.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(ROOT)
    return mod.build_parser()


def test_command_line_flag():
    p = _parser()
    assert p.parse_args([]).fused_bn_max is False
    assert p.parse_args(["--fused_bn_max"]).fused_bn_max is True
    both = p.parse_args(["--fused_bn_max", "--amp", "bf16"])
    assert both.fused_bn_max is True and both.amp == "bf16"


def test_flag_reaches_every_pointnetconv_and_nothing_else():
    """trainer.set_fused_bn_max sets the attribute on the three PointNetConv instances of a train.Net, on no other module, and not
    on the class: another Net built afterwards has it False everywhere."""
    from pointstowood_amd import ops, train, trainer
    net = train.Net(num_classes=1, C=8)
    convs = [m for m in net.modules() if isinstance(m, ops.PointNetConv)]
    assert len(convs) == 3 and all(m.fused_bn_max is False and "fused_bn_max" not in vars(m) for m in convs)
    keys = list(net.state_dict())
    assert trainer.set_fused_bn_max(net) == 3
    assert all(vars(m).get("fused_bn_max") is True for m in convs)
    assert [m for m in net.modules() if "fused_bn_max" in vars(m)] == convs
    assert ops.PointNetConv.fused_bn_max is False and "fused_bn_max" not in vars(train.Net)
    assert list(net.state_dict()) == keys
    other = train.Net(num_classes=1, C=8)
    assert all(m.fused_bn_max is False for m in other.modules() if isinstance(m, ops.PointNetConv))
    assert trainer.set_fused_bn_max(net, False) == 3 and all(m.fused_bn_max is False for m in convs)


def test_the_rounding_dz_is_compared_against():
    """tests/test_gpu_bn_max_io.py holds a 16-bit dz to the fp32 dz rounded by torch.Tensor.half() / .bfloat16() on the CPU: that is
    the rounding tests/half_io_ref.py and tests/bf16_io_ref.py define - their whole tables through it."""
    from tests import bf16_io_ref as BR
    from tests import half_io_ref as HR
    h = torch.from_numpy(HR.TABLE32.copy()).half().view(torch.int16).numpy().view(np.uint16)
    assert HR.same_half_bits(h, HR.TABLE16)
    b = torch.from_numpy(BR.TABLE32.copy()).bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert BR.same_bits(b, BR.TABLE16)
