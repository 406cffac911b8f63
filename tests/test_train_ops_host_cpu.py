"""The host helpers that every training operator of ``pointstowood_amd.ops`` goes through, without a device: the BatchNorm prelude
(``_check_bn``, ``_training_tick``), the running-statistics hand-over (``_running``, ``_write_back``), the derived ``half_io`` classes
and ``_lib.ws_bytes`` (the size queries are host arithmetic, as in tests/test_ws_bytes_cpu.py)."""
import pytest
import torch

from pointstowood_amd import _lib, ops

SUPPORTS = " supports BatchNorm1d(affine=True, track_running_stats=True, momentum=<float>) as the reference builds it"


def test_check_bn_refuses_in_order_with_each_operators_text():
    ops._check_bn(torch.nn.BatchNorm1d(4), "relu_bn")
    with pytest.raises(TypeError) as e:
        ops._check_bn(torch.nn.BatchNorm2d(4), "relu_bn")
    assert str(e.value) == "relu_bn: bn must be a torch.nn.BatchNorm1d"
    with pytest.raises(TypeError) as e:
        ops._check_bn(torch.nn.Identity(), "bn_chain", "bn_chain: every stage is ...")
    assert str(e.value) == "bn_chain: every stage is ..."
    for kw in (dict(affine=False), dict(track_running_stats=False), dict(momentum=None)):
        for who in ("relu_bn_max", "bn_chain", "relu_bn", "bn_relu_rowdot"):
            with pytest.raises(NotImplementedError) as e:
                ops._check_bn(torch.nn.BatchNorm1d(4, **kw), who, "unused")
            assert str(e.value) == who + SUPPORTS


def test_training_tick_refuses_one_row_before_it_counts():
    bns = [torch.nn.BatchNorm1d(3), torch.nn.BatchNorm1d(3), torch.nn.BatchNorm1d(3, track_running_stats=False)]
    bns[1].num_batches_tracked.fill_(41)
    for rows in (0, 1):
        with pytest.raises(ValueError) as e:
            ops._training_tick(torch.zeros(rows, 3), bns)
        assert str(e.value) == f"Expected more than 1 value per channel when training, got input size torch.Size([{rows}, 3])"
        assert [int(b.num_batches_tracked) for b in bns[:2]] == [0, 41]
    ops._training_tick(torch.zeros(2, 3), bns)
    assert [int(b.num_batches_tracked) for b in bns[:2]] == [1, 42] and bns[2].num_batches_tracked is None
    # the message is PyTorch's own (PyTorch counts the refused batch; the operators never have)
    with pytest.raises(ValueError) as e:
        torch.nn.BatchNorm1d(3).train()(torch.zeros(1, 3))
    assert str(e.value) == "Expected more than 1 value per channel when training, got input size torch.Size([1, 3])"


def test_running_is_the_modules_storage_unless_it_had_to_be_copied():
    own, half = torch.nn.BatchNorm1d(5), torch.nn.BatchNorm1d(5).half()
    running = ops._running([own, half])
    assert [t.data_ptr() for t in running[0]] == [own.running_mean.data_ptr(), own.running_var.data_ptr()]
    assert all(t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad for pair in running for t in pair)
    assert running[1][0].data_ptr() != half.running_mean.data_ptr()
    for pair in running:                                     # what a kernel would do: move them in place
        pair[0].add_(1.5)
        pair[1].mul_(3)
    copies = []
    real = torch.Tensor.copy_

    def counting(self, *a, **k):
        copies.append(self.data_ptr())
        return real(self, *a, **k)
    torch.Tensor.copy_ = counting
    try:
        ops._write_back([own, half], running)
    finally:
        torch.Tensor.copy_ = real
    assert copies == [half.running_mean.data_ptr(), half.running_var.data_ptr()]              # only the pair that was copied goes back
    for bn in (own, half):
        assert bn.running_mean.tolist() == [1.5] * 5 and bn.running_var.tolist() == [3.0] * 5
    assert half.running_mean.dtype == torch.float16


@pytest.mark.parametrize("name", ["_SegmentMax", "_ReluBnMax", "_BnChain", "_ReluBn", "_BnReluRowdot"])
def test_half_twin_is_a_class_of_its_own_name(name):
    base, twin = getattr(ops, name), getattr(ops, name + "Half")
    assert twin.__name__ == name + "Half" and issubclass(twin, base) and twin.__module__ == ops.__name__ and twin.__doc__
    assert twin._backward_cls.__name__ == name + "HalfBackward" and base._backward_cls.__name__ == name + "Backward"
    assert twin.forward is not base.forward and twin.backward is not base.backward
    assert twin._forward is base._forward and twin._backward is base._backward
    assert ops._EdgeLayer1Half._backward_cls.__name__ == "_EdgeLayer1HalfBackward" and not issubclass(ops._EdgeLayer1Half, ops._EdgeLayer1)


def test_ws_bytes_resolves_both_spellings_and_formats_its_refusal():
    L = _lib.lib()
    both = [n[4:-9] for n in _lib.SIGNATURES if n.endswith("_ws_bytes") and n[:-9] + "_ws_size" in _lib.SIGNATURES]
    assert both == []
    assert _lib.ws_bytes("relu_bn_max", 67, 9, 8) == L.p2w_relu_bn_max_ws_bytes(67, 9, 8) > 0
    assert _lib.ws_bytes("bn_chain", 67, 8, 3) == L.p2w_bn_chain_ws_size(67, 8, 3) > 0
    assert _lib.ws_bytes("relu_bn", 67, 8) == L.p2w_relu_bn_ws_size(67, 8) > 0
    assert _lib.ws_bytes("bn_relu_rowdot", 67, 8) == L.p2w_bn_relu_rowdot_ws_size(67, 8) > 0
    assert _lib.ws_bytes("interp_add_relu_bwd", 67, 3, 20) == L.p2w_interp_add_relu_bwd_ws_size(67, 3, 20) > 0
    assert _lib.ws_bytes("random_subset", 1000) == L.p2w_random_subset_ws_size(1000) > 0
    assert _lib.ws_bytes("cap_subset", 1000, 7) == L.p2w_cap_subset_ws_size(1000, 7) > 0
    for name, args, text in [("bn_chain", (1, 8, 3), "p2w_bn_chain_ws_size(1, 8, 3) failed"),
                             ("relu_bn", (67, 0), "p2w_relu_bn_ws_size(67, 0) failed"),
                             ("bn_relu_rowdot", (1, 8), "p2w_bn_relu_rowdot_ws_size(1, 8) failed"),
                             ("interp_add_relu_bwd", (10, 0, 10), "p2w_interp_add_relu_bwd_ws_size(10, 0, 10) failed"),
                             ("random_subset", (-1,), "p2w_random_subset_ws_size(-1) failed"),
                             ("cap_subset", (-1, 7), "p2w_cap_subset_ws_size(-1, 7) failed"),
                             ("relu_bn_max", (1, 1, 64), "p2w_relu_bn_max_ws_bytes(1, 1, 64) failed"),
                             ("poly1_focal", ((1 << 40) + 1,), "p2w_poly1_focal_ws_bytes(1099511627777) failed")]:
        with pytest.raises(RuntimeError) as e:
            _lib.ws_bytes(name, *args)
        assert str(e.value) == text
    with pytest.raises(AttributeError):
        _lib.ws_bytes("no_such_entry_point", 1)
