"""The fused optimiser step without a GPU: tests/optim_ref.py against torch's AdamW, clip_grad_norm_ and GradScaler's law in float64,
the fp32 replay against the float64 restatement within the derived caps, every guard of p2w_clip_adamw through ctypes, the constants and
the command-line flag."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from pointstowood_amd import _lib
from tests import optim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_and_records_mirror_the_header():
    hdr = open(os.path.join(ROOT, "include", "p2w.h")).read()
    for name, ours, theirs in (("CHUNK", _lib.OPTIM_CHUNK, R.CHUNK), ("GROUP", _lib.OPTIM_GROUP, R.GROUP),
                               ("MAX_TENSORS", _lib.OPTIM_MAX_TENSORS, R.MAX_TENSORS)):
        assert int(re.search(rf"#define P2W_OPTIM_{name} (\d+)", hdr).group(1)) == ours == theirs
    assert R.CHUNK == 256 * 16
    assert C.sizeof(_lib.OptimTensor) == 40 and C.sizeof(_lib.OptimHyper) == 72 and C.sizeof(_lib.OptimState) == 80
    for struct, cname in ((_lib.OptimTensor, "p2w_optim_tensor"), (_lib.OptimHyper, "p2w_optim_hyper"), (_lib.OptimState, "p2w_optim_state")):
        body = re.sub(r"/\*.*?\*/", " ", re.search(rf"typedef struct {cname} \{{(.*?)\}} {cname};", hdr, flags=re.S).group(1), flags=re.S)
        names = [n.strip().lstrip("*") for decl in body.split(";") if decl.strip()
                 for n in re.sub(r"^\s*(const )?[a-z0-9_]+\s*\*?", "", " ".join(decl.split()), count=1).split(",")]
        assert names == [n for n, _ in struct._fields_], (cname, names)
    assert _lib.OptimState.scale.offset == 20 and _lib.OptimState.t.offset == 32 and _lib.OptimState.decay.offset == 48


def test_restatement_equals_torch_adamw_behind_the_clip_in_float64():
    """5 steps of torch.optim.AdamW(foreach=False) + clip_grad_norm_(1.0) on float64 CPU tensors under OneCycleLR stepped after every
    step (lr and beta1 move), gradients below max_norm (steps 0, 2) and above (1, 3, 4): step64() on the same gradients agrees to
    1e-12 relative - operation orders differ, the function does not."""
    gen = torch.Generator().manual_seed(5)
    shapes = [(7, 5), (5,), (), (33,)]
    params = [torch.nn.Parameter(torch.randn(s, generator=gen, dtype=torch.float64)) for s in shapes]
    opt = torch.optim.AdamW(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, foreach=False)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-2, total_steps=6, pct_start=0.4)
    ps = [p.detach().numpy().copy() for p in params]
    ms, vs = [np.zeros_like(p) for p in ps], [np.zeros_like(p) for p in ps]
    state = R.new_state(1.0)
    seen = set()
    for step, size in enumerate([0.01, 3.0, 0.05, 10.0, 1.5]):
        gs = [torch.randn(s, generator=gen, dtype=torch.float64) * size for s in shapes]
        for p, g in zip(params, gs):
            p.grad = g.clone()
        group = opt.param_groups[0]
        hyper = dict(R.HYPER, lr=group["lr"], beta1=group["betas"][0], beta2=group["betas"][1], scaling=0)
        seen.add((hyper["lr"], hyper["beta1"]))
        norm = torch.nn.utils.clip_grad_norm_(params, max_norm=1.0)
        opt.step()
        sched.step()
        ps, ms, vs, rec = R.step64(ps, [g.numpy() for g in gs], ms, vs, state, hyper)
        state = {k: rec[k] for k in state}
        assert rec["norm"] == pytest.approx(float(norm), rel=1e-14) and (rec["coef"] == 1.0) == (float(norm) + 1e-6 <= 1.0)
        assert (rec["coef"] < 1.0) == (size > 1.0) and rec["t"] == step + 1
        for p, mine, m, v in zip(params, ps, ms, vs):
            np.testing.assert_allclose(mine, p.detach().numpy(), rtol=1e-12, atol=0)
            np.testing.assert_allclose(m, opt.state[p]["exp_avg"].numpy(), rtol=1e-12, atol=0)
            np.testing.assert_allclose(v, opt.state[p]["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
    assert len(seen) == 5 and len({b for _, b in seen}) > 1       # both really moved


def test_unscale_is_part_of_the_restatement():
    """A scaled gradient under scale 512 gives what the unscaled one gives under scale 1 (powers of two: exactly)."""
    rng = np.random.default_rng(1)
    p, g = rng.standard_normal(50), rng.standard_normal(50)
    z = np.zeros(50)
    a = R.step64([p], [g * 512.0], [z], [z], R.new_state(512.0), R.HYPER)
    b = R.step64([p], [g], [z], [z], R.new_state(1.0), dict(R.HYPER, scaling=0))
    for x, y in zip(a[:3], b[:3]):
        assert (x[0] == y[0]).all()
    assert a[3]["inv_scale"] == 1 / 512 and a[3]["scale"] == 512.0 and b[3]["scale"] == 1.0


def test_scale_law_table():
    """GradScaler.update with its constants (growth 2, backoff 0.5, interval 2000 or 2)."""
    H2 = dict(R.HYPER, growth_interval=2)
    s = R.new_state(512.0)
    s = R.scale_law(s, False, H2)
    assert s == dict(scale=512.0, growth_tracker=1, t=1, skipped=0)
    s = R.scale_law(s, False, H2)                                 # growth at the interval, tracker back to 0
    assert s == dict(scale=1024.0, growth_tracker=0, t=2, skipped=0)
    s = R.scale_law(s, False, H2)
    assert s == dict(scale=1024.0, growth_tracker=1, t=3, skipped=0)
    s = R.scale_law(s, True, H2)                                  # backoff, tracker reset, t does not advance
    assert s == dict(scale=512.0, growth_tracker=0, t=3, skipped=1)
    s = R.scale_law(s, True, H2)
    assert s == dict(scale=256.0, growth_tracker=0, t=3, skipped=2)
    s = R.scale_law(s, False, H2)
    assert s == dict(scale=256.0, growth_tracker=1, t=4, skipped=2)
    s = R.new_state(512.0)
    for _ in range(1999):
        s = R.scale_law(s, False, R.HYPER)
    assert s["scale"] == 512.0 and s["growth_tracker"] == 1999
    assert R.scale_law(s, False, R.HYPER) == dict(scale=1024.0, growth_tracker=0, t=2000, skipped=0)
    off = dict(H2, scaling=0)                                     # scaling off: the scale stays 1, the counters move
    s = R.scale_law(R.scale_law(R.new_state(1.0), False, off), False, off)
    assert s == dict(scale=1.0, growth_tracker=0, t=2, skipped=0)
    assert R.scale_law(s, True, off) == dict(scale=1.0, growth_tracker=0, t=2, skipped=1)


def test_scale_law_is_gradscalers():
    """The same sequence through torch.amp.GradScaler itself (on the CPU device)."""
    scaler = torch.amp.GradScaler("cpu", init_scale=512.0, growth_interval=2)
    w = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([w], lr=0.0)
    mine = R.new_state(512.0)
    for bad in (False, False, False, True, True, False, False):
        w.grad = torch.tensor([float("inf") if bad else 1.0])
        scaler.scale(torch.zeros(()))                             # (creates the scale tensor)
        scaler.step(opt)
        scaler.update()
        mine = R.scale_law(mine, bad, dict(R.HYPER, growth_interval=2))
        assert scaler.get_scale() == mine["scale"] and scaler._get_growth_tracker() == mine["growth_tracker"], (bad, mine)


def test_replay32_stays_within_the_caps_of_the_restatement():
    """The fp32 replay fed correctly rounded scalars against step64: every element within its cap (and not bit-equal: the caps are not
    vacuous), over two steps with a clip in the second."""
    rng = np.random.default_rng(2)
    n = 5000
    p, m, v = rng.standard_normal(n).astype(np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    state = R.new_state(512.0)
    for size in (0.001, 2.0):
        g = (rng.standard_normal(n) * size * 512.0).astype(np.float32)
        g[:5] = 0.0
        p64, m64, v64, rec = R.step64([p], [g], [m], [v], state, R.HYPER)
        cap_p, cap_m, cap_v = R.element_caps(p, g, m, v, rec, n)
        rec32 = dict(rec)
        rec32["norm"], rec32["coef"] = R.norm_coef32(rec["sumsq"], R.HYPER["max_norm"])
        p, m, v = R.replay32(p, g, m, v, rec32)
        ratios = [R.ratio(p, p64[0], cap_p), R.ratio(m, m64[0], cap_m), R.ratio(v, v64[0], cap_v)]
        print("replay32 / cap:", ratios)
        assert max(ratios) <= 1.0 and max(ratios) > 0.0
        assert (rec["coef"] < 1.0) == (size > 1.0)
        state = {k: rec[k] for k in state}


def _fake_table(ns, addr=4096, step=1 << 20):
    t = (_lib.OptimTensor * max(len(ns), 1))()
    for k, n in enumerate(ns):
        t[k].p, t[k].g, t[k].m, t[k].v = (addr + (4 * k + j) * step for j in range(4))
        t[k].n = n
    return t


def test_ws_size_host_arithmetic():
    """8 bytes per chunk of 4096 elements of one tensor, rounded up to the arena's 256; 0 for the sizes the call refuses."""
    L = _lib.lib()

    def size(ns):
        return L.p2w_clip_adamw_ws_size((C.c_int64 * max(len(ns), 1))(*ns), len(ns))
    up = lambda x: (x + 255) // 256 * 256
    for ns in ([1], [4096], [4097], [0, 0], [1, 0, 4095, 8193], [1 << 40], [5] * 4096, []):
        chunks = sum((n + 4095) // 4096 for n in ns)
        assert size(ns) == up(8 * max(chunks, 1)), ns
    for ns in ([-1], [(1 << 40) + 1], [1 << 40, 1], [1] * 4097):
        assert size(ns) == 0, ns
    assert L.p2w_clip_adamw_ws_size(None, 1) == 0 and L.p2w_clip_adamw_ws_size(None, -1) == 0


def test_argument_refusals_come_back_before_any_launch():
    """Fake addresses that are never dereferenced: every status below is returned before a launch (no GPU is needed)."""
    L = _lib.lib()
    A, U = 4096, 4100
    EINVAL, ENULL, EALIGN, EWORKSPACE = -1, -2, -3, -4

    def call(ns=(10, 5000), table="fake", T=None, state=A, ws=A, ws_size=1 << 20, hyper="default", **hy):
        t = _fake_table(ns) if isinstance(table, str) else table
        h = _lib.OptimHyper(**dict(R.HYPER, **hy)) if isinstance(hyper, str) else hyper
        return L.p2w_clip_adamw(t, len(ns) if T is None else T, C.byref(h) if h is not None else None, state, ws, ws_size, None)
    # sizes
    assert call(T=-1) == EINVAL and call(ns=[1] * 4097) == EINVAL and call(ns=(10, -1)) == EINVAL
    assert call(ns=((1 << 40) + 1,)) == EINVAL and call(ns=(1 << 40, 1)) == EINVAL
    # hyper-parameters outside torch's ranges
    for bad in (dict(lr=-1e-3), dict(lr=float("nan")), dict(lr=float("inf")), dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0),
                dict(beta2=float("nan")), dict(eps=-1e-8), dict(weight_decay=-1.0), dict(max_norm=-1.0), dict(max_norm=float("inf")),
                dict(growth_factor=1.0), dict(growth_factor=float("inf")), dict(backoff_factor=1.0), dict(backoff_factor=0.0),
                dict(growth_interval=0), dict(scaling=2)):
        assert call(**bad) == EINVAL, bad
        assert call(**dict(dict(scaling=0), **bad)) == EINVAL, bad        # with scaling off too
    # nothing to do: OK, nothing launched, nothing written - state and ws are not even looked at
    assert call(ns=()) == 0 and call(ns=(), table=None, state=None, ws=None, ws_size=0) == 0
    assert call(ns=(0, 0, 0)) == 0 and call(ns=(0,), state=None, ws=None, ws_size=0) == 0
    # null pointers
    assert call(table=None) == ENULL and call(hyper=None) == ENULL and call(state=None) == ENULL and call(ws=None) == ENULL
    for field in ("p", "g", "m", "v"):
        t = _fake_table((10, 5000))
        setattr(t[1], field, None)
        assert call(table=t) == ENULL, field
    # alignment: state and ws 16 bytes, tensors 4
    assert call(state=U) == EALIGN and call(ws=U) == EALIGN and call(state=A + 8) == EALIGN
    for field in ("p", "g", "m", "v"):
        t = _fake_table((10, 5000))
        setattr(t[0], field, A + 2)
        assert call(table=t) == EALIGN, field
    # (4-byte aligned tensors pass the alignment guard and reach the size guard)
    need = L.p2w_clip_adamw_ws_size((C.c_int64 * 2)(10, 5000), 2)
    assert need == 256
    t = _fake_table((10, 5000), addr=U)
    assert call(table=t, ws_size=need - 1) == EWORKSPACE and call(ws_size=0) == EWORKSPACE
    big = L.p2w_clip_adamw_ws_size((C.c_int64 * 1)(1 << 30), 1)
    assert big == 8 << 18 and call(ns=(1 << 30,), ws_size=big - 1) == EWORKSPACE


def test_empty_entries_pointers_are_not_looked_at():
    L = _lib.lib()
    t = _fake_table((10, 0))
    t[1].p = t[1].g = t[1].m = t[1].v = None
    h = _lib.OptimHyper(**R.HYPER)
    assert L.p2w_clip_adamw(t, 2, C.byref(h), 4096, 4096, 0, None) == -4      # past the pointer guards, refused for the size alone
    t[1].p = 4098
    assert L.p2w_clip_adamw(t, 2, C.byref(h), 4096, 4096, 0, None) == -4


def test_command_line_flag():
    import train as cli
    assert cli.build_parser().parse_args([]).fused_step is False
    assert cli.build_parser().parse_args(["--fused_step"]).fused_step is True
    assert "--fused_step" in cli.build_parser().format_help()


def test_construction_refuses_what_the_kernels_do_not_take():
    """Host tensors, other dtypes, several groups: refused at construction, before the library is needed."""
    from pointstowood_amd.optim import ClipAdamW
    w = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ClipAdamW([w])
    with pytest.raises(ValueError, match="one parameter group"):
        ClipAdamW([{"params": [w]}, {"params": [torch.nn.Parameter(torch.zeros(2))]}])
    for bad in (dict(lr=-1.0), dict(betas=(1.0, 0.9)), dict(eps=-1.0), dict(weight_decay=-1.0), dict(max_norm=-1.0), dict(loss_scale=0.0),
                dict(growth_factor=1.0), dict(backoff_factor=1.0), dict(growth_interval=0)):
        with pytest.raises(ValueError):
            ClipAdamW([w], **bad)
