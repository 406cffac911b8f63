"""p2w_clip_adamw (csrc/p2w_optim.hip) through the C ABI on the GPU, against tests/optim_ref.py: the fp64 norm within its cap, norm and coef
bit for bit from the read-back sumsq, the seven scalars within their caps, p', m', v' BIT FOR BIT against the fp32 numpy replay fed the
record's own scalars (at both access widths) and within the per-element caps of the float64 restatement; the skip on a non-finite
gradient, the scale law, determinism and the refusals.  Tensors of a few thousand elements; every reference is computed once."""
import ctypes as C

import numpy as np
import pytest
import torch

from pointstowood_amd import _lib
from tests import optim_ref as R

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 4095, 4096, 4097, 8193]                          # below, at and above one chunk; two chunks and one element
SEVENTY = [(37 * k) % 61 + 1 for k in range(70)]                  # two full groups of 32 and a remainder of 6
SEVENTY[5], SEVENTY[33], SEVENTY[64] = 4097, 5000, 4096
WITH_EMPTY = [0, 7, 0, 0, 4100, 1, 0]
_cases = {}


def case(ns, seed, gsize, scale=512.0):
    """Host tensors of a step (fp32 numpy, read-only): p ~ N(0, 1), m ~ N(0, 0.01), v = m^2-like positives, g ~ N(0, gsize) * scale with
    a few exact zeros; every float64 reference of it is computed by the tests once and kept here."""
    key = (tuple(ns), seed, gsize, scale)
    if key not in _cases:
        rng = np.random.default_rng(seed)
        f = np.float32
        c = dict(ns=list(ns), p=[], g=[], m=[], v=[])
        for n in ns:
            c["p"].append(rng.standard_normal(n).astype(f))
            g = (rng.standard_normal(n) * gsize * scale).astype(f)
            g[::97] = 0.0
            c["g"].append(g)
            c["m"].append((rng.standard_normal(n) * 0.01).astype(f))
            c["v"].append((rng.standard_normal(n) ** 2 * 1e-4).astype(f))
        for k in ("p", "g", "m", "v"):
            for a in c[k]:
                a.setflags(write=False)
        _cases[key] = c
    return _cases[key]


def record(scale=512.0, tracker=0, t=0, skipped=0):
    return _lib.OptimState(scale=scale, growth_tracker=tracker, t=t, skipped=skipped)


def as_dict(rec):
    return {name: getattr(rec, name) for name, _ in _lib.OptimState._fields_}


class Device:
    """The tensors of a case in four flat device buffers; tensor k starts 16-byte aligned (shift 0) or 4 bytes past such an address
    (shift 1: 4 but not 16 bytes aligned).  16 guard words of NaN-pattern sentinels lie between neighbours and are checked after a call."""
    GUARD = 0x7fc0a5a5

    def __init__(self, c, shift=0, g=None):
        self.ns, self.offs, cursor = c["ns"], [], 16
        for n in c["ns"]:
            self.offs.append(cursor + shift)
            cursor = (cursor + shift + n + 16 + 3) // 4 * 4
        self.total = cursor + 16
        self.buf = {}
        for k in ("p", "g", "m", "v"):
            flat = np.full(self.total, self.GUARD, np.uint32).view(np.float32)
            for o, a in zip(self.offs, (g if k == "g" and g is not None else c[k])):
                flat[o:o + a.size] = a
            self.buf[k] = torch.from_numpy(flat.copy()).cuda()
            assert self.buf[k].data_ptr() % 16 == 0
        self.table = (_lib.OptimTensor * max(len(self.ns), 1))()
        for i, (o, n) in enumerate(zip(self.offs, self.ns)):
            e = self.table[i]
            e.n = n
            if n:
                e.p, e.g, e.m, e.v = (self.buf[k].data_ptr() + 4 * o for k in ("p", "g", "m", "v"))
                assert e.p % 4 == 0 and (e.p % 16 == 0) == (shift == 0)

    def read(self, k):
        flat = self.buf[k].cpu().numpy()
        mask = np.ones(self.total, bool)
        for o, n in zip(self.offs, self.ns):
            mask[o:o + n] = False
        assert (flat.view(np.uint32)[mask] == self.GUARD).all(), f"a store outside the tensors of {k}"
        return [flat[o:o + n].copy() for o, n in zip(self.offs, self.ns)]


def ws_size(ns):
    return int(_lib.lib().p2w_clip_adamw_ws_size((C.c_int64 * max(len(ns), 1))(*ns), len(ns)))


def run(c, rec_in, hyper, shift=0, ws_fill=0xFF, g=None):
    """One call -> (status, p', m', v', g after, the record read back as a dict)."""
    d = Device(c, shift, g)
    state = torch.frombuffer(bytearray(bytes(rec_in)), dtype=torch.uint8).cuda()
    ws = torch.full((ws_size(c["ns"]),), ws_fill, dtype=torch.uint8, device="cuda")
    h = _lib.OptimHyper(**hyper)
    status = _lib.lib().p2w_clip_adamw(d.table, len(c["ns"]), C.byref(h), state.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream())
    torch.cuda.synchronize()
    rec = as_dict(_lib.OptimState.from_buffer_copy(state.cpu().numpy().tobytes()))
    return status, d.read("p"), d.read("m"), d.read("v"), d.read("g"), rec


def bits(xs):
    return np.concatenate([np.asarray(x, np.float32).view(np.uint32) for x in xs]) if len(xs) else np.zeros(0, np.uint32)


def check_finite_step(c, rec_in, hyper, out, label, g=None):
    """Everything the issue asks of a step that applies.  -> the worst error / cap of (p', m', v')."""
    status, p1, m1, v1, g1, rec = out
    gs = c["g"] if g is None else g
    assert status == 0
    assert (bits(g1) == bits(gs)).all(), "g was modified"
    n_total = sum(c["ns"])
    state = dict(scale=rec_in.scale, growth_tracker=rec_in.growth_tracker, t=rec_in.t, skipped=rec_in.skipped)
    p64, m64, v64, want = R.step64(c["p"], gs, c["m"], c["v"], state, hyper)
    # the counters and the scale
    assert rec["found_inf"] == 0 and want["found_inf"] == 0
    for k in ("scale", "growth_tracker", "t", "skipped"):
        assert rec[k] == want[k], (k, rec[k], want[k])
    assert np.float32(rec["inv_scale"]) == np.float32(want["inv_scale"])
    # sumsq within its cap; norm and coef bit for bit from it
    err, cap = abs(rec["sumsq"] - want["sumsq"]), R.sumsq_cap(want["sumsq"], n_total)
    print(f"{label}: sumsq {rec['sumsq']!r} err / cap {err / cap if cap else 0.0:.3g}")
    assert err <= cap
    norm, coef = R.norm_coef32(rec["sumsq"], hyper["max_norm"])
    assert np.float32(rec["norm"]).view(np.uint32) == norm.view(np.uint32) and np.float32(rec["coef"]).view(np.uint32) == coef.view(np.uint32)
    # the seven scalars
    S, caps = R.scalars64(hyper, want["t"]), R.scalar_caps(hyper, want["t"])
    for k in R.SCALARS:
        rel = abs(rec[k] - S[k]) / abs(S[k]) if S[k] else abs(rec[k])
        print(f"{label}: {k} {rec[k]!r} rel err / cap {rel / caps[k]:.3g}")
        assert rel <= caps[k], (k, rec[k], S[k])
    # bit for bit against the fp32 replay on the record's own scalars
    worst = [0.0, 0.0, 0.0]
    for i, n in enumerate(c["ns"]):
        rp, rm, rv = R.replay32(c["p"][i], gs[i], c["m"][i], c["v"][i], rec)
        for name, got, ref in (("p", p1[i], rp), ("m", m1[i], rm), ("v", v1[i], rv)):
            bad = np.flatnonzero(got.view(np.uint32) != ref.view(np.uint32))
            assert bad.size == 0, (label, name, i, n, bad[:5], got[bad[:5]], ref[bad[:5]])
        if n:
            cp, cm, cv = R.element_caps(c["p"][i], gs[i], c["m"][i], c["v"][i], want, n_total)
            for j, (got, ref, cap) in enumerate(((p1[i], p64[i], cp), (m1[i], m64[i], cm), (v1[i], v64[i], cv))):
                worst[j] = max(worst[j], R.ratio(got, ref, cap))
    print(f"{label}: worst error / cap  p {worst[0]:.3g}  m {worst[1]:.3g}  v {worst[2]:.3g}")
    assert max(worst) <= 1.0
    return rec


def check_skipped_step(c, rec_in, hyper, out, g):
    status, p1, m1, v1, g1, rec = out
    assert status == 0 and rec["found_inf"] == 1
    for k, got in (("p", p1), ("m", m1), ("v", v1)):
        assert (bits(got) == bits(c[k])).all(), k                  # byte-equal to before
    assert (bits(g1) == bits(g)).all()
    assert rec["t"] == rec_in.t and rec["skipped"] == rec_in.skipped + 1 and rec["growth_tracker"] == 0
    assert rec["scale"] == (rec_in.scale * hyper["backoff_factor"] if hyper["scaling"] else 1.0)
    assert not np.isfinite(rec["sumsq"])


@pytest.mark.parametrize("shift", [0, 1], ids=["16-byte", "4-byte"])
@pytest.mark.parametrize("gsize", [1e-3, 1.0], ids=["below", "above"])
def test_finite_step(gsize, shift):
    """A norm below max_norm (coef exactly 1: the unclipped update, the same bits as with max_norm out of reach) and one above it, on
    tensors of 1 .. 8193 elements at both access widths, from a record in mid-training (t = 3, tracker 7, skipped 2)."""
    c = case(SIZES, 11, gsize)
    rec_in = record(512.0, tracker=7, t=3, skipped=2)
    out = run(c, rec_in, R.HYPER, shift)
    rec = check_finite_step(c, rec_in, R.HYPER, out, f"{gsize} shift {shift}")
    assert rec["t"] == 4 and rec["growth_tracker"] == 8 and rec["skipped"] == 2 and rec["scale"] == 512.0
    if gsize < 1:
        assert rec["coef"] == 1.0 and rec["norm"] < 1.0
        free = run(c, rec_in, dict(R.HYPER, max_norm=1e6), shift)
        assert free[5]["coef"] == 1.0
        for a, b in zip(out[1:4], free[1:4]):
            assert (bits(a) == bits(b)).all()
    else:
        assert rec["coef"] < 1.0 and rec["norm"] > 1.0
    other = run(c, rec_in, R.HYPER, 1 - shift)                     # the other access width: the same bits
    for a, b in zip(out[1:4], other[1:4]):
        assert (bits(a) == bits(b)).all()
    assert other[5] == out[5]


@pytest.mark.parametrize("ns", [SEVENTY, WITH_EMPTY], ids=["70-tensors", "empty-entries"])
def test_tables(ns):
    """70 tensors = two full groups and a remainder (5 launches); a table whose entries 0, 2, 3 and 6 are empty, with null pointers."""
    c = case(ns, 12, 0.05)
    rec_in = record(512.0)
    for shift in (0, 1):
        rec = check_finite_step(c, rec_in, R.HYPER, run(c, rec_in, R.HYPER, shift), f"{len(ns)} tensors shift {shift}")
        assert rec["t"] == 1 and rec["coef"] < 1.0


def test_first_step_from_zero_moments():
    """t = 0 and zero moments, as ClipAdamW starts: the first step's bias corrections are 1 - beta."""
    c = dict(case(SIZES, 13, 0.5))
    c["m"] = [np.zeros_like(a) for a in c["m"]]
    c["v"] = [np.zeros_like(a) for a in c["v"]]
    rec_in = record(512.0)
    rec = check_finite_step(c, rec_in, R.HYPER, run(c, rec_in, R.HYPER), "first step")
    assert rec["t"] == 1


def test_gradients_of_1e25_apply():
    """Their fp32 squares overflow, the fp64 sum does not: the step applies, clipped."""
    c = dict(case(SIZES, 14, 1.0))
    rng = np.random.default_rng(3)
    c["g"] = [(np.where(rng.random(n) < 0.5, -1e25, 1e25)).astype(np.float32) for n in SIZES]
    assert not np.isfinite(np.float32(1e25 / 512) * np.float32(1e25 / 512))
    rec_in = record(512.0, t=1)
    rec = check_finite_step(c, rec_in, R.HYPER, run(c, rec_in, R.HYPER), "1e25")
    assert np.isfinite(rec["sumsq"]) and rec["sumsq"] > 3.5e38 and 0 < rec["coef"] < 1e-20 and rec["t"] == 2


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("planted", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("scaling", [1, 0], ids=["scaled", "unscaled"])
def test_a_non_finite_gradient_skips_the_step(scaling, planted, where):
    """One inf / NaN in the first element of the first tensor or the last element of the last: p, m, v byte-equal to before, t unchanged,
    skipped + 1, the scale halved (scaling off: it stays 1, the step is still skipped and counted), tracker 0."""
    c = case(SIZES, 15, 0.01)
    g = [a.copy() for a in c["g"]]
    if where == "first":
        g[0][0] = planted
    else:
        g[-1][-1] = planted
    hyper = dict(R.HYPER, scaling=scaling)
    rec_in = record(512.0 if scaling else 1.0, tracker=5, t=9, skipped=1)
    check_skipped_step(c, rec_in, hyper, run(c, rec_in, hyper, g=g), g)


def test_growth_interval_two_and_scaling_off():
    """The scale doubles after two finite steps; with scaling off it stays 1 while the counters move."""
    c = case(SIZES, 16, 0.01)
    H2 = dict(R.HYPER, growth_interval=2)
    rec_in = record(512.0)
    rec = check_finite_step(c, rec_in, H2, run(c, rec_in, H2), "growth 1")
    assert (rec["scale"], rec["growth_tracker"], rec["t"]) == (512.0, 1, 1)
    rec_in = record(512.0, tracker=1, t=1)
    rec = check_finite_step(c, rec_in, H2, run(c, rec_in, H2), "growth 2")
    assert (rec["scale"], rec["growth_tracker"], rec["t"]) == (1024.0, 0, 2)
    off = dict(H2, scaling=0)
    c1 = case(SIZES, 16, 0.01, scale=1.0)
    rec_in = record(1.0, tracker=1, t=1)
    rec = check_finite_step(c1, rec_in, off, run(c1, rec_in, off), "scaling off")
    assert (rec["scale"], rec["growth_tracker"], rec["t"], rec["inv_scale"]) == (1.0, 0, 2, 1.0)


def test_same_bits_on_every_run_whatever_the_workspace_held():
    c = case(SEVENTY, 17, 0.2)
    rec_in = record(512.0, t=2)
    a = run(c, rec_in, R.HYPER, ws_fill=0xFF)
    b = run(c, rec_in, R.HYPER, ws_fill=0xFF)
    z = run(c, rec_in, R.HYPER, ws_fill=0x00)
    assert a[0] == 0 and a[5]["found_inf"] == 0
    for other in (b, z):
        for x, y in zip(a[1:4], other[1:4]):
            assert (bits(x) == bits(y)).all()
        assert np.float64(a[5]["sumsq"]).view(np.uint64) == np.float64(other[5]["sumsq"]).view(np.uint64) and a[5] == other[5]


def test_refused_calls_write_nothing():
    """Bad hyper-parameter, missing pointer, misaligned record, workspace one byte short: the status, and a sentinel-filled record and
    workspace, p, m and v untouched."""
    L = _lib.lib()
    c = case(SIZES, 18, 0.1)
    d = Device(c)
    need = ws_size(SIZES)
    state = torch.full((96,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    good = _lib.OptimHyper(**R.HYPER)
    bad = _lib.OptimHyper(**dict(R.HYPER, beta1=1.0))
    no_g = (_lib.OptimTensor * len(SIZES))(*d.table)
    no_g[3].g = None
    odd_p = (_lib.OptimTensor * len(SIZES))(*d.table)
    odd_p[2].p = d.table[2].p + 2
    s = _lib.stream()
    sp, wp = state.data_ptr(), ws.data_ptr()
    assert L.p2w_clip_adamw(d.table, len(SIZES), C.byref(bad), sp, wp, need, s) == -1
    assert L.p2w_clip_adamw(d.table, -1, C.byref(good), sp, wp, need, s) == -1
    assert L.p2w_clip_adamw(no_g, len(SIZES), C.byref(good), sp, wp, need, s) == -2
    assert L.p2w_clip_adamw(d.table, len(SIZES), C.byref(good), None, wp, need, s) == -2
    assert L.p2w_clip_adamw(d.table, len(SIZES), C.byref(good), sp + 8, wp, need, s) == -3
    assert L.p2w_clip_adamw(odd_p, len(SIZES), C.byref(good), sp, wp, need, s) == -3
    assert L.p2w_clip_adamw(d.table, len(SIZES), C.byref(good), sp, wp, need - 1, s) == -4
    assert L.p2w_clip_adamw(d.table, 0, C.byref(good), sp, wp, need, s) == 0              # nothing to do: nothing written either
    torch.cuda.synchronize()
    assert bool((state == 0xA5).all()) and bool((ws == 0xA5).all())
    for k in ("p", "m", "v", "g"):
        assert (bits(d.read(k)) == bits(c[k])).all(), k
