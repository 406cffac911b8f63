"""float64 restatement of p2w_clip_adamw (csrc/p2w_optim.hip, optim.ClipAdamW), the fp32 replay of its update and the caps the GPU tests
hold the kernels to.

  step64()    one step in float64 on given tensors: the global norm of the unscaled gradients, clip_grad_norm_'s coefficient,
              GradScaler.update's scale law, the step count and AdamW (amsgrad=False, maximize=False).
              tests/test_optim_ref_cpu.py pins it against torch.optim.AdamW(foreach=False) + clip_grad_norm_ in float64.
  scale_law() the counters alone.
  scalars64() the seven per-step scalars in Python floats (double).
  replay32()  the update's operation order of include/p2w.h in numpy fp32, one rounding per operation, fed the scalars of a record:
              what the kernel must give bit for bit (it is built without contraction and has no fma).

Caps (EPS = 2^-23, h = EPS / 2 = the relative error of one correctly rounded fp32 operation, D = 2^-53 likewise for fp64; TINY = 2^-149
is added per operation for results in the subnormal range; first-order running errors, doubled at the end for the second order, as in
tests/bn_chain_ref.py):

  sumsq       inv_scale = fl32(1 / scale) errs by h, u = fl32(g inv_scale) by 2 h in all, its exact square by 4 h (+ second order:
              2.5 EPS is taken); the fp64 sum of n terms in any fixed order by n D: cap (2.5 EPS + (n + 2) D) sumsq.
  norm, coef  bit for bit from the record's sumsq (sqrt and the fp32 operations are correctly rounded); against float64 coef errs by
              e_coef = (2.5 EPS + (n + 2) D) / 2 [sumsq] + h [norm's rounding] + h [fl32(max_norm)] + h [the sum] + h [the division].
  scalars     each is evaluated in fp64 and rounded once: h, plus the fp64 evaluation.  The device's double pow is allowed POW_ULP = 16
              ulp (OpenCL's bound for pow; the reference's own Python pow gets the same): 1 - b^t then errs by 16 D b^t relative to
              b^t, so step_size by h + (2 * 16 D b1^t / (1 - b1^t) + 4 D) and rsb2 by h + (16 D b2^t / (1 - b2^t) + 4 D); the others
              by h + 2 D.
  p', m', v'  with e_s = 0.51 EPS for every scalar (what the line above allows with room) the operations give
                  u  = fl(g inv):            e_u  = 2 h |u|
                  gc = fl(u coef):           e_gc = (2 h + e_coef + h) |gc|
                  p1 = fl(p decay):          e_p1 = (e_s + h) |p1|
                  a  = fl(gc - m):           e_a  = e_gc + h |a|
                  b  = fl(a omb1):           e_b  = e_a omb1 + (e_s + h) |b|
                  m' = fl(m + b):            e_m  = e_b + h |m'|
                  c  = fl(v beta2):          e_c  = (e_s + h) |c|
                  q  = fl(omb2 gc):          e_q  = omb2 e_gc + (e_s + h) |q|
                  r  = fl(q gc):             e_r  = e_q |gc| + |q| e_gc + h |r|
                  v' = fl(c + r):            e_v  = e_c + e_r + h |v'|
                  s  = sqrt(v'):             e_sq = e_v / (2 s) + h s            (where v' = 0: sqrt(e_v), since sqrt(x) <= sqrt(e_v) for 0 <= x <= e_v)
                  w  = fl(s rsb2):           e_w  = e_sq rsb2 + (e_s + h) |w|
                  d  = fl(w + eps):          e_d  = e_w + e_s eps + h d
                  x  = fl(m' / d):           e_x  = e_m / d + |x| e_d / d + h |x|
                  y  = fl(step_size x):      e_y  = step_size e_x + (e_s + h) |y|
                  p' = fl(p1 - y):           e_p  = e_p1 + e_y + h |p'|
              cap = 2 e.  The tests print the worst error / cap; a cap is derived here and never tuned to a kernel's output."""
import math

import numpy as np

EPS = 2.0 ** -23
H = EPS / 2
D = 2.0 ** -53
TINY = 2.0 ** -149
POW_ULP = 16
CHUNK, GROUP, MAX_TENSORS = 4096, 32, 4096                         # P2W_OPTIM_*
SCALARS = ("decay", "omb1", "beta2", "omb2", "step_size", "rsb2", "eps")
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, max_norm=1.0, growth_factor=2.0, backoff_factor=0.5,
             growth_interval=2000, scaling=1)


def new_state(scale=512.0):
    return dict(scale=float(scale), growth_tracker=0, t=0, skipped=0)


def scale_law(state, found_inf, hyper):
    """GradScaler.update's law and the step count -> the next (scale, growth_tracker, t, skipped)."""
    scale, tracker, t, skipped = state["scale"], state["growth_tracker"], state["t"], state["skipped"]
    if found_inf:
        if hyper["scaling"]:
            scale *= hyper["backoff_factor"]
        tracker, skipped = 0, skipped + 1
    else:
        t, tracker = t + 1, tracker + 1
        if tracker == hyper["growth_interval"]:
            if hyper["scaling"]:
                scale *= hyper["growth_factor"]
            tracker = 0
    if not hyper["scaling"]:
        scale = 1.0
    return dict(scale=scale, growth_tracker=tracker, t=t, skipped=skipped)


def scalars64(hyper, t):
    b1, b2 = hyper["beta1"], hyper["beta2"]
    return dict(decay=1.0 - hyper["lr"] * hyper["weight_decay"], omb1=1.0 - b1, beta2=b2, omb2=1.0 - b2,
                step_size=hyper["lr"] / (1.0 - b1 ** t), rsb2=1.0 / math.sqrt(1.0 - b2 ** t), eps=hyper["eps"])


def scalar_caps(hyper, t):
    """Relative cap of each fp32 scalar of the record against scalars64()."""
    b1t, b2t = hyper["beta1"] ** t, hyper["beta2"] ** t
    caps = {k: H + 2 * D for k in SCALARS}
    caps["step_size"] = H + 2 * POW_ULP * D * b1t / (1.0 - b1t) + 4 * D
    caps["rsb2"] = H + POW_ULP * D * b2t / (1.0 - b2t) + 4 * D
    return caps


def sumsq_cap(sumsq, n):
    return (2.5 * EPS + (n + 2) * D) * sumsq


def step64(ps, gs, ms, vs, state, hyper):
    """One step on lists of arrays (any float dtype, taken to float64; nothing is modified) -> (ps', ms', vs', record) with record = the
    next state plus sumsq, norm, coef, inv_scale, found_inf and the seven scalars."""
    inv = 1.0 / state["scale"] if hyper["scaling"] else 1.0
    us = [np.asarray(g, np.float64) * inv for g in gs]
    with np.errstate(all="ignore"):
        sumsq = float(sum(float((u * u).sum()) for u in us))
    found_inf = not math.isfinite(sumsq)
    rec = scale_law(state, found_inf, hyper)
    norm = math.sqrt(sumsq) if sumsq >= 0 else float("nan")
    coef = min(1.0, hyper["max_norm"] / (norm + 1e-6)) if not found_inf else float("nan")
    rec.update(sumsq=sumsq, norm=norm, coef=coef, inv_scale=inv, found_inf=int(found_inf))
    ps, ms, vs = ([np.array(x, np.float64) for x in xs] for xs in (ps, ms, vs))
    if found_inf:
        return ps, ms, vs, rec
    S = scalars64(hyper, rec["t"])
    rec.update(S)
    out = ([], [], [])
    for p, u, m, v in zip(ps, us, ms, vs):
        gc = u * coef
        m1 = m + (gc - m) * S["omb1"]
        v1 = v * S["beta2"] + S["omb2"] * gc * gc
        d = np.sqrt(v1) * S["rsb2"] + S["eps"]
        for o, x in zip(out, (p * S["decay"] - S["step_size"] * (m1 / d), m1, v1)):
            o.append(x)
    return (*out, rec)


def replay32(p, g, m, v, rec):
    """The update of include/p2w.h in numpy fp32, every operation rounded once, on the scalars of ``rec`` (a record as read back).
    -> (p', m', v'); the inputs unchanged on found_inf."""
    p, g, m, v = (np.asarray(x, np.float32) for x in (p, g, m, v))
    if rec["found_inf"]:
        return p.copy(), m.copy(), v.copy()
    f = np.float32
    inv, coef, decay, omb1, beta2, omb2, step_size, rsb2, eps = (f(rec[k]) for k in ("inv_scale", "coef") + SCALARS)
    with np.errstate(all="ignore"):
        u = g * inv
        gc = u * coef
        p1 = p * decay
        m1 = m + (gc - m) * omb1
        v1 = v * beta2 + (omb2 * gc) * gc
        d = np.sqrt(v1) * rsb2 + eps
        p2 = p1 - step_size * (m1 / d)
    assert p2.dtype == m1.dtype == v1.dtype == np.float32
    return p2, m1, v1


def norm_coef32(sumsq, max_norm):
    """norm and coef as the finalising workgroup forms them from its fp64 sumsq."""
    f = np.float32
    with np.errstate(all="ignore"):
        norm = f(np.sqrt(np.float64(sumsq)))
        coef = np.minimum(f(1.0), f(max_norm) / (norm + f(1e-6)))
    return norm, f(coef)


def element_caps(p, g, m, v, rec64, n_total):
    """(cap_p, cap_m, cap_v) per element for fp32 results against step64()'s, from the float64 values (the docstring's recurrences)."""
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    es = 0.51 * EPS
    e_coef = (2.5 * EPS + (n_total + 2) * D) / 2 + 4 * H
    inv, coef = rec64["inv_scale"], rec64["coef"]
    decay, omb1, beta2, omb2, step_size, rsb2, eps = (rec64[k] for k in SCALARS)
    u = g * inv
    gc = u * coef
    e_gc = (3 * H + e_coef) * abs(gc) + TINY
    p1 = p * decay
    e_p1 = (es + H) * abs(p1) + TINY
    a = gc - m
    e_a = e_gc + H * abs(a)
    b = a * omb1
    e_b = e_a * omb1 + (es + H) * abs(b) + TINY
    m1 = m + b
    e_m = e_b + H * abs(m1)
    c = v * beta2
    e_c = (es + H) * abs(c) + TINY
    q = omb2 * gc
    e_q = omb2 * e_gc + (es + H) * abs(q) + TINY
    r = q * gc
    e_r = e_q * abs(gc) + abs(q) * e_gc + H * abs(r) + TINY
    v1 = c + r
    e_v = e_c + e_r + H * abs(v1)
    s = np.sqrt(v1)
    e_sq = np.where(s > 0, e_v / (2 * np.where(s > 0, s, 1.0)), np.sqrt(e_v)) + H * s
    w = s * rsb2
    e_w = e_sq * rsb2 + (es + H) * abs(w) + TINY
    d = w + eps
    e_d = e_w + es * eps + H * d
    x = m1 / d
    e_x = e_m / d + abs(x) * e_d / d + H * abs(x) + TINY
    y = step_size * x
    e_y = step_size * e_x + (es + H) * abs(y) + TINY
    p2 = p1 - y
    e_p = e_p1 + e_y + H * abs(p2)
    return 2 * e_p, 2 * e_m, 2 * e_v


def ratio(got, want, cap):
    """Worst |got - want| / cap (0 / 0 counts as 0)."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    cap = np.asarray(cap, np.float64)
    r = np.where(err == 0, 0.0, err / np.where(cap > 0, cap, 1.0) + np.where(cap > 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0
