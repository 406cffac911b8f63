"""float64 references of p2w_bn_chain / p2w_bn_chain_bwd (csrc/p2w_bnchain.hip, ops.bn_chain), the per-element caps the GPU tests
hold the kernels to, and the case.

A chain has L stages over z [M, C]; stage s has the input u_{s-1} (u_0 = z):
    v = a u_{s-1} + b (a depthwise convolution with kernel size 1; absent: v = u_{s-1}),   xhat = (v - mean) invstd,
    y = xhat gamma + beta,   u_s = relu ? max(y, 0) : y;         out = u_L, or max(u_L + res, 0) with a residual.

Two references:

  chain64()      everything in float64 with its own statistics - the algebra (the closed forms of the backward, ddw_w's among them).
                 tests/test_bn_chain_ref_cpu.py holds it against PyTorch's float64 autograd of the literal composition; the operator
                 and module tests on the GPU compare both routes with it.
  forward_reference() / backward_reference()
                 what the kernels must give on the fp32 tensors THEY are given, stage by stage: stage s is computed on the kernel's
                 own rounded mean and invstd of the stages in front of it.  The kernel's fp32 arithmetic is IEEE operation by
                 operation (no fma, built with -ffp-contract=off), so replay32() - the same operations in torch fp32 on the CPU -
                 reproduces its intermediate values; the references take the column sums' terms and every ReLU mask from that replay
                 (a float64 recomputation could put a value next to 0 on the other side of the ReLU than the kernel has it).

Caps (EPS = 2^-23, one ulp of 1; a correctly rounded fp32 operation errs by at most EPS / 2 relative; D = 2^-53 likewise for fp64; a
sum of n given terms in any fixed order errs by at most (n - 1) / 2 ulp of sum |terms| and gets n ulp, twice the textbook bound, as in
bn_max_ref).  M rows; u = the replayed fp32 input of the stage, S1 = sum u, A2 = sum u^2 / M (u^2 is exact in fp64), mean_u = S1 / M:

  mean        = fl32(a mean_u + b): the fp64 sum, division, product and sum err by (M + 4) D (|a| sum |u| / M + |b|), the rounding by
              EPS / 2 |mean| -> cap EPS |mean| + (M + 4) D (|a| mean |u| + |b|).
  var         (never stored) = a^2 max(A2 - mean_u^2, 0) in fp64: dv = (M + 6) D a^2 (A2 + mean_u^2); the clamp cannot add to it.
  invstd      = fl32(1 / sqrt(var + eps)): cap EPS invstd + invstd dv / (2 (var + eps))            (bn_max_ref's line).
  running_mean = fl32((1 - m) r + m mean): cap EPS |value| + 4 D (|r| + |mean|) + m (M + 4) D (|a| mean |u| + |b|).
  running_var  likewise with var M / (M - 1): cap EPS |value| + 4 D (|r| + var) + 2 m dv.
  out         in float64 on the kernel's rounded mean and invstd of every stage; the kernel's own fp32 operations are bounded by a
              running error e (first order), stage by stage, e_0 = 0:
                  v = fl(fl(a u) + b):        e_v  = |a| e + EPS (|a u| + |v|) / 2
                  xhat = fl(fl(v - mean) invstd):  e_x  = (e_v + EPS / 2 |v - mean|) invstd + EPS / 2 |xhat|
                  y = fl(fl(xhat gamma) + beta):   e_y  = e_x |gamma| + EPS / 2 (|xhat gamma| + |y|)
                  ReLU is 1-Lipschitz:             e    = e_y
              and out = max(fl(u_L + res), 0): e + EPS / 2 |u_L + res|.  cap = 2 e (the second order and the doubled textbook bound).
  dres        = g where out > 0, else 0, on the kernel's own out: cap 0.
  gy          the gradient that enters stage s.  For s = L it is g (masked), given: e_g = 0.  Through a stage, with k1 = dbeta / M,
              k2 = dgamma / M (fp32, from the fp64 sums; their errors are those of dbeta and dgamma below over M, plus EPS / 2),
              sc = fl(gamma invstd), T = (|gy| + |k1| + |xhat k2|) |gamma| invstd |a|:
                  gv a = fl(fl(fl(fl(gy - k1) - fl(xhat k2)) sc) a): six roundings of EPS / 2 on at most T -> 4 EPS T with k1's and k2's
                  own roundings; what the inputs carry propagates as (e_g + e_k1 + |xhat| e_k2) |gamma| invstd |a|.
              e_g of the next stage down = the sum of the two.
  dbeta       = fl32(sum gy): cap EPS |dbeta| + M D sum |gy| + sum e_g.
  dgamma      = fl32(sum gy xhat) with the replayed fp32 xhat: cap EPS |dgamma| + (M + 1) D sum |gy xhat| + sum e_g |xhat|.
  ddw_w       = fl32(gamma invstd (sum gy u - (dbeta / M) sum u - (dgamma / M) sum xhat u)) = sum gv u, the three products and five sums in
              fp64: cap EPS |ddw_w| + |gamma| invstd ((M + 6) D (sum |gy u| + |k1| sum |u| + |k2| sum |xhat u|)
                                                      + sum e_g |u| + (sum e_g / M) sum |u| + (sum e_g |xhat| / M) sum |xhat u|).
              Its value is far below its terms: the cap is relative to the terms, as any summation of them must be.
  ddw_b       exactly 0: sum gv = gamma invstd (sum gy - M k1 - k2 sum xhat) = 0 for sum xhat = 0 - BatchNorm removes a bias in front
              of it; the kernel writes 0.0 and the test asks for that.
  dz          = the gradient below stage 1: cap e_g of it.

The tests print the worst ratio per tensor; a cap is derived here and never tuned to a kernel's output."""
import torch

from tests.conv_train_ref import ratio  # noqa: F401  (the tests take it from here)

EPS = 2.0 ** -23
D = 2.0 ** -53
ROWS = 32                           # P2W_BN_CHAIN_ROWS
MOMENTUM, BN_EPS = 0.1, 1e-5

# ------------------------------------------------------------------------------------------------ the case
M_ROWS = 4133                       # odd; 130 work items of 32 rows, the last one partial (5): the reduction's second batch of 128 items is entered
WIDTHS = [6, 16, 132]               # 4-byte lanes; one quad per lane (4 quads); 33 quads per row
ALL_NEG, CONST, GAMMA_NEG, GAMMA_ZERO, DW_ZERO, DW_NEG = 0, 1, 2, 3, 4, 5          # planted columns
# (relu, depthwise) per stage, residual
PATTERNS = {
    "expand": ([(True, False), (True, True)], False),                          # the block's four chains
    "middle": ([(True, False), (True, False), (True, True)], False),
    "tail": ([(True, False), (False, False)], False),
    "project": ([(False, False)], True),
    "one": ([(True, True)], False),                                            # and what they leave out: L = 1 without, L = 2 and 3 with a residual
    "two_res": ([(True, True), (False, False)], True),
    "three_res": ([(False, True), (True, False), (True, True)], True),
}
_cases = {}


def case(name, C, M=M_ROWS):
    """z [M, C], g [M, C], the residual and the stages of PATTERNS[name] as dicts of fp32 tensors (a, b or None, gamma, beta,
    running_mean, running_var, relu).  Planted: column ALL_NEG has beta = -10 in stage 1 (all-negative before the ReLU where stage 1
    has one: the next stage sees a constant zero and a variance of 0), column CONST of z is constant, gamma < 0 in column 2, 9, ...
    of every stage, gamma = 0 in column GAMMA_ZERO of every stage, a depthwise weight of 0 in column DW_ZERO and a negative one in
    column DW_NEG."""
    key = (name, C, M)
    if key not in _cases:
        pattern, has_res = PATTERNS[name]
        g = torch.Generator().manual_seed(sum(map(ord, name)) * 1000 + 10 * C + M % 7)
        z = torch.randn(M, C, generator=g)
        z[:, CONST] = 0.1
        stages = []
        for s, (relu, dw) in enumerate(pattern):
            gamma = torch.rand(C, generator=g) * 1.5 + 0.25
            gamma[torch.arange(C) % 7 == GAMMA_NEG] *= -1.0
            gamma[GAMMA_ZERO] = 0.0
            beta = torch.randn(C, generator=g)
            if s == 0:
                beta[ALL_NEG] = -10.0
                gamma[ALL_NEG] = gamma[ALL_NEG].abs()
            a = b = None
            if dw:
                a, b = torch.randn(C, generator=g), 0.5 * torch.randn(C, generator=g)
                a[DW_ZERO] = 0.0
                a[DW_NEG] = -a[DW_NEG].abs() - 0.1
            stages.append(dict(a=a, b=b, gamma=gamma, beta=beta, running_mean=0.1 * torch.randn(C, generator=g),
                               running_var=torch.rand(C, generator=g) + 0.5, relu=relu))
        _cases[key] = dict(z=z, g=torch.randn(M, C, generator=g), res=torch.randn(M, C, generator=g) if has_res else None, stages=stages)
    return _cases[key]


# ------------------------------------------------------------------------------------------------ float64 throughout: the algebra
def chain64(z, stages, res=None, g=None, momentum=MOMENTUM, eps=BN_EPS):
    """Forward and, with g, backward of the chain in float64 with its own statistics.  Returns a dict: out, mean / var / invstd /
    running_mean / running_var (lists per stage) and dz, dres, dgamma, dbeta, ddw_w, ddw_b (lists; None entries without a depthwise).
    ddw_w is taken from the closed form gamma invstd (sum gy u - (dbeta / M) sum u - (dgamma / M) invstd a M var_u), ddw_b is 0."""
    M = z.shape[0]
    u = z.double()
    keep = []
    r = dict(mean=[], var=[], invstd=[], running_mean=[], running_var=[])
    for st in stages:
        a, b = (st["a"].double(), st["b"].double()) if st["a"] is not None else (None, None)
        mu_u = u.sum(0) / M
        var_u = ((u * u).sum(0) / M - mu_u * mu_u).clamp_min(0.0)
        mean, var = (a * mu_u + b, a * a * var_u) if a is not None else (mu_u, var_u)
        invstd = 1.0 / torch.sqrt(var + eps)
        v = a * u + b if a is not None else u
        xhat = (v - mean) * invstd
        y = xhat * st["gamma"].double() + st["beta"].double()
        keep.append((u, xhat, y, a, invstd, var_u))
        u = torch.relu(y) if st["relu"] else y
        r["mean"].append(mean), r["var"].append(var), r["invstd"].append(invstd)
        r["running_mean"].append((1 - momentum) * st["running_mean"].double() + momentum * mean)
        r["running_var"].append((1 - momentum) * st["running_var"].double() + momentum * var * M / (M - 1))
    r["out"] = u if res is None else torch.relu(u + res.double())
    if g is None:
        return r
    gg = g.double()
    r["dres"] = None
    if res is not None:
        gg = torch.where(r["out"] > 0, gg, torch.zeros_like(gg))
        r["dres"] = gg
    for k in ("dgamma", "dbeta", "ddw_w", "ddw_b"):
        r[k] = [None] * len(stages)
    for s in range(len(stages) - 1, -1, -1):
        st = stages[s]
        u_in, xhat, y, a, invstd, var_u = keep[s]
        gy = torch.where(y > 0, gg, torch.zeros_like(gg)) if st["relu"] else gg
        dbeta, dgamma = gy.sum(0), (gy * xhat).sum(0)
        gam = st["gamma"].double()
        gg = gam * invstd * (gy - dbeta / M - xhat * dgamma / M)
        if a is not None:
            r["ddw_w"][s] = gam * invstd * ((gy * u_in).sum(0) - (dbeta / M) * u_in.sum(0) - (dgamma / M) * invstd * a * M * var_u)
            r["ddw_b"][s] = torch.zeros_like(dbeta)
            gg = a * gg
        r["dgamma"][s], r["dbeta"][s] = dgamma, dbeta
    r["dz"] = gg
    return r


def composition(z, stages, res=None):
    """The literal composition in z's dtype under ordinary autograd (F.batch_norm(training=True), relu, w * x + b); `stages` holds
    tensors of that dtype (a, b, gamma, beta may require grad; running_mean and running_var are updated in place)."""
    import torch.nn.functional as F
    x = z
    for st in stages:
        if st["a"] is not None:
            x = st["a"] * x + st["b"]
        x = F.batch_norm(x, st["running_mean"], st["running_var"], st["gamma"], st["beta"], True, MOMENTUM, BN_EPS)
        if st["relu"]:
            x = torch.relu(x)
    return x if res is None else torch.relu(x + res)


# ------------------------------------------------------------------------------------------------ what the kernels must give
def replay32(z, stages, mean, invstd):
    """The kernel's forward arithmetic in torch fp32 on the CPU, one rounded operation at a time, on fp32 mean / invstd [L, C]: per
    stage the input u, xhat and the output (after the ReLU)."""
    u, rows = z.float(), []
    for s, st in enumerate(stages):
        v = st["a"] * u + st["b"] if st["a"] is not None else u
        xhat = (v - mean[s]) * invstd[s]
        y = xhat * st["gamma"] + st["beta"]
        out = torch.where(y < 0, torch.zeros_like(y), y) if st["relu"] else y
        rows.append(dict(u=u, xhat=xhat, out=out))
        u = out
    return rows


def forward_reference(z, stages, res, mean32, invstd32, momentum=MOMENTUM, eps=BN_EPS):
    """float64 results of p2w_bn_chain on fp32 inputs, stage s on the kernel's own mean32 / invstd32 [L, C] of the stages in front of
    it: (ref, caps), dicts of mean, invstd, running_mean, running_var [L, C] and out [M, C] (module docstring)."""
    M, L = z.shape[0], len(stages)
    rows = replay32(z, stages, mean32, invstd32)
    ref = {k: [] for k in ("mean", "invstd", "running_mean", "running_var")}
    caps = {k: [] for k in ref}
    for s, st in enumerate(stages):
        u = rows[s]["u"].double()
        a, b = (st["a"].double(), st["b"].double()) if st["a"] is not None else (torch.ones(u.shape[1], dtype=torch.float64),
                                                                                torch.zeros(u.shape[1], dtype=torch.float64))
        mu_u, A2 = u.sum(0) / M, (u * u).sum(0) / M
        var_u = (A2 - mu_u * mu_u).clamp_min(0.0)
        mean, var = a * mu_u + b, a * a * var_u
        invstd = 1.0 / torch.sqrt(var + eps)
        rm = (1 - momentum) * st["running_mean"].double() + momentum * mean
        rv = (1 - momentum) * st["running_var"].double() + momentum * var * M / (M - 1)
        dm = (M + 4) * D * (a.abs() * u.abs().sum(0) / M + b.abs())
        dv = (M + 6) * D * a * a * (A2 + mu_u * mu_u)
        for k, v in (("mean", mean), ("invstd", invstd), ("running_mean", rm), ("running_var", rv)):
            ref[k].append(v)
        caps["mean"].append(EPS * mean.abs() + dm)
        caps["invstd"].append(EPS * invstd + invstd * dv / (2 * (var + eps)))
        caps["running_mean"].append(EPS * rm.abs() + 4 * D * (st["running_mean"].double().abs() + mean.abs()) + momentum * dm)
        caps["running_var"].append(EPS * rv.abs() + 4 * D * (st["running_var"].double().abs() + var) + 2 * momentum * dv)
    ref = {k: torch.stack(v) for k, v in ref.items()}
    caps = {k: torch.stack(v) for k, v in caps.items()}
    # out in float64 on the rounded statistics, with the running bound of the kernel's own fp32 operations
    u, e = z.double(), torch.zeros(z.shape, dtype=torch.float64)
    for s, st in enumerate(stages):
        mu, inv, gam, bet = mean32[s].double(), invstd32[s].double(), st["gamma"].double(), st["beta"].double()
        if st["a"] is not None:
            a, b = st["a"].double(), st["b"].double()
            v = a * u + b
            e = a.abs() * e + EPS / 2 * ((a * u).abs() + v.abs())
        else:
            v = u
        xhat = (v - mu) * inv
        e = (e + EPS / 2 * (v - mu).abs()) * inv + EPS / 2 * xhat.abs()
        y = xhat * gam + bet
        e = e * gam.abs() + EPS / 2 * ((xhat * gam).abs() + y.abs())
        u = torch.relu(y) if st["relu"] else y
    if res is not None:
        t = u + res.double()
        e = e + EPS / 2 * t.abs()
        u = torch.relu(t)
    ref["out"], caps["out"] = u, 2 * e
    return ref, caps


def backward_reference(g, z, stages, out32, mean32, invstd32):
    """float64 results of p2w_bn_chain_bwd on the fp32 tensors it is given (out32: the forward's output where the chain has a residual,
    else None): (ref, caps), dicts of dz [M, C], dres (or None), dgamma, dbeta, ddw_w, ddw_b [L, C] (0 for a stage without a
    depthwise; module docstring)."""
    M, L, C = z.shape[0], len(stages), z.shape[1]
    rows = replay32(z, stages, mean32, invstd32)
    gg = g.double()
    ref, caps = dict(dres=None), dict(dres=None)
    if out32 is not None:
        gg = torch.where(out32 > 0, gg, torch.zeros_like(gg))
        ref["dres"], caps["dres"] = gg, torch.zeros_like(gg)
    e = torch.zeros_like(gg)
    names = ("dgamma", "dbeta", "ddw_w", "ddw_b")
    for k in names:
        ref[k], caps[k] = torch.zeros(L, C, dtype=torch.float64), torch.zeros(L, C, dtype=torch.float64)
    for s in range(L - 1, -1, -1):
        st, row = stages[s], rows[s]
        u, xhat = row["u"].double(), row["xhat"].double()
        live = row["out"] > 0 if st["relu"] else torch.ones_like(row["out"], dtype=torch.bool)
        gy, e = torch.where(live, gg, torch.zeros_like(gg)), torch.where(live, e, torch.zeros_like(e))
        dbeta, dgamma = gy.sum(0), (gy * xhat).sum(0)
        cap_db = EPS * dbeta.abs() + M * D * gy.abs().sum(0) + e.sum(0)
        cap_dg = EPS * dgamma.abs() + (M + 1) * D * (gy * xhat).abs().sum(0) + (e * xhat.abs()).sum(0)
        gam, inv = st["gamma"].double(), invstd32[s].double()
        k1, k2 = dbeta / M, dgamma / M
        e_k1, e_k2 = cap_db / M + EPS / 2 * k1.abs(), cap_dg / M + EPS / 2 * k2.abs()
        ref["dgamma"][s], ref["dbeta"][s], caps["dgamma"][s], caps["dbeta"][s] = dgamma, dbeta, cap_dg, cap_db
        a = st["a"].double() if st["a"] is not None else torch.ones(C, dtype=torch.float64)
        if st["a"] is not None:
            ref["ddw_w"][s] = gam * inv * ((gy * u).sum(0) - k1 * u.sum(0) - k2 * (xhat * u).sum(0))
            su, sxu = u.abs().sum(0), (xhat * u).abs().sum(0)
            caps["ddw_w"][s] = EPS * ref["ddw_w"][s].abs() + gam.abs() * inv * (
                (M + 6) * D * ((gy * u).abs().sum(0) + k1.abs() * su + k2.abs() * sxu)
                + (e * u.abs()).sum(0) + e.sum(0) / M * su + (e * xhat.abs()).sum(0) / M * sxu)
        scale = gam.abs() * inv * a.abs()
        T = (gy.abs() + k1.abs() + (xhat * k2).abs()) * scale
        gg = gam * inv * (gy - k1 - xhat * k2) * a
        e = (e + e_k1 + xhat.abs() * e_k2) * scale + 4 * EPS * T
    ref["dz"], caps["dz"] = gg, e
    return ref, caps
