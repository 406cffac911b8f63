"""float64 references of p2w_relu_bn_max / p2w_relu_bn_max_bwd (csrc/p2w_bnmax.hip, ops.relu_bn_max) on the fp32 tensors the kernels
are given, the per-element caps the GPU tests hold them to, and the case.

Caps (EPS = 2^-23, one ulp of 1; a correctly rounded fp32 operation errs by at most EPS / 2 relative; D = 2^-53 likewise for fp64; a
sum of n given terms in any fixed order errs by at most (n - 1) / 2 ulp of sum |terms| and gets n ulp, twice the textbook bound, as in
conv_train_ref).  E rows, y = relu(z), S1 = sum y, S2 = sum y^2 (y^2 is exact in fp64), A2 = S2 / E:

  ext, arg    comparisons and copies only: cap 0, bit for bit.
  mean        = fl32(S1 / E): the fp64 sum and division err by (E + 1) D |mean|, the rounding by EPS / 2 |mean| -> cap EPS |mean|
              (E D < EPS / 2 for every E < 2^29).  A column of zeros has mean 0 exactly.
  var         (never stored) = max(A2 - mean^2, 0) in fp64: dv = (E + 4) D (A2 + mean^2); the clamp cannot add to it.
  invstd      = fl32(1 / sqrt(var + eps)): d(invstd) = invstd / (2 (var + eps)) dv, plus 3 D and EPS / 2 relative of its own ->
              cap EPS invstd + invstd dv / (2 (var + eps)).
  running_mean = fl32((1 - m) r + m mean): three fp64 operations on given terms and one rounding -> cap EPS |value| + 4 D (|r| + |mean|).
  running_var  likewise with var E / (E - 1): cap EPS |value| + 4 D (|r| + var) + 2 m dv.
  out         = fl(fl(fl(fl(ext - mean) invstd) gamma) + beta) on the ROUNDED mean and invstd: what mean and invstd carry propagates as
              |gamma| (invstd cap_mean + |ext - mean| cap_invstd); the four operations of its own add at most EPS / 2 each of
              A = (|ext| + |mean|) invstd |gamma| + |beta|, 2 EPS A -> 4 EPS A.  cap = the sum of the two.  An all-zero column has
              ext = mean = 0 and cap_mean = 0: out = fl(+-0 + beta) = beta, and the test asks for that exactly.  Empty targets: cap 0.
  dbeta       = fl32(sum of the M' non-empty targets' g in fp64): cap EPS |dbeta| + M' D sum |g|.
  dgamma      = fl32(sum g xhat_ext), xhat_ext = (ext - mean) invstd in fp64 on the given fp32 mean and invstd (three fp64 operations
              per term): cap EPS |dgamma| + (M' + 3) D sum |g xhat_ext|.
  dz          where z > 0: dy = fl(fl(fl(gi - k1) - fl(xhat k2)) fl(gamma invstd)), xhat = fl(fl(y - mean) invstd), k1 = fl32(dbeta / E),
              k2 = fl32(dgamma / E) from the fp64 sums (EPS relative each, by the two lines above).  On T = (|gi| + |k1| + |xhat k2|)
              |gamma| invstd: k1 1, gi - k1 1/2, xhat 1 and k2 1 and their product 1/2, the difference 1/2, gamma invstd 1/2, the last
              product 1/2: 5.5 EPS T -> cap 8 EPS T.  Where z <= 0 the cap is 0: the kernel must write 0.

The tests print the worst ratio per tensor; a cap is derived here and never tuned to a kernel's output."""
import torch

from tests.conv_train_ref import ratio  # noqa: F401  (the tests take it from here)

EPS = 2.0 ** -23
D = 2.0 ** -53
GROUP = 16                          # P2W_BN_GROUP
MOMENTUM, BN_EPS = 0.1, 1e-5

# ------------------------------------------------------------------------------------------------ the case
M_DST, TRAILING_EMPTY = 1100, 9     # 69 groups of 16 targets, the last one partial (12); the last 9 targets have no rows
ALL_NEG, CONST, GAMMA_NEG, GAMMA_ZERO = 0, 1, 2, 3          # planted columns
TIE_TARGET = 40                     # every row <= 0 in every column (except the constant one): all ties, the first row wins
WIDTHS = [6, 16, 128, 512]          # 4-byte lanes; one quad per lane with 4 lanes per row; the model's narrowest and widest
_case, _cols = {}, {}


def targets():
    """1100 targets: degrees drawn from 0..32 with 0, 1, 32, 33, 100 and 1500 planted at targets 0..5, 5 rows at TIE_TARGET, nine
    trailing targets without rows; E is made odd."""
    if not _case:
        g = torch.Generator().manual_seed(91)
        deg = torch.randint(0, 33, (M_DST,), generator=g)
        deg[:6] = torch.tensor([0, 1, 32, 33, 100, 1500])
        deg[TIE_TARGET] = 5
        deg[M_DST - TRAILING_EMPTY:] = 0
        if int(deg.sum()) % 2 == 0:
            deg[6] += 1
        ptr = torch.cat([torch.zeros(1, dtype=torch.long), deg.cumsum(0)])
        E = int(ptr[-1])
        assert E % 2 == 1 and E % GROUP and M_DST % GROUP and int(deg[6]) <= 33
        _case.update(deg=deg, ptr=ptr.to(torch.int32), index=torch.repeat_interleave(torch.arange(M_DST), deg), E=E)
    return _case


def columns(C2):
    """z [E, C2] = randn with the planted columns and target, gamma, beta, the running statistics (fp32) and the output gradient g."""
    if C2 not in _cols:
        c = targets()
        g = torch.Generator().manual_seed(300 + C2)
        E = c["E"]
        z = torch.randn(E, C2, generator=g)
        tie = slice(int(c["ptr"][TIE_TARGET]), int(c["ptr"][TIE_TARGET + 1]))
        z[tie] = -z[tie].abs()
        z[tie.start + 1, 4:] = 0.0                                    # (a zero among the negatives: still a tie at y = 0)
        z[:, ALL_NEG] = -z[:, ALL_NEG].abs() - 0.01
        z[:, CONST] = 0.1
        gamma = torch.rand(C2, generator=g) * 1.5 + 0.25
        gamma[torch.arange(C2) % 7 == GAMMA_NEG] *= -1.0              # column 2, 9, 16, ...
        gamma[GAMMA_ZERO] = 0.0
        assert gamma[GAMMA_NEG] < 0 and gamma[ALL_NEG] > 0 and gamma[CONST] > 0
        _cols[C2] = dict(z=z, gamma=gamma, beta=torch.randn(C2, generator=g), running_mean=0.1 * torch.randn(C2, generator=g),
                         running_var=torch.rand(C2, generator=g) + 0.5, g=torch.randn(M_DST, C2, generator=g))
    return _cols[C2]


# ------------------------------------------------------------------------------------------------ the references
def segment_extremum(y, index, M, neg):
    """(ext [M, C], arg [M, C]) in y's dtype: per target the maximum of y over its rows, the minimum in the columns where `neg`; the
    lowest row that holds it; 0 and -1 for a target without rows."""
    E, C = y.shape
    key = torch.where(neg[None, :], -y, y)
    idx = index[:, None].expand(E, C)
    best = torch.full((M, C), -float("inf"), dtype=y.dtype).scatter_reduce(0, idx, key, reduce="amax", include_self=True)
    rows = torch.where(key == best[index], torch.arange(E)[:, None].expand(E, C), torch.full((E, C), E))
    arg = torch.full((M, C), E, dtype=torch.long).scatter_reduce(0, idx, rows, reduce="amin", include_self=True)
    empty = arg == E
    ext = torch.where(neg[None, :], -best, best)
    ext = torch.where(empty, torch.zeros_like(ext), ext) + 0.0          # (+ 0.0: no -0 from the sign flip)
    return ext, torch.where(empty, torch.full_like(arg, -1), arg)


def forward_reference(z, index, M, gamma, beta, running_mean, running_var, momentum=MOMENTUM, eps=BN_EPS):
    """float64 results of p2w_relu_bn_max on fp32 inputs: dict of ext, arg, mean, var, invstd, out, running_mean, running_var, and the
    caps of mean, invstd, running_mean, running_var.  (out's cap needs the kernel's rounded mean and invstd: out_cap.)"""
    z, gamma, beta = z.double(), gamma.double(), beta.double()
    E = z.shape[0]
    y = torch.relu(z)
    mean, A2 = y.sum(0) / E, (y * y).sum(0) / E
    var = (A2 - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    ext, arg = segment_extremum(y, index, M, gamma < 0)
    out = torch.where(arg >= 0, (ext - mean) * invstd * gamma + beta, torch.zeros_like(ext))
    rm = (1 - momentum) * running_mean.double() + momentum * mean
    rv = (1 - momentum) * running_var.double() + momentum * var * E / (E - 1)
    dv = (E + 4) * D * (A2 + mean * mean)
    cap_invstd = EPS * invstd + invstd * dv / (2 * (var + eps))
    caps = dict(mean=EPS * mean.abs(), invstd=cap_invstd, running_mean=EPS * rm.abs() + 4 * D * (running_mean.double().abs() + mean.abs()),
                running_var=EPS * rv.abs() + 4 * D * (running_var.double().abs() + var) + 2 * momentum * dv)
    return dict(ext=ext, arg=arg, mean=mean, var=var, invstd=invstd, out=out, running_mean=rm, running_var=rv), caps


def out_cap(ref, caps, gamma, beta):
    """The cap of out [M, C2] (module docstring)."""
    ga, ext, mean, invstd = gamma.double().abs(), ref["ext"], ref["mean"], ref["invstd"]
    prop = ga * (invstd * caps["mean"] + (ext - mean).abs() * caps["invstd"])
    own = 4 * EPS * ((ext.abs() + mean.abs()) * invstd * ga + beta.double().abs())
    return torch.where(ref["arg"] >= 0, prop + own, torch.zeros_like(ext))


def backward_reference(g, z, index, arg, ext, mean, invstd, gamma):
    """float64 results of p2w_relu_bn_max_bwd on the fp32 (int) tensors it is given: (dz, dgamma, dbeta), (cap_dz, cap_dgamma, cap_dbeta)."""
    g, z, ext, mean, invstd, gamma = (t.double() for t in (g, z, ext, mean, invstd, gamma))
    E = z.shape[0]
    live = arg >= 0
    gl = torch.where(live, g, torch.zeros_like(g))
    xe = torch.where(live, (ext - mean) * invstd, torch.zeros_like(ext))
    dbeta, dgamma = gl.sum(0), (gl * xe).sum(0)
    n_live = float(live[:, 0].sum())
    cap_db = EPS * dbeta.abs() + n_live * D * gl.abs().sum(0)
    cap_dg = EPS * dgamma.abs() + (n_live + 3) * D * (gl * xe).abs().sum(0)
    y = torch.relu(z)
    xhat = (y - mean) * invstd
    gi = torch.where(arg[index] == torch.arange(E)[:, None], g[index], torch.zeros_like(z))
    k1, k2 = dbeta / E, dgamma / E
    dy = gamma * invstd * (gi - k1 - xhat * k2)
    pos = z > 0
    dz = torch.where(pos, dy, torch.zeros_like(dy))
    T = (gi.abs() + k1.abs() + (xhat * k2).abs()) * gamma.abs() * invstd
    return (dz, dgamma, dbeta), (torch.where(pos, 8 * EPS * T, torch.zeros_like(T)), cap_dg, cap_db)


def composition(z, index, M, bn):
    """The plain route in z's dtype on the CPU under ordinary autograd: segment max (first-row ties) of bn(relu(z)); bn's mode decides."""
    from oracle import ops as O
    return O.segment_max_rows(bn(torch.relu(z)), index, M)
