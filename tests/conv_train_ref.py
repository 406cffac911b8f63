"""float64 references of the training route of ops.PointNetConv (csrc/p2w_edge.hip, ops.edge_layer1): the hoisted formulation of
the layer in plain torch, the two kernels' results with the per-element caps the GPU tests hold them to, and the cases.

Caps (EPS = 2^-23, one ulp of 1; a correctly rounded fp32 operation errs by at most EPS / 2 relative):

  geo[e, 0:3] = rel / (maxd + 1e-8).  rel = fl(pos_j - pos_i) on fp32 inputs: EPS / 2.  |rel| = sqrt of three products and two sums
      of such differences: (2 * 1/2 + 3 * 1/2) EPS on the square, half of it after the root, plus the root's own EPS / 2: 1.75 EPS; the
      max of such values errs by no more than its worst member; + 1e-8: EPS / 2; the division: EPS / 2.  Total 3.25 EPS -> cap
      4 EPS |geo|.  Where the reference is exactly 0 (a neighbour on its target, fp32 inputs) the cap is 0: the kernel must give 0.
      geo[e, 3] is a copy: cap 0.
  pre-activation z = (((P + g0 w0) + g1 w1) + g2 w2) + g3 w3: every product carries geo's 4 EPS and its own EPS / 2, each of the four
      sums adds EPS / 2 of the partial sum, which |P| + sum |g_d w_d| =: S bounds: (4 + 1/2 + 4 * 1/2) EPS S = 6.5 EPS S -> cap 8 EPS S.
      ReLU is 1-Lipschitz, so H1 = relu(z) holds the same cap.
  backward sums of exactly given fp32 terms, n of them in any fixed order: (n - 1) EPS / 2 sum |terms| -> cap n EPS sum |terms|
      (constant 1 on the issue's len * 2^-23 * sum |terms|, which is twice the textbook bound).  gP[s, c]: n = the run length of
      source s.  gWg[d, c]: terms geo[e, d] gZ[e, c], one product each: n = E + 1.  gR[s] = sum_c gP[s, c] Wg[3, c]: the products and
      the C1 sums on top of gP's own error: n = len + C1 + 1 over the terms gZ[e, c] Wg[3, c].  A source without edges has no
      terms: cap 0, the kernel must write 0."""
import torch

from oracle import ops as O

EPS = 2.0 ** -23
E8 = float(torch.tensor(1e-8, dtype=torch.float32))        # the fp32 constant of `max_distances + 1e-8`


# ------------------------------------------------------------------------------------------------ the layer, hoisted
def hoisted_conv(x, pos_src, pos_dst, ei, local_nn):
    """The training route's formulation on the CPU in the tensors' dtype under ordinary autograd: P = x W1x^T + b1 per source,
    H1 = relu(P[j] + geo Wg) per edge, the rest of local_nn, segment max over the targets (oracle.ops)."""
    j, i = ei[0], ei[1]
    M, F_in, lin1 = pos_dst.shape[0], x.shape[1], local_nn[0][0]
    P = torch.nn.functional.linear(x, lin1.weight[:, :F_in], lin1.bias)
    rel = pos_src[j, :3] - pos_dst[i, :3]
    maxd = O.scatter_max(torch.norm(rel, dim=1, keepdim=True), i, dim=0, dim_size=M)[0]
    geo = torch.cat([rel / (maxd[i] + 1e-8), pos_src[j, 3:4]], 1)
    H1 = torch.relu(P[j] + geo @ lin1.weight[:, F_in:F_in + 4].t())
    return O.segment_max_rows(local_nn[1](H1), i, M)


# ------------------------------------------------------------------------------------------------ the kernels' case
N_SRC, M_DST = 600, 400
HUB, COINCIDENT, LONG = 17, 5, 6           # the source half the plot points at, the target that sits on its neighbours, a long target
_case = {}


def edge_case():
    """400 targets, 600 sources.  Degrees drawn from 0..32 with 0, 1, 32, 33 and 100 planted at targets 0..4, target 5 with seven
    neighbours that all coincide with it (sources 580..586), target 6 with 1500 edges; source 17 referenced by about 3000 edges
    spread over the targets; sources 587..599 referenced by nobody."""
    if not _case:
        g = torch.Generator().manual_seed(77)
        deg = torch.randint(0, 33, (M_DST,), generator=g)
        deg[:5] = torch.tensor([0, 1, 32, 33, 100])
        deg[COINCIDENT], deg[LONG] = 7, 1500
        i = torch.repeat_interleave(torch.arange(M_DST), deg)
        E = i.numel()
        j = torch.randint(0, 580, (E,), generator=g)
        hub = torch.randperm(E, generator=g)[:3000]
        j[hub] = HUB
        j[i == COINCIDENT] = torch.arange(580, 587)
        pos_src, pos_dst = torch.rand(N_SRC, 4, generator=g), torch.rand(M_DST, 4, generator=g)
        pos_src[580:587, :3] = pos_dst[COINCIDENT, :3]
        ptr = torch.cat([torch.zeros(1, dtype=torch.long), deg.cumsum(0)]).to(torch.int32)
        _case.update(deg=deg, i=i, src=j.to(torch.int32), ptr=ptr, pos_src=pos_src, pos_dst=pos_dst, E=E)
    return _case


_fwd = {}


def forward_case(C1):
    """P, Wg (fp32) of width C1 on edge_case() and the float64 results: geo, H1, and their caps."""
    if C1 not in _fwd:
        c = edge_case()
        g = torch.Generator().manual_seed(100 + C1)
        P, Wg = torch.randn(N_SRC, C1, generator=g), torch.randn(4, C1, generator=g)
        j, i = c["src"].long(), c["i"]
        ps, pd = c["pos_src"].double(), c["pos_dst"].double()
        rel = ps[j, :3] - pd[i, :3]
        maxd = torch.zeros(M_DST, dtype=torch.float64).scatter_reduce(0, i, rel.norm(dim=1), reduce="amax", include_self=True)
        geo = torch.cat([rel / (maxd[i, None] + E8), ps[j, 3:4]], 1)
        cap_geo = 4 * EPS * geo.abs()
        cap_geo[:, 3] = 0
        z = P.double()[j] + geo @ Wg.double()
        S = P.double()[j].abs() + geo.abs() @ Wg.double().abs()
        _fwd[C1] = dict(P=P, Wg=Wg, geo=geo, cap_geo=cap_geo, H1=torch.relu(z), cap_H1=8 * EPS * S)
    return _fwd[C1]


def backward_reference(gH, H1, geo, src, Wg, n_src):
    """float64 sums of p2w_edge_l1_bwd on the fp32 tensors it is given, and the caps: (gP, gR, gWg), (cap_gP, cap_gR, cap_gWg)."""
    gZ = torch.where(H1 > 0, gH, torch.zeros_like(gH)).double()
    j, E, C1 = src.long(), gH.shape[0], gH.shape[1]
    run = torch.bincount(j, minlength=n_src).double()
    rows = lambda t: torch.zeros((n_src, t.shape[1]), dtype=torch.float64).index_add_(0, j, t)      # noqa: E731
    gP, aP = rows(gZ), rows(gZ.abs())
    w3 = Wg.double()[3]
    gR, aR = rows(gZ * w3).sum(1), rows((gZ * w3).abs()).sum(1)
    gWg, aW = geo.double().t() @ gZ, geo.double().abs().t() @ gZ.abs()
    return (gP, gR, gWg), (run[:, None] * EPS * aP, (run + C1 + 1) * EPS * aR, (E + 1) * EPS * aW)


def ratio(got, ref, cap):
    """Worst |got - ref| / cap over all elements (cap 0: the element must be exact); NaN counts as inf."""
    err = (got.double() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    safe = torch.where(cap > 0, cap, torch.ones_like(cap))
    r = torch.where(cap > 0, err / safe, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0
