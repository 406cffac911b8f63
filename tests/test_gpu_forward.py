"""End-to-end and per-level parity of the HIP forward (pointstowood_amd.Net on cuda:0) against
(a) the golden vectors produced by the reference's own model code and (b) the CPU oracle run live.

Tolerances: indices bit-exact; level features 2e-4 (abs+rel, fp32 accumulation-order noise through
up to 25 layers, K <= 2048); logits 4e-4 absolute, which bounds the wood probability error by 1e-4
(|d sigmoid| <= 0.25 |d logit|) - the north-star's parity bar; probabilities checked at 1e-4 too."""
import numpy as np
import pytest
import torch

from oracle import net as onet
from pointstowood_amd import synthetic_voxels as synth, synthetic_weights as weights
from tests import golden_util as G

pytestmark = pytest.mark.gpu


class _D:
    pass


def _run(inp, C, k, wseed, keep=None, precision="f16x3"):
    from pointstowood_amd import Net
    net = Net(num_classes=1, C=C, k=k, precision=precision)
    net.load_state_dict(weights.synth_state_dict(1, C, seed=wseed), strict=True)
    net = net.cuda().eval()
    d = _D()
    d.pos, d.batch = inp["pos"].cuda(), inp["batch"].cuda()
    d.reflectance, d.sf = inp["reflectance"].cuda(), inp["sf"].cuda()
    out = net(d, keep=keep)
    torch.cuda.synchronize()
    _run.range_fallbacks = net._engine.range_fallbacks    # (forwards the f16x3 range guard recomputed on the fp32 path)
    return out, d


def _edges(lv, k):
    from pointstowood_amd.ops import _edges
    return _edges(lv.nbr[: lv.n], lv.deg[: lv.n])


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("name", G.ALL_CASES)
def test_forward_matches_reference_vectors(name, precision):
    g, inp, meta = G.load(name)
    keep = {}
    logits, d = _run(inp, meta["C"], meta["k"], meta["wseed"], keep, precision)
    geo = keep["geometry"]
    for l in (1, 2, 3):
        lv = geo.levels[l]
        G.check(g, f"idx{l}", lv.idx[: lv.n].long(), what="geometry ")
        e = _edges(lv, meta["k"])
        G.check(g, f"edge{l}.q", e[0], what="geometry ")
        G.check(g, f"edge{l}.c", e[1], what="geometry ")
    G.check(g, "stem", keep["stem"], rtol=1e-5, atol=1e-6)
    assert d.x is keep["stem"]
    for n in ("sa1_module.conv", "sa1_module.out", "sa2_module.conv", "sa2_module.out", "sa3_module.conv",
              "sa3_module.out", "sa4_module.out", "fp4_module.out", "fp3_module.out", "fp2_module.out",
              "fp1_module.out"):
        G.check(g, n, keep[n], rtol=2e-4, atol=2e-4, what="features ")
    G.check(g, "logits", logits, rtol=0.0, atol=4e-4)
    G.check(g, "probs", torch.sigmoid(logits), atol=1e-4)


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_forward_matches_live_oracle_mixed_batch(precision):
    vox = [synth.uniform_voxel(2.0, 5000, 41, True), synth.surface_voxel(2.0, 2500, 42, True),
           synth.uniform_voxel(4.0, 300, 43, False), synth.uniform_voxel(2.0, 16384, 44, True)]
    inp = synth.collate(vox)
    C, k, wseed = 8, 32, 3
    sd = weights.synth_state_dict(1, C, seed=wseed)
    cap = {}
    ref = onet.forward(sd, inp["pos"], inp["batch"], inp["reflectance"], inp["sf"], k=k, capture=cap)
    keep = {}
    got, _ = _run(inp, C, k, wseed, keep, precision)
    geo = keep["geometry"]
    for l in (1, 2, 3):
        lv = geo.levels[l]
        assert torch.equal(lv.idx[: lv.n].long().cpu(), cap[f"sa{l}_module.idx"])
        e = _edges(lv, k).cpu()
        assert torch.equal(e[0], cap[f"sa{l}_module.edge_q"]) and torch.equal(e[1], cap[f"sa{l}_module.edge_c"])
    assert (got.cpu() - ref).abs().max() <= 4e-4
    assert (torch.sigmoid(got.cpu()) - torch.sigmoid(ref)).abs().max() <= 1e-4


# Single-plane precisions (one MFMA per product: the reference's own GPU arithmetic, predicter.py:197 autocast): same
# geometry bit for bit, features to the operand precision; they do NOT meet the 1e-4 probability bar and the limits below
# say by how much (measured max |dprob| over the six reference cases on MI355X: fp16 2.8e-3..1.5e-2, bf16 2.0e-2..1.2e-1;
# configs[4] at full size: fp16 mean 1.4e-3 / 0.18 % of labels flip, bf16 mean 1.1e-2 / 1.5 %).
SINGLE_PLANE_PROB_LIMIT = {"fp16": 3e-2, "bf16": 2.5e-1}


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("name", G.CASES)
def test_single_plane_precisions_against_reference_vectors(name, precision):
    g, inp, meta = G.load(name)
    keep = {}
    logits, d = _run(inp, meta["C"], meta["k"], meta["wseed"], keep, precision)
    geo = keep["geometry"]
    for l in (1, 2, 3):                       # geometry is fp32 and independent of the feature precision
        lv = geo.levels[l]
        G.check(g, f"idx{l}", lv.idx[: lv.n].long(), what="geometry ")
        e = _edges(lv, meta["k"])
        G.check(g, f"edge{l}.c", e[1], what="geometry ")
    G.check(g, "stem", keep["stem"], rtol=1e-5, atol=1e-6)          # the stem is fp32 VALU in every mode
    rel = {"fp16": 3e-2, "bf16": 2.5e-1}[precision]
    G.check(g, "sa1_module.conv", keep["sa1_module.conv"], rtol=rel, atol=rel)
    assert bool(torch.isfinite(logits).all())
    if "probs" in g:
        ref = torch.from_numpy(g["probs"])
        got = torch.sigmoid(logits).cpu()
    else:
        rows = torch.from_numpy(g["probs__rows"].astype(np.int64))
        ref, got = torch.from_numpy(g["probs__sample"]), torch.sigmoid(logits).cpu()[rows]
    err = (got - ref).abs().max().item()
    print(f"{precision} {name}: max |dprob| vs reference = {err:.3e}")
    assert err <= SINGLE_PLANE_PROB_LIMIT[precision], err


@pytest.mark.parametrize("precision", ["f16x3", "fp16"])
def test_multi_class_head(precision):
    """num_classes > 1 (conv2 as one more narrow GEMM, logits [classes, N] like the reference's squeeze(x.t())): the H
    path against the fp32-MFMA path."""
    from pointstowood_amd import Net
    inp = synth.collate([synth.uniform_voxel(2.0, 3000, 51, True), synth.uniform_voxel(2.0, 700, 52, True)])
    sd = weights.synth_state_dict(3, 8, seed=2)
    outs = {}
    for prec in ("fp32", precision):
        net = Net(num_classes=3, C=8, k=32, precision=prec)
        net.load_state_dict(sd, strict=True)
        net = net.cuda().eval()
        d = _D()
        d.pos, d.batch, d.reflectance, d.sf = (inp[n].cuda() for n in ("pos", "batch", "reflectance", "sf"))
        outs[prec] = net(d).cpu()
    assert outs["fp32"].shape == (3, 3700)
    tol = 4e-4 if precision == "f16x3" else 5e-2
    assert (outs[precision] - outs["fp32"]).abs().max() <= tol * max(1.0, outs["fp32"].abs().max().item())


def test_forward_is_deterministic_and_batch_order_is_voxel_major():
    g, inp, meta = G.load("ragged_b2_refl_c8")
    a, _ = _run(inp, meta["C"], meta["k"], meta["wseed"])
    b, _ = _run(inp, meta["C"], meta["k"], meta["wseed"])
    assert torch.equal(a, b)


@pytest.mark.parametrize("precision", ["f16x3", "fp16"])
def test_packed_pointnetconv_is_bit_identical(precision):
    """P2W_SA_PACK8 (targets with <= 8 neighbours share an MFMA tile four at a time, the others keep their own tile) only
    re-arranges the rows of the fused PointNetConv's GEMM: logits must be bit-identical with and without it - on sparse voxels
    (most targets small), on a dense one (ball query at its cap: every target large) and on a mixed batch with tiny voxels."""
    from pointstowood_amd import Net
    batches = [synth.collate([synth.uniform_voxel(2.0, 6000, 81, True), synth.uniform_voxel(2.0, 900, 82, False)]),
               synth.collate([synth.uniform_voxel(0.3, 5000, 83, True)]),                      # dense: ~32 neighbours everywhere
               synth.collate([synth.uniform_voxel(2.0, 3, 84, True), synth.uniform_voxel(1.0, 4000, 85, True),
                              synth.uniform_voxel(4.0, 2000, 86, False)])]
    net = Net(num_classes=1, C=8, k=32, precision=precision)
    net.load_state_dict(weights.synth_state_dict(1, 8, seed=9), strict=True)
    net = net.cuda().eval()

    def mk(b):
        d = _D()
        d.pos, d.batch, d.reflectance, d.sf = b["pos"].cuda(), b["batch"].cuda(), b["reflectance"].cuda(), b["sf"].cuda()
        return d
    outs = {}
    for pack in (True, False):
        net(mk(batches[0]))                    # builds the engine
        net._engine.sa_pack = pack
        outs[pack] = [net(mk(b)).clone() for b in batches]
    torch.cuda.synchronize()
    for a, b in zip(outs[True], outs[False]):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


@pytest.mark.parametrize("option", ["fp1_cell_order", "gemm_stream_k", "fp_hoist", "fp_hoist_everywhere"])
@pytest.mark.parametrize("precision", ["f16x3", "fp16"])
def test_engine_switches_keep_the_logits(option, precision):
    """The A/B switches give the default path's results: `fp1_cell_order` (level-0 features in the sampler's cell order, logits
    scattered back: rows are only re-arranged) bit for bit; `gemm_stream_k` (GEMM rows behind the whole chip rounds as a split-K tail: a tail tile's K range is
    summed in pieces) and `fp_hoist` (an FP module's layer 0 on the coarse rows, interpolation in the GEMM's epilogue; "everywhere":
    all four modules take the route, FP1 on rows in cell order) within the last fp32 bits of the accumulators, far inside the
    parity bar - on ragged batches with tiny voxels, through forward and through Net.stream."""
    from pointstowood_amd import Net
    batches = [synth.collate([synth.uniform_voxel(2.0, 6000, 91, True), synth.uniform_voxel(2.0, 900, 92, False)]),
               synth.collate([synth.uniform_voxel(2.0, 3, 94, True), synth.uniform_voxel(1.0, 4000, 95, True),
                              synth.uniform_voxel(4.0, 2000, 96, False), synth.uniform_voxel(2.0, 40, 97, True)]),
               synth.collate([synth.surface_voxel(2.0, 12000, 98, False)])]
    sd = weights.synth_state_dict(1, 32, seed=4)

    def mk(b):
        d = _D()
        d.pos, d.batch, d.reflectance, d.sf = b["pos"].cuda(), b["batch"].cuda(), b["reflectance"].cuda(), b["sf"].cuda()
        return d
    outs = {}
    for on in (False, True):
        kw = dict(fp_hoist=on, fp_hoist_ratio=1.0, fp1_cell_order=True) if option == "fp_hoist_everywhere" else {option: on}
        net = Net(num_classes=1, C=32, k=32, precision=precision, **kw)
        net.load_state_dict(sd, strict=True)
        net = net.cuda().eval()
        outs[on] = [net(mk(b)).clone() for b in batches] + [o.clone() for o in net.stream(mk(b) for b in batches)]
    torch.cuda.synchronize()
    for a, b in zip(outs[True], outs[False]):
        assert bool(torch.isfinite(a).all()) and a.shape == b.shape
        if option in ("gemm_stream_k", "fp_hoist", "fp_hoist_everywhere"):   # (fp_hoist: the same function with the interpolation behind the coarse GEMM)
            lim = 6e-5 if precision == "f16x3" else 6e-2    # (fp16: an H value one rounding apart moves a logit by ~1e-3 .. 1e-2)
            assert (a - b).abs().max() <= lim
        else:
            assert torch.equal(a, b)


def test_stream_pipeline_equals_sequential_forward():
    """Net.stream (geometry of batch i+1 overlapped with features of batch i on a second HIP stream) must return
    bit-identical logits to one forward per batch, in order."""
    from pointstowood_amd import Net
    vox = [synth.uniform_voxel(2.0, n, 70 + i, i % 2 == 0) for i, n in enumerate((3000, 800, 5000, 256, 2048, 4096))]
    batches = [synth.collate(vox[0:2]), synth.collate(vox[2:3]), synth.collate(vox[3:6]), synth.collate(vox[1:3])]
    net = Net(num_classes=1, C=8, k=32)
    net.load_state_dict(weights.synth_state_dict(1, 8, seed=5), strict=True)
    net = net.cuda().eval()

    def mk(b):
        d = _D()
        d.pos, d.batch, d.reflectance, d.sf = b["pos"].cuda(), b["batch"].cuda(), b["reflectance"].cuda(), b["sf"].cuda()
        return d
    seq = [net(mk(b)).clone() for b in batches]
    torch.cuda.synchronize()
    for _ in range(2):
        got = [o.clone() for o in net.stream(mk(b) for b in batches)]
        torch.cuda.synchronize()
        assert len(got) == len(seq) and all(torch.equal(a, b) for a, b in zip(got, seq))
    # feature phases of several batches in flight (the default is 2), with and without the second chunk-chain stream, over a
    # longer sequence: same logits, same order
    many = [batches[i % 4] for i in range(11)]
    for kw in (dict(feature_streams=1, res_streams=1), dict(feature_streams=2, res_streams=2, res_chunk_rows=2048),
               dict(feature_streams=3, res_streams=1)):
        net2 = Net(num_classes=1, C=8, k=32, **kw)
        net2.load_state_dict(weights.synth_state_dict(1, 8, seed=5), strict=True)
        net2 = net2.cuda().eval()
        got = [o.clone() for o in net2.stream(mk(b) for b in many)]
        torch.cuda.synchronize()
        own = [net2(mk(b)).clone() for b in batches]       # (another chunking plans other split-K tails: last fp32 bits may differ
        assert len(got) == 11 and all(torch.equal(a, own[i % 4]) for i, a in enumerate(got)), kw   # from `seq`, never from `own`)
        assert all((a - seq[i % 4]).abs().max() <= 2e-4 for i, a in enumerate(got)), kw
    # the table sampler's overflow redo INSIDE the pipeline (the geometry of that batch is replaced while the next one's is being
    # launched): a fresh engine whose first call is the stream, the oversized batch (three 4 m voxels) in it twice
    big = synth.collate([synth.uniform_voxel(4.0, 6000, 190 + i, True) for i in range(3)])
    mixed = [batches[0], big, batches[1], big]
    nets = []
    for _ in range(2):
        nets.append(Net(num_classes=1, C=8, k=32))
        nets[-1].load_state_dict(weights.synth_state_dict(1, 8, seed=5), strict=True)
        nets[-1] = nets[-1].cuda().eval()
    got = [o.clone() for o in nets[0].stream(mk(b) for b in mixed)]
    torch.cuda.synchronize()
    # level 0 of that batch takes the sort by itself (3 x 216 000 cells > 32 per point x 18 000 points); level 1's table holds
    # 31 cells of 0.08 m per axis and voxel, a 4 m voxel spans 50: that level overflows
    print("table scale after the stream:", nets[0]._engine._table_scale)
    assert nets[0]._engine._table_scale[1] >= 8              # (it was 1: the redo ran in the stream)
    own = [nets[1](mk(b)).clone() for b in mixed]
    torch.cuda.synchronize()
    assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got, own))


def test_lone_forward_with_searches_beside_the_features_is_bit_identical():
    """EngineOptions.overlap (default): inside ONE forward the six searches run on a second stream beside the feature phase
    (per-search events, the stem and SA1's hoisted product enqueued before the host waits for the level sizes).  Same logits,
    bit for bit, as the strictly sequential order - also with the 8-launch sampler entry point, the searches enqueued first,
    one chunk chain, a high-priority search stream - on ragged batches, a batch whose table sampler overflows (4 m voxels:
    the geometry is redone with the sort while the discarded searches are still in flight) and repeated calls."""
    from pointstowood_amd import Net
    vox = [synth.uniform_voxel(2.0, n, 170 + i, i % 2 == 0) for i, n in enumerate((3000, 800, 5000, 256, 2048, 4096))]
    big = [synth.uniform_voxel(4.0, 6000, 190 + i, True) for i in range(3)]
    batches = [synth.collate(vox[0:2]), synth.collate(big), synth.collate(vox[2:3]), synth.collate(vox[3:6]), synth.collate(big[:1] + vox[:1])]

    def mk(b):
        d = _D()
        d.pos, d.batch, d.reflectance, d.sf = b["pos"].cuda(), b["batch"].cuda(), b["reflectance"].cuda(), b["sf"].cuda()
        return d

    def run(**kw):
        net = Net(num_classes=1, C=8, k=32, **kw)
        net.load_state_dict(weights.synth_state_dict(1, 8, seed=5), strict=True)
        net = net.cuda().eval()
        outs = [net(mk(b)).clone() for b in batches] + [net(mk(b)).clone() for b in batches[:2]]
        torch.cuda.synchronize()
        assert net._engine.range_fallbacks == 0
        return outs
    ref = run(overlap=False, single_res_streams=1)
    for kw in (dict(), dict(table_prepared=False), dict(early_first=False), dict(single_res_streams=1), dict(search_priority=-1),
               dict(search_stagger=True), dict(overlap=False)):
        got = run(**kw)
        if kw.get("single_res_streams", 2) == 1 or "overlap" in kw:
            assert all(torch.equal(a, b) for a, b in zip(got, ref)), kw
        else:   # (two chunk chains plan the same GEMMs: these small batches have one chunk per level, so the bits agree too)
            assert all(torch.equal(a, b) for a, b in zip(got, ref)), kw


def test_table_sampler_recovers_after_oversized_voxels():
    """one batch of 4 m voxels grows the table sampler's remembered extent (x 8); a later batch of MANY nominal 2 m voxels,
    for which a table of that extent no longer fits, must not fall to the sort sampler for the life of the engine: it probes the
    largest smaller table that fits - and gets it.  Same logits as a fresh engine either way."""
    from pointstowood_amd import Net
    sd = weights.synth_state_dict(1, 8, seed=2)

    def mk(vox):
        b = synth.collate(vox)
        d = _D()
        d.pos, d.batch, d.reflectance, d.sf = b["pos"].cuda(), b["batch"].cuda(), b["reflectance"].cuda(), b["sf"].cuda()
        return d
    big = [synth.uniform_voxel(4.0, 12000, 500 + i, False) for i in range(3)]
    many = [synth.uniform_voxel(2.0, 7000, 600 + i, False) for i in range(48)]     # 48 x 216000 x 8 cells > the table's maximum
    net = Net(num_classes=1, C=8, k=32)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    keep = {"geometry_only": True}
    net(mk(big), keep=keep)
    eng = net._engine
    assert eng._table_scale[0] >= 8                      # the 4 m voxels overflowed the nominal level-0 table once
    keep = {"geometry_only": True}
    out = net(mk(many), keep=keep)
    assert 0 in keep["geometry"].table_levels and 0 in keep["geometry"].table_probes     # level 0 ran on a (probed) table, not the sort
    fresh = Net(num_classes=1, C=8, k=32)
    fresh.load_state_dict(sd, strict=True)
    fresh = fresh.cuda().eval()
    assert torch.equal(out, fresh(mk(many)))


def _rescaled(sd, spots, s):
    """`sd` with the activations at `spots` multiplied by s and the consuming weights divided by s: the same function (ReLU and
    the eval-mode BatchNorm / depthwise affines are positively homogeneous), but the tensors BETWEEN the two GEMMs are s times
    as large - what a checkpoint with extreme BatchNorm scales does to an arithmetic with a limited range."""
    out = {k: v.clone() for k, v in sd.items()}
    for kind, p in spots:
        if kind == "dsc":      # residual block: second depthwise-separable conv - its BN + ReLU output is the pointwise conv's input
            out[p + ".depthwise_bn.weight"] *= s
            out[p + ".depthwise_bn.bias"] *= s
            out[p + ".pointwise_conv.weight"] /= s
        else:                  # MLP (model.py:198-202): layer 0 = Lin + ReLU, its output is layer 1's input
            out[p + ".0.0.weight"] *= s
            out[p + ".0.0.bias"] *= s
            out[p + ".1.0.weight"] /= s
    return out


@pytest.mark.parametrize("scale", [1.0e6, 1.0e-7])
def test_range_guard_recomputes_what_f16x3_cannot_carry(scale):
    """A recipe checkpoint whose intermediate activations sit at 1e6 (the fp16 hi plane saturates at 65504) or at 1e-7 (both
    planes on fp16's subnormal floor): the forward must still meet the parity bar against the fp32 oracle - the range watch
    sees the layer, the batch is recomputed on the fp32 MFMA path, a warning says so - through forward and through Net.stream;
    an ordinary checkpoint never takes the fallback.  Without the guard the same checkpoint is silently wrong."""
    import warnings
    from pointstowood_amd import Net
    sd0 = weights.synth_state_dict(1, 8, seed=3)
    spots = [("dsc", "sa2_module.residual_block.conv.3"), ("mlp", "fp2_module.NN")]
    sd = _rescaled(sd0, spots, scale)
    vox = [synth.uniform_voxel(2.0, 3000, 31, True), synth.uniform_voxel(2.0, 1200, 32, False)]
    b = synth.collate(vox)
    ref = onet.forward(sd, b["pos"].clone(), b["batch"], b["reflectance"], b["sf"], k=32)
    ref0 = onet.forward(sd0, b["pos"].clone(), b["batch"], b["reflectance"], b["sf"], k=32)
    assert (ref - ref0).abs().max() < 2e-4           # the rescaled checkpoint IS the same function

    def mk():
        d = _D()
        d.pos, d.batch, d.reflectance, d.sf = b["pos"].cuda(), b["batch"].cuda(), b["reflectance"].cuda(), b["sf"].cuda()
        return d
    net = Net(num_classes=1, C=8, k=32)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = net(mk()).cpu()
        outs = [o.cpu() for o in net.stream(mk() for _ in range(3))]
    assert net._engine.range_fallbacks == 4 and any("fp32 MFMA path" in str(x.message) for x in w)
    for o in [out] + outs:
        assert (o - ref).abs().max() <= 4e-4 and (torch.sigmoid(o) - torch.sigmoid(ref)).abs().max() <= 1e-4
    # the ordinary checkpoint stays on the f16x3 path
    net0 = Net(num_classes=1, C=8, k=32)
    net0.load_state_dict(sd0, strict=True)
    net0 = net0.cuda().eval()
    o0 = net0(mk()).cpu()
    assert net0._engine.range_fallbacks == 0 and (o0 - ref0).abs().max() <= 4e-4
    # ... and this is what the guard is for
    raw = Net(num_classes=1, C=8, k=32, range_guard=False)
    raw.load_state_dict(sd, strict=True)
    raw = raw.cuda().eval()
    assert (raw(mk()).cpu() - ref).abs().max() > 1e-3


def test_predict_cli_on_a_voxel_directory(tmp_path):
    """predict.py --voxels: dataset feed -> sampler -> forward -> sigmoid/threshold/un-shift, against the CPU oracle."""
    import importlib.util
    import os
    from oracle import host as ohost
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("p2w_predict", os.path.join(root, "predict.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    g = torch.Generator().manual_seed(9)
    vdir = tmp_path / "voxels"
    vdir.mkdir()
    raws = []
    for i, n in enumerate((600, 1500, 300)):
        pc = torch.cat([torch.rand(n, 3, generator=g) * 2 + 40 * i, torch.rand(n, 1, generator=g) * 2 - 1, torch.rand(n, 2, generator=g)], 1)
        torch.save(pc, vdir / f"voxel_{i}.pt")
        raws.append(pc)
    sd = weights.synth_state_dict(1, 32, seed=0)
    torch.save({"model_state_dict": {"module." + k: v for k, v in sd.items()}}, tmp_path / "m.pth")
    out = mod.main(["--voxels", str(vdir), "--model", str(tmp_path / "m.pth"), "--odir", str(tmp_path / "o"),
                    "--batch_size", "2", "--is-wood", "0.5"])
    assert out.shape == (2400, 5) and os.path.exists(tmp_path / "o" / "classified_voxels.npy")
    torch.set_num_threads(min(os.cpu_count() or 1, 16))   # predict.py sets all cores like the reference; the oracle crawls there
    # oracle: classify every voxel alone is NOT equivalent (batch-global grid origin), so rebuild the same batches
    from pointstowood_amd.predicter import PointBudgetSampler, VoxelDataset
    ds = VoxelDataset(str(vdir))
    ref_rows = []
    for batch in PointBudgetSampler(ds.preload(), 262144, 256):      # the CLI's default: forwards packed by a point budget
        feeds = [ohost.feed(ds.raw(i)) for i in batch]
        b = synth.collate(feeds)
        logits = onet.forward(sd, b["pos"], b["batch"], b["reflectance"], b["sf"], k=32)
        ref_rows.append(ohost.consume(logits, b["pos"], b["batch"], b["local_shift"], 0.5))
    ref = np.vstack(ref_rows)
    assert np.abs(out[:, :3] - ref[:, :3]).max() <= 1e-4            # un-shifted coordinates
    assert np.abs(out[:, 4] - ref[:, 4]).max() <= 1e-4              # wood probability
    far = np.abs(ref[:, 4] - 0.5) > 2e-4
    assert (out[far, 3] == ref[far, 3]).all()                        # labels (away from the decision threshold)
    # --reference-sampler: the reference's BalancedBatchSampler (global numpy RNG, remainder dropped) through the same stream
    # pipeline = one classify_batch per batch of that sampler under the same seed, row for row
    from pointstowood_amd import DataLoader, Net
    from pointstowood_amd.predicter import BalancedBatchSampler, classify_batch, load_model
    np.random.seed(5)
    out_ref = mod.main(["--voxels", str(vdir), "--model", str(tmp_path / "m.pth"), "--odir", str(tmp_path / "o2"),
                        "--batch_size", "2", "--reference-sampler"])
    torch.set_num_threads(min(os.cpu_count() or 1, 16))   # (main() sets all cores again: every later CPU-oracle test would crawl)
    net = Net(num_classes=1).cuda()
    load_model(str(tmp_path / "m.pth"), net, "cuda")
    net.eval()
    np.random.seed(5)
    loop = np.vstack([classify_batch(net, d, 0.5, "cuda")
                      for d in DataLoader(ds, batch_sampler=BalancedBatchSampler(ds, 2, reference=True), num_workers=0)])
    assert out_ref.shape == loop.shape and out_ref.shape[0] < 2400 and np.array_equal(out_ref, loop)   # (3 voxels, 2 per batch: one dropped)


def test_voxeliser_on_gpu_matches_cpu_restatement():
    from oracle import preprocess as OP
    from pointstowood_amd import preprocessing as PP
    from tests.test_host_cpu import _plot
    pc = _plot(n=40000, seed=3, refl=True)
    ref, nz_ref = OP.voxelise(pc, (2.0, 4.0), min_pts=64, max_pts=100000)
    got, nz = PP.voxelise(pc.cuda(), (2.0, 4.0), min_pts=64, max_pts=100000)
    assert torch.equal(nz.cpu(), nz_ref) and len(got) == len(ref)
    for a, b in zip(got, ref):
        a = a.cpu()
        assert a.shape == b.shape
        cols = [0, 1, 2] + list(range(4, b.shape[1]))
        assert torch.equal(a[:, cols], b[:, cols])                       # membership, order, coordinates, n_z: exact
        assert (a[:, 3] - b[:, 3]).abs().max() <= 5e-5                   # erfinv differs in the last bits between devices


def test_bench_contract_line():
    """bench.py --full prints ONE JSON line with the contract's keys (driver contract + roofline + cpu_baseline objects)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--steps", "3", "--warmup", "1", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, P2W_BENCH_WATCHDOG="300"))
    assert r.returncode == 0, r.stderr[-6000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in d, key
    assert d["metric"] == "classified points/sec" and d["unit"] == "points/s" and d["n_gpus"] == 1 and d["steps"] == 3
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    rf = d["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in rf, key
    assert rf["bound"] in ("hbm", "mfma") and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    assert abs(d["value"] - 8 * 16384 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    # the diagnostics come first, the contract keys last (a reader that keeps the line's tail keeps them); the lone-forward and the
    # PCIe-inclusive figures close the line
    keys = list(d)
    assert keys.index("workloads") < keys.index("metric") < keys.index("roofline") < keys.index("single_call") < keys.index("pcie_inclusive")
    assert keys[-1] == "pcie_inclusive" and d["single_call"]["ms_per_step"] > 0 and d["pcie_inclusive"]["ms_per_step"] > 0
    assert "error" not in d["workloads"]


def test_bench_plain_line_and_outputs(tmp_path):
    """A plain bench.py run prints ONE JSON line with the headline keys and nothing of --full; --dump-outputs writes the last
    timed step's logits, and a second run on the same arguments writes the same bits."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for i in range(2):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "5", "--warmup", "1",
                            "--dump-outputs", str(tmp_path / str(i))],
                           capture_output=True, text=True, timeout=300, env=dict(os.environ, P2W_BENCH_WATCHDOG="240"))
        assert r.returncode == 0, r.stderr[-6000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert d["metric"] == "classified points/sec" and d["unit"] == "points/s" and d["higher_is_better"] is True
        assert d["dtype"] == "f16x3" and d["steps"] == 5 and d["warmup"] == 1 and d["ms_per_step"] > 0
        assert abs(d["value"] - 8 * 16384 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
        for key in ("roofline", "workloads", "cpu_baseline", "single_call", "pcie_inclusive", "search", "kernel_ms_per_step"):
            assert key not in d, key
        assert sorted(os.listdir(tmp_path / str(i))) == ["logits.npy"]
        outs.append(np.load(tmp_path / str(i) / "logits.npy"))
    assert outs[0].dtype == np.float32 and outs[0].shape == (8 * 16384,) and np.isfinite(outs[0]).all()
    assert np.array_equal(outs[0], outs[1])


# ---- INTEGRATION.md route B as a composition: the reference forward's statements over pointstowood_amd.ops -----------------
@pytest.mark.parametrize("name", ["u2_2k_k16_c32", "ragged_b2_refl_c8", "surface_cap_c4"])
def test_reference_forward_over_the_operator_module_matches_reference_vectors(name):
    """oracle/net.py restates Net.forward statement by statement over an operator module; with ops = pointstowood_amd.ops
    (voxel_grid, consecutive_cluster, radius, knn, scatter_max, global_max_pool, knn_interpolate on the GPU, the dense
    layers by PyTorch on the same device) the composition must reproduce the vectors the reference's own model produced:
    what a maintainer gets from swapping the imports of src/model.py (route B)."""
    from pointstowood_amd import ops as H
    g, inp, meta = G.load(name)
    sd = {k: v.cuda() for k, v in weights.synth_state_dict(1, meta["C"], seed=meta["wseed"]).items()}
    cap = {}
    logits = onet.forward(sd, inp["pos"].cuda(), inp["batch"].cuda(), inp["reflectance"].cuda(), inp["sf"].cuda(),
                          k=meta["k"], capture=cap, ops=H)
    assert onet.ops.__name__ == "oracle.ops"     # the swap is scoped to the call
    for l in (1, 2, 3):
        G.check(g, f"idx{l}", cap[f"sa{l}_module.idx"], what="route B ")
        G.check(g, f"edge{l}.q", cap[f"sa{l}_module.edge_q"], what="route B ")
        G.check(g, f"edge{l}.c", cap[f"sa{l}_module.edge_c"], what="route B ")
    for n in ("sa1_module.conv", "sa2_module.out", "sa3_module.out", "sa4_module.out", "fp4_module.out", "fp1_module.out"):
        G.check(g, n, cap[n], rtol=2e-4, atol=2e-4, what="route B ")
    G.check(g, "logits", logits, rtol=1e-4, atol=4e-4)
    G.check(g, "probs", torch.sigmoid(logits), atol=1e-4)


def test_engine_switches_are_keyword_arguments_and_do_not_change_results():
    """EngineOptions through Net(...): every combination gives bit-identical logits (sort sampler, whole-voxel searches,
    no packing of low-degree targets, no search hints), and nothing is read from the environment."""
    import os
    from pointstowood_amd import Net
    from pointstowood_amd.engine import EngineOptions
    inp = synth.collate([synth.uniform_voxel(2.0, 6000, 61, True), synth.surface_voxel(2.0, 3000, 62, True)])
    sd = weights.synth_state_dict(1, 8, seed=4)
    d = _D()
    d.pos, d.batch, d.reflectance, d.sf = (inp[k].cuda() for k in ("pos", "batch", "reflectance", "sf"))
    outs = []
    os.environ["P2W_SAMPLER"], os.environ["P2W_SEARCH"] = "nonsense", "nonsense"     # would have been read (and broken) before
    try:
        for kw in ({}, dict(sampler="sort"), dict(search="brute"), dict(sa_pack=False, fp_hints=False), dict(table_cells_per_point=0.0),
                   dict(res_streams=1, chunk_full_rounds=False), dict(search_index=False, search_box=7), dict(res_chunk_rows=4096)):
            net = Net(num_classes=1, C=8, k=32, **kw)
            net.load_state_dict(sd, strict=True)
            outs.append(net.cuda().eval()(d).clone())
            assert net._engine.options == EngineOptions(**kw)
    finally:
        del os.environ["P2W_SAMPLER"], os.environ["P2W_SEARCH"]
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    with pytest.raises(TypeError):
        Net(num_classes=1, C=8, no_such_option=1)
    with pytest.raises(ValueError):
        Net(num_classes=1, C=8, sampler="hash")


def _fuzz_voxel(rng, seed):
    """One random voxel: a generator, a size from a few points to a few thousand, and one of the shapes that stress the
    geometry kernels' tie rules (exact duplicates, points in a plane, points on a lattice, a tiny extent)."""
    n = int(rng.choice([12, 40, 130, 700, 1500, 3000, 6000]))
    side = float(rng.choice([0.5, 2.0, 4.0, 9.0]))       # (the voxeliser makes 2 m and 4 m cells; the forward takes any extent)
    refl = bool(rng.integers(0, 2))
    v = synth.surface_voxel(side, max(n, 60), seed, refl) if rng.random() < 0.3 else synth.uniform_voxel(side, n, seed, refl)
    p = v["pos"] + v["local_shift"]
    kind = int(rng.integers(0, 5))
    if kind == 1:                                   # a fifth of the points are exact copies of others
        m = max(1, p.shape[0] // 5)
        p[-m:] = p[:m]
    elif kind == 2:                                 # all points in one horizontal plane
        p[:, 2] = p[0, 2]
    elif kind == 3:                                 # lattice: equal distances everywhere (ties decided by index)
        p = torch.round(p / 0.125) * 0.125
    elif kind == 4:                                 # 5 cm extent: every level's grid collapses to a few cells
        p = p * 0.025
    return synth._finish(p.contiguous(), v["reflectance"])


def _fp_neighbours_expected(geo, f):
    """knn_interpolate's k = 2 assignment of fine level f into level f + 1 by the CPU oracle, as [n, 2] (-1 = no neighbour)."""
    from oracle import ops as oops
    fine, coarse = geo.levels[f], geo.levels[f + 1]
    nf, nc = fine.n, coarse.n
    e = oops.knn(coarse.xyzr[:nc, :3].cpu(), fine.xyzr[:nf, :3].cpu(), 2, batch_x=coarse.batch[:nc].cpu().long(),
                 batch_y=fine.batch[:nf].cpu().long())
    first = torch.ones(e.shape[1], dtype=torch.bool)
    first[1:] = e[0, 1:] != e[0, :-1]
    exp = torch.full((nf, 2), -1, dtype=torch.long)
    exp[e[0][first], 0] = e[1][first]
    exp[e[0][~first], 1] = e[1][~first]
    return exp


_FUZZ0 = int(__import__("os").environ.get("P2W_FUZZ_SEED0", "0"))     # (longer hunts: P2W_FUZZ_SEED0=1000 P2W_FUZZ_SEEDS=1500)


@pytest.mark.parametrize("seed", range(_FUZZ0, _FUZZ0 + int(__import__("os").environ.get("P2W_FUZZ_SEEDS", "24"))))
def test_forward_fuzz_against_live_oracle(seed):
    """Random small batches (ragged sizes down to fewer points than k, duplicates, planes, lattices, tiny extents, reflectance
    on and off, C and k varied): neighbour structure bit-exact, wood probability within 1e-4 of the CPU oracle."""
    rng = np.random.default_rng(1000 + seed)
    B = int(rng.integers(1, 6))
    vox = [_fuzz_voxel(rng, 5000 + 17 * seed + b) for b in range(B)]
    if not any(bool((v["reflectance"] != 0).any()) for v in vox) and seed % 2:
        vox[0]["reflectance"] = torch.linspace(-1, 1, vox[0]["pos"].shape[0])
    inp = synth.collate(vox)
    C, k, wseed = int(rng.choice([4, 8])), int(rng.choice([8, 16, 32])), int(rng.integers(0, 100))
    sd = weights.synth_state_dict(1, C, seed=wseed)
    cap = {}
    ref = onet.forward(sd, inp["pos"], inp["batch"], inp["reflectance"], inp["sf"], k=k, capture=cap)
    keep = {}
    got, _ = _run(inp, C, k, wseed, keep, "f16x3")
    geo = keep["geometry"]
    for l in (1, 2, 3):
        lv = geo.levels[l]
        assert torch.equal(lv.idx[: lv.n].long().cpu(), cap[f"sa{l}_module.idx"]), f"level {l} sample"
        e = _edges(lv, k).cpu()
        assert torch.equal(e[0], cap[f"sa{l}_module.edge_q"]) and torch.equal(e[1], cap[f"sa{l}_module.edge_c"]), f"level {l} edges"
    for f in (0, 1, 2):   # the interpolation searches (a bogus-hint rescan once returned the nearest point twice)
        nbr, deg = geo.fp_nbr[f]
        n = geo.levels[f].n
        ours = nbr[:n].cpu().long().clone()
        ours[torch.arange(2)[None, :] >= deg[:n].cpu().long()[:, None]] = -1
        if f == 0 and geo.rows0_sorted:   # level 0's rows are kept in the sampler's cell order (fp1_cell_order)
            unsorted = torch.empty_like(ours)
            unsorted[geo.order[:n].cpu().long()] = ours
            ours = unsorted
        assert torch.equal(ours, _fp_neighbours_expected(geo, f)), f"interpolation neighbours of level {f}"
    assert torch.isfinite(got).all()
    assert _run.range_fallbacks == 0      # recipe weights on degenerate geometry still sit inside what f16x3 carries: no fp32 fallback
    assert bool(((got.cpu() - ref).abs() <= 4e-4 + 2e-5 * ref.abs()).all())   # (logits of tiny voxels reach +-60)
    assert (torch.sigmoid(got.cpu()) - torch.sigmoid(ref)).abs().max() <= 1e-4


@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("P2W_FUZZ_STREAMS", "3"))))
def test_stream_pipeline_fuzz(seed):
    """A random sequence of ragged batches through Net.stream (tables, workspaces and allocator pools are re-used across
    batches of very different shapes): bit-identical to one forward per batch on a fresh model."""
    from pointstowood_amd import Net
    rng = np.random.default_rng(7000 + seed)
    C, k = int(rng.choice([4, 8])), int(rng.choice([8, 32]))
    batches = []
    for i in range(9):
        vox = [_fuzz_voxel(rng, 9000 + 100 * seed + 10 * i + b) for b in range(int(rng.integers(1, 5)))]
        batches.append(synth.collate(vox))

    def mk(b):
        d = _D()
        d.pos, d.batch, d.reflectance, d.sf = b["pos"].cuda(), b["batch"].cuda(), b["reflectance"].cuda(), b["sf"].cuda()
        return d

    def model():
        net = Net(num_classes=1, C=C, k=k)
        net.load_state_dict(weights.synth_state_dict(1, C, seed=seed), strict=True)
        return net.cuda().eval()
    seq = []
    for b in batches:
        seq.append(model()(mk(b)).clone())      # a fresh engine per batch: no state carried over
    net = model()
    for _ in range(2):
        got = [o.clone() for o in net.stream(mk(b) for b in batches)]
        torch.cuda.synchronize()
        assert len(got) == len(seq)
        for i, (a, b) in enumerate(zip(got, seq)):
            assert torch.equal(a, b), f"batch {i}"
