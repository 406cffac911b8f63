"""The Poly-1 focal loss, the parts that need no GPU: tests/loss_ref.py against the values recorded from the reference's class, the
fixtures' integrity, the module's and the C entry point's argument checks (they return before any launch)."""
import ctypes
import hashlib
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

from pointstowood_amd import _lib
from pointstowood_amd import loss as PL
from tests import loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "loss")
CASES = [(c, k) for c in R.CONFIGS for k in R.LABEL_KINDS]
NAN = float("nan")


def _inputs():
    return dict(np.load(os.path.join(GOLDEN, "inputs.npz")))


def _rel_close(got, want, rel):
    return bool(np.all(np.abs(got - want) <= rel * np.abs(want)))


def test_fixture_inputs_follow_the_recipe():
    inp, made = _inputs(), R.make_inputs()
    assert int(inp["seed"]) == R.FIXTURE_SEED and len(inp["logits"]) == 17 + 4099
    for k, v in made.items():
        assert v.dtype == np.float32 and np.array_equal(v, inp[k], equal_nan=True), k
    edge = inp["logits"][:17]
    assert np.isnan(edge[10]) and np.isinf(edge[11]) and np.isinf(edge[12]) and edge[0] == 10 and edge[2] > 10 and edge[13] < 10
    assert set(np.unique(inp["labels"])) == {0.0, 1.0} and 0 <= inp["labels_soft"].min() and inp["labels_soft"].max() <= 1
    recorded = json.load(open(os.path.join(GOLDEN, "configs.json")))
    assert recorded == {k: {"kwargs": kw, "weight": w} for k, (kw, w) in R.CONFIGS.items()}


@pytest.mark.parametrize("config,kind", CASES)
def test_loss_ref_equals_the_recorded_float64_reference(config, kind):
    """Every element, losses and gradients, to 1e-12 relative - so the rows whose recorded value is 0 (the NaN logit's loss, the
    gradient beyond +-10 and at NaN / +-inf) must be exactly 0; the reduced values and their gradients too."""
    logits, labels, weight, kwargs = R.case_tensors(_inputs(), config, kind)
    g = np.load(os.path.join(GOLDEN, f"{config}__{kind}.npz"))
    loss, dloss = R.reference(logits, labels, weight, **kwargs)
    assert loss.dtype == np.float64 and np.isfinite(loss).all() and np.isfinite(dloss).all()
    assert _rel_close(loss, g["loss64"], 1e-12) and _rel_close(dloss, g["grad64"], 1e-12)
    assert loss[10] == 0 and dloss[10] == 0                                    # NaN logit
    beyond = ~((logits >= -10) & (logits <= 10))
    assert beyond[[2, 3, 4, 5, 10, 11, 12, 15, 16]].all() and not beyond[[0, 1, 13, 14]].any()
    assert (dloss[beyond] == 0).all() and (g["grad64"][beyond] == 0).all() and (g["grad32"][beyond] == 0).all()
    assert dloss[0] != 0 and dloss[1] != 0                                     # exactly +-10 keeps its gradient
    inf = [11, 12]                                                             # +-inf: the loss of the clamped logit
    w_inf = weight[inf] if weight is not None and len(weight) > 1 else weight
    assert np.array_equal(loss[inf], R.reference(np.asarray([10.0, -10.0]), labels[inf], w_inf, **kwargs)[0])
    n = len(loss)
    red = kwargs["reduction"]
    if red == "none":
        assert np.array_equal(g["reduced64"], g["loss64"]) and np.array_equal(g["rgrad64"], g["grad64"])
    else:
        want = loss.sum() / (n if red == "mean" else 1)
        assert abs(want - float(g["reduced64"])) <= 1e-12 * abs(want)
        assert _rel_close(dloss / (n if red == "mean" else 1), g["rgrad64"], 1e-12)
    # the torch restatement, differentiated by autograd in float64, is the same function
    x = torch.from_numpy(logits).double().requires_grad_()
    w = None if weight is None else torch.from_numpy(weight).double()
    out = R.composite(x, torch.from_numpy(labels).double(), w, **dict(kwargs, reduction="none"))
    out.sum().backward()
    assert _rel_close(out.detach().numpy(), g["loss64"], 1e-12) and _rel_close(x.grad.numpy(), g["grad64"], 1e-12)


def test_recorded_noise_is_the_references_own_float32_error():
    noise = json.load(open(os.path.join(GOLDEN, "noise.json")))["cases"]
    assert sorted(noise) == sorted(f"{c}__{k}" for c, k in CASES)
    for name, v in noise.items():
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        assert v["loss"] == float(np.abs(g["loss32"].astype(np.float64) - g["loss64"]).max())
        assert v["grad"] == float(np.abs(g["grad32"].astype(np.float64) - g["grad64"]).max())
        assert 1e-8 < v["loss"] < 1e-5 and 1e-8 < v["grad"] < 1e-5, (name, v)


def test_loss_fixture_manifest_matches_the_files():
    man = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    files = sorted(f for f in os.listdir(GOLDEN) if f != "manifest.json")
    assert sorted(man) == files and len(files) == len(CASES) + 3
    for f in files:
        assert hashlib.sha256(open(os.path.join(GOLDEN, f), "rb").read()).hexdigest() == man[f], f
        assert os.path.getsize(os.path.join(GOLDEN, f)) < 1 << 20


def test_loss_chunk_mirrors_the_header():
    hdr = open(os.path.join(ROOT, "include", "p2w.h")).read()
    assert int(re.search(r"#define P2W_LOSS_CHUNK (\d+)", hdr).group(1)) == _lib.LOSS_CHUNK
    assert _lib.LOSS_CHUNK % 1024 == 0


HOST_MAIN = r"""
#include "p2w_loss.hip"
#include <cstdio>
#include <cstdlib>
#include <vector>
static std::vector<float> rd(const char* f, size_t n) {
    std::vector<float> v(n);
    FILE* h = fopen(f, "rb");
    if (!h || fread(v.data(), 4, n, h) != n) abort();
    fclose(h);
    return v;
}
// argv: n logits labels weight(or -) epsilon gamma alpha label_smoothing eps out
int main(int argc, char** argv) {
    if (argc != 11) return 2;
    const size_t n = strtoul(argv[1], nullptr, 10);
    const auto x = rd(argv[2], n), y = rd(argv[3], n);
    std::vector<float> w(n, 1.0f);
    if (argv[4][0] != '-') w = rd(argv[4], n);
    const double epsilon = atof(argv[5]), gamma = atof(argv[6]), alpha = atof(argv[7]), ls = atof(argv[8]), eps = atof(argv[9]);
    LfParams P;                                  // as p2w_poly1_focal fills it
    P.epsilon = (float)epsilon; P.gamma = (float)gamma; P.gamma1 = (float)(gamma + 1.0);
    P.eps_lo = (float)eps; P.eps_hi = (float)(1.0 - eps);
    P.has_alpha = alpha == alpha; P.alpha = P.has_alpha ? (float)alpha : 0.0f; P.alpha1 = P.has_alpha ? (float)(1.0 - alpha) : 0.0f;
    P.has_ls = ls == ls; P.ls_scale = P.has_ls ? (float)(1.0 - ls) : 1.0f; P.ls_shift = P.has_ls ? (float)(0.5 * ls) : 0.0f;
    std::vector<float> out(2 * n);
    for (size_t i = 0; i < n; ++i) {
        float d = 0.0f;
        out[i] = lf_element<true>(x[i], y[i], w[i], P, d);
        out[n + i] = d;
    }
    FILE* h = fopen(argv[10], "wb");
    if (!h || fwrite(out.data(), 4, 2 * n, h) != 2 * n) abort();
    fclose(h);
    return 0;
}
"""


def test_element_arithmetic_compiled_for_the_host(tmp_path):
    """The kernel's per-element function (``lf_element`` of csrc/p2w_loss.hip compiles for host and device) run on the CPU over
    every recorded case: every element within the GPU tests' bound, 8 x the reference's own float32 noise, the NaN row exactly 0 and
    the gradient beyond +-10 exactly 0.  The host's expf / log1pf / powf are not the device's: the GPU tests stay the check of those."""
    import shutil
    import subprocess
    from pointstowood_amd import build as B
    hipcc = B._hipcc()
    if shutil.which(hipcc) is None and not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = tmp_path / "host_main.cpp"
    src.write_text(HOST_MAIN)
    exe = tmp_path / "host_main"
    r = subprocess.run([hipcc, *B.FLAGS, "-I", B.CSRC, "-x", "hip", str(src), "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    inp = _inputs()
    n = len(inp["logits"])
    for k in ("logits", "labels", "labels_soft", "weight_n"):
        inp[k].tofile(tmp_path / f"{k}.bin")
    np.full(n, inp["weight_1"][0], dtype=np.float32).tofile(tmp_path / "weight_1.bin")
    noise = json.load(open(os.path.join(GOLDEN, "noise.json")))["cases"]
    beyond = ~((inp["logits"] >= -10) & (inp["logits"] <= 10))
    for config, kind in CASES:
        kwargs, wkind = R.CONFIGS[config]
        a = dict(R.DEFAULTS, **kwargs)
        arg = lambda v: "nan" if v is None else repr(float(v))          # noqa: E731
        out = tmp_path / "out.bin"
        r = subprocess.run([str(exe), str(n), str(tmp_path / "logits.bin"), str(tmp_path / ("labels.bin" if kind == "binary" else "labels_soft.bin")),
                            "-" if wkind is None else str(tmp_path / f"weight_{wkind}.bin"), arg(a["epsilon"]), arg(a["gamma"]), arg(a["alpha"]),
                            arg(a["label_smoothing"]), arg(a["eps"]), str(out)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (config, kind, r.stderr)
        got = np.fromfile(out, dtype=np.float32).astype(np.float64)
        g = np.load(os.path.join(GOLDEN, f"{config}__{kind}.npz"))
        nz = noise[f"{config}__{kind}"]
        el, eg = np.abs(got[:n] - g["loss64"]).max(), np.abs(got[n:] - g["grad64"]).max()
        assert el <= 8 * nz["loss"] and eg <= 8 * nz["grad"], (config, kind, el / nz["loss"], eg / nz["grad"])
        assert got[10] == 0 and got[n + 10] == 0 and (got[n:][beyond] == 0).all() and got[n] != 0 and got[n + 1] != 0


def test_poly1_focal_argument_errors():
    """p2w_poly1_focal refuses bad sizes and scalars, a missing, misaligned or short workspace and misaligned arrays before it
    launches anything; the workspace holds one float64 per chunk."""
    L = _lib.lib()
    assert L.p2w_version() == 610
    n = 100000
    need = int(L.p2w_poly1_focal_ws_bytes(n))
    chunks = -(-n // _lib.LOSS_CHUNK)
    assert 8 * chunks <= need < 8 * chunks + 256 and need % 256 == 0
    assert int(L.p2w_poly1_focal_ws_bytes(0)) > 0 and int(L.p2w_poly1_focal_ws_bytes(-1)) == 0
    assert int(L.p2w_poly1_focal_ws_bytes((1 << 40) + 1)) == 0 and int(L.p2w_poly1_focal_ws_bytes(1 << 40)) >= 8 << 28
    buf = ctypes.create_string_buffer(need + 16)
    ws = (ctypes.addressof(buf) + 15) & ~15
    fake = 16

    def call(logits=fake, labels=fake, weight=None, weight_n=0, n=n, epsilon=0.1, gamma=2.0, alpha=0.25, ls=NAN, eps=1e-6, loss=fake,
             dloss=fake, total=fake, ws=ws, ws_bytes=need):
        return L.p2w_poly1_focal(logits, labels, weight, weight_n, n, epsilon, gamma, alpha, ls, eps, loss, dloss, total, ws, ws_bytes, None)

    assert call(n=-1) == -1 and call(n=(1 << 40) + 1) == -1
    assert call(weight=fake, weight_n=2) == -1 and call(weight=fake, weight_n=0) == -1 and call(weight_n=1) == -1
    assert call(gamma=-0.5) == -1 and call(gamma=NAN) == -1 and call(gamma=float("inf")) == -1
    assert call(epsilon=NAN) == -1 and call(epsilon=float("-inf")) == -1
    assert call(alpha=float("inf")) == -1 and call(ls=float("inf")) == -1
    assert call(eps=0.0) == -1 and call(eps=0.5) == -1 and call(eps=NAN) == -1 and call(eps=-1e-6) == -1
    assert call(ws=None) == -2 and call(ws=ws + 4) == -3 and call(ws_bytes=need - 1) == -4
    assert call(logits=None) == -2 and call(labels=None) == -2
    assert call(logits=20) == -3 and call(labels=20) == -3 and call(loss=20) == -3 and call(dloss=20) == -3
    assert call(weight=20, weight_n=n) == -3


def test_module_refuses_host_tensors_and_bad_arguments():
    x, y = torch.zeros(8), torch.zeros(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PL.Poly1FocalLoss()(x, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PL.poly1_focal(x, y, reduction="mean")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PL.EpochScores().add(x, y)
    with pytest.raises(ValueError, match="elements"):
        PL.Poly1FocalLoss()(x, torch.zeros(7))
    with pytest.raises(ValueError, match="weight"):
        PL.Poly1FocalLoss(weight=torch.ones(3))(x, y)
    for bad in (dict(eps=0.0), dict(eps=0.5), dict(eps=-1.0), dict(eps=NAN), dict(gamma=-1.0), dict(gamma=NAN), dict(gamma=float("inf")),
                dict(epsilon=NAN), dict(epsilon=float("inf")), dict(alpha=NAN), dict(alpha=float("-inf"))):
        with pytest.raises(ValueError, match=next(iter(bad))):
            PL.Poly1FocalLoss(**bad)
        with pytest.raises(ValueError, match=next(iter(bad))):
            PL.poly1_focal(x, y, **bad)
    m = PL.Poly1FocalLoss()
    m.gamma = -2.0                       # the reference's attributes stay assignable: checked again at the call
    with pytest.raises(ValueError, match="gamma"):
        m(x, y)
    with pytest.raises(ValueError, match="logits only"):
        PL.Poly1FocalLoss()(x, y.clone().requires_grad_())
    with pytest.raises(ValueError, match="logits only"):
        PL.Poly1FocalLoss(weight=torch.ones(8, requires_grad=True))(x, y)


def test_module_keeps_the_references_constructor():
    sig = inspect.signature(PL.Poly1FocalLoss.__init__)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[1:]] == [
        ("epsilon", 0.1), ("gamma", 2.0), ("alpha", 0.25), ("reduction", "none"), ("weight", None), ("label_smoothing", None), ("eps", 1e-6)]
    assert list(inspect.signature(PL.Poly1FocalLoss.forward).parameters) == ["self", "logits", "labels", "label_weights"]
    m = PL.Poly1FocalLoss(alpha=None, label_smoothing=0.1, reduction="mean")
    assert isinstance(m, torch.nn.Module) and m.alpha is None and m.label_smoothing == 0.1 and m.reduction == "mean"


def test_epoch_scores_add_never_reads_the_device():
    """``add`` runs once per training step: no ``.cpu()`` / ``.item()`` / ``.tolist()`` / ``.numpy()`` / ``float(tensor)`` in it or in
    the slot bookkeeping it calls, and ``evaluate.confusion`` is called with ``strict=False`` (its only host read)."""
    for fn in (PL.EpochScores.add, PL.EpochScores._slot):
        src = inspect.getsource(fn)
        assert not re.search(r"\.(cpu|item|tolist|numpy)\(|\bfloat\(|\bint\(|\bbool\(|synchronize", src), fn
    assert "strict=False" in inspect.getsource(PL.EpochScores.add)
    assert inspect.getsource(PL.EpochScores.result).count(".cpu()") == 1


def test_loss_module_imports_no_oracle_and_no_sklearn():
    src = open(os.path.join(ROOT, "pointstowood_amd", "loss.py")).read()
    assert not re.search(r"^\s*(from|import)\s+(oracle|sklearn|tests)\b", src, re.M)
