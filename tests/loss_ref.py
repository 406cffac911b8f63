"""Reference for the Poly-1 focal loss (p2w_poly1_focal, include/p2w.h; pointstowood_amd.loss): the composite of the reference's
``pointstowood/src/loss.py:28-73`` restated, once in float64 numpy with the closed-form derivative and no autograd (``reference``) and
once in plain torch operations in the inputs' dtype (``composite``: what autograd differentiates, and what the reference's class
executes on a GPU).  ``make_inputs`` is the recipe of the committed fixture (tests/golden/make_golden_loss.py) extended by seed.  No
GPU and no reference checkout are needed: tests/test_loss_cpu.py holds this module against the values recorded from the reference.
"""
import numpy as np
import torch

EDGE_LOGITS = [10.0, -10.0, 10.000001, -10.000001, 12.0, -12.0, 0.0, -0.0, 1e-9, -1e-9, float("nan"), float("inf"), float("-inf"),
               9.999999, -9.999999, 88.0, -104.0]
FIXTURE_SEED, FIXTURE_DRAWS = 20261018, 4099

# name -> (constructor arguments, weight: None / "n" / "1"); every one is recorded with the binary and with the soft labels
CONFIGS = {
    "trainer": (dict(reduction="mean", gamma=2.0, alpha=None, label_smoothing=0.1), None),
    "defaults": (dict(reduction="none"), None),
    "sum_g15": (dict(reduction="sum", gamma=1.5, alpha=0.4, epsilon=1.0, eps=1e-3), None),
    "gamma0": (dict(reduction="none", gamma=0.0), None),
    "g05_weight_n": (dict(reduction="mean", gamma=0.5, eps=1e-4), "n"),
    "g05_weight_1": (dict(reduction="sum", gamma=0.5, eps=1e-4), "1"),
}
LABEL_KINDS = ("binary", "soft")
DEFAULTS = dict(epsilon=0.1, gamma=2.0, alpha=0.25, reduction="none", label_smoothing=None, eps=1e-6)


def make_inputs(n=len(EDGE_LOGITS) + FIXTURE_DRAWS, seed=FIXTURE_SEED):
    """logits [n] float32 = the 17 edge logits (as many as fit) followed by draws of randn * 4; labels [n] Bernoulli(0.3); labels_soft
    [n] uniform in [0, 1]; weight_n [n] uniform in [0.25, 2.25]; weight_1 [1]."""
    g = np.random.default_rng(seed)
    edge = np.asarray(EDGE_LOGITS[:n], dtype=np.float32)
    logits = np.concatenate([edge, (g.standard_normal(n - len(edge)) * 4).astype(np.float32)])
    return {
        "logits": logits,
        "labels": (g.random(n) < 0.3).astype(np.float32),
        "labels_soft": g.random(n).astype(np.float32),
        "weight_n": (0.25 + 2 * g.random(n)).astype(np.float32),
        "weight_1": np.asarray([1.75], dtype=np.float32),
    }


def case_tensors(inputs, config, labels_kind):
    """(logits, labels, weight or None, constructor arguments) of one recorded case, numpy float32."""
    kwargs, wkind = CONFIGS[config]
    w = None if wkind is None else inputs["weight_" + wkind]
    return inputs["logits"], inputs["labels" if labels_kind == "binary" else "labels_soft"], w, dict(DEFAULTS, **kwargs)


def _pow(x, e):
    return np.ones_like(x) if e == 0 else np.power(x, e)


def reference(logits, labels, weight=None, epsilon=0.1, gamma=2.0, alpha=0.25, reduction="none", label_smoothing=None, eps=1e-6):
    """(loss [n], dloss [n]) in float64: the per-element loss and its derivative with respect to the logit under PyTorch's autograd
    conventions (a clamp passes the gradient inside its closed range and gives 0 outside - so for a NaN -, the BCE term's derivative
    is (sigmoid(z) - y) * weight, a zero exponent contributes nothing).  ``reduction`` is ignored: reduce the result."""
    with np.errstate(all="ignore"):
        x = np.asarray(logits, dtype=np.float64).reshape(-1)
        y = np.asarray(labels, dtype=np.float64).reshape(-1)
        w = 1.0 if weight is None else np.asarray(weight, dtype=np.float64).reshape(-1)
        lo, hi = eps, 1 - eps
        z_in = (x >= -10) & (x <= 10)
        z = np.clip(x, -10, 10)                                    # (np.clip keeps a NaN, as torch.clamp does)
        if label_smoothing is not None:
            y = y * (1 - label_smoothing) + 0.5 * label_smoothing
        s = 1 / (1 + np.exp(-z))
        p_in = (s >= lo) & (s <= hi)
        p = np.clip(s, lo, hi)
        ce = ((1 - y) * z - (np.minimum(z, 0) - np.log1p(np.exp(-np.abs(z))))) * w      # = max(z, 0) - z y + log1p(exp(-|z|)), in ATen's order
        ce_in = ce <= 100
        ce_c = np.where(ce > 100, 100.0, ce)
        pt = y * p + (1 - y) * (1 - p)
        pt_in = (pt >= lo) & (pt <= hi)
        q = 1 - np.clip(pt, lo, hi)
        fw = _pow(q, gamma)
        fw_in = fw <= 2
        fw_c = np.where(fw > 2, 2.0, fw)
        at = np.ones_like(y) if alpha is None else alpha * y + (1 - alpha) * (1 - y)
        poly = epsilon * _pow(q, gamma + 1)
        poly_in = poly <= 100
        l = at * (fw_c * ce_c) + np.where(poly > 100, 100.0, poly)
        l_in = (l >= 0) & (l <= 100)
        loss = np.where(np.isnan(l), 0.0, np.clip(l, 0, 100))

        g_fl = np.where(l_in, at, 0.0)
        g_fw = np.where(fw_in, g_fl * ce_c, 0.0)
        g_ce = np.where(ce_in, g_fl * fw_c, 0.0)
        g_poly = np.where(l_in & poly_in, epsilon, 0.0)
        g_q = np.zeros_like(x)
        if gamma != 0:
            g_q = g_q + g_fw * (gamma * _pow(q, gamma - 1))
        g_q = g_q + g_poly * ((gamma + 1) * _pow(q, gamma))
        g_pt = np.where(pt_in, -g_q, 0.0)
        g_p = np.where(p_in, g_pt * y - g_pt * (1 - y), 0.0)
        g_z = g_p * ((1 - s) * s) + g_ce * ((s - y) * w)
        return loss, np.where(z_in, g_z, 0.0)


def composite(logits, labels, weight=None, epsilon=0.1, gamma=2.0, alpha=0.25, reduction="none", label_smoothing=None, eps=1e-6):
    """The same composite in plain torch operations, in the dtype and on the device of ``logits``, differentiable by autograd."""
    F = torch.nn.functional
    z = torch.clamp(logits, min=-10, max=10)
    y = labels
    if label_smoothing is not None:
        y = y * (1 - label_smoothing) + 0.5 * label_smoothing
    p = torch.clamp(torch.sigmoid(z), min=eps, max=1 - eps)
    ce = torch.clamp(F.binary_cross_entropy_with_logits(z, y, weight=weight, reduction="none"), max=100.0)
    pt = torch.clamp(y * p + (1 - y) * (1 - p), min=eps, max=1 - eps)
    focal = torch.clamp(torch.pow(1 - pt, gamma), max=2.0) * ce
    if alpha is not None:
        focal = (alpha * y + (1 - alpha) * (1 - y)) * focal
    loss = focal + torch.clamp(epsilon * torch.pow(1 - pt, gamma + 1), max=100.0)
    loss = torch.clamp(loss, min=0.0, max=100.0)
    loss = torch.where(torch.isnan(loss), torch.zeros_like(loss), loss)
    if reduction == "mean":
        return loss.mean()
    if reduction == "sum":
        return loss.sum()
    return loss
