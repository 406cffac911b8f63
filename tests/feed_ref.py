"""Reference for the training feed (p2w_train_feed, include/p2w.h; pointstowood_amd.feed), written from the reference's formulas
(pointstowood/src/augmentation.py:5-12,41-55, pointstowood/src/trainer.py:46-60) and from the generator's publication, and from nothing
of the package under test: a float64 restatement, a pure-numpy Philox4x32-10 with the header's Box-Muller, and the error caps the tests
hold the kernel and the fixtures to, each derived here from operation counts and magnitudes.

u = 2^-24 is the unit roundoff of float32 (round to nearest), u64 = 2^-53 that of float64.
"""
from __future__ import annotations

import json
import os

import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53
CHUNK = 256
STREAM = 0x50325746
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_feed")


# ---- the reference's formulas in float64 -------------------------------------------------------------------------------------------

def angles_cos_sin(u_angles):
    """float32 cos / sin of ``deg2rad(u * 180 - 90)`` as the reference computes them (torch, float32), returned as float64."""
    import torch
    rot = torch.deg2rad(torch.as_tensor(np.asarray(u_angles, dtype=np.float32)).reshape(3) * 180 - 90)
    return torch.cos(rot).double().numpy(), torch.sin(rot).double().numpy()


def rotation_matrices(u_angles):
    """(roll, pitch, yaw) of rotate_3d in float64, entries the float32 cos / sin values."""
    c, s = angles_cos_sin(u_angles)
    roll = np.array([[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]], dtype=np.float64)
    pitch = np.array([[c[1], 0, s[1]], [0, 1, 0], [-s[1], 0, c[1]]], dtype=np.float64)
    yaw = np.array([[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1]], dtype=np.float64)
    return roll, pitch, yaw


def decisions(u_refl, u_pos, mode):
    """(refl_mode, rotate) of augmentations() for float32 draws: 0 keep, 1 silence, 2 perturb."""
    u_refl, u_pos = np.float32(u_refl), np.float32(u_pos)
    refl_mode = 1 if u_refl < np.float32(0.25) else 0
    if mode == "train" and u_refl >= np.float32(0.25) and u_refl < np.float32(0.5):
        refl_mode = 2
    return refl_mode, bool(u_pos < np.float32(0.25))


def item_f64(pos, refl, refl_mode, rotate, u_angles=None, noise=None):
    """The reference's item in float64, in ITS order of operations: augment (rotate the raw coordinates through roll, pitch and yaw),
    centre, sf.  pos [n, 3] and refl [n] float32 (exact in float64); noise [n] float32 for refl_mode 2.  Returns pos, refl, sf."""
    p = np.asarray(pos, dtype=np.float64)
    r = np.asarray(refl, dtype=np.float64)
    if refl_mode == 1:
        r = np.zeros_like(r)
    elif refl_mode == 2:
        r = r + np.asarray(noise, dtype=np.float64)
    if rotate:
        roll, pitch, yaw = rotation_matrices(u_angles)
        p = p @ roll @ pitch @ yaw
    p = p - p.mean(axis=0)
    sf = np.sqrt((p ** 2).sum(axis=1)).max() if len(p) else 0.0
    return p, r, sf


def sf_f32(pos32):
    """The header's sf from the WRITTEN float32 positions: max of sqrtf((px px + py py) + pz pz), every operation rounded to float32
    (numpy's float32 arithmetic and sqrt are correctly rounded); NaN if any norm is NaN (torch.max); 0 for no row."""
    p = np.asarray(pos32, dtype=np.float32)
    if len(p) == 0:
        return np.float32(0)
    nrm = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
    return np.float32(np.nan) if np.isnan(nrm).any() else nrm.max()


# ---- caps --------------------------------------------------------------------------------------------------------------------------

def kernel_pos_cap(pos_raw, rotate, R64=None):
    """Per-element cap [n, 3] of |kernel pos - float64 pos| for one voxel.

    mean: the float64 sum of n values of magnitude <= M in any order errs by at most (n - 1) u64 sum|x|, the division adds u64 |mean|:
    at most (n + 1) u64 M per coordinate, for the kernel and for the float64 restatement alike -> 2 (n + 1) u64 M.
    d = fl32(x - mean): ONE rounding, u |d|.
    not rotated: p = d.  rotated: p_j = sum_i d_i R_ij with R rounded to float32 (u |R_ij| each), a product and two fmaf (three
    roundings, each at most u times a partial sum that is at most S_j = sum_i |d_i| |R_ij|): (1 + 1 + 3) u S_j, and second-order terms
    covered by the factor (1 + 2^-20).  The mean's error passes through R with sum_i |R_ij| <= sqrt(3)."""
    x = np.asarray(pos_raw, dtype=np.float64)
    n = len(x)
    M = np.abs(x).max() if n else 0.0
    mean_err = 2 * (n + 1) * U64 * M
    d = np.abs(x - x.mean(axis=0))
    if not rotate:
        return U32 * d * (1 + 2.0 ** -20) + mean_err
    S = d @ np.abs(np.asarray(R64, dtype=np.float64))
    return 5 * U32 * S * (1 + 2.0 ** -20) + np.sqrt(3.0) * mean_err


def reference_pos_cap(pos_raw, rotate):
    """Scalar cap of |reference float32 pos - float64 restatement| per element of one voxel: the reference's OWN float32 noise.

    With m = max_i ||x_i|| over the raw rows (rotations preserve it):
    rotate_3d: three float32 3 x 3 products in turn.  An entry of one product is a 3-term dot product, error <= 3 u sum_i |x_i| |R_ij|
    <= 3 u m (Cauchy-Schwarz, unit columns), so the row's error vector has norm <= 3 sqrt(3) u m, and the later rotations carry it on
    unchanged in norm: <= 9 sqrt(3) u m after three.  (The matrices' entries are the same float32 cos / sin values in the restatement.)
    torch.mean in float32: at most n u m per coordinate in the worst order.  The subtraction: one rounding, <= u * 2 m.
    Total (16 + 2 + n) u m when rotated, (2 + n) u m otherwise; second-order terms in the factor 1.01."""
    x = np.asarray(pos_raw, dtype=np.float64)
    n = len(x)
    m = np.sqrt((x ** 2).sum(axis=1)).max() if n else 0.0
    ops = (16 if rotate else 0) + 2 + n
    return 1.01 * ops * U32 * m


def reference_sf_cap(pos_cap, sf):
    """The norm is 1-Lipschitz in the row: sqrt(3) pos_cap; two products, two sums and a square root in float32: <= 3 u sf."""
    return np.sqrt(3.0) * pos_cap + 3 * U32 * abs(sf) * 1.01


# ---- Philox4x32-10 and the header's Box-Muller -------------------------------------------------------------------------------------

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """counter [..., 4] and key [2] (or [..., 2]) of 32-bit words -> [..., 4] uint32.  Salmon et al., SC'11: per round
    (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)); the key grows by (W0, W1) between rounds."""
    c = np.asarray(counter, dtype=np.uint64) & np.uint64(0xffffffff)
    k = np.broadcast_to(np.asarray(key, dtype=np.uint64) & np.uint64(0xffffffff), c.shape[:-1] + (2,))
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    mask, sh = np.uint64(0xffffffff), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & mask, (p0 >> sh) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(W0)) & mask, (k1 + np.uint64(W1)) & mask
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def feed_words(n, voxel, epoch, seed):
    """The words of rows 0 .. n - 1 of voxel ``voxel``: counter (i, voxel, epoch, STREAM), key (seed low, seed high)."""
    ctr = np.zeros((n, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = np.arange(n), voxel, epoch, STREAM
    return philox4x32_10(ctr, [seed & 0xffffffff, (seed >> 32) & 0xffffffff])


def uniforms(words):
    w = np.asarray(words, dtype=np.uint32)
    u1 = ((w[..., 0] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24      # (0, 1], exact in float32
    u2 = (w[..., 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24              # [0, 1)
    return u1, u2


def box_muller_f64(words):
    """z = sqrt(-2 ln u1) cos(2 pi u2) in float64 of the header's u1, u2."""
    u1, u2 = uniforms(words)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


# OpenCL full-profile accuracy of the single-precision functions the device math library (OCML) implements: log <= 3 ulp, cos <= 4 ulp;
# sqrtf is correctly rounded in the default hipcc build (-fhip-fp32-correctly-rounded-divide-sqrt).
ULP_LOG, ULP_COS = 3, 4
TWO_PI_F = float(np.float32(6.2831855))


def z_cap(words):
    """Per-element cap of |device z - box_muller_f64|, with e = 2^-23 (one ulp relative to a value's own magnitude, at most):
    L = logf(u1): relative error <= ULP_LOG e.  t = -2 L: exact.  r = sqrtf(t): half the relative error of t, plus one rounding u.
    a = fl32(6.2831855f u2): |da| <= u a + u2 |6.2831855f - 2 pi|.  c = cosf(a): |dc| <= |da| (cos is 1-Lipschitz) + ULP_COS e (|c| <= 1).
    z = fl32(r c): |dz| <= r |dc| + |c| dr + u |z|.  Second-order terms: the factor 1.001."""
    u1, u2 = uniforms(words)
    e = 2.0 ** -23
    r = np.sqrt(-2.0 * np.log(u1))
    a = 2.0 * np.pi * u2
    c = np.cos(a)
    dr = r * (ULP_LOG * e / 2 + U32)
    da = U32 * a + u2 * abs(TWO_PI_F - 2.0 * np.pi)
    dc = da + ULP_COS * e
    return 1.001 * (r * dc + np.abs(c) * dr + U32 * np.abs(r * c))


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------

def load_cases():
    """name -> dict of arrays / scalars of every recorded case (tests/golden/train_feed/<name>.npz) with its json attributes."""
    meta = json.load(open(os.path.join(GOLDEN, "cases.json")))
    out = {}
    for name, attrs in meta["cases"].items():
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        out[name] = dict(attrs, **{k: z[k] for k in z.files})
    return out
