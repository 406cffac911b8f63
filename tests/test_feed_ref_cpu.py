"""The training feed's references and host-side parts, without a GPU: tests/feed_ref.py against the fixtures recorded from the
reference (tests/golden/train_feed/, tests/golden/make_golden_train_feed.py), the generator against its published known answers, the
plan's decisions, the --tune schedule, the workspace arithmetic of p2w_train_feed and the command line."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pointstowood_amd import _lib
from tests import feed_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.load_cases()
NAMES = sorted(CASES)


def test_fixture_manifest_and_cases():
    man = json.load(open(os.path.join(R.GOLDEN, "manifest.json")))
    files = sorted(f for f in os.listdir(R.GOLDEN) if f != "manifest.json")
    assert sorted(man) == files and len(files) == len(CASES) + 3
    for f in files:
        assert hashlib.sha256(open(os.path.join(R.GOLDEN, f), "rb").read()).hexdigest() == man[f], f
        assert os.path.getsize(os.path.join(R.GOLDEN, f)) < 1 << 20
    # the three reflectance branches x rotated or not in train mode, the four that exist in test mode, +300 m and the origin
    seen = {(c["mode"], c["refl_mode"], c["rotate"]) for c in CASES.values()}
    assert {("train", r, rot) for r in (0, 1, 2) for rot in (False, True)} <= seen
    assert {("test", r, rot) for r in (0, 1) for rot in (False, True)} <= seen and not any(m == "test" and r == 2 for m, r, _ in seen)
    assert CASES["plot300"]["offset"][0] == 300.0 and CASES["plot300"]["rotate"] and max(c["n"] for c in CASES.values()) <= 2000


@pytest.mark.parametrize("name", NAMES)
def test_decisions_match_the_recorded_branches(name):
    c = CASES[name]
    assert R.decisions(c["u_refl"][0], c["u_pos"][0], c["mode"]) == (c["refl_mode"], c["rotate"])


@pytest.mark.parametrize("name", NAMES)
def test_float64_restatement_agrees_with_the_reference_within_its_own_noise(name):
    """pos within reference_pos_cap (derived in feed_ref from the reference's operation counts and the coordinates' magnitude: large at
    +300 m), sf within reference_sf_cap, the reflectance exact when kept or silenced and within half an ulp of the sum when perturbed,
    y exact."""
    c = CASES[name]
    pc = c["pc"]
    pos, refl, sf = R.item_f64(pc[:, :3], pc[:, 3], c["refl_mode"], c["rotate"], c["u_angles"], c["noise"])
    cap = R.reference_pos_cap(pc[:, :3], c["rotate"])
    err = np.abs(c["pos"].astype(np.float64) - pos).max()
    print(f"{name}: pos err {err:.3e} cap {cap:.3e}")
    assert err <= cap
    assert abs(float(c["sf"]) - sf) <= R.reference_sf_cap(cap, sf)
    if c["refl_mode"] == 2:
        assert (np.abs(c["reflectance"].astype(np.float64) - refl) <= 0.5 * np.spacing(np.abs(c["reflectance"]))).all()
        assert c["noise"].std() > 0.05
    else:
        assert np.array_equal(c["reflectance"].astype(np.float64), refl)
    assert np.array_equal(c["y"], pc[:, 4])


def test_the_reference_noise_is_large_at_plot_coordinates():
    """The point of centring first: at +300 m the reference's own float32 error is far above what float32 resolves near the origin."""
    errs = {}
    for name in ("plot300", "origin"):
        c = CASES[name]
        pos, _, _ = R.item_f64(c["pc"][:, :3], c["pc"][:, 3], c["refl_mode"], c["rotate"], c["u_angles"], c["noise"])
        errs[name] = np.abs(c["pos"].astype(np.float64) - pos).max()
    assert errs["plot300"] > 1e-5 > errs["origin"], errs


KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    got = R.philox4x32_10(np.array(counter, dtype=np.uint64), key)
    assert " ".join(f"{int(w):08x}" for w in got) == want


def test_philox_is_vectorised_consistently():
    ctr = np.array([k[0] for k in KAT], dtype=np.uint64)
    one = R.philox4x32_10(ctr, KAT[2][1])
    for i in range(3):
        assert np.array_equal(one[i], R.philox4x32_10(ctr[i], KAT[2][1]))
    w = R.feed_words(5, 3, 7, (9 << 32) | 11)
    ctr = np.array([2, 3, 7, R.STREAM], dtype=np.uint64)
    assert np.array_equal(w[2], R.philox4x32_10(ctr, [11, 9]))
    u1, u2 = R.uniforms(w)
    assert (u1 > 0).all() and (u1 <= 1).all() and (u2 >= 0).all() and (u2 < 1).all()
    assert (R.z_cap(w) < 2e-5).all()


def test_plan_from_draws_decisions_and_edges():
    from pointstowood_amd import feed as F
    edges = json.load(open(os.path.join(R.GOLDEN, "edges.json")))
    assert len(edges) == 16
    for mode in ("train", "test"):
        rows = [e for e in edges if e["mode"] == mode]
        plan = F.plan_from_draws([e["u_refl"] for e in rows], [e["u_pos"] for e in rows], np.full((len(rows), 3), 0.75), mode)
        assert plan.dtype == F.PLAN_DTYPE and plan.dtype.itemsize == 48
        for e, rec in zip(rows, plan):
            assert int(rec["refl_mode"]) == e["refl_mode"] and bool(rec["rotate"]) == e["rotate"], e
            assert R.decisions(e["u_refl"], e["u_pos"], mode) == (e["refl_mode"], e["rotate"]), e
    # exactly 0.25 is not silenced and not rotated; exactly 0.5 is not perturbed (the reference's <, >= and <)
    p = F.plan_from_draws([0.25, 0.5, 0.0, 0.4999], [0.25, 0.0, 0.9, 0.2], np.zeros((4, 3)), "train")
    assert p["refl_mode"].tolist() == [2, 0, 1, 2] and p["rotate"].tolist() == [0, 1, 0, 1]
    p = F.plan_from_draws([0.25, 0.5, 0.0, 0.4999], [0.25, 0.0, 0.9, 0.2], np.zeros((4, 3)), "test")
    assert p["refl_mode"].tolist() == [0, 0, 1, 0]
    with pytest.raises(ValueError):
        F.plan_from_draws([0.1], [0.1], np.zeros((1, 3)), "predict")
    ident = F.identity_plan(3)
    assert (ident["refl_mode"] == 0).all() and (ident["rotate"] == 0).all() and (ident["R"] == np.eye(3, dtype=np.float32).reshape(9)).all()


def test_plan_rotation_is_the_rounded_float64_product():
    from pointstowood_amd import feed as F
    g = torch.Generator().manual_seed(3)
    u = torch.rand(6, 3, generator=g)
    plan = F.plan_from_draws(torch.zeros(6), torch.tensor([0.0, 0.9, 0.1, 0.2, 0.3, 0.24]), u, "train")
    for i in range(6):
        roll, pitch, yaw = R.rotation_matrices(u[i].numpy())
        want = (roll @ pitch @ yaw).astype(np.float32) if plan["rotate"][i] else np.eye(3, dtype=np.float32)
        assert np.array_equal(plan["R"][i].reshape(3, 3), want), i
        if plan["rotate"][i]:
            assert np.abs(want.astype(np.float64) @ want.astype(np.float64).T - np.eye(3)).max() < 1e-6
    assert plan["rotate"].tolist() == [1, 0, 1, 1, 0, 1]


def test_draw_plan_is_a_function_of_the_generator():
    from pointstowood_amd import feed as F
    a = F.draw_plan(500, "train", torch.Generator().manual_seed(5))
    b = F.draw_plan(500, "train", torch.Generator().manual_seed(5))
    c = F.draw_plan(500, "test", torch.Generator().manual_seed(5))
    assert a.tobytes() == b.tobytes()
    assert set(a["refl_mode"].tolist()) == {0, 1, 2} and set(c["refl_mode"].tolist()) == {0, 1}
    assert np.array_equal(a["rotate"], c["rotate"]) and np.array_equal(a["refl_mode"] == 1, c["refl_mode"] == 1)
    g = torch.Generator().manual_seed(5)
    u_refl, u_pos, u_ang = torch.rand(500, generator=g), torch.rand(500, generator=g), torch.rand(500, 3, generator=g)
    assert F.plan_from_draws(u_refl, u_pos, u_ang, "train").tobytes() == a.tobytes()


def test_tune_schedule_against_the_recorded_sequence():
    from pointstowood_amd.trainer import CosineAnnealingWarmupRestarts
    rec = json.load(open(os.path.join(R.GOLDEN, "tune_lr.json")))
    assert len(rec["lr"]) >= 3 * rec["kwargs"]["first_cycle_steps"] + 1
    opt = torch.optim.AdamW(torch.nn.Linear(2, 1).parameters(), lr=1e-6, weight_decay=1e-2)
    sched = CosineAnnealingWarmupRestarts(opt, **rec["kwargs"])
    got = [opt.param_groups[0]["lr"]]
    for _ in range(len(rec["lr"]) - 1):
        sched.step()
        got.append(opt.param_groups[0]["lr"])
    # the same float64 expression evaluated once: a few ulps at most
    assert np.allclose(got, rec["lr"], rtol=1e-13, atol=0), np.abs(np.array(got) - np.array(rec["lr"])).max()
    assert got[0] == 1e-8 and got[10] == 1e-8 and max(got) == pytest.approx(1e-6, rel=1e-12) and max(got[10:20]) == pytest.approx(5e-7, rel=1e-12)
    with pytest.raises(ValueError):
        CosineAnnealingWarmupRestarts(opt, first_cycle_steps=5, warmup_steps=5)


def test_feed_constants_mirror_the_header():
    hdr = open(os.path.join(ROOT, "include", "p2w.h")).read()
    assert int(re.search(r"#define P2W_FEED_CHUNK (\d+)", hdr).group(1)) == _lib.FEED_CHUNK == R.CHUNK
    assert int(re.search(r"#define P2W_FEED_STREAM (0x[0-9a-fA-F]+)u", hdr).group(1), 16) == _lib.FEED_STREAM == R.STREAM
    from pointstowood_amd import feed as F
    body = re.search(r"typedef struct p2w_feed_plan \{(.*?)\} p2w_feed_plan;", hdr, flags=re.S).group(1)
    fields = re.findall(r"(int32_t|float) ([a-zA-Z_]+)(\[9\])?;", body)
    assert [f[1] for f in fields] == list(F.PLAN_DTYPE.names)


def test_ws_size_host_arithmetic_and_refusals():
    """n / P2W_FEED_CHUNK + B chunks of four float64, rounded up to the arena's 256 bytes; 0 for the sizes the call refuses."""
    L = _lib.lib()
    for n, B in [(0, 0), (0, 1), (1, 1), (255, 1), (256, 1), (257, 3), (4097, 5), (131072, 8), (1 << 40, 1)]:
        chunks = n // 256 + B
        assert L.p2w_train_feed_ws_size(n, B) == (chunks * 32 + 255) // 256 * 256, (n, B)
    for n, B in [(-1, 1), (10, -1), ((1 << 40) + 1, 1)]:
        assert L.p2w_train_feed_ws_size(n, B) == 0, (n, B)


def test_argument_refusals_come_back_before_any_launch():
    """Fake addresses that are never dereferenced: every status below is returned before a launch (no GPU is needed)."""
    L = _lib.lib()
    A, U = 4096, 4100

    def call(B=2, n=10, V=3, n_set=20, xyzr=A, plan=A, ws=A, ws_size=1 << 20, pos=A, noise=None, ids=A):
        return L.p2w_train_feed(xyzr, A, A, n_set, V, ids, A, B, n, plan, 1, 0, noise, pos, A, A, A, A, A, None, ws, ws_size, None)
    assert call(B=-1) == -1 and call(n=-1) == -1 and call(V=0) == -1 and call(n_set=-1) == -1 and call(n=(1 << 40) + 1) == -1
    assert call(B=0) == 0 and call(n=0) == 0                     # nothing to do: OK, nothing written
    assert call(xyzr=None) == -2 and call(pos=None) == -2 and call(ids=None) == -2 and call(ws=None) == -2
    assert call(xyzr=U) == -3 and call(plan=U) == -3 and call(ws=U) == -3
    assert call(ws_size=L.p2w_train_feed_ws_size(10, 2) - 1) == -4
    assert call(B=0x7fffffff, n=1 << 40, ws_size=1 << 62) == -1   # more chunks than a grid holds


REFERENCE_FLAGS = ["--device", "--num_procs", "--num_epochs", "--checkpoint_saves", "--model", "--resolution", "--grid_size", "--min_pts",
                   "--max_pts", "--batch_size", "--augmentation", "--preprocess", "--test", "--tune", "--stop_early", "--wandb",
                   "--verbose"]


def test_train_command_line_parses():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for flag in REFERENCE_FLAGS + ["--wdir", "--seed"]:
        assert flag in r.stdout, flag
    sys.path.insert(0, ROOT)
    import train as cli
    a = cli.build_parser().parse_args([])
    assert (a.num_epochs, a.batch_size, a.min_pts, a.max_pts, a.model, a.grid_size, a.checkpoint_saves) == \
        (2, 2, 8192, 16384, "model.pth", [2.0, 4.0], 1)
    assert not (a.augmentation or a.preprocess or a.test or a.tune or a.stop_early or a.wandb or a.verbose) and a.seed == 141190
