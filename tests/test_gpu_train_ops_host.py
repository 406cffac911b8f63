"""The host layer of the training operators against its recording (tests/train_ops_record.py, tests/golden/train_ops_host.json): every
case of the helper runs on the tree under test and must give the record of the commit the fixture names - the same bits of every
output, gradient and running statistic, the same counters, the same ``grad_fn`` class, the same tensors saved for the backward in the
same order and dtypes, the same exception and message where the operator refuses.  Equality only: nothing here has a tolerance."""
import json

import pytest

from tests import train_ops_record as R

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(R.GOLDEN))
CASES = R.cases()
HALF = ("float16", "bfloat16")


@pytest.fixture(scope="module")
def H():
    from pointstowood_amd import ops
    return ops


def test_fixture_names_its_commit_and_holds_every_case():
    assert len(GOLDEN["recorded_from"]) == 40 and set(GOLDEN["cases"]) == set(CASES)
    assert len(GOLDEN["refusals"]) >= 60 and len(GOLDEN["evals"]) >= 6


@pytest.mark.parametrize("name", list(CASES))
def test_case_equals_its_record(H, name):
    before = H.half_io
    got, want = CASES[name](H), GOLDEN["cases"][name]
    assert H.half_io is before
    assert got == want, f"{name}\n now      {got}\n recorded {want}"


def test_refusals_equal_their_records_and_move_nothing(H):
    got, want = R.GROUPS["refusals"](H), GOLDEN["refusals"]
    assert set(got) == set(want)
    for name in want:
        assert got[name] == want[name], f"{name}\n now      {got[name]}\n recorded {want[name]}"
        assert "raises" in got[name] and got[name]["state_unchanged"] is True, (name, got[name])


def test_eval_mode_moves_no_counter_and_no_statistic(H):
    got, want = R.GROUPS["evals"](H), GOLDEN["evals"]
    assert got == want
    for name, rec in got.items():
        assert rec.get("state_unchanged") is True and "raises" not in rec, (name, rec)


# ------------------------------------------------------------------------------------------------ what the recording itself must say
def _of(op, *parts):
    return {n: r for n, r in GOLDEN["cases"].items() if n.startswith(op + "-") and all(f"-{p}" in n for p in parts)}


def test_recorded_routes_save_what_half_io_promises():
    """The fixture is a recording, not a tautology: on a 16-bit route with ``half_io`` on no fp32 tensor with the rows dimension is saved
    by the operators that take z as it is, with it off the fp32 copy is, and the route shows in ``grad_fn``."""
    for op, cls in (("global_max_pool", "_SegmentMax"), ("relu_bn_max", "_ReluBnMax"), ("bn_relu_rowdot", "_BnReluRowdot")):
        for n, r in _of(op, "grad").items():
            on, half = "-on-" in n, "f16-" in n
            assert r["grad_fn"] == cls + ("HalfBackward" if on else "Backward"), n
            rows = [s for s in r["saved"] if s.startswith(f"{R.ROWS}x")]
            if op != "global_max_pool":
                assert len(rows) == 1 and rows[0].endswith(("float16" if "bf16" not in n else "bfloat16") if on else "float32"), (n, rows)
            else:
                assert rows == [], (n, rows)
            assert half or not on
    for op, cls in (("bn_chain", "_BnChain"), ("relu_bn", "_ReluBn")):
        for n, r in _of(op, "grad").items():
            on = "-on-" in n
            rows = [s for s in r["saved"] if s.startswith(f"{R.ROWS}x")]
            assert len(rows) == (2 if "-res-" in n else 1), (n, rows)
            assert rows[0].endswith(HALF if on else "float32"), (n, rows)
            assert all(s.endswith("float32") for s in rows[1:]), (n, rows)
            if on:
                assert r["grad_fn"] == cls + "HalfBackward", n
            elif "out_own" in n:
                assert r["grad_fn"] == "ToCopyBackward0", n              # the caller's .to(out_dtype) behind the fp32 route
            else:
                assert r["grad_fn"] == cls + "Backward", n
    for n, r in _of("edge_layer1", "grad").items():
        E = [s for s in r["saved"] if s.startswith("301")]
        if "out_none" in n:
            assert r["grad_fn"] == "_EdgeLayer1Backward" and E == ["301x8:float32", "301x4:float32", "301:int32"], (n, E)
        else:
            assert r["grad_fn"] == "_EdgeLayer1HalfBackward" and E == ["301x4:float32", "301:int32"], (n, E)
    for n, r in GOLDEN["cases"].items():
        if n.endswith("no_grad"):
            assert r["saved"] == [] and r["grad_fn"] is None and "grads" not in r, n
        if not n.startswith(("global_max_pool", "edge_layer1", "interp_add_relu")):
            assert r["nbt"] and all(v == 1 for v in r["nbt"]), n


def test_recorded_routes_agree_bit_for_bit():
    """``half_io`` on and off are the same bits: the two records of a 16-bit case differ in ``grad_fn`` and in what is saved, not in a hash."""
    pairs = 0
    for n, on in GOLDEN["cases"].items():
        if "-on-" not in n:
            continue
        off = GOLDEN["cases"][n.replace("-on-", "-off-")]
        for k in ("out", "grads", "stats", "nbt"):
            assert on.get(k) == off.get(k), (n, k)
        pairs += 1
    assert pairs > 100
