"""What stopping and resuming a training run has outside the GPU: the state of the warm-restart schedule, the fingerprint comparison,
the signal handlers of the stop request and train.py's three flags."""
import signal

import pytest
import torch


def _schedule(lr=1e-6):
    from pointstowood_amd import trainer as TR
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    return opt, TR.CosineAnnealingWarmupRestarts(opt, first_cycle_steps=7, cycle_mult=1.5, max_lr=1e-3, min_lr=1e-5, warmup_steps=3,
                                                 gamma=0.5)


def test_the_warm_restart_schedule_round_trips_at_every_step_of_three_cycles():
    """Cycles of 7, 9 and 12 steps (cycle_mult 1.5 over the 4, 6, 9 steps behind the warm-up): a schedule restored at step k into a
    fresh object, its optimiser's group restored before it, gives the same rates as the one that ran on - to the end of cycle three."""
    total = 7 + 9 + 12
    opt, ref = _schedule()
    rates, states = [], []
    for _ in range(total + 1):
        states.append((ref.state_dict(), opt.state_dict()))
        ref.step()
        rates.append(opt.param_groups[0]["lr"])
    assert ref.cycle == 3 and set(states[0][0]) == {"cycle", "cycle_steps", "t"}
    assert [s[0]["cycle"] for s in states].count(0) == 7 and [s[0]["cycle"] for s in states].count(1) == 9
    for k, (sched_state, opt_state) in enumerate(states):
        opt2, got = _schedule(lr=0.5)
        opt2.load_state_dict(opt_state)
        got.load_state_dict(sched_state)
        assert got.state_dict() == sched_state and opt2.param_groups[0]["lr"] == opt_state["param_groups"][0]["lr"]
        after = []
        for _ in range(k, total + 1):
            got.step()
            after.append(opt2.param_groups[0]["lr"])
        assert after == rates[k:], k


def test_fingerprint_mismatch():
    from pointstowood_amd.trainer import fingerprint_mismatch
    a = {"seed": 5, "batch_size": 2, "amp": "fp16", "fused_step": False, "train_voxels": 8, "train_lengths_sha256": "ab" * 32}
    assert fingerprint_mismatch(a, dict(a)) == []
    assert fingerprint_mismatch(a, {**a, "seed": 6}) == [("seed", 5, 6)]
    several = fingerprint_mismatch(a, {**a, "amp": "bf16", "fused_step": True, "train_voxels": 7})
    assert several == [("amp", "fp16", "bf16"), ("fused_step", False, True), ("train_voxels", 8, 7)]
    missing = dict(a)
    del missing["batch_size"]
    assert fingerprint_mismatch(a, missing) == [("batch_size", 2, "<absent>")]
    assert fingerprint_mismatch(missing, a) == [("batch_size", "<absent>", 2)]
    assert fingerprint_mismatch(a, {**a, "fused_step": 0}) == [("fused_step", False, 0)]           # a flag is not a number


def test_stop_handlers_set_the_request_and_put_the_previous_handlers_back():
    from pointstowood_amd import trainer as TR
    seen = []

    def mine(signum, frame):
        seen.append(signum)
    before = {s: signal.signal(s, mine) for s in (signal.SIGTERM, signal.SIGINT)}
    try:
        TR.clear_stop()
        assert not TR.stop_requested()
        with TR.stop_handlers():
            assert signal.getsignal(signal.SIGTERM) is not mine and signal.getsignal(signal.SIGINT) is not mine
            signal.raise_signal(signal.SIGTERM)
            assert TR.stop_requested() and seen == []
            TR.clear_stop()
            assert not TR.stop_requested()
            signal.raise_signal(signal.SIGINT)
            assert TR.stop_requested() and seen == []
        assert signal.getsignal(signal.SIGTERM) is mine and signal.getsignal(signal.SIGINT) is mine
        TR.clear_stop()
        signal.raise_signal(signal.SIGTERM)                     # outside the context: the handler from before, no request
        assert seen == [signal.SIGTERM] and not TR.stop_requested()
        with pytest.raises(RuntimeError):                       # the handlers come back on an error too
            with TR.stop_handlers():
                raise RuntimeError("inside")
        assert signal.getsignal(signal.SIGTERM) is mine
        TR.request_stop()
        assert TR.stop_requested()
    finally:
        TR.clear_stop()
        for s, h in before.items():
            signal.signal(s, h)


def test_the_command_line_has_the_three_flags(capsys):
    import train
    p = train.build_parser()
    d = p.parse_args([])
    assert d.state_every is None and d.stop_at is None and not d.resume and d.resume is None
    a = p.parse_args(["--stop_at", "2:3", "--state_every", "5", "--resume"])
    assert a.stop_at == (2, 3) and a.state_every == 5 and a.resume is True
    assert p.parse_args(["--stop_at", "1:0"]).stop_at == (1, 0) and p.parse_args(["--state_every", "0"]).state_every == 0
    for bad in ("2", "2:", ":3", "2:3:4", "a:b", "2.5:1", "0:1", "2:-1", "2-3"):
        with pytest.raises(SystemExit):
            p.parse_args(["--stop_at", bad])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        train.parse_args(["--resume", "--preprocess"])
    assert "--resume" in capsys.readouterr().err
    assert train.parse_args(["--resume"]).resume is True and train.parse_args(["--preprocess"]).preprocess is True
