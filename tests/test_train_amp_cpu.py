"""What the bfloat16 training mode has outside the GPU: train.py's flag and the dtype code of the C ABI."""
import pytest


def test_the_command_line_has_the_flag():
    """train.py --amp {fp16,bf16}, default fp16."""
    import train
    p = train.build_parser()
    assert p.parse_args([]).amp == "fp16" and p.parse_args(["--amp", "bf16"]).amp == "bf16" and p.parse_args(["--amp", "fp16"]).amp == "fp16"
    with pytest.raises(SystemExit):
        p.parse_args(["--amp", "fp32"])


def test_the_binding_and_the_header_agree_on_the_code():
    import os
    import re
    from pointstowood_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "p2w.h")).read()
    codes = {name: int(v) for name, v in re.findall(r"^#define P2W_(F32|F16|BF16) (\d+)$", header, re.M)}
    assert codes == {"F32": _lib.F32, "F16": _lib.F16, "BF16": _lib.BF16} and _lib.BF16 == 2
