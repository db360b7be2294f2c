"""The memory-bound entry points of the library give, bit for bit, what the commit before the
split of csrc/pointwise.hip gave: losses, gradient norm and clip, Adam / AdamW / Adadelta with
and without the EMA, the stand-alone EMA update, the SSIM forward, the image metrics and the
PReLU backward (cases and inputs: tests/_pointwise_bits.py; recorded by
tests/golden/make_pointwise_golden.py into tests/golden/pointwise_bits.json).

These kernels reduce in a fixed order and use no atomics, so the same call gives the same
bits on every run: the comparison is exact equality."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _pointwise_bits as PB  # noqa: E402

with open(os.path.join(HERE, "golden", "pointwise_bits.json")) as f:
    GOLDEN = json.load(f)


def test_golden_has_exactly_the_groups():
    assert sorted(GOLDEN) == sorted(PB.GROUPS)


@pytest.mark.parametrize("group", sorted(PB.GROUPS))
def test_bits_equal_the_recorded_ones(group):
    got = json.loads(json.dumps(PB.GROUPS[group]()))
    want = GOLDEN[group]
    assert sorted(got) == sorted(want)
    wrong = [k for k in sorted(want) if got[k] != want[k]]
    for k in wrong:
        print(f"{k}: got {got[k]} recorded {want[k]}")
    assert not wrong
