#!/usr/bin/env python3
"""Record tests/golden/pointwise_bits.json: the bits the loss, clip, optimizer, EMA, SSIM,
metrics and PReLU-backward entry points give on the inputs of tests/_pointwise_bits.py.

    python tests/golden/make_pointwise_golden.py [OUT.json]

Run on the GPU with the library of the commit whose results are to be pinned (the file in
the repository was recorded with the commit before csrc/pointwise.hip was split);
tests/test_gpu_pointwise_bits.py asserts exact equality with it.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import _pointwise_bits as PB  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "pointwise_bits.json")
    golden = {name: fn() for name, fn in PB.GROUPS.items()}
    with open(out, "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {out}: {sum(len(g) for g in golden.values())} cases in {len(golden)} groups")


if __name__ == "__main__":
    main()
