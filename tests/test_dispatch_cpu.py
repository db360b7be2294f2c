"""The host dispatch of the conv launchers, pinned without a GPU: which kernel
instantiation, how many splits and how many channel chunks every descriptor of two
grids gets (scripts/make_dispatch_golden.py holds the grids and wrote
tests/golden/dispatch.json).  The probes run the launchers' decisions in-process on
fake, 16-byte aligned pointers; nothing is launched.  A dispatch decision that moves
fails here as a diff of kernel names.  (The golden records the default dispatch: no
RDN_* knob set.)"""
import importlib.util
import json
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_sweeps():
    spec = importlib.util.spec_from_file_location(
        "make_dispatch_golden", os.path.join(REPO, "scripts", "make_dispatch_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load_sweeps()


@pytest.fixture(scope="module")
def golden_dispatch():
    with open(G.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def wgrad_records():
    from vub_image_denoising_amd import _hip as H
    return list(G.sweep_wgrad(H.load_library(), H))


@pytest.fixture(scope="module")
def fwd_records():
    from vub_image_denoising_amd import _hip as H
    return list(G.sweep_fwd(H.load_library(), H))


def _check(records, want):
    got = G.summarise(records)
    assert got["descriptors"] == want["descriptors"]
    moved = {n: (want["names"].get(n, 0), got["names"].get(n, 0))
             for n in sorted(set(want["names"]) | set(got["names"])) if want["names"].get(n) != got["names"].get(n)}
    assert not moved, f"kernel name: descriptors (golden, now): {moved}"
    assert got["sha256"] == want["sha256"], "same kernels per name, but a descriptor's name, splits or chunks moved"


def test_wgrad_dispatch_matches_golden(wgrad_records, golden_dispatch):
    """Kernel, splits (rdn_wgrad_splits) and chunks (rdn_wgrad_chunks) of the 21120
    weight-gradient descriptors; none of them depends on the CU count."""
    assert all(rc == 0 for _, rc, *_ in wgrad_records)
    _check(wgrad_records, golden_dispatch["wgrad"])


def test_fwd_dispatch_matches_golden(fwd_records, golden_dispatch):
    """Kernel of the 30464 forward / input-gradient descriptors.  The halo kernel's block
    pairing and conv3_big's plans go by the CU count: compared on a 256-CU device (what a
    failed device query counts as) only."""
    assert all(rc == 0 for _, rc, *_ in fwd_records)
    cus256 = not torch.cuda.is_available() or torch.cuda.get_device_properties(0).multi_processor_count == 256
    if cus256:
        _check(fwd_records, golden_dispatch["fwd"])
    else:
        assert len(fwd_records) == golden_dispatch["fwd"]["descriptors"]


def test_no_dispatch_reaches_the_removed_variants(wgrad_records, fwd_records):
    """Facts that need no golden: the 3x3 gather of conv_gemm_kernel / wgrad_kernel and the
    bf16 wgrad3_halo_kernel are gone, the LDS-DMA kernel is built for 8 tile shapes, and the
    rows kernel stays inside its accumulator budget (two blocks per CU)."""
    names = {r[2] for r in wgrad_records} | {r[2] for r in fwd_records}
    assert not [n for n in names if re.match(r"conv_gemm_kernel<.*,0(,split)?>$", n)]
    assert not [n for n in names if n.startswith("wgrad3_halo_kernel<bf16")]
    assert all(re.match(r"wgrad_kernel<(bf16|f32),\d+,\d+,\d+>$", n) for n in names if n.startswith("wgrad_kernel<"))
    glds = {n for n in names if n.startswith("wgrad3_glds_kernel<")}
    assert glds == {f"wgrad3_glds_kernel<bf16,{bm},{ck}>" for bm in (32, 64) for ck in (32, 64, 80, 96)}
    rows = [re.match(r"wgrad3_rows_kernel<bf16,(\d+),(\d+)(,gate)?>$", n) for n in names
            if n.startswith("wgrad3_rows_kernel<")]
    assert rows and all(m and int(m.group(1)) * int(m.group(2)) <= 2560 for m in rows)
