"""SIDD metrics, CPU side: the numpy restatement of scikit-image 0.22's PSNR/SSIM
(oracle/metrics_ref.py; skimage itself is not installed here) pinned against an
independent float64 brute-force window loop and closed forms, and the
SIDDMatDataset item transform (ToTensor + Normalize(0.5, 0.5)) on a .mat written
here.  Parity of the GPU kernel with this oracle: tests/test_gpu_metrics.py."""
import numpy as np
import pytest
import torch

from oracle import metrics_ref as M


@pytest.mark.parametrize("shape", [(7, 7, 1), (12, 15, 3), (20, 9, 2)])
def test_ssim_matches_bruteforce(shape):
    rng = np.random.default_rng(sum(shape))
    a = rng.uniform(-1, 1, shape).astype(np.float32)
    b = np.clip(a + 0.2 * rng.standard_normal(shape), -1, 1).astype(np.float32)
    assert abs(M.ssim(a, b, 2.0, channel_axis=-1) - M.ssim_bruteforce(a, b, 2.0)) < 1e-6


@pytest.mark.parametrize("kind", M.FLAT_KINDS)
@pytest.mark.parametrize("hw", M.FLAT_SHAPES)
def test_flat_planes_fp32_reference_within_5e6_of_float64(hw, kind):
    """The inputs of tests/test_gpu_metrics.py::test_flat_planes_match_float64: on exactly
    those planes the fp32 skimage restatement is within 5e-6 of the float64 window loop, so
    the GPU test's 2e-5 sits 4x above what the reference arithmetic itself needs.  (Fails
    if the planes are ever swapped for ones on which that bound is not achievable.)"""
    gt, x, ref = M.flat_planes_ref(kind, *hw)
    assert gt.shape == x.shape == (M.FLAT_N, 1, *hw) and gt.dtype == x.dtype == np.float32
    assert np.abs(gt).max() <= 1 and np.abs(x).max() <= 1
    assert np.abs(x - gt).max() < 1e-2 and not np.array_equal(gt, x)
    flat = gt[:, :, hw[0] // 4:] if kind == "step" else gt
    assert abs(flat.mean() - (0.95 if kind == "bright" else -0.97)) < 1e-3 and flat.std() < 2e-3
    if kind == "step":
        assert gt[:, :, :hw[0] // 4].std() > 0.4
    err = [abs(M.ssim(g[0], o[0], 2.0) - r) for g, o, r in zip(gt, x, ref)]
    print(f"{hw} {kind}: |fp32 oracle - float64| max {max(err):.2e}")
    assert max(err) <= 5e-6
    # the vectorised float64 window loop (the 256^2 plane's reference) is the loop's number
    assert abs(M.ssim_windows64(gt[0, 0], x[0, 0], 2.0) - ref[0]) < 1e-12


def test_closed_forms():
    a = np.full((9, 11, 1), 0.3, np.float32)
    b = np.full((9, 11, 1), -0.2, np.float32)
    c1 = 0.02 ** 2
    assert abs(M.ssim(a, b, 2.0, channel_axis=-1) - (2 * 0.3 * -0.2 + c1) / (0.09 + 0.04 + c1)) < 1e-6
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, (16, 16, 3)).astype(np.float32)
    assert M.ssim(x, x, 2.0, channel_axis=-1) == pytest.approx(1.0, abs=1e-6)
    assert M.psnr(x, x, 2.0) == float("inf")
    y = x + np.float32(0.1)
    mse = np.mean((x - y) ** 2, dtype=np.float64)
    assert M.psnr(x, y, 2.0) == pytest.approx(10 * np.log10(4.0 / mse), rel=1e-12)
    # channel_axis=0 (CHW) and -1 (HWC) give the same number
    z = np.clip(x + 0.05, -1, 1)
    assert M.ssim(x, z, 2.0, channel_axis=-1) == pytest.approx(
        M.ssim(x.transpose(2, 0, 1), z.transpose(2, 0, 1), 2.0, channel_axis=0), abs=1e-12)


def test_sidd_mat_dataset_items(tmp_path):
    import scipy.io
    from vub_image_denoising_amd.evaluate_SIDD import SIDDMatDataset
    rng = np.random.default_rng(0)
    noisy = rng.integers(0, 256, (2, 3, 16, 16, 3), dtype=np.uint8)
    gt = rng.integers(0, 256, (2, 3, 16, 16, 3), dtype=np.uint8)
    scipy.io.savemat(tmp_path / "n.mat", {"ValidationNoisyBlocksSrgb": noisy})
    scipy.io.savemat(tmp_path / "g.mat", {"ValidationGtBlocksSrgb": gt})
    ds = SIDDMatDataset(str(tmp_path / "n.mat"), str(tmp_path / "g.mat"))
    assert len(ds) == 6
    n4, g4 = ds[4]    # image 1, block 1 (evaluate_SIDD.py:31-33)
    assert n4.shape == (3, 16, 16) and n4.dtype == torch.float32
    want = (noisy[1, 1].transpose(2, 0, 1).astype(np.float32) / 255 - 0.5) / 0.5
    np.testing.assert_allclose(n4.numpy(), want, rtol=0, atol=1e-7)
    np.testing.assert_allclose(g4.numpy(), (gt[1, 1].transpose(2, 0, 1).astype(np.float32) / 255 - 0.5) / 0.5,
                               rtol=0, atol=1e-7)
