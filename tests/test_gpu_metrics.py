"""rdn_image_metrics (csrc/metrics.hip) on the GPU against the CPU oracle
(oracle/metrics_ref.py: scikit-image 0.22 PSNR / SSIM restated, pinned in
tests/test_metrics_cpu.py).  Tolerance: the kernel keeps fp32 running sums of the 7
window rows' horizontal sums (formed afresh every 7th row) where scipy's
uniform_filter slides its sums in double and rounds the window means to fp32; on
zero-mean texture the cropped-mean SSIM agrees to ~1e-6 -- the tests allow 2e-5
absolute on SSIM and 1e-4 dB on PSNR (float64 sums on both sides).

The same 2e-5 holds per plane against float64 (oracle ssim_bruteforce) on
near-constant planes far from 0, where uxx - ux^2 cancels to ~1e-6 from terms of size
1 and a rounding error kept in a running sum goes straight into the variance
(test_flat_planes_match_float64; tests/test_metrics_cpu.py shows that the fp32
reference itself is within 5e-6 of float64 on exactly those planes).  Measured,
max over the 8 planes of a case, |GPU - float64| (running sums never re-formed ->
re-formed every 7th row):
  70x13   dark 5.0e-5 -> 5.5e-6   bright 5.2e-5 -> 3.7e-6   step 2.8e-5 -> 7.1e-6
  70x16   dark 6.0e-5 -> 4.6e-6   bright 6.6e-5 -> 8.2e-6   step 4.5e-5 -> 4.6e-6
  134x13  dark 2.6e-5 -> 7.2e-6   bright 4.4e-5 -> 5.5e-6   step 2.0e-5 -> 3.7e-6
  70x70   dark 1.1e-5 -> 2.9e-6   bright 1.3e-5 -> 2.0e-6   step 1.0e-5 -> 3.8e-6
  256x256 dark 8.9e-7 -> 7.2e-8
(data range 1, one 70x13 plane near 0.98, not asserted: 1.2e-4 -> 1.2e-5.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import metrics_ref as M  # noqa: E402


def _pair(rng, shape, noise=0.1, clip=True):
    a = rng.uniform(-1, 1, shape).astype(np.float32)
    # smooth structure so SSIM is far from 0 and from 1
    a = (a + np.roll(a, 1, -1) + np.roll(a, 1, -2)) / 3
    b = a + noise * rng.standard_normal(shape).astype(np.float32)
    if clip:
        b = np.clip(b, -1, 1)
    return a.astype(np.float32), b.astype(np.float32)


# (incl. several column tiles, and the 64-block SIDD batch of bench.py's metrics leg)
@pytest.mark.parametrize("shape", [(1, 1, 7, 7), (2, 3, 13, 70), (3, 3, 64, 64), (4, 3, 256, 256), (1, 2, 45, 130),
                                   (1, 3, 7, 8), (2, 3, 40, 520), (5, 3, 100, 248), (64, 3, 256, 256)])
def test_image_metrics_match_oracle(shape):
    from vub_image_denoising_amd.metrics import image_metrics
    rng = np.random.default_rng(shape[2] * 1000 + shape[3])
    a, b = _pair(rng, shape)
    psnr, ssim = image_metrics(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), 2.0)
    rp, rs = M.batch_metrics(a, b, 2.0)
    np.testing.assert_allclose(psnr.cpu().numpy(), rp, rtol=0, atol=1e-4)
    np.testing.assert_allclose(ssim.cpu().numpy(), rs, rtol=0, atol=2e-5)


def _flat_check(gt, x, ref, what):
    """Per-plane |GPU - float64| <= 2e-5 (N planes, C = 1: nothing is averaged over channels
    or images) and PSNR within 1e-4 dB of the oracle's; the figures are printed first."""
    from vub_image_denoising_amd.metrics import image_metrics
    psnr, ssim = image_metrics(torch.from_numpy(gt).cuda(), torch.from_numpy(x).cuda(), 2.0)
    ssim, psnr = ssim.cpu().numpy(), psnr.cpu().numpy()
    err = np.abs(ssim.astype(np.float64) - ref)
    print(f"flat planes {what}: |GPU - float64| per plane max {err.max():.2e} "
          f"[{' '.join(f'{e:.1e}' for e in err)}], SSIM {ref.min():.4f}..{ref.max():.4f}")
    np.testing.assert_allclose(psnr, [M.psnr(g, o, 2.0) for g, o in zip(gt, x)], rtol=0, atol=1e-4)
    assert err.max() <= 2e-5, (what, err)


@pytest.mark.parametrize("kind", M.FLAT_KINDS)
@pytest.mark.parametrize("hw", M.FLAT_SHAPES)
def test_flat_planes_match_float64(hw, kind):
    gt, x, ref = M.flat_planes_ref(kind, *hw)
    assert gt.shape == (M.FLAT_N, 1, *hw)
    _flat_check(gt, x, ref, f"{hw[0]}x{hw[1]} {kind}")


def test_flat_plane_256_matches_float64():
    """The realistic width (one column tile of 320 threads, four row tiles); the float64
    reference is the vectorised window loop (pinned to ssim_bruteforce in test_metrics_cpu)."""
    gt, x = M.flat_planes("dark", 256, 256, n=1)
    ref = np.array([M.ssim_windows64(gt[0, 0], x[0, 0], 2.0)])
    _flat_check(gt, x, ref, "256x256 dark")


def test_flat_plane_data_range_1_report():
    """No assertion on the kernel at data range 1 (the reference code uses 2; with planes near
    the top of the range the fp32 oracle itself is 1e-5 .. 2.5e-5 from float64 on narrow planes):
    prints where the kernel and the fp32 oracle stand on one 70x13 plane near 0.98."""
    from vub_image_denoising_amd.metrics import image_metrics
    rng = np.random.default_rng(5)
    gt = np.clip(0.98 + 1e-3 * rng.standard_normal((1, 1, 70, 13)), 0, 1).astype(np.float32)
    x = np.clip(gt + 1e-3 * rng.standard_normal(gt.shape), 0, 1).astype(np.float32)
    _, ssim = image_metrics(torch.from_numpy(gt).cuda(), torch.from_numpy(x).cuda(), 1.0)
    ref = M.ssim_bruteforce(gt[0].transpose(1, 2, 0), x[0].transpose(1, 2, 0), 1.0)
    orc = M.ssim(gt[0, 0], x[0, 0], 1.0)
    print(f"data range 1, 70x13 near 0.98: |GPU - float64| {abs(ssim.item() - ref):.2e}, "
          f"|fp32 oracle - float64| {abs(orc - ref):.2e} (SSIM {ref:.4f})")


def test_identical_and_edge_cases():
    from vub_image_denoising_amd.metrics import image_metrics, peak_signal_noise_ratio, structural_similarity
    rng = np.random.default_rng(3)
    a, b = _pair(rng, (2, 3, 32, 40))
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    psnr, ssim = image_metrics(ta, ta, 2.0)
    assert torch.isinf(psnr).all() and torch.allclose(ssim, torch.ones_like(ssim), atol=1e-6)
    # skimage-named single-image wrappers: HWC with channel_axis=-1 as evaluate_SIDD.py:63-64
    hwc_a, hwc_b = ta[1].permute(1, 2, 0), tb[1].permute(1, 2, 0)
    assert structural_similarity(hwc_a, hwc_b, data_range=2, channel_axis=-1) == pytest.approx(
        M.ssim(a[1].transpose(1, 2, 0), b[1].transpose(1, 2, 0), 2.0, channel_axis=-1), abs=2e-5)
    assert peak_signal_noise_ratio(hwc_a, hwc_b, data_range=2) == pytest.approx(M.psnr(a[1], b[1], 2.0), abs=1e-4)
    with pytest.raises(ValueError):
        image_metrics(ta[:, :, :6], tb[:, :, :6], 2.0)      # smaller than the 7x7 window
    with pytest.raises(RuntimeError):
        image_metrics(torch.from_numpy(a), torch.from_numpy(b), 2.0)   # CPU tensors: no fallback


def test_evaluate_model_end_to_end(tmp_path):
    """evaluate_SIDD.evaluate_model over a synthetic .mat: its averages equal the
    oracle's metrics of the same denoised blocks."""
    import scipy.io
    from torch.utils.data import DataLoader
    import vub_image_denoising_amd as vm
    from vub_image_denoising_amd.diffusion_RDUnet import DiffusionModel
    from vub_image_denoising_amd.evaluate_SIDD import SIDDMatDataset, evaluate_model
    rng = np.random.default_rng(7)
    gt = rng.integers(0, 256, (2, 3, 32, 32, 3), dtype=np.uint8)
    noisy = np.clip(gt.astype(np.int32) + rng.integers(-20, 21, gt.shape), 0, 255).astype(np.uint8)
    scipy.io.savemat(tmp_path / "n.mat", {"ValidationNoisyBlocksSrgb": noisy})
    scipy.io.savemat(tmp_path / "g.mat", {"ValidationGtBlocksSrgb": gt})
    ds = SIDDMatDataset(str(tmp_path / "n.mat"), str(tmp_path / "g.mat"))
    torch.manual_seed(0)
    model = DiffusionModel(vm.RDUNet_T(base_filters=16), timesteps=4).cuda()
    outs = []
    orig = model.improved_sampling

    def sampler(x):
        y = orig(x)
        outs.append(y.clone())
        return y

    p, s, t_ms, samples = evaluate_model(model, DataLoader(ds, batch_size=4), "cuda", sampler=sampler)
    den = torch.cat(outs).cpu().numpy()
    ref_gt = np.stack([ds[i][1].numpy() for i in range(len(ds))])
    rp, rs = M.batch_metrics(ref_gt, den, 2.0)
    assert p == pytest.approx(float(np.mean(rp)), abs=1e-4)
    assert s == pytest.approx(float(np.mean(rs)), abs=2e-5)
    assert t_ms > 0 and len(samples) == 0   # 6 blocks: none in the reference's sample range 11..14
