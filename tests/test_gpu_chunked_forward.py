"""The chunked forward-only path of engine.run_unet: a no-grad batch of more than
FWD_CHUNK_PIXELS pixels runs as chunks of images and is concatenated.  Here the
threshold is lowered to 2 x 32 x 32, so a 5 x 3 x 32 x 32 batch runs as chunks of 2, 2
and 1 images (a remainder chunk, served by a second cached engine).

* placement: rows [i:i+bc] of the chunked output are bit-identical to a direct call on
  x[i:i+bc], t[i:i+bc] of a fresh module with the same weights and no chunking (same
  batch, same engine shape, so this holds with split-K on): a wrong slice of x or t, a
  wrong concatenation order or a stale cached engine shows;
* t that is broadcast over the batch ([1,1,1,1] and 0-dim) is not sliced; a per-pixel
  t map [5,1,32,32] is;
* whole batch, split-K off: chunked == unchunked bit for bit (the images are
  independent and no kernel plan depends on the batch size);
* whole batch, split-K on: the number of split-K slices of a layer depends on the
  engine's batch (rdn_conv_fwd_splits looks at the tile grid), so a batch-2 or batch-1
  chunk may sum in another order than the batch-5 engine: the forward is not
  batch-invariant with split-K on (known).  Only the bounds of a
  different fp32 summation order hold (tests/test_gpu_splitk.py): rel-L2 1e-5 in fp32,
  1e-2 in bf16."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, S = 5, 32
CHUNK = 2 * S * S
DTYPES = [("fp32", torch.float32), ("bf16", torch.bfloat16)]


def _model(dtype):
    import vub_image_denoising_amd as vm
    torch.manual_seed(0)
    m = vm.RDUNet_T(base_filters=16).cuda().eval()
    m.set_compute_dtype(dtype)
    return m


def _x():
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).cuda()
    for i in range(B):
        for j in range(i):
            assert not torch.equal(x[i], x[j])
    return x


def _t(kind):
    g = torch.Generator().manual_seed(12)
    if kind == "per_sample":
        return torch.tensor([0.1, 0.3, 0.5, 0.7, 0.9]).view(B, 1, 1, 1).cuda()
    if kind == "one":
        return torch.tensor([0.4]).view(1, 1, 1, 1).cuda()
    if kind == "zero_dim":
        return torch.tensor(0.6).cuda()
    assert kind == "map"
    return torch.rand(B, 1, S, S, generator=g).cuda()


def _chunked(monkeypatch, m, x, t):
    from vub_image_denoising_amd import engine as E
    with monkeypatch.context() as mp:
        mp.setattr(E, "FWD_CHUNK_PIXELS", CHUNK)
        with torch.no_grad():
            return m(x, t).clone()


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize("dtype,tdt", DTYPES)
@pytest.mark.parametrize("kind", ["per_sample", "one", "zero_dim", "map"])
def test_chunk_placement(monkeypatch, dtype, tdt, kind):
    from vub_image_denoising_amd import engine as E
    assert E.SPLITK and E.FWD_CHUNK_PIXELS == 1 << 23
    x, t = _x(), _t(kind)
    m = _model(dtype)
    y = _chunked(monkeypatch, m, x, t)
    assert y.shape == x.shape
    # the module holds exactly two forward-only engines of this dtype: B = 2 and B = 1
    keys = sorted(k for k in m._rdn_engines if k[3] == tdt and not k[-1])
    assert [k[:3] for k in keys] == [(1, S, S), (2, S, S)], list(m._rdn_engines)
    assert all(len(m._rdn_engines[k]) == 1 for k in keys)
    assert len(m._rdn_engines) == 2
    # direct calls, unpatched threshold, fresh module with the same weights
    ref = _model(dtype)
    sliced = t.dim() > 0 and t.size(0) == B
    assert sliced == (kind in ("per_sample", "map"))
    for i in range(0, B, 2):
        ti = t[i:i + 2] if sliced else t
        with torch.no_grad():
            yi = ref(x[i:i + 2], ti)
        assert torch.equal(y[i:i + 2], yi), f"{kind}: rows {i}:{i + 2} of the chunked output"
    assert (1, S, S) in {k[:3] for k in ref._rdn_engines} and not any(k[0] == B for k in ref._rdn_engines)
    if kind != "map":   # distinct images (and t) give distinct rows
        assert not torch.equal(y[0], y[1]) and not torch.equal(y[2], y[4])


@pytest.mark.parametrize("dtype,tdt", DTYPES)
@pytest.mark.parametrize("split", [False, True])
def test_chunked_equals_whole_batch(monkeypatch, dtype, tdt, split):
    """Split-K off: bit-identical.  Split-K on: the slice count depends on the engine's
    batch, so only the summation-order bounds hold (module docstring)."""
    from vub_image_denoising_amd import engine as E
    monkeypatch.setattr(E, "SPLITK", split)
    x, t = _x(), _t("per_sample")
    y_chunk = _chunked(monkeypatch, _model(dtype), x, t)
    whole = _model(dtype)
    with torch.no_grad():
        y_whole = whole(x, t)
    assert [k[:3] for k in whole._rdn_engines] == [(B, S, S)]
    r = _rel(y_chunk, y_whole)
    print(f"{dtype} split={split}: chunked vs whole batch rel-L2 {r:.3e}, bit-identical {torch.equal(y_chunk, y_whole)}")
    if not split:
        assert torch.equal(y_chunk, y_whole)
    assert r <= (1e-5 if dtype == "fp32" else 1e-2)
