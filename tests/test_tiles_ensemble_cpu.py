"""Host side of the geometric self-ensemble (no GPU): the new names in the header, the
library and the binding, the argument checks of rdn_tile_gather_d4 / rdn_tile_accum_d4
(fake pointers: every check returns before a launch), the Python and command-line
arguments, and the self-consistency of the restatement in tests/_tiles_ens_ref.py."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tiles_ens_ref as ER  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATHER, ACCUM = "rdn_tile_gather_d4", "rdn_tile_accum_d4"
FAKE = 4096      # never dereferenced


def _lib():
    from vub_image_denoising_amd import _hip as H
    return H.load_library()


def test_new_names_are_declared_exported_and_bound():
    from vub_image_denoising_amd import _hip as H
    from vub_image_denoising_amd import sampling
    with open(os.path.join(REPO, "include", "rdunet_hip.h")) as f:
        header = f.read()
    raw = ctypes.CDLL(H.LIB_PATH)        # untyped: a plain symbol lookup in the library's exports
    lib = _lib()
    for name in (GATHER, ACCUM):
        assert f"int {name}(" in header
        assert hasattr(raw, name)
        assert name in H.SIGNATURES and len(H.SIGNATURES[name][1]) == (13 if name == GATHER else 12)
        assert getattr(lib, name).argtypes == H.SIGNATURES[name][1]
    for name in ("tile_gather_d4", "tile_accum_d4"):
        assert callable(getattr(sampling, name))


def _gather(lib, img=FAKE, n=1, c=3, h=64, w=64, tile=32, ov=8, d0=0, nd=1, first=0, count=1, tiles=FAKE):
    return lib.rdn_tile_gather_d4(img, n, c, h, w, tile, ov, d0, nd, first, count, tiles, None)


def _accum(lib, src=FAKE, acc=FAKE, n_tiles=4, c=3, th=32, tw=32, d0=0, nd=1, n_ens=8, first=0, count=1):
    return lib.rdn_tile_accum_d4(src, acc, n_tiles, c, th, tw, d0, nd, n_ens, first, count, None)


def _fails(rc, lib, entry, *names):
    msg = lib.rdn_last_error()
    assert rc == -1, (rc, msg)
    assert entry.encode() in msg, msg
    for name in names:
        assert name in msg, msg


GRID_BAD = [  # the existing grid checks: (h, w, tile, overlap, c, name in the message)
    (64, 64, 20, 4, 3, b"tile="),
    (64, 64, 8, 0, 3, b"tile="),
    (64, 64, 32, -1, 3, b"overlap="),
    (64, 64, 32, 17, 3, b"overlap="),
    (7, 64, 32, 8, 3, b"h="),
    (64, 7, 32, 8, 3, b"w="),
    (64, 64, 32, 8, 0, b"c="),
    (64, 64, 32, 8, 9, b"c="),
]


@pytest.mark.parametrize("h,w,tile,ov,c,name", GRID_BAD)
def test_gather_d4_grid_checks(h, w, tile, ov, c, name):
    lib = _lib()
    _fails(_gather(lib, h=h, w=w, tile=tile, ov=ov, c=c), lib, GATHER, name)


PASS_BAD = [  # (d0, nd, names in the message); n_ens = 8 for the accumulate
    (0, 0, (b"nd=",)),
    (0, -3, (b"nd=",)),
    (-1, 1, (b"d0=",)),
    (5, 4, (b"d0=", b"nd=")),
    (8, 1, (b"d0=", b"nd=")),
    (0, 9, (b"d0=", b"nd=")),
]


@pytest.mark.parametrize("d0,nd,names", PASS_BAD)
def test_pass_checks(d0, nd, names):
    lib = _lib()
    _fails(_gather(lib, d0=d0, nd=nd), lib, GATHER, *names)
    _fails(_accum(lib, d0=d0, nd=nd), lib, ACCUM, *names)


@pytest.mark.parametrize("d0,nd", [(0, 8), (2, 4), (3, 2), (1, 4)])
def test_a_pass_must_not_straddle_d4_on_non_square_tiles(d0, nd):
    lib = _lib()
    # a 16 x 64 image at tile 32 has 16 x 32 tiles
    _fails(_gather(lib, h=16, w=64, d0=d0, nd=nd), lib, GATHER, b"d0=", b"nd=", b"straddle")
    _fails(_accum(lib, th=16, tw=32, d0=d0, nd=nd), lib, ACCUM, b"d0=", b"nd=", b"straddle")


def test_counts_and_null_pointers():
    lib = _lib()
    _fails(_gather(lib, img=None), lib, GATHER, b"img")
    _fails(_gather(lib, tiles=None), lib, GATHER, b"tiles")
    _fails(_gather(lib, n=0), lib, GATHER, b"n=")
    _fails(_gather(lib, first=-1), lib, GATHER, b"first=")
    _fails(_gather(lib, count=0), lib, GATHER, b"count=")
    _fails(_accum(lib, src=None), lib, ACCUM, b"src")
    _fails(_accum(lib, acc=None), lib, ACCUM, b"acc")
    _fails(_accum(lib, n_tiles=0), lib, ACCUM, b"n_tiles=")
    _fails(_accum(lib, first=-1), lib, ACCUM, b"first=")
    _fails(_accum(lib, count=0), lib, ACCUM, b"count=")
    _fails(_accum(lib, c=0), lib, ACCUM, b"c=")
    _fails(_accum(lib, c=9), lib, ACCUM, b"c=")
    _fails(_accum(lib, th=12), lib, ACCUM, b"th=")
    _fails(_accum(lib, tw=4), lib, ACCUM, b"tw=")


@pytest.mark.parametrize("n_ens", [0, 3, 5, 6, 7, 16, -1])
def test_accum_n_ens_must_be_1_2_4_8(n_ens):
    lib = _lib()
    _fails(_accum(lib, n_ens=n_ens), lib, ACCUM, b"n_ens=")


@pytest.mark.parametrize("d0,nd,n_ens", [(0, 2, 1), (0, 4, 2), (1, 2, 2), (2, 3, 4), (4, 4, 4)])
def test_accum_pass_must_fit_the_ensemble(d0, nd, n_ens):
    lib = _lib()
    _fails(_accum(lib, d0=d0, nd=nd, n_ens=n_ens), lib, ACCUM, b"n_ens=", b"d0=", b"nd=")


def test_accum_past_the_end_launches_nothing():
    lib = _lib()
    assert _accum(lib, n_tiles=2, nd=4, first=8, count=5) == 0      # surplus items only: fake pointers untouched


# ------------------------------------------------------------------ Python and command line
@pytest.mark.parametrize("bad", [3, 0, 16, -1, 5, "8", None])
def test_denoise_tiled_rejects_other_ensembles_before_the_device(bad):
    import vub_image_denoising_amd as vm
    with pytest.raises(ValueError, match="ensemble"):
        vm.denoise_tiled(None, torch.zeros(1, 3, 40, 40), ensemble=bad)


def test_ensemble_1_still_asks_for_device_tensors():
    import vub_image_denoising_amd as vm
    model = vm.DiffusionModel(vm.RDUNet_T(base_filters=16), timesteps=2)
    for n in (1, 8):
        with pytest.raises(RuntimeError, match="GPU"):
            model.denoise_image(torch.zeros(1, 3, 40, 40), ensemble=n)


def test_cli_parser_ensemble():
    from vub_image_denoising_amd.denoise_image import build_parser
    base = ["--checkpoint", "c.pth", "--input", "i.png", "--output", "o.png"]
    assert build_parser().parse_args(base).ensemble == 1
    for n in (1, 2, 4, 8):
        assert build_parser().parse_args(base + ["--ensemble", str(n)]).ensemble == n
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--ensemble", "3"])


def test_evaluate_sidd_main_takes_ensemble():
    import inspect
    from vub_image_denoising_amd import evaluate_SIDD
    assert inspect.signature(evaluate_SIDD.main).parameters["ensemble"].default == 1
    with pytest.raises(ValueError, match="ensemble"):
        evaluate_SIDD.main(ensemble=3)


def test_passes_of_sampling_are_the_restatement():
    from vub_image_denoising_amd.sampling import ensemble_passes
    for n in (1, 2, 4, 8):
        for th, tw in ((32, 32), (16, 32), (40, 24)):
            assert ensemble_passes(n, th, tw) == ER.passes(n, th, tw)


# ------------------------------------------------------------------ the restatement itself
SHAPES = [(16, 32), (40, 24), (32, 32)]


def _tile(th, tw, seed=0):
    return torch.rand(th, tw, generator=torch.Generator().manual_seed(seed + 100 * th + tw))


@pytest.mark.parametrize("th,tw", SHAPES)
def test_inverse_of_transform_is_identity(th, tw):
    u = _tile(th, tw)
    for d in range(8):
        t = ER.transform(u, d)
        assert t.shape == ((tw, th) if d & 4 else (th, tw))
        assert torch.equal(ER.inverse(t, d), u)
        assert torch.equal(ER.transform(ER.inverse(t, d), d), t)
    # the eight transforms of an asymmetric tile are distinct
    if th == tw:
        ts = [ER.transform(u, d) for d in range(8)]
        assert all(not torch.equal(ts[a], ts[b]) for a in range(8) for b in range(a))


@pytest.mark.parametrize("th,tw", SHAPES)
def test_element_formula_is_the_flip_transpose_form(th, tw):
    u = _tile(th, tw, seed=1)
    for d in range(8):
        assert torch.equal(ER.transform_elementwise(u, d), ER.transform(u, d)), d


def test_passes_and_work_item_order():
    assert ER.passes(8, 32, 32) == [(0, 8)] and ER.passes(4, 32, 32) == [(0, 4)] and ER.passes(1, 32, 32) == [(0, 1)]
    assert ER.passes(8, 16, 32) == [(0, 4), (4, 4)]
    assert ER.passes(4, 16, 32) == [(0, 4)] and ER.passes(2, 16, 32) == [(0, 2)] and ER.passes(1, 16, 32) == [(0, 1)]
    for n in (1, 2, 4, 8):
        for th, tw in SHAPES:
            ds = [d for d0, nd in ER.passes(n, th, tw) for d in range(d0, d0 + nd)]
            assert ds == list(range(n))                       # every transform once, ascending
            for d0, nd in ER.passes(n, th, tw):
                assert th == tw or len({bool(d & 4) for d in range(d0, d0 + nd)}) == 1     # one tile shape per pass
    # tile-major: the transforms of a tile are adjacent, in ascending d
    assert [ER.work_item(w, 4, 4) for w in range(9)] == [(0, 4), (0, 5), (0, 6), (0, 7), (1, 4), (1, 5), (1, 6), (1, 7), (2, 4)]
    assert [ER.work_item(w, 1, 3) for w in range(5)] == [(0, 1), (0, 2), (0, 3), (1, 1), (1, 2)]
    # a batch past the end repeats the last item
    assert ER.batch_items(5, 5, 3, 0, 2) == [(2, 1)] * 5
    assert ER.batch_items(3, 5, 3, 0, 2) == [(1, 1), (2, 0), (2, 1), (2, 1), (2, 1)]


@pytest.mark.parametrize("th,tw,n", [(32, 32, 8), (16, 32, 8), (16, 32, 4), (40, 24, 2), (32, 32, 1)])
def test_sum_is_the_same_bits_at_any_batch_boundary(th, tw, n):
    n_tiles, C = 3, 2
    g = torch.Generator().manual_seed(5)
    members = torch.rand(n_tiles, n, C, th, tw, generator=g) * 2 - 1     # v_d of every tile, already mapped back
    want = torch.stack([ER.ensemble_mean(members[t]) for t in range(n_tiles)])
    results = []
    for batch in (1, 2, 3, 5, 7, n_tiles * 8):
        acc = torch.full((n_tiles, C, th, tw), float("nan"))
        for d0, nd in ER.passes(n, th, tw):
            items = [ER.work_item(w, d0, nd) for w in range(n_tiles * nd)]
            for first in range(0, n_tiles * nd, batch):
                src = torch.stack([ER.transform(members[t, d], d) for t, d in ER.batch_items(first, batch, n_tiles, d0, nd)])
                assert items[first] == ER.batch_items(first, batch, n_tiles, d0, nd)[0]
                ER.accumulate(acc, src, d0, nd, n, first, batch)
        results.append(acc)
    for acc in results:
        assert torch.equal(acc, want)
