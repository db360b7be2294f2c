"""CPU-only checks of the host side: the C-ABI library loads and exports every
symbol include/rdunet_hip.h declares (no compute calls without a GPU), the
drop-in module API (names, state_dict, init parity), and host logic."""
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    src = open(os.path.join(REPO, "include", "rdunet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rdn_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    import ctypes
    from vub_image_denoising_amd import _hip as H
    lib = H.load_library()
    decl = _declared_symbols()
    assert len(decl) >= 20
    for name in decl:
        assert hasattr(lib, name), name
        assert name in H.SIGNATURES, f"{name} not bound in _hip.SIGNATURES"
    assert lib.rdn_version().startswith(b"rdunet_hip")
    # argument validation runs on the host, no GPU touched
    d = H.ConvDesc()
    assert lib.rdn_conv_fwd(ctypes.byref(d), None) == -1
    assert b"null" in lib.rdn_last_error()


def test_struct_layout_matches_header():
    """ctypes struct field order/types mirror the C typedefs."""
    from vub_image_denoising_amd import _hip as H
    src = open(os.path.join(REPO, "include", "rdunet_hip.h")).read()
    body = re.search(r"typedef struct rdn_conv_desc \{(.*?)\} rdn_conv_desc;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\**\s*([a-z_0-9]+)\s*[,;]", body)
    assert names == [f for f, _ in H.ConvDesc._fields_]
    body = re.search(r"typedef struct rdn_wgrad_desc \{(.*?)\} rdn_wgrad_desc;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\**\s*([a-z_0-9]+)\s*[,;]", body)
    assert names == [f for f, _ in H.WgradDesc._fields_]
    body = re.search(r"typedef struct rdn_dense3_desc \{(.*?)\} rdn_dense3_desc;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\**\s*([a-z_0-9]+)\s*(?:\[\d+\])?\s*[,;]", body)
    assert names == [f for f, _ in H.Dense3Desc._fields_]


def test_dense3_level_validation_on_host():
    """rdn_dense3_fwd rejects an unknown x_c and a level-1 descriptor with short packed
    K before anything is launched (no GPU needed)."""
    import ctypes
    from vub_image_denoising_amd import _hip as H
    lib = H.load_library()
    d = H.Dense3Desc()
    d.n, d.h, d.w = 1, 32, 32
    d.x, d.x_pl = 4096, 32 * 32 * 32
    for k in range(3):
        d.out[k] = d.pre[k] = d.wp[k] = 4096 * (k + 2)
        d.bias[k] = d.alpha[k] = 4096
    d.kp[0], d.kp[1], d.kp[2] = 576, 896, 1152
    d.x_c = 48
    assert lib.rdn_dense3_fwd(ctypes.byref(d), None) == -1 and b"x_c" in lib.rdn_last_error()
    d.x_c = 64
    d.kp[1] = 864   # conv_1 needs the packed K of 96 channels rounded to 64: 896
    assert lib.rdn_dense3_fwd(ctypes.byref(d), None) < 0 and b"packed K" in lib.rdn_last_error()
    d.kp[1], d.h = 896, 24   # level-1 grid must be a multiple of 16
    assert lib.rdn_dense3_fwd(ctypes.byref(d), None) < 0 and b"H % 16" in lib.rdn_last_error()


def _dw_pair(ck, ncols, nhw, gated=True, gout_c0=None):
    """Descriptor pair of one fused dgrad + wgrad launch over fake, 16-byte aligned
    pointers: bf16, `ck` dY channels, `ncols` input channels."""
    from vub_image_denoising_amd import _hip as H
    d, wg = H.ConvDesc(), H.WgradDesc()
    d.dtype = wg.dtype = H.RDN_BF16
    d.gather = wg.gather = H.RDN_G_CONV3
    d.n, d.h, d.w = wg.n, wg.h, wg.w = nhw
    d.hin, d.win = wg.hin, wg.win = nhw[1], nhw[2]
    d.cin = wg.mdim = ck
    d.ncols = d.cout = wg.ndim = ncols
    d.kp = (9 * ck + 63) // 64 * 64
    d.x = wg.a = 1 << 20
    d.wp, d.out, wg.b, wg.ws = 2 << 20, 3 << 20, 4 << 20, 5 << 20
    d.x_ps = wg.a_ps = ck
    d.out_ps = wg.b_ps = ncols
    if gated:
        d.gate = wg.a_gate = 6 << 20
        d.gate_alpha = wg.a_gate_alpha = 7 << 20
        d.gate_ps = wg.a_gate_ps = ck
        wg.part = 8 << 20
    if gout_c0 is not None:
        d.gout, d.gout_pre, d.gout_alpha, d.gout_part = 9 << 20, 10 << 20, 11 << 20, 12 << 20
        d.gout_c0 = gout_c0
        d.gout_ps = d.gout_pre_ps = ncols - gout_c0
    return d, wg


# (dY channels, input channels, variant) -> kernel, column parts; the variant is "" (gated),
# "pregated" (no gate, no partials) or the first channel of a gate-out tail
_DW_SERVED = (
    [((ck, nc, ""), (f"conv3_dw_kernel<bf16,{nc},{ck}>", 1)) for ck in (16, 32) for nc in (32, 48, 64, 80)]
    + [((32, 96, ""), ("conv3_dw_kernel<bf16,48,32,h2>", 2)),
       ((32, 128, ""), ("conv3_dw_kernel<bf16,64,32,h2>", 2)),
       ((64, 160, ""), ("conv3_dw_kernel<bf16,32,64,h5>", 5)),
       ((64, 160, "pregated"), ("conv3_dw_kernel<bf16,32,64,h5,pregated>", 5)),
       ((32, 96, 32), ("conv3_dw_kernel<bf16,48,32,h2,go>", 2)),
       ((32, 64, 0), ("conv3_dw_kernel<bf16,64,32,go>", 1))])


def test_fused_dgrad_wgrad_dispatch_table():
    """The fused pair's host dispatch without a GPU: kernel name, split count, columns per
    slab and gate-out partial rows of every served shape, and the pairs it leaves to the
    separate kernels.  Split counts are those of a 256-CU device (what a failed device
    query counts as): 8 x parts at one tile, min(256 / (8 parts), 8 tiles per XCD) x 8 x
    parts at (2, 64, 64)."""
    import ctypes
    from vub_image_denoising_amd import _hip as H
    lib = H.load_library()
    cus256 = not torch.cuda.is_available() or torch.cuda.get_device_properties(0).multi_processor_count == 256

    def probe(d, wg):
        buf = ctypes.create_string_buffer(128)
        rc = lib.rdn_conv_dgrad_wgrad_kernel_name(ctypes.byref(d), ctypes.byref(wg), buf, 128)
        return (rc, buf.value.decode(), lib.rdn_conv_dgrad_wgrad_splits(ctypes.byref(d), ctypes.byref(wg)),
                lib.rdn_conv_dgrad_wgrad_cols(ctypes.byref(d), ctypes.byref(wg)),
                lib.rdn_conv_dgrad_wgrad_gate_rows(ctypes.byref(d), ctypes.byref(wg)))

    def pair(key, nhw):
        ck, nc, var = key
        return _dw_pair(ck, nc, nhw, gated=var != "pregated", gout_c0=var if isinstance(var, int) else None)

    assert len(_DW_SERVED) == 14
    for key, (name, nh) in _DW_SERVED:
        for nhw, splits in (((1, 8, 16), 8 * nh), ((2, 64, 64), {1: 64, 2: 128, 5: 240}[nh])):
            rc, got, sp, cols, rows = probe(*pair(key, nhw))
            assert (rc, got, cols) == (0, name, key[1] // nh), (key, nhw, rc, got, cols)
            go = isinstance(key[2], int)
            assert (rows > 0) == go and (not go or rows == sp), (key, nhw, rows, sp)
            if cus256:
                assert sp == splits, (key, nhw, sp)
            else:
                assert sp > 0 and sp % (8 * nh) == 0, (key, nhw, sp)
        d, wg = pair(key, (1, 12, 16))   # ragged tile rows: not served
        assert probe(d, wg) == (1, "", 0, 0, 0), key
    for ck, nc in ((16, 96), (32, 112), (64, 128), (48, 48)):
        assert probe(*_dw_pair(ck, nc, (2, 64, 64))) == (1, "", 0, 0, 0), (ck, nc)


def test_state_dict_keys_and_shapes_match_oracle_spec():
    import vub_image_denoising_amd as vm
    from oracle.rdunet_ref import param_shapes
    for F0 in (16, 32):
        sd = vm.RDUNet_T(base_filters=F0).state_dict()
        spec = param_shapes(F0)
        assert list(sd.keys()) == list(spec.keys())
        assert all(tuple(sd[k].shape) == spec[k] for k in sd)
    sd = vm.RDUNet(channels=3, base_filters=16).state_dict()
    assert list(sd.keys()) == list(param_shapes(16, 3, 3).keys())


def test_init_matches_reference_rng_stream(golden):
    """torch.manual_seed(0); RDUNet_T(16) draws the same initial weights as the
    reference constructor (fixture: per-tensor sums recorded from the reference)."""
    if "init16_sums" not in golden.files:
        pytest.skip("fixture predates init sums")
    import vub_image_denoising_amd as vm
    torch.manual_seed(0)
    sd = vm.RDUNet_T(base_filters=16).state_dict()
    sums = np.array([v.double().sum().item() for v in sd.values()])
    np.testing.assert_allclose(sums, golden["init16_sums"], rtol=1e-6, atol=1e-9)


def test_backward_routing_plan():
    """Every gradient buffer is stored once before any accumulation, in
    backward execution order."""
    from vub_image_denoising_amd.engine import _assign_backward, _plan
    prog = _plan(32, 3, True, 3)
    layers, bufs = prog.layers, prog.bufs
    _assign_backward(layers)
    assert len(layers) == 69
    seen = set()
    for L in reversed(layers):
        if L.accum:
            assert L.dsrc.buf in seen, L.name
        else:
            assert L.dsrc.buf not in seen, L.name
        seen.add(L.dsrc.buf)
    acc = {L.name for L in layers if L.accum}
    # the skip-connection buffers receive down_l's gradient on top of up_l.conv's
    assert {"down_0.conv", "down_1.conv", "down_2.conv"} <= acc
    for L in layers:
        if L.dst is not None:
            assert "d" + L.dst.buf in {"d" + b for b in bufs}


def test_cpu_tensors_fail_loudly():
    import vub_image_denoising_amd as vm
    m = vm.RDUNet_T(base_filters=16)
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(1, 3, 16, 16), torch.zeros(1, 1, 1, 1))


def test_block_forward_needs_gpu_tensors():
    """A block's own forward runs on the GPU engine (no CPU path)."""
    import vub_image_denoising_amd as vm
    with pytest.raises(RuntimeError, match="GPU"):
        vm.DenoisingBlock(32, 16, 32)(torch.zeros(1, 32, 8, 8))


def test_block_programs():
    """Every block of Unet_model.py:23-89 maps to an engine Program with the
    reference's parameter names, input/output levels and channel counts."""
    import vub_image_denoising_amd as vm
    from vub_image_denoising_amd.engine import block_program
    cases = [(vm.DenoisingBlock(32, 16, 32), [("X", 0, 32)], 0, 32, True, 4),
             (vm.InputBlock(4, 32), [("X", 0, 4)], 0, 32, False, 2),
             (vm.OutputBlock(32, 3), [("X", 0, 32)], 0, 3, False, 2),
             (vm.DownsampleBlock(32, 64), [("X", 0, 32)], 1, 64, False, 1),
             (vm.UpsampleBlock(64, 32, 32), [("U", 1, 64), ("CAT", 0, 32)], 0, 32, False, 2)]
    for blk, inputs, olvl, oc, resid, nl in cases:
        prog = block_program(blk)
        assert prog.inputs == inputs and prog.out_level == olvl and prog.out_channels == oc
        assert prog.resid_input == resid and len(prog.layers) == nl
        names = {n for n, _ in blk.named_parameters()}
        for L in prog.layers:
            assert {L.name + ".weight", L.name + ".bias", L.act + ".weight"} <= names
        assert prog.layers[-1].dst is None and all(L.dst is not None for L in prog.layers[:-1])
    with pytest.raises(ValueError, match="multiples of 8"):
        block_program(vm.DenoisingBlock(12, 6, 12))
    with pytest.raises(ValueError, match="out_channels"):
        block_program(vm.DenoisingBlock(32, 16, 48))


def test_trainer_variants_keep_reference_signatures():
    """The three reference scripts declare different trainer signatures
    (diffusion_RDUnet.py:76,117; main_diffusion_RDUnet.py:237,275;
    diffusion_RDUnet_direct.py:228,266): each drop-in module keeps its own."""
    import inspect
    from vub_image_denoising_amd import diffusion_RDUnet as A, diffusion_RDUnet_direct as D, main_diffusion_RDUnet as M

    def names(f):   # the reference's positional parameters (keyword-only extensions allowed)
        return [n for n, q in inspect.signature(f).parameters.items() if q.kind != q.KEYWORD_ONLY]

    assert names(A.train_step_checkpointed)[:7] == ["model", "clean_images", "noisy_images", "optimizer",
                                                    "accumulation_steps", "distribution_choice", "clip_value"]
    assert names(A.train_model_checkpointed)[:8] == ["model", "train_loader", "val_loader", "optimizer", "scheduler",
                                                     "writer", "output_dir", "distribution_choice"]
    for mod in (M, D):
        assert names(mod.train_step_checkpointed) == ["model", "clean_images", "noisy_images", "optimizer",
                                                      "accumulation_steps", "clip_value"]
        assert names(mod.train_model_checkpointed) == ["model", "train_loader", "val_loader", "optimizer", "scheduler",
                                                       "writer", "num_epochs", "start_epoch", "accumulation_steps",
                                                       "clip_value"]
        assert names(mod.load_checkpoint) == ["model", "optimizer", "scheduler", "checkpoint_path"]
    # direct variant: forward = forward_diffusion + direct_sampling (diffusion_RDUnet_direct.py:203-206)
    assert D.DiffusionModel.forward is not A.DiffusionModel.forward
    assert issubclass(D.DiffusionModel, A.DiffusionModel)


def test_conv_layer_extra_is_a_read_only_view_of_the_typed_state():
    """``ConvLayer.extra`` (read by bench.py, tests and scripts) is built from the typed
    fields: exactly the keys info / splitk / dense3 / dw / gates / side_slab, each
    present only where the layer has that state, and it takes no writes."""
    from vub_image_denoising_amd.engine import ConvLayer, LayerBwd, Slice

    def layer(name):
        return ConvLayer(name, name + ".actv", "c3", 0, 32, 32, 16, 16, Slice("X"), Slice("X", 32), "PRE_" + name)

    fwd = layer("conv_0")            # forward-only engine, nothing planned yet
    assert dict(fwd.extra) == {} and fwd.bwd is None
    assert "dense3" not in fwd.extra and "splitk" not in fwd.extra and "dw" not in fwd.extra
    assert fwd.extra.get("info", {}) == {} and fwd.extra.get("gates") is None
    fwd.info = {"fwd": ("fwd", "conv_0", "some_kernel", 1234, 56)}
    fwd.splitk, fwd.dense3, fwd.dense3_skip = 4, object(), True
    assert set(fwd.extra) == {"info", "splitk", "dense3"}
    assert fwd.extra["info"]["fwd"][3] == 1234 and fwd.extra["splitk"] == 4 and fwd.extra["dense3"] is fwd.dense3

    side, fused = layer("conv_1"), layer("conv_2")   # train engine: side-stream layer, fused finisher
    side.bwd = LayerBwd(1, 1, 4096, 0, [0, 1, 2], [0, 64, 128], side_slab=0, gated_by=fused)
    fused.bwd = LayerBwd(0, 0, 8192, 0, [3, 4, 5], [192, 256, 320], dw=True, gates=side)
    side.info = fused.info = {}
    assert set(side.extra) == {"info", "dw", "side_slab"}    # (gated_by stays engine-internal)
    assert side.extra["dw"] is False and side.extra["side_slab"] == 0
    assert set(fused.extra) == {"info", "dw", "gates"}
    assert fused.extra["dw"] is True and fused.extra["gates"] is side and "side_slab" not in fused.extra
    for L in (fwd, side, fused):
        with pytest.raises(TypeError):
            L.extra["dw"] = True
        with pytest.raises(TypeError):
            del L.extra["info"]
        with pytest.raises(AttributeError):
            L.extra = {}


def test_reduce_entries_share_one_argument_check():
    """The three reduce entries reject a bad job before anything is launched (no GPU
    needed), with the calling entry and the job index in the error text."""
    import ctypes
    from vub_image_denoising_amd import _hip as H
    lib = H.load_library()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16   # 16-byte aligned, never dereferenced
    assert lib.rdn_wgrad_reduce(p, 2, 16, 6, 3, 9, p, 0, None, 0, None, None, None) == -1     # ndim % 4
    assert b"rdn_wgrad_reduce: job 0" in lib.rdn_last_error()
    assert lib.rdn_wgrad_reduce_cols(p, 2, 16, 32, 9, p, 96, 80, 0, None, 0, None, None, None) == -1   # past gstride
    assert b"rdn_wgrad_reduce_cols: job 0" in lib.rdn_last_error()
    good = dict(ws=p, grad=p, splits=2, mdim=16, ndim=8, ndim_real=3, taps=9, gstride=3)
    jobs = (H.ReduceJob * 2)(H.ReduceJob(**good), H.ReduceJob(**{**good, "splits": 0}))
    assert lib.rdn_wgrad_reduce_batch(jobs, 2, None) == -1
    assert b"rdn_wgrad_reduce_batch: job 1" in lib.rdn_last_error()
    assert lib.rdn_wgrad_reduce_batch(jobs, H.REDUCE_BATCH_MAX + 1, None) == -1
    assert b"1..8 jobs" in lib.rdn_last_error()


def test_reduce_jobs_tile_the_layer_gradient():
    """``engine.reduce_jobs`` (the one place with the column-part arithmetic): a plain
    layer is one job over all its slabs; a fused layer in nh column parts is nh jobs whose
    columns [gci0, gci0 + ndim_real) tile [0, ndim_real of the layer) without gap or
    overlap, whose slab pointers advance by sh * mdim * taps * cols floats, of which only
    part 0 carries the dalpha/dbias partials, and which sum sh partial rows when the
    kernel gates in its loader (a row per slab of part 0), else the PReLU pass's rows."""
    from vub_image_denoising_amd.engine import GATE_LOADER, GATE_PRELU, LayerBwd, reduce_jobs

    WS, GBASE, PWS, GOFF = 0x10000, 0x7000000, 0x5000, [256, 8192, 8448]

    def jobs(splits, mdim, ndim, ndim_real, taps, cols, gate, part_rows):
        S = LayerBwd(3, 1, 4096, 0, [0, 1, 2], GOFF, gate=gate, dw=cols < ndim or gate == GATE_LOADER,
                     wgrad=(splits, mdim, ndim, ndim_real, taps), dw_cols=cols, part_rows=part_rows, pws=PWS)
        out = reduce_jobs(S, WS, GBASE)
        for j in out:   # every job writes this layer's three gradients, accumulating
            assert (j.grad, j.dbias, j.dalpha) == (GBASE + GOFF[0], GBASE + GOFF[1], GBASE + GOFF[2])
            assert (j.mdim, j.taps, j.gstride, j.accumulate) == (mdim, taps, ndim_real, 1)
            assert (j.sl, j.blocks, j.pblocks) == (0, 0, 0)   # the library's to fill
        return out

    # plain layers: a side-stream 3x3 with padded columns (PReLU pass: 37 rows), a loader-gated
    # stride-2 one (part_splits 0: as many rows as splits)
    for args, ps in (((12, 16, 8, 3, 9, 8, GATE_PRELU, 37), 37), ((20, 64, 32, 32, 4, 32, GATE_LOADER, 0), 0)):
        (j,) = jobs(*args)
        assert (j.ws, j.part, j.splits, j.ndim, j.ndim_real, j.gci0, j.part_splits) == (WS, PWS, args[0], args[2], args[3], 0, ps)

    # h2 (64 = 2 x 32 columns) and h5 (160 = 5 x 32), loader-gated and pre-gated
    for nh, splits in ((2, 512), (5, 1280)):
        for gate, rows in ((GATE_LOADER, 0), (GATE_PRELU, 41)):
            mdim, cols, taps = 32 if nh == 2 else 64, 32, 9
            out = jobs(splits, mdim, nh * cols, nh * cols, taps, cols, gate, rows)
            sh = splits // nh
            assert len(out) == nh
            assert [(j.gci0, j.gci0 + j.ndim_real) for j in out] == [(h * cols, (h + 1) * cols) for h in range(nh)]
            assert [j.ws for j in out] == [WS + h * sh * mdim * taps * cols * 4 for h in range(nh)]
            assert [j.part for j in out] == [PWS] + [None] * (nh - 1)
            assert all((j.splits, j.ndim, j.ndim_real) == (sh, cols, cols) for j in out)
            assert all(j.part_splits == (sh if gate == GATE_LOADER else rows) for j in out)
