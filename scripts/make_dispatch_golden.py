#!/usr/bin/env python3
"""Host dispatch of the conv launchers over two descriptor grids, without a GPU.

The probes (rdn_wgrad_kernel_name / rdn_conv_kernel_name) run the launchers' whole
decision on fake, 16-byte aligned pointers and return the kernel instantiation they
would launch.  `sweep_wgrad()` / `sweep_fwd()` yield one record per descriptor;
`summarise()` turns a sweep into what tests/golden/dispatch.json holds per grid: the
map kernel name -> number of descriptors and a SHA-256 of the canonical dump of every
(descriptor key, return code, name, splits, chunks).  tests/test_dispatch_cpu.py
imports the sweeps from here.

Writing the golden (only when a dispatch decision is MEANT to move): build the library
from the commit whose answers are to be recorded, set no RDN_* variable, and run

    python scripts/make_dispatch_golden.py --lib path/to/librdunet_hip.so

The one textual rule applied to the recorded names: `wgrad_kernel<T,BM,BN,WMW,gather>`
is written without its last field (the kernel lost that template parameter; the
recorded library still printed it).  Values that depend on the CU count are those of a
256-CU device (what a failed device query counts as).
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

GOLDEN = os.path.join(REPO, "tests", "golden", "dispatch.json")

SHAPES_WGRAD = [(1, 8, 16), (1, 13, 21), (16, 32, 32), (2, 64, 64), (16, 256, 256)]
MDIMS = [3, 8, 16, 24, 32, 48, 64, 96, 128, 160, 256, 512]
NDIMS = list(range(8, 321, 8)) + [384, 512, 640, 1024]
SHAPES_FWD = SHAPES_WGRAD + [(16, 128, 128), (1, 256, 256)]
CINS = [8, 16, 24, 32, 48, 64, 80, 96, 128, 160, 192, 256, 320, 384, 512, 640]
NCOLS = [3, 8, 16, 24, 32, 48, 64, 80, 96, 112, 128, 160, 192, 256, 320, 512, 640]

_OLD_WGRAD = re.compile(r"^(wgrad_kernel<\w+,\d+,\d+,\d+),\d+>$")


def canonical_name(name):
    """The one rename between the recorded library and this tree (see the module text)."""
    return _OLD_WGRAD.sub(r"\1>", name)


def _up(v, m):
    return (v + m - 1) // m * m


def sweep_wgrad(lib, H):
    """(key, rc, name, splits, chunks) of every weight-gradient descriptor of the grid."""
    buf = C.create_string_buffer(128)
    for dtype in (H.RDN_BF16, H.RDN_F32):
        for gather in (H.RDN_G_CONV3, H.RDN_G_S2):
            up = 2 if gather == H.RDN_G_S2 else 1
            for n, h, w in SHAPES_WGRAD:
                for mdim in MDIMS:
                    for ndim in NDIMS:
                        for gate in (0, 1):
                            d = H.WgradDesc()
                            d.dtype, d.gather = dtype, gather
                            d.n, d.h, d.w, d.hin, d.win = n, h, w, up * h, up * w
                            d.a, d.b, d.ws = 1 << 20, 2 << 20, 3 << 20
                            d.mdim, d.ndim = mdim, ndim
                            d.a_ps, d.b_ps = _up(mdim, 8), ndim
                            if gate:
                                d.a_gate, d.a_gate_alpha, d.part = 4 << 20, 5 << 20, 6 << 20
                                d.a_gate_ps = d.a_ps
                            rc = lib.rdn_wgrad_kernel_name(C.byref(d), buf, 128)
                            key = f"w:{dtype}:{gather}:{n}x{h}x{w}:{mdim}:{ndim}:{gate}"
                            yield (key, rc, canonical_name(buf.value.decode()), lib.rdn_wgrad_splits(C.byref(d)),
                                   lib.rdn_wgrad_chunks(C.byref(d)))


def sweep_fwd(lib, H):
    """(key, rc, name, "", "") of every forward / input-gradient descriptor of the grid."""
    buf = C.create_string_buffer(128)
    epi = H.EPI_BIAS | H.EPI_PRELU | H.EPI_STORE_PRE
    for dtype in (H.RDN_BF16, H.RDN_F32):
        for gather, taps in ((H.RDN_G_CONV3, 9), (H.RDN_G_S2, 4), (H.RDN_G_PIX, 1)):
            up = 2 if gather == H.RDN_G_S2 else 1
            for n, h, w in SHAPES_FWD:
                for cin in CINS:
                    kp = lib.rdn_conv3_packed_k(cin, dtype) if gather == H.RDN_G_CONV3 else _up(taps * cin, 64)
                    for ncols in NCOLS:
                        for gate in ((0, 1) if gather == H.RDN_G_CONV3 else (0,)):
                            for flags in (0, epi):
                                d = H.ConvDesc()
                                d.dtype, d.gather, d.flags = dtype, gather, flags
                                d.n, d.h, d.w, d.hin, d.win = n, h, w, up * h, up * w
                                d.cin, d.kp, d.ncols, d.cout = cin, kp, ncols, ncols
                                d.x, d.wp, d.out = 1 << 20, 2 << 20, 3 << 20
                                d.x_ps, d.out_ps = cin, _up(ncols, 8)
                                if flags:
                                    d.bias, d.alpha, d.pre = 4 << 20, 5 << 20, 6 << 20
                                    d.pre_ps = d.out_ps
                                if gate:
                                    d.gate, d.gate_alpha, d.gate_ps = 7 << 20, 8 << 20, cin
                                rc = lib.rdn_conv_kernel_name(C.byref(d), buf, 128)
                                key = f"f:{dtype}:{gather}:{n}x{h}x{w}:{cin}:{ncols}:{gate}:{flags}"
                                yield (key, rc, canonical_name(buf.value.decode()), "", "")


def summarise(records):
    names, sha, n = {}, hashlib.sha256(), 0
    for rec in records:
        n += 1
        label = rec[2] if rec[1] == 0 else f"(rc {rec[1]})"
        names[label] = names.get(label, 0) + 1
        sha.update(("|".join(str(v) for v in rec) + "\n").encode())
    return {"descriptors": n, "names": dict(sorted(names.items())), "sha256": sha.hexdigest()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", required=True, help="librdunet_hip.so built from the commit to record")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    knobs = sorted(k for k in os.environ if k.startswith("RDN_"))
    if knobs:
        sys.exit(f"unset {', '.join(knobs)}: the golden records the default dispatch")
    from vub_image_denoising_amd import _hip as H
    lib = H.load_library(os.path.abspath(a.lib))
    out = {"wgrad": summarise(sweep_wgrad(lib, H)), "fwd": summarise(sweep_fwd(lib, H))}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for grid, s in out.items():
        print(f"{grid}: {s['descriptors']} descriptors, {len(s['names'])} names, sha256 {s['sha256'][:16]}")


if __name__ == "__main__":
    main()
