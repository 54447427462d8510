#!/usr/bin/env python3
"""which kernel runs every conv layer of a handle, without a GPU (sd_conv_forms; the rules are in csrc/conv_form.cpp).
usage: python scripts/list_forms.py H W B encoder precision [small_batch] [--frames N]
       encoder: vgg | resnet50; precision: f32 | bf16x2 | mixed | plan | bf16x3 | f16x2; small_batch: 0 | 1 | 2 (f16x2 only)
SEMDEPTH_DISABLE=name,... is honoured as everywhere (latched when the handle is made)."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402
from semantic_depth_amd import _lib as L  # noqa: E402

PRECISIONS = {"f32": L.SD_PREC_F32, "bf16x2": L.SD_PREC_BF16X2, "mixed": L.SD_PREC_MIXED, "plan": L.SD_PREC_PLAN, "bf16x3": L.SD_PREC_BF16X3,
              "f16x2": L.SD_PREC_F16X2}


def main(argv):
    frames = 0
    if "--frames" in argv:
        i = argv.index("--frames")
        frames = int(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
    if len(argv) not in (5, 6) or argv[3] not in ("vgg", "resnet50") or argv[4] not in PRECISIONS:
        sys.exit(__doc__)
    H, W, B = (int(a) for a in argv[:3])
    graft.build()
    lib = L.load()
    h = C.c_void_p()
    st = lib.sd_create(C.byref(h), 0, H, W, B, L.SD_ENC_VGG if argv[3] == "vgg" else L.SD_ENC_RESNET50, PRECISIONS[argv[4]])
    if st != L.SD_OK:
        sys.exit(f"sd_create: {lib.sd_status_string(st).decode()}")
    if len(argv) == 6 and int(argv[5]):
        L.check(lib, h, lib.sd_set_small_batch(h, int(argv[5])), "sd_set_small_batch")
    for name, net in (("fcn8s", L.SD_NET_FCN8S), ("monodepth", L.SD_NET_MONODEPTH)):
        print(f"# {name}, {frames or 'a full pass of ' + str(lib.sd_pass_frames(h))} frame(s)")
        for layer, (label, slices) in L.conv_forms(lib, h, net, frames).items():
            print(f"{layer:28s} {label}" + (f"  x{slices} + reduce" if slices > 1 else ""))
    lib.sd_destroy(h)


if __name__ == "__main__":
    main(sys.argv[1:])
