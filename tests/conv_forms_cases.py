"""The configurations of tests/golden/conv_forms.json and how a listing is taken for one of them (no GPU: a handle plans on the host).

A configuration is (encoder, precision, H, W, max_batch, small-batch level, SEMDEPTH_DISABLE name or None).  Its golden entry is
``{net: {label: [layers]}}`` for a full pass -- the layers grouped by the verbose label sd_conv_forms gives them, ``label xS`` for a layer split into
S slices --, ``"frames=1": {net: {layer: label}}`` with the layers whose label differs in a call of one frame, and ``"workspace"``: the workspace
bytes of sd_query_memory.  The FCN listing does not depend on the encoder and is kept under resnet50 only."""
import ctypes as C
import json
import os

from semantic_depth_amd import _lib as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_forms.json")
PRECISIONS = {"f32": L.SD_PREC_F32, "bf16x2": L.SD_PREC_BF16X2, "mixed": L.SD_PREC_MIXED, "plan": L.SD_PREC_PLAN, "bf16x3": L.SD_PREC_BF16X3,
              "f16x2": L.SD_PREC_F16X2}
ENCODERS = {"vgg": L.SD_ENC_VGG, "resnet50": L.SD_ENC_RESNET50}
NETS = {"fcn8s": L.SD_NET_FCN8S, "monodepth": L.SD_NET_MONODEPTH}
GEOMETRIES = [(128, 256, 1), (256, 512, 8), (512, 1024, 32), (384, 1280, 4)]        # (the last: not a power of two; monodepth-vgg needs multiples of 128)
# every switch name plan.cpp knows (sd_create refuses any other)
SWITCHES = ["dma", "dma3", "direct", "stem", "fold", "tail1", "pool_fuse", "planar", "n16", "fuse1", "fuse4", "flat", "rowskip", "dma_big", "mfma16", "png_waves"]


def configurations():
    out = []
    for enc in ENCODERS:
        for prec in PRECISIONS:
            for H, W, B in GEOMETRIES:
                out.append((enc, prec, H, W, B, 0, None))
        for H, W, _ in GEOMETRIES:          # small-batch handles of one frame (the rules read cus = 256 where no device answers)
            for level in (1, 2):
                out.append((enc, "f16x2", H, W, 1, level, None))
    for prec in ("bf16x3", "f16x2"):
        for sw in SWITCHES:
            out.append(("resnet50", prec, 256, 512, 8, 0, sw))
    return out


def key(cfg):
    enc, prec, H, W, B, level, sw = cfg
    return f"{enc} {prec} {H}x{W}x{B} small_batch={level} disable={sw or '-'}"


class handle:
    """a planning handle of a configuration: ``with handle(lib, cfg) as h``"""

    def __init__(self, lib, cfg):
        self.lib, self.cfg = lib, cfg

    def __enter__(self):
        enc, prec, H, W, B, level, sw = self.cfg
        old = os.environ.get("SEMDEPTH_DISABLE")
        if sw:
            os.environ["SEMDEPTH_DISABLE"] = sw
        else:
            os.environ.pop("SEMDEPTH_DISABLE", None)
        try:
            self.h = C.c_void_p()
            assert self.lib.sd_create(C.byref(self.h), 0, H, W, B, ENCODERS[enc], PRECISIONS[prec]) == 0, self.cfg
        finally:
            if old is None:
                os.environ.pop("SEMDEPTH_DISABLE", None)
            else:
                os.environ["SEMDEPTH_DISABLE"] = old
        if level:
            assert self.lib.sd_set_small_batch(self.h, level) == 0, self.cfg
        return self.h

    def __exit__(self, *exc):
        self.lib.sd_destroy(self.h)


def keyed(label, slices):
    return label if slices == 1 else f"{label} x{slices}"


def grouped(forms):
    """{label or 'label xS': [layers]} of a {layer: (label, slices)} listing"""
    out = {}
    for name, form in forms.items():
        out.setdefault(keyed(*form), []).append(name)
    return out


def workspace(lib, h):
    ws = C.c_size_t()
    assert lib.sd_query_memory(h, None, None, C.byref(ws)) == 0
    return ws.value


def entry(lib, cfg):
    """the golden entry of one configuration, taken from the library"""
    out = {}
    with handle(lib, cfg) as h:
        for net in NETS:
            if net == "fcn8s" and cfg[0] != "resnet50":
                continue
            full, one = L.conv_forms(lib, h, NETS[net], 0), L.conv_forms(lib, h, NETS[net], 1)
            assert list(full) == list(one)
            out[net] = grouped(full)
            out.setdefault("frames=1", {})[net] = {k: keyed(*one[k]) for k in full if one[k] != full[k]}
        out["workspace"] = workspace(lib, h)
    return out


def golden():
    with open(GOLDEN) as f:
        return json.load(f)
