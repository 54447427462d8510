"""GPU: a handle launches the kernels sd_conv_forms lists, and both networks compute bit for bit what tests/golden/conv_net_digests.json holds.

The digests were recorded from the launch path before the per-layer kernel choice moved into csrc/conv_form.cpp (one resolver, one table per
handle): sha256 of the f32 logits and of the raw disparity pair, and the count of fp16-saturated values.  Each case also reads the (layer, kernel)
pairs of its own launches -- the per-layer lines sd_profile_read prints under SEMDEPTH_PROFILE_VERBOSE -- and holds them to Engine.conv_forms.

What pins what: the profile label and the listing are read from the same ConvForm record, so that comparison shows that every listed layer is launched
once (and a split layer reduced), not that the label names the instantiation dispatched -- the launchers index their instantiations by the record's
variant, and only the digests see a wrong one.  Some switches give the digests of the default handle (rowskip and stem on both engines, flat and n16 on
bf16x3: kernels that compute the same bits); their cases pin the listing through tests/golden/conv_forms.json and the launch count here.  The
labels themselves were compared with what the previous launch path printed, layer by layer, when the goldens were recorded.

Coverage (checked on the CPU below): the label families these cases reach include every family of the 512 x 1024 x 32 default listings of all six
precisions except the two that need the full size:
    conv_dma block 5 (256 x 256, "<2,4,4,2>"): its rule asks for 512 tiles of a full pass;
    conv_split 128 x 256 ("conv_split*<2,4,2,2>"): 512 tiles of the call."""
import hashlib
import json
import os
import tempfile

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
import conv_forms_cases as cc
from semantic_depth_amd import _lib as L
from semantic_depth_amd import weights as Wt

DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_net_digests.json")
DISABLE = ["dma", "dma3", "flat", "rowskip", "stem", "direct", "fold", "n16", "tail1"]
NEEDS_FULL_SIZE = ("<2,4,4,2>", "conv_split_kernel<2,4,2,2", "conv_split_x3_kernel<2,4,2,2>", "conv_split_f16w_kernel<2,4,2,2>")


def cases():
    """(encoder, precision, H, W, max_batch, small-batch level, SEMDEPTH_DISABLE name or None, frames of the call)"""
    out = [("resnet50", p, 256, 512, 8, 0, None, 8) for p in cc.PRECISIONS]
    out += [("vgg", p, 256, 512, 8, 0, None, 8) for p in ("bf16x3", "f16x2", "bf16x2", "mixed")]      # (the last two: conv_dma's 256 x 32 block of enc/conv1b)
    out += [("resnet50", "f16x2", 128, 256, 1, level, None, 1) for level in (0, 1, 2)]
    out += [("resnet50", p, 256, 512, 8, 0, sw, 8) for p in ("bf16x3", "f16x2") for sw in DISABLE]
    out += [("resnet50", p, 256, 512, 8, 0, None, 3) for p in ("bf16x3", "f16x2")]          # the call-dependent path: 3 frames on a handle of 8
    return out


def case_id(case):
    enc, prec, H, W, B, level, sw, frames = case
    return f"{enc}-{prec}-{H}x{W}x{B}-sb{level}-{sw or 'default'}-frames{frames}"


_weights = {}


def weights(name):
    if name not in _weights:
        _weights[name] = Wt.make_fcn8s_weights(1, decoder_std=0.05) if name == "fcn8s" else Wt.make_monodepth_weights(name, 2)
    return _weights[name]


class stderr_lines:
    """the lines the library writes to file descriptor 2 inside the block"""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.lines = self.tmp.read().decode(errors="replace").splitlines()
        self.tmp.close()


def launched(lines):
    """{(layer, kernel)} of the [sd_profile] lines"""
    return {(ln.split()[1], ln.split("TF/s", 1)[1].strip()) for ln in lines if ln.startswith("[sd_profile]")}


def run_case(case):
    """{"logits", "disp_raw": sha256, "fp16_saturated_values", "launched": {net: pairs}, "forms": {net: listing}} of one case"""
    from semantic_depth_amd.engine import Engine
    enc, prec, H, W, B, level, sw, frames = case
    old = {k: os.environ.get(k) for k in ("SEMDEPTH_DISABLE", "SEMDEPTH_PROFILE_VERBOSE")}
    os.environ["SEMDEPTH_PROFILE_VERBOSE"] = "1"
    os.environ.pop("SEMDEPTH_DISABLE", None)
    if sw:
        os.environ["SEMDEPTH_DISABLE"] = sw
    try:
        eng = Engine(H, W, B, enc, precision=prec, small_batch=level)        # (both variables are latched here)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    eng.load_weights(L.SD_NET_FCN8S, weights("fcn8s"))
    eng.load_weights(L.SD_NET_MONODEPTH, weights(enc))
    fr = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (frames, H, W, 3), dtype=np.uint8)).cuda()
    out = {"launched": {}, "forms": {}}
    eng.profile(True)
    for net, nid in cc.NETS.items():
        if net == "fcn8s":
            out["logits"] = hashlib.sha256(eng.fcn8s_forward(fr, want_logits=True)["logits"].cpu().numpy().tobytes()).hexdigest()
        else:
            out["disp_raw"] = hashlib.sha256(eng.monodepth_forward(fr, want_raw=True)[1].cpu().numpy().tobytes()).hexdigest()
        with stderr_lines() as err:
            eng.profile_read()
        out["launched"][net] = launched(err.lines)
        out["forms"][net] = eng.conv_forms(nid, frames)
    eng.profile(False)
    out["fp16_saturated_values"] = eng.saturation_count()
    eng.close()
    return out


def expected_launches(forms):
    """the (layer, kernel) pairs of a listing: a split layer's reduce launch follows its GEMM / direct launch"""
    out = set()
    for name, form in forms.items():
        out |= {(name, k) for k in L.conv_launches(*form)}
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_a_handle_launches_what_it_lists_and_computes_what_it_did(case):
    with open(DIGESTS) as f:
        want = json.load(f)[case_id(case)]
    got = run_case(case)
    for net in cc.NETS:
        assert got["launched"][net] == expected_launches(got["forms"][net]), net
    assert {k: got[k] for k in want} == want


def family(label):
    return label.split(" x")[0]


def test_the_gpu_cases_reach_every_family_of_the_full_size_listings():
    """CPU, from the listing: every label of the default 512 x 1024 x 32 handles (all six precisions, both encoders) is launched by a case above,
    except those that need the full size (NEEDS_FULL_SIZE)."""
    graft.build()
    lib = L.load()
    reached = set()
    for enc, prec, H, W, B, level, sw, frames in cases():
        with cc.handle(lib, (enc, prec, H, W, B, level, sw)) as h:
            for nid in cc.NETS.values():
                reached |= {family(cc.keyed(*f)) for f in L.conv_forms(lib, h, nid, frames).values()}
    missing = set()
    for enc in cc.ENCODERS:
        for prec in cc.PRECISIONS:
            with cc.handle(lib, (enc, prec, 512, 1024, 32, 0, None)) as h:
                for nid in cc.NETS.values():
                    missing |= {lab for lab, _ in L.conv_forms(lib, h, nid, 0).values()} - reached
    left = {m for m in missing if not any(s in m for s in NEEDS_FULL_SIZE)}
    assert not left, sorted(left)
