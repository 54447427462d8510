"""Every layer of both networks ALONE against a float64 reference (oracle/layers.py): one forward under SEMDEPTH_KEEP_ACTIVATIONS=1, then, layer
by layer, the GPU's own stored input tensor(s) through the float64 layer on the CPU against the GPU's stored output, held to the per-element
bound of oracle/layers.py (derived from the formats, not fitted).  Upstream error never enters: what is compared is one kernel's arithmetic,
addressing and output rounding.

    python scripts/layer_check.py > profiles/layer_check_worst_ratios.txt

writes one line per (engine, geometry, kernel label): the worst |delta| / bound, the layer it occurred in and the output maps (height x width) the
label ran on, and one comment line per case with its seconds.  tests/test_gpu_layers.py imports CASES / run_case() from here and asserts what this
prints (but for the seconds: a case at a size that is no power of two may not take longer than the slowest 256 x 512 case of 8 frames, and since
seconds compare within one run only, main() here checks that over its own run and a pytest run of single cases does not).  Beside the power-of-two frame sizes the cases hold 192 x 256, 320 x 192 and 384 x 128 (vgg), a pass fed 3 frames on a handle of 4 and the
small-batch forms at 192 x 256, and fc6 / fc7 alone at 192 x 1024 with 16 frames (_odd_cases): partial row tiles behind full ones, maps 3 and 5 pixels high or wide, GEMMs whose M is no multiple of 256.
Such a case names in need_at the kernel and the map extent it is there for, and fails where the planner routed the layer elsewhere.

Reading a failure: "<layer> [<kernel label>] image i, y, x, channel c: |delta| / bound = r" names the layer, the kernel the handle records for it
(the label of Engine.conv_forms / SEMDEPTH_PROFILE_VERBOSE) and the worst element.  r <= 1 passes.  A ratio of a few units on many layers of one engine points at a format
term of the bound (oracle/layers.py SCHEMES / OUT_FORMATS); hundreds and more on one layer, at an edge pixel, the last image or one channel group, is a
kernel, a weight relayout or a planner bug -- see tests/test_layer_check_cpu.py for what each kind of mistake looks like."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

KEEP = "SEMDEPTH_KEEP_ACTIVATIONS"
FC_CHANNELS = np.r_[0:64, 2016:2080, 4032:4096]      # fc6 / fc7 at full size: the first 64, 64 across the tile boundary at 2048, the last 64


# predicates on the output extent (map height, map width) of a checked group, by name (need_at below)
EXTENT = {
    # full 16-row tiles and then a partial one (TH = 16 of conv_direct.hip, T3_TH of conv_direct3.hip)
    "partial row tile after full ones": lambda h, w: h > 16 and h % 16 != 0,
    # an upconv's output is twice its source
    "source 3, 5 or 6 rows high": lambda h, w: h in (6, 10, 12),
    "3 or 5 rows or columns": lambda h, w: h in (3, 5) or w in (3, 5),
    "6 rows": lambda h, w: h == 6,
}


def case(net, precision, H, W, frames, max_batch=None, small_batch=0, images="all", only=None, need=(), need_at=()):
    """net: 'fcn8s' | 'resnet50' | 'vgg'.  images: 'all' or 'ends' (first and last frame's images).  only: check these layers alone (fc6 / fc7 at full
    size).  need: kernel-label prefixes that must have run (a silently rerouted layer must not make the case pass).  need_at: ((kernel-label
    prefix, layer-name prefix, name of an EXTENT predicate), ...): a checked layer of that name, run by that kernel, must have an output map the
    predicate holds for -- the proof that the case met the tile edge it is there for."""
    assert all(e in EXTENT for _, _, e in need_at)
    return dict(net=net, precision=precision, H=H, W=W, frames=frames, max_batch=max_batch or frames, small_batch=small_batch, images=images,
                only=only, need=tuple(need), need_at=tuple(need_at))


def case_id(c):
    s = f"{c['net']}-{c['precision']}-{c['H']}x{c['W']}-B{c['frames']}of{c['max_batch']}"
    if c["small_batch"]:
        s += f"-small{c['small_batch']}"
    if c["only"]:
        s += "-" + "+".join(c["only"])
    return s


def _cases():
    out = []
    for p in ("f32", "bf16x3", "f16x2", "bf16x2", "plan"):
        out.append(case("fcn8s", p, 64, 128, 2))
    for p in ("f32", "bf16x3", "f16x2", "bf16x2", "plan", "mixed"):
        out.append(case("resnet50", p, 64, 128, 2))
    for p in ("f16x2", "bf16x3"):
        out.append(case("vgg", p, 128, 128, 1))
        out.append(case("resnet50", p, 64, 448, 1))      # the inward-shifted last tile column
        out.append(case("resnet50", p, 64, 64, 1))       # three overlapping tile columns
    # routing geometry: 256 x 512, an engine of 8 frames, all 8 fed; the float64 side for the first and the last frame's images
    # (the families each case claims: the stem kernels, the direct kernel in its 64-channel passes of 128 .. 512-channel layers, the LDS-DMA and phased
    # 256 x 256 GEMM blocks with their precomputed gathers <1> / <2>, the folded upconvs, the one-launch decoder tail)
    fam = {("fcn8s", "bf16x3"): ("conv_stem_x3_kernel", "conv_direct_x3_kernel<2,2>", "conv_dma_x3_kernel"),
           ("fcn8s", "f16x2"): ("conv_stem_hs_kernel", "conv_direct_hs_kernel<2,2>", "conv_dma_hs_kernel"),
           ("fcn8s", "plan"): ("conv_stem_kernel", "conv_direct_kernel<2,2>", "conv_direct_f16w_kernel", "conv_direct_f16w_x2_kernel", "conv_direct_f16x1_kernel",
                               "conv_dma_f16x1_kernel"),
           ("resnet50", "bf16x3"): ("conv_stem_x3_kernel", "conv_dma3_kernel<1>", "conv_dma3_kernel<2>", "conv_dma_x3_kernel", "conv_split_x3_kernel",
                                    "conv_direct_x3_kernel<2,2>", "conv_direct_x3_fold_kernel", "dec_tail1_x3_kernel"),
           ("resnet50", "f16x2"): ("conv_stem_hs_kernel", "conv_dma_hs_phased_kernel<1>", "conv_dma_hs_kernel", "conv_split_hs_kernel", "conv_direct_hs_kernel<2,2>",
                                   "conv_direct_hs_kernel<1,n16>", "conv_direct_hs_fold_kernel", "dec_tail1_hs_kernel"),
           ("resnet50", "plan"): ("conv_stem_f16w_kernel", "conv_dma_f16x1_kernel", "conv_split_f16w_kernel", "conv_direct_f16x1_kernel",
                                  "conv_direct_f16w_kernel<1,n16>")}
    for n in ("fcn8s", "resnet50"):
        for p in ("f16x2", "bf16x3", "plan"):
            out.append(case(n, p, 256, 512, 8, images="ends", need=fam[(n, p)]))
    # the 256 x 256 block of the LDS-DMA kernel runs on the three-product bf16 engine at this size (test_gpu_nets.py)
    out.append(case("resnet50", "bf16x2", 256, 512, 8, images="ends", need=("conv_dma_kernel<2,4,4,2>", "conv_stem_kernel", "conv_direct_kernel<2,2>")))
    # the small-batch forms (f16x2 handles only: sd_set_small_batch refuses the others): split-K GEMM layers, level 2 also the split direct layers
    for n in ("fcn8s", "resnet50"):
        out.append(case(n, "f16x2", 256, 512, 1, small_batch=1, need=("conv_splitk_hs_kernel", "splitk_reduce_kernel")))
        out.append(case(n, "f16x2", 256, 512, 1, small_batch=2, need=("conv_splitk_hs_kernel", "conv_direct_splitc_hs_kernel", "splitc_reduce_kernel")))
    # fc6 / fc7 alone at full size: the row-grouped, tap-skipping form of the phased GEMM block
    out.append(case("fcn8s", "bf16x3", 512, 1024, 8, images="ends", only=("fc6", "fc7"), need=("conv_dma3_kernel<2>", "conv_dma3_kernel<1>")))
    out.append(case("fcn8s", "f16x2", 512, 1024, 8, images="ends", only=("fc6", "fc7"), need=("conv_dma_hs_phased_kernel<2>", "conv_dma_hs_phased_kernel<1>")))
    return out + _odd_cases()


# Frame sizes that are no power of two (every case above has map heights 2^n: a 16-row tile covers a whole map or an exact number of tiles).
#   192 x 256  maps 96x128, 48x64, 24x32, 12x16, 6x8, 3x4: the widths 128 / 64 / 32 keep the 3x3 layers on the direct kernels, the 24-row maps are one
#              full row tile and a partial one (res3_x/conv2, iconv4, conv4_x and conv3_3 with its fused pool), the folded upconvs
#              read 3- and 6-row sources (upconv6 / upconv5), fc6 runs on 6x8
#   320 x 192  maps 160x96 .. 5x3: three tile columns at 96, the generic and GEMM routes below with M no multiple of 256, fc6 on 10x6, the
#              deconv heads on one tile and a half
#   384 x 128  vgg: the 3x1 deepest map and the folded upconv7 on it; the 24 / 12 / 6-row maps are 8 / 4 / 2 wide, so the GEMM routes run them (the
#              direct kernel needs a width that is a multiple of 32 and stays on 192x64 and 96x32)
_PART, _SRC = "partial row tile after full ones", "source 3, 5 or 6 rows high"
# Per split engine, the kernel labels of the MI355X run behind profiles/layer_check_worst_ratios.txt:
#   stem      the stem kernel
#   direct    the direct 3x3 kernel that must have met a 24-row map
#   upfold    monodepth: the kernel of the folded upconv6 / upconv5 (the GEMM-block form; the folded form of the DIRECT kernel starts at upconv4 on bf16x3)
#   pool4     FCN-8s: the kernel of conv4_3 with its fused 2x2 pool, over the 24-row map
_EDGE = {("resnet50", "bf16x3"): dict(stem="conv_stem_x3_kernel", direct="conv_direct_x3_kernel<2,2>", upfold="conv_dma3_kernel<2>"),
         ("resnet50", "f16x2"): dict(stem="conv_stem_hs_kernel", direct="conv_direct_hs_kernel<2,2>", upfold="conv_dma_hs_kernel<2,4,2,2>"),
         ("resnet50", "bf16x2"): dict(stem="conv_stem_kernel", direct="conv_direct_kernel<2,2>", upfold="conv_dma_kernel<2,4,2,2>"),
         ("resnet50", "plan"): dict(stem="conv_stem_f16w_kernel", direct="conv_direct_f16x1_kernel<2,2>", upfold="conv_dma_f16x1_kernel<2,4,2,2>"),
         ("resnet50", "mixed"): dict(stem="conv_stem_f16w_kernel", direct="conv_direct_f16w_kernel<2,2>", upfold="conv_dma_f16w_kernel<2,4,2,2>"),
         ("fcn8s", "bf16x3"): dict(stem="conv_stem_x3_kernel", direct="conv_direct_x3_kernel<2,2>", pool4="conv_direct_x3_kernel<2,2>"),
         ("fcn8s", "f16x2"): dict(stem="conv_stem_hs_kernel", direct="conv_direct_hs_kernel<2,2>", pool4="conv_direct_hs_kernel<2,2>"),
         ("fcn8s", "bf16x2"): dict(stem="conv_stem_kernel", direct="conv_direct_kernel<2,2>", pool4="conv_direct_kernel<2,2>"),
         ("fcn8s", "plan"): dict(stem="conv_stem_kernel", direct="conv_direct_f16w_x2_kernel<2,2>", pool4="conv_direct_f16x1_kernel<2,2>")}


def _odd_cases():
    out = []

    def edge(n, p, splitc=None):
        """need / need_at of a 192 x 256 case.  splitc: the label that runs the 24-row direct layers instead (small-batch level 2)"""
        if p == "f32":          # (one kernel, conv_igemm, for every layer: nothing to be rerouted)
            return dict(need=(), need_at=())
        e = _EDGE[(n, p)]
        direct = splitc or e["direct"]
        at = [(direct, "", _PART)]
        if n == "resnet50":     # res3_x/conv2 and iconv4 are the 24-row direct layers; upconv6 / upconv5 read the 3x4 and the 6x8 map
            at += [(e["upfold"], "dec/upconv6", _SRC), (e["upfold"], "dec/upconv5", _SRC)]
            if p == "bf16x3":   # (128 outputs: the folded form of the DIRECT kernel, on a 24-row output)
                at += [("conv_direct_x3_fold_kernel", "dec/upconv4", _PART)]
        else:
            at += [(splitc or e["pool4"], "conv4_3+pool4", _PART)]
        return dict(need=(e["stem"], direct), need_at=tuple(at))

    for n in ("resnet50", "fcn8s"):
        for p in ("f32", "bf16x3", "f16x2", "bf16x2", "plan") + (("mixed",) if n == "resnet50" else ()):
            out.append(case(n, p, 192, 256, 1, **edge(n, p)))
        for p in ("f32", "bf16x3", "f16x2", "plan"):      # (any kernel: the 96- and 24-wide maps leave the direct kernels; res5 is 5x3)
            out.append(case(n, p, 320, 192, 1, need_at=(("", "enc/res5_3/conv3", "3 or 5 rows or columns"),) if n == "resnet50" else ()))
    for p in ("f16x2", "bf16x3"):
        out.append(case("vgg", p, 384, 128, 1, need_at=(("", "enc/conv7b", "3 or 5 rows or columns"),
                                                        (_EDGE[("resnet50", p)]["upfold"], "dec/upconv7", _SRC))))
    # a pass fed 3 frames on a handle of 4.  run_case first runs a full pass of 4 OTHER frames on the handle, so that the slots behind the fed
    # images hold another image's activations and not the zeros of a fresh arena (zeros are what a padding row holds anyway: a kernel that counts
    # the handle's images as real would pass on them); only the fed images are read back and compared
    for n in ("resnet50", "fcn8s"):
        for p in ("f16x2", "bf16x3"):
            out.append(case(n, p, 192, 256, 3, max_batch=4, **edge(n, p)))
    # the small-batch forms, whose partial last row tile had only run at 256 x 512 ("Rows of a partial last tile are not stored")
    for n in ("fcn8s", "resnet50"):
        e = edge(n, "f16x2")
        out.append(case(n, "f16x2", 192, 256, 1, small_batch=1, need=e["need"] + ("conv_splitk_hs_kernel", "splitk_reduce_kernel"), need_at=e["need_at"]))
        e = edge(n, "f16x2", splitc="conv_direct_splitc_hs_kernel")      # level 2 runs the 24-row direct layers split along their chunk axis
        out.append(case(n, "f16x2", 192, 256, 1, small_batch=2, need=e["need"] + ("conv_splitk_hs_kernel", "splitc_reduce_kernel"), need_at=e["need_at"]))
    # fc6 on a 6-row map in its row-grouped, tap-skipping form (at 192 x 256 and 320 x 192 fc6 / fc7 are too small for the phased GEMM block and run on
    # conv_split_* / conv_splitk: the block wants 128 tiles of a full pass, a row group 256 / Wout images).  192 x 1024 with 16 frames: the 6 x 32 map,
    # two groups of 8 images per output row, every output row within reach of a padding row of the 7 x 7 taps
    out.append(case("fcn8s", "bf16x3", 192, 1024, 16, images="ends", only=("fc6", "fc7"), need=("conv_dma3_kernel<2>", "conv_dma3_kernel<1>"),
                    need_at=(("conv_dma3_kernel<2>", "fc6", "6 rows"),)))
    out.append(case("fcn8s", "f16x2", 192, 1024, 16, images="ends", only=("fc6", "fc7"), need=("conv_dma_hs_phased_kernel<2>", "conv_dma_hs_phased_kernel<1>"),
                    need_at=(("conv_dma_hs_phased_kernel<2>", "fc6", "6 rows"),)))
    return out


CASES = _cases()


_weights = {}


def _frames(B, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def run_case(c, log=None):
    """-> dict(rows=[(group name, kernel label, oracle.layers.Worst)], extents=[(group name, kernel label, (output map height, width))] (of a
    conv with its fused 2x2 pool: the map the conv runs on, twice the stored one),
    uncovered=[op names], labels={op: label}, missing=[needed families that did not run], unmet=[need_at requirements no checked layer met],
    seconds).  Sets (and restores) the environment switch an engine latches when it is created."""
    from oracle import layers as LY
    from semantic_depth_amd import _lib as L, weights as Wt
    from semantic_depth_amd.engine import Engine
    t0 = time.time()
    fcn = c["net"] == "fcn8s"
    net_id = L.SD_NET_FCN8S if fcn else L.SD_NET_MONODEPTH
    enc = "resnet50" if fcn else c["net"]
    H, W, B = c["H"], c["W"], c["frames"]
    saved = {k: os.environ.get(k) for k in (KEEP,)}
    os.environ[KEEP] = "1"
    try:
        eng = Engine(H, W, c["max_batch"], enc, precision=c["precision"], small_batch=c["small_batch"])
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    if c["net"] not in _weights:          # seeded weights with non-zero biases, made once per network
        _weights[c["net"]] = (Wt.make_fcn8s_weights(1, decoder_std=0.05, bias_std=0.1) if fcn else
                              Wt.make_monodepth_weights(enc, 2, gain=1.5 if enc == "vgg" else 1.0, bias_std=0.05))
    w = _weights[c["net"]]
    layers = LY.fcn8s_layers() if fcn else LY.monodepth_layers(enc)
    eng.load_weights(net_id, w)
    fr = _frames(B, H, W, seed=H + W + B)
    assert all(not np.array_equal(fr[i], fr[j]) for i in range(B) for j in range(i))      # (a mixed-up image must show)
    dev = torch.from_numpy(fr).cuda()
    if c["max_batch"] > B:
        # a partial pass: an earlier FULL pass of other frames leaves its activations in every image slot of every tensor (each has memory of its
        # own under KEEP), those behind the B fed images included
        other = _frames(c["max_batch"], H, W, seed=H + W + B + 1)
        assert all(not np.array_equal(o, f) for o in other for f in fr)
        other = torch.from_numpy(other).cuda()
        eng.fcn8s_forward(other) if fcn else eng.monodepth_forward(other)
        stale = eng.net_tensor(net_id, "conv1_1" if fcn else "enc/conv1")      # (that pass's last image is there to be read behind the fed ones)
        assert stale.shape[0] == (1 if fcn else 2) * c["max_batch"] and float(stale[-1].abs().max()) > 0
    logits = None
    if fcn:
        logits = eng.fcn8s_forward(dev, want_logits=True)["logits"]
    else:
        eng.monodepth_forward(dev, want_raw=True)
    # the kernel of each conv layer of this call: the handle's own record (Engine.conv_forms), which run_plan launches from
    labels = {op: " + ".join(L.conv_launches(*form)) for op, form in eng.conv_forms(net_id, B).items()}
    # the images the float64 side looks at
    nimg = B if fcn else 2 * B
    per = 1 if fcn else 2
    sel = list(range(nimg)) if c["images"] == "all" or B == 1 else list(range(per)) + list(range(nimg - per, nimg))
    images = fr if fcn else np.stack([im for f in fr for im in (f, f[:, ::-1])], 0)
    plan = eng.precision_plan()["fcn8s" if fcn else "monodepth"][0]
    tokens = ()
    if c["precision"] == "plan":
        tokens = tuple(t.strip() for t in eng.lib.sd_default_plan(net_id).decode().split(","))
    cache = {"frames": np.ascontiguousarray(images[sel])}

    def get(name):
        """the GPU's stored tensor as float64 NCHW (the selected images), None where the plan holds no tensor of that name"""
        if name in cache:
            return cache[name]
        if name == "logits":
            t = logits
        else:
            try:
                t = eng.net_tensor(net_id, name)
            except L.SdError as e:
                if "unknown tensor" not in str(e):
                    raise
                cache[name] = None
                return None
        assert t.shape[0] == nimg, (case_id(c), name, tuple(t.shape))      # the images of THIS pass, not those the handle has room for
        t = t[torch.as_tensor(sel, device=t.device)].cpu()
        if name == "input_pre":
            t = t[..., :3]                     # (the f32 engine stores the zero fourth channel of its float4 gathers)
        cache[name] = t.permute(0, 3, 1, 2).contiguous().to(torch.float64)
        return cache[name]

    widths, h_, w_ = {"frames": W}, {}, {}
    numerics = None
    rows, extents, covered, pending = [], [], set(), []
    scale = None if fcn else LY.mono_input_scale(plan)
    for i, Lr in enumerate(layers):
        if c["only"] and Lr.name not in c["only"]:
            if Lr.name in labels:
                covered.add(Lr.name)           # (a case that looks at named layers alone does not count the others)
            continue
        got = get(Lr.name)
        if got is None:
            nxt = layers[i + 1] if i + 1 < len(layers) else None
            fused_pool = Lr.kind == "conv" and nxt is not None and nxt.kind == "pool2" and nxt.srcs[0].name == Lr.name
            in_tail = Lr.name in ("dec/upconv1", "dec/iconv1") and "dec/tail1" in labels
            assert fused_pool or in_tail, f"{case_id(c)}: the plan holds no tensor '{Lr.name}' and no fusion explains it"
            pending.append(Lr)
            continue
        group, pending = pending + [Lr], []
        tensors = {}
        for g in group:
            for s in g.srcs:
                if s.name not in [x.name for x in group]:
                    tensors[s.name] = get(s.name)
                    assert tensors[s.name] is not None, (case_id(c), g.name, s.name)
        if numerics is None:
            for Lw in layers:                   # the width of every map (a head's form depends on it): from the frame size and the strides
                src = Lw.srcs[0]
                wi = widths[src.name] * (2 if src.up else 1)
                widths[Lw.name] = {"pool2": wi // 2, "pool3z": (wi - 1) // 2 + 1, "deconv": wi * Lw.stride, "deconv_add": wi * Lw.stride}.get(
                    Lw.kind, (wi - 1) // (Lw.srcs[0].stride or Lw.stride) + 1 if Lw.kind == "conv" else wi)
            numerics = LY.layer_numerics(layers, c["precision"] if not (fcn and c["precision"] == "mixed") else "bf16x2", plan, tokens, widths)
        co = None
        if Lr.name == "dec/disp1":
            co = [0]                            # only disp_left_est[0] is computed (plan.cpp: nout = 1)
        elif Lr.name in ("fc6", "fc7") and c["only"]:
            co = FC_CHANNELS
            got = got[:, torch.as_tensor(co)]
        ref, bnd = LY.check_group(group, tensors, w, numerics, co, scale)
        wst = LY.compare("+".join(g.name for g in group), got, ref, bnd)
        wst.index = (sel[wst.index[0]],) + tuple(wst.index[1:])
        ops = [g.name for g in group if g.name in labels] + (["dec/tail1"] if Lr.name == "dec/disp1" and len(group) == 3 else [])
        covered.update(ops)
        label = " | ".join(labels[o] for o in ops) if ops else {"pool2": "maxpool2", "pool3z": "maxpool3z", "deconv": "deconv16s8_head",
                                                               "deconv_add": "deconv4s2_add", "conv": "conv_smalln"}.get(Lr.kind, Lr.kind)
        rows.append((wst.layer, label, wst))
        hw = tuple(int(v) * (2 if len(group) == 2 and Lr.kind == "pool2" else 1) for v in got.shape[2:])      # (a fused pool: the conv's own map)
        extents.append((wst.layer, label, hw))
        if log:
            log(f"  {wst.layer:34s} {label:44s} {hw[0]:4d}x{hw[1]:<4d} {wst.ratio:9.4f}  at {wst.index}")
    assert not pending, [g.name for g in pending]
    all_labels = " ".join(labels.values())
    unmet = [f"{lab} on a layer '{pre}*' with an output map of: {e}" for lab, pre, e in c["need_at"]
             if not any(lab in label and name.startswith(pre) and EXTENT[e](*hw) for name, label, hw in extents)]
    res = dict(rows=rows, extents=extents, uncovered=sorted(set(labels) - covered), labels=labels, missing=[f for f in c["need"] if f not in all_labels],
               unmet=unmet, seconds=time.time() - t0, plan=plan)
    eng.close()
    return res


def failure_lines(c, res):
    return [f"{case_id(c)}: {name} [{label}] image {w.index[0]}, y {w.index[1]}, x {w.index[2]}, channel {w.index[3]}: |delta| / bound = {w.ratio:.4g} "
            f"(|delta| {w.delta:.4g}, bound {w.bound:.4g}, ref {w.ref:.6g})" for name, label, w in res["rows"] if not w.ratio <= 1.0]


def table_lines(c, res):
    """one line per kernel label of the case: the worst ratio, the layer it occurred in, and the output maps (height x width) the label ran on"""
    worst, maps = {}, {}
    for name, label, w in res["rows"]:
        if label not in worst or w.ratio > worst[label][0]:
            worst[label] = (w.ratio, name)
    for name, label, hw in res["extents"]:
        maps.setdefault(label, set()).add(hw)
    return [f"{c['precision']:7s} {c['net']:9s} {c['H']}x{c['W']} B={c['frames']}/{c['max_batch']}" + (f" small_batch={c['small_batch']}" if c["small_batch"] else "") +
            f"  {label:60s} {r:8.4f}  {name:34s} maps " + " ".join(f"{h}x{w}" for h, w in sorted(maps[label], reverse=True))
            for label, (r, name) in sorted(worst.items())]


def _is_256x512_of_8_frames(c):
    """the cases whose slowest sets the time a case at a size that is no power of two may take (main)"""
    return (c["H"], c["W"], c["frames"]) == (256, 512, 8)


def main():
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    print("# worst |delta| / bound per (engine, geometry, kernel label) and the layer it occurred in; scripts/layer_check.py on the MI355X")
    per_engine, per_engine_odd, bad, secs = {}, {}, [], {}
    for c in CASES:
        res = run_case(c)
        for line in table_lines(c, res):
            print(line, flush=True)
        top = max(res["rows"], key=lambda r: r[2].ratio)
        odd = c["H"] & (c["H"] - 1) != 0      # a frame height that is no power of two
        for table in (per_engine,) + ((per_engine_odd,) if odd else ()):
            if top[2].ratio > table.get(c["precision"], (0, "", ""))[0]:
                table[c["precision"]] = (top[2].ratio, case_id(c), top[0] + " [" + top[1] + "]")
        bad += failure_lines(c, res) + [f"{case_id(c)}: uncovered op {o}" for o in res["uncovered"]] + [f"{case_id(c)}: {f} did not run" for f in res["missing"]]
        bad += [f"{case_id(c)}: no {u}" for u in res["unmet"]]
        secs[case_id(c)] = (res["seconds"], odd, _is_256x512_of_8_frames(c))
        print(f"# {case_id(c)}: {len(res['rows'])} layers, {len(res['uncovered'])} uncovered ops, {res['seconds']:.1f} s", flush=True)
    print("# worst line per engine")
    for p, (r, cid, where) in per_engine.items():
        print(f"# {p:7s} {r:8.4f}  {cid}  {where}")
    print("# worst line per engine at the frame sizes that are no power of two")
    for p, (r, cid, where) in per_engine_odd.items():
        print(f"# {p:7s} {r:8.4f}  {cid}  {where}")
    limit = max(s for s, _, b8 in secs.values() if b8)
    slowest = max((s, cid) for cid, (s, odd, _) in secs.items() if odd)
    print(f"# slowest 256x512 B8 case {limit:.1f} s; slowest case at a size that is no power of two {slowest[0]:.1f} s ({slowest[1]})")
    bad += [f"{cid}: {s:.1f} s, longer than the slowest 256x512 B8 case ({limit:.1f} s)" for cid, (s, odd, _) in secs.items() if odd and s > limit]
    print("# " + ("every layer inside its bound, no op uncovered" if not bad else "OUTSIDE:"))
    for b in bad:
        print("# " + b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
