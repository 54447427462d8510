"""Every layer of both networks ALONE against a float64 reference (oracle/layers.py): one forward under SEMDEPTH_KEEP_ACTIVATIONS=1, then, layer
by layer, the GPU's own stored input tensor(s) through the float64 layer on the CPU against the GPU's stored output, held to the per-element
bound of oracle/layers.py (derived from the formats, not fitted).  Upstream error never enters: what is compared is one kernel's arithmetic,
addressing and output rounding.

    python scripts/layer_check.py > profiles/layer_check_worst_ratios.txt

writes one line per (engine, geometry, kernel label): the worst |delta| / bound and the layer it occurred in.  tests/test_gpu_layers.py imports
CASES / run_case() from here and asserts what this prints.

Reading a failure: "<layer> [<kernel label>] image i, y, x, channel c: |delta| / bound = r" names the layer, the kernel instantiation that ran it
(SEMDEPTH_PROFILE_VERBOSE's label) and the worst element.  r <= 1 passes.  A ratio of a few units on many layers of one engine points at a format
term of the bound (oracle/layers.py SCHEMES / OUT_FORMATS); hundreds and more on one layer, at an edge pixel, the last image or one channel group, is a
kernel, a weight relayout or a planner bug -- see tests/test_layer_check_cpu.py for what each kind of mistake looks like."""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

KEEP, VERBOSE = "SEMDEPTH_KEEP_ACTIVATIONS", "SEMDEPTH_PROFILE_VERBOSE"
FC_CHANNELS = np.r_[0:64, 2016:2080, 4032:4096]      # fc6 / fc7 at full size: the first 64, 64 across the tile boundary at 2048, the last 64


def case(net, precision, H, W, frames, max_batch=None, small_batch=0, images="all", only=None, need=()):
    """net: 'fcn8s' | 'resnet50' | 'vgg'.  images: 'all' or 'ends' (first and last frame's images).  only: check these layers alone (fc6 / fc7 at full
    size).  need: kernel-label prefixes that must have run (a silently rerouted layer must not make the case pass)."""
    return dict(net=net, precision=precision, H=H, W=W, frames=frames, max_batch=max_batch or frames, small_batch=small_batch, images=images,
                only=only, need=tuple(need))


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
    return out


CASES = _cases()


class _Stderr:
    """the bytes the library writes to file descriptor 2 inside the block (the per-layer lines of sd_profile_read)"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


_weights = {}


def _frames(B, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def run_case(c, log=None):
    """-> dict(rows=[(group name, kernel label, oracle.layers.Worst)], uncovered=[op names], labels={op: label}, missing=[needed families that did
    not run], seconds).  Sets (and restores) the two environment switches an engine latches when it is created."""
    from oracle import layers as LY
    from semantic_depth_amd import _lib as L, weights as Wt
    from semantic_depth_amd.engine import Engine
    t0 = time.time()
    fcn = c["net"] == "fcn8s"
    net_id = L.SD_NET_FCN8S if fcn else L.SD_NET_MONODEPTH
    enc = "resnet50" if fcn else c["net"]
    H, W, B = c["H"], c["W"], c["frames"]
    saved = {k: os.environ.get(k) for k in (KEEP, VERBOSE)}
    os.environ[KEEP] = os.environ[VERBOSE] = "1"
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
    assert B == 1 or not np.array_equal(fr[0], fr[-1])
    dev = torch.from_numpy(fr).cuda()
    eng.profile(True)
    logits = None
    if fcn:
        logits = eng.fcn8s_forward(dev, want_logits=True)["logits"]
    else:
        eng.monodepth_forward(dev, want_raw=True)
    with _Stderr() as cap:
        eng.profile_read()
    eng.profile(False)
    labels = {}
    for line in cap.text.splitlines():
        if line.startswith("[sd_profile]"):
            op, lab = line.split()[1], line.split("TF/s", 1)[1].strip()
            labels[op] = labels[op] + " + " + lab if op in labels else lab
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
        t = t[torch.as_tensor(sel, device=t.device)].cpu()
        if name == "input_pre":
            t = t[..., :3]                     # (the f32 engine stores the zero fourth channel of its float4 gathers)
        cache[name] = t.permute(0, 3, 1, 2).contiguous().to(torch.float64)
        return cache[name]

    widths, h_, w_ = {"frames": W}, {}, {}
    numerics = None
    rows, covered, pending = [], set(), []
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
        if log:
            log(f"  {wst.layer:34s} {label:44s} {wst.ratio:9.4f}  at {wst.index}")
    assert not pending, [g.name for g in pending]
    all_labels = " ".join(labels.values())
    res = dict(rows=rows, uncovered=sorted(set(labels) - covered), labels=labels, missing=[f for f in c["need"] if f not in all_labels],
               seconds=time.time() - t0, plan=plan)
    eng.close()
    return res


def failure_lines(c, res):
    return [f"{case_id(c)}: {name} [{label}] image {w.index[0]}, y {w.index[1]}, x {w.index[2]}, channel {w.index[3]}: |delta| / bound = {w.ratio:.4g} "
            f"(|delta| {w.delta:.4g}, bound {w.bound:.4g}, ref {w.ref:.6g})" for name, label, w in res["rows"] if not w.ratio <= 1.0]


def table_lines(c, res):
    """one line per kernel label of the case: the worst ratio and the layer it occurred in"""
    worst = {}
    for name, label, w in res["rows"]:
        if label not in worst or w.ratio > worst[label][0]:
            worst[label] = (w.ratio, name)
    return [f"{c['precision']:7s} {c['net']:9s} {c['H']}x{c['W']} B={c['frames']}/{c['max_batch']}" + (f" small_batch={c['small_batch']}" if c["small_batch"] else "") +
            f"  {label:60s} {r:8.4f}  {name}" for label, (r, name) in sorted(worst.items())]


def main():
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    print("# worst |delta| / bound per (engine, geometry, kernel label) and the layer it occurred in; scripts/layer_check.py on the MI355X")
    per_engine, bad = {}, []
    for c in CASES:
        res = run_case(c)
        for line in table_lines(c, res):
            print(line, flush=True)
        top = max(res["rows"], key=lambda r: r[2].ratio)
        if top[2].ratio > per_engine.get(c["precision"], (0, "", ""))[0]:
            per_engine[c["precision"]] = (top[2].ratio, case_id(c), top[0] + " [" + top[1] + "]")
        bad += failure_lines(c, res) + [f"{case_id(c)}: uncovered op {o}" for o in res["uncovered"]] + [f"{case_id(c)}: {f} did not run" for f in res["missing"]]
        print(f"# {case_id(c)}: {len(res['rows'])} layers, {len(res['uncovered'])} uncovered ops, {res['seconds']:.1f} s", file=sys.stderr, flush=True)
    print("# worst line per engine")
    for p, (r, cid, where) in per_engine.items():
        print(f"# {p:7s} {r:8.4f}  {cid}  {where}")
    print("# " + ("every layer inside its bound, no op uncovered" if not bad else "OUTSIDE:"))
    for b in bad:
        print("# " + b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
