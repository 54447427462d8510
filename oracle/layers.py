"""Layer-by-layer restatement of oracle/nets.py, with a per-element error bound for every layer.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  ``fcn8s_layers()`` / ``monodepth_layers(encoder)`` list the two graphs as
``Layer`` records in execution order; a layer is a function of NAMED input tensors (NCHW torch tensors), named after the tensor
the engine's planner gives its output (``conv3_2``, ``pool4``, ``enc/res3_2/conv3``, ``dec/iconv4`` ...), so that one layer can be
computed from the GPU's own stored inputs (``Engine.net_tensor``) and compared with the GPU's stored output: upstream error never
enters, what remains is one kernel's arithmetic, addressing and output rounding.

PINNED to oracle/nets.py: ``chain()`` uses the same torch calls in the same order, and tests/test_layer_check_cpu.py asserts that it
reproduces ``nets.fcn8s_forward`` / ``nets.monodepth_forward`` in float64 bit for bit.

The bound of a layer (``bound()``), per output element:

    bound = (LAMBDA * sqrt(K) * 2^-24 + u_drop) * S  +  u_out * max(S, |ref|)  +  S_w  +  S_in  +  a_act  +  a_floor

  S       conv(|x|, |w|) + |b| with the layer's own geometry, times the activation's Lipschitz constant (1 for ReLU / ELU / none,
          0.3 / 4 for 0.3 * sigmoid)
  K       the layer's true reduction length (k * k * input channels; 1 for the element-wise ops)
  S_w     conv(|x|, u_w |w| + w_abs): the weight planes' rounding (relative u_w, absolute w_abs where the low plane is an fp16 subnormal)
  S_in    u_in * S: only where a layer reads fewer planes of its input than the tensor stores
  u_*     from the header comment of csrc/split_fmt.hpp, one table each for the product schemes (SCHEMES) and the output formats (OUT_FORMATS)
  a_act   the activation's own documented absolute error (ACT)
  LAMBDA  8: the probabilistic rounding-error constant.  A correct f32 accumulation of K terms leaves LAMBDA sqrt(K) u S with a chance
          below 1e-9 per element for K <= 25088 (the error of a length-K f32 chain is a sum of K roundings of at most u |partial sum|
          each; eight standard deviations of its sqrt(K) u S scale).

Nothing in it is fitted to the code under test.  Composite layers (a conv whose 2x2 pool is fused into its epilogue, the one-launch
decoder tail) propagate the bound: through a following conv as conv(bound_1, |w_2|) * Lipschitz + own, through a max-pool as the
window maximum (``check_group`` does this when it is handed a run of layers).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from . import nets

LAMBDA = 8.0
U32 = 2.0 ** -24


# ------------------------------------------------------------------------------------------
# the numerics tables
# ------------------------------------------------------------------------------------------
# product scheme -> (u_w, w_abs, u_drop).  w_abs is in units of the layer's max |w| where noted.
#   f32     exact operands (kernels.hpp:41); the issue's table allows the same 2^-23 as bf16x3
#   bf16x3  split_fmt.hpp:14-19: operands exact, the three dropped terms "below 2^-23 |x w| together"
#   f16x2   split_fmt.hpp:20-30 (HS): w' = w 2^k in two fp16 planes, 2^-23; dropped x_lo * w_lo < 2^-24; w_lo is a subnormal fp16
#           (spacing 2^-24) below |w'| = 2^-3 with max |w'| >= 2^12: an absolute 2^-25 / 2^12 = 2^-37 of the layer's max |w|
#   bf16x2  split_fmt.hpp:2-4: hi + lo bf16 planes, 16 bits -> 2^-17; "dropped term ~2^-18"
#   f16w    split_fmt.hpp:5-10: weights in two fp16 planes (22 bits -> 2^-23, nothing dropped); w_lo "of an ordinary weight is an fp16
#           subnormal" (plan.cpp f16_split): absolute 2^-25
#   f16x1   split_fmt.hpp:5-10 + kernels.hpp:44: the weight rounded ONCE to fp16, U_F16 (absolute 2^-25 below 2^-14)
#   f16xw   split_fmt.hpp:11-13 + kernels.hpp:45: the same weight rounding, both activation planes read
# U_F16, one rounding to ONE fp16 plane: split_fmt.hpp:6 "rounded ONCE to fp16 (11 bits)".  Round-to-nearest to an 11-bit significand is off by
# up to half a unit in the last place, 2^-11 |v| for a value just above a power of two; the "2^-12" of split_fmt.hpp:8 is the typical size
# of that rounding, not its bound.  (Seen on the MI355X: conv1_1 of the plan engine stores 267.124 as 267.0 + a multiple of 0.25, 0.1237 away --
# inside fp16's half-ulp of 0.125 at 256..512, outside 2^-12 |v| = 0.065.)
U_F16 = 2.0 ** -11
@dataclass(frozen=True)
class SchemeTerms:
    u_w: float
    w_abs: float = 0.0          # absolute weight error
    w_abs_rel_max: float = 0.0  # absolute weight error in units of max |w| of the layer
    u_drop: float = 0.0


SCHEMES = {
    "f32": SchemeTerms(0.0, u_drop=2.0 ** -23),
    "bf16x3": SchemeTerms(0.0, u_drop=2.0 ** -23),
    "f16x2": SchemeTerms(2.0 ** -23, w_abs_rel_max=2.0 ** -37, u_drop=2.0 ** -24),
    "bf16x2": SchemeTerms(2.0 ** -17, u_drop=2.0 ** -18),
    "f16w": SchemeTerms(2.0 ** -23, w_abs=2.0 ** -25),
    "f16x1": SchemeTerms(U_F16, w_abs=2.0 ** -25),
    "f16xw": SchemeTerms(U_F16, w_abs=2.0 ** -25),
    "exact": SchemeTerms(0.0),
}
# output format -> (u_out, a_floor)
#   f32 / bf16x3  exact (split_fmt.hpp:14-16: "nothing is rounded when a tensor ... is stored")
#   hs      split_fmt.hpp:20-23: 22 significand bits -> 2^-23; the scaled lo plane is an fp16 subnormal (spacing 2^-24) where hi is:
#           2^-25 / 2^11 = 2^-36 absolute
#   bf16x2  split_fmt.hpp:2-3: 2^-17 (f32 exponent range: no floor)
#   f16     split_fmt.hpp:5-6: ONE fp16 plane, U_F16; fp16 subnormal spacing 2^-24 -> 2^-25 absolute
#   f16x2   split_fmt.hpp:11: hi + unscaled lo, 2^-23; lo is subnormal below |v| ~ 2^-3 -> 2^-25 absolute
OUT_FORMATS = {"f32": (0.0, 0.0), "bf16x3": (0.0, 0.0), "hs": (2.0 ** -23, 2.0 ** -36), "bf16x2": (2.0 ** -17, 0.0),
               "f16": (U_F16, 2.0 ** -25), "f16x2": (2.0 ** -23, 2.0 ** -25)}
_FMT_ORDER = {"bf16x2": 0, "f16": 1, "f16x2": 2}
# activation -> (Lipschitz constant, absolute error of the GPU's form)
#   elu        kernels.hpp:143-155: |abs error| < 2.5e-7 (fast_elu) / < 2e-7 (fast_elu_split)
#   sigmoid03  0.3f * (1 / (1 + expf(-v))) (kernels.hpp:164): expf, an add, a divide and a multiply, each within an f32 rounding or two
#              of a value <= 0.3 -> 8 * 2^-24 * 0.3
ACT = {None: (1.0, 0.0), "relu": (1.0, 0.0), "elu": (1.0, 2.5e-7), "sigmoid03": (0.3 / 4.0, 8 * U32 * 0.3)}
U_IN_HI_ONLY = U_F16           # split_fmt.hpp:13: "Any other fp16 layer reads the hi plane of such a tensor as if it were the one-plane format"
U_W_FOLD = 2.0 ** -24          # plan.cpp (OpDesc::fold): the taps that read the same source pixel are added and rounded once to f32
U_W_INPUT_SCALE = 2.0 ** -23   # plan.cpp apply_precision_plan: the 1 / 255 of the input moves into the weights (two f32 roundings)


# ------------------------------------------------------------------------------------------
# the graphs
# ------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Src:
    name: str
    up: bool = False          # read through a x2 nearest-neighbour upsample
    stride: int = 0           # 0: the layer's stride (the shortcut of a bottleneck block carries its own)


@dataclass(frozen=True)
class Layer:
    name: str                 # = the planner's name of the output tensor
    kind: str                 # pre_vgg | pre_mono | conv | pool2 | pool3z | deconv_add | deconv
    srcs: tuple = ()
    weights: tuple = ()       # ((weight name, bias name), ...): one pair, or one per source for a 'sum' layer
    k: int = 1
    stride: int = 1
    act: str | None = None
    join: str = "cat"         # several sources: 'cat' (channel concat, one weight) or 'sum' (one weight each, outputs added)
    tf_same: bool = False     # padding given to conv2d (the VGG body) instead of an explicit zero pad (monodepth's conv())
    head: bool = False        # a few-channel head (score / disparity): an f32 per-thread kernel unless the planner makes it a direct conv


_VGG_BLOCKS = (("conv1_1", "conv1_2"), ("conv2_1", "conv2_2"), ("conv3_1", "conv3_2", "conv3_3"), ("conv4_1", "conv4_2", "conv4_3"),
               ("conv5_1", "conv5_2", "conv5_3"))


def fcn8s_layers():
    out = [Layer("input_pre", "pre_vgg", (Src("frames"),))]
    x = "input_pre"
    for s, blk in enumerate(_VGG_BLOCKS, start=1):
        for n in blk:
            out.append(Layer(n, "conv", (Src(x),), ((f"vgg/{n}/filter", f"vgg/{n}/biases"),), 3, 1, "relu", tf_same=True))
            x = n
        out.append(Layer(f"pool{s}", "pool2", (Src(x),)))
        x = f"pool{s}"
    out.append(Layer("fc6", "conv", (Src("pool5"),), (("vgg/fc6/filter", "vgg/fc6/biases"),), 7, 1, "relu", tf_same=True))
    out.append(Layer("fc7", "conv", (Src("fc6"),), (("vgg/fc7/filter", "vgg/fc7/biases"),), 1, 1, "relu", tf_same=True))
    for n, src in (("score7", "fc7"), ("score4", "pool4"), ("score3", "pool3")):
        out.append(Layer(n, "conv", (Src(src),), ((f"dec/{n}/kernel", f"dec/{n}/bias"),), 1, 1, None, tf_same=True, head=True))
    out.append(Layer("first_skip", "deconv_add", (Src("score7"), Src("score4")), (("dec/deconv1/kernel", "dec/deconv1/bias"),), 4, 2))
    out.append(Layer("second_skip", "deconv_add", (Src("first_skip"), Src("score3")), (("dec/deconv2/kernel", "dec/deconv2/bias"),), 4, 2))
    out.append(Layer("logits", "deconv", (Src("second_skip"),), (("dec/deconv3/kernel", "dec/deconv3/bias"),), 16, 8))
    return out


def _wb(n):
    return ((n + "/weights", n + "/biases"),)


def monodepth_layers(encoder: str = "resnet50"):
    out = [Layer("input_pre", "pre_mono", (Src("frames"),))]
    cv = lambda n, srcs, k, s, act="elu", **kw: out.append(Layer(n, "conv", tuple(srcs), _wb(n), k, s, act, **kw))
    if encoder == "vgg":
        x, feats = "input_pre", []
        for i, k in enumerate([7, 5, 3, 3, 3, 3, 3], start=1):
            cv(f"enc/conv{i}a", [Src(x)], k, 1)
            cv(f"enc/conv{i}b", [Src(f"enc/conv{i}a")], k, 2)
            x = f"enc/conv{i}b"
            feats.append(x)
        skips = {lvl: feats[lvl - 2] for lvl in range(2, 8)}
        top = 7
    elif encoder == "resnet50":
        cv("enc/conv1", [Src("input_pre")], 7, 2)
        out.append(Layer("enc/pool1", "pool3z", (Src("enc/conv1"),)))
        x, stage_out = "enc/pool1", {}
        for stage, blocks in ((2, 3), (3, 4), (4, 6), (5, 3)):
            for b in range(1, blocks + 1):
                p, stride = f"enc/res{stage}_{b}", (2 if b == blocks else 1)
                cv(p + "/conv1", [Src(x)], 1, 1)
                cv(p + "/conv2", [Src(p + "/conv1")], 3, stride)
                out.append(Layer(p + "/conv3", "conv", (Src(p + "/conv2", stride=1), Src(x, stride=stride)),
                                 (_wb(p + "/conv3")[0], _wb(p + "/proj")[0]), 1, 1, "elu", join="sum"))
                x = p + "/conv3"
            stage_out[stage] = x
        skips = {6: stage_out[4], 5: stage_out[3], 4: stage_out[2], 3: "enc/pool1", 2: "enc/conv1"}
        top = 6
    else:
        raise ValueError(encoder)
    disp_prev = None
    for lvl in range(top, 0, -1):
        cv(f"dec/upconv{lvl}", [Src(x, up=True)], 3, 1)
        cat = [Src(f"dec/upconv{lvl}")]
        if lvl in skips:
            cat.append(Src(skips[lvl]))
        if lvl <= 3:
            cat.append(Src(disp_prev, up=True))
        cv(f"dec/iconv{lvl}", cat, 3, 1)
        x = f"dec/iconv{lvl}"
        if lvl <= 4:
            cv(f"dec/disp{lvl}", [Src(x)], 3, 1, "sigmoid03", head=True)
            disp_prev = f"dec/disp{lvl}"
    return out


# ------------------------------------------------------------------------------------------
# one layer
# ------------------------------------------------------------------------------------------
def _t(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype)


def _weights(layer, w, dtype, co=None):
    """[(OIHW weight, bias)] of a conv layer (IOHW for the transposed ones), restricted to the output channels ``co``"""
    out = []
    for wn, bn in layer.weights:
        wa, ba = w[wn], w[bn]
        if co is not None:
            if layer.kind != "conv":
                raise ValueError("output-channel subsets exist for conv layers only")
            wa, ba = wa[..., np.asarray(co)], ba[np.asarray(co)]
        out.append((nets._conv_w(wa, dtype), _t(ba, dtype)))     # HWIO -> OIHW; a transposed conv's HWOI -> IOHW by the same permutation
    return out


def _read(x, src):
    """a source as the layer sees it: through the x2 nearest-neighbour upsample where the layer reads it so"""
    return nets._Mono.up(x) if src.up else x


def _linear(layer, xs, wbs):
    """the layer before its activation, with the torch calls of oracle/nets.py in their order; the bound calls it with |x|, |w|, |b| for the same
    geometry"""
    if layer.kind == "conv":
        p = (layer.k - 1) // 2
        if layer.join == "sum":
            y = None
            for x, src, (wt, b) in zip(xs, layer.srcs, wbs):
                s = src.stride or layer.stride
                t = F.conv2d(F.pad(x, (p, p, p, p)), wt, b, stride=s)
                y = t if y is None else y + t
            return y
        x = [_read(x, s) for x, s in zip(xs, layer.srcs)]
        x = x[0] if len(x) == 1 else torch.cat(x, 1)
        wt, b = wbs[0]
        if layer.tf_same:
            return F.conv2d(x, wt, b, padding=p, stride=layer.stride)
        return F.conv2d(F.pad(x, (p, p, p, p)), wt, b, stride=layer.stride)
    if layer.kind in ("deconv", "deconv_add"):
        wt, b = wbs[0]
        y = F.conv_transpose2d(xs[0], wt, b, stride=layer.stride, padding=(layer.k - layer.stride) // 2)
        return y + xs[1] if layer.kind == "deconv_add" else y
    raise ValueError(layer.kind)


def _act(y, act):
    if act == "relu":
        return F.relu(y)
    if act == "elu":
        return F.elu(y)
    if act == "sigmoid03":
        return 0.3 * torch.sigmoid(y)
    return y


def evaluate(layer: Layer, xs, w, dtype=torch.float64, co=None, input_scale=None):
    """the layer's output (NCHW, ``dtype``) from its input tensors ``xs`` (NCHW, one per source; 'frames' is the uint8 NHWC batch).
    ``input_scale``: pre_mono only -- the engine's input scale (1 / 255 unless the plan moved it into the first layer's weights)."""
    if layer.kind == "pre_vgg":
        return nets.vgg_preprocess(np.asarray(xs[0]), dtype)
    if layer.kind == "pre_mono":
        # the caller of nets.monodepth_forward divides in float32 (test_gpu_nets / compute_disparity): frame.astype(f32) / 255
        f = np.asarray(xs[0]).astype(np.float32)
        f = f / 255 if input_scale is None else f * np.float32(input_scale)
        return _t(f, dtype).permute(0, 3, 1, 2).contiguous()
    xs = [x.to(dtype) for x in xs]
    if input_scale is not None and layer.srcs[0].name == "input_pre":
        xs = [xs[0] * (input_scale / 255.0)]      # the stem of such a plan carries the 1 / 255 in its weights: the same function of the stored input
    if layer.kind == "pool2":
        return F.max_pool2d(xs[0], 2, 2)
    if layer.kind == "pool3z":
        return nets._Mono.maxpool3(None, xs[0])
    return _act(_linear(layer, xs, _weights(layer, w, dtype, co)), layer.act)


def reduction_length(layer: Layer, xs) -> int:
    if layer.kind == "conv":
        return layer.k * layer.k * sum(int(x.shape[1]) for x in xs)
    if layer.kind in ("deconv", "deconv_add"):        # the taps that reach one output pixel, and the skip tensor's add
        return (layer.k // layer.stride) ** 2 * int(xs[0].shape[1]) + (1 if layer.kind == "deconv_add" else 0)
    return 1


@dataclass(frozen=True)
class Numerics:
    """how the engine ran one layer: product scheme, output format, and the extra relative terms (cited where they are set)"""
    scheme: str = "f32"
    out_fmt: str = "f32"
    u_in: float = 0.0
    u_w_extra: float = 0.0


def bound(layer: Layer, xs, w, num: Numerics = Numerics(), co=None, in_bounds=None, input_scale=None):
    """(ref, bound), both float64 NCHW.  ``in_bounds``: per-source error bounds of the inputs (composite layers), propagated through |w|."""
    ref = evaluate(layer, xs, w, torch.float64, co, input_scale)
    sch, (u_out, a_floor), (lip, a_act) = SCHEMES[num.scheme], OUT_FORMATS[num.out_fmt], ACT[layer.act]
    if layer.kind in ("pool2", "pool3z"):
        b = torch.zeros_like(ref)
        if in_bounds is not None and in_bounds[0] is not None:
            pad = F.pad(in_bounds[0], (1, 1, 1, 1)) if layer.kind == "pool3z" else in_bounds[0]
            b = F.max_pool2d(pad, 3 if layer.kind == "pool3z" else 2, 2)
        return ref, b
    if layer.kind in ("pre_vgg", "pre_mono"):
        # element-wise, K = 1: |x| + |mean| (resp. |x| * scale) rounded to f32 once, then to the output format
        if layer.kind == "pre_vgg":
            S = ref.abs() + 2.0 * torch.tensor(nets.VGG_MEAN_BGR, dtype=torch.float64).view(1, 3, 1, 1)      # >= |x| + |mean|
        else:
            S = ref.abs()
        return ref, (LAMBDA * U32 + u_out) * S + a_floor
    xa = [x.to(torch.float64).abs() for x in xs]
    if input_scale is not None and layer.srcs[0].name == "input_pre":
        xa = [xa[0] * (input_scale / 255.0)]
    wb = _weights(layer, w, torch.float64, co)
    zero_b = lambda wt, b: torch.zeros_like(b)
    wabs = [(wt.abs(), b.abs()) for wt, b in wb]
    xz = [xa[0], torch.zeros_like(xa[1])] if layer.kind == "deconv_add" else xa      # (the skip tensor is added, not multiplied by a weight)
    S0 = _linear(layer, xz, [(wt, zero_b(wt, b)) for wt, b in wabs])                # conv(|x|, |w|)
    S = S0 + wabs[0][1].view(1, -1, 1, 1) + (wabs[1][1].view(1, -1, 1, 1) if layer.join == "sum" else 0.0) + (xa[1] if layer.kind == "deconv_add" else 0.0)
    K = reduction_length(layer, xs)
    # S_w = conv(|x|, u_w |w| + w_abs) = u_w conv(|x|, |w|) + w_abs conv(|x|, 1): the second a box sum of |x|, the same for every output channel
    wmax = max(float(np.abs(w[wn]).max()) for wn, _ in layer.weights)      # (the slots of one accumulator share one scale)
    w_abs = sch.w_abs + sch.w_abs_rel_max * wmax
    S_w = (sch.u_w + num.u_w_extra) * S0
    if w_abs:
        ones = [(torch.ones_like(wt[:, :1] if layer.kind.startswith("deconv") else wt[:1]), torch.zeros(1, dtype=torch.float64)) for wt, _ in wabs]
        S_w = S_w + w_abs * _linear(layer, xz, ones)
    bnd = (LAMBDA * np.sqrt(K) * U32 + sch.u_drop + num.u_in) * S + S_w
    if in_bounds is not None and any(b is not None for b in in_bounds):
        ib = [torch.zeros_like(x) if b is None else b for x, b in zip(xa, in_bounds)]
        bnd = bnd + _linear(layer, ib, [(wt, zero_b(wt, b)) for wt, b in wabs])
    # the output format rounds the STORED value: u_out S for ReLU / ELU / none (|out| <= S), u_out |out| for 0.3 * sigmoid, whose value is not
    # small where S is (0.15 at S = 0)
    return ref, bnd * lip + u_out * torch.maximum(lip * S, ref.abs()) + a_act + a_floor


# ------------------------------------------------------------------------------------------
# chains and checks
# ------------------------------------------------------------------------------------------
def chain(layers, frames, w, dtype=torch.float64, start=None, override=None, input_scale=None):
    """every tensor of the graph, computed layer by layer: {name: NCHW tensor}.  ``override``: tensors that replace a layer's output (the
    layers behind it are computed from the replacement); ``start``: a dict of tensors already known, layers that produce them are skipped."""
    t = {"frames": frames}
    if start:
        t.update(start)
    for L in layers:
        if override and L.name in override:
            t[L.name] = override[L.name].to(dtype)
            continue
        if L.name in t:
            continue
        t[L.name] = evaluate(L, [t[s.name] for s in L.srcs], w, dtype, input_scale=input_scale)
    return t


def layer_numerics(layers, precision: str, f16_ops=(), plan_tokens=(), width=None, folded=()):
    """{layer name: Numerics} for an engine of ``precision`` ('f32', 'bf16x3', 'f16x2', 'bf16x2', 'plan', 'mixed').

    f16_ops      Engine.precision_plan()[net][0]: the conv layers on the fp16 schemes, ':1' / ':x' suffixed (plan.cpp apply_precision_plan)
    plan_tokens  the tokens of the plan string (sd_default_plan): a per-thread head named EXACTLY makes its input ONE fp16 plane
    width        {tensor name: W}: a disparity head that feeds the next iconv runs as a direct conv on the engine's scheme where its
                 map is a multiple of 32 wide (plan.cpp smalln), as an f32 per-thread kernel otherwise
    The format rules restate plan.cpp (tensor(): the engine's activation format; smalln(): heads that feed nothing are f32; the deconv
    ladder is f32; apply_precision_plan(): an fp16 layer's sources become fp16 planes, a stand-alone pool keeps its source's format)."""
    base = {"f32": "f32", "bf16x3": "bf16x3", "f16x2": "f16x2", "bf16x2": "bf16x2", "plan": "bf16x2", "mixed": "bf16x2"}[precision]
    act_fmt = {"f32": "f32", "bf16x3": "bf16x3", "f16x2": "hs", "bf16x2": "bf16x2"}[base]
    f16 = {}
    for s in f16_ops:
        n, _, suf = s.partition(":")
        f16[n] = {"": "f16w", "1": "f16x1", "x": "f16xw"}[suf]
    by_name = {L.name: L for L in layers}
    consumers = {}
    for L in layers:
        for s in L.srcs:
            consumers.setdefault(s.name, []).append(L.name)
    scheme, fmt = {}, {"frames": "f32"}
    for L in layers:
        lvl = int(L.name[-1]) if L.name.startswith("dec/disp") else 0
        direct_head = L.head and lvl > 1 and base not in ("f32", "bf16x3") and width is not None and width.get(L.srcs[0].name, 1) % 32 == 0
        if L.kind in ("pool2", "pool3z", "pre_vgg", "pre_mono"):
            scheme[L.name] = "exact"
        elif L.kind in ("deconv", "deconv_add") or (L.head and not direct_head):
            scheme[L.name] = "f32"
        else:
            scheme[L.name] = f16.get(L.name, base)
        f32_out = L.kind in ("deconv", "deconv_add") or (L.head and not (lvl > 1))
        fmt[L.name] = "f32" if f32_out else act_fmt
    if base == "bf16x2":
        up = lambda n, want: fmt.__setitem__(n, want) if fmt[n] != "f32" and _FMT_ORDER[fmt[n]] < _FMT_ORDER[want] else None
        for L in layers:
            if scheme[L.name] in ("f16w", "f16x1", "f16xw"):
                for s in L.srcs:
                    up(s.name, "f16x2" if scheme[L.name] == "f16xw" else "f16")
            elif L.head and scheme[L.name] == "f32" and L.name in plan_tokens and fmt[L.srcs[0].name] == "bf16x2":
                fmt[L.srcs[0].name] = "f16"
        for _ in range(4):      # a stand-alone pool keeps the format of its source (a fused one has no source tensor: harmless)
            for L in layers:
                if L.kind in ("pool2", "pool3z"):
                    a, b = L.srcs[0].name, L.name
                    if fmt[a] != "f32" and fmt[b] != "f32" and fmt[a] != fmt[b]:
                        hi = max(fmt[a], fmt[b], key=_FMT_ORDER.get)
                        fmt[a] = fmt[b] = hi
    out = {}
    for L in layers:
        u_in = 0.0
        if scheme[L.name] in ("f16w", "f16x1") and any(fmt[s.name] == "f16x2" for s in L.srcs):
            u_in = U_IN_HI_ONLY
        extra = 0.0
        if L.name.startswith("dec/upconv") and base != "f32":
            extra += U_W_FOLD
        if L.name in f16 and L.srcs and L.srcs[0].name == "input_pre" and by_name["input_pre"].kind == "pre_mono":
            extra += U_W_INPUT_SCALE
        out[L.name] = Numerics(scheme[L.name], fmt[L.name], u_in, extra)
    return out


def mono_input_scale(f16_ops) -> float | None:
    """plan.cpp apply_precision_plan: a monodepth stem on an fp16 scheme reads the frame as 0..255 (exact in fp16) and carries the 1 / 255
    in its weights.  None: the default (frame / 255)."""
    names = {s.partition(":")[0] for s in f16_ops}
    return 1.0 if ("enc/conv1" in names or "enc/conv1a" in names) else None


@dataclass
class Worst:
    layer: str
    ratio: float
    index: tuple          # (image, y, x, channel)
    delta: float
    bound: float
    ref: float


def compare(name, got, ref, bnd) -> Worst:
    """worst |got - ref| / bound over a layer (all NCHW); the index is reported as (image, y, x, channel)"""
    got = torch.as_tensor(got).to(torch.float64)
    assert got.shape == ref.shape == bnd.shape, (name, got.shape, ref.shape, bnd.shape)
    d = (got - ref).abs()
    nan = ~torch.isfinite(got)
    r = torch.where(bnd > 0, d / bnd.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    r = torch.where(nan, torch.full_like(r, float("inf")), r)
    i = int(torch.argmax(r))
    n, c, y, x = np.unravel_index(i, tuple(r.shape))
    return Worst(name, float(r.reshape(-1)[i]), (int(n), int(y), int(x), int(c)), float(d.reshape(-1)[i]), float(bnd.reshape(-1)[i]),
                 float(ref.reshape(-1)[i]))


def check_group(group, tensors, w, numerics, co=None, input_scale=None):
    """(ref, bound) of the LAST layer of ``group``, a run of layers of which only the last one's output is materialised (one layer, a conv
    with its fused pool, or the one-launch decoder tail): inner outputs are the float64 reference's, their bounds are propagated."""
    inner, inner_b = {}, {}
    for j, L in enumerate(group):
        xs = [inner.get(s.name, tensors.get(s.name)) for s in L.srcs]
        ib = [inner_b.get(s.name) for s in L.srcs]
        last = j == len(group) - 1
        ref, b = bound(L, xs, w, numerics[L.name], co if last else None, ib if any(v is not None for v in ib) else None, input_scale)
        inner[L.name], inner_b[L.name] = ref, b
    return ref, b
