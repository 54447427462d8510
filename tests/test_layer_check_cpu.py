"""The layer checker (oracle/layers.py) on the CPU: the layer list is oracle/nets.py restated, a correct float32 implementation passes the
per-element bound with room to spare, and seven seeded kernel mistakes -- each of them invisible to the max-normalised 1e-3 check the network
tests use -- leave it by an order of magnitude or more.  Five more mistakes need a map with a partial row tile behind a full one, an odd source
height, a GEMM whose M is no multiple of 256 or a pass fed fewer frames than the handle holds: each is an exact no-op at the power-of-two
geometry (GEOM) and leaves the bound at the new one (GEOM_ODD).  No GPU: this is the proof that tests/test_gpu_layers.py can fail."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import layers as LY
from oracle import nets
from semantic_depth_amd import weights as Wt

F64 = torch.float64
GEOM = {"fcn8s": (64, 128), "resnet50": (64, 128), "vgg": (128, 128)}


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


class _Recording(dict):
    """a weight dict that counts how often oracle/nets.py reads each entry"""

    def __init__(self, w):
        super().__init__(w)
        self.reads = {}

    def __getitem__(self, k):
        self.reads[k] = self.reads.get(k, 0) + 1
        return super().__getitem__(k)


# the frame sizes of the layer check that are no power of two (scripts/layer_check.py), one frame each (a monodepth pass: the frame and its flipped
# copy).  resnet50 maps: 96x128, 48x64, 24x32 (one full 16-row tile and a partial one), 12x16, 6x8, 3x4 resp. 160x96, 80x48, 40x24, 20x12, 10x6, 5x3
GEOM_ODD = {"192x256": ("resnet50", 192, 256), "320x192": ("resnet50", 320, 192)}


class Net:
    def __init__(self, key, odd=None):
        """odd: a key of GEOM_ODD -- that geometry, one frame, without the run of oracle/nets.py (the mutants need the chained tensors alone)"""
        H, W = GEOM[key] if odd is None else GEOM_ODD[odd][1:]
        rng = np.random.default_rng(11)
        self.key = key
        if key == "fcn8s":
            self.layers = LY.fcn8s_layers()
            self.w = Wt.make_fcn8s_weights(1, decoder_std=0.05, bias_std=0.1)
            self.frames = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
            self.out = "logits"
        else:
            self.layers = LY.monodepth_layers(key)
            self.w = Wt.make_monodepth_weights(key, 2, gain=1.5 if key == "vgg" else 1.0, bias_std=0.05)
            fr = rng.integers(0, 256, (2 if key == "resnet50" and odd is None else 1, H, W, 3), dtype=np.uint8)
            # the images of a monodepth pass: every frame and its fliplr copy
            self.frames = np.stack([im for f in fr for im in (f, f[:, ::-1])], 0)
            self.out = "dec/disp1"
        if odd is not None:
            self.t64 = LY.chain(self.layers, self.frames, self.w, F64)
            self.t32 = LY.chain(self.layers, self.frames, self.w, torch.float32)
            return
        # oracle/nets.py itself, in float64, with its reads of the weights and its pool calls counted
        rec, pools, real_pool = _Recording(self.w), [], F.max_pool2d
        F.max_pool2d = lambda *a, **k: (pools.append(1), real_pool(*a, **k))[1]
        try:
            if key == "fcn8s":
                self.nets_out, self.nets_taps = nets.fcn8s_forward(self.frames, rec, dtype=F64, return_taps=True)
            else:
                self.nets_out = nets.monodepth_forward(self.frames.astype(np.float32) / 255, rec, key, dtype=F64, all_scales=True)
        finally:
            F.max_pool2d = real_pool
        self.nets_reads, self.nets_pools = rec.reads, len(pools)
        self.t64 = LY.chain(self.layers, self.frames, self.w, F64)
        self.t32 = LY.chain(self.layers, self.frames, self.w, torch.float32)

    def by_name(self, n):
        return next(L for L in self.layers if L.name == n)

    def inputs(self, L, dtype=F64):
        return [self.t32[s.name] if s.name == "frames" else self.t32[s.name].to(dtype) for s in L.srcs]


_nets = {}


@pytest.fixture(scope="module", params=["fcn8s", "resnet50", "vgg"])
def net(request):
    if request.param not in _nets:
        _nets[request.param] = Net(request.param)
    return _nets[request.param]


@pytest.fixture(scope="module")
def mono():
    if "resnet50" not in _nets:
        _nets["resnet50"] = Net("resnet50")
    return _nets["resnet50"]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


# ------------------------------------------------------------------------------------------------------------------------------
def test_chained_layers_reproduce_the_network_oracle_bit_for_bit(net):
    if net.key == "fcn8s":
        assert np.array_equal(_nhwc(net.t64["logits"]), net.nets_out)
        for tap, name in (("layer3", "pool3"), ("layer4", "pool4"), ("layer7", "fc7"), ("score7", "score7"), ("first_skip", "first_skip"),
                          ("second_skip", "second_skip")):
            assert np.array_equal(_nhwc(net.t64[name]), net.nets_taps[tap]), name
    else:
        for lvl in (1, 2, 3, 4):
            assert np.array_equal(_nhwc(net.t64[f"dec/disp{lvl}"]), net.nets_out[lvl]), lvl


def test_layer_list_is_complete(net):
    """every conv / score / deconv / head of oracle/nets.py reads its weight and its bias exactly once, every pool is one call: the layer list
    names the same weights once each and holds as many pools -- nothing of the graph is left out, nothing is there twice"""
    named = [n for L in net.layers for pair in L.weights for n in pair]
    assert len(named) == len(set(named))
    assert set(named) == set(net.nets_reads) == set(net.w)
    assert all(v == 1 for v in net.nets_reads.values()), {k: v for k, v in net.nets_reads.items() if v != 1}
    assert sum(L.kind in ("pool2", "pool3z") for L in net.layers) == net.nets_pools
    names = [L.name for L in net.layers]
    assert len(names) == len(set(names))
    produced = {"frames"}
    for L in net.layers:                      # every source is produced before it is read
        assert all(s.name in produced for s in L.srcs), L.name
        produced.add(L.name)
    if net.key == "fcn8s":
        assert len(net.layers) == 1 + 13 + 5 + 2 + 3 + 2 + 1
    elif net.key == "resnet50":
        assert len(net.layers) == 1 + 1 + 1 + 16 * 3 + 6 * 2 + 4
    else:
        assert len(net.layers) == 1 + 14 + 7 * 2 + 4


def test_a_correct_float32_implementation_passes(net):
    """the same float32 inputs through torch's float32 layer (the stand-in for a correct kernel) and through the float64 reference: every
    element within the f32 scheme's bound, the worst ratio printed per layer kind"""
    worst = {}
    for L in net.layers:
        xs = net.inputs(L)
        co = None
        if L.name in ("fc6", "fc7"):         # (as on the GPU: 192 of the 4096 channels keep the float64 side short)
            co = np.r_[0:64, 2016:2080, 4032:4096]
        got = LY.evaluate(L, [x if isinstance(x, np.ndarray) else x.float() for x in xs], net.w, torch.float32, co)
        ref, bnd = LY.bound(L, xs, net.w, LY.Numerics("exact" if L.kind.startswith(("pool", "pre")) else "f32", "f32"), co)
        wst = LY.compare(L.name, got, ref, bnd)
        assert wst.ratio <= 1.0, wst
        key = (L.kind, L.k)
        if wst.ratio > worst.get(key, (0, ""))[0]:
            worst[key] = (wst.ratio, L.name)
    print(net.key, "worst |delta| / bound of the float32 stand-in:", {f"{k[0]} {k[1]}x{k[1]}": (round(v[0], 4), v[1]) for k, v in worst.items()})


# ------------------------------------------------------------------------------------------------------------------------------
# seeded mutants.  Each is a mistake a kernel can make; each must leave the bound by >= 10x on some element and stay under the old budget.
def _conv_parts(net, name):
    L = net.by_name(name)
    xs = net.inputs(L)
    return L, xs, LY._weights(L, net.w, F64)


def _verdict(net, L, got, num=LY.Numerics("f32", "f32"), xs=None):
    xs = net.inputs(L) if xs is None else xs
    ref, bnd = LY.bound(L, xs, net.w, num)
    wst = LY.compare(L.name, got, ref, bnd)
    e_layer = relerr(got.numpy(), ref.numpy())
    e_net = None
    if e_layer >= 1e-3:      # not hidden at the layer itself: the rest of the network has to hide it
        out = LY.chain(net.layers, net.frames, net.w, F64, override={L.name: got}, start={k: v for k, v in net.t64.items()
                                                                                         if k in _before(net, L.name)})[net.out]
        e_net = relerr(out.numpy(), net.t64[net.out].numpy())
    return wst, e_layer, e_net


def _before(net, name):
    names = ["frames"] + [L.name for L in net.layers]
    return set(names[:names.index(name)])


def _assert_mutant(tag, wst, e_layer, e_net):
    print(f"mutant {tag}: {wst.layer} worst |delta|/bound {wst.ratio:.3g} at (image, y, x, channel) {wst.index}; relerr layer {e_layer:.2e}"
          + ("" if e_net is None else f", network output {e_net:.2e}"))
    assert wst.ratio >= 10.0, (tag, wst)
    assert min(e_layer, 1.0 if e_net is None else e_net) < 1e-3, (tag, e_layer, e_net)      # the max-normalised check would have passed it


def test_mutant_replicate_instead_of_zero_padding(mono):
    """the right halo column of one 16-channel chunk holds the edge pixel instead of zero.  (Replicated padding on every border of every channel
    moves the network output by 1e-2 and more in any layer of either network: that the network tests do see.)"""
    L, (x,), ((wt, b),) = _conv_parts(mono, "enc/res5_1/conv2")
    xp = F.pad(x, (1, 1, 1, 1))
    xp[:, :16, 1:-1, -1] = x[:, :16, :, -1]
    got = F.elu(F.conv2d(xp, wt, b, stride=L.stride))
    _assert_mutant("replicate padding", *_verdict(mono, L, got))


def test_mutant_one_tap_zeroed_for_one_output_channel(mono):
    L, (x,), ((wt, b),) = _conv_parts(mono, "enc/res5_1/conv2")
    wt = wt.clone()
    wt[17, :, 1, 2] = 0                      # (the tap right of the centre: on the 2 x 4 map it reads real pixels in three columns of four)
    got = F.elu(F.conv2d(F.pad(x, (1, 1, 1, 1)), wt, b, stride=L.stride))
    _assert_mutant("tap zeroed", *_verdict(mono, L, got))


def test_mutant_one_input_channel_of_one_tap_dropped_on_the_last_two_rows(mono):
    L, (x,), ((wt, b),) = _conv_parts(mono, "enc/res4_2/conv2")
    ref = F.elu(F.conv2d(F.pad(x, (1, 1, 1, 1)), wt, b, stride=L.stride))
    wt = wt.clone()
    wt[:, 5, 0, 1] = 0                       # (the tap above the centre: real pixels on the last two of the four output rows)
    got = ref.clone()
    got[:, :, -2:, :] = F.elu(F.conv2d(F.pad(x, (1, 1, 1, 1)), wt, b, stride=L.stride))[:, :, -2:, :]
    assert torch.equal(got[:, :, :-2], ref[:, :, :-2]) and not torch.equal(got, ref)
    _assert_mutant("channel of a tap dropped on the last rows", *_verdict(mono, L, got))


def test_mutant_last_image_reads_the_first_row_of_image_0(mono):
    """the bottom padding row of the LAST image of the pass is not zero: the taps that reach it read what lies behind the image in a ring of
    images, the first row of image 0 (one 16-channel chunk; all 512 channels move the network output by 4e-3)"""
    L, (x,), ((wt, b),) = _conv_parts(mono, "enc/res5_1/conv2")
    xp = F.pad(x, (1, 1, 1, 1))
    xp[-1, :16, -1, 1:-1] = x[0, :16, 0, :]
    got = F.elu(F.conv2d(xp, wt, b, stride=L.stride))
    wst, e_layer, e_net = _verdict(mono, L, got)
    assert wst.index[0] == x.shape[0] - 1
    _assert_mutant("last image's padding row from image 0", wst, e_layer, e_net)


@pytest.mark.parametrize("scheme", ["bf16x2", "f16x2"])
def test_mutant_low_weight_plane_dropped_for_16_output_channels(scheme, mono):
    """the weights of 16 output channels reduced to their high plane: bf16 hi of the bf16 x 2 scheme, fp16 hi of w * 2^k of the HS scheme
    (split_fmt.hpp).  Checked against THAT scheme's bound, on the stems (short reductions, K = 147 and K = 27, where a weight's rounding is
    not buried under the accumulation term of the bound)."""
    if scheme == "bf16x2":
        net = mono
        L, (x,), ((wt, b),) = _conv_parts(net, "enc/conv1")
        wm = wt.clone()
        wm[16:32] = wt[16:32].float().bfloat16().double()
        got = F.elu(F.conv2d(F.pad(x, (3, 3, 3, 3)), wm, b, stride=2))
    else:
        if "fcn8s" not in _nets:
            _nets["fcn8s"] = Net("fcn8s")
        net = _nets["fcn8s"]
        L, (x,), ((wt, b),) = _conv_parts(net, "conv1_1")
        wm = wt.clone()
        k = 2.0 ** (12 - np.floor(np.log2(float(wt.abs().max()))))          # max |w 2^k| in [2^12, 2^13)
        wm[16:32] = (wt[16:32] * k).half().double() / k
        got = F.relu(F.conv2d(x, wm, b, padding=1))
    fmt = {"bf16x2": "bf16x2", "f16x2": "hs"}[scheme]
    wst, e_layer, e_net = _verdict(net, L, got, LY.Numerics(scheme, fmt))
    assert 16 <= wst.index[3] < 32
    _assert_mutant(f"low weight plane dropped ({scheme})", wst, e_layer, e_net)


def test_mutant_shortcut_of_a_strided_block_read_at_stride_1(mono):
    """one channel octet (a 16-byte run of the gather) of the projection shortcut of the last strided block is read at pixel (y, x) instead of
    (2y, 2x).  (All 2048 channels move the network output by 1.5e-2: that the network tests do see.)"""
    L = mono.by_name("enc/res5_3/conv3")
    assert L.srcs[1].stride == 2
    xs = mono.inputs(L)
    (w3, b3), (wp, bp) = LY._weights(L, mono.w, F64)
    h, w_ = xs[0].shape[2:]
    good = F.conv2d(xs[1][:, 8:], wp[:, 8:], None, stride=2)
    bad = F.conv2d(xs[1][:, :8], wp[:, :8], bp)[:, :, :h, :w_]
    got = F.elu(F.conv2d(xs[0], w3, b3) + good + bad)
    _assert_mutant("shortcut at stride 1", *_verdict(mono, L, got))


def test_mutant_upsampled_source_of_an_iconv_read_without_the_upsample(mono):
    """the centre tap of ONE output channel of iconv3 reads the disparity source at pixel (y, x) instead of (y // 2, x // 2) (nothing beyond the
    source).  (The same for all 64 output channels moves the raw disparity by 8e-3, for all nine taps by 1.7e-2: that the network tests see.)"""
    L = mono.by_name("dec/iconv3")
    assert L.srcs[2].up and L.srcs[2].name == "dec/disp4"
    xs = mono.inputs(L)
    (wt, b), = LY._weights(L, mono.w, F64)
    d = xs[2]
    right = nets._Mono.up(d)
    wrong = F.pad(d, (0, d.shape[3], 0, d.shape[2]))
    pre = F.conv2d(F.pad(torch.cat([xs[0], xs[1], right], 1), (1, 1, 1, 1)), wt, b)
    c0, co = xs[0].shape[1] + xs[1].shape[1], 40
    pre[:, co] += (wt[co, c0:c0 + 2, 1, 1].view(1, 2, 1, 1) * (wrong - right)).sum(1)
    _assert_mutant("iconv source not upsampled", *_verdict(mono, L, F.elu(pre)))


# ------------------------------------------------------------------------------------------------------------------------------
# mistakes that need a frame size that is no power of two (or a pass fed fewer frames than the handle holds).  Each is written as the tile logic a
# kernel would have and run on the SAME layer twice: at the old geometry (GEOM), where it must be an exact no-op (torch.equal with the correct
# output: the cases at power-of-two sizes cannot see it), and at the new one (GEOM_ODD), where it must leave the bound by >= 10x and stay under the
# max-normalised budget.  Each is confined to a channel octet / chunk and to the 16 output columns of one MFMA fragment (or less): wider, the network
# output moves by 2e-3 .. 7e-3 and the network tests see it too (the figures are in the docstrings).
_odd_nets = {}


def _odd(key):
    if key not in _odd_nets:
        _odd_nets[key] = Net(GEOM_ODD[key][0], odd=key)
    return _odd_nets[key]


def _old_and_new(tag, old, new, name, mutate):
    """mutate(L, xs, wbs, ref, net) -> the mutated output of layer ``name`` (ref: the correct float64 output of the same inputs)"""
    for net in (old, new):
        L, xs, wbs = _conv_parts(net, name)
        ref = LY.evaluate(L, xs, net.w, F64)
        got = mutate(L, xs, wbs, ref, net)
        if net is old:
            assert torch.equal(got, ref), tag
            print(f"\nmutant {tag}: a no-op on the {tuple(ref.shape[2:])} map of {name} at {GEOM[old.key][0]}x{GEOM[old.key][1]}")
        else:
            assert not torch.equal(got, ref), tag
            wst, e_layer, e_net = _verdict(net, L, got)
            print(f"mutant {tag}: on the {tuple(ref.shape[2:])} map of {name}:")
            _assert_mutant(tag, wst, e_layer, e_net)
    return wst


def _conv3(L, x, wt, b):
    return F.elu(F.conv2d(F.pad(x, (1, 1, 1, 1)), wt, b, stride=L.stride))


def test_mutant_top_halo_of_a_partial_row_tile_taken_as_image_border(mono):
    """row tiles of TH = min(H, 16) rows: the PARTIAL tile behind full ones -- rows 16 .. 23 of a 24-row map, the second row tile -- loads its
    top halo row as if it were the image border (zero), for one channel octet and the 16 output columns of one fragment.  A map of 2^n rows is
    one tile or full tiles only: the 8-row map at 64x128, and the 32-row map res3 has at 256x512, which the mistake leaves alone as well
    (a mistake in the top halo of EVERY tile behind the first the 256x512 cases would see).  (A whole 16-channel chunk moves the network
    output by 2.0e-3, with all 128 output channels by 7.0e-3: that the network tests see.)"""
    def mutate(L, xs, wbs, ref, net):
        (x,), ((wt, b),) = xs, wbs
        H, got = x.shape[2], ref.clone()
        TH = min(H, 16)
        for y0 in range(TH, H, TH):
            if y0 + TH > H:
                xt = x.clone()
                xt[:, :8, y0 - 1] = 0
                got[:, :16, y0] = _conv3(L, xt, wt, b)[:, :16, y0]
        return got
    new = _odd("192x256")
    wst = _old_and_new("top halo of the partial row tile", mono, new, "enc/res3_1/conv2", mutate)
    assert wst.index[1] == 16 and wst.index[3] < 16
    # two full row tiles (the res3 map of the 256x512 cases is 32 rows high): the same 24 rows and 8 more
    L, (x,), ((wt, b),) = _conv_parts(new, "enc/res3_1/conv2")
    x32 = torch.cat([x, x[:, :, :8]], 2)
    ref32 = _conv3(L, x32, wt, b)
    assert torch.equal(mutate(L, (x32,), ((wt, b),), ref32, new), ref32)
    print("mutant top halo of the partial row tile: a no-op on a 32-row map (two full tiles)")


def test_mutant_bottom_halo_below_a_partial_row_tile_is_the_next_image(mono):
    """the bottom halo row is zeroed where a tile ENDS on the last row (y0 + TH == H) instead of where it reaches it (>=): below the partial
    tile of rows 16 .. 23 the kernel reads row 24 of the image, which in memory is the first row of the next image of the pass (one channel octet,
    16 output columns; the last image would read behind the tensor, so the images before it).  (A 16-channel chunk and all 128 output channels:
    1.9e-3 at the network output.)"""
    def mutate(L, xs, wbs, ref, net):
        (x,), ((wt, b),) = xs, wbs
        N, H, got = x.shape[0], x.shape[2], ref.clone()
        TH = min(H, 16)
        for y0 in range(0, H, TH):
            if y0 + TH > H:
                xp = F.pad(x, (1, 1, 1, 1))
                xp[:N - 1, :8, H + 1, 1:-1] = x[1:, :8, 0, :]
                got[:N - 1, :16, H - 1] = F.elu(F.conv2d(xp, wt, b, stride=L.stride))[:N - 1, :16, H - 1]
        return got
    wst = _old_and_new("bottom halo below the partial tile", mono, _odd("192x256"), "enc/res3_1/conv2", mutate)
    assert wst.index[0] == 0 and wst.index[1] == 23 and wst.index[3] < 16


def test_mutant_k_step_dropped_in_the_last_partial_gemm_tile(mono):
    """a 1x1 layer as a GEMM of M = N H W rows in tiles of 256: for the rows of a last PARTIAL tile the k-loop of ONE output column ends one
    8-channel MFMA step early.  M = 4 * 8 * 16 = 512 at 64x128; 2 * 40 * 24 = 1920 = 7.5 tiles at 320x192 (of the stride-1 1x1 layers only those
    of res3 have a whole number of tiles at the old size and a partial one at a new one; of the other GPU cases at power-of-two heights only 64x448,
two images, has such a remainder there: M = 896).  (The 16 columns of a fragment: 1.6e-3 at the
    network output, a 32-channel k-chunk with them 3.5e-3.)"""
    def mutate(L, xs, wbs, ref, net):
        (x,), ((wt, b),) = xs, wbs
        N, C, H, W = x.shape
        M = N * H * W
        rows = x.permute(0, 2, 3, 1).reshape(M, C)
        got = ref.permute(0, 2, 3, 1).reshape(M, -1).clone()
        for m0 in range(0, M, 256):
            if m0 + 256 > M:
                got[m0:, :1] = F.elu(rows[m0:, :C - 8] @ wt[:1, :C - 8, 0, 0].T + b[:1])
        return got.reshape(N, H, W, -1).permute(0, 3, 1, 2).contiguous()
    wst = _old_and_new("k-step dropped in the GEMM remainder", mono, _odd("320x192"), "enc/res3_3/conv1", mutate)
    n, y, x_, c = wst.index
    assert (n * 40 + y) * 24 + x_ >= 1792 and c == 0


def test_mutant_unpaired_last_source_row_of_a_folded_upconv_clamped_one_row_short(mono):
    """the folded upconv walks its SOURCE rows in pairs; the row an odd-height source leaves over is read at min(y, H - 2), clamped at 0 (one
    16-channel chunk, one 64-channel output pass).  The 1x2 source of upconv6 at 64x128 is its own clamp, the 3x4 source at 192x256 reads row 1 for
    row 2.  (All 512 output channels: 2.1e-3 at the network output.)"""
    def mutate(L, xs, wbs, ref, net):
        (x,), ((wt, b),) = xs, wbs
        H, src, got = x.shape[2], x.clone(), ref.clone()
        for y in range(H - H % 2, H):
            src[:, :16, y] = x[:, :16, min(y, max(H - 2, 0))]
        got[:, :64] = _conv3(L, nets._Mono.up(src), wt, b)[:, :64]
        return got
    L = mono.by_name("dec/upconv6")
    assert L.srcs[0].up and _odd("192x256").t64[L.srcs[0].name].shape[2] == 3 and mono.t64[L.srcs[0].name].shape[2] == 1
    wst = _old_and_new("odd source row of the folded upconv", mono, _odd("192x256"), "dec/upconv6", mutate)
    assert wst.index[1] >= 3 and wst.index[3] < 64


def test_mutant_images_the_pass_was_not_fed_counted_as_real(mono):
    """a handle that holds more images than the pass was fed: the test 'is this the last image' uses the handle's count, so the bottom padding row
    of the last FED image is not zero but the first row of the slot behind it, which holds an image of an earlier pass -- scripts/layer_check.py runs
    such a pass before a partial one; in a fresh, zero-filled arena the mistake would read zeros and pass -- (one channel octet, 16
    output columns).  With as many frames fed as held -- every case before the partial pass -- the two counts agree.  (A 16-channel chunk and all
    128 output channels: 2.1e-3 at the network output.)"""
    held = {id(mono): mono.frames.shape[0], id(_odd("192x256")): 2 * _odd("192x256").frames.shape[0]}

    def mutate(L, xs, wbs, ref, net):
        (x,), ((wt, b),) = xs, wbs
        N, got = x.shape[0], ref.clone()
        if held[id(net)] > N:
            stale = x[0]                     # (what an earlier pass left in slot N: an image's activations of the same layer)
            xp = F.pad(x, (1, 1, 1, 1))
            xp[N - 1, :8, -1, 1:-1] = stale[:8, 0, :]
            got[N - 1, :16, -1] = F.elu(F.conv2d(xp, wt, b, stride=L.stride))[N - 1, :16, -1]
        return got
    wst = _old_and_new("images beyond those fed counted as real", mono, _odd("192x256"), "enc/res3_1/conv2", mutate)
    assert wst.index[0] == _odd("192x256").frames.shape[0] - 1 and wst.index[1] == 23


# ------------------------------------------------------------------------------------------------------------------------------
def _layer_check_script():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("layer_check", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts",
                                                                              "layer_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_extent_requirements_of_the_gpu_cases():
    """the predicates the GPU cases assert extents with hold on the maps they are named for and on none of a power-of-two frame; every
    192x256 case on a split engine requires its stem, its direct kernel on a partial row tile and (monodepth) the folded upconv6 / upconv5"""
    LC = _layer_check_script()
    part, src, small = (LC.EXTENT[k] for k in ("partial row tile after full ones", "source 3, 5 or 6 rows high", "3 or 5 rows or columns"))
    assert part(24, 32) and part(40, 24) and part(20, 12) and not any(part(h, 32) for h in (1, 2, 4, 8, 12, 16, 32, 48, 64, 96, 128, 256, 512))
    assert src(6, 8) and src(12, 16) and src(10, 6) and not any(src(h, 8) for h in (2, 4, 8, 16, 24, 32, 64, 128, 256, 512))
    assert small(3, 4) and small(5, 3) and small(3, 1) and not any(small(h, 2 * h) for h in (1, 2, 4, 6, 8, 16))
    ids = [LC.case_id(c) for c in LC.CASES]
    assert len(ids) == len(set(ids))
    seen = 0
    for c in LC.CASES:
        if (c["H"], c["W"]) != (192, 256) or c["precision"] == "f32":
            continue
        seen += 1
        assert any("conv_stem" in f for f in c["need"]), LC.case_id(c)
        assert any("conv_direct" in lab and e == "partial row tile after full ones" for lab, _, e in c["need_at"]), LC.case_id(c)
        if c["net"] == "resnet50":
            assert {"dec/upconv6", "dec/upconv5"} <= {pre for _, pre, e in c["need_at"] if e == "source 3, 5 or 6 rows high"}, LC.case_id(c)
        if c["frames"] > 1:
            fr = LC._frames(c["frames"], c["H"], c["W"], seed=c["H"] + c["W"] + c["frames"])
            assert all(not np.array_equal(fr[i], fr[j]) for i in range(len(fr)) for j in range(i))
    assert seen == 9 + 4 + 4 and sum(c["max_batch"] > c["frames"] for c in LC.CASES) == 4
