"""GPU: results do not depend on the hidden state a call runs in -- what the arenas held when they were bound (A), whether the planner
reuses activation memory (B), what earlier calls left behind (C) and how many workgroups the persistent kernels run on (D).  All four are
reference-free bit-identity properties: two runs that differ in the state alone must agree byte for byte.  A defect of this kind -- a kernel
that reads a padded channel, a row of a partial tile, an image beyond B or a partial-sum slot it never wrote -- hides below the 1e-3 to 1e-5
bounds of the parity tests as long as the memory happens to hold zeros; here the memory holds NaNs (0xFF), huge finite values (0x7B) or the
stale data of another frame and another network.  D is anchored to the CPU oracle as well, at the bounds the parity tests already use.

Every engine is built directly (no engine cache: the state of an engine is the subject), from one shared set of seeded weights; the outputs
of the zero-filled, reuse-on engine of a configuration are computed once and shared by A and B."""
import numpy as np
import pytest
import torch

from oracle import nets
from semantic_depth_amd import _lib as L
from semantic_depth_amd import weights as Wt
from semantic_depth_amd.engine import Camera, Engine, FP16_PLANE_ENGINES, RangeError, RoadWidthParams
from gpu_common import dev, relerr
from test_gpu_geometries import _frames as _block_frames      # noisy 8 x 8 blocks (device tensor)
from test_gpu_nets import _frames                              # uniform noise (numpy)

pytestmark = pytest.mark.gpu

KEEP = "SEMDEPTH_KEEP_ACTIVATIONS"
FILLS = [0xFF, 0x7B]       # NaN as f32 / bf16 / fp16; large but finite in all three (fp16 61280, bf16 / f32 ~1.3e36): what fmaxf / v_med3 drop from a NaN stays visible

# (precision, monodepth encoder, H, W, max_batch, small_batch level)
PRECISIONS = ["f32", "bf16x3", "f16x2", "bf16x2", "plan"]
CONFIGS = ([(p, "resnet50", 64, 128, 3, 0) for p in PRECISIONS] + [(p, "vgg", 128, 256, 3, 0) for p in PRECISIONS] +
           # the partial-sum scratch of the split-K GEMM layers (level 1) and of the chunk-split direct 3x3 layers (level 2: they exist from 128 x 256 on)
           [("f16x2", "resnet50", 64, 128, 1, 1), ("f16x2", "resnet50", 64, 128, 1, 2), ("f16x2", "resnet50", 128, 256, 1, 2)])
_id = lambda c: "-".join(str(v) for v in c)

_weights_cache, _ref_cache, _oracle_cache = {}, {}, {}


def _weights(which, **kw):
    """seeded weight dicts, generated once per module: "fcn" (seed 1) or a monodepth encoder (seed 2), as the neighbouring parity tests make them"""
    key = (which, tuple(sorted(kw.items())))
    if key not in _weights_cache:
        if which == "fcn":
            _weights_cache[key] = Wt.make_fcn8s_weights(1, **(kw or dict(decoder_std=0.05, bias_std=0.1)))
        else:
            _weights_cache[key] = Wt.make_monodepth_weights(which, **(kw or dict(seed=2, gain=1.5 if which == "vgg" else 1.0, bias_std=0.05)))
    return _weights_cache[key]


def _build(cfg, fill=0, wf=None, wm=None):
    prec, enc, H, W, mb, sb = cfg
    eng = Engine(H, W, mb, enc, precision=prec, small_batch=sb, arena_fill=fill)
    eng.load_weights(L.SD_NET_FCN8S, wf if wf is not None else _weights("fcn"))
    eng.load_weights(L.SD_NET_MONODEPTH, wm if wm is not None else _weights(enc))
    return eng


def _guard(out, key, call):
    """a RangeError (the clamp counters count NaNs) is a finding to report beside the outputs, not the end of the comparison"""
    try:
        return call()
    except RangeError as e:
        out[key] = "RangeError: " + str(e)[:60]
        return None


def _net_outputs(eng, fr, batches):
    """logits, the three masks, the raw disparity pair and the post-processed disparity of one call per batch size, then the clamp count"""
    out = {}
    for B in batches:
        f = fr[:B].contiguous()
        seg = _guard(out, f"B{B}/fcn_error", lambda: eng.fcn8s_forward(f, want_logits=True))
        for k in ("logits", "road", "fence", "argmax"):
            out[f"B{B}/{k}"] = seg[k].clone() if seg else None
        mono = _guard(out, f"B{B}/mono_error", lambda: eng.monodepth_forward(f, want_raw=True))
        out[f"B{B}/disp_pp"], out[f"B{B}/disp_raw"] = (mono[0].clone(), mono[1].clone()) if mono else (None, None)
    out["saturation_count"] = eng.saturation_count()
    _guard(out, "check_range", eng.check_range)
    return out


def _camera(H, W, disp_pp):
    """the camera of test_gpu_geometries.py"""
    return Camera(W / 2 - 0.5, H / 2 - 0.5, 10.0 * float(disp_pp.median()) * W, 1.0, float(W))


def _path_outputs(eng, fr, cam):
    """process_batch with both chains: the records, the gathered road / fence clouds and the denoised ones (their valid prefixes: the rest of a
    cloud buffer is never written)"""
    B = fr.shape[0]
    out = {}
    r = _guard(out, "path_error", lambda: eng.process_batch(fr, [cam] * B, RoadWidthParams(), approach="both", want_final=True))
    if r is None:
        return out
    out.update(records=r["records"].clone(), f2f=r["f2f"].clone(), disp_pp=r["disp_pp"].clone(), road=r["seg"]["road"].clone(),
               fence=r["seg"]["fence"].clone(), n_road=r["fuse"]["n_road"].clone(), n_fence=r["fuse"]["n_fence"].clone(), n_road_final=r["road_final"]["n"].clone())
    cap = r["fuse"]["road_xyz"].shape[1]
    clip = lambda n: max(0, min(int(n), cap))
    counts = Engine.f2f_records(r["f2f"])["counts"]
    for b in range(B):
        for k in ("road", "fence"):
            n = clip(r["fuse"][f"n_{k}"][b])
            out[f"{k}_xyz/{b}"], out[f"{k}_rgb/{b}"] = r["fuse"][f"{k}_xyz"][b, :n].clone(), r["fuse"][f"{k}_rgb"][b, :n].clone()
        n = clip(r["road_final"]["n"][b])
        out[f"road_final_xyz/{b}"], out[f"road_final_rgb/{b}"] = r["road_final"]["xyz"][b, :n].clone(), r["road_final"]["rgb"][b, :n].clone()
        for side, n in (("left", clip(counts[b][5])), ("right", clip(counts[b][6]))):
            out[f"fence_{side}_xyz/{b}"], out[f"fence_{side}_rgb/{b}"] = r["fence_final"][f"{side}_xyz"][b, :n].clone(), r["fence_final"][f"{side}_rgb"][b, :n].clone()
    out["saturation_count"] = eng.saturation_count()
    _guard(out, "check_range", eng.check_range)
    return out


def _bits(t):
    return t.contiguous().view(torch.uint8)      # (bytes: a NaN equals itself, -0.0 differs from 0.0)


def _differences(got, ref):
    """[(key, what differs)] over the keys of both runs; tensors are compared byte for byte (torch.equal on their bytes)"""
    bad = []
    for k in sorted(set(ref) | set(got)):
        g, r = got.get(k), ref.get(k)
        if isinstance(r, torch.Tensor) and isinstance(g, torch.Tensor):
            if g.shape != r.shape or g.dtype != r.dtype:
                bad.append((k, f"shape / dtype {tuple(g.shape)} {g.dtype} != {tuple(r.shape)} {r.dtype}"))
            elif not torch.equal(_bits(g), _bits(r)):
                ne = (g != r) | (g != g) if g.is_floating_point() else (g != r)
                note = f"{int(ne.sum())} of {g.numel()} elements differ"
                if g.is_floating_point():
                    note += f", {int(torch.isnan(g).sum())} NaN, max |delta| {float((g.double() - r.double()).abs().nan_to_num(0.0).max()):.3e}"
                bad.append((k, note))
        elif isinstance(r, torch.Tensor) or isinstance(g, torch.Tensor) or g != r:
            bad.append((k, f"{g!r} != {r!r}"))
    return bad


def _reference(cfg, monkeypatch):
    """the outputs of the zero-filled engine of a configuration with the production placement (arena reuse on), computed once"""
    if cfg not in _ref_cache:
        monkeypatch.delenv(KEEP, raising=False)
        prec, enc, H, W, mb, sb = cfg
        fr = dev(_frames(mb, H, W, seed=3))
        eng = _build(cfg)
        out = _net_outputs(eng, fr, sorted({1, mb}))
        _ref_cache[cfg] = dict(out=out, workspace=eng.bytes["workspace"], plan=eng.small_batch_plan(), frames=fr)
        eng.close()
        assert out["saturation_count"] == 0 and "check_range" not in out, out           # the weights fit the fp16 planes: every clamp below is spurious
        for k, v in out.items():
            if isinstance(v, torch.Tensor) and v.is_floating_point():
                assert bool(torch.isfinite(v).all()), k
        assert float(out[f"B{mb}/disp_raw"].std()) > 1e-4 and float(out[f"B{mb}/logits"].std()) > 1e-4      # not constant maps
    return _ref_cache[cfg]


# ------------------------------------------------------------------------------------------------------------------- A. poisoned arenas
@pytest.mark.parametrize("fill", FILLS, ids=hex)
@pytest.mark.parametrize("cfg", CONFIGS, ids=_id)
def test_outputs_do_not_depend_on_what_the_arenas_held(cfg, fill, monkeypatch):
    """sd_bind_memory: "the arenas may hold anything".  The weight arenas and the workspace are filled with 0xFF (NaN in every plane format) or 0x7B
    (huge, finite) before they are bound; a call of one frame on the handle of three (the slots of images 1, 2 are still poison), then a call of
    three.  Everything equals the zero-filled engine's bit for bit, and nothing was clamped."""
    monkeypatch.delenv(KEEP, raising=False)
    ref = _reference(cfg, monkeypatch)
    prec, enc, H, W, mb, sb = cfg
    if sb:
        plan = ref["plan"]
        assert plan["fcn8s"] or plan["monodepth"], plan         # the partial-sum scratch is in play
        if sb == 2 and H * W >= 128 * 256:
            assert plan["fcn8s"].get("conv4_2", 1) > 1, plan      # ... that of a chunk-split direct 3x3 layer too
    eng = _build(cfg, fill=fill)
    got = _net_outputs(eng, ref["frames"], sorted({1, mb}))
    eng.close()
    bad = _differences(got, ref["out"])
    assert not bad, (cfg, hex(fill), bad)
    assert got["saturation_count"] == 0
    if prec in ("f16x2", "plan"):
        assert prec in FP16_PLANE_ENGINES and "check_range" not in got


@pytest.mark.parametrize("fill", FILLS, ids=hex)
@pytest.mark.parametrize("precision", ["f16x2"])
def test_whole_path_does_not_depend_on_what_the_arenas_held(precision, fill, monkeypatch):
    """process_batch (both chains) in poisoned arenas: the workspace regions of the fuse kernels and of the road / fence chains.  Records and clouds
    equal the zero-filled run byte for byte."""
    monkeypatch.delenv(KEEP, raising=False)
    cfg = (precision, "resnet50", 64, 128, 3, 0)
    H, W, B = 64, 128, 3
    fr = dev(_frames(B, H, W, seed=3))
    outs = {}
    cam = None
    for f in (0, fill):
        eng = _build(cfg, fill=f)
        pp = eng.monodepth_forward(fr)                 # (both engines run the same calls: the history is test C's subject)
        cam = cam or _camera(H, W, pp)
        outs[f] = _path_outputs(eng, fr, cam)
        eng.close()
    assert "path_error" not in outs[0] and int(outs[0]["n_road"].min()) > 0, {k: v for k, v in outs[0].items() if not isinstance(v, torch.Tensor) or v.numel() <= 8}
    print("points: road", outs[0]["n_road"].tolist(), "fence", outs[0]["n_fence"].tolist(), "road final", outs[0]["n_road_final"].tolist())
    bad = _differences(outs[fill], outs[0])
    assert not bad, (hex(fill), bad)
    assert outs[fill]["saturation_count"] == 0 and "check_range" not in outs[fill]


# --------------------------------------------------------------------------------------------------------------- B. reuse versus no reuse
@pytest.mark.parametrize("cfg", CONFIGS, ids=_id)
def test_arena_reuse_changes_addresses_never_bits(cfg, monkeypatch):
    """plan.cpp places activations first-fit over lifetimes; SEMDEPTH_KEEP_ACTIVATIONS=1 (the layer-by-layer tests run under it) gives every tensor
    memory of its own.  The two placements differ in addresses alone."""
    monkeypatch.delenv(KEEP, raising=False)
    ref = _reference(cfg, monkeypatch)               # reuse on
    monkeypatch.setenv(KEEP, "1")
    eng = _build(cfg)
    got = _net_outputs(eng, ref["frames"], sorted({1, cfg[4]}))
    kept = eng.bytes["workspace"]
    eng.close()
    assert ref["workspace"] < kept, (ref["workspace"], kept)          # reuse did happen on the reference side: the comparison is of two placements
    bad = _differences(got, ref["out"])
    assert not bad, (cfg, bad)


# --------------------------------------------------------------------------------------------------------------------- C. call history
@pytest.mark.parametrize("precision,level", [("bf16x3", 0), ("f16x2", 0), ("f16x2", 2)])
def test_a_call_does_not_depend_on_the_calls_before_it(precision, level, monkeypatch):
    """reuse on: every region holds the stale data of an earlier frame or of the other network.  FCN-8s and monodepth on frames A (noisy blocks:
    another scale than B's), then FCN-8s, monodepth and process_batch on frames B -- against a fresh engine that only ever saw B."""
    monkeypatch.delenv(KEEP, raising=False)
    H, W, B = 128, 256, 2
    cfg = (precision, "resnet50", H, W, B, level)
    fa, fb = _block_frames(B, H, W, seed=11), dev(_frames(B, H, W, seed=12))
    assert not torch.equal(fa, fb)

    def b_calls(eng, cam):
        out = _net_outputs(eng, fb, [B])
        cam = cam or _camera(H, W, out[f"B{B}/disp_pp"])
        out.update({"path/" + k: v for k, v in _path_outputs(eng, fb, cam).items()})
        return out, cam

    fresh = _build(cfg)
    if level:
        assert fresh.small_batch_plan()["fcn8s"].get("conv4_2", 1) > 1, fresh.small_batch_plan()
    ref, cam = b_calls(fresh, None)
    fresh.close()
    used = _build(cfg)
    used.fcn8s_forward(fa, want_logits=True)
    used.monodepth_forward(fa, want_raw=True)
    got, _ = b_calls(used, cam)
    used.close()
    assert ref["saturation_count"] == 0 and int(ref["path/n_road"].min()) > 0
    bad = _differences(got, ref)
    assert not bad, (cfg, bad)


# --------------------------------------------------------------------------------------------------------------------- D. reserved CUs
def _conv_direct_items(W, H, images, nsplit, th=16):
    return (W // 32) * ((H + th - 1) // th) * images * nsplit          # kernels.hpp conv_direct_items: 32 x th pixel tiles of every 64-channel pass


@pytest.mark.parametrize("precision", ["bf16x3", "f16x2", "bf16x2"])
def test_reserved_cus_change_the_grid_never_the_result(precision, monkeypatch):
    """sd_set_reserved_cus: "Results do not depend on it".  It sets the workgroup count of the persistent kernels (conv_direct, conv_direct3,
    conv_stem, dec_tail) and so how many tiles one workgroup walks and whether its double buffers swap.  256 x 512, B = 2: conv1_2 of FCN-8s has 512
    tiles -- 4 per workgroup with 128 CUs reserved on the 256-CU part, 2 with none, an uneven 2 / 3 with 1 or 37."""
    monkeypatch.delenv(KEEP, raising=False)
    monkeypatch.setenv("SEMDEPTH_PROFILE_VERBOSE", "1")        # (latched at sd_create: profile buckets carry the instantiation's name)
    H, W, B = 256, 512, 2
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = _conv_direct_items(W, H, B, 1)
    assert tiles > 2 * (cus - 128) > 0 and -(-tiles // cus) != -(-tiles // (cus - 128)), (tiles, cus)
    eng = _build((precision, "resnet50", H, W, B, 0))
    fr = dev(_frames(B, H, W, seed=5))
    assert eng.lib.sd_set_reserved_cus(eng.h, 129) == L.SD_ERR_INVALID and eng.lib.sd_set_reserved_cus(eng.h, -1) == L.SD_ERR_INVALID
    cam = None

    def run():
        nonlocal cam
        out = {}
        out["logits"] = eng.fcn8s_forward(fr, want_logits=True)["logits"].clone()
        pp, raw = eng.monodepth_forward(fr, want_raw=True)
        out["disp_raw"] = raw.clone()
        cam = cam or _camera(H, W, pp)
        out["records"] = eng.process_batch(fr, [cam] * B, RoadWidthParams())["records"].clone()
        return out

    eng.reserve_cus(0)
    ref = run()
    assert int(Engine.records(ref["records"])["n_road"].min()) > 0
    for n in (1, 37, 128):
        eng.reserve_cus(n)
        if n == 128:
            eng.profile(True)
        got = run()
        if n == 128:
            kernels = {b["kernel"] for b in eng.profile_read()}
            eng.profile(False)
        bad = _differences(got, ref)
        assert not bad, (precision, n, bad)
    eng.close()
    # not vacuous: the persistent kernels did run.  (dec_tail1 is a launch of the two fp32-grade engines only: the planner builds level 1 of the
    # decoder layer by layer for bf16x2, whose direct kernel then carries those layers)
    wanted = ("conv_direct", "conv_stem") + (("dec_tail1",) if precision in ("bf16x3", "f16x2") else ())
    for prefix in wanted:
        assert any(k.startswith(prefix) for k in kernels), (prefix, sorted(kernels))
    assert len(kernels) < 32, sorted(kernels)                   # (sd_profile_read drops what does not fit its 32 buckets)


def _oracle(H, W, B):
    """the CPU oracle's logits (float64) and raw disparities (float32, as the parity tests hold them) of the anchor case, computed once"""
    key = (H, W, B)
    if key not in _oracle_cache:
        wf, wm = _weights("fcn"), _weights("resnet50", seed=5, bias_std=0.05)
        frn = _frames(B, H, W, seed=H + 3)
        ref_l = nets.fcn8s_forward(frn, wf, dtype=torch.float64)
        ref_d = []
        for i in range(B):
            f = frn[i].astype(np.float32) / 255
            ref_d.append(nets.monodepth_forward(np.stack((f, np.fliplr(f)), 0), wm, "resnet50")[..., 0])
        _oracle_cache[key] = (wf, wm, frn, ref_l, ref_d)
    return _oracle_cache[key]


@pytest.mark.parametrize("precision", ["f16x2", "bf16x3"])
def test_half_the_chip_reserved_still_computes_the_oracles_networks(precision, monkeypatch):
    """the anchor of D: identical bits could be identically wrong.  128 x 256, B = 3, 128 CUs reserved, against the CPU oracle at the bounds the parity
    tests hold these two engines to at this size, none of its own: raw disparity < 1e-5 per frame against nets.monodepth_forward
    (test_folded_upconvs_of_the_three_product_fp16_engine: same weights, same frames), logits < 1e-5 against nets.fcn8s_forward in float64
    (test_bf16x3_is_fp32_grade_against_a_float64_oracle)."""
    monkeypatch.delenv(KEEP, raising=False)
    H, W, B = 128, 256, 3
    wf, wm, frn, ref_l, ref_d = _oracle(H, W, B)
    eng = _build((precision, "resnet50", H, W, B, 0), wf=wf, wm=wm)
    eng.reserve_cus(128)
    lg = eng.fcn8s_forward(dev(frn), want_logits=True)["logits"].cpu().numpy()
    _, raw = eng.monodepth_forward(dev(frn), want_raw=True)
    raw = raw.cpu().numpy()
    assert eng.saturation_count() == 0
    eng.close()
    el = relerr(lg, ref_l)
    ed = [relerr(raw[i], ref_d[i]) for i in range(B)]
    print(precision, "128 CUs reserved: logits vs float64 oracle", el, "raw disparity vs oracle", ed)
    assert el < 1e-5
    assert max(ed) < 1e-5
