"""The disparity-image rule of include/semdepth.h restated in numpy, the cases of tests/golden/disp_image.npz, and the checker that
holds an implementation to that fixture.  Shared by tests/golden/make_disp_image_golden.py (which supplies Pillow's resize and
matplotlib's imsave) and the tests (which never import either: they pass the project's pinned resample).

Every float32 step is explicit: numpy scalars of type np.float32 and float32 arrays only, so no step is silently done in double."""
import numpy as np

F32 = np.float32
MAPS = ("gray", "plasma")


def byte_scale(disp, mult=1.0):
    """steps 1-3 for one [h,w] map: (bytes u8 [h,w], flag)"""
    v = np.asarray(disp, F32) * F32(mult)                               # float32 array times float32 scalar
    assert v.dtype == F32
    fin = np.isfinite(v)
    if fin.any():
        lo, hi = F32(v[fin].min()), F32(v[fin].max())
        with np.errstate(over="ignore"):
            cs = F32(hi - lo)
        if cs == 0:
            cs = F32(1.0)
    else:
        lo, cs = F32(0.0), F32(1.0)
    scale = F32(np.float64(255.0) / np.float64(cs))
    with np.errstate(invalid="ignore", over="ignore"):
        diff = np.where(fin, v, F32(0.0)).astype(F32) - lo
        t = (diff * scale).astype(F32)
    assert diff.dtype == F32 and t.dtype == F32
    t = np.where(t > 0, t, F32(0.0)).astype(F32)                          # (clip; a product that is not a number gives 0)
    t = np.minimum(t, F32(255.0))
    out = (t + F32(0.5)).astype(F32).astype(np.int32).astype(np.uint8)    # add 0.5f, truncate
    out[~fin] = 0
    return out, int(not fin.all())


def colour_index(img8):
    """step 5 for one resized byte image: integer floor"""
    p = np.asarray(img8).astype(np.int64)
    lo8, hi8 = int(p.min()), int(p.max())
    if hi8 == lo8:
        return np.zeros(p.shape, np.int64)
    return np.minimum(255, 256 * (p - lo8) // (hi8 - lo8))


def colour_index_float32(p, lo8, hi8):
    """what matplotlib does with a uint8 image (arrays broadcast): Normalize in float32, then int(x * 256) with 256 -> 255"""
    x = (np.asarray(p).astype(F32) - np.asarray(lo8).astype(F32)) / (np.asarray(hi8).astype(F32) - np.asarray(lo8).astype(F32))
    x = (x * F32(256.0)).astype(F32)
    x = np.where(x == 256, F32(255.0), x)
    return x.astype(np.int64)


def restate(disp, mults, out_h, out_w, table_rgb, resize, mistake=None):
    """the rule for f32 [B,h,w] ``disp``: (images u8 [B,out_h,out_w,3] BGR, flags i32 [B]).  ``table_rgb`` u8 [256,3];
    ``resize(img8 [h,w], out_h, out_w) -> u8 [out_h,out_w]`` is Pillow's bilinear resample (or the project's pinned twin of it).
    ``mistake`` seeds one of MISTAKES (test_disp_image_cpu.py: the checker has to catch each)."""
    disp = np.asarray(disp, F32)
    B, h, w = disp.shape
    mults = [1.0] * B if mults is None else list(mults)
    table = np.asarray(table_rgb, np.uint8)
    if mistake == "identity_gray":
        table = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1) if (table[:, 0] == table[:, 2]).all() else table
    out = np.empty((B, out_h, out_w, 3), np.uint8)
    flags = np.zeros(B, np.int32)
    for b in range(B):
        if mistake == "batch_range":           # one range for the whole batch: frame b scaled inside the stacked maps
            stack = np.concatenate([disp[i] * F32(mults[i]) for i in range(B)], axis=0)
            img8 = byte_scale(stack, 1.0)[0][b * h:(b + 1) * h]
            flags[b] = int(not np.isfinite(disp[b] * F32(mults[b])).all())
        elif mistake == "float64_scale":
            v = disp[b].astype(np.float64) * float(mults[b])
            lo, hi = v.min(), v.max()
            cs = (hi - lo) or 1.0
            img8 = (np.clip((v - lo) * (255.0 / cs), 0, 255) + 0.5).astype(np.uint8)
        else:
            img8, flags[b] = byte_scale(disp[b], mults[b])
        big = img8 if (h, w) == (out_h, out_w) else np.asarray(resize(img8, out_h, out_w), np.uint8)
        idx = colour_index(big)
        if mistake == "round_index":
            p = big.astype(np.int64)
            lo8, hi8 = int(p.min()), int(p.max())
            idx = np.zeros_like(p) if hi8 == lo8 else np.minimum(255, (256 * (p - lo8) + (hi8 - lo8) // 2) // (hi8 - lo8))
        rgb = table[idx]
        out[b] = rgb if mistake == "swap_plasma" and not (table[:, 0] == table[:, 2]).all() else rgb[..., ::-1]
    return out, flags


MISTAKES = ("batch_range", "round_index", "identity_gray", "float64_scale", "swap_plasma")


def boundary_values(lo, hi, count):
    """float32 values inside [lo, hi] whose byte differs between the float32 rule and a float64 one (the product lands on a .5
    boundary on one side only): found by walking the floats next to every boundary"""
    lo, hi = F32(lo), F32(hi)
    scale32 = F32(np.float64(255.0) / np.float64(F32(hi - lo)))
    scale64 = 255.0 / (float(hi) - float(lo))
    found = []
    for k in range(1, 255):
        v = F32((k + 0.5) / scale64 + float(lo))
        for _ in range(4):
            v = np.nextafter(v, F32(-np.inf))
        for _ in range(9):
            b32 = int(F32(F32(F32(v - lo) * scale32) + F32(0.5)))
            b64 = int((float(v) - float(lo)) * scale64 + 0.5)
            if b32 != b64 and lo < v < hi:
                found.append(v)
                break
            v = np.nextafter(v, F32(np.inf))
        if len(found) == count:
            break
    return np.array(found, F32)


def make_cases():
    """name -> dict(disp f32 [B,h,w], mults f32 [B], out_h, out_w): the cases of the fixture, seeded"""
    rng = np.random.default_rng(20240607)

    def rnd(B, h, w, lo=0.0, hi=1.0):
        return (rng.random((B, h, w), dtype=np.float32) * F32(hi - lo) + F32(lo)).astype(F32)

    cases = {}
    cases["up_8x16_20x40"] = dict(disp=rnd(1, 8, 16, 0.002, 0.09), mults=[1.0], out_h=20, out_w=40)
    cases["same_8x16"] = dict(disp=rnd(1, 8, 16, 0.002, 0.09), mults=[3800.0], out_h=8, out_w=16)
    cases["shrink_16x32_5x7"] = dict(disp=rnd(1, 16, 32), mults=[1.0], out_h=5, out_w=7)
    cases["odd_7x13_9x11"] = dict(disp=rnd(1, 7, 13, -4.0, 9.0), mults=[1.0], out_h=9, out_w=11)
    cases["tiny_3x5_1x1"] = dict(disp=rnd(1, 3, 5), mults=[1.0], out_h=1, out_w=1)
    cases["constant"] = dict(disp=np.full((1, 8, 16), 0.0371, F32), mults=[3800.0], out_h=20, out_w=40)
    two = np.where(rng.random((1, 8, 16)) < 0.5, F32(0.01), F32(0.07)).astype(F32)
    cases["two_valued"] = dict(disp=two, mults=[1.0], out_h=20, out_w=40)
    # a fine checkerboard over a weak ramp: every 4 x 4 block of the shrink averages to mid grey, the resized range is narrow
    yy, xx = np.mgrid[0:16, 0:32]
    narrow = (((yy + xx) & 1).astype(F32) + (xx.astype(F32) * F32(0.004)))[None].astype(F32)
    cases["narrow_16x32_4x8"] = dict(disp=narrow, mults=[1.0], out_h=4, out_w=8)
    m = rnd(1, 8, 16, 0.001, 0.12)
    cases["mult_1"] = dict(disp=m, mults=[1.0], out_h=20, out_w=40)
    cases["mult_3800"] = dict(disp=m.copy(), mults=[3800.0], out_h=20, out_w=40)
    b3 = np.concatenate([rnd(1, 8, 16, 0.0, 1e-3), rnd(1, 8, 16, 5.0, 5000.0), rnd(1, 8, 16, -3.0, 2.0)])
    cases["batch3"] = dict(disp=b3, mults=[1.0, 1.0, 3800.0], out_h=20, out_w=40)
    # pixels on the .5 boundaries of the byte scaling, where float32 and float64 arithmetic give different bytes
    edge = rnd(1, 8, 16, 0.011, 0.0899)
    edge[0, 0, 0], edge[0, 0, 1] = F32(0.0107), F32(0.0903)
    bv = boundary_values(edge[0, 0, 0], edge[0, 0, 1], 40)
    assert len(bv) >= 8, len(bv)
    edge.reshape(-1)[2:2 + len(bv)] = bv
    cases["boundary_same"] = dict(disp=edge, mults=[1.0], out_h=8, out_w=16)
    for c in cases.values():
        c["mults"] = np.asarray(c["mults"], F32)
    return cases


def check(impl, golden):
    """run ``impl(disp, mults, out_h, out_w, cmap) -> (images BGR, flags)`` on every case of the loaded fixture ``golden`` for both maps
    and return the list of "<case>/<map>" whose pixels differ from imsave's (or whose flag is set: the fixture has no non-finite value)"""
    bad = []
    for name in [str(n) for n in golden["names"]]:
        disp, mults = golden[name + "/disp"], golden[name + "/mults"]
        out_h, out_w = (int(v) for v in golden[name + "/size"])
        for cmap in MAPS:
            img, flags = impl(disp, mults, out_h, out_w, cmap)
            want = golden["{}/{}".format(name, cmap)]
            if np.asarray(img).shape != want.shape or not np.array_equal(np.asarray(img)[..., ::-1], want) or np.any(np.asarray(flags)):
                bad.append("{}/{}".format(name, cmap))
    return bad
