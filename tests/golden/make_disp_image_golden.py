"""Record tests/golden/disp_image.npz: what scipy.misc.imresize + plt.imsave (semantic_depth.py:681-683) leave for the cases of
tests/disp_image_cases.py.

    python tests/golden/make_disp_image_golden.py

Needs Pillow and matplotlib (recorded with 12.2.0 and 3.10.8).  scipy.misc.imresize is gone from scipy: its byte scaling comes from the
restatement in disp_image_cases.byte_scale (float32 steps, the numpy of the reference's time), the resample is
PIL.Image.fromarray(bytes, 'L').resize((w, h), BILINEAR) as imresize did it, and the colours are read back from the PNG plt.imsave wrote.
The file holds `names`, both colour tables (`table/gray`, `table/plasma`, u8 [256,3] RGB), and per case `<name>/disp`, `<name>/mults`,
`<name>/size` and `<name>/gray`, `<name>/plasma` (u8 [B,out_h,out_w,3] RGB), and the two versions."""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import disp_image_cases as D  # noqa: E402

GOLDEN = os.path.join(HERE, "disp_image.npz")


def pillow_resize(img8, out_h, out_w):
    from PIL import Image
    return np.asarray(Image.fromarray(np.ascontiguousarray(img8, np.uint8), "L").resize((out_w, out_h), Image.BILINEAR))


def imsave_rgb(img8, cmap):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from PIL import Image
    buf = io.BytesIO()
    plt.imsave(buf, img8, cmap=cmap, format="png")
    buf.seek(0)
    rgba = np.asarray(Image.open(buf))
    assert rgba.shape == img8.shape + (4,) and (rgba[..., 3] == 255).all(), rgba.shape
    return rgba[..., :3].copy()


def main():
    import matplotlib
    import PIL
    out = {"pillow_version": np.array(PIL.__version__), "matplotlib_version": np.array(matplotlib.__version__)}
    tables = {m: matplotlib.colormaps[m](np.arange(256), bytes=True)[:, :3].astype(np.uint8) for m in D.MAPS}
    for m in D.MAPS:
        out["table/" + m] = tables[m]
    cases = D.make_cases()
    out["names"] = np.array(list(cases))
    for name, c in cases.items():
        disp, mults, oh, ow = c["disp"], c["mults"], c["out_h"], c["out_w"]
        out[name + "/disp"], out[name + "/mults"], out[name + "/size"] = disp, mults, np.array([oh, ow], np.int32)
        for m in D.MAPS:
            imgs = []
            for b in range(disp.shape[0]):
                img8, flag = D.byte_scale(disp[b], mults[b])
                assert flag == 0
                big = pillow_resize(img8, oh, ow)          # (imresize resizes even to the same size: Pillow copies then)
                imgs.append(imsave_rgb(big, m))
            out["{}/{}".format(name, m)] = np.stack(imgs)
            # the restatement itself agrees with imsave on its own cases, and every seeded mistake shows on at least one
            got, _ = D.restate(disp, mults, oh, ow, tables[m], pillow_resize)
            assert np.array_equal(got[..., ::-1], out["{}/{}".format(name, m)]), (name, m)
    big = pillow_resize(D.byte_scale(cases["narrow_16x32_4x8"]["disp"][0])[0], 4, 8)
    assert big.min() > 0 and big.max() < 255 and big.min() < big.max(), (big.min(), big.max())
    np.savez_compressed(GOLDEN, **out)
    golden = np.load(GOLDEN)
    for mistake in D.MISTAKES:
        bad = D.check(lambda d, mu, oh, ow, m: D.restate(d, mu, oh, ow, tables[m], pillow_resize, mistake), golden)
        assert bad, mistake
        print(mistake, "->", bad)
    assert not D.check(lambda d, mu, oh, ow, m: D.restate(d, mu, oh, ow, tables[m], pillow_resize), golden)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
