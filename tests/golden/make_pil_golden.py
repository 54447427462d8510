"""Record tests/golden/pil_bilinear.npz: Pillow's Image.resize(..., BILINEAR) on the seeded inputs of tests/seg_eval_cases.py.

    python tests/golden/make_pil_golden.py

Needs Pillow (recorded with 12.2.0).  The file holds, per geometry, `<name>/src` and `<name>/dst`, and the Pillow version."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import seg_eval_cases as S  # noqa: E402


def main():
    import PIL
    out = {"pillow_version": np.array(PIL.__version__)}
    for name, (h, w, c, dh, dw) in S.GEOMETRIES.items():
        src = S.source(name)
        out[name + "/src"] = src
        out[name + "/dst"] = S.pillow_resize(src, dh, dw)
    np.savez_compressed(S.GOLDEN, **out)
    print(S.GOLDEN, os.path.getsize(S.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
