"""Cases for the segmentation score (csrc/pil_resample.hpp, host_seg_eval.cpp, seg_eval_gpu.hip, semantic_depth_amd/evaluate.py), shared by
tests/test_seg_eval_cpu.py, tests/test_gpu_seg_eval.py and tests/golden/make_pil_golden.py.

pil_resize_np restates Pillow's ImagingResample (8-bit, bilinear) in numpy, independently of the library, with switches for three seeded
mistakes.  The yardstick of the resample is Pillow itself: tests/golden/pil_bilinear.npz holds Pillow's outputs for GEOMETRIES (the GPU
machine may have no Pillow; the golden travels).  The yardstick of the confusion counts is np.bincount."""
import ctypes as C
import os

import numpy as np

from semantic_depth_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pil_bilinear.npz")
LABEL_FILES = ("berlin_00125_gtFine_labelIds.png", "berlin_00126_gtFine_labelIds.png")      # tests/golden/, mode L, 1200 x 1600

# name -> (src_h, src_w, channels, dst_h, dst_w): downscale by no round factor, upscale, one axis unchanged (each way), and the factors
# of the real geometry (1200 x 1600 -> 256 x 512: 4.6875 x 3.125) on a block image of the label ids the tables tell apart
GEOMETRIES = {
    "down_37x53_c3": (37, 53, 3, 16, 24),
    "up_16x24_c1": (16, 24, 1, 37, 53),
    "rows_only_33x64_c1": (33, 64, 1, 32, 64),
    "cols_only_100x77_c3": (100, 77, 3, 100, 33),
    "label_blocks_75x100_c1": (75, 100, 1, 16, 32),
}
MISTAKES = ("no_round_between", "floor_xmin_no_clamp", "unnormalised")


def source(name: str) -> np.ndarray:
    """the seeded input of a geometry, u8 [h, w, c]"""
    h, w, c = GEOMETRIES[name][:3]
    rng = np.random.default_rng(sorted(GEOMETRIES).index(name) + 20261020)
    if name.startswith("label_blocks"):
        blocks = np.array([0, 7, 13], np.uint8)[rng.integers(0, 3, (-(-h // 9), -(-w // 11)))]
        return np.ascontiguousarray(np.kron(blocks, np.ones((9, 11), np.uint8))[:h, :w, None])
    return rng.integers(0, 256, (h, w, c), dtype=np.uint8)


# ---- the numpy restatement ----------------------------------------------------------------------------------------------------------
def windows_np(n_in: int, n_out: int, mistake: str | None = None):
    """[(xmin, k int64 [n])] per destination sample.  floor_xmin_no_clamp: the window starts at floor(center - support + 0.5) and is not
    clamped at 0 (xmin may be negative: the caller replicates the edge sample) -- what a kernel computes that floors and clamps the
    SAMPLE index where Pillow truncates and clamps the WINDOW.  With the clamp kept, floor and the truncating cast give the same
    windows (both are <= 0 exactly when the other is), which is why the mistake is stated without it."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    out = []
    for d in range(n_out):
        center = (d + 0.5) * scale
        if mistake == "floor_xmin_no_clamp":
            xmin = int(np.floor(center - support + 0.5))
        else:
            xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        i = np.arange(xmax - xmin, dtype=np.float64)
        w = np.maximum(0.0, 1.0 - np.abs((i + xmin - center + 0.5) * (1.0 / fs)))
        if mistake != "unnormalised":
            w = w / w.sum()
        out.append((xmin, (0.5 + w * (1 << 22)).astype(np.int64)))
    return out


def _pass(img: np.ndarray, n_out: int, mistake, rounded: bool) -> np.ndarray:
    """resample axis 1 of [rows, n_in, c]; rounded: clip_u8((2^21 + sum) >> 22), else the exact sum as float64 / 2^22"""
    n_in = img.shape[1]
    out = np.zeros((img.shape[0], n_out, img.shape[2]), np.float64 if not rounded else np.uint8)
    for d, (xmin, k) in enumerate(windows_np(n_in, n_out, mistake)):
        idx = np.clip(np.arange(xmin, xmin + len(k)), 0, n_in - 1)
        taps = img[:, idx, :]
        if rounded:
            acc = (1 << 21) + (taps.astype(np.int64) * k[None, :, None]).sum(1)
            out[:, d, :] = np.clip(acc >> 22, 0, 255)
        else:
            out[:, d, :] = (taps.astype(np.float64) * k[None, :, None]).sum(1) / (1 << 22)
    return out


def pil_resize_np(img: np.ndarray, dst_h: int, dst_w: int, mistake: str | None = None) -> np.ndarray:
    """Image.resize((dst_w, dst_h), BILINEAR) of u8 [h, w, c]: horizontal pass, uint8, vertical pass; an unchanged axis is skipped"""
    assert mistake is None or mistake in MISTAKES
    h, w, c = img.shape
    cur = img
    if dst_w != w:
        cur = _pass(cur, dst_w, mistake, rounded=mistake != "no_round_between")
    if dst_h != h:
        if cur.dtype != np.uint8:            # no_round_between: the vertical pass reads the unrounded sums; one rounding at the end
            acc = _pass(cur.transpose(1, 0, 2), dst_h, mistake, rounded=False).transpose(1, 0, 2)
            return np.clip(np.floor(acc + 0.5), 0, 255).astype(np.uint8)
        cur = _pass(cur.transpose(1, 0, 2), dst_h, mistake, rounded=True).transpose(1, 0, 2)
    if cur.dtype != np.uint8:
        cur = np.clip(np.floor(cur + 0.5), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(cur)


def pillow_resize(img: np.ndarray, dst_h: int, dst_w: int) -> np.ndarray:
    from PIL import Image
    im = Image.fromarray(img[:, :, 0] if img.shape[2] == 1 else img)
    out = np.asarray(im.resize((dst_w, dst_h), Image.BILINEAR))
    return np.ascontiguousarray(out.reshape(dst_h, dst_w, img.shape[2]))


# ---- the host twins through ctypes ----------------------------------------------------------------------------------------------------
def host_resize(frames: np.ndarray, dst_h: int, dst_w: int, channels: int | None = None, pixel_stride: int | None = None, reverse: bool = False):
    """sd_resize_pil_bilinear_u8_host on u8 [B, h, w, stride] -> (status, u8 [B, dst_h, dst_w, channels])"""
    lib = L.load()
    frames = np.ascontiguousarray(frames)
    B, h, w, s = frames.shape
    channels = channels or s
    pixel_stride = pixel_stride or s
    out = np.zeros((B, dst_h, dst_w, channels), np.uint8)
    st = lib.sd_resize_pil_bilinear_u8_host(frames.ctypes.data_as(C.c_void_p), B, h, w, pixel_stride, channels, int(reverse),
                                            out.ctypes.data_as(C.c_void_p), dst_h, dst_w)
    return st, out


def host_confusion(pred: np.ndarray, labels: np.ndarray, table: np.ndarray, counts: np.ndarray | None = None):
    """sd_seg_confusion_host on u8 [B, h, w] -> (status, int64 [B, 10])"""
    lib = L.load()
    pred, labels, table = np.ascontiguousarray(pred), np.ascontiguousarray(labels), np.ascontiguousarray(table, dtype=np.uint8)
    B, h, w = pred.shape
    if counts is None:
        counts = np.zeros((B, L.SD_SEG_CELLS), np.int64)
    st = lib.sd_seg_confusion_host(pred.ctypes.data_as(C.c_void_p), labels.ctypes.data_as(C.c_void_p), B, h, w, table.ctypes.data_as(C.c_void_p),
                                   counts.ctypes.data_as(C.c_void_p))
    return st, counts


def bincount_confusion(pred: np.ndarray, labels: np.ndarray, table: np.ndarray) -> np.ndarray:
    """int64 [B, 10] by np.bincount: cell 3 * table[label] + pred, predictions above 2 in cell 9"""
    out = []
    for p, l in zip(pred, labels):
        cell = np.where(p > 2, 9, table[l].astype(np.int64) * 3 + np.minimum(p, 2))
        out.append(np.bincount(cell.ravel(), minlength=10))
    return np.stack(out).astype(np.int64)


def confusion_inputs(h: int, w: int, B: int = 1, seed: int = 0, absent: int | None = None):
    """seeded (pred, labels): predictions 0..2, label ids 0..33 with 7 and 13 frequent; absent: a class no prediction names"""
    rng = np.random.default_rng(4000 + seed + 31 * h + w)
    pred = rng.integers(0, 3, (B, h, w), dtype=np.uint8)
    if absent is not None:
        pred[pred == absent] = (absent + 1) % 3
    ids = np.array([7, 7, 7, 13, 13, 11, 12, 16, 0, 1, 23, 33, 255], np.uint8)
    labels = ids[rng.integers(0, len(ids), (B, h, w))]
    return pred, labels


# ---- a Cityscapes-layout tree -----------------------------------------------------------------------------------------------------------
def write_fixture_tree(root: str, golden_dir: str, frame_hw=(1200, 1600)):
    """gtFine/test/berlin/<the two committed label images>, leftImg8bit/test/berlin/<seeded noise frames written by outputs.write_png>
    -> (gt_dir, imgs_dir)"""
    import shutil
    from semantic_depth_amd import outputs
    gt = os.path.join(root, "gtFine", "test")
    im = os.path.join(root, "leftImg8bit", "test")
    os.makedirs(os.path.join(gt, "berlin"))
    os.makedirs(os.path.join(im, "berlin"))
    rng = np.random.default_rng(77)
    for name in LABEL_FILES:
        shutil.copy(os.path.join(golden_dir, name), os.path.join(gt, "berlin", name))
        # smooth-ish noise: blocks keep the PNG small and the resample non-trivial
        frame = np.kron(rng.integers(0, 256, (frame_hw[0] // 8, frame_hw[1] // 8, 3), dtype=np.uint8), np.ones((8, 8, 1), np.uint8))
        outputs.write_png(os.path.join(im, "berlin", name.replace("_gtFine_labelIds", "_leftImg8bit")), frame)
    return gt, im
