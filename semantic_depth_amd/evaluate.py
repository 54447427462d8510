"""Score the segmentation against labelled frames: the test mode of fcn8s/fcn.py (FCN.inference, :384-492).

    python -m semantic_depth_amd.evaluate --gt DATA/gtFine/test --imgs DATA/leftImg8bit/test --weights fcn8s.npz

The reference walks a Cityscapes-layout folder, resizes frame AND label image with scipy.misc.imresize (= PIL bilinear; Engine.resize_pil),
feeds the RGB frame to FCN-8s, scores argmax against helper.prepare_ground_truth with tf.metrics.mean_iou, writes test_set_iou_<time>.txt
and saves the overlay images.  Here the per-pixel work runs on the GPU (csrc/seg_eval_gpu.hip) around the engine's network call; the
per-frame 3 x 3 count matrices come to the host once, and everything below them is a few float32 operations.

Two deviations, both stated where they apply: the prediction is the engine's argmax of the LOGITS (the reference takes argmax of the
float32 softmax, which can differ only where rounding in the softmax creates a tie), and mean_iou restates tf.metrics.mean_iou from its
source -- TensorFlow is not available to pin it ([UPSTREAM] unpinned, as elsewhere in the documents)."""
from __future__ import annotations

import ctypes as C
import glob
import os

import numpy as np

from . import _lib as L

ROAD_COLOR, FENCE_COLOR, ALPHA = (128, 64, 128), (190, 153, 153), 64      # fcn.py:450, :457 (RGB, as the frames are there)


def label_table(dataset: str = "robo", mode: str = "test") -> np.ndarray:
    """helper.prepare_ground_truth (:149-177) as a table label id -> class, u8 [256]: road (id 7) = 0, fence = 1, everything else = 2.
    Fence is id 13 for 'robo...' datasets and for 'city...' in test mode, the construction group 11..16 for 'city...' in train mode."""
    t = np.full(256, 2, np.uint8)
    t[7] = 0
    if dataset[0:4] == "city" and mode == "train":
        t[11:17] = 1
    elif (dataset[0:4] == "city" and mode == "test") or dataset[0:4] == "robo":
        t[13] = 1
    else:
        raise ValueError(f"label_table: dataset {dataset!r} / mode {mode!r} (the reference knows 'city...' with 'train' | 'test', and 'robo...')")
    return t


def labelled_pairs(gt_dir: str, imgs_dir: str) -> list:
    """helper.get_files_paths (:119-133): for every city folder under imgs_dir the '*_gtFine_labelIds.png' files of gt_dir/<city> and the
    '*.png' files of imgs_dir/<city>; both lists sorted, then zipped -> [(label file, frame file)].  The reference zips blindly; lists
    of different lengths are refused here."""
    gt, imgs = [], []
    for city in os.listdir(imgs_dir):
        gt += glob.glob(os.path.join(gt_dir, city, "*_gtFine_labelIds.png"))
        imgs += glob.glob(os.path.join(imgs_dir, city, "*.png"))
    gt.sort()
    imgs.sort()
    if len(gt) != len(imgs):
        raise ValueError(f"labelled_pairs: {len(gt)} label files under {gt_dir} but {len(imgs)} frames under {imgs_dir}")
    return list(zip(gt, imgs))


def class_iou(cm) -> tuple:
    """(iou float32 [3], valid bool [3]) of a 3 x 3 count matrix [label class][predicted class], the way tf.metrics.mean_iou forms them:
    the sums are exact (float64 accumulators there), cast to float32, then diag / (row_sum + col_sum - diag) in float32; a class with a
    zero denominator is not valid and its quotient is 0 / 1."""
    cm = np.asarray(cm, np.int64).reshape(3, 3)
    over_row = cm.sum(0).astype(np.float64).astype(np.float32)
    over_col = cm.sum(1).astype(np.float64).astype(np.float32)
    diag = np.diagonal(cm).astype(np.float64).astype(np.float32)
    den = (over_row + over_col - diag).astype(np.float32)
    valid = den != 0
    return (diag / np.where(den > 0, den, np.float32(1))).astype(np.float32), valid


def mean_iou(cm) -> np.float32:
    """tf.metrics.mean_iou on a 3 x 3 count matrix ([UPSTREAM] unpinned): the float32 mean of class_iou over the valid classes, summed in
    class order; 0 when no class is valid."""
    iou, valid = class_iou(cm)
    n = np.float32(valid.sum())
    if not n > 0:
        return np.float32(0)
    s = np.float32(0)
    for v in iou:
        s = np.float32(s + v)
    return np.float32(s / n)


def summarise(per_frame, pairs=None) -> dict:
    """the result record from int64 [N, 3, 3] per-frame matrices.  running_mean_iou[i] is what the reference appends to test_ious after
    frame i: iou_op ACCUMULATES, so it is the mean IoU of frames 0..i together, not of frame i.  mean_of_running is the reference's
    'test mean' (sum(test_ious) / len(test_ious), float32) -- the number its file and the thesis report; mean_iou is the mean IoU of the
    whole set, = running_mean_iou[-1]."""
    per_frame = np.asarray(per_frame, np.int64).reshape(-1, 3, 3)
    running = [mean_iou(c) for c in np.cumsum(per_frame, axis=0)]
    total = per_frame.sum(0)
    acc = np.float32(0)
    for v in running:
        acc = np.float32(acc + v)
    iou, valid = class_iou(total)
    return dict(per_frame=per_frame, total=total, class_iou=iou, class_valid=valid, mean_iou=mean_iou(total), running_mean_iou=running,
                mean_of_running=np.float32(acc / np.float32(len(running))) if running else np.float32(0), pairs=list(pairs or []))


def iou_file_text(result: dict) -> str:
    """the text of fcn.py:488-492: one running value per line, then the 'test mean', no trailing newline.  "{}".format of a numpy float32
    (what sess.run returns there) goes through Python's float: the float32 value with a double's digits, e.g. 0.6833333373069763"""
    return "".join("{}\n".format(v) for v in result["running_mean_iou"]) + "IoU metric of Testing set: {}".format(result["mean_of_running"])


def write_test_set_iou(path: str, result: dict) -> str:
    with open(path, "w") as f:
        f.write(iou_file_text(result))
    return path


def _host_resize(frames: np.ndarray, H: int, W: int, channels: int, reverse: bool) -> np.ndarray:
    lib = L.load()
    B, h, w, s = frames.shape
    out = np.empty((B, H, W, channels), np.uint8)
    st = lib.sd_resize_pil_bilinear_u8_host(frames.ctypes.data_as(C.c_void_p), B, h, w, s, channels, int(reverse), out.ctypes.data_as(C.c_void_p), H, W)
    L.check(lib, None, st, "sd_resize_pil_bilinear_u8_host")
    return out


def evaluate_files(gt_dir: str, imgs_dir: str, engine, dataset: str = "robo", route: str = "device", images_dir: str | None = None,
                   batch: int | None = None) -> dict:
    """FCN.inference (:384-492) over labelled_pairs(gt_dir, imgs_dir) on ``engine`` (FCN-8s weights loaded; frames are resampled to its
    H x W) -> summarise()'s record.
    route='device': the files are read by the existing FrameFeeder, both the frame (BGR -> RGB) and channel 0 of the label image go
    through Engine.resize_pil, Engine.fcn8s_forward gives argmax, Engine.seg_confusion adds each frame's matrix into ONE int64 [N,10] device
    tensor, which is read once at the end.  route='host': the host twins (sd_resize_pil_bilinear_u8_host, sd_seg_confusion_host) around the
    same network call; it exists for the tests and the rate script.  Both give the same record.
    The prediction is the engine's argmax of the logits; the reference takes argmax of the float32 softmax (see the module text).  A
    prediction above 2 (none can come from fcn8s_forward) raises ValueError.
    images_dir: the overlay images of :443-470 -- the road colour, then the fence colour pasted with alpha 64 where the engine's masks
    (softmax > 0.5) are set, at the network's size, no banner -- through Engine.compose_result_frames and the host PNG writer, named like
    the frame files.  batch defaults to the engine's max_batch."""
    import torch

    from . import outputs
    from .frame_io import FrameFeeder
    if route not in ("device", "host"):
        raise ValueError(f"evaluate_files: route must be 'device' or 'host', not {route!r}")
    table = label_table(dataset, "test")
    pairs = labelled_pairs(gt_dir, imgs_dir)
    N = len(pairs)
    if N == 0:
        raise ValueError(f"evaluate_files: no labelled frames under {imgs_dir}")
    H, W = engine.H, engine.W
    batch = int(batch or engine.max_batch)
    if images_dir:
        os.makedirs(images_dir, exist_ok=True)
    dev = torch.device(engine.device)
    feed_dev = dev if route == "device" else "cpu"
    counts = torch.zeros((N, L.SD_SEG_CELLS), dtype=torch.int64, device=dev) if route == "device" else np.zeros((N, L.SD_SEG_CELLS), np.int64)
    kw = dict(engine=engine) if route == "device" else {}
    with FrameFeeder([p[0] for p in pairs], batch, device=feed_dev, **kw) as gts, \
            FrameFeeder([p[1] for p in pairs], batch, device=feed_dev, **kw) as imgs:
        for (gt, lo), (frames, lo2) in zip(gts, imgs):
            n = int(frames.shape[0])
            assert lo == lo2 and gt.shape[0] == n
            if route == "device":
                rgb = engine.resize_pil(frames, H, W, channels=3, reverse=True)
                lab = engine.resize_pil(gt, H, W, channels=1, pixel_stride=3).view(n, H, W)
                net = engine.fcn8s_forward(rgb)
                engine.seg_confusion(net["argmax"], lab, table, out=counts[lo:lo + n])
            else:
                rgb_h = _host_resize(np.ascontiguousarray(frames.numpy()), H, W, 3, True)
                lab_h = _host_resize(np.ascontiguousarray(gt.numpy()), H, W, 1, False).reshape(n, H, W)
                rgb = torch.from_numpy(rgb_h).to(dev)
                net = engine.fcn8s_forward(rgb)
                pred = np.ascontiguousarray(net["argmax"].cpu().numpy())
                lib = L.load()
                st = lib.sd_seg_confusion_host(pred.ctypes.data_as(C.c_void_p), lab_h.ctypes.data_as(C.c_void_p), n, H, W,
                                               table.ctypes.data_as(C.c_void_p), counts[lo:lo + n].ctypes.data_as(C.c_void_p))
                L.check(lib, None, st, "sd_seg_confusion_host")
            if images_dir:
                records = torch.zeros((n, 104), dtype=torch.uint8, device=dev)           # found = 0: no banner
                over = engine.compose_result_frames(rgb, net["road"], net["fence"], records, H, W, ROAD_COLOR, FENCE_COLOR, ALPHA)
                names = [os.path.join(images_dir, os.path.basename(p[1])) for p in pairs[lo:lo + n]]
                outputs.write_png_batch(names, over.cpu().numpy()[..., ::-1])        # (the writer takes BGR)
    c = counts.cpu().numpy() if route == "device" else counts
    bad = np.nonzero(c[:, 9])[0]
    if bad.size:
        raise ValueError(f"evaluate_files: {int(c[:, 9].sum())} prediction(s) above 2 in frame(s) {bad[:8].tolist()}: not an argmax over three classes")
    return summarise(c[:, :9].reshape(N, 3, 3), pairs)


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(description="mean IoU of an FCN-8s checkpoint over a Cityscapes-layout folder (fcn.py test mode)")
    ap.add_argument("--gt", required=True, help="label root, e.g. data/roborace750/gtFine/test (city folders with *_gtFine_labelIds.png)")
    ap.add_argument("--imgs", required=True, help="frame root, e.g. data/roborace750/leftImg8bit/test")
    ap.add_argument("--weights", required=True, help="FCN-8s weights: an .npz of TF-layout arrays, a TF checkpoint prefix or a frozen .pb")
    ap.add_argument("--precision", default="f32")
    ap.add_argument("--dataset", default="robo")
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--route", default="device", choices=("device", "host"))
    ap.add_argument("--images", default=None, help="folder for the overlay images")
    ap.add_argument("--out", default=None, help="the test_set_iou text file (default: print only)")
    a = ap.parse_args(argv)
    from .api import _load_weight_arg
    from .engine import Engine
    eng = Engine(a.height, a.width, a.batch, precision=a.precision)
    try:
        eng.load_weights(L.SD_NET_FCN8S, _load_weight_arg(a.weights))
        res = evaluate_files(a.gt, a.imgs, eng, dataset=a.dataset, route=a.route, images_dir=a.images, batch=a.batch)
    finally:
        eng.close()
    if a.out:
        write_test_set_iou(a.out, res)
    print(f"frames: {len(res['pairs'])}")
    for name, v, ok in zip(("road", "fence", "else"), res["class_iou"], res["class_valid"]):
        print(f"IoU {name}: {v if ok else 'n/a (class absent)'}")
    print(f"mean IoU of the set: {res['mean_iou']}")
    print(f"IoU metric of Testing set: {res['mean_of_running']}      (the reference's mean of its running values)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
