"""Host restatements used by the sequence-output tests (tests/test_sequence_outputs.py, tests/test_gpu_sequence_outputs.py)."""
import numpy as np

ROAD = (128, 64, 128)
FENCE_SEQ = (190, 153, 153)      # semantic_depth_cityscapes_sequence.py:481
FENCE_SINGLE = (160, 10, 10)     # semantic_depth.py:565
ALPHA = 64


def pil_paste(frame, road, fence, road_color=ROAD, fence_color=FENCE_SEQ, alpha=ALPHA):
    """street_im.paste(road_mask, mask=road_mask); street_im.paste(fence_mask, mask=fence_mask) (seq:463-485) in integers:
    Pillow's BLEND, t = dst*(255-a) + src*a + 128, ((t >> 8) + t) >> 8, on the masked pixels; the others are unchanged."""
    img = np.asarray(frame).astype(np.int32)
    for mask, col in ((road, road_color), (fence, fence_color)):
        m = np.asarray(mask).astype(bool)
        if m.ndim == img.ndim - 1:
            m = m[..., None]
        t = img * (255 - alpha) + np.asarray(col, np.int32) * alpha + 128
        img = np.where(m, ((t >> 8) + t) >> 8, img)
    return img.astype(np.uint8)


def pillow_paste(frame, road, fence, road_color=ROAD, fence_color=FENCE_SEQ, alpha=ALPHA):
    """the same through Pillow itself (RGBA mask images pasted with themselves as mask, as the reference does)"""
    from PIL import Image
    street = Image.fromarray(np.ascontiguousarray(frame))
    for mask, col in ((road, road_color), (fence, fence_color)):
        m = np.asarray(mask).astype(bool)
        rgba = np.zeros(m.shape + (4,), np.uint8)
        rgba[m] = tuple(col) + (alpha,)
        im = Image.fromarray(rgba)                      # (4 channels: RGBA)
        street.paste(im, None, im)
    return np.asarray(street)


def banner_rows(h):
    """rows cv2.rectangle((0,0), (w, int(0.25*h)), ..., -1) fills (inclusive corner, clipped: outputs.draw_overlay)"""
    return min(int(0.25 * h), h - 1) + 1
