#!/usr/bin/env python3
"""dev tool: the JPEG encoder of the result video beside PIL on the CPU (fidelity gap in dB, file sizes beside PIL's restart_marker_rows=1
files, the largest excess of |qQ - c| over Q/2 against a float64 DCT) and, unless --host-only, the kernel time of Engine.encode_jpeg (three
launches) between device events and the stream bytes per frame beside the png="device" stream of the same frame.
usage: python scripts/mjpeg_rate.py [--host-only] [--batch 32] [--height 1024] [--width 2048] [--quality 90] [--calls 20] [--out FILE]
Prints one JSON object; per-kernel times are not taken here (they need a rocprofv3 --kernel-trace --stats run of their own)."""
import argparse
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)


def composed_like(seed, h, w):
    """smooth content under a flat banner, the look of a composed result image"""
    from png_device_cases import smooth_frame
    small = smooth_frame(seed, 128, 256)
    return np.ascontiguousarray(np.kron(small, np.ones((h // 128, w // 256, 1), np.uint8))[:h, :w])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as graft
    graft.build()
    import jpeg_enc_cases as JC
    from PIL import Image
    from scipy.fft import dctn
    from semantic_depth_amd import frame_io, outputs
    res = dict(cpu=dict(cases={}), quality=a.quality)
    worst = -1e9
    for name in JC.CASE_NAMES:
        img, q = JC.cases()[name]
        ours = JC.host_stream(name)
        buf, rst = io.BytesIO(), io.BytesIO()
        Image.fromarray(img[..., ::-1]).save(buf, "JPEG", quality=q, subsampling=2)
        Image.fromarray(img[..., ::-1]).save(rst, "JPEG", quality=q, subsampling=2, restart_marker_rows=1)
        d, comps = JC.decoded_coefficients(ours)
        excess = -1e9
        for c, plane in enumerate(JC.planes(img)):
            bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
            ref = dctn((plane.astype(np.float64) - 128.0).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3), axes=(2, 3), norm="ortho").reshape(bh, bw, 64)
            Q = np.array(d.qt[c][:], np.float64)
            excess = max(excess, float((np.abs(comps[c] * Q - ref) - Q / 2).max()))
        worst = max(worst, excess)
        e = dict(quality=q, shape=list(img.shape[:2]), bytes=len(ours), pil_restart_rows_1_bytes=len(rst.getvalue()), pil_bytes=len(buf.getvalue()),
                 dct_excess_over_half_quantum=round(excess, 4))
        if img.std() > 0:
            po, pp = psnr(frame_io.decode_jpeg(ours), img), psnr(frame_io.decode_jpeg(buf.getvalue()), img)
            if np.isfinite(po) and np.isfinite(pp):
                e.update(psnr_db=round(po, 3), pil_psnr_db=round(pp, 3), gap_db=round(po - pp, 3))
        res["cpu"]["cases"][name] = e
    res["cpu"]["largest_dct_excess_over_half_quantum"] = round(worst, 4)
    res["cpu"]["smallest_gap_db"] = min(e["gap_db"] for e in res["cpu"]["cases"].values() if "gap_db" in e)
    if not a.host_only:
        import torch
        from semantic_depth_amd.engine import Engine
        eng = Engine(128, 256, 1, "resnet50")
        try:
            frames = np.stack([composed_like(s % 4, a.height, a.width) for s in range(a.batch)])
            dev = torch.from_numpy(frames).cuda()
            stride = 1024 + a.height * a.width * 3 // 2
            for _ in range(3):
                streams, sizes, flags = eng.encode_jpeg(dev, a.quality, stream_stride=stride)
            torch.cuda.synchronize()
            times = []
            for _ in range(a.calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                streams, sizes, flags = eng.encode_jpeg(dev, a.quality, stream_stride=stride)
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            sz = sizes.cpu().numpy()
            same = streams[0, :int(sz[0])].cpu().numpy().tobytes() == outputs.encode_jpeg_host(frames[0], a.quality)
            psz = eng.encode_png(dev)[1].cpu().numpy()
            res["device"] = dict(batch=a.batch, height=a.height, width=a.width, calls=a.calls, stream_stride=stride,
                                 encode_jpeg_ms_per_call_three_launches=dict(median=round(float(np.median(times)), 3), min=round(min(times), 3),
                                                                             max=round(max(times), 3)),
                                 kernels_timed_apart=False, frame0_equals_host_statement=bool(same), flags=int(flags.sum()),
                                 jpeg_bytes_per_frame=int(sz.mean()), png_device_stream_bytes_per_frame=int(psz.mean()),
                                 raw_bytes_per_frame=a.height * a.width * 3)
        finally:
            eng.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
