"""Input stage, host side: the frame reader that replaces ``cv2.imread`` (semantic_depth.py:105; seq:123) and a
feeder that keeps the GPU supplied.

    imread(path)            8-bit PNG or Huffman JPEG -> u8 [h,w,3] BGR, exactly cv2.imread's IMREAD_COLOR result: ONE native call
                            (sd_png_decode_bgr: chunk walk, zlib inflate, scanline reconstruction, BGR shuffle, palette;
                            sd_jpeg_decode_bgr: libjpeg's default decode path and the EXIF orientation, restated)
    FrameFeeder             the sorted file list (seq:689) batch by batch: ONE native call per batch (sd_decode_files_bgr, C++ threads)
                            reads and decodes straight into a pinned staging buffer, one batch ahead of the GPU; the cubic resize to
                            the network shape happens ON the GPU (Engine.resize_cubic), so the host never touches a pixel after the decode

PNG decode stays on the host on purpose: DEFLATE and the PNG predictors are serial byte recurrences; a frame costs a few
milliseconds of one core (scripts/feed_rate.py measures decode, pinned H2D and resize rates against the benchmarked
frames/s; DESIGN.md quotes them).  JPEG frames (the reference's own example frame is one) have two routes: ``jpeg="host"``, the
default, decodes them completely on the host threads as well; ``jpeg="device"`` keeps only the serial part there -- the Huffman
decoder, to quantised coefficients (sd_decode_files_jpeg_coef) -- and runs the inverse DCT, the chroma upsampling, the colour
conversion and the EXIF orientation on the GPU (Engine.jpeg_reconstruct), byte for byte the host route's frames.
"""
from __future__ import annotations

import ctypes as C
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib as L

_SIG = b"\x89PNG\r\n\x1a\n"
_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def png_size(buf: bytes) -> tuple[int, int]:
    """(height, width) of a PNG this reader takes (8-bit, non-interlaced); ValueError otherwise"""
    lib = L.load()
    h, w = C.c_int(), C.c_int()
    if lib.sd_png_decode_bgr(buf, len(buf), None, 0, C.byref(h), C.byref(w)) != L.SD_OK:
        if bytes(buf[:8]) != _SIG:
            raise ValueError("not a PNG file")
        raise ValueError("unsupported or corrupt PNG (8-bit, non-interlaced gray / gray+alpha / RGB / RGBA / palette only)")
    return h.value, w.value


def decode_png(buf: bytes) -> np.ndarray:
    """PNG bytes -> u8 [h,w,3] BGR (cv2.IMREAD_COLOR semantics: 3 channels, alpha dropped, gray replicated, palette expanded).
    One native call (sd_png_decode_bgr: chunk walk, zlib inflate, scanline reconstruction, shuffle), the interpreter lock released."""
    h, w = png_size(buf)
    out = np.empty((h, w, 3), np.uint8)
    lib = L.load()
    if lib.sd_png_decode_bgr(buf, len(buf), out.ctypes.data_as(C.c_void_p), out.nbytes, None, None) != L.SD_OK:
        raise ValueError("PNG: corrupt stream (inflate / filter type / palette index)")
    return out


def image_size(buf: bytes) -> tuple[int, int]:
    """(height, width) of a PNG or Huffman JPEG (SOF0 / SOF1 / SOF2) as cv2.imread would return it (JPEG: after the EXIF orientation)"""
    lib = L.load()
    h, w = C.c_int(), C.c_int()
    if lib.sd_image_decode_bgr(buf, len(buf), None, 0, C.byref(h), C.byref(w)) != L.SD_OK:
        raise ValueError("not a PNG / JPEG this reader takes (PNG: 8-bit non-interlaced; JPEG: baseline, extended-sequential or progressive Huffman, 8-bit, "
                         "gray or YCbCr 4:4:4 / 4:2:2 / 4:2:0)")
    return h.value, w.value


def decode_jpeg(buf: bytes) -> np.ndarray:
    """JPEG bytes (baseline / extended-sequential / progressive Huffman) -> u8 [h,w,3] BGR = cv2.imread: libjpeg's default decode path (ISLOW inverse DCT, fancy chroma upsampling,
    fixed-point YCbCr -> RGB) and the EXIF orientation, restated natively (sd_jpeg_decode_bgr)"""
    if bytes(buf[:2]) != b"\xff\xd8":
        raise ValueError("not a JPEG file")
    return decode_image(buf)


def decode_image(buf: bytes) -> np.ndarray:
    h, w = image_size(buf)
    out = np.empty((h, w, 3), np.uint8)
    if L.load().sd_image_decode_bgr(buf, len(buf), out.ctypes.data_as(C.c_void_p), out.nbytes, None, None) != L.SD_OK:
        raise ValueError("corrupt image stream")
    return out


def imread(path: str) -> np.ndarray:
    """cv2.imread(path) for 8-bit PNG and Huffman JPEG (SOF0 / SOF1 / SOF2) files (semantic_depth.py:105; seq:123)"""
    with open(path, "rb") as f:
        buf = f.read()
    return decode_png(buf) if buf[:8] == _SIG else decode_image(buf)


def _avi_chunks(f, start: int, end: int):
    """(fourcc, payload offset, payload size) of the chunks in [start, end) of an open RIFF file"""
    import struct
    pos = start
    while pos + 8 <= end:
        f.seek(pos)
        head = f.read(8)
        if len(head) < 8:
            return
        cc, size = head[:4], struct.unpack("<I", head[4:])[0]
        yield cc, pos + 8, size
        pos += 8 + size + (size & 1)


def _avi_layout(f):
    """(avih fields, strh fields, offset of the 'movi' fourcc, (offset, size) of the idx1 payload or None) of an open AVI file"""
    import struct
    f.seek(0)
    head = f.read(12)
    if len(head) < 12 or head[:4] != b"RIFF" or head[8:] != b"AVI ":
        raise ValueError("not a RIFF AVI file")
    end = 8 + struct.unpack("<I", head[4:8])[0]
    avih = strh = movi = idx1 = None
    for cc, off, size in _avi_chunks(f, 12, end):
        f.seek(off)
        if cc == b"LIST":
            kind = f.read(4)
            if kind == b"movi":
                movi = off
            elif kind == b"hdrl":
                for c2, o2, s2 in _avi_chunks(f, off + 4, off + size):
                    f.seek(o2)
                    if c2 == b"avih":
                        avih = struct.unpack("<14I", f.read(56))
                    elif c2 == b"LIST" and f.read(4) == b"strl" and strh is None:
                        for c3, o3, s3 in _avi_chunks(f, o2 + 4, o2 + s2):
                            if c3 == b"strh":
                                f.seek(o3)
                                strh = struct.unpack("<4s4sIHHIIIIIIII4h", f.read(56))
        elif cc == b"idx1":
            idx1 = (off, size)
    if avih is None or strh is None or movi is None:
        raise ValueError("AVI file without avih / strh / movi")
    return avih, strh, movi, idx1


def avi_info(path: str) -> dict:
    """width, height, frames, rate and scale (frames per second = rate / scale) and the stream handler of an AVI file's first stream"""
    with open(path, "rb") as f:
        avih, strh, _, _ = _avi_layout(f)
    return dict(width=int(avih[8]), height=int(avih[9]), frames=int(strh[9]), rate=int(strh[7]), scale=int(strh[6]), handler=strh[1])


def avi_frames(path: str):
    """the frames of a Motion-JPEG AVI (outputs.MjpegAviWriter's files) as byte strings -- each a complete JPEG file, decode_jpeg reads it --
    in index order, read through idx1 (offsets relative to the 'movi' fourcc)"""
    import struct
    with open(path, "rb") as f:
        _, _, movi, idx1 = _avi_layout(f)
        if idx1 is None:
            raise ValueError("AVI file without an idx1 index")
        f.seek(idx1[0])
        index = f.read(idx1[1])
        for k in range(0, len(index) - 15, 16):
            cc, _flags, off, size = struct.unpack("<4sIII", index[k:k + 16])
            if cc[2:] not in (b"dc", b"db"):
                continue
            f.seek(movi + off)
            head = f.read(8)
            if head[:4] != cc or struct.unpack("<I", head[4:])[0] != size:
                raise ValueError(f"AVI index entry {k // 16} does not point at its chunk")
            yield f.read(size)


def _cgroup_cpu_quota():
    """CPUs the cgroup quota allows (v2: cpu.max "<quota> <period>" | "max <period>"; v1: cpu.cfs_quota_us / cpu.cfs_period_us), or None"""
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
        return None if q == "max" else max(1, int(int(q) / int(per)))
    except (OSError, ValueError):
        pass
    try:
        with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
            q = int(f.read())
        with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
            per = int(f.read())
        return None if q <= 0 or per <= 0 else max(1, q // per)
    except (OSError, ValueError):
        return None


def _local_ranks() -> int:
    """ranks that share this node: LOCAL_WORLD_SIZE (torch.distributed.run, bench.py's launcher), Open MPI's / MPICH's / Slurm's per-node counts
    (SLURM_TASKS_PER_NODE is always set by srun, SLURM_NTASKS_PER_NODE only with --ntasks-per-node), else WORLD_SIZE -- the conservative single-node
    assumption for a job started by hand with RANK / WORLD_SIZE: on several nodes it UNDER-subscribes the decode threads (affinity / WORLD_SIZE each),
    never over-subscribes them --, else 1"""
    import os
    for k in ("LOCAL_WORLD_SIZE", "OMPI_COMM_WORLD_LOCAL_SIZE", "MPI_LOCALNRANKS", "SLURM_NTASKS_PER_NODE", "SLURM_TASKS_PER_NODE", "WORLD_SIZE"):
        v = os.environ.get(k, "")
        try:
            n = int(v.split("(")[0])           # (Slurm writes "8(x2)" for heterogeneous jobs)
        except ValueError:
            continue
        if n >= 1:
            return n
    return 1


def default_decode_workers() -> int:
    """decode threads of ONE rank: the CPUs this process may run on (its affinity mask, capped by the cgroup CPU quota -- os.cpu_count()
    reports the host's 256 whatever the container may use) divided by the ranks of the node (_local_ranks), at least 1, at most 128.
    Eight ranks on a 256-CPU node get 32 threads each instead of 8 x 128."""
    import os
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 8
    q = _cgroup_cpu_quota()
    if q is not None:
        n = min(n, q)
    return max(1, min(n // _local_ranks(), 128))


class FrameFeeder:
    """iterate over (frames u8 [n,h,w,3] on ``device``, first global index) for the sorted ``paths``: every batch is read and decoded
    by ONE native call (sd_decode_files_bgr: ``workers`` C++ threads, no interpreter lock) straight into a pinned staging buffer,
    uploaded asynchronously, one batch ahead of the consumer (two staging buffers).
    ``jpeg="device"`` (needs ``engine``, an engine.Engine whose handle launches the kernels, and a GPU ``device``): the JPEG files of a
    batch are only entropy-decoded on the host (sd_decode_files_jpeg_coef into a pinned int16 staging buffer, one batch ahead as well);
    each frame's coefficients are uploaded asynchronously and Engine.jpeg_reconstruct writes the frames into the same u8 [n,h,w,3]
    device tensor behind the upload, on the current stream.  PNG files of such a batch go the BGR way into that tensor.  The frames,
    indices and batch boundaries are those of ``jpeg="host"``."""

    def __init__(self, paths, batch: int, device="cuda", workers: int = 0, jpeg: str = "host", engine=None):
        import os
        import torch
        self.paths, self.batch, self.device = list(paths), batch, torch.device(device)
        if jpeg not in ("host", "device"):
            raise ValueError(f"FrameFeeder: jpeg must be 'host' or 'device', not {jpeg!r}")
        if jpeg == "device" and self.device.type != "cuda":
            raise ValueError("FrameFeeder: jpeg='device' reconstructs the frames on the GPU; device='cpu' has none")
        if jpeg == "device" and engine is None:
            raise ValueError("FrameFeeder: jpeg='device' needs engine= (the handle that launches the reconstruction kernels)")
        self.jpeg, self.engine = jpeg, engine
        self._pinned_coef = [None, None]
        self._pinned_png = [None, None]
        self.workers = workers if workers > 0 else default_decode_workers()
        self._torch = torch
        self._pinned = [None, None]
        self._lib = L.load()

    def close(self):
        self._pinned = [None, None]
        self._pinned_coef = [None, None]
        self._pinned_png = [None, None]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _decode_into(self, slot: int, lo: int, hi: int):
        torch = self._torch
        with open(self.paths[lo], "rb") as f:
            h, w = image_size(f.read())
        buf = self._pinned[slot]
        if buf is None or tuple(buf.shape[1:3]) != (h, w) or buf.shape[0] < hi - lo:
            buf = self._pinned[slot] = torch.empty((self.batch, h, w, 3), dtype=torch.uint8, pin_memory=self.device.type == "cuda")
        n = hi - lo
        arr = (C.c_char_p * n)(*[os_fsencode(p) for p in self.paths[lo:hi]])
        status = (C.c_int * n)()
        st = self._lib.sd_decode_files_bgr(arr, n, h, w, C.c_void_p(buf.data_ptr()), h * w * 3, self.workers, status)
        if st != L.SD_OK:
            bad = [(self.paths[lo + i], status[i]) for i in range(n) if status[i] != L.SD_OK]
            raise ValueError(f"FrameFeeder: {len(bad)} frame(s) of the batch could not be read as {h}x{w} PNG / JPEG frames: {bad[:3]}")
        return buf[:n]

    @staticmethod
    def _header_size(path) -> tuple:
        """(h, w) after the orientation from the head of the file: the frame header and the EXIF segment come before the first scan, so
        256 KiB nearly always hold them; the whole file is read only when they do not"""
        with open(path, "rb") as f:
            try:
                return image_size(f.read(256 << 10))
            except ValueError:
                f.seek(0)
                return image_size(f.read())

    @staticmethod
    def coef_stride_bytes(h: int, w: int) -> int:
        """bytes that hold the coefficients of any JPEG frame this reader takes whose size after the orientation is h x w: three
        components at the full rate, padded to whole 16 x 16 MCUs (4:4:4 needs 3 planes of 8-padded size, 4:2:0 1.5 of 16-padded
        size; the bound is symmetric in h and w, so it covers the transposing orientations), rounded up to the 16 bytes the kernels load"""
        return 3 * (-(-h // 16) * 16) * (-(-w // 16) * 16) * 2

    def _decode_coef_into(self, slot: int, lo: int, hi: int):
        """device route, host part of one batch: -> (pinned int16 [n, stride / 2] coefficients, descriptors, [(i, pinned BGR frame)]
        of the files that are not JPEGs, (h, w))"""
        torch = self._torch
        h, w = self._header_size(self.paths[lo])          # the header pass: the batch's frame size fixes the staging stride
        stride = self.coef_stride_bytes(h, w)
        n = hi - lo
        buf = self._pinned_coef[slot]
        if buf is None or buf.shape[1] != stride // 2 or buf.shape[0] < n:
            buf = self._pinned_coef[slot] = torch.empty((self.batch, stride // 2), dtype=torch.int16, pin_memory=True)
        arr = (C.c_char_p * n)(*[os_fsencode(p) for p in self.paths[lo:hi]])
        status = (C.c_int * n)()
        descs = (L.sd_jpeg_frame_desc * n)()
        st = self._lib.sd_decode_files_jpeg_coef(arr, n, h, w, C.c_void_p(buf.data_ptr()), stride, descs, self.workers, status)
        if st != L.SD_OK:
            bad = [(self.paths[lo + i], status[i]) for i in range(n) if status[i] not in (L.SD_OK, L.SD_ERR_FORMAT)]
            raise ValueError(f"FrameFeeder: {len(bad)} frame(s) of the batch could not be read as {h}x{w} PNG / JPEG frames: {bad[:3]}")
        others = [i for i in range(n) if status[i] == L.SD_ERR_FORMAT]
        png = []
        if others:                                        # not JPEGs: the BGR route, into a pinned buffer of their own
            pb = self._pinned_png[slot]
            if pb is None or tuple(pb.shape[1:3]) != (h, w):
                pb = self._pinned_png[slot] = torch.empty((self.batch, h, w, 3), dtype=torch.uint8, pin_memory=True)
            k = len(others)
            arr2 = (C.c_char_p * k)(*[os_fsencode(self.paths[lo + i]) for i in others])
            status2 = (C.c_int * k)()
            if self._lib.sd_decode_files_bgr(arr2, k, h, w, C.c_void_p(pb.data_ptr()), h * w * 3, self.workers, status2) != L.SD_OK:
                bad = [(self.paths[lo + i], status2[j]) for j, i in enumerate(others) if status2[j] != L.SD_OK]
                raise ValueError(f"FrameFeeder: {len(bad)} frame(s) of the batch could not be read as {h}x{w} PNG / JPEG frames: {bad[:3]}")
            png = [(i, pb[j]) for j, i in enumerate(others)]
        return buf[:n], descs, png, (h, w)

    def _reconstruct(self, host):
        """device route, GPU part of one batch, all on the current stream: per-frame asynchronous uploads of the coefficients each
        frame really has (a 4:2:0 frame has half of a 4:4:4 frame's), the two kernels, the PNG frames' uploads"""
        torch = self._torch
        coef, descs, png, (h, w) = host
        n = coef.shape[0]
        dev = torch.empty((n, h, w, 3), dtype=torch.uint8, device=self.device)
        is_png = {i for i, _ in png}
        jp = [i for i in range(n) if i not in is_png]
        if jp:
            cdev = torch.empty((len(jp), coef.shape[1]), dtype=torch.int16, device=self.device)
            sub = (L.sd_jpeg_frame_desc * len(jp))()
            for j, i in enumerate(jp):
                used = descs[i].coef_elems()
                cdev[j, :used].copy_(coef[i, :used], non_blocking=True)
                sub[j] = descs[i]
            # a run of consecutive JPEG frames is a contiguous slice of the batch tensor: the kernels write straight into it (a batch
            # without PNG files is one run), and nothing but the coefficient copies crosses the bus
            j0 = 0
            while j0 < len(jp):
                j1 = j0 + 1
                while j1 < len(jp) and jp[j1] == jp[j1 - 1] + 1:
                    j1 += 1
                run = (L.sd_jpeg_frame_desc * (j1 - j0))(*[sub[j] for j in range(j0, j1)])
                self.engine.jpeg_reconstruct(cdev[j0:j1], run, out=dev[jp[j0]:jp[j0] + (j1 - j0)])
                j0 = j1
        for i, frame in png:
            dev[i].copy_(frame, non_blocking=True)
        return dev

    def __iter__(self):
        torch = self._torch
        n = len(self.paths)
        ranges = [(a, min(a + self.batch, n)) for a in range(0, n, self.batch)]
        if not ranges:
            return
        with ThreadPoolExecutor(max_workers=1) as ahead:
            decode = self._decode_coef_into if self.jpeg == "device" else self._decode_into
            fut = ahead.submit(decode, 0, *ranges[0])
            events = [None, None]
            for k, (lo, hi) in enumerate(ranges):
                host = fut.result()
                if k + 1 < len(ranges):
                    slot = (k + 1) & 1
                    if events[slot] is not None:
                        events[slot].synchronize()          # the upload out of that staging buffer (two batches ago) has finished
                    fut = ahead.submit(decode, slot, *ranges[k + 1])
                dev = self._reconstruct(host) if self.jpeg == "device" else host.to(self.device, non_blocking=True)
                if self.device.type == "cuda":
                    events[k & 1] = torch.cuda.Event()
                    events[k & 1].record()
                yield dev, lo


def os_fsencode(p) -> bytes:
    import os
    return os.fsencode(p)
