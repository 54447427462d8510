"""Input stage, host side: the frame reader that replaces ``cv2.imread`` (semantic_depth.py:105; seq:123) and a
feeder that keeps the GPU supplied.

    imread(path)            8-bit PNG or Huffman JPEG -> u8 [h,w,3] BGR, exactly cv2.imread's IMREAD_COLOR result: ONE native call
                            (sd_png_decode_bgr: chunk walk, zlib inflate, scanline reconstruction, BGR shuffle, palette;
                            sd_jpeg_decode_bgr: libjpeg's default decode path and the EXIF orientation, restated)
    FrameFeeder             the sorted file list (seq:689) batch by batch: ONE native call per batch (sd_decode_files_bgr, C++ threads)
                            reads and decodes straight into a pinned staging buffer, one batch ahead of the GPU; the cubic resize to
                            the network shape happens ON the GPU (Engine.resize_cubic), so the host never touches a pixel after the decode

PNG decode stays on the host by default: DEFLATE and the PNG predictors are serial byte recurrences; a frame costs a few
milliseconds of one core (scripts/feed_rate.py measures decode, pinned H2D and resize rates against the benchmarked
frames/s; DESIGN.md quotes them).  ``png="device"`` keeps only the chunk walk and the inflate there (sd_inflate_files_png) and runs
the predictors -- a row per lane, the rows of a frame one pixel behind each other --, the channel shuffle and the palette lookup on
the GPU (Engine.png_reconstruct), byte for byte the host route's frames.  JPEG frames (the reference's own example frame is one) have two routes: ``jpeg="host"``, the
default, decodes them completely on the host threads as well; ``jpeg="device"`` keeps only the serial part there -- the Huffman
decoder, to quantised coefficients (sd_decode_files_jpeg_coef) -- and runs the inverse DCT, the chroma upsampling, the colour
conversion and the EXIF orientation on the GPU (Engine.jpeg_reconstruct), byte for byte the host route's frames;
``jpeg="device_entropy"`` moves the Huffman decoder to the GPU as well for files with restart intervals (the project's own encoder,
MJPEG cameras, Pillow's restart_marker_rows / restart_marker_blocks): the host only finds the markers (sd_plan_files_jpeg_entropy, a
byte scan), Engine.jpeg_entropy_decode decodes one restart interval per lane, and every other file falls back to the host decoder.
``jpeg="device_sync"`` reaches the files without restart intervals too: the host writes the scan without stuffing and markers
(sd_plan_files_jpeg_sync) and Engine.jpeg_sync_decode decodes it in short pieces that find the decoder's state by themselves.
"""
from __future__ import annotations

import ctypes as C
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib as L

SYNC_PIECE_BYTES = 64       # jpeg="device_sync": bytes of the clean stream one lane decodes ("JPEG entropy decoding in pieces")

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
    indices and batch boundaries are those of ``jpeg="host"``.
    ``jpeg="device_entropy"`` (same needs): the worker thread only PLANS the JPEG files of a batch (sd_plan_files_jpeg_entropy: header
    parse and a byte scan for the restart markers) and copies their scan bytes into pinned staging, one batch ahead as well.  The scan
    bytes go up instead of the coefficients -- also a much smaller upload, at most a few bits per coefficient instead of 16 -- and
    Engine.jpeg_entropy_decode fills the coefficient tensor on the GPU, one restart interval per lane; Engine.jpeg_reconstruct then runs
    as on the "device" route.  A file is eligible when it is a sequential 8-bit file with ONE interleaved scan, DRI > 0, and nothing in
    its scan data but stuffed bytes, the expected RSTk markers and the closing EOI (include/semdepth.h states the rule).  Every other
    JPEG (progressive, multi-scan, no restart intervals, truncated, stray markers) and every frame whose stream the kernel flags is
    decoded by the host decoder (sd_decode_files_jpeg_coef) and uploaded into its slot; a frame that decoder refuses as well raises what
    the "device" route raises.  ``entropy_fallback`` lists (global frame index, "ineligible" | "flagged") of the frames that took the
    host decoder during the last iteration.  The kernel's per-frame status words come back through pinned memory on a copy stream of
    the feeder's own: the feeder waits on that stream, never on the compute stream.  Frames, indices, batch boundaries and the PNG
    handling are those of the other routes.  It takes the Huffman decoder off the host threads; it is not the faster feeder yet: with one
    interval per MCU row it measured slower than ``jpeg="device"`` at 512x1024, 1024x2048 and 3024x4032.
    ``jpeg="device_sync"`` (same needs): the entropy route for files WITHOUT restart intervals as well -- what Pillow's default save,
    cv2.imwrite and most cameras write.  The worker thread plans the files (sd_plan_files_jpeg_sync) and writes their CLEAN streams
    (stuffing resolved, RST markers dropped) into pinned staging; Engine.jpeg_sync_decode cuts every interval -- a scan without DRI is
    one -- into pieces of ``sync_piece`` bytes that find the decoder's state by themselves, decodes a piece per lane and verifies the
    chain of states, so a status word of 0 means the sequential decode.  Ineligible files (progressive, multi-scan, stray markers) and
    frames the kernels flag (refused streams, pieces that did not synchronise, bits that ran out) go through the host decoder;
    ``sync_fallback`` lists them as ``entropy_fallback`` does.  Frames, indices and batch boundaries are those of the other routes.
    ``png="device"`` (same needs; combines with every ``jpeg=`` choice): the worker thread only walks the chunks of the batch's PNG
    files and inflates their IDAT streams into pinned staging (sd_inflate_files_png), one batch ahead as well.  The filtered scanlines
    go up as they are -- about the byte count of the BGR frame -- and Engine.png_reconstruct runs the filter recurrence, the channel
    map and the palette lookup on the GPU, a run of consecutive PNG frames per launch, straight into the batch tensor.  The files that
    are not PNGs go down the ``jpeg=`` route.  Frames, indices and batch boundaries are those of ``png="host"``; a file the inflate
    refuses, and a palette frame the kernel flags for an index beyond its palette, raise what the host route raises.  The status words
    are read back only for a batch that holds a palette frame, on the same copy stream ("PNG reconstruction on the
    device")."""

    def __init__(self, paths, batch: int, device="cuda", workers: int = 0, jpeg: str = "host", engine=None, png: str = "host",
                 sync_piece: int = SYNC_PIECE_BYTES):
        import os
        import torch
        self.paths, self.batch, self.device = list(paths), batch, torch.device(device)
        if png not in ("host", "device"):
            raise ValueError(f"FrameFeeder: png must be 'host' or 'device', not {png!r}")
        if png != "host" and self.device.type != "cuda":
            raise ValueError(f"FrameFeeder: png={png!r} reconstructs the frames on the GPU; device='cpu' has none")
        if png != "host" and engine is None:
            raise ValueError(f"FrameFeeder: png={png!r} needs engine= (the handle that launches the reconstruction kernels)")
        self.png = png
        self._pinned_rows = [None, None]
        self._others = [None, None]           # png="device": per staging slot, the feeder that takes the batch's files that are not PNGs
        if jpeg not in ("host", "device", "device_entropy", "device_sync"):
            raise ValueError(f"FrameFeeder: jpeg must be 'host', 'device', 'device_entropy' or 'device_sync', not {jpeg!r}")
        if sync_piece not in (32, 64, 128, 256, 512, 1024):
            raise ValueError(f"FrameFeeder: sync_piece must be a power of two from 32 to 1024, not {sync_piece!r}")
        self.sync_piece = sync_piece
        self.sync_fallback = []
        if jpeg != "host" and self.device.type != "cuda":
            raise ValueError(f"FrameFeeder: jpeg={jpeg!r} reconstructs the frames on the GPU; device='cpu' has none")
        if jpeg != "host" and engine is None:
            raise ValueError(f"FrameFeeder: jpeg={jpeg!r} needs engine= (the handle that launches the reconstruction kernels)")
        self.jpeg, self.engine = jpeg, engine
        self.entropy_fallback = []
        self._pinned_ent = [None, None]
        self._copy_stream = None
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
        self._pinned_ent = [None, None]
        self._pinned_rows = [None, None]
        for f in self._others:
            if f is not None:
                f.close()
        self._others = [None, None]

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

    def _host_coef(self, slot, idx, lo, h, w):
        """the host coefficient decoder on the files lo + i, i in idx -> (pinned int16 rows, descriptors), or the ValueError of the
        "device" route"""
        torch = self._torch
        stride = self.coef_stride_bytes(h, w)
        buf = self._pinned_coef[slot] if slot is not None else None
        if buf is None or buf.shape[1] != stride // 2 or buf.shape[0] < len(idx):
            buf = torch.empty((max(self.batch, len(idx)), stride // 2), dtype=torch.int16, pin_memory=True)
            if slot is not None:
                self._pinned_coef[slot] = buf
        k = len(idx)
        arr = (C.c_char_p * k)(*[os_fsencode(self.paths[lo + i]) for i in idx])
        status = (C.c_int * k)()
        descs = (L.sd_jpeg_frame_desc * k)()
        st = self._lib.sd_decode_files_jpeg_coef(arr, k, h, w, C.c_void_p(buf.data_ptr()), stride, descs, self.workers, status)
        if st != L.SD_OK:
            bad = [(self.paths[lo + i], status[j]) for j, i in enumerate(idx) if status[j] not in (L.SD_OK, L.SD_ERR_FORMAT)]
            raise ValueError(f"FrameFeeder: {len(bad)} frame(s) of the batch could not be read as {h}x{w} PNG / JPEG frames: {bad[:3]}")
        return buf, descs

    def _plan_into(self, slot: int, lo: int, hi: int):
        """entropy and sync routes, host part of one batch: the plan call into pinned staging (the sync route's writes the clean
        stream there), the host coefficient decoder for the JPEGs that are not eligible, the BGR route for the files that are not JPEGs"""
        sync = self.jpeg == "device_sync"
        frame_t, interval_t = (L.sd_jpeg_sync_frame, L.sd_jpeg_sync_interval) if sync else (L.sd_jpeg_entropy_frame, L.sd_jpeg_interval)
        import os
        torch = self._torch
        h, w = self._header_size(self.paths[lo])
        n = hi - lo
        sizes = []
        for p in self.paths[lo:hi]:
            try:
                sizes.append(os.path.getsize(p))
            except OSError:
                sizes.append(0)
        byte_stride = max(16, -(-max(sizes) // 16) * 16)            # the scan bytes are fewer than the file's
        ivs = max(64, min(-(-h // 8) * -(-w // 8), 16384))          # ranges per frame: a file with more falls back to the host decoder
        T = L.SD_JPEG_ENTROPY_TABLES
        st_ = self._pinned_ent[slot]
        if st_ is None or st_["bytes"].shape[1] < byte_stride or st_["ivs"] != ivs:
            def pin(nbytes):
                return torch.empty((nbytes,), dtype=torch.uint8, pin_memory=True)
            st_ = self._pinned_ent[slot] = dict(
                bytes=torch.empty((self.batch, byte_stride), dtype=torch.uint8, pin_memory=True), ivs=ivs,
                descs=pin(self.batch * C.sizeof(L.sd_jpeg_frame_desc)), frames=pin(self.batch * C.sizeof(frame_t)),
                tables=pin(self.batch * T * C.sizeof(L.sd_jpeg_huff_table)), intervals=pin(self.batch * ivs * C.sizeof(interval_t)),
                status=torch.empty((self.batch,), dtype=torch.int32, pin_memory=True))
        byte_stride = st_["bytes"].shape[1]
        # the records live in the pinned buffers: the C call uploads them with asynchronous copies, and a slot is not planned into again
        # before the event of its last batch has passed
        descs = (L.sd_jpeg_frame_desc * n).from_address(st_["descs"].data_ptr())
        frames = (frame_t * n).from_address(st_["frames"].data_ptr())
        tables = (L.sd_jpeg_huff_table * (n * T)).from_address(st_["tables"].data_ptr())
        intervals = (interval_t * (n * ivs)).from_address(st_["intervals"].data_ptr())
        arr = (C.c_char_p * n)(*[os_fsencode(p) for p in self.paths[lo:hi]])
        status = (C.c_int * n)()
        if sync:
            self._lib.sd_plan_files_jpeg_sync(arr, n, h, w, self.sync_piece, C.c_void_p(st_["bytes"].data_ptr()), byte_stride, descs, frames, tables,
                                              intervals, ivs, self.workers, status)
        else:
            self._lib.sd_plan_files_jpeg_entropy(arr, n, h, w, C.c_void_p(st_["bytes"].data_ptr()), byte_stride, descs, frames, tables, intervals,
                                                 ivs, self.workers, status)
        others = [i for i in range(n) if status[i] == L.SD_ERR_FORMAT]
        eligible = [i for i in range(n) if status[i] == L.SD_OK and frames[i].eligible]
        # every other file -- not eligible, unreadable, too large for the staging -- is the host decoder's: it decodes it or raises what
        # the "device" route raises for the batch
        fallback = [i for i in range(n) if i not in others and i not in eligible]
        fb = self._host_coef(slot, fallback, lo, h, w) if fallback else None
        png = []
        if others:
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
        return dict(n=n, lo=lo, size=(h, w), pinned=st_, descs=descs, frames=frames, tables=tables, intervals=intervals, ivs=ivs,
                    eligible=eligible, fallback=fallback, fb=fb, png=png)

    def _entropy_reconstruct(self, host):
        """entropy route, GPU part of one batch on the current stream: the scan bytes' upload, the entropy kernels, the uploads of the
        host-decoded frames, the status words' way back on the feeder's copy stream, then the reconstruction of the "device" route.
        The sync route is the same walk with Engine.jpeg_sync_decode on the clean streams; its flagged frames are real (a stream the
        pieces did not synchronise on, or whose bits ran out, is the host decoder's to decide) and are listed in ``sync_fallback``."""
        torch = self._torch
        sync = self.jpeg == "device_sync"
        fell = self.sync_fallback if sync else self.entropy_fallback
        n, lo, (h, w), pin = host["n"], host["lo"], host["size"], host["pinned"]
        dev = torch.empty((n, h, w, 3), dtype=torch.uint8, device=self.device)
        cstride = self.coef_stride_bytes(h, w) // 2
        descs = (L.sd_jpeg_frame_desc * n)()
        jp = sorted(host["eligible"] + host["fallback"])
        cdev = torch.empty((n, cstride), dtype=torch.int16, device=self.device) if jp else None
        if host["eligible"]:
            # whole rows of the staging buffer (its stride is the largest file of the batches so far): one contiguous pinned copy
            sdev = torch.empty((n, pin["bytes"].shape[1]), dtype=torch.uint8, device=self.device)
            sdev.copy_(pin["bytes"][:n], non_blocking=True)
            status = torch.empty((n,), dtype=torch.int32, device=self.device)
            if sync:
                self.engine.jpeg_sync_decode(sdev, host["descs"], host["frames"], host["tables"], host["intervals"], host["ivs"], self.sync_piece,
                                             out=cdev, status=status)
            else:
                self.engine.jpeg_entropy_decode(sdev, host["descs"], host["frames"], host["tables"], host["intervals"], host["ivs"], out=cdev,
                                                status=status)
            for i in host["eligible"]:
                descs[i] = host["descs"][i]
            if self._copy_stream is None:
                self._copy_stream = torch.cuda.Stream(self.device)
            done = torch.cuda.Event()
            done.record()
            with torch.cuda.stream(self._copy_stream):
                self._copy_stream.wait_event(done)
                pin["status"][:n].copy_(status, non_blocking=True)
            status.record_stream(self._copy_stream)
        if host["fallback"]:
            buf, fdescs = host["fb"]
            for j, i in enumerate(host["fallback"]):
                k = fdescs[j].coef_elems()
                cdev[i, :k].copy_(buf[j, :k], non_blocking=True)
                descs[i] = fdescs[j]
                fell.append((lo + i, "ineligible"))
        if host["eligible"]:
            self._copy_stream.synchronize()                 # the feeder's own stream: the status words are in pinned memory now
            flagged = [i for i in host["eligible"] if int(pin["status"][i]) != 0]
            # Defensive only: the tests know no stream the host decoder accepts and the kernel flags, so in practice the host decoder
            # raises here what the "device" route raises.  Should it accept, its coefficients replace the slot's.
            if flagged:
                buf, fdescs = self._host_coef(None, flagged, lo, h, w)
                pin["flagged_coef"] = buf                   # (pinned, read by asynchronous copies: kept until this staging slot is planned into again)
                for j, i in enumerate(flagged):
                    k = fdescs[j].coef_elems()
                    cdev[i, :k].copy_(buf[j, :k], non_blocking=True)
                    descs[i] = fdescs[j]
                    fell.append((lo + i, "flagged"))
                fell.sort()
        j0 = 0
        while j0 < len(jp):                                 # runs of consecutive JPEG frames, as on the "device" route
            j1 = j0 + 1
            while j1 < len(jp) and jp[j1] == jp[j1 - 1] + 1:
                j1 += 1
            run = (L.sd_jpeg_frame_desc * (j1 - j0))(*[descs[jp[j]] for j in range(j0, j1)])
            self.engine.jpeg_reconstruct(cdev[jp[j0]:jp[j0] + (j1 - j0)], run, out=dev[jp[j0]:jp[j0] + (j1 - j0)])
            j0 = j1
        for i, frame in host["png"]:
            dev[i].copy_(frame, non_blocking=True)
        return dev

    @staticmethod
    def png_rows_stride(h: int, w: int) -> int:
        """bytes that hold the filtered rows of any 8-bit PNG frame of h x w: a filter byte plus four channels per row, rounded up to the
        16 bytes the kernel loads"""
        return -(-(h * (1 + 4 * w)) // 16) * 16

    def _inflate_into(self, slot: int, lo: int, hi: int):
        """PNG device route, host part of one batch: the chunk walk and the inflate of every PNG file into pinned staging
        (sd_inflate_files_png); the files that are not PNGs go down the ``jpeg=`` route of a feeder of their own"""
        torch = self._torch
        h, w = self._header_size(self.paths[lo])
        stride = self.png_rows_stride(h, w)
        n = hi - lo
        st_ = self._pinned_rows[slot]
        if st_ is None or st_["rows"].shape[1] != stride:
            st_ = self._pinned_rows[slot] = dict(
                rows=torch.empty((self.batch, stride), dtype=torch.uint8, pin_memory=True),
                descs=torch.empty((self.batch * C.sizeof(L.sd_png_frame_desc),), dtype=torch.uint8, pin_memory=True),
                status=torch.empty((self.batch,), dtype=torch.int32, pin_memory=True))
        # the descriptors live in the pinned buffer: the C call uploads them with an asynchronous copy, and a slot is not inflated into
        # again before the event of its last batch has passed
        descs = (L.sd_png_frame_desc * n).from_address(st_["descs"].data_ptr())
        arr = (C.c_char_p * n)(*[os_fsencode(p) for p in self.paths[lo:hi]])
        status = (C.c_int * n)()
        st = self._lib.sd_inflate_files_png(arr, n, h, w, C.c_void_p(st_["rows"].data_ptr()), stride, descs, self.workers, status)
        if st != L.SD_OK:
            bad = [(self.paths[lo + i], status[i]) for i in range(n) if status[i] not in (L.SD_OK, L.SD_ERR_FORMAT)]
            raise ValueError(f"FrameFeeder: {len(bad)} frame(s) of the batch could not be read as {h}x{w} PNG / JPEG frames: {bad[:3]}")
        others = [i for i in range(n) if status[i] == L.SD_ERR_FORMAT]
        rest = None
        if others:
            sub = self._others[slot]
            if sub is None:
                sub = self._others[slot] = FrameFeeder([], self.batch, device=self.device, workers=self.workers, jpeg=self.jpeg,
                                                       engine=self.engine if self.jpeg != "host" else None, sync_piece=self.sync_piece)
            sub.paths = [self.paths[lo + i] for i in others]
            stage = {"host": sub._decode_into, "device": sub._decode_coef_into, "device_entropy": sub._plan_into, "device_sync": sub._plan_into}[self.jpeg]
            rest = stage(slot, 0, len(others))
            rh, rw = tuple(rest.shape[1:3]) if self.jpeg == "host" else (rest[3] if self.jpeg == "device" else rest["size"])
            if (rh, rw) != (h, w):
                bad = [(p, L.SD_ERR_INVALID) for p in sub.paths]
                raise ValueError(f"FrameFeeder: {len(bad)} frame(s) of the batch could not be read as {h}x{w} PNG / JPEG frames: {bad[:3]}")
        return dict(n=n, lo=lo, size=(h, w), pinned=st_, descs=descs, others=others, rest=rest, slot=slot)

    def _png_reconstruct(self, host):
        """PNG device route, GPU part of one batch on the current stream: the uploads of the rows each frame really has, one kernel per
        run of consecutive PNG frames writing straight into the batch tensor, the status words' way back on the feeder's copy stream when
        the batch holds a palette frame, then the frames of the other files"""
        torch = self._torch
        n, lo, (h, w), pin, descs = host["n"], host["lo"], host["size"], host["pinned"], host["descs"]
        dev = torch.empty((n, h, w, 3), dtype=torch.uint8, device=self.device)
        others = set(host["others"])
        pg = [i for i in range(n) if i not in others]
        status = None
        if pg:
            stride = pin["rows"].shape[1]
            rdev = torch.empty((n, stride), dtype=torch.uint8, device=self.device)
            status = torch.zeros((n,), dtype=torch.int32, device=self.device)
            for i in pg:
                used = -(-descs[i].rows_bytes() // 16) * 16
                rdev[i, :used].copy_(pin["rows"][i, :used], non_blocking=True)
            size = C.sizeof(L.sd_png_frame_desc)
            j0 = 0
            while j0 < len(pg):                                 # a run of consecutive PNG frames is a contiguous slice of the batch tensor
                j1 = j0 + 1
                while j1 < len(pg) and pg[j1] == pg[j1 - 1] + 1:
                    j1 += 1
                i0, m = pg[j0], j1 - j0
                run = (L.sd_png_frame_desc * m).from_address(pin["descs"].data_ptr() + i0 * size)
                self.engine.png_reconstruct(rdev[i0:i0 + m], run, out=dev[i0:i0 + m], status=status[i0:i0 + m])
                j0 = j1
        palette = [i for i in pg if descs[i].color_type == 3]
        if palette:                                             # only an index beyond the palette can be flagged
            if self._copy_stream is None:
                self._copy_stream = torch.cuda.Stream(self.device)
            done = torch.cuda.Event()
            done.record()
            with torch.cuda.stream(self._copy_stream):
                self._copy_stream.wait_event(done)
                pin["status"][:n].copy_(status, non_blocking=True)
            status.record_stream(self._copy_stream)
        if host["others"]:
            sub = self._others[host["slot"]]
            rest = host["rest"]
            if self.jpeg == "host":
                rdev2 = rest.to(self.device, non_blocking=True)
            else:
                rdev2 = (sub._reconstruct if self.jpeg == "device" else sub._entropy_reconstruct)(rest)
                self.entropy_fallback += [(lo + host["others"][j], why) for j, why in sub.entropy_fallback]
                self.sync_fallback += [(lo + host["others"][j], why) for j, why in sub.sync_fallback]
                del sub.entropy_fallback[:], sub.sync_fallback[:]
            for j, i in enumerate(host["others"]):
                dev[i].copy_(rdev2[j], non_blocking=True)
        if palette:
            self._copy_stream.synchronize()                     # the feeder's own stream: the status words are in pinned memory now
            bad = [(self.paths[lo + i], L.SD_ERR_INVALID) for i in palette if int(pin["status"][i]) != 0]
            if bad:                                             # what the host route raises for a file with an index beyond its palette
                raise ValueError(f"FrameFeeder: {len(bad)} frame(s) of the batch could not be read as {h}x{w} PNG / JPEG frames: {bad[:3]}")
        return dev

    def __iter__(self):
        torch = self._torch
        n = len(self.paths)
        ranges = [(a, min(a + self.batch, n)) for a in range(0, n, self.batch)]
        if not ranges:
            return
        with ThreadPoolExecutor(max_workers=1) as ahead:
            decode = {"host": self._decode_into, "device": self._decode_coef_into, "device_entropy": self._plan_into, "device_sync": self._plan_into}[self.jpeg]
            rebuild = {"device": self._reconstruct, "device_entropy": self._entropy_reconstruct, "device_sync": self._entropy_reconstruct}.get(self.jpeg)
            if self.png == "device":
                decode, rebuild = self._inflate_into, self._png_reconstruct
            self.entropy_fallback = []
            self.sync_fallback = []
            fut = ahead.submit(decode, 0, *ranges[0])
            events = [None, None]
            for k, (lo, hi) in enumerate(ranges):
                host = fut.result()
                if k + 1 < len(ranges):
                    slot = (k + 1) & 1
                    if events[slot] is not None:
                        events[slot].synchronize()          # the upload out of that staging buffer (two batches ago) has finished
                    fut = ahead.submit(decode, slot, *ranges[k + 1])
                dev = rebuild(host) if rebuild else host.to(self.device, non_blocking=True)
                if self.device.type == "cuda":
                    events[k & 1] = torch.cuda.Event()
                    events[k & 1].record()
                yield dev, lo


def os_fsencode(p) -> bytes:
    import os
    return os.fsencode(p)
