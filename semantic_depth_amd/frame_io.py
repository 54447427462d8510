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
frames/s; DESIGN.md quotes them), and JPEG frames (the reference's own example frame is one) are decoded completely on the host
threads as well.  The opt-in routes keep only the serial part of a decode on the host and finish the frames on the GPU, byte for byte
the host route's: ``png="device"`` (the PNG predictors), ``jpeg="device"`` (everything behind the Huffman decoder),
``jpeg="device_entropy"`` (the Huffman decoder too, for files with restart intervals) and ``jpeg="device_sync"`` (for files without
them as well).  Each is a stage of the feeder below, described there.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from types import SimpleNamespace

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
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 8
    q = _cgroup_cpu_quota()
    if q is not None:
        n = min(n, q)
    return max(1, min(n // _local_ranks(), 128))


def _runs(values):
    """(position of the first, length) of every run of consecutive integers in the ascending list ``values``: a run of consecutive
    frames is a contiguous slice of the batch tensor, so a kernel writes straight into it"""
    p0 = 0
    while p0 < len(values):
        p1 = p0 + 1
        while p1 < len(values) and values[p1] == values[p1 - 1] + 1:
            p1 += 1
        yield p0, p1 - p0
        p0 = p1


def _unreadable(bad, size) -> ValueError:
    """what every route raises for the (path, status) pairs ``bad`` of a batch"""
    h, w = size
    return ValueError(f"FrameFeeder: {len(bad)} frame(s) of the batch could not be read as {h}x{w} PNG / JPEG frames: {bad[:3]}")


@dataclass
class StagedBatch:
    """what the host halves of a batch hand to the device halves: ``n`` frames from global index ``lo`` of ``size`` (h, w) after the
    orientation; ``kind[i]`` names the stage that took frame i; ``pinned[name]`` is that stage's pinned staging in use (the asynchronous
    uploads read it, so it is not written again before the event of this batch has passed) and ``payload[name]`` what its host half made
    for its device half"""
    n: int
    lo: int
    size: tuple
    kind: list
    pinned: dict = field(default_factory=dict)
    payload: dict = field(default_factory=dict)


class _Stage:
    """one way from files to frames.  ``host(slot, batch, idx)`` runs on the worker thread: it reads the files ``idx`` (ascending batch
    indices) into the pinned staging of ``slot``, marks the frames it takes in ``batch.kind``, raises for a file nobody can read and
    returns the indices that are the next stage's.  ``device(batch, dev)`` runs on the consumer's thread: the uploads and launches of
    its frames on the current stream into the u8 [n,h,w,3] tensor ``dev`` (it makes the tensor when it is the first stage) -> dev.
    ``settle(batch)`` runs after every device half of the batch: the place for a read-back that need not hold up the other stages.
    Row j of a stage's staging and device tensors belongs to the file idx[j]."""
    name = None

    def __init__(self, feeder):
        self.f = feeder
        self.staging = [None, None]           # pinned, per slot: this stage's own, released by its close()

    def close(self):
        self.staging = [None, None]

    def settle(self, batch):
        pass

    def take(self, batch, idx):
        for i in idx:
            batch.kind[i] = self.name

    def rows(self, batch):
        """the rows j of this stage's frames"""
        return [j for j, i in enumerate(batch.payload[self.name].idx) if batch.kind[i] == self.name]

    def tensor(self, batch, dev):
        h, w = batch.size
        return dev if dev is not None else self.f._torch.empty((batch.n, h, w, 3), dtype=self.f._torch.uint8, device=self.f.device)

    def files(self, batch, idx, call, refuse=True):
        """one native batch call ``call(paths, k, status)`` on the files idx -> the per-file statuses; a file that is not the call's
        format (SD_ERR_FORMAT) is left to the next stage, any other failure raises unless ``refuse`` is off"""
        paths = [self.f.paths[batch.lo + i] for i in idx]
        arr = (C.c_char_p * len(idx))(*[os.fsencode(p) for p in paths])
        status = (C.c_int * len(idx))()
        if call(arr, len(idx), status) != L.SD_OK and refuse:
            raise _unreadable([(p, s) for p, s in zip(paths, status) if s not in (L.SD_OK, L.SD_ERR_FORMAT)], batch.size)
        return status


class _BgrStage(_Stage):
    """the last stage of every route and the only one of the default route: sd_decode_files_bgr (C++ threads, no interpreter lock)
    reads and decodes PNG and JPEG files completely, straight into pinned u8 frames; the device half is their asynchronous upload"""
    name = "bgr"

    def host(self, slot, batch, idx):
        f, torch = self.f, self.f._torch
        h, w = batch.size
        buf = self.staging[slot]
        if buf is None or tuple(buf.shape[1:3]) != (h, w):
            buf = self.staging[slot] = torch.empty((f.batch, h, w, 3), dtype=torch.uint8, pin_memory=f.device.type == "cuda")
        self.files(batch, idx, lambda arr, k, status: f._lib.sd_decode_files_bgr(arr, k, h, w, C.c_void_p(buf.data_ptr()), h * w * 3, f.workers, status))
        self.take(batch, idx)
        batch.pinned[self.name], batch.payload[self.name] = buf, SimpleNamespace(idx=idx)
        return []

    def device(self, batch, dev):
        buf, idx = batch.pinned[self.name], batch.payload[self.name].idx
        if dev is None:                                   # the whole batch is this stage's: one copy
            return buf[:batch.n].to(self.f.device, non_blocking=True)
        for j, i in enumerate(idx):
            dev[i].copy_(buf[j], non_blocking=True)
        return dev


class _JpegDeviceStage(_Stage):
    """what the stages that reconstruct JPEG frames on the GPU share: the host coefficient decoder and Engine.jpeg_reconstruct (inverse
    DCT, chroma upsampling, colour conversion, EXIF orientation), byte for byte the host decoder's frames"""

    def host_coef(self, batch, idx, buf=None):
        """the host Huffman decoder (sd_decode_files_jpeg_coef) on the files idx -> (pinned int16 rows -- ``buf`` where it fits --,
        descriptors, statuses)"""
        f, torch = self.f, self.f._torch
        h, w = batch.size
        stride = f.coef_stride_bytes(h, w)                # the batch's frame size fixes the staging stride
        if buf is None or buf.shape[1] != stride // 2 or buf.shape[0] < len(idx):
            buf = torch.empty((max(f.batch, len(idx)), stride // 2), dtype=torch.int16, pin_memory=True)
        descs = (L.sd_jpeg_frame_desc * len(idx))()
        status = self.files(batch, idx, lambda arr, k, status: f._lib.sd_decode_files_jpeg_coef(arr, k, h, w, C.c_void_p(buf.data_ptr()), stride, descs,
                                                                                                   f.workers, status))
        return buf, descs, status

    @staticmethod
    def replace_coef(cdev, descs, rows, buf, src):
        """a host decode of the frames ``rows`` takes their place: row p of the pinned ``buf`` with descriptor src[p] -> row rows[p] of
        ``cdev`` and of ``descs``, asynchronously"""
        for p, j in enumerate(rows):
            used = src[p].coef_elems()
            cdev[j, :used].copy_(buf[p, :used], non_blocking=True)
            descs[j] = src[p]

    def reconstruct(self, batch, dev, cdev, descs):
        idx, rows = batch.payload[self.name].idx, self.rows(batch)
        for p0, m in _runs([idx[j] for j in rows]):
            j0, i0 = rows[p0], idx[rows[p0]]
            run = (L.sd_jpeg_frame_desc * m)(*[descs[j] for j in range(j0, j0 + m)])
            self.f.engine.jpeg_reconstruct(cdev[j0:j0 + m], run, out=dev[i0:i0 + m])


class _CoefStage(_JpegDeviceStage):
    """``jpeg="device"``: the JPEG files are only entropy-decoded on the host, into a pinned int16 staging buffer; each frame's
    coefficients are uploaded asynchronously and Engine.jpeg_reconstruct writes the frames into the batch tensor behind the upload"""
    name = "coef"

    def host(self, slot, batch, idx):
        buf, descs, status = self.host_coef(batch, idx, self.staging[slot])
        self.staging[slot] = buf
        self.take(batch, [i for i, s in zip(idx, status) if s == L.SD_OK])
        batch.pinned[self.name], batch.payload[self.name] = buf, SimpleNamespace(idx=idx, descs=descs)
        return [i for i, s in zip(idx, status) if s == L.SD_ERR_FORMAT]

    def device(self, batch, dev):
        torch = self.f._torch
        buf, p, rows = batch.pinned[self.name], batch.payload[self.name], self.rows(batch)
        dev = self.tensor(batch, dev)
        if rows:
            cdev = torch.empty((len(p.idx), buf.shape[1]), dtype=torch.int16, device=self.f.device)
            for j in rows:                                # what each frame really has (a 4:2:0 frame has half of a 4:4:4 frame's)
                used = p.descs[j].coef_elems()
                cdev[j, :used].copy_(buf[j, :used], non_blocking=True)
            self.reconstruct(batch, dev, cdev, p.descs)
        return dev


class _EntropyStage(_JpegDeviceStage):
    """``jpeg="device_entropy"``: the worker thread only PLANS the JPEG files (sd_plan_files_jpeg_entropy: header parse and a byte scan
    for the restart markers) and copies their scan bytes into pinned staging.  The scan bytes go up instead of the coefficients -- at
    most a few bits per coefficient instead of 16 -- and Engine.jpeg_entropy_decode fills the coefficient tensor on the GPU, one restart
    interval per lane; Engine.jpeg_reconstruct then runs as on the "device" route.  A file is eligible when it is a sequential 8-bit
    file with ONE interleaved scan, DRI > 0, and nothing in its scan data but stuffed bytes, the expected RSTk markers and the closing
    EOI (include/semdepth.h states the rule).  Every other JPEG (progressive, multi-scan, no restart intervals, truncated, stray markers,
    too large for the staging) and every frame whose stream the kernel flags is decoded by the host decoder and uploaded into its slot;
    a frame that decoder refuses as well raises what the "device" route raises.  ``FrameFeeder.entropy_fallback`` lists those frames.
    It takes the Huffman decoder off the host threads; it is not the faster feeder yet: with one interval per MCU row it measured
    slower than ``jpeg="device"`` at 512x1024, 1024x2048 and 3024x4032."""
    name, fell = "entropy", "entropy_fallback"
    frame_t, interval_t = L.sd_jpeg_entropy_frame, L.sd_jpeg_interval

    def plan(self, arr, k, size, pin, plan, status):
        return self.f._lib.sd_plan_files_jpeg_entropy(arr, k, *size, C.c_void_p(pin.bytes.data_ptr()), pin.bytes.shape[1], plan.descs, plan.frames,
                                                      plan.tables, plan.intervals, plan.ivs, self.f.workers, status)

    def decode(self, sdev, plan, cdev, status):
        self.f.engine.jpeg_entropy_decode(sdev, plan.descs, plan.frames, plan.tables, plan.intervals, plan.ivs, out=cdev, status=status)

    def host(self, slot, batch, idx):
        f, torch = self.f, self.f._torch
        h, w = batch.size
        k = len(idx)
        sizes = []
        for i in idx:
            try:
                sizes.append(os.path.getsize(f.paths[batch.lo + i]))
            except OSError:
                sizes.append(0)
        byte_stride = max(16, -(-max(sizes) // 16) * 16)            # the scan bytes are fewer than the file's
        ivs = max(64, min(-(-h // 8) * -(-w // 8), 16384))          # ranges per frame: a file with more falls back to the host decoder
        T = L.SD_JPEG_ENTROPY_TABLES
        pin = self.staging[slot]
        if pin is None or pin.bytes.shape[1] < byte_stride or pin.ivs != ivs:
            def pinned(nbytes):
                return torch.empty((nbytes,), dtype=torch.uint8, pin_memory=True)
            pin = self.staging[slot] = SimpleNamespace(
                bytes=torch.empty((f.batch, byte_stride), dtype=torch.uint8, pin_memory=True), ivs=ivs, coef=None, flagged_coef=None,
                descs=pinned(f.batch * C.sizeof(L.sd_jpeg_frame_desc)), frames=pinned(f.batch * C.sizeof(self.frame_t)),
                tables=pinned(f.batch * T * C.sizeof(L.sd_jpeg_huff_table)), intervals=pinned(f.batch * ivs * C.sizeof(self.interval_t)),
                status=torch.empty((f.batch,), dtype=torch.int32, pin_memory=True))
        # the records live in the pinned buffers: the C call uploads them with asynchronous copies, and a slot is not planned into again
        # before the event of its last batch has passed
        plan = SimpleNamespace(idx=idx, ivs=ivs, descs=(L.sd_jpeg_frame_desc * k).from_address(pin.descs.data_ptr()),
                               frames=(self.frame_t * k).from_address(pin.frames.data_ptr()),
                               tables=(L.sd_jpeg_huff_table * (k * T)).from_address(pin.tables.data_ptr()),
                               intervals=(self.interval_t * (k * ivs)).from_address(pin.intervals.data_ptr()))
        status = self.files(batch, idx, lambda arr, k, status: self.plan(arr, k, batch.size, pin, plan, status), refuse=False)
        plan.eligible = [j for j in range(k) if status[j] == L.SD_OK and plan.frames[j].eligible]
        # every other JPEG -- not eligible, unreadable, too large for the staging -- is the host decoder's: it decodes it or raises what
        # the "device" route raises for the batch
        plan.fallback = [j for j in range(k) if status[j] != L.SD_ERR_FORMAT and j not in plan.eligible]
        if plan.fallback:
            pin.coef, plan.fdescs, _ = self.host_coef(batch, [idx[j] for j in plan.fallback], pin.coef)
        self.take(batch, [idx[j] for j in range(k) if status[j] != L.SD_ERR_FORMAT])
        batch.pinned[self.name], batch.payload[self.name] = pin, plan
        return [idx[j] for j in range(k) if status[j] == L.SD_ERR_FORMAT]

    def device(self, batch, dev):
        """the scan bytes' upload, the entropy kernels, the uploads of the host-decoded frames, the status words' way back on the
        feeder's copy stream, then the reconstruction of the "device" route"""
        f, torch = self.f, self.f._torch
        pin, plan = batch.pinned[self.name], batch.payload[self.name]
        dev = self.tensor(batch, dev)
        k = len(plan.idx)
        if not self.rows(batch):
            return dev
        fell = []
        descs = (L.sd_jpeg_frame_desc * k)()
        cdev = torch.empty((k, f.coef_stride_bytes(*batch.size) // 2), dtype=torch.int16, device=f.device)
        if plan.eligible:
            # whole rows of the staging buffer (its stride is the largest file of the batches so far): one contiguous pinned copy
            sdev = torch.empty((k, pin.bytes.shape[1]), dtype=torch.uint8, device=f.device)
            sdev.copy_(pin.bytes[:k], non_blocking=True)
            status = torch.empty((k,), dtype=torch.int32, device=f.device)
            self.decode(sdev, plan, cdev, status)
            for j in plan.eligible:
                descs[j] = plan.descs[j]
            arrived = f._read_back(status, pin.status[:k])
        if plan.fallback:
            self.replace_coef(cdev, descs, plan.fallback, pin.coef, plan.fdescs)
            fell += [(j, "ineligible") for j in plan.fallback]
        if plan.eligible:
            arrived()
            flagged = [j for j in plan.eligible if int(pin.status[j]) != 0]
            # On the entropy route this is defensive only: the tests know no stream the host decoder accepts and the kernel flags, so in
            # practice the host decoder raises here what the "device" route raises.  Should it accept, its coefficients replace the slot's
            # (from a pinned buffer that asynchronous copies read: kept until this staging slot is planned into again).
            if flagged:
                pin.flagged_coef, fdescs, _ = self.host_coef(batch, [plan.idx[j] for j in flagged])
                self.replace_coef(cdev, descs, flagged, pin.flagged_coef, fdescs)
                fell += [(j, "flagged") for j in flagged]
        f._fell_back(self.fell, [(batch.lo + plan.idx[j], why) for j, why in fell])
        self.reconstruct(batch, dev, cdev, descs)
        return dev


class _SyncStage(_EntropyStage):
    """``jpeg="device_sync"``: the entropy route for files WITHOUT restart intervals as well -- what Pillow's default save, cv2.imwrite
    and most cameras write.  The worker thread plans the files (sd_plan_files_jpeg_sync) and writes their CLEAN streams (stuffing
    resolved, RST markers dropped) into pinned staging; Engine.jpeg_sync_decode cuts every interval -- a scan without DRI is one -- into
    pieces of ``sync_piece`` bytes that find the decoder's state by themselves, decodes a piece per lane and verifies the chain of
    states, so a status word of 0 means the sequential decode.  Ineligible files (progressive, multi-scan, stray markers) and frames the
    kernels flag (refused streams, pieces that did not synchronise, bits that ran out: real cases, the host decoder's to decide) go
    through the host decoder; ``FrameFeeder.sync_fallback`` lists them."""
    name, fell = "sync", "sync_fallback"
    frame_t, interval_t = L.sd_jpeg_sync_frame, L.sd_jpeg_sync_interval

    def plan(self, arr, k, size, pin, plan, status):
        return self.f._lib.sd_plan_files_jpeg_sync(arr, k, *size, self.f.sync_piece, C.c_void_p(pin.bytes.data_ptr()), pin.bytes.shape[1], plan.descs,
                                                   plan.frames, plan.tables, plan.intervals, plan.ivs, self.f.workers, status)

    def decode(self, sdev, plan, cdev, status):
        self.f.engine.jpeg_sync_decode(sdev, plan.descs, plan.frames, plan.tables, plan.intervals, plan.ivs, self.f.sync_piece, out=cdev, status=status)


class _PngRowsStage(_Stage):
    """``png="device"``: the worker thread only walks the chunks of the PNG files and inflates their IDAT streams into pinned staging
    (sd_inflate_files_png).  The filtered scanlines go up as they are -- about the byte count of the BGR frame -- and
    Engine.png_reconstruct runs the filter recurrence, the channel map and the palette lookup on the GPU, a run of consecutive PNG
    frames per launch, straight into the batch tensor.  A file the inflate refuses, and a palette frame the kernel flags for an index
    beyond its palette, raise what the host route raises.  The status words are read back only for a batch that holds a palette frame,
    on the feeder's copy stream, after the other stages' launches ("PNG reconstruction on the device")."""
    name = "png_rows"

    def host(self, slot, batch, idx):
        f, torch = self.f, self.f._torch
        h, w = batch.size
        stride = f.png_rows_stride(h, w)
        pin = self.staging[slot]
        if pin is None or pin.rows.shape[1] != stride:
            pin = self.staging[slot] = SimpleNamespace(
                rows=torch.empty((f.batch, stride), dtype=torch.uint8, pin_memory=True),
                descs=torch.empty((f.batch * C.sizeof(L.sd_png_frame_desc),), dtype=torch.uint8, pin_memory=True),
                status=torch.empty((f.batch,), dtype=torch.int32, pin_memory=True))
        # the descriptors live in the pinned buffer: the C call uploads them with an asynchronous copy, and a slot is not inflated into
        # again before the event of its last batch has passed
        descs = (L.sd_png_frame_desc * len(idx)).from_address(pin.descs.data_ptr())
        status = self.files(batch, idx, lambda arr, k, status: f._lib.sd_inflate_files_png(arr, k, h, w, C.c_void_p(pin.rows.data_ptr()), stride, descs,
                                                                                             f.workers, status))
        self.take(batch, [i for i, s in zip(idx, status) if s == L.SD_OK])
        batch.pinned[self.name], batch.payload[self.name] = pin, SimpleNamespace(idx=idx, descs=descs, arrived=None, palette=[])
        return [i for i, s in zip(idx, status) if s == L.SD_ERR_FORMAT]

    def device(self, batch, dev):
        f, torch = self.f, self.f._torch
        pin, p, rows = batch.pinned[self.name], batch.payload[self.name], self.rows(batch)
        dev = self.tensor(batch, dev)
        if not rows:
            return dev
        k = len(p.idx)
        rdev = torch.empty((k, pin.rows.shape[1]), dtype=torch.uint8, device=f.device)
        status = torch.zeros((k,), dtype=torch.int32, device=f.device)
        for j in rows:                                              # the rows each frame really has
            used = -(-p.descs[j].rows_bytes() // 16) * 16
            rdev[j, :used].copy_(pin.rows[j, :used], non_blocking=True)
        for p0, m in _runs([p.idx[j] for j in rows]):
            j0, i0 = rows[p0], p.idx[rows[p0]]
            run = (L.sd_png_frame_desc * m).from_address(pin.descs.data_ptr() + j0 * C.sizeof(L.sd_png_frame_desc))
            f.engine.png_reconstruct(rdev[j0:j0 + m], run, out=dev[i0:i0 + m], status=status[j0:j0 + m])
        p.palette = [j for j in rows if p.descs[j].color_type == 3]
        if p.palette:                                               # only an index beyond the palette can be flagged
            p.arrived = f._read_back(status, pin.status[:k])
        return dev

    def settle(self, batch):
        pin, p = batch.pinned[self.name], batch.payload[self.name]
        if p.arrived:
            p.arrived()
            bad = [(self.f.paths[batch.lo + p.idx[j]], L.SD_ERR_INVALID) for j in p.palette if int(pin.status[j]) != 0]
            if bad:                                                 # what the host route raises for a file with an index beyond its palette
                raise _unreadable(bad, batch.size)


class FrameFeeder:
    """iterate over (frames u8 [n,h,w,3] on ``device``, first global index) for the sorted ``paths``, ``batch`` files at a time, one
    batch ahead of the consumer (two staging slots).  Every route yields the frames of ``frame_io.imread``, with the same indices and
    batch boundaries, and raises the same ValueError for a batch with a file that cannot be read at the batch's size (that of its first
    file).  ``png="device"`` and ``jpeg="device" | "device_entropy" | "device_sync"`` move work from the ``workers`` host threads to the
    GPU; they need ``engine`` (an engine.Engine whose handle launches the kernels) and a GPU ``device``.

    A route is a chain of stages (``stages``): the PNG-rows stage when ``png="device"``, the chosen JPEG stage, the host BGR stage.
    Each has a host half (worker thread: files -> pinned staging) and a device half (the consumer's thread: uploads and launches on
    the current stream); a stage handles the files it is given and names the rest, which go to the next stage.  The stages' docstrings
    describe the routes.  ``entropy_fallback`` / ``sync_fallback`` list (global frame index, "ineligible" | "flagged") of the frames that
    took the host decoder on those routes during the last iteration.  Status words come back through pinned memory on a copy stream of
    the feeder's own: the feeder waits on that stream, never on the compute stream."""

    def __init__(self, paths, batch: int, device="cuda", workers: int = 0, jpeg: str = "host", engine=None, png: str = "host",
                 sync_piece: int = SYNC_PIECE_BYTES):
        import torch
        self.paths, self.batch, self.device = list(paths), batch, torch.device(device)
        if png not in ("host", "device"):
            raise ValueError(f"FrameFeeder: png must be 'host' or 'device', not {png!r}")
        if png != "host" and self.device.type != "cuda":
            raise ValueError(f"FrameFeeder: png={png!r} reconstructs the frames on the GPU; device='cpu' has none")
        if png != "host" and engine is None:
            raise ValueError(f"FrameFeeder: png={png!r} needs engine= (the handle that launches the reconstruction kernels)")
        jpeg_stages = {"host": (), "device": (_CoefStage,), "device_entropy": (_EntropyStage,), "device_sync": (_SyncStage,)}
        if jpeg not in jpeg_stages:
            raise ValueError(f"FrameFeeder: jpeg must be 'host', 'device', 'device_entropy' or 'device_sync', not {jpeg!r}")
        if sync_piece not in (32, 64, 128, 256, 512, 1024):
            raise ValueError(f"FrameFeeder: sync_piece must be a power of two from 32 to 1024, not {sync_piece!r}")
        if jpeg != "host" and self.device.type != "cuda":
            raise ValueError(f"FrameFeeder: jpeg={jpeg!r} reconstructs the frames on the GPU; device='cpu' has none")
        if jpeg != "host" and engine is None:
            raise ValueError(f"FrameFeeder: jpeg={jpeg!r} needs engine= (the handle that launches the reconstruction kernels)")
        self.png, self.jpeg, self.engine, self.sync_piece = png, jpeg, engine, sync_piece
        self.entropy_fallback, self.sync_fallback = [], []
        self.workers = workers if workers > 0 else default_decode_workers()
        self._torch = torch
        self._lib = L.load()
        self._copy_stream = None
        self.stages = [stage(self) for stage in ((_PngRowsStage,) if png == "device" else ()) + jpeg_stages[jpeg] + (_BgrStage,)]

    def close(self):
        for stage in self.stages:
            stage.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

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

    @staticmethod
    def png_rows_stride(h: int, w: int) -> int:
        """bytes that hold the filtered rows of any 8-bit PNG frame of h x w: a filter byte plus four channels per row, rounded up to the
        16 bytes the kernel loads"""
        return -(-(h * (1 + 4 * w)) // 16) * 16

    def _decode_into(self, slot: int, lo: int, hi: int) -> StagedBatch:
        """the host half of one batch, on the worker thread: the size of the first file is the batch's, every stage takes its files of
        those it is given and the rest goes to the next stage"""
        batch = StagedBatch(hi - lo, lo, self._header_size(self.paths[lo]), [None] * (hi - lo))
        rest = list(range(hi - lo))
        for stage in self.stages:
            if rest:
                rest = stage.host(slot, batch, rest)
        return batch

    def _upload(self, batch: StagedBatch):
        """the device half of one batch, all on the current stream, stage by stage -> the u8 [n,h,w,3] device tensor"""
        mine = [stage for stage in self.stages if stage.name in batch.payload]
        dev = None
        for stage in mine:
            dev = stage.device(batch, dev)
        for stage in mine:
            stage.settle(batch)
        return dev

    def _read_back(self, status, pinned):
        """start the copy of the device tensor ``status`` into ``pinned`` on the feeder's own stream, behind the work queued on the current
        stream so far -> a function that returns once the words are in pinned memory"""
        torch = self._torch
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(self.device)
        done = torch.cuda.Event()
        done.record()
        with torch.cuda.stream(self._copy_stream):
            self._copy_stream.wait_event(done)
            pinned.copy_(status, non_blocking=True)
        status.record_stream(self._copy_stream)
        return self._copy_stream.synchronize

    def _fell_back(self, which: str, frames):
        """note (global index, why) of frames that took the host decoder in ``entropy_fallback`` or ``sync_fallback``"""
        fell = getattr(self, which)
        fell += frames
        fell.sort()

    def __iter__(self):
        torch = self._torch
        n = len(self.paths)
        ranges = [(a, min(a + self.batch, n)) for a in range(0, n, self.batch)]
        if not ranges:
            return
        with ThreadPoolExecutor(max_workers=1) as ahead:
            self.entropy_fallback, self.sync_fallback = [], []
            fut = ahead.submit(self._decode_into, 0, *ranges[0])
            events = [None, None]
            for k, (lo, hi) in enumerate(ranges):
                host = fut.result()
                if k + 1 < len(ranges):
                    slot = (k + 1) & 1
                    if events[slot] is not None:
                        events[slot].synchronize()          # the upload out of that staging buffer (two batches ago) has finished
                    fut = ahead.submit(self._decode_into, slot, *ranges[k + 1])
                dev = self._upload(host)
                if self.device.type == "cuda":
                    events[k & 1] = torch.cuda.Event()
                    events[k & 1].record()
                yield dev, lo
