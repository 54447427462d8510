"""The files the entropy-route tests run on (tests/test_jpeg_entropy_cpu.py on the CPU, tests/test_gpu_jpeg_entropy.py on the GPU) and the
calls they compare.  The yardstick everywhere is the existing host decoder (sd_jpeg_decode_coefficients / sd_jpeg_decode_bgr through
tests/jpeg_cases.py), never the new code against itself."""
import ctypes as C
import io

import numpy as np

import jpeg_cases as J
from semantic_depth_amd import _lib as L

FILL = 0xA5
FILL16 = np.frombuffer(bytes([FILL, FILL]), np.int16)[0]


def own_jpeg(img, quality):
    """the project's encoder (sd_jpeg_encode_bgr_host): one restart interval per MCU row"""
    from semantic_depth_amd import outputs
    return outputs.encode_jpeg_host(np.ascontiguousarray(img), quality)


def _noise(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def own_files():
    """[(name, bytes)] from the project's encoder: one interval without any RST marker, padding in both directions, an EOB- and
    ZRL-heavy file, codes longer than 9 bits with dozens of stuffed bytes, 11 intervals (the RST counter wraps)"""
    rng = np.random.default_rng(31)
    out = [("own_16x16_q50", own_jpeg(J._img(rng, 16, 16), 50)),
           ("own_17x23_q75", own_jpeg(J._img(rng, 17, 23), 75)),
           ("own_48x80_q1", own_jpeg(J._img(rng, 48, 80), 1)),
           ("own_48x80_q100_noise", own_jpeg(_noise(rng, 48, 80), 100)),
           ("own_176x16_q80", own_jpeg(J._img(rng, 176, 16), 80))]
    assert b"\xff\xd0" not in out[0][1][600:] and out[3][1].count(b"\xff\x00") >= 24
    return out


def pil_files(PILImage):
    """[(name, bytes)] written by Pillow with restart intervals: intervals that cross MCU rows and a short last one at the three
    samplings, file-specific tables, a gray frame, 289 intervals of one MCU, quality 100 on noise at 4:2:2"""
    rng = np.random.default_rng(32)
    out = []

    def save(name, img, gray=False, **kw):
        b = io.BytesIO()
        im = PILImage.fromarray(img)
        (im.convert("L") if gray else im).save(b, "JPEG", **kw)
        assert b"\xff\xdd" in b.getvalue(), name
        out.append((name, b.getvalue()))
    for opt in (False, True):
        for ss in (0, 1, 2):
            save(f"pil_50x70_blocks3_ss{ss}{'_opt' if opt else ''}", J._img(rng, 50, 70), quality=85, subsampling=ss, restart_marker_blocks=3, optimize=opt)
    save("pil_gray_33x41_rows1", J._img(rng, 33, 41), gray=True, quality=80, restart_marker_rows=1)
    save("pil_136x136_blocks1_444", J._img(rng, 136, 136), quality=85, subsampling=0, restart_marker_blocks=1)
    save("pil_q100_noise_422", _noise(rng, 40, 56), quality=100, subsampling=1, restart_marker_blocks=2)
    return out


def mutation_seeds(PILImage):
    """the frame recipe of jpeg_cases.mutated_jpegs (45 x 61, rng seed 11, q80) saved with restart_marker_blocks=2 at subsampling 0, 1, 2"""
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:45, 0:61]
    a = (np.stack([(yy * 3 + xx) % 256, (xx * 5) % 256, (yy * xx) % 256], -1).astype(np.uint8)) ^ rng.integers(0, 32, (45, 61, 3), dtype=np.uint8)
    seeds = []
    for ss in (0, 1, 2):
        b = io.BytesIO()
        PILImage.fromarray(a).save(b, "JPEG", quality=80, subsampling=ss, restart_marker_blocks=2)
        seeds.append(b.getvalue())
    return seeds, rng


def scan_start(buf):
    """offset of the first byte of entropy-coded data (behind the first SOS header)"""
    p = 2
    while True:
        assert buf[p] == 0xFF
        m, n = buf[p + 1], int.from_bytes(buf[p + 2:p + 4], "big")
        if m == 0xDA:
            return p + 2 + n
        p += 2 + n


def damaged_scans(PILImage):
    """[bytes]: 150 mutations per seed, each flipping 1..4 random bits at positions from the first scan byte to three bytes before the end"""
    seeds, rng = mutation_seeds(PILImage)
    out = []
    for seed in seeds:
        lo, hi = scan_start(seed), len(seed) - 3
        for _ in range(150):
            f = bytearray(seed)
            for _ in range(int(rng.integers(1, 5))):
                f[int(rng.integers(lo, hi))] ^= 1 << int(rng.integers(0, 8))
            out.append(bytes(f))
    return out


# ---------------------------------------------------------------------------------------------------------------- the calls
class Plan:
    """sd_jpeg_entropy_plan of one file: status, desc, frame, tables, intervals (a ctypes array of ``cap`` entries)"""

    def __init__(self, buf, cap=4096):
        self.buf = buf
        self.desc = L.sd_jpeg_frame_desc()
        self.frame = L.sd_jpeg_entropy_frame()
        self.tables = (L.sd_jpeg_huff_table * L.SD_JPEG_ENTROPY_TABLES)()
        self.intervals = (L.sd_jpeg_interval * cap)()
        self.status = L.load().sd_jpeg_entropy_plan(buf, len(buf), C.byref(self.desc), C.byref(self.frame), self.tables, self.intervals, cap)

    @property
    def eligible(self):
        return self.status == L.SD_OK and self.frame.eligible == 1

    @property
    def scan(self):
        return self.buf[self.frame.scan_begin:self.frame.scan_end]


class Batch:
    """the arrays sd_jpeg_entropy_decode(_host) take for a list of Plans: scan bytes at a 16-byte stride, records, tables, ranges at
    ``interval_stride``, a coefficient stride that holds the largest frame (a multiple of 16 bytes)"""

    def __init__(self, plans):
        self.plans, B = plans, len(plans)
        self.B = B
        el = [p for p in plans if p.eligible]
        self.byte_stride = max([16] + [-(-len(p.scan) // 16) * 16 for p in el])
        self.interval_stride = max([1] + [p.frame.n_intervals for p in el])
        self.coef_stride = max([64] + [-(-p.desc.coef_elems() // 8) * 8 for p in el]) + 8        # (8 elements of room behind the largest frame)
        self.bytes = np.zeros((B, self.byte_stride), np.uint8)
        self.descs = (L.sd_jpeg_frame_desc * B)()
        self.frames = (L.sd_jpeg_entropy_frame * B)()
        self.tables = (L.sd_jpeg_huff_table * (B * L.SD_JPEG_ENTROPY_TABLES))()
        self.intervals = (L.sd_jpeg_interval * (B * self.interval_stride))()
        for b, p in enumerate(plans):
            self.descs[b] = p.desc
            self.frames[b] = p.frame
            if not p.eligible:
                self.frames[b].eligible = 0
                continue
            self.bytes[b, :len(p.scan)] = np.frombuffer(p.scan, np.uint8)
            for k in range(L.SD_JPEG_ENTROPY_TABLES):
                self.tables[b * L.SD_JPEG_ENTROPY_TABLES + k] = p.tables[k]
            for i in range(p.frame.n_intervals):
                self.intervals[b * self.interval_stride + i] = p.intervals[i]

    def host(self, **over):
        """sd_jpeg_entropy_decode_host -> (status of the call, int16 [B, coef_stride] filled with 0xA5 before it, int32 [B] status words)"""
        coef = np.full((self.B, self.coef_stride), FILL16, np.int16)
        status = np.full(self.B, -1, np.int32)
        a = dict(byte_stride=self.byte_stride, descs=self.descs, frames=self.frames, intervals=self.intervals,
                 interval_stride=self.interval_stride, coef_stride_bytes=self.coef_stride * 2)
        a.update(over)
        st = L.load().sd_jpeg_entropy_decode_host(self.bytes.ctypes.data_as(C.c_void_p), a["byte_stride"], a["descs"], a["frames"], a["intervals"],
                                                  a["interval_stride"], self.tables, self.B, coef.ctypes.data_as(C.c_void_p), a["coef_stride_bytes"],
                                                  status.ctypes.data_as(C.c_void_p))
        return st, coef, status

    def device(self, eng, **over):
        """sd_jpeg_entropy_decode on the current stream -> (status of the call, device int16 [B, coef_stride] filled with 0xA5 before it,
        device int32 [B] filled with -1)"""
        import torch
        lib = L.load()
        dev = torch.from_numpy(self.bytes).cuda()
        coef = torch.full((self.B, self.coef_stride), int(FILL16), dtype=torch.int16, device="cuda")
        status = torch.full((self.B,), -1, dtype=torch.int32, device="cuda")
        need = C.c_size_t()
        assert lib.sd_jpeg_entropy_workspace(self.B, self.interval_stride, C.byref(need)) == L.SD_OK
        ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
        a = dict(byte_stride=self.byte_stride, descs=self.descs, frames=self.frames, intervals=self.intervals,
                 interval_stride=self.interval_stride, coef_stride_bytes=self.coef_stride * 2, workspace_bytes=need.value)
        a.update(over)
        st = lib.sd_jpeg_entropy_decode(eng.h, C.c_void_p(dev.data_ptr()), a["byte_stride"], a["descs"], a["frames"], a["intervals"],
                                        a["interval_stride"], self.tables, self.B, C.c_void_p(coef.data_ptr()), a["coef_stride_bytes"],
                                        C.c_void_p(status.data_ptr()), C.c_void_p(ws.data_ptr()), a["workspace_bytes"],
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()          # (the host arrays and the workspace live until the copies and kernels have run)
        return st, coef, status

    def copies(self):
        """deep copies of the records a test wants to damage: (descs, frames, intervals)"""
        return ((L.sd_jpeg_frame_desc * self.B).from_buffer_copy(bytes(self.descs)),
                (L.sd_jpeg_entropy_frame * self.B).from_buffer_copy(bytes(self.frames)),
                (L.sd_jpeg_interval * len(self.intervals)).from_buffer_copy(bytes(self.intervals)))


def check_frame(name, plan, coef_row, status_word):
    """frame decoded by the new code == sd_jpeg_decode_coefficients of the same file: descriptor bytes, every coefficient, status 0, and
    the fill behind the frame's own elements"""
    st, ref, d = J.coef_decode(plan.buf)
    assert st == L.SD_OK, name
    assert bytes(plan.desc) == bytes(d), name
    n = d.coef_elems()
    assert status_word == 0, (name, int(status_word))
    assert np.array_equal(coef_row[:n], ref[:n]), (name, int((coef_row[:n] != ref[:n]).sum()))
    assert (coef_row[n:] == FILL16).all(), name
