"""The files the sync-route tests run on (tests/test_jpeg_sync_cpu.py on the CPU, tests/test_gpu_jpeg_sync.py on the GPU), the calls they
compare, two hand-assembled streams, and a Python restatement of the passes of semantic_depth_amd/csrc/jpeg_sync.hpp with switches for
three seeded mistakes.  The yardstick everywhere is the existing host decoder (sd_jpeg_decode_coefficients / sd_jpeg_decode_bgr through
tests/jpeg_cases.py), never the new code against itself."""
import ctypes as C
import io

import numpy as np

import jpeg_cases as J
import jpeg_entropy_cases as E
from semantic_depth_amd import _lib as L

FILL16 = E.FILL16
PIECES = (32, 128)
GROUP = L.SD_JPEG_SYNC_GROUP


# ---------------------------------------------------------------------------------------------------------------- the files
def _save(PILImage, img, gray=False, **kw):
    b = io.BytesIO()
    im = PILImage.fromarray(img)
    (im.convert("L") if gray else im).save(b, "JPEG", **kw)
    return b.getvalue()


def dri_less_files(PILImage):
    """[(name, bytes)]: the recipes of jpeg_entropy_cases.pil_files saved without restart options, a gray frame, a 96 x 160 uniform-noise
    frame at quality 100 and 4:2:2 (about 40 KB: five workgroups of 32-byte pieces), a 16 x 16 frame whose scan is shorter than one
    128-byte piece"""
    rng = np.random.default_rng(32)
    out = []
    for opt in (False, True):
        for ss in (0, 1, 2):
            out.append((f"plain_50x70_ss{ss}{'_opt' if opt else ''}", _save(PILImage, J._img(rng, 50, 70), quality=85, subsampling=ss, optimize=opt)))
    out.append(("plain_gray_33x41", _save(PILImage, J._img(rng, 33, 41), gray=True, quality=80)))
    out.append(("plain_136x136_444", _save(PILImage, J._img(rng, 136, 136), quality=85, subsampling=0)))
    out.append(("plain_q100_noise_422_40x56", _save(PILImage, E._noise(rng, 40, 56), quality=100, subsampling=1)))
    out.append(("plain_q100_noise_422_96x160", _save(PILImage, E._noise(rng, 96, 160), quality=100, subsampling=1)))
    out.append(("plain_16x16_q30", _save(PILImage, J._img(rng, 16, 16), quality=30, subsampling=2)))
    for name, buf in out:
        assert b"\xff\xdd" not in buf, name
    assert len(out[-2][1]) > 4 * GROUP * 32 and len(out[-1][1]) - E.scan_start(out[-1][1]) < 128
    return out


def intact_files(PILImage):
    """every intact file of the issue: the entropy route's files (with DRI), the DRI-less ones, and the stream whose last token is fed by
    zero bits past the end"""
    return E.own_files() + E.pil_files(PILImage) + dri_less_files(PILImage) + [("crafted_last_token_past_the_end", last_token_past_the_end())]


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def crafted_gray(height, width, dc_bits, scan):
    """a gray baseline file around `scan`: quantisation table of ones, a DC table with the single code of dc_bits zeros (category 0), an AC
    table with 0x01 at 7 bits (code 0000000) and EOB at 8 bits (code 00000010)"""
    dc_counts = bytes(1 if l == dc_bits else 0 for l in range(1, 17))
    ac_counts = bytes(1 if l in (7, 8) else 0 for l in range(1, 17))
    return (b"\xff\xd8" + _seg(0xDB, b"\x00" + bytes([1] * 64)) + _seg(0xC0, b"\x08" + height.to_bytes(2, "big") + width.to_bytes(2, "big") + b"\x01\x01\x11\x00") +
            _seg(0xC4, b"\x00" + dc_counts + b"\x00") + _seg(0xC4, b"\x10" + ac_counts + b"\x01\x00") + _seg(0xDA, b"\x01\x01\x00\x00\x3f\x00") + scan + b"\xff\xd9")


def never_synchronising(height=160, width=160):
    """A stream on which a late starter never falls into step: every token is one byte (DC 00, AC +1 01, AC -1 00, EOB 02).  The first
    block is DC + EOB, every later block DC + 63 coefficients of +1 except the 62nd, which is -1 -- so every byte at a multiple of 64 is
    00, which a decoder waiting for a DC symbol accepts: started there it stays 62 zigzag positions off for ever and meets no anomaly.
    160 x 160: 400 blocks, 25538 bytes, 799 pieces of 32 bytes = more than three workgroups."""
    blocks = (height // 8) * (width // 8)
    later = bytes([0x00] + [0x00 if k == 62 else 0x01 for k in range(1, 64)])
    scan = b"\x00\x02" + later * (blocks - 1)
    assert all(scan[i] == 0 for i in range(0, len(scan), 64)) and b"\xff" not in scan
    return crafted_gray(height, width, 8, scan)


def last_token_past_the_end():
    """one 8 x 8 block: a 4-bit DC code and 63 coefficients of one byte each, the last one -1 (eight zero bits) beginning 4 bits before
    the end of the 63rd byte -- and the stream ends there: the token begins inside the scan and is completed by the zero bits both
    decoders supply past the end"""
    bits = "0000" + "00000001" * 62 + "0000"
    assert len(bits) == 504
    return crafted_gray(8, 8, 4, int(bits, 2).to_bytes(63, "big"))


def dri_less_mutation_seeds(PILImage):
    """the frame of jpeg_entropy_cases.mutation_seeds saved without restart options at subsampling 0, 1, 2"""
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:45, 0:61]
    a = (np.stack([(yy * 3 + xx) % 256, (xx * 5) % 256, (yy * xx) % 256], -1).astype(np.uint8)) ^ rng.integers(0, 32, (45, 61, 3), dtype=np.uint8)
    return [_save(PILImage, a, quality=80, subsampling=ss) for ss in (0, 1, 2)], rng


def damaged_scans(PILImage):
    """jpeg_entropy_cases.damaged_scans() (450 files with DRI) plus the same mutation on the DRI-less seeds (150 each)"""
    out = list(E.damaged_scans(PILImage))
    seeds, rng = dri_less_mutation_seeds(PILImage)
    for seed in seeds:
        lo, hi = E.scan_start(seed), len(seed) - 3
        for _ in range(150):
            f = bytearray(seed)
            for _ in range(int(rng.integers(1, 5))):
                f[int(rng.integers(lo, hi))] ^= 1 << int(rng.integers(0, 8))
            out.append(bytes(f))
    return out


# ---------------------------------------------------------------------------------------------------------------- the calls
class Plan:
    """sd_jpeg_sync_plan of one file at piece length S: status, desc, frame, tables, intervals, clean (the clean stream)"""

    def __init__(self, buf, S, cap=4096):
        self.buf, self.S = buf, S
        self.desc = L.sd_jpeg_frame_desc()
        self.frame = L.sd_jpeg_sync_frame()
        self.tables = (L.sd_jpeg_huff_table * L.SD_JPEG_ENTROPY_TABLES)()
        self.intervals = (L.sd_jpeg_sync_interval * cap)()
        room = np.full(len(buf) + 16, 0xEE, np.uint8)
        self.status = L.load().sd_jpeg_sync_plan(buf, len(buf), S, C.byref(self.desc), C.byref(self.frame), self.tables, self.intervals, cap,
                                                 room.ctypes.data_as(C.c_void_p), len(buf))
        self.clean = bytes(room[:self.frame.clean_bytes]) if self.eligible else b""
        assert (room[self.frame.clean_bytes if self.eligible else len(buf):] == 0xEE).all()      # (an ineligible file's walk may have written into its room)

    @property
    def eligible(self):
        return self.status == L.SD_OK and self.frame.eligible == 1


class Batch:
    """the arrays sd_jpeg_sync_decode(_host) take for a list of Plans of one piece length"""

    def __init__(self, plans):
        self.plans, B = plans, len(plans)
        self.B, self.S = B, plans[0].S
        el = [p for p in plans if p.eligible]
        self.byte_stride = max([16] + [-(-len(p.clean) // 16) * 16 for p in el])
        self.interval_stride = max([1] + [p.frame.n_intervals for p in el])
        self.max_pieces = max([1] + [p.frame.n_pieces for p in el])
        self.coef_stride = max([64] + [-(-p.desc.coef_elems() // 8) * 8 for p in el]) + 8        # (8 elements of room behind the largest frame)
        self.bytes = np.zeros((B, self.byte_stride), np.uint8)
        self.descs = (L.sd_jpeg_frame_desc * B)()
        self.frames = (L.sd_jpeg_sync_frame * B)()
        self.tables = (L.sd_jpeg_huff_table * (B * L.SD_JPEG_ENTROPY_TABLES))()
        self.intervals = (L.sd_jpeg_sync_interval * (B * self.interval_stride))()
        for b, p in enumerate(plans):
            self.descs[b] = p.desc
            self.frames[b] = p.frame
            if not p.eligible:
                self.frames[b].eligible = 0
                continue
            self.bytes[b, :len(p.clean)] = np.frombuffer(p.clean, np.uint8)
            for k in range(L.SD_JPEG_ENTROPY_TABLES):
                self.tables[b * L.SD_JPEG_ENTROPY_TABLES + k] = p.tables[k]
            for i in range(p.frame.n_intervals):
                self.intervals[b * self.interval_stride + i] = p.intervals[i]

    def _args(self, over):
        a = dict(byte_stride=self.byte_stride, descs=self.descs, frames=self.frames, intervals=self.intervals, interval_stride=self.interval_stride,
                 tables=self.tables, subseq_bytes=self.S, coef_stride_bytes=self.coef_stride * 2)
        a.update(over)
        return a

    def host(self, **over):
        """sd_jpeg_sync_decode_host -> (status of the call, int16 [B, coef_stride] filled with 0xA5 before it, int32 [B] status words)"""
        coef = np.full((self.B, self.coef_stride), FILL16, np.int16)
        status = np.full(self.B, -1, np.int32)
        a = self._args(over)
        st = L.load().sd_jpeg_sync_decode_host(self.bytes.ctypes.data_as(C.c_void_p), a["byte_stride"], a["descs"], a["frames"], a["intervals"],
                                               a["interval_stride"], a["tables"], self.B, a["subseq_bytes"], coef.ctypes.data_as(C.c_void_p),
                                               a["coef_stride_bytes"], status.ctypes.data_as(C.c_void_p))
        return st, coef, status

    def device(self, eng, **over):
        """sd_jpeg_sync_decode on the current stream -> (status of the call, device int16 [B, coef_stride] filled with 0xA5 before it,
        device int32 [B] filled with -1)"""
        import torch
        lib = L.load()
        dev = torch.from_numpy(self.bytes).cuda()
        coef = torch.full((self.B, self.coef_stride), int(FILL16), dtype=torch.int16, device="cuda")
        status = torch.full((self.B,), -1, dtype=torch.int32, device="cuda")
        need = C.c_size_t()
        assert lib.sd_jpeg_sync_workspace(self.B, self.interval_stride, self.max_pieces, C.byref(need)) == L.SD_OK
        ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
        a = self._args(dict(workspace_bytes=need.value))
        a.update(over)
        st = lib.sd_jpeg_sync_decode(eng.h, C.c_void_p(dev.data_ptr()), a["byte_stride"], a["descs"], a["frames"], a["intervals"], a["interval_stride"],
                                     a["tables"], self.B, a["subseq_bytes"], C.c_void_p(coef.data_ptr()), a["coef_stride_bytes"],
                                     C.c_void_p(status.data_ptr()), C.c_void_p(ws.data_ptr()), a["workspace_bytes"],
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()          # (the host arrays and the workspace live until the copies and kernels have run)
        return st, coef, status

    def copies(self):
        """deep copies of the records a test wants to damage: (descs, frames, intervals, tables)"""
        return ((L.sd_jpeg_frame_desc * self.B).from_buffer_copy(bytes(self.descs)),
                (L.sd_jpeg_sync_frame * self.B).from_buffer_copy(bytes(self.frames)),
                (L.sd_jpeg_sync_interval * len(self.intervals)).from_buffer_copy(bytes(self.intervals)),
                (L.sd_jpeg_huff_table * len(self.tables)).from_buffer_copy(bytes(self.tables)))


def check_frame(name, plan, coef_row, status_word):
    """jpeg_entropy_cases.check_frame: the frame equals sd_jpeg_decode_coefficients of the same file, status 0, the fill behind it intact"""
    E.check_frame(name, plan, coef_row, status_word)


# ---------------------------------------------------------------------------------------------------------------- the restatement
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
MISTAKES = ("compare_without_u", "own_by_end", "dc_not_reset")


def _extend(v, t):
    return v - (1 << t) + 1 if v < (1 << (t - 1)) else v


class Model:
    """The passes of jpeg_sync.hpp on one planned file, written from the header's prose: state (p, u, k); a token belongs to the piece in
    which it begins; zero bits past the interval's end; the carry-on rule; speculative rounds inside a workgroup of 256 pieces and inside an
    interval; one lane per later workgroup started from its predecessor's end record after the speculative pass; placement by an
    exclusive scan; the write pass with the verification; the DC scan per interval and component.  ``mistake``: one of MISTAKES."""

    def __init__(self, plan, mistake=None):
        assert mistake is None or mistake in MISTAKES
        self.mistake, fr = mistake, plan.frame
        self.fr, self.S = fr, plan.S
        self.bits = "".join(f"{b:08b}" for b in plan.clean)
        self.ivs = [(plan.intervals[i].begin, plan.intervals[i].end, plan.intervals[i].first_piece) for i in range(fr.n_intervals)]
        self.tab = [dict(look=list(t.look), mincode=list(t.mincode), maxcode=list(t.maxcode), valptr=list(t.valptr), vals=list(t.vals)) for t in plan.tables]
        self.luma = fr.comp_h[0] * fr.comp_v[0]
        self.upm = 1 if fr.ncomp == 1 else self.luma + 2
        self.elems = plan.desc.coef_elems()

    def _peek(self, p, k, end_bit):
        s = self.bits[p:max(p, min(p + k, end_bit))]
        return int(s.ljust(k, "0"), 2)

    def _sym(self, p, tab, end_bit):
        e = tab["look"][self._peek(p, 9, end_bit)]
        if e:
            return e & 255, e >> 8
        code = self._peek(p, 16, end_bit)
        for l in range(10, 17):
            c = code >> (16 - l)
            if tab["maxcode"][l] >= 0 and tab["mincode"][l] <= c <= tab["maxcode"][l]:
                return tab["vals"][tab["valptr"][l] + c - tab["mincode"][l]], l
        return -1, 0

    def _step(self, st, end_bit):
        """one token: -> (new state, events); events: ("c", zigzag index, value), ("a", code), ("u",)"""
        p, u, k = st
        c = 0 if u < self.luma else 1 + u - self.luma
        ev, done = [], False
        if k == 0:
            t, n = self._sym(p, self.tab[self.fr.comp_dc[c]], end_bit)
            if t < 0:
                return (p + 16, u, k), [("a", 1)]
            p += n
            if t > 15:
                ev.append(("a", 2))
                t = 0
            ev.append(("c", 0, _extend(self._peek(p, t, end_bit), t) if t else 0))
            p += t
            k = 1
        else:
            rs, n = self._sym(p, self.tab[4 + self.fr.comp_ac[c]], end_bit)
            if rs < 0:
                return (p + 16, u, k), [("a", 1)]
            p += n
            r, s = rs >> 4, rs & 15
            if not s:
                if r == 15:
                    k += 16
                    done = k > 63
                else:
                    done = True
            else:
                k += r
                v = _extend(self._peek(p, s, end_bit), s)
                p += s
                if k > 63:
                    ev.append(("a", 4))
                    done = True
                else:
                    ev.append(("c", k, v))
                    k += 1
                    done = k > 63
        if done:
            k, u = 0, (u + 1) % self.upm
            ev.append(("u",))
        return (p, u, k), ev

    def _run(self, st, iv_end, piece_end_bit):
        """every token of the piece from st -> (end state, events)"""
        events = []
        while st[0] < piece_end_bit:
            new, ev = self._step(st, iv_end * 8)
            if self.mistake == "own_by_end" and new[0] > piece_end_bit:
                break
            st = new
            events += ev
        return st, events

    def _same(self, a, b):
        return (a[0], a[2]) == (b[0], b[2]) if self.mistake == "compare_without_u" else a == b

    def _block(self, first_mcu, q):
        fr = self.fr
        m, u = first_mcu + q // self.upm, q % self.upm
        mx, my, mcus = m % fr.mcus_x, m // fr.mcus_x, fr.mcus_x * fr.mcus_y
        if u < self.luma:
            ch, cv = fr.comp_h[0], fr.comp_v[0]
            return ((my * cv + u // ch) * (fr.mcus_x * ch) + mx * ch + u % ch) * 64
        return (mcus * self.luma + (u - self.luma) * mcus + my * fr.mcus_x + mx) * 64

    def decode(self):
        """-> (status word, int16 coefficients)"""
        fr, S = self.fr, self.S
        where = []                                            # per piece: (interval, begin bit, end bit, first piece, last piece)
        for i, (b, e, fp) in enumerate(self.ivs):
            n = max(1, -(-(e - b) // S))
            for j in range(n):
                where.append((i, min(b + j * S, e) * 8, min(b + (j + 1) * S, e) * 8, fp, fp + n - 1))
        P = len(where)
        assert P == fr.n_pieces
        rec = [None] * P
        group_end = []
        for base in range(0, P, GROUP):
            lanes = min(GROUP, P - base)
            held, active = {}, {}
            for t in range(lanes):
                iv, b, e, fp, lp = where[base + t]
                st, ev = self._run((b, 0, 0), self.ivs[iv][1], e)
                rec[base + t] = (st, sum(1 for x in ev if x[0] == "u"))
                held[t] = st
                active[t] = base + t < min(lp, base + lanes - 1)
            r = 1
            while r < GROUP and any(active.values()):
                for t in range(lanes):
                    if not active[t]:
                        continue
                    j = base + t + r
                    iv, _, _, _, lp = where[base + t]
                    st, ev = self._run(held[t], self.ivs[iv][1], where[j][2])
                    stop = self._same(st, rec[j][0])
                    rec[j] = (st, sum(1 for x in ev if x[0] == "u"))
                    held[t] = st
                    if stop or j >= min(lp, base + lanes - 1):
                        active[t] = False
                r += 1
            group_end.append(rec[base + lanes - 1])
        for g in range(1, len(group_end)):
            first = g * GROUP
            iv, _, _, fp, lp = where[first]
            if fp == first:
                continue
            st = group_end[g - 1][0]
            for j in range(first, min(lp, first + GROUP - 1, P - 1) + 1):
                st, ev = self._run(st, self.ivs[iv][1], where[j][2])
                stop = self._same(st, rec[j][0])
                rec[j] = (st, sum(1 for x in ev if x[0] == "u"))
                if stop:
                    break
        before = np.concatenate([[0], np.cumsum([n for _, n in rec])])
        coef = np.zeros(self.elems, np.int16)
        status = 0
        total = fr.mcus_x * fr.mcus_y
        for i in range(P):
            iv, b, e, fp, lp = where[i]
            first_mcu = iv * fr.restart_interval
            limit = min(fr.restart_interval, total - first_mcu) * self.upm
            q = int(before[i] - before[fp])
            st, ev = self._run((b, 0, 0) if i == fp else rec[i - 1][0], self.ivs[iv][1], e)
            refusal, units = 0, 0
            for x in ev:
                if x[0] == "u":
                    q, units = q + 1, units + 1
                elif q < limit:
                    if x[0] == "c" and x[2]:
                        coef[self._block(first_mcu, q) + ZIGZAG[x[1]]] = x[2]
                    elif x[0] == "a" and not refusal:
                        refusal = x[1]
            code = refusal or (5 if not self._same(st, rec[i][0]) or units != rec[i][1] else (6 if i == lp and q < limit else 0))
            status = status or code
        for c in range(fr.ncomp):
            per = fr.comp_h[c] * fr.comp_v[c]
            pred = 0
            for j in range(total * per):
                m, r = j // per, j % per
                at = self._block(0, m * self.upm + (self.luma + c - 1 if c else r))
                head = r == 0 and m % fr.restart_interval == 0
                pred = int(coef[at]) if head and (self.mistake != "dc_not_reset" or j == 0) else pred + int(coef[at])
                if not -32767 <= pred <= 32767:
                    status = status or 3
                coef[at] = np.int16(((pred + 32768) & 0xFFFF) - 32768)
        return status, coef
