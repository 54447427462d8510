#!/usr/bin/env python3
"""Golden vector for the JPEG reader: a progressive 4:2:0 frame with the scan script of the reference's example frame
(assets/images/test_munich/test_3.jpg, written by jpeg-recompress), which Pillow cannot produce: a JFIF header, a COM segment,
one DQT segment with both tables, a DHT segment before every scan, non-interleaved DC scans per component, luma AC in two spectral
bands at Al = 2 followed by two refinement scans, then each chroma AC band whole.

    Y  DC | Cb DC | Cr DC | Y AC 1-12 Al 2 | Y AC 13-63 Al 2 | Y AC 1-63 Ah 2 Al 1 | Y AC 1-63 Ah 1 Al 0 | Cb AC 1-63 | Cr AC 1-63

The encoder below is a plain numpy / Python restatement of ITU-T T.81 Annex G (progressive Huffman coding) with per-scan optimal
tables (Annex K.2).  The expected pixels are Pillow's decode (libjpeg-turbo at its default settings, what cv2.imread uses).
    python tests/golden/make_jpeg_scan_golden.py   ->  tests/golden/jpeg_scan_script.jpg + jpeg_scan_script.json
"""
import hashlib
import io
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
H, W = 389, 517                  # not multiples of the 16 x 16 MCU
QUALITY = 88
SCANS = [((0,), 0, 0, 0, 0), ((1,), 0, 0, 0, 0), ((2,), 0, 0, 0, 0),
         ((0,), 1, 12, 0, 2), ((0,), 13, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 1, 63, 1, 0),
         ((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0)]

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                    + [99] * 32)


def scaled(q):
    s = 5000 // QUALITY if QUALITY < 50 else 200 - 2 * QUALITY
    return np.clip((q * s + 50) // 100, 1, 255)


def image():
    """photo-like content: smooth shading, hard-edged shapes, fine texture and noise (every frequency band gets coefficients)"""
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    r = 120 + 90 * np.sin(xx / 57.0) * np.cos(yy / 41.0)
    g = 60 + 150 * yy / H
    b = 200 - 140 * xx / W
    for _ in range(14):
        cy, cx, rad = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(10, 70)
        m = (yy - cy) ** 2 + (xx - cx) ** 2 < rad ** 2
        col = rng.uniform(0, 255, 3)
        r[m], g[m], b[m] = col
    tex = 25 * np.sin(xx * 1.3 + yy * 0.7) * (xx > W / 2)
    a = np.stack([r + tex, g - tex, b], -1) + rng.normal(0, 6, (H, W, 3))
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def coefficients(rgb):
    """JFIF colour conversion, 2x2 chroma averaging, 8x8 FDCT, quantisation -> per component [rows, cols, 64] in zigzag order"""
    f = rgb.astype(np.float64)
    y = 0.299 * f[..., 0] + 0.587 * f[..., 1] + 0.114 * f[..., 2]
    cb = -0.168736 * f[..., 0] - 0.331264 * f[..., 1] + 0.5 * f[..., 2] + 128
    cr = 0.5 * f[..., 0] - 0.418688 * f[..., 1] - 0.081312 * f[..., 2] + 128
    ph, pw = -(-H // 16) * 16, -(-W // 16) * 16
    pad = lambda p: np.pad(p, ((0, ph - H), (0, pw - W)), mode="edge")
    y, cb, cr = pad(y), pad(cb), pad(cr)
    down = lambda p: p.reshape(ph // 2, 2, pw // 2, 2).mean(axis=(1, 3))
    u = np.arange(8)
    m = np.sqrt(np.where(u == 0, 1.0, 2.0) / 8)[:, None] * np.cos((2 * u[None, :] + 1) * u[:, None] * np.pi / 16)
    out = []
    for p, q in ((y, scaled(Q_LUMA)), (down(cb), scaled(Q_CHROMA)), (down(cr), scaled(Q_CHROMA))):
        bh, bw = p.shape[0] // 8, p.shape[1] // 8
        blk = (p - 128).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
        d = np.einsum("ux,abxy,vy->abuv", m, blk, m).reshape(bh, bw, 64)
        out.append(np.rint(d / q).astype(np.int64)[..., ZIGZAG])
    return out


class Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, n):
        for i in range(n - 1, -1, -1):
            self.acc = (self.acc << 1) | ((v >> i) & 1)
            self.n += 1
            if self.n == 8:
                self.out.append(self.acc)
                if self.acc == 0xFF:
                    self.out.append(0)
                self.acc, self.n = 0, 0

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


class Coder:
    """one scan's entropy coder; with ``table`` None it only counts symbols"""
    def __init__(self, table):
        self.table, self.freq, self.bits = table, np.zeros(256, np.int64), Bits()
        self.eobrun, self.be = 0, []

    def sym(self, s):
        self.freq[s] += 1
        if self.table is not None:
            code, n = self.table[s]
            self.bits.put(code, n)

    def put(self, v, n):
        if self.table is not None and n:
            self.bits.put(v, n)

    def emit_eobrun(self):
        if self.eobrun:
            nb = self.eobrun.bit_length() - 1
            self.sym(nb << 4)
            self.put(self.eobrun & ((1 << nb) - 1), nb)
            self.eobrun = 0
            for b in self.be:
                self.put(b, 1)
            self.be = []


def encode_scan(coef, Ss, Se, Ah, Al, coder, nblk):
    bh, bw = nblk
    last_dc = 0
    for i in range(bh):
        for j in range(bw):
            c = coef[i, j]
            if Ss == 0:                                            # DC first scan (Ah = 0 here)
                v = int(c[0]) >> Al
                d, last_dc = v - last_dc, v
                nb = abs(d).bit_length()
                coder.sym(nb)
                coder.put(d if d >= 0 else d - 1 + (1 << nb), nb)
            elif Ah == 0:                                          # AC first scan
                r = 0
                for k in range(Ss, Se + 1):
                    t = int(c[k])
                    a = abs(t) >> Al
                    if a == 0:
                        r += 1
                        continue
                    coder.emit_eobrun()
                    while r > 15:
                        coder.sym(0xF0)
                        r -= 16
                    nb = a.bit_length()
                    coder.sym((r << 4) + nb)
                    coder.put(a if t > 0 else (~a) & ((1 << nb) - 1), nb)
                    r = 0
                if r > 0:
                    coder.eobrun += 1
                    if coder.eobrun == 0x7FFF:
                        coder.emit_eobrun()
            else:                                                  # AC refinement scan
                absv = [abs(int(c[k])) >> Al for k in range(Ss, Se + 1)]
                eob = max([k for k, a in enumerate(absv) if a == 1], default=-1)
                r, br = 0, []
                for k, a in enumerate(absv):
                    if a == 0:
                        r += 1
                        continue
                    while r > 15 and k <= eob:
                        coder.emit_eobrun()
                        coder.sym(0xF0)
                        r -= 16
                        for b in br:
                            coder.put(b, 1)
                        br = []
                    if a > 1:
                        br.append(a & 1)
                        continue
                    coder.emit_eobrun()
                    coder.sym((r << 4) + 1)
                    coder.put(0 if c[Ss + k] < 0 else 1, 1)
                    for b in br:
                        coder.put(b, 1)
                    br, r = [], 0
                if r > 0 or br:
                    coder.eobrun += 1
                    coder.be += br
                    if coder.eobrun == 0x7FFF or len(coder.be) > 1000 - 64 + 1:
                        coder.emit_eobrun()
    coder.emit_eobrun()


def optimal_table(freq):
    """Annex K.2: code lengths limited to 16 bits -> (BITS[1..16], HUFFVAL)"""
    freq = list(int(f) for f in freq) + [1]
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1 = c2 = -1
        for i, f in enumerate(freq):
            if f and (c1 < 0 or f <= freq[c1]):
                c1 = i
        for i, f in enumerate(freq):
            if f and i != c1 and (c2 < 0 or f <= freq[c2]):
                c2 = i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * 33
    for s in codesize:
        if s:
            bits[s] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = [v for n in range(1, 33) for v in range(256) if codesize[v] == n]
    return bits[1:17], vals


def canonical(bits, vals):
    table, code, k = {}, 0, 0
    for n in range(1, 17):
        for _ in range(bits[n - 1]):
            table[vals[k]] = (code, n)
            code += 1
            k += 1
        code <<= 1
    return table


def segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def encode(rgb):
    coefs = coefficients(rgb)
    # blocks a non-interleaved scan covers: ceil(component size / 8) (A.2.2), not the MCU-padded count
    nblk = [(-(-H // 8), -(-W // 8)), (-(-H // 16), -(-W // 16)), (-(-H // 16), -(-W // 16))]
    out = bytearray(b"\xFF\xD8")
    out += segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += segment(0xFE, b"progressive 4:2:0, per-scan tables")
    out += segment(0xDB, bytes([0]) + bytes(scaled(Q_LUMA)[ZIGZAG].tolist()) + bytes([1]) + bytes(scaled(Q_CHROMA)[ZIGZAG].tolist()))
    out += segment(0xC2, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for comps, Ss, Se, Ah, Al in SCANS:
        ci = comps[0]
        counter = Coder(None)
        encode_scan(coefs[ci], Ss, Se, Ah, Al, counter, nblk[ci])
        bits, vals = optimal_table(counter.freq)
        tc, th = (0 if Ss == 0 else 1), (0 if ci == 0 else 1)
        out += segment(0xC4, bytes([(tc << 4) | th] + bits + vals))
        coder = Coder(canonical(bits, vals))
        encode_scan(coefs[ci], Ss, Se, Ah, Al, coder, nblk[ci])
        coder.bits.flush()
        sel = (th << 4) | th
        out += segment(0xDA, bytes([1, ci + 1, sel, Ss, Se, (Ah << 4) | Al]))
        out += coder.bits.out
    return bytes(out + b"\xFF\xD9")


def main():
    from PIL import Image
    rgb = image()
    buf = encode(rgb)
    im = Image.open(io.BytesIO(buf))
    assert im.info.get("progressive") and im.size == (W, H)
    bgr = np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])
    err = np.abs(bgr[..., ::-1].astype(np.int64) - rgb).mean()
    assert err < 10.0, err                                 # the stream decodes to the image it was made from (noise sigma 6)
    probes = [(0, 0), (H // 2, W // 2), (H - 1, W - 1), (7, W - 2), (H - 3, 9), (200, 300)]
    with open(os.path.join(HERE, "jpeg_scan_script.jpg"), "wb") as fh:
        fh.write(buf)
    with open(os.path.join(HERE, "jpeg_scan_script.json"), "w") as fh:
        json.dump({"made_with": "make_jpeg_scan_golden.py; expected pixels decoded by Pillow (libjpeg-turbo), default decode settings",
                   "file": "jpeg_scan_script.jpg", "file_sha256": hashlib.sha256(buf).hexdigest(), "shape": list(bgr.shape),
                   "scans": [[list(c), ss, se, ah, al] for c, ss, se, ah, al in SCANS],
                   "bgr_sha256": hashlib.sha256(bgr.tobytes()).hexdigest(),
                   "probe_pixels_bgr": {f"{y},{x}": bgr[y, x].tolist() for y, x in probes}}, fh, indent=1, sort_keys=True)
    print(f"wrote jpeg_scan_script.jpg ({len(buf)} bytes, mean abs error vs the source image {err:.2f})")


if __name__ == "__main__":
    main()
