"""Shared by tests/test_png_device_cpu.py and tests/test_gpu_png_device.py: the numpy statement of the filtered bytes of the device
PNG route (include/semdepth.h), frames whose residual stream is forced byte by byte, and a parser of a dynamic block's header."""
import ctypes as C
import zlib

import numpy as np

from semantic_depth_amd import _lib as L

CHUNK = 32768            # C of the stream format


def lib():
    import __graft_entry__ as graft
    graft.build()
    return L.load()


def bound(h, w):
    n = h * (1 + 3 * w)
    return 2 + n + 16 * (-(-n // CHUNK)) + 16


def encode_host(img):
    """sd_png_encode_zlib_host(img) as bytes"""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    ws, stride, size = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert lib().sd_png_encode_workspace(1, h, w, C.byref(ws), C.byref(stride)) == L.SD_OK
    assert stride.value == bound(h, w)
    out = np.full(stride.value, 0xA5, np.uint8)
    st = lib().sd_png_encode_zlib_host(img.ctypes.data_as(C.c_void_p), h, w, out.ctypes.data_as(C.c_void_p), out.size, C.byref(size))
    assert st == L.SD_OK, st
    return out[:size.value].tobytes()


def paeth_rows(img):
    """u8 [h, 1 + 3w]: filter byte 4 and the Paeth residuals of the RGB bytes (bpp 3, zero outside the image)"""
    h, w = img.shape[:2]
    x = img[..., ::-1].reshape(h, 3 * w).astype(np.int32)
    a = np.zeros_like(x); a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x); b[1:] = x[:-1]
    c = np.zeros_like(x); c[1:, 3:] = x[:-1, :-3]
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    rows = np.empty((h, 1 + 3 * w), np.uint8)
    rows[:, 0] = 4
    rows[:, 1:] = (x - pred).astype(np.uint8)
    return rows


def unfilter(rows, h, w):
    rows = np.ascontiguousarray(rows, np.uint8)
    out = np.empty((h, w, 3), np.uint8)
    assert lib().sd_png_unfilter_bgr(rows.ctypes.data_as(C.c_void_p), h, w, 3, out.ctypes.data_as(C.c_void_p)) == L.SD_OK
    return out


def forced(h, w, flat):
    """(image, filtered bytes): the image whose filtered bytes are ``flat`` (length h (1 + 3w)) with every row's first byte set to 4 --
    filter and unfilter are inverse, so the encoder sees exactly these residuals"""
    rows = np.array(flat, np.uint8).reshape(h, 1 + 3 * w).copy()
    rows[:, 0] = 4
    img = unfilter(rows, h, w)
    assert np.array_equal(paeth_rows(img), rows)
    return img, rows.reshape(-1)


def shape_for(n):
    """(h, w) with h (1 + 3w) == n, both within 1..16384, the squarest such frame"""
    best = None
    for w in range(1, 16385):
        if n % (1 + 3 * w) == 0 and 1 <= n // (1 + 3 * w) <= 16384:
            h = n // (1 + 3 * w)
            if best is None or abs(h - w) < abs(best[0] - best[1]):
                best = (h, w)
    assert best is not None, n
    return best


RUNS = (3, 4, 258, 259, 260, 261, 262, 516, 517)


def forced_cases():
    """name -> (h, w, flat filtered bytes before the row starts are set to 4).  Long runs are runs of the byte 4, so that a row's filter
    byte falls inside them without cutting them."""
    rng = np.random.default_rng(7)
    cases = {}
    # one value over three chunks: each chunk is one literal and matches only
    cases["constant_3_chunks"] = (40, 700, np.full(40 * 2101, 4, np.uint8))
    # a black image: zero residuals between the filter bytes
    cases["zeros_3_chunks"] = (40, 700, np.zeros(40 * 2101, np.uint8))
    # runs of exactly these lengths, separated by distinct bytes that differ from the run value and from each other
    seq, sep = [8], 10                           # (8: between the row's filter byte and the first run)
    for n in RUNS:
        seq += [4] * n + [sep, sep + 1]
        sep += 2
    flat = (np.arange(3001) % 200 + 50).astype(np.uint8)
    flat[1:1 + len(seq)] = seq
    cases["exact_runs"] = (1, 1000, flat)
    # a run across the chunk boundary at 32768, in bytes without other runs
    flat = ((np.arange(20 * 2101) * 7) % 251 + 5).astype(np.uint8)
    flat[CHUNK - 68:CHUNK + 132] = 4
    cases["run_across_chunks"] = (20, 700, flat)
    # no run at all
    flat = np.full(8 * 901, 10, np.uint8)                     # (few values, so that the chunk is a dynamic block, no two neighbours equal)
    flat[1::2] = (np.arange(8 * 901 // 2) * 5) % 7 + 20
    cases["no_run"] = (8, 300, flat)
    # a geometric literal histogram: counts 1, 1, 2, 4, ..., 2^14 over exactly one chunk, the commonest value (4, the filter byte) on the
    # even positions, so that no two neighbours are equal; an unconstrained Huffman tree over these counts is deeper than 15
    h, w = 2, 5461
    assert h * (1 + 3 * w) == CHUNK
    flat = np.empty(CHUNK, np.uint8)
    flat[0::2] = 4
    odd = np.concatenate([np.full(c, 100 + i, np.uint8) for i, c in enumerate([1, 1] + [2 ** k for k in range(1, 14)])])
    assert len(odd) == CHUNK // 2
    flat[1::2] = rng.permutation(odd)
    cases["geometric"] = (h, w, flat)
    return cases


def smooth_frame(seed, h=256, w=512, sigma=8.0):
    """uniform noise blurred with a separable Gaussian, rescaled to 0..255, the top quarter the banner colour"""
    x = np.random.default_rng(seed).random((h, w, 3))

    def blur_matrix(n):
        d = np.arange(n)[:, None] - np.arange(n)[None, :]
        k = np.exp(-0.5 * (d / sigma) ** 2)
        return k / k.sum(axis=1, keepdims=True)

    x = np.einsum("ij,jwc->iwc", blur_matrix(h), x)
    x = np.einsum("ij,hjc->hic", blur_matrix(w), x)
    x = np.round((x - x.min()) / (x.max() - x.min()) * 255.0).astype(np.uint8)
    x[:h // 4] = (159, 157, 156)
    return x


class Bits:
    def __init__(self, data, pos=0):
        self.d, self.p = data, pos * 8

    def get(self, n):
        v = 0
        for i in range(n):
            v |= ((self.d[self.p >> 3] >> (self.p & 7)) & 1) << i
            self.p += 1
        return v


def _decode_table(lens):
    code, table = 0, {}
    for ln in range(1, 16):
        for s, v in enumerate(lens):
            if v == ln:
                table[(ln, code)] = s
                code += 1
        code <<= 1
    return table


def decode_tokens(data, byte_pos=2):
    """the tokens of the dynamic block at ``byte_pos``: ("lit", value) / ("match", length, distance), up to the end-of-block symbol"""
    r = Bits(data, byte_pos)
    ll, dl = parse_dynamic_header(data, byte_pos, r)
    lt, dt = _decode_table(ll), _decode_table(dl)

    def sym(table):
        c, n = 0, 0
        while (n, c) not in table:
            c, n = (c << 1) | r.get(1), n + 1
            assert n <= 15
        return table[(n, c)]

    base = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    extra = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    out = []
    while True:
        s = sym(lt)
        if s < 256:
            out.append(("lit", s))
        elif s == 256:
            return out
        else:
            length = base[s - 257] + r.get(extra[s - 257])
            d = sym(dt)
            assert d == 0, "only distance 1 is ever coded"
            out.append(("match", length, 1))


def parse_dynamic_header(data, byte_pos=2, r=None):
    """(literal/length code lengths, distance code lengths) of the dynamic block that starts at ``byte_pos`` of ``data``"""
    r = r if r is not None else Bits(data, byte_pos)
    assert r.get(1) == 0 and r.get(2) == 2, "not a non-final dynamic block"
    hlit, hdist, hclen = r.get(5) + 257, r.get(5) + 1, r.get(4) + 4
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    cl = [0] * 19
    for i in range(hclen):
        cl[order[i]] = r.get(3)
    assert max(cl) <= 7 and sum(2.0 ** -v for v in cl if v) == 1.0
    code, table = 0, {}
    for ln in range(1, 8):
        for s in range(19):
            if cl[s] == ln:
                table[(ln, code)] = s
                code += 1
        code <<= 1
    lens = []
    while len(lens) < hlit + hdist:
        c, n = 0, 0
        while (n, c) not in table:
            c, n = (c << 1) | r.get(1), n + 1
            assert n <= 7
        s = table[(n, c)]
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + r.get(2))
        elif s == 17:
            lens += [0] * (3 + r.get(3))
        else:
            lens += [0] * (11 + r.get(7))
    assert len(lens) == hlit + hdist
    return lens[:hlit], lens[hlit:]


def check_stream(stream, img, rows=None):
    """the stream inflates (Adler-32 included) to the Paeth rows of img, which unfilter to img"""
    h, w = img.shape[:2]
    raw = zlib.decompress(stream)
    want = paeth_rows(img) if rows is None else rows
    assert raw == want.tobytes()
    assert np.array_equal(unfilter(np.frombuffer(raw, np.uint8), h, w), img)
    assert stream[:2] == b"\x78\x01" and stream[-9:-4] == b"\x01\x00\x00\xff\xff" and len(stream) <= bound(h, w)
