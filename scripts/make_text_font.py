#!/usr/bin/env python3
"""The stroke font of csrc/text_draw.hpp, as a construction: every glyph is straight strokes between grid points chosen here and arcs of
ellipses SAMPLED BY FORMULA (centre, radii, angles, number of chords; each point rounded to the unit grid), so the table has a source one
can read and change.  Nothing is taken from another font's tables; only the metrics the result images' layout was made for are kept
(cap height 21, x-height 14, descenders to -7, advance <= 24, at most 32 segments per glyph).

    python scripts/make_text_font.py            prints the table block of text_draw.hpp (between its BEGIN / END markers)
    python scripts/make_text_font.py --check    compares it with the header (tests/test_text_cpu.py does the same)
"""
import math
import os
import sys

CAP, XH, DESC = 21, 14, -7


def rnd(v):
    return int(math.floor(v + 0.5))


def arc(cx, cy, rx, ry, a0, a1, n):
    """n chords of the ellipse from angle a0 to a1 (degrees, counter-clockwise from +x; a1 < a0 runs clockwise), rounded to the grid"""
    pts = []
    for i in range(n + 1):
        a = math.radians(a0 + (a1 - a0) * i / n)
        p = (rnd(cx + rx * math.cos(a)), rnd(cy + ry * math.sin(a)))
        if not pts or pts[-1] != p:
            pts.append(p)
    return pts


def ring(cx, cy, rx, ry, n, start=90):
    return arc(cx, cy, rx, ry, start, start - 360, n)


def square(x, y):
    return [(x, y), (x + 2, y), (x + 2, y + 2), (x, y + 2), (x, y)]


def rot(pts, cx2, cy2):
    """half a turn about (cx2 / 2, cy2 / 2)"""
    return [(cx2 - x, cy2 - y) for x, y in pts]


# ---- shared pieces
CAP_STEM = [(3, 0), (3, CAP)]
BOWL = ring(8, 7, 5, 7, 12, start=0)                       # the lower-case bowl, x 3..13, touching a stem at either side
SHOULDER = [(3, 9)] + arc(8, 9, 5, 5, 180, 0, 6) + [(13, 0)]
SIX = ring(9, 6.5, 6, 6.5, 12, start=180) + arc(11, 8, 8, 13, 180, 70, 5)
COMMA = [square(3, 0), [(5, 0), (4, -3), (3, -4)]]
PAREN = arc(12, 7, 8, 16.17, 120, 240, 6)

G = {
    " ": (12, []),
    "0": (18, [ring(9, 10.5, 6, 10.5, 16)]),
    "1": (18, [[(5, 16), (9, CAP), (9, 0)]]),
    "2": (18, [arc(9, 15, 6, 6, 160, -45, 7) + [(3, 0), (15, 0)]]),
    "3": (18, [arc(9, 16, 5, 5, 150, -90, 6) + arc(9, 5.5, 6, 5.5, 90, -150, 7)]),
    "4": (18, [[(12, 0), (12, CAP), (2, 6), (16, 6)]]),
    "5": (18, [[(14, CAP), (5, CAP), (4, 12)] + arc(9, 6.5, 6, 6.5, 140, -150, 8)]),
    "6": (18, [SIX]),
    "7": (18, [[(3, CAP), (15, CAP), (7, 0)]]),
    "8": (18, [ring(9, 16, 5, 5, 12), ring(9, 5.5, 6, 5.5, 12)]),
    "9": (18, [rot(SIX, 18, CAP)]),
    "A": (18, [[(2, 0), (9, CAP), (16, 0)], [(4, 6), (14, 6)]]),
    "B": (19, [CAP_STEM, [(3, CAP)] + arc(9, 16, 5, 5, 90, -90, 6) + [(3, 11)], arc(10, 5.5, 6, 5.5, 90, -90, 6) + [(3, 0)]]),
    "C": (20, [arc(10.5, 10.5, 7.5, 10.5, 50, 310, 12)]),
    "D": (20, [CAP_STEM, [(3, CAP)] + arc(8, 10.5, 9, 10.5, 90, -90, 10) + [(3, 0)]]),
    "E": (17, [CAP_STEM, [(3, CAP), (14, CAP)], [(3, 11), (12, 11)], [(3, 0), (14, 0)]]),
    "F": (16, [CAP_STEM, [(3, CAP), (14, CAP)], [(3, 11), (11, 11)]]),
    "G": (21, [arc(10.5, 10.5, 7.5, 10.5, 50, 360, 14) + [(12, 11)]]),
    "H": (20, [CAP_STEM, [(17, 0), (17, CAP)], [(3, 11), (17, 11)]]),
    "I": (6, [CAP_STEM]),
    "J": (14, [[(10, CAP)] + arc(6, 6, 4, 6, 0, -180, 6)]),
    "K": (18, [CAP_STEM, [(16, CAP), (3, 8)], [(7, 12), (16, 0)]]),
    "L": (15, [[(3, CAP), (3, 0), (13, 0)]]),
    "M": (22, [[(3, 0), (3, CAP), (11, 4), (19, CAP), (19, 0)]]),
    "N": (20, [[(3, 0), (3, CAP), (17, 0), (17, CAP)]]),
    "O": (21, [ring(10.5, 10.5, 7.5, 10.5, 16)]),
    "P": (18, [CAP_STEM, [(3, CAP)] + arc(9, 15.5, 6, 5.5, 90, -90, 6) + [(3, 10)]]),
    "Q": (21, [ring(10.5, 10.5, 7.5, 10.5, 16), [(12, 5), (19, -2)]]),
    "R": (18, [CAP_STEM, [(3, CAP)] + arc(9, 15.5, 6, 5.5, 90, -90, 6) + [(3, 10)], [(9, 10), (16, 0)]]),
    "S": (18, [arc(9, 15.5, 6, 5.5, 30, 270, 7) + arc(9, 5, 6.5, 5, 90, -150, 7)]),
    "T": (16, [[(8, 0), (8, CAP)], [(1, CAP), (15, CAP)]]),
    "U": (20, [[(3, CAP)] + arc(10, 7, 7, 7, 180, 360, 8) + [(17, CAP)]]),
    "V": (18, [[(2, CAP), (9, 0), (16, CAP)]]),
    "W": (24, [[(2, CAP), (7, 0), (12, 17), (17, 0), (22, CAP)]]),
    "X": (18, [[(3, CAP), (15, 0)], [(15, CAP), (3, 0)]]),
    "Y": (18, [[(2, CAP), (9, 10), (9, 0)], [(16, CAP), (9, 10)]]),
    "Z": (18, [[(3, CAP), (15, CAP), (3, 0), (15, 0)]]),
    "a": (16, [[(13, XH), (13, 0)], BOWL]),
    "b": (16, [[(3, CAP), (3, 0)], BOWL]),
    "c": (15, [arc(8, 7, 5, 7, 45, 315, 9)]),
    "d": (16, [[(13, CAP), (13, 0)], BOWL]),
    "e": (16, [[(3, 7)] + arc(8, 7, 5, 7, 0, 320, 11)]),
    "f": (10, [arc(8, 17, 4, 4, 80, 180, 3) + [(4, 0)], [(1, XH), (8, XH)]]),
    "g": (16, [[(13, XH)] + arc(8, -2, 5, 5, 0, -150, 5), BOWL]),
    "h": (16, [[(3, CAP), (3, 0)], SHOULDER]),
    "i": (6, [[(3, 20), (3, CAP)], [(3, XH), (3, 0)]]),
    "j": (8, [[(5, 20), (5, CAP)], [(5, XH)] + arc(2, -3, 3, 4, 0, -90, 3)]),
    "k": (15, [[(3, CAP), (3, 0)], [(12, XH), (3, 5)], [(6, 8), (13, 0)]]),
    "l": (8, [[(3, CAP)] + arc(6, 3, 3, 3, 180, 270, 3)]),
    "m": (22, [[(3, XH), (3, 0)], [(3, 10)] + arc(7, 10, 4, 4, 180, 0, 5) + [(11, 0)], [(11, 10)] + arc(15, 10, 4, 4, 180, 0, 5) + [(19, 0)]]),
    "n": (16, [[(3, XH), (3, 0)], SHOULDER]),
    "o": (16, [ring(8, 7, 5, 7, 14)]),
    "p": (16, [[(3, XH), (3, DESC)], BOWL]),
    "q": (16, [[(13, XH), (13, DESC)], BOWL]),
    "r": (11, [[(3, XH), (3, 0)], [(3, 9)] + arc(8, 9, 5, 5, 180, 60, 4)]),
    "s": (14, [arc(7, 10.5, 4, 3.5, 30, 270, 6) + arc(7, 3.5, 4, 3.5, 90, -150, 6)]),
    "t": (10, [[(4, 20)] + arc(7, 3, 3, 3, 180, 270, 3), [(1, XH), (8, XH)]]),
    "u": (16, [[(3, XH)] + arc(8, 5, 5, 5, 180, 360, 6), [(13, XH), (13, 0)]]),
    "v": (14, [[(2, XH), (7, 0), (12, XH)]]),
    "w": (20, [[(2, XH), (6, 0), (10, 12), (14, 0), (18, XH)]]),
    "x": (14, [[(2, XH), (12, 0)], [(12, XH), (2, 0)]]),
    "y": (14, [[(2, XH), (7, 0)], [(12, XH), (7, 0), (5, -5), (3, DESC), (2, DESC)]]),
    "z": (14, [[(2, XH), (12, XH), (2, 0), (12, 0)]]),
    ".": (8, [square(3, 0)]),
    ",": (8, COMMA),
    ":": (8, [square(3, 0), square(3, 10)]),
    ";": (8, COMMA + [square(3, 10)]),
    "'": (6, [[(4, CAP), (3, 15)]]),
    "-": (14, [[(2, 8), (12, 8)]]),
    "+": (18, [[(9, 15), (9, 1)], [(2, 8), (16, 8)]]),
    "/": (14, [[(12, CAP), (2, -4)]]),
    "(": (10, [PAREN]),
    ")": (10, [[(10 - x, y) for x, y in PAREN]]),
    "%": (22, [[(18, CAP), (4, 0)], ring(6, 16, 4, 5, 8), ring(16, 5, 4, 5, 8)]),
    "=": (18, [[(2, 11), (16, 11)], [(2, 5), (16, 5)]]),
}
BOX = (14, [[(2, 0), (12, 0), (12, CAP), (2, CAP), (2, 0)]])


def segs(polys):
    out = []
    for p in polys:
        for a, b in zip(p[:-1], p[1:]):
            out.append((a[0], a[1], b[0], b[1]))
    return out


def table() -> str:
    order = [("\0", BOX)] + sorted(G.items())
    seen = {}
    allseg, glyphs, index = [], [], [0] * 128
    for gi, (ch, (adv, polys)) in enumerate(order):
        s = segs(polys)
        assert len(s) <= 32 and adv <= 24, (ch, len(s))
        for x0, y0, x1, y1 in s:
            assert 0 <= x0 <= adv and 0 <= x1 <= adv and DESC <= y0 <= CAP and DESC <= y1 <= CAP, (ch, x0, y0, x1, y1)
        key = tuple(sorted(min((a, b, c, d), (c, d, a, b)) for a, b, c, d in s))
        assert not s or key not in seen, (ch, seen.get(key))
        seen[key] = ch
        glyphs.append((len(allseg), len(s), adv, ch))
        allseg += s
        if gi:
            index[ord(ch)] = gi
    out = ["constexpr int kSegCount = %d, kGlyphCount = %d;" % (len(allseg), len(glyphs)), "constexpr int8_t kSeg[kSegCount][4] = {"]
    for first, n, adv, ch in glyphs:
        out.append("    // %s" % ("the box of every other byte" if ch == "\0" else ("space" if ch == " " else ch)))
        row = allseg[first:first + n]
        for i in range(0, len(row), 8):
            out.append("    " + " ".join("{%d, %d, %d, %d}," % s for s in row[i:i + 8]))
    out.append("};")
    out.append("constexpr Glyph kGlyph[kGlyphCount] = {")
    for i in range(0, len(glyphs), 8):
        out.append("    " + " ".join("{%d, %d, %d}," % g[:3] for g in glyphs[i:i + 8]))
    out.append("};")
    out.append("constexpr uint8_t kIndex[128] = {")
    for i in range(0, 128, 16):
        out.append("    " + " ".join("%d," % v for v in index[i:i + 16]))
    out.append("};")
    return "\n".join(out) + "\n"


BEGIN, END = "// BEGIN font table (scripts/make_text_font.py)\n", "// END font table\n"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "semantic_depth_amd", "csrc", "text_draw.hpp")


def header_table() -> str:
    txt = open(HEADER).read()
    return txt[txt.index(BEGIN) + len(BEGIN):txt.index(END)]


if __name__ == "__main__":
    if "--check" in sys.argv:
        sys.exit(0 if header_table() == table() else "text_draw.hpp's font table is not what scripts/make_text_font.py prints")
    sys.stdout.write(table())
