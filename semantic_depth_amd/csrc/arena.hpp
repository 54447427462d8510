// The one walker every scratch layout is written with (DESIGN.md "where scratch layouts live").  No HIP: a plain host compiler builds
// this header and every *_layout() that uses it (scripts/check_layouts.cpp does).
//
// A layout function walks its buffer front to back once and returns the named offsets plus `total`; the size query returns .total and
// the launcher forms every pointer as workspace + l.name, so a region cannot be carved without being counted.
#pragma once
#include <cstddef>

namespace sdarena {

constexpr size_t round_up(size_t v, size_t align) { return (v + align - 1) / align * align; }

struct Walker {
    size_t off = 0;      // bytes walked so far
    size_t pad = 0;      // of them, bytes skipped to reach an alignment
    // the next region: `bytes` at a multiple of `align` (relative to the buffer, whose base is aligned at least as much); returns its offset
    size_t take(size_t bytes, size_t align) {
        const size_t at = round_up(off, align);
        pad += at - off;
        off = at + bytes;
        return at;
    }
    // the walk's end rounded up to `align`: a layout's total, or the offset of a part that begins aligned
    size_t end(size_t align = 1) { return take(0, align); }
    // a total that history fixed as (sum of the unpadded region sizes) + slack: the slack is the last region, at end(), and what the
    // walk spent on padding comes out of it (scripts/check_layouts.cpp holds pad <= slack over every legal argument)
    size_t end_with_slack(size_t slack) const { return off - pad + slack; }
};

}  // namespace sdarena
