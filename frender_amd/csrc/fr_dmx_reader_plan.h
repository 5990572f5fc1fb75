// fr_dmx_reader_plan.h — the arithmetic of `demux --gz-reader gpu` (fr_dmx_reader.hip) that needs no device:
// how far a staged piece of a BGZF file reaches in whole members, which of its members the next batch decodes
// and where, and what a window keeps of the one before it.  Plain C++ (no HIP, no allocation): the reader
// includes it, and so does the stand-alone host program of the tests (tests/native/frp_host.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace fr {
namespace rdr {

constexpr uint64_t MEMBER_MAX = 65536;  // the format's bound on a member's size and on its decoded size
constexpr uint64_t SLACK = 16;          // addressable bytes past a window's end (the loader's 16-byte loads)

inline uint32_t rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

// The whole members at the front of data[0, n), a piece of a file that starts at a member's first byte:
// returns their bytes.  A header is the one fr_bgzf_probe accepts (FLG == FEXTRA alone, XLEN 6, the BC
// subfield alone, 26 <= BSIZE + 1).  at_eof: the piece ends with the file.  *bad: the bytes at the returned
// offset are not such a header, or the file ends inside a member (NUL padding included: the host reader's
// to judge).  A member the piece cuts is left for the next piece (not bad).
inline size_t whole_members(const uint8_t* data, size_t n, bool at_eof, bool* bad, size_t* count = nullptr) {
    size_t pos = 0, k = 0;
    *bad = false;
    while (pos < n) {
        const uint8_t* h = data + pos;
        if (n - pos < 18) {
            *bad = at_eof;
            break;
        }
        if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || h[3] != 4 || rd16(h + 10) != 6 || h[12] != 'B' ||
            h[13] != 'C' || rd16(h + 14) != 2) {
            *bad = true;
            break;
        }
        const size_t bsize = (size_t)rd16(h + 16) + 1;
        if (bsize < 26) {
            *bad = true;
            break;
        }
        if (n - pos < bsize) {
            *bad = at_eof;
            break;
        }
        pos += bsize;
        ++k;
    }
    if (count) *count = k;
    return pos;
}

// What a window keeps of the previous one: bytes [keep_from, len) move to its front.
inline uint64_t carry_len(uint64_t len, uint64_t keep_from) { return keep_from < len ? len - keep_from : 0; }

// Bytes a window's buffer must hold before a fill to `want` bytes behind a carry: members are taken while the
// window is below `want`, so it ends below max(carry, want) + one member; the slack follows.
inline uint64_t window_capacity(uint64_t carry, uint64_t want) {
    return (carry > want ? carry : want) + MEMBER_MAX + SLACK;
}

// The next batch: members ms[first, n) are taken in order while the window, `have` bytes so far, is below
// `want` (the host loop's `while size < window`).  Member first + j decodes in[in_off[2j], in_off[2j + 1])
// to window[out_off[j], out_off[j + 1]); out_off[count] is the window's new size.  in_off holds 2 x and
// out_off 1 + the members offered.  M has in_off, in_len, isize (fr::BgzfMember).  Returns count.
template <class M>
inline size_t plan_batch(const M* ms, size_t n, size_t first, uint64_t have, uint64_t want, uint64_t* in_off,
                         uint64_t* out_off) {
    size_t j = 0;
    out_off[0] = have;
    while (first + j < n && have < want) {
        const M& m = ms[first + j];
        in_off[2 * j] = m.in_off;
        in_off[2 * j + 1] = m.in_off + m.in_len;
        have += m.isize;
        out_off[++j] = have;
    }
    return j;
}

}  // namespace rdr
}  // namespace fr
