// fr_inflate_core.h — the deflate *decoder* shared by the GPU kernel (fr_inflate.hip) and its host
// build (tests/native/fri_host.cpp): one raw deflate stream (RFC 1951) whose decoded size is known in
// advance, from in[0, in_len) into out[0, out_len).  Stored, fixed and dynamic blocks in any sequence.
//
// Verdict.  INFL_OK means: the stream's final block ended, exactly out_len bytes were produced and the
// input was consumed to its last byte (the bit position rounded up to a byte equals in_len).  INFL_OK
// implies that zlib (inflate with windowBits -15) accepts the same bytes and produces the same output;
// the caller sends everything else to the host decoder, which owns the error behaviour.  Huffman code
// sets must be complete, except zlib's one exception: a distance set of a single code of length 1.
// Over-subscribed sets and every other incomplete set are rejected.
//
// Memory-safety contract, on host and device alike, for ANY input bytes:
//   * no read outside in[0, in_len): the stream is read through P::stage, which checks every byte it
//     loads; a read past the end yields zero bits, and the decoder stops with INFL_INPUT at the first
//     symbol that used one;
//   * no write outside out[0, out_len): a literal needs pos < out_len, a match or a stored block
//     len <= out_len - pos, checked before the first byte is written;
//   * no back-reference before out[0]: dist <= pos, checked before the copy;
//   * no table index that is not bounded by construction: code lengths are 4-bit fields, table
//     indices are masked peeks of at most the table's width, sorted-symbol indices are clamped;
//   * every loop iteration consumes at least one input bit, produces at least one output byte, or ends
//     with an error: a Huffman code has at least one bit, a block header three, and bits past the end
//     are counted as consumed, so the INFL_INPUT check bounds every loop by in_len.  No input spins.
//
// Execution model.  The decode state (bit buffer, positions, tables) is uniform over the lanes of one
// wave; P (the platform) says which lane writes shared state and spreads the parallel parts -- table
// fills, match copies, stored copies -- over the lanes.  The host platform runs the lanes as loops.
//   P::lane0()                 this lane writes the uniform shared state
//   P::for_lanes(n, f)         f(i) for i in [0, n), dealt to the lanes
//   P::sync()                  what the lanes wrote is visible to every lane
//   P::put(pos, byte)          one output byte
//   P::copy_match(pos, d, n)   out[pos + i] = out[pos + i - d], i in [0, n), in steps of 64
//   P::copy_in(pos, src, n)    out[pos + i] = src[i]
//   P::stage(in, len, at, &e)  a buffer of the stream's bytes [at, e), e >= at + 4, zeros from len on
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define FRI_HD __host__ __device__ inline
#else
#define FRI_HD inline
#endif

namespace fri {

enum : uint8_t {
    INFL_OK = 0,
    INFL_BTYPE = 1,    // block type 3
    INFL_STORED = 2,   // stored LEN != ~NLEN
    INFL_CODELEN = 3,  // bad code-length set: over-subscribed, incomplete, bad repeat, counts out of range, no end-of-block
    INFL_SYMBOL = 4,   // invalid literal/length or distance symbol
    INFL_DIST = 5,     // distance before the start of the output
    INFL_INPUT = 6,    // input exhausted
    INFL_OVERRUN = 7,  // output would overrun out_len
    INFL_SHORT = 8,    // output short of out_len, or input left over
};

constexpr uint32_t MAX_OUT = 65536;     // decoded bytes of one stream (a BGZF member's bound)
constexpr uint32_t MAX_IN = 1u << 28;   // compressed bytes of one stream (bit positions fit 32 bits)
constexpr uint32_t LBITS = 10, DBITS = 8, CBITS = 7;  // primary table widths: literal/length, distance, code length
constexpr uint32_t NLSYM = 288, NDSYM = 32, NCSYM = 19;
constexpr uint32_t NOSYM = 0xFFFFu;

// one code set: a primary table over the next `bits` input bits (entry = length << 9 | symbol, 0: the
// code is longer or absent) and the canonical form (symbols sorted by length, counts per length) that
// decodes what the primary table does not hold
struct Tables {
    uint16_t lt[1u << LBITS], dt[1u << DBITS], ct[1u << CBITS];
    uint16_t lcnt[16], dcnt[16], ccnt[16];
    uint16_t lsym[NLSYM], dsym[NDSYM], csym[NCSYM + 1];
    uint16_t next[16], offs[16];     // build: next canonical code / next sorted slot per length
    uint8_t ll[NLSYM + NDSYM];       // the block's literal/length then distance code lengths
    uint8_t cl[NCSYM + 1];           // the header's code-length code lengths
};

FRI_HD uint32_t bitrev(uint32_t v, uint32_t n) {  // the low n bits of v reversed (n <= 15)
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1 - i);
    return r;
}

// LSB-first bit reader over in[0, in_len).  ip counts the bytes taken into the buffer, bytes past the
// end (zeros) included, so consumed() keeps growing when the input is exhausted.  The stream is read
// through a window the platform stages (P::stage: bytes [at, end) of the stream, zeros past in_len; on the
// GPU 1 KiB in LDS, so the decode loop has no global load whose wait would also drain its stores); nxt is
// the word at ip, loaded one refill ahead.
struct BitR {
    const uint8_t* in;
    uint32_t in_len, ip, bc;
    uint64_t bb;
    uint32_t nxt;
    const uint8_t* win;    // the staged window: stream bytes [wbase, wend)
    uint32_t wbase, wend;
    template <class P>
    FRI_HD uint32_t load32(P& p) {
        if (ip < wbase || ip + 4 > wend) {
            win = p.stage(in, in_len, ip, &wend);
            wbase = ip;
        }
        uint32_t v;
        memcpy(&v, win + (ip - wbase), 4);
        return v;
    }
    template <class P>
    FRI_HD void refill(P& p) {  // at least 33 bits afterwards
        while (bc <= 32) {
            bb |= (uint64_t)nxt << bc;
            bc += 32;
            ip += 4;
            nxt = load32(p);
        }
    }
    template <class P>
    FRI_HD void seek(P& p, uint32_t byte) {  // restart at a byte position
        ip = byte;
        bb = 0;
        bc = 0;
        nxt = load32(p);
    }
    FRI_HD uint32_t peek(uint32_t n) const { return (uint32_t)bb & ((1u << n) - 1u); }
    FRI_HD void skip(uint32_t n) {
        bb >>= n;
        bc -= n;
    }
    FRI_HD uint32_t take(uint32_t n) {
        const uint32_t v = peek(n);
        skip(n);
        return v;
    }
    FRI_HD uint64_t consumed() const { return (uint64_t)ip * 8 - bc; }
    FRI_HD bool exhausted() const { return consumed() > (uint64_t)in_len * 8; }
};

// Build one code set from n code lengths (each <= 15).  0, or INFL_CODELEN for a set that is
// over-subscribed or incomplete (dist: a single code of length 1 is taken, as zlib takes it).
template <class P>
FRI_HD uint8_t build(P& p, Tables& T, const uint8_t* lens, uint32_t n, uint32_t bits, uint16_t* tab, uint16_t* cnt,
                     uint16_t* sym, uint32_t sym_cap, bool dist) {
    if (p.lane0()) {
        for (uint32_t l = 0; l < 16; ++l) cnt[l] = 0;
        for (uint32_t s = 0; s < n; ++s) cnt[lens[s] & 15u]++;
    }
    p.for_lanes(1u << bits, [&](uint32_t i) { tab[i] = 0; });
    p.sync();
    int32_t left = 1;
    for (uint32_t l = 1; l < 16; ++l) {
        left = left * 2 - (int32_t)cnt[l];
        if (left < 0) return INFL_CODELEN;
    }
    if (left > 0 && !(dist && n - cnt[0] == 1 && cnt[1] == 1)) return INFL_CODELEN;
    if (p.lane0()) {
        uint32_t code = 0, off = 0;
        for (uint32_t l = 1; l < 16; ++l) {
            T.next[l] = (uint16_t)code;
            T.offs[l] = (uint16_t)off;
            code = (code + cnt[l]) << 1;
            off += cnt[l];
        }
    }
    p.sync();
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = lens[s] & 15u;
        if (!l) continue;
        const uint32_t c = T.next[l], o = T.offs[l];
        if (p.lane0()) {
            T.next[l] = (uint16_t)(c + 1);
            T.offs[l] = (uint16_t)(o + 1);
            sym[o < sym_cap ? o : sym_cap - 1] = (uint16_t)s;
        }
        if (l <= bits) {
            const uint32_t r = bitrev(c, l) & ((1u << l) - 1u);
            const uint16_t e = (uint16_t)(l << 9 | s);
            p.for_lanes(1u << (bits - l), [&](uint32_t k) { tab[r | k << l] = e; });
        }
        p.sync();
    }
    return INFL_OK;
}

// the next symbol of a code set (at least 15 bits in the buffer), NOSYM when no code matches
FRI_HD uint32_t decode_sym(BitR& br, const uint16_t* tab, uint32_t bits, const uint16_t* cnt, const uint16_t* sym,
                           uint32_t sym_cap) {
    const uint32_t e = tab[br.peek(bits)];
    if (e) {
        br.skip(e >> 9);
        return e & 511u;
    }
    int32_t code = 0, first = 0, index = 0;  // canonical walk, one bit per length
    uint32_t v = br.peek(15);
    for (uint32_t l = 1; l < 16; ++l) {
        code |= (int32_t)(v & 1u);
        v >>= 1;
        const int32_t count = cnt[l];
        if (code - count < first) {
            const uint32_t k = (uint32_t)(index + (code - first));
            br.skip(l);
            return sym[k < sym_cap ? k : sym_cap - 1];
        }
        index += count;
        first = (first + count) << 1;
        code <<= 1;
    }
    return NOSYM;  // nothing consumed: every caller ends with an error
}

template <class P>
FRI_HD uint8_t read_dynamic(P& p, Tables& T, BitR& br) {
    br.refill(p);
    const uint32_t hlit = br.take(5) + 257, hdist = br.take(5) + 1, hclen = br.take(4) + 4;
    if (hlit > 286 || hdist > 30) return INFL_CODELEN;
    p.for_lanes(NCSYM + 1, [&](uint32_t i) { T.cl[i] = 0; });
    p.sync();
    for (uint32_t i = 0; i < hclen; ++i) {
        br.refill(p);
        const uint32_t v = br.take(3);
        const uint32_t at = (uint8_t)"\x10\x11\x12\x00\x08\x07\x09\x06\x0a\x05\x0b\x04\x0c\x03\x0d\x02\x0e\x01\x0f"[i];
        if (p.lane0()) T.cl[at] = (uint8_t)v;
    }
    p.sync();
    if (br.exhausted()) return INFL_INPUT;
    if (build(p, T, T.cl, NCSYM, CBITS, T.ct, T.ccnt, T.csym, NCSYM, false)) return INFL_CODELEN;
    const uint32_t total = hlit + hdist;
    for (uint32_t n = 0; n < total;) {
        br.refill(p);
        const uint32_t s = decode_sym(br, T.ct, CBITS, T.ccnt, T.csym, NCSYM);
        if (s == NOSYM) return br.exhausted() ? INFL_INPUT : INFL_CODELEN;
        uint32_t rep = 1, val = s;
        if (s >= 16) {
            val = 0;
            if (s == 16) {
                if (n == 0) return INFL_CODELEN;
                val = T.ll[n - 1];
                rep = 3 + br.take(2);
            } else if (s == 17) {
                rep = 3 + br.take(3);
            } else {
                rep = 11 + br.take(7);
            }
        }
        if (br.exhausted()) return INFL_INPUT;
        if (rep > total - n) return INFL_CODELEN;
        p.for_lanes(rep, [&](uint32_t k) { T.ll[n + k] = (uint8_t)(val & 15u); });
        p.sync();
        n += rep;
    }
    if (T.ll[256] == 0) return INFL_CODELEN;  // no end-of-block code
    if (build(p, T, T.ll, hlit, LBITS, T.lt, T.lcnt, T.lsym, NLSYM, false)) return INFL_CODELEN;
    if (build(p, T, T.ll + hlit, hdist, DBITS, T.dt, T.dcnt, T.dsym, NDSYM, true)) return INFL_CODELEN;
    return INFL_OK;
}

template <class P>
FRI_HD void build_fixed(P& p, Tables& T) {
    p.for_lanes(NLSYM + NDSYM,
                [&](uint32_t i) { T.ll[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5); });
    p.sync();
    (void)build(p, T, T.ll, NLSYM, LBITS, T.lt, T.lcnt, T.lsym, NLSYM, false);
    (void)build(p, T, T.ll + NLSYM, NDSYM, DBITS, T.dt, T.dcnt, T.dsym, NDSYM, true);
}

// One stream.  *produced: the bytes written to the output (out_len exactly when the status is INFL_OK).
template <class P>
FRI_HD uint8_t inflate_stream(P& p, Tables& T, const uint8_t* in, uint32_t in_len, uint32_t out_len, uint32_t* produced) {
    BitR br{in, in_len, 0, 0, 0, 0, in, 0, 0};
    br.seek(p, 0);
    uint32_t pos = 0;
    bool fixed_now = false;  // T holds the fixed code set
    *produced = 0;
    if (in_len > MAX_IN || out_len > MAX_OUT) return INFL_OVERRUN;
    for (;;) {
        br.refill(p);
        const uint32_t last = br.take(1), type = br.take(2);
        if (br.exhausted()) return INFL_INPUT;
        if (type == 3) return INFL_BTYPE;
        if (type == 0) {
            br.skip(br.bc & 7u);  // to the byte boundary (ip * 8 is one, so the buffer's bit count tells)
            br.refill(p);
            const uint32_t len = br.take(16), nlen = br.take(16);
            if (br.exhausted()) return INFL_INPUT;
            if (len != (~nlen & 0xFFFFu)) return INFL_STORED;
            const uint32_t src = (uint32_t)(br.consumed() >> 3);  // <= in_len: not exhausted
            if (len > in_len - src) return INFL_INPUT;
            if (len > out_len - pos) return INFL_OVERRUN;
            p.copy_in(pos, in + src, len);
            pos += len;
            *produced = pos;
            br.seek(p, src + len);
        } else {
            if (type == 1) {
                if (!fixed_now) build_fixed(p, T);
                fixed_now = true;
            } else {
                fixed_now = false;
                const uint8_t st = read_dynamic(p, T, br);
                if (st) return st;
            }
            for (;;) {
                br.refill(p);
                const uint32_t s = decode_sym(br, T.lt, LBITS, T.lcnt, T.lsym, NLSYM);
                if (br.exhausted()) return INFL_INPUT;
                if (s < 256) {
                    if (pos >= out_len) return INFL_OVERRUN;
                    p.put(pos, (uint8_t)s);
                    *produced = ++pos;
                    continue;
                }
                if (s == 256) break;
                if (s > 285) return INFL_SYMBOL;  // 286, 287 and NOSYM
                const uint32_t li = s - 257;
                const uint32_t leb = (li < 8 || li == 28) ? 0 : (li - 4) >> 2;
                const uint32_t len = (li < 8 ? 3 + li : li == 28 ? 258 : 3 + ((4 + (li & 3)) << leb)) + br.take(leb);
                br.refill(p);
                const uint32_t ds = decode_sym(br, T.dt, DBITS, T.dcnt, T.dsym, NDSYM);
                if (ds > 29) return br.exhausted() ? INFL_INPUT : INFL_SYMBOL;  // 30, 31 and NOSYM
                const uint32_t deb = ds < 4 ? 0 : (ds >> 1) - 1;
                const uint32_t dist = (ds < 4 ? 1 + ds : 1 + ((2 + (ds & 1)) << deb)) + br.take(deb);
                if (br.exhausted()) return INFL_INPUT;
                if (dist > pos) return INFL_DIST;
                if (len > out_len - pos) return INFL_OVERRUN;
                p.copy_match(pos, dist, len);
                pos += len;
                *produced = pos;
            }
        }
        if (last) break;
    }
    if (pos != out_len) return INFL_SHORT;
    if ((br.consumed() + 7) / 8 != in_len) return INFL_SHORT;  // input left over
    return INFL_OK;
}

// ---- the host platform: the lanes as loops ----------------------------------------------------
struct HostP {
    uint8_t* out;
    uint8_t stg[64];
    const uint8_t* stage(const uint8_t* in, uint32_t in_len, uint32_t at, uint32_t* end) {
        for (uint32_t k = 0; k < sizeof stg; ++k) stg[k] = at + k < in_len ? in[at + k] : 0;
        *end = at + (uint32_t)sizeof stg;
        return stg;
    }
    bool lane0() const { return true; }
    template <class F>
    void for_lanes(uint32_t n, F f) const {
        for (uint32_t i = 0; i < n; ++i) f(i);
    }
    void sync() const {}
    void put(uint32_t pos, uint8_t b) const { out[pos] = b; }
    void copy_match(uint32_t pos, uint32_t d, uint32_t n) const {
        for (uint32_t base = 0; base < n; base += 64)  // one 64-lane step: lane i reads before any lane writes
            for (uint32_t i = 0; i < 64 && base + i < n; ++i) out[pos + base + i] = out[pos + base - d + i % d];
    }
    void copy_in(uint32_t pos, const uint8_t* src, uint32_t n) const {
        if (n) memcpy(out + pos, src, n);
    }
};

}  // namespace fri
