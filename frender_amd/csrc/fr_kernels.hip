// fr_kernels.hip — the tally (chunk_kernel), the gfx950 kernel of frender's scan hot path: frender.py:154-181
// scan_file + :199-205 merge, one pass over the decoded FASTQ bytes in HBM (R1-R4 of SURVEY.md §8.0).
// (The other table kernels, the launch log's aggregation and synth are fr_table.hip; the two files share
// fr_table_dev.h.  The Hamming classifier is fr_classify.hip.)
//
// Design notes: the tally is HBM-bound byte work.  A workgroup takes a chunk of
// 4-KiB wave-tiles by ticket and each of its four waves walks a quarter of it without workgroup
// barriers: lanes classify their 64-B segments in registers (line-end / ' ' / ':' bitmaps by v_perm
// lookups and dot4 gathers), find every 4th line from the wave's line count, parse each header
// lane-owned from the bitmaps and the wave's LDS copy of the tile, pack the code 3 bits/char and
// count it in an LDS open-addressing table shared by the workgroup; each chunk's table is
// committed to the HBM table (or to the launch log) once.  Line phases are guessed per wave and
// verified per chunk and per launch (decoupled look-back over 8-B {tag, value} granules).
#include "../../include/frender_amd.h"
#include "fr_internal.h"
#include "fr_table_dev.h"

namespace fr {

#if defined(FR_STAMPS) && FR_STAMPS == 1  // diagnostic builds only: per-wave shader cycles of the chunk loop's phases (DevState::stamp)
#define FR_STAMP_DECL u64 st_[8] = {0, 0, 0, 0, 0, 0, 0, 0}; u64 tq_ = __builtin_amdgcn_s_memtime();
#define FR_STAMP(i) do { const u64 n_ = __builtin_amdgcn_s_memtime(); st_[i] += n_ - tq_; tq_ = n_; } while (0)
#define FR_STAMP_FLUSH(k0) do { st_[6] = __builtin_amdgcn_s_memtime() - (k0); \
    if ((threadIdx.x & 63) == 0) for (int i_ = 0; i_ < 8; ++i_) atomicAdd((unsigned long long*)&a.st->stamp[i_], \
        (unsigned long long)st_[i_]); } while (0)
#else
#define FR_STAMP_DECL
#define FR_STAMP(i) do { } while (0)
#define FR_STAMP_FLUSH(k0) do { } while (0)
#endif

#if defined(FR_STAMPS) && FR_STAMPS == 2  // diagnostic builds only: the commit's phases instead
#define FR_CSTAMP(i) do { const u64 n_ = __builtin_amdgcn_s_memtime(); cst_[i] += n_ - cq_; cq_ = n_; } while (0)
#else
#define FR_CSTAMP(i) do { } while (0)
#endif

#if defined(FR_STAMPS) && FR_STAMPS == 4  // diagnostic builds only: where a wave's walk time goes (walk_wave's
// steps, DevState::stamp: 0 the next tile's VMEM wait, 1 LDS copy + classify, 2 rare drain + bitmaps, 3 header
// parse, 4 walk steps counted, 5 whole-kernel wave cycles, 6 walk calls)
#define FR_WSTAMP_DECL u64 wst_[4] = {0, 0, 0, 0}; u64 wq_ = __builtin_amdgcn_s_memtime();
#define FR_WSTAMP(i) do { const u64 n_ = __builtin_amdgcn_s_memtime(); wst_[i] += n_ - wq_; wq_ = n_; } while (0)
#define FR_WSTAMP_RESET() do { wq_ = __builtin_amdgcn_s_memtime(); } while (0)
#define FR_WSTAMP_FLUSH(steps) do { if ((threadIdx.x & 63) == 0) { \
    for (int i_ = 0; i_ < 4; ++i_) atomicAdd((unsigned long long*)&a.st->stamp[i_], (unsigned long long)wst_[i_]); \
    atomicAdd((unsigned long long*)&a.st->stamp[4], (unsigned long long)(steps)); \
    atomicAdd((unsigned long long*)&a.st->stamp[6], 1ull); } } while (0)
#else
#define FR_WSTAMP_DECL
#define FR_WSTAMP(i) do { } while (0)
#define FR_WSTAMP_RESET() do { } while (0)
#define FR_WSTAMP_FLUSH(steps) do { } while (0)
#endif

#ifdef FR_DEBUG_PRINT  // diagnostic builds only: trace the tally kernel's chunk loop (workgroup 0, lane 0 of each wave)
#define FR_TRACE(...) do { if (blockIdx.x == 0 && (threadIdx.x & 63) == 0) printf(__VA_ARGS__); } while (0)
#else
#define FR_TRACE(...) do { } while (0)
#endif

#define FR_COLD __forceinline__  // rare paths stay inline (out of line, the calls made the hot loop spill)

// ------------------------------------------------------------------------------------
// small helpers
// ------------------------------------------------------------------------------------

// exact per-byte equality of w against the byte replicated in c -> 4-bit mask (byte i -> bit i)
__device__ __forceinline__ u32 eq4(u32 w, u32 c) {
    const u32 t = w ^ c;
    const u32 z = ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) & 0x80808080u;
    return (((z >> 7) * 0x00204081u) >> 21) & 0xFu;
}

__device__ __forceinline__ u32 hi4(u32 w) {  // bytes >= 0x80
    return ((((w & 0x80808080u) >> 7) * 0x00204081u) >> 21) & 0xFu;
}

// byte -> fast-key symbol (A1 C2 G3 T4 N5 +6), 0 if outside the fast alphabet
__device__ __forceinline__ u32 sym_of(u32 c) {
    const u32 i = (c >> 1) & 7u;
    const u64 expect = 0x4E002B0047544341ull;  // idx: 0 A,1 C,2 T,3 G,4 -,5 +,6 -,7 N
    const u32 symtab = 0x50603421u;
    const bool ok = ((expect >> (8 * i)) & 0xFFu) == c;
    return ok ? ((symtab >> (4 * i)) & 0xFu) : 0u;
}

// Fused byte classifier, 4 bytes per call: per byte, bit0 line end ('\n' or '\r'), bit1 '\r',
// bit2 ' ', bit3 ':', bit4 byte >= 0x80.  Three 8-entry lookups through v_perm_b32, ANDed: on bits
// [2:0], on bits [5:3], and on bits [7:6].  '\n' = 00 001 010, '\r' = 00 001 101, ' ' = 00 100 000,
// ':' = 00 111 010: each class is the one byte whose two table entries both carry its bit; bit 4 is
// in every entry of the first two tables and in the third only for bits [7:6] = 1x (checked for
// all 256 bytes).
__device__ __forceinline__ u32 classify4(u32 w) {
    const u32 lo3 = __builtin_amdgcn_perm(0x10101310u, 0x10191014u, w & 0x07070707u);
    const u32 mid3 = __builtin_amdgcn_perm(0x18101014u, 0x10101310u, (w >> 3) & 0x07070707u);
    const u32 top2 = __builtin_amdgcn_perm(0u, 0x1010000Fu, (w >> 6) & 0x03030303u);
    return lo3 & mid3 & top2;
}

// The same classes from two lookups (round 4): bits [2:0] and bits [6:3] of the byte.  The 16-entry
// lookup leans on v_perm's fixed selectors (8-11: the sign bits of table bytes 1, 3, 5, 7, all 0 here;
// 12: 0x00; 13-15: 0xFF), so bytes 0x68-0x7F would read "every class" from it: the lo-table entries
// that carry a class also carry bit 7, and a class word with bit 7 set (the ASCII bytes h j m p r u x
// z }) sends the wave-tile to classify4.  Bit 7 of the byte is not looked at: a byte >= 0x80 sends the
// wave-tile there too.  Every other ASCII byte gets exactly classify4's bits 0-3 (checked for all 128).
__device__ __forceinline__ u32 classify4_fast(u32 w) {
    const u32 lo3 = __builtin_amdgcn_perm(0x00008300u, 0x00890084u, w & 0x07070707u);
    const u32 hi4 = __builtin_amdgcn_perm(0x08000004u, 0x00000300u, (w >> 3) & 0x0F0F0F0Fu);
    return lo3 & hi4;
}

// Class K of 16 bytes (four class words, byte i of word j = position 4j + i) -> a 16-bit mask.
// v_dot4_u32_u8 gathers the flag bytes at full rate: weights 1,2,4,8 place word 0's bytes at
// bits 0-3, weights 16..128 word 1's at bits 4-7 (every product is scaled by 2^K, undone at
// the end); no quarter-rate 32-bit multiplies.
template <int K>
__device__ __forceinline__ u32 gather16(u32 c0, u32 c1, u32 c2, u32 c3) {
    constexpr u32 M = 0x01010101u << K;
    u32 v = __builtin_amdgcn_udot4(c0 & M, 0x08040201u, 0u, false);
    v = __builtin_amdgcn_udot4(c1 & M, 0x80402010u, v, false);
    u32 u = __builtin_amdgcn_udot4(c2 & M, 0x08040201u, 0u, false);
    u = __builtin_amdgcn_udot4(c3 & M, 0x80402010u, u, false);
    return (v | (u << 8)) >> K;
}

// The tally's classifier works on pairs of dwords (FR_CLS_PAIR 1, the product build).  FR_CLS_PAIR 0
// keeps the one-dword loop over classify4_fast: scripts/build_exp.sh NAME "-DFR_CLS_PAIR=0" builds it
// from the same tree for A/B runs.  Results do not depend on the switch.
#ifndef FR_CLS_PAIR
#define FR_CLS_PAIR 1
#endif

// classify4_fast's two lookups on two consecutive dwords, with two variants of the tables: variant A
// (dword wa, bytes 0-3 of the pair) puts its class flags in the low nibble, variant B (dword wb, bytes
// 4-7) the same classes four bits higher, and the two class words are ORed.  Byte i of the pair word:
//   bit 0 line end of byte i          bit 4 line end of byte 4 + i
//   bit 1 ':' of byte i               bit 5 ':' of byte 4 + i
//   bit 3 ' ' of byte i               bit 7 ' ' of byte 4 + i
//   bit 2 '\r' and bit 6 the sentinel, of either byte: only ever tested over the whole wave-tile.
// A class then takes one mask and one v_dot4_u32_u8 per 8 bytes (gather16p), not per 4.
// v_perm's selectors 8-11 return the sign bit of table bytes 1, 3, 5, 7, so no hi-table entry at an odd
// index may carry bit 7, or bytes 0x40-0x5F would read 0xFF: '\n' and '\r' (index 1) and ':' (index 7)
// cannot sit at bit 7 of variant B, ' ' (index 4) can.  Selectors 13-15 return 0xFF, so bytes 0x68-0x7F
// get their lo-table entry as it is: the entries that carry a class also carry the sentinel, and a pair
// word with the sentinel set (the ASCII bytes h j m p r u x z }, the same nine in both variants, as with
// classify4_fast) sends the wave-tile to classify4.  Both index masks keep bit 7 of the byte (0x87, and
// five bits of w >> 3), so a byte >= 0x80 selects 0xFF in both tables: its class word is 0xFF, sentinel
// included, and the wave-tile goes to classify4 as well, with no OR chain over the raw bytes.  The flagged
// set is those nine ASCII bytes and 0x80-0xFF; every other byte gets exactly its classes
// (tests/test_classifier_pair_tables.py, all 256 bytes in both variants).
constexpr u32 PAIR_CR = 0x04040404u, PAIR_SENTINEL = 0x40404040u;
__device__ __forceinline__ u32 classify8_pair(u32 wa, u32 wb) {
    const u32 lo_a = __builtin_amdgcn_perm(0x00004500u, 0x00430048u, wa & 0x87878787u);
    const u32 hi_a = __builtin_amdgcn_perm(0x02000008u, 0x00000500u, (wa >> 3) & 0x1F1F1F1Fu);
    const u32 lo_b = __builtin_amdgcn_perm(0x00005400u, 0x007000C0u, wb & 0x87878787u);
    const u32 hi_b = __builtin_amdgcn_perm(0x20000080u, 0x00001400u, (wb >> 3) & 0x1F1F1F1Fu);
    // (lo_a & hi_a) | b in one v_bitop3 (truth table 0xF0 & 0xCC | 0xAA): left to itself the compiler keeps
    // the two halves apart and ORs them once more for the wave-tile test
    return __builtin_amdgcn_bitop3_b32(lo_a, hi_a, lo_b & hi_b, 0xEAu);
}

// Class K (0 line end, 1 ':', 3 ' ') of 16 bytes (two pair words) -> a 16-bit mask scaled by 2^K.
// Weights 1, 2, 4, 8 sum byte i's low-nibble flag to bit i and its high-nibble flag to bit 4 + i: 8 bytes
// in natural order per dot4, no carry (each nibble sums to at most 15).
template <int K>
__device__ __forceinline__ u32 gather16p(u32 d0, u32 d1) {
    constexpr u32 M = 0x11111111u << K;
    const u32 v = __builtin_amdgcn_udot4(d0 & M, 0x08040201u, 0u, false);
    const u32 u = __builtin_amdgcn_udot4(d1 & M, 0x08040201u, 0u, false);
    return v | (u << 8);
}

// (a << S) | b as one v_lshl_or_b32, whatever the optimizer would make of the expression around it
template <int S>
__device__ __forceinline__ u32 lshl_or(u32 a, u32 b) {
    u32 r;
    asm("v_lshl_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "n"(S), "v"(b));
    return r;
}

// four gather16p quarters -> the segment's 64-bit bitmap; the 2^K scale is undone once per 32-bit half.
// Per half: the low quarter's shift (none for K = 0) and one v_lshl_or_b32.  Written as plain shifts and ORs the
// compiler spreads the shifts over the dot4 results again: two shifts, a v_lshl_or and a v_or3 per half.
template <int K>
__device__ __forceinline__ u64 join16p(const u32 (&g)[4]) {
    const u32 lo = lshl_or<16 - K>(g[1], g[0] >> K), hi = lshl_or<16 - K>(g[3], g[2] >> K);
    return ((u64)hi << 32) | (u64)lo;
}

__device__ __forceinline__ u64 agent_load(const u64* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void agent_store(u64* p, u64 v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// ------------------------------------------------------------------------------------
// the tally kernel (v8): per-wave walkers
//
// A workgroup takes a chunk (a contiguous run of wave-tiles) by ticket and splits it into four
// contiguous parts, one per wave.  Each wave walks its part alone: no workgroup barrier inside the
// tile loop, so a wave that waits for its next tile's loads does not hold the other three (round 2
// had two barriers per 16-KiB workgroup tile; MI355X measurements in profiles/r03a_ubench_tile.txt:
// the barrier-free walk is 8-12 % faster at equal loads and parse work).  A wave-tile is 4 KiB: lane
// L holds the 64-B segment [64 L, 64 L + 64) in registers, loaded one wave-tile ahead, classifies it
// there, and stores its ' ' / ':' / line-end bitmaps and its bytes to the wave's own LDS area, where
// the lane-owned header parse reads them.  Tiles overlap by one segment (stride TSTEP), so a
// header's bitmap window always has a successor segment.
//
// Line phase per wave: the first wave of chunk 0 starts at the range's exact line count; every
// other wave guesses its starting phase from its first wave-tile (FASTQ structure, infer_phase).
// After the walk the chunk's four counts give each wave's phase relative to the chunk start; a wave
// whose guess disagrees makes the chunk redo with the derived phases, a wave that could not guess
// walks again with its derived phase.  The chunk start itself is exact (chunk 0, or a decoupled
// look-back) or, for device feeds, the first wave's guess, committed at once and checked for the
// whole launch by verify_launch.  Correctness never depends on a guess.
// ------------------------------------------------------------------------------------
struct alignas(16) LSlot {  // one ds_read_b128 reads key, count and first offset together
    u64 key;                 // 0 = empty
    u32 cnt;
    u32 mino;                // min range offset of the code's records, ~0 = none
};

constexpr int NW = WG / 64;                  // waves per workgroup
constexpr int SEGS = TILE / SEG;             // segments per wave-tile (= lanes)
constexpr u32 RARE_WAVE = RARE_RING / NW;    // rare-event ring entries per wave

struct ScanShared {
    u32 raw[NW][TILE / 4];   // each wave's current wave-tile (the parse reads code bytes here)
    LSlot ls[NS];            // LDS hash table of this workgroup's chunk
    u64 bsp[NW][SEGS + 2];   // per wave, per 64-B segment of its staged tile: ' ' | line-end bitmap
    u64 bcol[NW][SEGS + 2];  //                                              ':' bitmap
    u64 beol[NW][SEGS + 2];  //                                              '\r' | '\n' bitmap
                             // entries SEGS, SEGS + 1 stay zero: window words past the tile
    u64 wcount[NW];          // pass 0: line terminators of each wave's part of the chunk
    int wphase[NW];          // pass 0: the phase each wave parsed with (mod 4), -1 count only
    u32 rq_tail[NW];         // rare-event ring: events pushed by each wave (monotonic)
    u64 tile_excl;
    u64 cbase;               // the chunk's first byte in the range: positions inside a chunk are u32 offsets
                             // from it (chunks are <= 512 tiles), so a range may exceed 4 GiB
    u32 chunk;
    u32 nkeys;               // occupied LDS slots
    u32 created;             // HBM slots this workgroup created (added to n_keys once, at exit)
    u32 flags;
    u32 last;                // this workgroup published the launch's last chunk count (runs verify_launch)
    u32 spec;                // side effects are buffered (a phase in use is a guess); the chunk may be redone
    u32 spec_bad;            // a speculation buffer overflowed: redo this chunk exactly
    u32 ncold;               // cold list fill
    u32 nexo;                // buffered exotic records
    u32 err_off;             // min range offset of a header without ' ' (buffered), ~0 none
    u32 log_on;              // commit: pairs this commit logs
    u32 exo_p[EXO_BUF], exo_start[EXO_BUF], exo_len[EXO_BUF];
};

typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) u32 lds_u32;
typedef __attribute__((address_space(3))) u32x4 lds_u32x4;
typedef __attribute__((address_space(3))) u64 lds_u64;
typedef __attribute__((address_space(3))) u8 lds_u8;

// Ordinal of a record: file tag << 44 | its header's file offset rounded down to a multiple of 4.  Record
// starts are >= 4 bytes apart (four lines of >= 1 byte), so the rounding keeps every comparison of two
// records' ordinals, i.e. the first-occurrence order; it lets the launch log's fold keep a first
// occurrence in 32 bits for launches up to 16 GiB (log_reduce_kernel).  Every path rounds alike.
__device__ __forceinline__ u64 make_ord(const ScanArgs& a, u64 off_in_range) {
    return ((u64)a.file_tag << ORD_SHIFT) | ((a.file_offset + off_in_range) & ~3ull);
}

__device__ __forceinline__ u32 wave_id() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }

// this wave's LDS stores are complete: later reads by other lanes of the wave see them (a wave's LDS
// operations execute in order; the wait also keeps the compiler from moving reads above the stores).
// LDS only: outstanding global loads (the next tile) stay in flight.
__device__ __forceinline__ void lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// workgroup barrier that orders LDS only: outstanding global loads, stores and atomics stay in flight
// (__syncthreads() would wait for every one of them)
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

__device__ FR_COLD void direct_insert(ScanShared& sh, const ScanArgs& a, u64 key, u32 off) {
    if (global_insert(a.tabv, a.st, key, 1, make_ord(a, sh.cbase + off), a.file_tag)) atomicAdd(&sh.created, 1u);
}

__device__ __forceinline__ void rare_push(ScanShared& sh, const ScanArgs& a, u32 p, u32 kind, u32 x, u32 y);

// An LDS-table miss of the tile loop, held in the lane until the next tile's top (walk_wave): gfx950 counts
// stores and loads in one vmcnt, so a cold-list store issued after the next tile's loads is waited for, up to
// its acknowledge from L2, at the loop-top wait for those loads.  Flushed ahead of them it has a wave-tile's
// time to drain.
constexpr u32 COLD_NONE = 0xFFFFFFFFu;
struct ColdPend {
    u64 key;
    u32 off;  // the record's chunk offset, COLD_NONE: nothing pending
};

// what a cold-list entry needs beside the miss itself; none of it changes during a walk
typedef __attribute__((address_space(1))) u32x4 global_u32x4;  // a global (not flat) store, whatever the optimizer infers
struct ColdDest {
    global_u32x4* list;  // this workgroup's cold list
    u32 cap;
    u64 obase;    // file offset of the chunk's first byte: an entry's ordinal is tag | (obase + off) & ~3 (make_ord)
    u64 tag;      // file tag << ORD_SHIFT
};

__device__ __forceinline__ u32 uniform32(u32 v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ u64 uniform64(u64 v) {
    return ((u64)uniform32((u32)(v >> 32)) << 32) | uniform32((u32)v);
}

__device__ __forceinline__ ColdDest cold_dest(const ScanShared& sh, const ScanArgs& a) {
    ColdDest d;
    d.cap = uniform32(a.cold_cap);
    d.list = (global_u32x4*)uniform64((u64)(a.cold + 2ull * ((u64)blockIdx.x * d.cap)));
    d.obase = uniform64(a.file_offset + sh.cbase);
    d.tag = (u64)uniform32(a.file_tag) << ORD_SHIFT;
    return d;
}

// Park one LDS-table miss in the workgroup's cold list (committed with the chunk), in two steps: claim the
// entry's index i, then one 16-byte store {key, ordinal} (the list is 16-byte aligned: hipMalloc, 16-byte
// entries).  A full list: the chunk is redone exactly when it speculates, else the insert goes to the HBM table,
// directly from drain_rare or queued for it from the tile loop.
__device__ __forceinline__ u32 cold_claim(ScanShared& sh) { return atomicAdd(&sh.ncold, 1u); }

template <bool DRAIN>
__device__ __forceinline__ void cold_put_at(ScanShared& sh, const ScanArgs& a, const ColdDest& d, u64 key, u32 off,
                                            u32 i) {
    if (i < d.cap) {
        const u64 ord = d.tag | ((d.obase + off) & ~3ull);
        // ablation 16: the context's first three launches fill the lists, later ones leave them as they are
        if (!(ABLATE & 16u) || a.epoch <= 3u) d.list[i] = u32x4{(u32)key, (u32)(key >> 32), (u32)ord, (u32)(ord >> 32)};
        else asm volatile("" ::"v"(ord), "v"(key));
        return;
    }
    if (sh.spec) {  // cannot insert while speculating: this chunk will be redone exactly
        atomicOr(&sh.spec_bad, 1u);
        return;
    }
    // exact phase and a full cold list: insert directly (queued out of the hot loop)
    if (DRAIN) direct_insert(sh, a, key, off);
    else rare_push(sh, a, off, 3u, (u32)key, (u32)(key >> 32));
}

template <bool DRAIN>
__device__ __forceinline__ void cold_put(ScanShared& sh, const ScanArgs& a, const ColdDest& d, u64 key, u32 off) {
    cold_put_at<DRAIN>(sh, a, d, key, off, cold_claim(sh));
}

// The lanes' pending misses, if any, go to the cold list; the whole wave calls both halves, and a scalar branch
// skips them when no lane holds a miss.  walk_wave claims before the tile copy and stores after it, so the LDS
// atomic's round trip passes under the copy's four ds_write_b128 instead of behind them.
__device__ __forceinline__ bool cold_flush_claim(ScanShared& sh, const ColdPend& pd, u32& i) {
    const bool any = __ballot(pd.off != COLD_NONE) != 0;
    i = 0;
    if (any && pd.off != COLD_NONE) i = cold_claim(sh);
    return any;
}
__device__ __forceinline__ void cold_flush_store(ScanShared& sh, const ScanArgs& a, const ColdDest& d, ColdPend& pd,
                                                 bool any, u32 i) {
    if (!any) return;
    if (pd.off != COLD_NONE) cold_put_at<false>(sh, a, d, pd.key, pd.off, i);
    pd.off = COLD_NONE;
}

// DRAIN (drain_rare's paths): a miss is stored at once.  Otherwise (the tile loop) it stays pending in pd, and a
// lane that already holds one (a second header in its segment: records shorter than 64 B) stores the older first.
template <bool DRAIN = false>
__device__ __forceinline__ void lds_insert(ScanShared& sh, const ScanArgs& a, u64 key, u32 off, const ColdDest* d,
                                           ColdPend* pd) {
    // one 32-bit multiply (keys hold <= 63 bits: fold the top down first)
    u32 h = (((u32)key ^ (u32)(key >> 27)) * 0x9E3779B1u) >> (32 - LOG_NS);
#pragma unroll 2
    for (int pr = 0; pr < LPROBE; ++pr) {
        // volatile through an explicit LDS pointer: a volatile access through a generic pointer
        // keeps its flat form (flat loads wait on vmcnt(0), i.e. on every outstanding HBM op).  The key
        // count is read in the same round as the slot (a new key's claim then costs no extra round trip)
        u32x4 sl = *(const lds_u32x4*)&sh.ls[h];
        u32 nk = *(const lds_u32*)&sh.nkeys;
        asm volatile("" : "+v"(sl), "+v"(nk) :: "memory");  // both loads in one round, not moved or reused
        u64 k = ((u64)sl.y << 32) | sl.x;
        u32 mino = sl.w;
        if (k == 0) {
            // a full LDS table stops claiming slots: the code goes to the cold list; the codes
            // already resident (the hot ones arrive first) keep aggregating here
            if (nk >= a.flush_at) break;
            const u64 old = atomicCAS((unsigned long long*)&sh.ls[h].key, 0ull, (unsigned long long)key);
            if (old == 0) {
                atomicAdd(&sh.nkeys, 1u);
                k = key;
            } else {
                k = old;
            }
            mino = 0xFFFFFFFFu;
        }
        if (k == key) {
            atomicAdd(&sh.ls[h].cnt, 1u);
            // mino only decreases, so a stale read can only cause a redundant atomic
            if (off < mino) atomicMin(&sh.ls[h].mino, off);
            return;
        }
        h = (h + 1) & (NS - 1);
    }
    // an LDS-table miss
    if (DRAIN) {
        cold_put<true>(sh, a, cold_dest(sh, a), key, off);
    } else {
        if (pd->off != COLD_NONE) cold_put<false>(sh, a, *d, pd->key, pd->off);
        pd->key = key;
        pd->off = off;
    }
}

// Rare events (exotic codes, headers without ' ', headers whose code leaves the bitmap window,
// direct HBM inserts, UTF-8 checks) go to the wave's ring in HBM and are handled by drain_rare at
// the wave's next tile, so their code adds no registers to the tile loop.  Entry: {chunk offset,
// kind, x, y}.  No fence here (a release would wait for the next tile's loads): drain_rare fences.
__device__ __forceinline__ void rare_push(ScanShared& sh, const ScanArgs& a, u32 p, u32 kind, u32 x, u32 y) {
    const u32 wid = wave_id();
    const u32 i = atomicAdd(&sh.rq_tail[wid], 1u);
    a.rare[(u64)blockIdx.x * RARE_RING + wid * RARE_WAVE + (i & (RARE_WAVE - 1u))] = make_uint4(p, kind, x, y);
}

// Decoupled look-back over the launch's chunk descriptors {tag = 2*epoch + inclusive, value}.
// The chunk's own aggregate was published before (chunk_kernel); this resolves its exclusive
// prefix, reading 256 predecessors per poll (4 per lane), and publishes the inclusive prefix.
// Returns the number of line terminators in chunks [0, t) of the range.
__device__ __forceinline__ u64 lookback(const ScanArgs& a, u32 t, u32 agg, int lane) {
    if (t == 0) return 0;  // chunk 0 published its inclusive value directly
    const u64 tagI = (u64)(2u * a.epoch + 1u) << 32;
    u64 excl = 0;
    i64 j = (i64)t - 1;
    u32 spins = 0;
    for (;;) {
        u64 sv[4], rdy[4], inc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const i64 idx = j - 64 * k - lane;
            sv[k] = idx >= 0 ? agent_load(&a.tiles[idx]) : tagI;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const u32 tag = (u32)(sv[k] >> 32);
            const bool ready = (tag >> 1) == a.epoch;
            rdy[k] = __ballot(ready);
            inc[k] = __ballot(ready && (tag & 1u));
        }
        int kf = 4, lf = 63;
#pragma unroll
        for (int k = 3; k >= 0; --k)
            if (inc[k]) {
                kf = k;
                lf = __ffsll((long long)inc[k]) - 1;
            }
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const u64 need = k < kf ? ~0ull : k == kf ? (lf == 63 ? ~0ull : ((1ull << (lf + 1)) - 1ull)) : 0ull;
            ok &= (rdy[k] & need) == need;
        }
        if (!ok) {
            if (++spins > SPIN_MAX) {
                if (lane == 0) atomicOr(&a.st->spin_fail, 1u);
                return 0;
            }
            if (spins > 2) __builtin_amdgcn_s_sleep(8);
            continue;
        }
        u64 contrib = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < kf || (k == kf && lane <= lf)) contrib += (u32)sv[k];
        excl += wave_sum_u64(contrib);
        if (kf < 4) break;
        j -= 256;
    }
    if (lane == 0) {
        agent_store(&a.tiles[t], tagI | (u64)(u32)(excl + agg));
        if (spins) {
            atomicMax(&a.st->spin_max, spins);
            atomicAdd((unsigned long long*)&a.st->spin_total, (unsigned long long)spins);
        }
    }
    return excl;
}

// validate UTF-8 for the range bytes [s0, s0+n) (only called when a byte >= 0x80 is present);
// bytes are read from HBM (the range, and before it when readable), -1 past them.
__device__ FR_COLD bool utf8_segment_ok(const ScanArgs& a, u64 s0, u32 n) {
    auto byte_at = [&](i64 q) -> int {
        if (q < 0 && !a.pre_valid) return -1;
        if (q >= (i64)a.avail) return -1;
        return (int)a.buf[q];
    };
    for (i64 q = (i64)s0; q < (i64)s0 + (i64)n; ++q) {
        const int b = byte_at(q);
        if (b < 0x80) continue;
        if (b >= 0x80 && b <= 0xBF) {  // continuation: must be claimed by a lead
            bool claimed = false;
            for (int j = 1; j <= 3; ++j) {
                const int c = byte_at(q - j);
                if (c < 0) break;
                if (c >= 0x80 && c <= 0xBF) continue;
                const int need = c >= 0xF0 ? 4 : c >= 0xE0 ? 3 : c >= 0xC0 ? 2 : 1;
                claimed = need > j;
                break;
            }
            if (!claimed) return false;
            continue;
        }
        int need;
        if (b >= 0xC2 && b <= 0xDF) need = 2;
        else if (b >= 0xE0 && b <= 0xEF) need = 3;
        else if (b >= 0xF0 && b <= 0xF4) need = 4;
        else return false;
        for (int j = 1; j < need; ++j) {
            const int c = byte_at(q + j);
            if (c < 0x80 || c > 0xBF) return false;
            if (j == 1) {
                if (b == 0xE0 && c < 0xA0) return false;
                if (b == 0xED && c > 0x9F) return false;
                if (b == 0xF0 && c < 0x90) return false;
                if (b == 0xF4 && c > 0x8F) return false;
            }
        }
    }
    return true;
}

// d, pd: the tile loop's (DRAIN = false) cold-list destination and the lane's pending miss
template <bool DRAIN = false>
__device__ __forceinline__ void count_code(ScanShared& sh, const ScanArgs& a, u32 p, u64 key,
                                           const ColdDest* d = nullptr, ColdPend* pd = nullptr) {
    if ((ABLATE & 4u) || a.exo_only) {  // ablation / exotic-only replay: skip the hash insert
        asm volatile("" ::"v"(key));
        return;
    }
    lds_insert<DRAIN>(sh, a, key, p, d, pd);
}

// code bytes [q, q+n) of the range (exact byte reads) -> wide key (fr_internal.h), false when the
// code is outside the wide form.  Only called for codes that are not fast keys.
__device__ bool wide_encode(const ScanArgs& a, u64 q, u64 n, u64& key) {
    if (n < 1 || n > (u64)WIDE_MAXN + 1) return false;
    int lower = -1, plus = WIDE_NOPLUS, nl = 0;
    u64 v = 0, pw = 1;
    for (u64 k = 0; k < n; ++k) {
        const u32 c = a.buf[q + k];
        if (c == '+') {
            if (plus != WIDE_NOPLUS) return false;
            plus = nl;
            continue;
        }
        const u32 lc = c | 0x20u;
        const int d = lc == 'a' ? 0 : lc == 'c' ? 1 : lc == 'g' ? 2 : lc == 't' ? 3 : lc == 'n' ? 4 : -1;
        if (d < 0 || nl >= WIDE_MAXN) return false;
        const int isl = (c & 0x20u) ? 1 : 0;
        if (lower < 0) lower = isl;
        else if (lower != isl) return false;
        v += (u64)d * pw;
        pw *= 5;
        ++nl;
    }
    if (lower < 0) return false;  // no letter
    const int n1 = plus == WIDE_NOPLUS ? nl : plus, n2 = plus == WIDE_NOPLUS ? 0 : nl - plus;
    if (n1 > MAXSYM || n2 > MAXSYM) return false;
    key = WIDE_BIT | ((u64)lower << 62) | ((u64)plus << 57) | (v + (pw - 1) / 4);
    return true;
}

// a code the fast encoder did not take (header p: chunk offset; code [start, start + n): range offsets): exact
// fast form (defensive), wide key, or an exotic record captured verbatim (speculating: its position
// is buffered and the bytes stay resident in HBM)
__device__ void exotic_record(const ScanArgs& a, u32 p, u64 start, u64 n, ScanShared& sh) {
    {
        bool fast = n >= 1 && n <= (u64)MAXSYM;
        u64 key = 0;
        for (u64 i = 0; fast && i < n; ++i) {
            const u32 sy = sym_of(a.buf[start + i]);
            fast = sy != 0;
            key |= (u64)sy << (3 * i);
        }
        if (fast || wide_encode(a, start, n, key)) {
            count_code<true>(sh, a, p, key);
            return;
        }
    }
    if (sh.spec) {  // speculating: remember where it is; the bytes stay resident in HBM
        const u32 k = atomicAdd(&sh.nexo, 1u);
        if (k < (u32)EXO_BUF) {
            sh.exo_p[k] = p;
            sh.exo_start[k] = (u32)(start - sh.cbase);
            sh.exo_len[k] = (u32)n;
        } else {
            atomicOr(&sh.spec_bad, 1u);
        }
        return;
    }
    const u64 i = atomicAdd((unsigned long long*)&a.st->n_exotic, 1ull);
    const u64 po = atomicAdd((unsigned long long*)&a.st->exo_pool_used, (unsigned long long)n);
    if (i < a.tabv.exo_cap && po + n <= a.tabv.exo_pool_cap) {
        a.tabv.exo_ord[i] = make_ord(a, sh.cbase + p);
        a.tabv.exo_off[i] = po;
        a.tabv.exo_len[i] = (u32)n;
        for (u64 k = 0; k < n; ++k) a.tabv.exo_pool[po + k] = a.buf[start + k];
    } else {
        atomicOr(&a.st->cap_flags, 4u);
    }
}

__device__ __forceinline__ void nospace(const ScanArgs& a, u32 p, ScanShared& sh) {  // IndexError (:169)
    if (sh.spec) atomicMin(&sh.err_off, p);
    else atomicMin((unsigned long long*)&a.st->err_nospace, (unsigned long long)(a.file_offset + sh.cbase + p));
}

// slow path (rare): a header whose code does not end inside its bitmap windows, parsed byte by
// byte from HBM.  R2 (frender.py:169): the token after the first ' ' up to the next ' ' or line
// end, then its suffix after the last ':'.  p = the header's chunk offset.
__device__ FR_COLD void process_header_global(ScanShared& sh, const ScanArgs& a, u32 p) {
    const u64 eof = a.avail;
    auto rd = [&](u64 q) -> u32 { return (u32)a.buf[q]; };
    u64 q = sh.cbase + p;
    for (;;) {
        if (q >= eof) return nospace(a, p, sh);
        const u32 c = rd(q);
        if (c == ' ') break;
        if (c == '\n' || c == '\r') return nospace(a, p, sh);
        ++q;
    }
    const u64 sp1 = q++;
    i64 lc = -1;
    for (;;) {
        if (q >= eof) break;
        const u32 c = rd(q);
        if (c == ' ' || c == '\n' || c == '\r') break;
        if (c == ':') lc = (i64)q;
        ++q;
    }
    const u64 start = (lc >= 0 ? (u64)lc : sp1) + 1;
    const u64 n = q - start;
    u64 key = 0;
    bool fast = n >= 1 && n <= (u64)MAXSYM;
    for (u64 i = 0; fast && i < n; ++i) {
        const u32 sy = sym_of(rd(start + i));
        fast = sy != 0;
        key |= (u64)sy << (3 * i);
    }
    if (fast) count_code<true>(sh, a, p, key);
    else exotic_record(a, p, start, n, sh);
}

// ---- wave-tile staging: lane-contiguous segments classified straight from registers ---------
// Lane L loads its own 64-byte segment [64 L, 64 L + 64) of the wave-tile (four 16-B loads through
// a wave-uniform buffer descriptor) one tile ahead, classifies it in registers and stores it and
// its bitmaps to the wave's LDS area.  (Coalesced 1-KiB-per-instruction loads with an LDS
// transpose, and LDS-DMA rings, measured slower: profiles/r03a_ubench_tile.txt.)
struct SegRegs {
    uint4 v[SEG / 16];
    u32 nx;  // first dword of the next segment (zero past the staged bytes)
};

__device__ __forceinline__ void seg_fetch(const ScanArgs& a, u32 t, SegRegs& r, int lane, bool with_nx = false) {
    const u64 tile0 = (u64)t * TSTEP;
    const u32 nb = (u32)min((u64)TILE, a.avail - tile0);
    const u64 base = (u64)(a.buf + tile0);
    const u32 lo = __builtin_amdgcn_readfirstlane((u32)base), hi = __builtin_amdgcn_readfirstlane((u32)(base >> 32));
    const u8* ub = (const u8*)(((u64)hi << 32) | lo);
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)ub, (short)0, (int)__builtin_amdgcn_readfirstlane(nb),
                                                        0x00020000);
#pragma unroll
    for (int k = 0; k < SEG / 16; ++k) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane * SEG, k * 16, 0);
        r.v[k] = make_uint4(v[0], v[1], v[2], v[3]);
    }
    r.nx = with_nx ? __builtin_amdgcn_raw_buffer_load_b32(rsrc, lane * SEG + SEG, 0, 0) : 0u;  // '\r' path only
}

// the data end (a segment, or the dword after it, reaches past avail): bytewise loads, zeros past
// the staged bytes (the buffer range check is trusted only for whole vectors)
__device__ __attribute__((noinline)) SegRegs seg_load_tail(const ScanArgs& a, u32 t, int lane) {
    const u64 tile0 = (u64)t * TSTEP;
    const u32 nb = (u32)min((u64)TILE, a.avail - tile0);
    const u32 s0 = lane * SEG;
    u32 w[SEG / 4 + 1];
    for (int k = 0; k <= SEG / 4; ++k) {
        u32 v = 0;
        for (u32 q = 0; q < 4; ++q) {
            const u32 o = s0 + 4 * k + q;
            if (o < nb) v |= (u32)a.buf[tile0 + o] << (8 * q);
        }
        w[k] = v;
    }
    SegRegs r;
    for (int k = 0; k < SEG / 16; ++k) r.v[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    r.nx = w[SEG / 4];
    return r;
}

// every lane's segment loads of wave-tile t (and the dword after them) lie inside the data
__device__ __forceinline__ bool seg_in_range(const ScanArgs& a, u32 t) {
    return (u64)t * TSTEP + (TILE + SEG + 4) <= a.avail;
}

__device__ __forceinline__ void seg_load(const ScanArgs& a, u32 t, SegRegs& r, int lane) {
    if (__builtin_expect(seg_in_range(a, t), 1)) seg_fetch(a, t, r, lane);
    else r = seg_load_tail(a, t, lane);
}

struct SegClass {
    u64 tmask, sp, col, eol;  // terminators (own bytes), and the parse bitmaps (staged bytes)
    u32 c, x;                 // popcount(tmask), its inclusive wave scan
    u32 wtot;                 // the wave's terminators (own bytes of the wave-tile)
    bool hi;                  // a byte >= 0x80 among the own bytes (UTF-8 check, kind 4)
};

template <class Src>
__device__ __forceinline__ SegClass seg_classify_src(const ScanArgs& a, u32 t, const Src& src, int lane);

struct Cls16 {  // a segment's class bitmaps in 16-bit quarters, and the OR of its class words
    u32 eol[4], sp[4], col[4], acc;
};

// classify4 over the lane's segment, re-read from memory: the exact path of seg_classify_src
__device__ __attribute__((noinline)) Cls16 classes_exact(const ScanArgs& a, u32 t, int lane) {
    SegRegs q;
    if (seg_in_range(a, t)) seg_fetch(a, t, q, lane);
    else q = seg_load_tail(a, t, lane);
    Cls16 r;
    r.acc = 0;
#pragma unroll
    for (int qv = 0; qv < SEG / 16; ++qv) {
        const u32 c0 = classify4(q.v[qv].x), c1 = classify4(q.v[qv].y), c2 = classify4(q.v[qv].z),
                  c3 = classify4(q.v[qv].w);
        r.eol[qv] = gather16<0>(c0, c1, c2, c3);
        r.sp[qv] = gather16<2>(c0, c1, c2, c3);
        r.col[qv] = gather16<3>(c0, c1, c2, c3);
        r.acc |= c0 | c1 | c2 | c3;
    }
    return r;
}

__device__ __forceinline__ SegClass seg_classify(const ScanArgs& a, u32 t, const SegRegs& r, int lane) {
    return seg_classify_src(a, t, [&](int k) { return r.v[k]; }, lane);
}

// src(k): the segment's k-th 16 bytes (registers, or a read of the wave's LDS copy: then only one
// quarter of the segment is live at a time)
template <class Src>
__device__ __forceinline__ SegClass seg_classify_src(const ScanArgs& a, u32 t, const Src& src, int lane) {
    const u64 tile0 = (u64)t * TSTEP;
    const u32 tlen = (u32)min((u64)TSTEP, a.len - tile0);
    const u32 bl = (u32)min((u64)TILE, a.avail - tile0);
    const u32 s0 = lane * SEG;
    SegClass sc;
    sc.tmask = 0;
    sc.sp = sc.col = sc.eol = 0;
    sc.hi = false;
    if (s0 < bl) {
        u32 eol16[4], sp16[4], col16[4];
        u32 acc = 0;
        auto join = [](const u32 (&g)[4]) {
            return ((u64)(g[2] | (g[3] << 16)) << 32) | (u64)(g[0] | (g[1] << 16));
        };
#if FR_CLS_PAIR
#pragma unroll
        for (int qv = 0; qv < SEG / 16; ++qv) {  // class words live one quarter at a time
            const uint4 v = src(qv);
            const u32 d0 = classify8_pair(v.x, v.y), d1 = classify8_pair(v.z, v.w);
            eol16[qv] = gather16p<0>(d0, d1);
            col16[qv] = gather16p<1>(d0, d1);
            sp16[qv] = gather16p<3>(d0, d1);
            acc |= d0 | d1;
        }
        u64 eol = join16p<0>(eol16), sp = join16p<3>(sp16), col = join16p<1>(col16);
        bool cr = (acc & PAIR_CR) != 0;
        // a sentinel byte or a byte >= 0x80 (0xFF from both tables: the raw bytes need no test of their own)
        const bool slow = (acc & PAIR_SENTINEL) != 0;
#else
        u32 raw = 0;
#pragma unroll
        for (int qv = 0; qv < SEG / 16; ++qv) {  // class words live one quarter at a time
            const uint4 v = src(qv);
            const u32 c0 = classify4_fast(v.x), c1 = classify4_fast(v.y), c2 = classify4_fast(v.z),
                      c3 = classify4_fast(v.w);
            eol16[qv] = gather16<0>(c0, c1, c2, c3);
            sp16[qv] = gather16<2>(c0, c1, c2, c3);
            col16[qv] = gather16<3>(c0, c1, c2, c3);
            acc |= c0 | c1 | c2 | c3;
            raw |= v.x | v.y | v.z | v.w;
        }
        u64 eol = join(eol16), sp = join(sp16), col = join(col16);
        bool cr = (acc & 0x02020202u) != 0;
        const bool slow = ((acc | raw) & 0x80808080u) != 0;
#endif
        // bit 4 (byte >= 0x80) exists in classify4's class words only (in a pair word it is a line end)
        u32 hib = 0;
        if (__builtin_expect(__ballot(slow) != 0, 0)) {  // a wave-uniform SGPR value: a scalar branch
            // a byte >= 0x80 or a fast-table sentinel somewhere in the wave-tile: the exact classifier,
            // out of line on the segment re-read from L2 (no register of the common path is held for it)
            const Cls16 e = classes_exact(a, t, lane);
            eol = join(e.eol);
            sp = join(e.sp);
            col = join(e.col);
            cr = (e.acc & 0x02020202u) != 0;
            hib = e.acc & 0x10101010u;
        }
        u64 tm = eol;
        if (__builtin_expect(__ballot(cr) != 0, 0)) {
            // '\r' somewhere in the wave (CRLF / CR files): a '\r' right before a '\n' ends no line.
            // The segment (and the byte after it) is re-read from L2 here, so no class word has to
            // stay live through the common path.
            SegRegs q;
            if (seg_in_range(a, t)) seg_fetch(a, t, q, lane, true);
            else q = seg_load_tail(a, t, lane);
            u32 cr16[4];
#pragma unroll
            for (int qv = 0; qv < SEG / 16; ++qv)
                cr16[qv] = gather16<1>(classify4(q.v[qv].x), classify4(q.v[qv].y), classify4(q.v[qv].z),
                                       classify4(q.v[qv].w));
            const u64 crm = join(cr16), nl = eol & ~crm;
            const u64 nxt = (q.nx & 0xFFu) == (u32)'\n' ? 1ull : 0ull;
            tm = eol & ~(crm & ((nl >> 1) | (nxt << 63)));
        }
        // a whole wave-tile (uniform; every one but the range's last two): all staged bytes are data and the own
        // bytes end with lane SEGS - 2's segment, so no lane has a partial mask to build
        if (__builtin_expect(bl == (u32)TILE && tlen == (u32)TSTEP, 1)) {
            sc.sp = sp;
            sc.col = col;
            sc.eol = eol;
            if (s0 < (u32)TSTEP) {
                sc.tmask = tm;
                sc.hi = hib != 0;
            }
        } else {
            const u32 bvalid = bl - s0;
            if (bvalid < SEG) {
                const u64 vm = (1ull << bvalid) - 1ull;
                sp &= vm;
                col &= vm;
                eol &= vm;
            }
            if (s0 < tlen) {
                const u32 valid = tlen - s0;
                if (valid < SEG) tm &= (1ull << valid) - 1ull;
            } else {
                tm = 0;
            }
            sc.sp = sp;
            sc.col = col;
            sc.eol = eol;
            if (s0 < tlen) {
                sc.tmask = tm;
                sc.hi = hib != 0;  // exact own-byte test in drain_rare (kind 4)
            }
        }
    }
    sc.c = __popcll(sc.tmask);
    // inclusive wave scan of c: DPP row shifts within 16-lane rows, then row broadcasts
    u32 x = sc.c;
    x += __builtin_amdgcn_update_dpp(0u, x, 0x111, 0xF, 0xF, true);  // row_shr:1
    x += __builtin_amdgcn_update_dpp(0u, x, 0x112, 0xF, 0xF, true);  // row_shr:2
    x += __builtin_amdgcn_update_dpp(0u, x, 0x114, 0xF, 0xF, true);  // row_shr:4
    x += __builtin_amdgcn_update_dpp(0u, x, 0x118, 0xF, 0xF, true);  // row_shr:8
    x += __builtin_amdgcn_update_dpp(0u, x, 0x142, 0xA, 0xF, false);  // row_bcast:15 -> rows 1, 3
    x += __builtin_amdgcn_update_dpp(0u, x, 0x143, 0xC, 0xF, false);  // row_bcast:31 -> rows 2, 3
    sc.x = x;
    sc.wtot = __builtin_amdgcn_readlane(x, 63);
    return sc;
}

__device__ FR_COLD void slow_header(ScanShared& sh, const ScanArgs& a, u32 p, int r, u32 start, u32 n);

// handle this wave's ring entries [from, to) (its lanes; the wave pushes nothing meanwhile)
__device__ __attribute__((noinline)) void drain_rare(ScanShared& sh, const ScanArgs& a, u32 wid, u32 from, u32 to,
                                                     int lane) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // the wave's ring stores are visible to its loads
    const uint4* q = a.rare + (u64)blockIdx.x * RARE_RING + wid * RARE_WAVE;
    for (u32 i = from + lane; i - from < to - from; i += 64) {
        const uint4 e = q[i & (RARE_WAVE - 1u)];
        if (e.y == 3u) {
            direct_insert(sh, a, ((u64)e.w << 32) | e.z, e.x);
        } else if (e.y == 4u) {  // UTF-8: the segment's own bytes [e.x, e.x + e.z) of the chunk
            const u64 x = sh.cbase + e.x;
            bool hi = false;
            for (u32 k = 0; k < e.z; ++k) hi |= a.buf[x + k] >= 0x80;
            if (hi) {
                atomicOr(&sh.flags, 1u);
                if (!utf8_segment_ok(a, x, e.z)) atomicOr(&sh.flags, 2u);
            }
        } else {
            slow_header(sh, a, e.x, (int)e.y, e.z, e.w);
        }
    }
}

// phase inference bitmaps of a wave's first tile: '@' and '+' (first bytes of header / separator
// lines); exact per-byte equality, once per wave and chunk
__device__ __forceinline__ void seg_marks(const SegRegs& r, u64& at, u64& plus) {
    at = 0;
    plus = 0;
#pragma unroll
    for (int qv = 0; qv < SEG / 16; ++qv) {
        const u32 w[4] = {r.v[qv].x, r.v[qv].y, r.v[qv].z, r.v[qv].w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            at |= (u64)eq4(w[k], 0x40404040u) << (qv * 16 + k * 4);
            plus |= (u64)eq4(w[k], 0x2B2B2B2Bu) << (qv * 16 + k * 4);
        }
    }
}

// Guess P = (lines before the wave-tile) mod 4 from its first PHASE_LINES complete lines: with lines
// indexed P+k+1 after the k-th terminator, a FASTQ record has a header ('@') at phase 0, '+' at
// phase 2 and equal seq/qual lengths at phases 1/3.  Exactly one consistent P -> the guess;
// otherwise -1 (unsure).  Bitmaps (staged by the caller, the wave's area): bcol = '@', beol = '+'.
// Line lengths include a '\r' of "\r\n" (equal on both lines of a consistently terminated record).
// All lanes at once (round 4; it was one lane walking the lines while the wave waited): the
// terminators e_0 .. e_PHASE_LINES of the tile go to LDS by their index in the tile (each lane writes
// its own, from the wave's terminator scan), then lane k checks line k = (e_k, e_{k+1}) against the
// four candidate phases and ballots decide.
__device__ __forceinline__ int infer_phase(ScanShared& sh, const SegClass& sc, int lane, u32 wid) {
    lds_u32* E = (lds_u32*)&sh.raw[wid][0];  // the wave's tile copy is free until its walk starts
    u32 i = sc.x - sc.c;                      // this lane's first terminator's index in the tile
    u64 m = sc.tmask;
    while (m && i <= (u32)PHASE_LINES) {
        E[i] = (u32)lane * SEG + (u32)__builtin_ctzll(m);
        m &= m - 1ull;
        ++i;
    }
    lds_fence();
    const u32 tot = __builtin_amdgcn_readlane(sc.x, 63);  // terminators in the tile
    const int K = (int)min(tot, (u32)PHASE_LINES + 1u) - 1;  // complete lines looked at
    if (K < 8) return -1;
    const bool valid = lane < K;
    int len = 0;
    bool is_at = false, is_plus = false;
    if (valid) {
        const u32 st = E[lane] + 1u;
        len = (int)E[lane + 1] - (int)st;
        is_at = len > 0 && ((sh.bcol[wid][st >> 6] >> (st & 63u)) & 1ull);
        is_plus = len > 0 && ((sh.beol[wid][st >> 6] >> (st & 63u)) & 1ull);
    }
    const int len2 = __shfl(len, lane - 2, 64);  // line k - 2: the phase-1 line before a phase-3 line
    int found = -1, nfound = 0;
#pragma unroll
    for (int P = 0; P < 4; ++P) {
        const int ph = (P + lane + 1) & 3;
        const bool bad = valid && ((ph == 0 && !is_at) || (ph == 2 && !is_plus) || (ph == 3 && lane >= 2 && len != len2));
        if (__ballot(bad) == 0) {
            found = P;
            ++nfound;
        }
    }
    return nfound == 1 ? found : -1;
}

// the line phase at wave-tile t, guessed from its content (infer_phase); -1 unsure.  Whole wave.
__device__ __attribute__((noinline)) int guess_phase(ScanShared& sh, const ScanArgs& a, u32 t, int lane, u32 wid) {
    SegRegs r;
    seg_load(a, t, r, lane);
    const SegClass sc = seg_classify(a, t, r, lane);
    u64 at, plus;
    seg_marks(r, at, plus);
    sh.bcol[wid][lane] = at;  // infer_phase: '@', '+'
    sh.beol[wid][lane] = plus;
    lds_fence();
    return infer_phase(sh, sc, lane, wid);
}

// Commit: resolve first, update last.  A wait for a load or CAS return also waits for every
// vector-memory op issued before it (vmcnt counts in order), and under the streaming load of the
// other workgroups each round trip is long; so every entry's table slot is found before any count
// is added.  resolve_batch walks CE entries per lane in rounds: the probe loads of all pending
// entries together, then the CASes that claim empty slots together; it adds nothing.  The count /
// first / tag atomics follow in apply_entry, fire-and-forget: an LDS-only barrier ends the commit.
struct Resolved {
    u32 slot;      // the key's slot; ~0: probe bound exceeded (the overflow list takes the entry)
    u32 tag;       // the slot's last_tag as loaded (0: claimed now, or unknown)
    u64 first;     // the slot's first as loaded (~0: claimed now, or unknown)
};

template <int CE>
__device__ __forceinline__ u32 resolve_batch(const ScanArgs& a, const u64 (&key)[CE], const bool (&valid)[CE],
                                             Resolved (&rs)[CE]) {
    const Table& T = a.tabv;
    bool pend[CE];
#pragma unroll
    for (int b = 0; b < CE; ++b) {
        rs[b].slot = (u32)table_home(key[b], T.mask);
        rs[b].first = ~0ull;
        rs[b].tag = 0;
        pend[b] = valid[b];
    }
    u32 made = 0;
    for (int round = 0; round < GPROBE; ++round) {
        bool any = false;
#pragma unroll
        for (int b = 0; b < CE; ++b) any |= pend[b];
        if (!any) return made;
        u64 k[CE];
#pragma unroll
        for (int b = 0; b < CE; ++b)
            if (pend[b]) {
                const GSlot* sl = &T.slots[rs[b].slot];
                const uint2 w0 = *(const uint2*)sl;
                const uint4 w1 = *((const uint4*)sl + 1);
                k[b] = ((u64)w0.y << 32) | w0.x;
                rs[b].first = ((u64)w1.y << 32) | w1.x;
                rs[b].tag = w1.z;
            }
        bool cas[CE];
#pragma unroll
        for (int b = 0; b < CE; ++b) {
            cas[b] = false;
            if (!pend[b]) continue;
            if (k[b] == key[b]) pend[b] = false;
            else if (k[b] == 0) cas[b] = true;
            else rs[b].slot = (rs[b].slot + 1u) & (u32)T.mask;
        }
        u64 old[CE];
#pragma unroll
        for (int b = 0; b < CE; ++b)
            if (cas[b]) old[b] = atomicCAS((unsigned long long*)&T.slots[rs[b].slot].key, 0ull, (unsigned long long)key[b]);
#pragma unroll
        for (int b = 0; b < CE; ++b) {
            if (!cas[b]) continue;
            if (old[b] == 0 || old[b] == key[b]) {  // claimed now, or by another workgroup meanwhile
                made += old[b] == 0 ? 1u : 0u;
                rs[b].first = ~0ull;
                rs[b].tag = 0;
                pend[b] = false;
            } else {
                rs[b].slot = (rs[b].slot + 1u) & (u32)T.mask;
            }
        }
    }
#pragma unroll
    for (int b = 0; b < CE; ++b)
        if (pend[b]) rs[b].slot = ~0u;
    return made;
}

// the fire-and-forget update of one resolved entry (or its overflow-list entry)
__device__ __forceinline__ void apply_entry(const ScanArgs& a, const Resolved& r, u64 key, u32 cnt, u64 ord) {
    const Table& T = a.tabv;
    if (r.slot == ~0u) {  // probe bound exceeded: the overflow list (reinserted after a rehash)
        const u64 i = atomicAdd((unsigned long long*)&a.st->n_overflow, 1ull);
        if (i < T.ovf_cap) {
            Overflow o;
            o.key = key;
            o.count = cnt;
            o.first = ord;
            o.tag = a.file_tag;
            o.pad = 0;
            T.ovf[i] = o;
        } else {
            atomicOr(&a.st->cap_flags, 2u);
        }
        return;
    }
    GSlot* sl = &T.slots[r.slot];
    if (ABLATE & 128u) {  // timing ablation: plain stores instead of atomics (wrong counts)
        sl->count = cnt;
        return;
    }
    atomicAdd((unsigned long long*)&sl->count, (unsigned long long)cnt);
    if (ord < r.first) atomicMin((unsigned long long*)&sl->first, (unsigned long long)ord);
    if (r.tag < a.file_tag) atomicMax(&sl->last_tag, a.file_tag);
}

struct Geom {  // the launch's chunk geometry (ScanArgs' normal or heavy set, chosen at the kernel start)
    u32 chunk_tiles, mid_chunks, num_chunks, down_g;
};
// After a chunk's commit (one lane): the launch's last commit decides the next launch's geometry
// from the device's own counters (no host snapshot): heavy when at least a quarter of the chunks
// since the reset sent their commits to the launch log.  Exotic-only replays leave it alone.
__device__ __forceinline__ void note_commit(const ScanArgs& a, const Geom& g, bool hv) {
    if (a.exo_only) return;
    // relaxed: the decision is a performance heuristic (a stale log_commits only delays a switch), and
    // a release here would write back the XCD's L2 once per chunk (MI355X_MICROARCH.md fence table)
    const u32 prev = __hip_atomic_fetch_add(&a.st->commits_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev != g.num_chunks - 1u) return;
    const u64 tot = __hip_atomic_load(&a.st->chunks_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + g.num_chunks;
    const u64 lc = __hip_atomic_load(&a.st->log_commits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&a.st->chunks_total, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&a.st->heavy[a.par ^ 1u], (lc && lc * 4 >= tot) ? 1u : 0u, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    if (hv) __hip_atomic_fetch_add(&a.st->heavy_launches, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&a.st->commits_done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// publish the LDS table and the cold list / buffered side effects into HBM (all threads): resolve
// every entry's slot, then add (resolve_batch / apply_entry), or append them to the launch log.
__device__ __attribute__((noinline)) void commit_buffers(ScanShared& sh, const ScanArgs& a, int tid, const Geom& g,
                                                        bool hv) {
#if defined(FR_STAMPS) && FR_STAMPS == 2
    u64 cst_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    u64 cq_ = __builtin_amdgcn_s_memtime();
#endif
    __syncthreads();
    FR_CSTAMP(0);
    u32 made = 0;
    if (ABLATE & 64u) {  // diag: flushed LDS slots and cold entries per commit
        u32 live = 0;
        for (int i = tid; i < NS; i += WG) live += sh.ls[i].key != 0;
        if (live) atomicAdd((unsigned long long*)&a.st->stamp[4], (unsigned long long)live);
        if (tid == 0) atomicAdd((unsigned long long*)&a.st->stamp[5], (unsigned long long)min(sh.ncold, a.cold_cap));
        if (tid == 0) atomicAdd((unsigned long long*)&a.st->stamp[6], 1ull);
    }
    const bool flush = !(ABLATE & 8u);  // ablation 8: no HBM flush of the LDS table / cold list
    const u64 cb = sh.cbase;  // LDS offsets are chunk offsets
    const u32 nc = flush ? min(sh.ncold, a.cold_cap) : 0u;
    const u32 nl = flush ? sh.nkeys : 0u;  // claimed LDS slots = the live ones
    // heavy commits (at least log_min pairs: many distinct codes per chunk) go to the launch log,
    // aggregated after the launch; lighter ones insert straight into the table
    bool logged = false;
    const u64* cl = a.cold + 2ull * (u64)blockIdx.x * a.cold_cap;
    // LDS scratch of the logged commit (the walks are done): per-part run counters
    u32* rcnt = &sh.raw[0][0];
    u32* rcur = rcnt + LOG_NSUB;
    u32* rbase = rcur + LOG_NSUB;  // each run's start in its part of the log
    static_assert(3 * LOG_NSUB * 4 <= sizeof(sh.raw), "log part scratch");
    u32* bcur = a.st->log_scur;  // the parts' cursors
    constexpr int CB = 8;  // cold entries per lane with their loads in flight together
    // a logged commit sends its hot codes (chunk count >= log_hot: few per chunk, their slots L2-warm)
    // straight to the table; the tail goes to the log, one run per part
    if (a.log && nl + nc && nl + nc >= a.log_min) {
        for (int i = tid; i < LOG_NSUB; i += WG) rcnt[i] = rcur[i] = 0;
        __syncthreads();
        for (int i = tid; i < NS; i += WG) {
            const LSlot e = sh.ls[i];
            if (e.key && e.cnt < a.log_hot) atomicAdd(&rcnt[log_bucket(e.key)], 1u);
        }
        for (u32 i0 = tid; i0 < nc; i0 += CB * WG) {
            u64 k[CB];
#pragma unroll
            for (int q = 0; q < CB; ++q) k[q] = i0 + q * WG < nc ? cl[2 * (i0 + q * WG)] : 0ull;
#pragma unroll
            for (int q = 0; q < CB; ++q)
                if (i0 + q * WG < nc) atomicAdd(&rcnt[log_bucket(k[q])], 1u);
        }
        if (tid == 0) sh.log_on = 0;
        __syncthreads();
        FR_CSTAMP(1);
        {  // one claim per part with a run, all in flight together
            constexpr int PR = (LOG_NSUB + WG - 1) / WG;
            u32 n[PR], base[PR], tot = 0;
#pragma unroll
            for (int j = 0; j < PR; ++j) {
                const int r = tid + j * WG;
                n[j] = r < LOG_NSUB ? rcnt[r] : 0u;
                tot += n[j];
            }
#pragma unroll
            for (int j = 0; j < PR; ++j) base[j] = n[j] ? atomicAdd(&bcur[tid + j * WG], n[j]) : 0u;
#pragma unroll
            for (int j = 0; j < PR; ++j)
                if (tid + j * WG < LOG_NSUB) rbase[tid + j * WG] = base[j];
            if (tot) atomicAdd(&sh.log_on, tot);
        }
        __syncthreads();
        FR_CSTAMP(2);
        if (tid == 0 && sh.log_on) {
            atomicAdd((unsigned long long*)&a.st->log_n, (unsigned long long)sh.log_on);
            atomicAdd((unsigned long long*)&a.st->log_commits, 1ull);
        }
        logged = sh.log_on != 0;  // else (nothing but hot codes) every pair inserts directly
    } else if (!a.log && !a.exo_only && tid == 0 && nl + nc && nl + nc >= a.log_min) {
        // a launch without a log (fr_tuning log = 0): count the commit that would have logged (note_commit's
        // heavy-geometry decision sees it)
        atomicAdd((unsigned long long*)&a.st->log_commits, 1ull);
    }
    if (logged) {
        constexpr int CL = NS / WG;
        const u64 ord0 = make_ord(a, 0);
        // a pair past its part's end inserts directly (the part's claimed range up to its end is
        // always written: the aggregation reads min(cursor, log_scap) entries)
        auto put = [&](u64 k, u64 off, u32 cnt) {
            const u32 r = log_bucket(k);
            const u64 pos = (u64)rbase[r] + atomicAdd(&rcur[r], 1u);
            const bool fits = cnt <= LOG_CNT_MAX;  // (a chunk holds fewer records unless its geometry is extreme)
            if (pos < a.log_scap) a.log[(u64)r * a.log_scap + pos] = fits ? LogEntry{k, log_pack(off, cnt)} : LogEntry{0, 0};
            if (pos >= a.log_scap || !fits) {  // (a zero key is skipped by the aggregation)
                const u64 k1[1] = {k};
                const bool v1[1] = {true};
                Resolved r1[1];
                made += resolve_batch<1>(a, k1, v1, r1);
                apply_entry(a, r1[0], k, cnt, make_ord(a, off));  // (off: a launch offset, or a multiple of 4 past ord0)
            }
        };
        u64 hk[CL];
        bool hv[CL];
#pragma unroll
        for (int b = 0; b < CL; ++b) {
            const LSlot e = sh.ls[tid + b * WG];
            hv[b] = e.key && e.cnt >= a.log_hot;
            hk[b] = e.key;
            if (e.key && !hv[b]) put(e.key, cb + e.mino, e.cnt);  // launch offsets (a logged range may exceed 4 GiB)
        }
        for (u32 i0 = tid; i0 < nc; i0 += CB * WG) {
            u64 k[CB], o[CB];
#pragma unroll
            for (int q = 0; q < CB; ++q) {
                const u32 i = i0 + q * WG;
                k[q] = i < nc ? cl[2 * i] : 0ull;
                o[q] = i < nc ? cl[2 * i + 1] : 0ull;
            }
#pragma unroll
            for (int q = 0; q < CB; ++q)
                if (i0 + q * WG < nc) put(k[q], o[q] - ord0, 1u);
        }
        Resolved rh[CL];
        made += resolve_batch<CL>(a, hk, hv, rh);
#pragma unroll
        for (int b = 0; b < CL; ++b) {
            if (!hv[b]) continue;
            const LSlot e = sh.ls[tid + b * WG];
            apply_entry(a, rh[b], e.key, e.cnt, make_ord(a, cb + e.mino));
        }
    } else if (flush) {
        constexpr int CL = NS / WG;  // LDS slots per lane; also cold entries per lane per batch
        Resolved* park = (Resolved*)&sh.raw[0][0];  // the walks are done: the tile area holds NS resolutions
        static_assert(sizeof(Resolved) * NS <= sizeof(sh.raw), "resolution parking");
        // the first cold batch's HBM reads lead: they land while the LDS slots resolve
        u64 ck[CL], co[CL];
        bool cv[CL];
#pragma unroll
        for (int b = 0; b < CL; ++b) {
            const u32 i = tid + b * WG;
            cv[b] = i < nc;
            ck[b] = cv[b] ? cl[2 * i] : 0;
            co[b] = cv[b] ? cl[2 * i + 1] : 0;
        }
        Resolved rc[CL];
        {
            u64 lk[CL];
            bool lv[CL];
            Resolved rs[CL];
#pragma unroll
            for (int b = 0; b < CL; ++b) {
                lk[b] = sh.ls[tid + b * WG].key;
                lv[b] = lk[b] != 0;
            }
            made += resolve_batch<CL>(a, lk, lv, rs);
#pragma unroll
            for (int b = 0; b < CL; ++b) park[tid + b * WG] = rs[b];
        }
        FR_CSTAMP(1);
        made += resolve_batch<CL>(a, ck, cv, rc);
        FR_CSTAMP(2);
        // every slot is known: the updates, none waited for
#pragma unroll
        for (int b = 0; b < CL; ++b) {
            const LSlot e = sh.ls[tid + b * WG];
            if (e.key) apply_entry(a, park[tid + b * WG], e.key, e.cnt, make_ord(a, cb + e.mino));
        }
#pragma unroll
        for (int b = 0; b < CL; ++b)
            if (cv[b]) apply_entry(a, rc[b], ck[b], 1u, co[b]);
        // a cold list of more than NS entries: further batches, each resolved, then applied
        for (u32 c0 = CL * WG; c0 < nc; c0 += CL * WG) {
#pragma unroll
            for (int b = 0; b < CL; ++b) {
                const u32 i = c0 + tid + b * WG;
                cv[b] = i < nc;
                ck[b] = cv[b] ? cl[2 * i] : 0;
                co[b] = cv[b] ? cl[2 * i + 1] : 0;
            }
            made += resolve_batch<CL>(a, ck, cv, rc);
#pragma unroll
            for (int b = 0; b < CL; ++b)
                if (cv[b]) apply_entry(a, rc[b], ck[b], 1u, co[b]);
        }
    }
    if (made) atomicAdd(&sh.created, made);
    // buffered exotic records and the first "no space" error
    const u32 ne = min(sh.nexo, (u32)EXO_BUF);
    for (u32 k = tid; k < ne; k += WG) {
        const u64 n = sh.exo_len[k];
        const u64 i = atomicAdd((unsigned long long*)&a.st->n_exotic, 1ull);
        const u64 po = atomicAdd((unsigned long long*)&a.st->exo_pool_used, (unsigned long long)n);
        if (i < a.tabv.exo_cap && po + n <= a.tabv.exo_pool_cap) {
            a.tabv.exo_ord[i] = make_ord(a, cb + sh.exo_p[k]);
            a.tabv.exo_off[i] = po;
            a.tabv.exo_len[i] = (u32)n;
            for (u64 q = 0; q < n; ++q) a.tabv.exo_pool[po + q] = a.buf[cb + sh.exo_start[k] + q];
        } else {
            atomicOr(&a.st->cap_flags, 4u);
        }
    }
    if (tid == 0 && sh.err_off != 0xFFFFFFFFu)
        atomicMin((unsigned long long*)&a.st->err_nospace, (unsigned long long)(a.file_offset + cb + sh.err_off));
    // (in here, not in the chunk loop: lane-divergent code at the loop's end made the structurizer move
    // it out of the loop, past the ticket barrier, for one lane)
    if (tid == 0) note_commit(a, g, hv);
    FR_CSTAMP(3);
    // LDS-only barriers from here: the commit's count atomics, log entries and exotic bytes stay in
    // flight (no later read in this launch needs them), while the LDS table is reset for the next chunk
    lds_barrier();
    FR_CSTAMP(4);
    for (int i = tid; i < NS; i += WG) sh.ls[i] = LSlot{0, 0, 0xFFFFFFFFu};
    if (tid == 0) {
        sh.nkeys = 0;
        sh.ncold = 0;
        sh.nexo = 0;
        sh.err_off = 0xFFFFFFFFu;
        sh.spec_bad = 0;
    }
    lds_barrier();
#if defined(FR_STAMPS) && FR_STAMPS == 2
    FR_CSTAMP(5);
    cst_[6] = nl;
    cst_[7] = nc;
    if ((tid & 63) == 0)
        for (int i_ = 0; i_ < 8; ++i_) atomicAdd((unsigned long long*)&a.st->stamp[i_], (unsigned long long)cst_[i_]);
#endif
}

// drop everything buffered (a redone chunk)
__device__ __forceinline__ void discard_buffers(ScanShared& sh, int tid) {
    __syncthreads();
    for (int i = tid; i < NS; i += WG) sh.ls[i] = LSlot{0, 0, 0xFFFFFFFFu};
    if (tid == 0) {
        sh.nkeys = 0;
        sh.ncold = 0;
        sh.nexo = 0;
        sh.err_off = 0xFFFFFFFFu;
        sh.spec_bad = 0;
    }
    __syncthreads();
}

__device__ __forceinline__ bool uniform_flag(u32 v) { return __builtin_amdgcn_readfirstlane(v) != 0; }

// code bytes at [start, start + n) of the wave's LDS copy -> fast key with v_perm SWAR, 4 bytes per
// step (false if outside the fast alphabet).  Byte index i = (c >> 1) & 7 selects the expected
// byte (A C T G - + - N) and its symbol (A1 C2 G3 T4 N5 +6); a byte is valid iff it equals the
// expected one.  Eight dwords from start & ~3 (bytes past the tile read the next area; masked off).
__device__ __forceinline__ void encode_load_lds(const ScanShared& sh, u32 wid, u32 start, u32 (&w)[8]) {
    const lds_u32* p = (const lds_u32*)(&sh.raw[wid][0]) + (start >> 2);
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = p[k];
}

__device__ __forceinline__ bool encode_pack(const u32 (&w)[8], u32 start, u32 n, u64& key) {
    if (n < 1 || n > (u32)MAXSYM) return false;
    const u32 sh = start & 3u;
    u64 kk = 0;
    u32 bad = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const u32 x = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh);  // code bytes 4k .. 4k+3
        const u32 idx = (x >> 1) & 0x07070707u;
        const u32 expect = __builtin_amdgcn_perm(0x4E002B00u, 0x47544341u, idx);
        const u32 sym = __builtin_amdgcn_perm(0x05000600u, 0x03040201u, idx);
        const int left = (int)n - 4 * k;  // bytes of the code in this word
        const u32 vm = left >= 4 ? 0xFFFFFFFFu : left <= 0 ? 0u : (0xFFFFFFFFu >> (32 - 8 * left));
        bad |= (expect ^ x) & vm;
        const u32 sv = sym & vm;
        const u32 packed = __builtin_amdgcn_udot4(sv, 0x00400801u, (sv >> 15) & 0xE00u, false);
        kk |= (u64)packed << (12 * k);
    }
    key = kk;
    return bad == 0;
}

// the rare header outcomes (chunk offsets): word-scan fallback, no ' ' (IndexError), or an exotic code
__device__ FR_COLD void slow_header(ScanShared& sh, const ScanArgs& a, u32 p, int r, u32 start, u32 n) {
    if (r == 2) process_header_global(sh, a, p);
    else if (r == 1) nospace(a, p, sh);
    else exotic_record(a, p, sh.cbase + start, n, sh);
}

// ---- header parse: two 64-bit bitmap windows, wave-uniform code length encode ---------------
// v_ffbl / v_ffbh return ~0 for 0, which the min tricks below rely on; the builtins add a
// compare and select per word (or make the zero case undefined).
__device__ __forceinline__ u32 ffbl32(u32 x) {
    u32 r;
    asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}
__device__ __forceinline__ u32 ffbh32(u32 x) {
    u32 r;
    asm("v_ffbh_u32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}
__device__ __forceinline__ u32 ctz64x(u64 x) { return min(ffbl32((u32)x), ffbl32((u32)(x >> 32)) | 32u); }  // ~0: none
// index of the highest set bit; negative (-64) when none
__device__ __forceinline__ int hsb64x(u64 x) { return (int)(min(ffbh32((u32)(x >> 32)), ffbh32((u32)x) | 32u) ^ 63u); }

// bits [b, b + 64) of the 128-bit (x0, x1), b in [0, 63]
__device__ __forceinline__ u64 window64(u64 x0, u64 x1, u32 b) { return (x0 >> b) | ((x1 << 1) << (63u - b)); }

// R2 on the wave-tile's bitmaps in two 64-bit windows: from the line start p the first ' ' or line
// end f1 (a line end first: no ' ', IndexError); from the token start q = f1 + 1 the token end f2
// and the last ':' before it.  0: code at [start, start + n) (tile offsets); 1: no ' '; 2: word-scan
// fallback (the first ' ' or the token end lies 64 or more bytes on, or the token starts past the
// staged bytes).
__device__ __forceinline__ int locate_code(const ScanShared& sh, u32 wid, u32 p, u32 bl, u32& start, u32& n) {
    // One LDS round for both windows: the token start q < p + 64 lies in word w or w + 1, so words w .. w + 2
    // hold everything either window reads (the loads go out together, before any branch; w <= 63 keeps
    // w + 2 inside the SEGS + 2 words).  Round 4 read the second window's words after the first window's
    // test: two dependent LDS round trips per header, each a bitmap pair at a time (four waits).
    const u32 w = min(p >> 6, (u32)SEGS - 1u), b = p & 63u;
    const lds_u64* S = (const lds_u64*)&sh.bsp[wid][w];
    const lds_u64* E = (const lds_u64*)&sh.beol[wid][w];
    const lds_u64* C = (const lds_u64*)&sh.bcol[wid][w];
    u64 s0 = S[0], s1 = S[1], s2 = S[2], e0 = E[0], e1 = E[1], c0 = C[0], c1 = C[1], c2 = C[2];
    // all eight in registers here: the compiler would otherwise sink each load into the branch that uses
    // it (one wait per load again)
    asm volatile("" : "+v"(s0), "+v"(s1), "+v"(s2), "+v"(e0), "+v"(e1), "+v"(c0), "+v"(c1), "+v"(c2));
    if (p >= bl) return 2;
    const u64 se = window64(s0, s1, b);
    const u64 eo = window64(e0, e1, b);
    const u32 f1 = ctz64x(se);
    const u32 q = p + f1 + 1u;
    if (f1 >= 64u) return 2;
    if (ctz64x(eo) == f1) return 1;
    if (q >= bl) return 2;
    const bool nxt = (q >> 6) != w;  // the token starts in word w + 1
    const u32 b2 = q & 63u;
    const u64 se2 = window64(nxt ? s1 : s0, nxt ? s2 : s1, b2);
    const u64 co2 = window64(nxt ? c1 : c0, nxt ? c2 : c1, b2);
    const u32 f2 = ctz64x(se2);
    if (f2 >= 64u) return 2;
    const int hc = hsb64x(co2 & ((1ull << f2) - 1ull));  // the last ':' of the token, < 0 none
    const u32 cs = (u32)max(hc + 1, 0);
    start = q + cs;
    n = f2 - cs;
    return 0;
}

// code bytes [start, start + n) from the wave's LDS copy -> fast key, n wave-uniform (nu): the
// per-word byte masks are scalars and only the words the code reaches are packed
__device__ __forceinline__ bool encode_uniform(const ScanShared& sh, u32 wid, u32 start, u32 nu, u64& key) {
    u32 w[8];
    encode_load_lds(sh, wid, start, w);
    const u32 al = start & 3u;
    u32 bad = 0, lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if ((u32)(4 * k) >= nu) break;  // uniform
        const u32 x = __builtin_amdgcn_alignbyte(w[k + 1], w[k], al);
        const u32 idx = (x >> 1) & 0x07070707u;
        const u32 expect = __builtin_amdgcn_perm(0x4E002B00u, 0x47544341u, idx);
        const u32 sym = __builtin_amdgcn_perm(0x05000600u, 0x03040201u, idx);
        const u32 left = nu - 4u * k;
        // each arm computes packed itself (a sym masked in one arm only made the compiler copy it in the other)
        u32 packed;
        if (left >= 4u) {
            bad = __builtin_amdgcn_bitop3_b32(expect, x, bad, 0xBEu);  // (expect ^ x) | bad in one op
            packed = __builtin_amdgcn_udot4(sym, 0x00400801u, (sym >> 15) & 0xE00u, false);
        } else {
            const u32 vm = 0xFFFFFFFFu >> (32u - 8u * left);  // uniform
            bad |= (expect ^ x) & vm;
            const u32 sv = sym & vm;
            // no fourth byte, so no term from above the dot4's 8-bit weights; a single byte is its own symbol
            packed = left == 1u ? sv : __builtin_amdgcn_udot4(sv, 0x00400801u, 0u, false);
        }
        if (k == 0) lo = packed;
        else if (k == 1) lo |= packed << 12;
        else if (k == 2) { lo |= packed << 24; hi = packed >> 8; }
        else hi |= packed << (12 * k - 32);
    }
    key = ((u64)hi << 32) | lo;
    return bad == 0;
}

// R2 from the line start p in ONE window of the ' ' | line-end bitmap and one of the ':' bitmap (round 6):
// f1 = the first ' ' or line end, the token end = the next one (the window's second set bit), the code
// start = one past the last ':' before the token end, or the token start when the token has none.  The
// byte at f1 tells a ' ' from a line end (IndexError), read from the wave's tile copy with the code.
// Branch-free: 0 code at [start, start + n) (tile offsets); 2 word-scan fallback (the line starts past the
// staged bytes, or no ' ' / line end within 64 bytes); 3 the token ends past the window (a first token of
// 40-odd bytes: Illumina instrument headers), which locate_code finishes from the token start.
__device__ __forceinline__ int locate_near(const ScanShared& sh, u32 wid, u32 p, u32 bl, u32& start, u32& n, u32& f1) {
    // p <= TILE (a segment's last byte ends the line before it), so word w <= SEGS and w + 1 lie inside the
    // SEGS + 2 words without a clamp; p == TILE is past the staged bytes and returns 2 whatever the window holds
    const u32 w = p >> 6, b = p & 63u;
    const lds_u64* S = (const lds_u64*)&sh.bsp[wid][w];
    const lds_u64* C = (const lds_u64*)&sh.bcol[wid][w];
    u64 s0 = S[0], s1 = S[1], c0 = C[0], c1 = C[1];
    asm volatile("" : "+v"(s0), "+v"(s1), "+v"(c0), "+v"(c1));  // one LDS round, before any use
    const u64 se = window64(s0, s1, b);
    const u64 co = window64(c0, c1, b);
    const u64 se1 = se & (se - 1ull);
    f1 = ctz64x(se);
    const u32 f2 = ctz64x(se1);
    const int hc = hsb64x(co & ((1ull << (f2 & 63u)) - 1ull));  // the last ':' before the token end (< 0: none)
    const u32 cs = (u32)max(hc, (int)f1) + 1u;                  // a ':' of the first token does not count
    start = p + cs;
    n = f2 - cs;
    return (p >= bl || se == 0ull) ? 2 : (se1 == 0ull ? 3 : 0);
}

__device__ __forceinline__ void parse_header(ScanShared& sh, const ScanArgs& a, u32 wid, u32 tile0, u32 p, u32 bl,
                                             const ColdDest& cd, ColdPend& pd) {
    u32 start = 0, n = 0, f1 = 0;
    int r = locate_near(sh, wid, p, bl, start, n, f1);
    if (__builtin_expect(__ballot(r == 3) != 0, 0)) {  // uniform: some lane's token ends past its first window
        if (r == 3) {
            r = locate_code(sh, wid, p, bl, start, n);  // decides "no ' '" itself
            f1 = 0xFFFFFFFFu;
        }
    }
    // the first delimiter's byte (in the staged bytes whenever r == 0 and f1 < 64): not a ' ' -> a line end
    const u32 dch = *((const lds_u8*)&sh.raw[wid][0] + min(p + f1, (u32)TILE - 1u));
    if (ABLATE & 2u) {
        asm volatile("" ::"v"(start), "v"(n), "v"(r), "v"(dch));
        return;
    }
    u64 key = 0;
    bool fast = false;
    if (r == 0 && n >= 1u && n <= (u32)MAXSYM) {
        const u32 nu = __builtin_amdgcn_readfirstlane(n);
        if (__ballot(n != nu) == 0) {
            fast = encode_uniform(sh, wid, start, nu, key);  // the common case
        } else {
            u32 w[8];
            encode_load_lds(sh, wid, start, w);
            fast = encode_pack(w, start, n, key);
        }
    }
    if (r == 0 && f1 < 64u && dch != (u32)' ') {  // the line ends before any ' ': IndexError (:169)
        r = 1;
        fast = false;
    }
    if (fast) count_code(sh, a, tile0 + p, key, &cd, &pd);
    else rare_push(sh, a, tile0 + p, (u32)r, tile0 + start, n);
}

// The line starts after every 4th terminator (lines == 0 mod 4) in this lane's segment, parsed
// where they lie.  L0 = lines before the wave-tile (absolute with -s, else mod 4 suffices).  The
// first header needs the skip-th set bit of the terminator mask; a second one in the same segment
// (records shorter than 64 B) takes the loop at the end.
template <bool LIM>
__device__ __forceinline__ void parse_own_headers(ScanShared& sh, const ScanArgs& a, u32 t, u32 ct,
                                                  const SegClass& sc, u64 L0, int lane, u32 wid, const ColdDest& cd,
                                                  ColdPend& pd) {
    const u64 tile0 = (u64)t * TSTEP;
    const u32 tile0c = (t - ct) * TSTEP;  // the tile's chunk offset (ct: the chunk's first tile)
    const u32 bl = (u32)min((u64)TILE, a.avail - tile0);
    const u64 rem64 = a.len - tile0;  // line starts p < pend are this launch's (uniform)
    const u32 pend = rem64 >= 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)rem64 + ((a.own_end && a.len < a.avail) ? 1u : 0u);
    const u32 lb = (u32)L0 + (sc.x - sc.c);  // terminators before this segment (low bits)
    const u32 skip = (3u - lb) & 3u;
    const u32 s0 = lane * SEG;
    // The skip-th terminator of the segment (skip <= 3), in 32 bits: the half that holds it follows from the low
    // half's popcount (sc.c's first v_bcnt), then up to three lowest bits of that half are cleared, each by one
    // compare, one subtract with borrow and one AND.  (It was three rounds on the 64-bit mask: a 64-bit add, a
    // compare, two selects and two ANDs each, then a 64-bit ctz, a 64-bit test and a 64-bit popcount.)
    const u32 tlo = (u32)sc.tmask, thi = (u32)(sc.tmask >> 32);
    const u32 clo = __popc(tlo);
    const bool in_lo = skip < clo;
    u32 hx = in_lo ? tlo : thi;
    const u32 hk = in_lo ? skip : skip - clo;
#pragma unroll
    for (u32 q = 0; q < 3; ++q) hx &= hx - (q < hk ? 1u : 0u);
    const bool have = sc.c > skip;              // the segment holds a header terminator
    const u32 hpos = ffbl32(hx) + (in_lo ? 0u : 32u);  // its bit (have)
    constexpr bool limited = LIM;  // -s (a.max_records > 0): the kernel instance's, so the common one has no record limit
    u64 rec = 0;
    if (limited) rec = (L0 + (sc.x - sc.c) + skip + 1u) >> 2;
    // the range's own first line start (position 0): lane 0 of the range's first tile; the rest is wave-uniform
    const bool own0s = t == 0 && a.own_start && (L0 & 3ull) == 0 && a.avail > 0 &&
                       (!limited || (i64)(L0 >> 2) < a.max_records);
    const bool own0 = own0s && lane == 0;
    // the first header terminator.  own0's header at position 0 comes first.
    const u32 p = own0 ? 0u : s0 + hpos + 1u;
    const bool ok = own0 || (have && p < pend && (!limited || (i64)rec < a.max_records));
    if (ok) parse_header(sh, a, wid, tile0c, p, bl, cd, pd);
    // another header in this segment (records shorter than 64 B; never at R=8's 74 B): uniform check
    bool more = ok && (own0 ? have : sc.c > skip + 4u);
    if (__builtin_expect(!__ballot(more), 1)) return;
    // the terminator mask from the first header terminator on (in 64 bits, for the loop below)
    u64 m = sc.tmask;
#pragma unroll
    for (u32 q = 0; q < 3; ++q) {
        const u64 d = m & (m - 1ull);
        m = q < skip ? d : m;
    }
    if (!own0) {
        m &= m - 1ull;
        m &= m - 1ull;
        m &= m - 1ull;
        m &= m - 1ull;
        ++rec;
    }
    while (__ballot(more)) {
        if (more) {
            const u32 pn = s0 + ctz64x(m) + 1u;
            more = pn < pend && (!limited || (i64)rec < a.max_records);
            if (more) parse_header(sh, a, wid, tile0c, pn, bl, cd, pd);
            ++rec;
            m &= m - 1ull;
            m &= m - 1ull;
            m &= m - 1ull;
            m &= m - 1ull;
            more = more && m != 0;
        }
    }
}

// One wave walks wave-tiles [tb, te) of the range; L0 = lines before tile tb (absolute, or only
// mod 4 without -s).  parse = false: count only.  Returns the line terminators in [tb, te).  No
// workgroup barrier: every LDS area the walk writes is this wave's.  Per step: the tile's bytes
// (in registers since the previous step) go to the wave's LDS copy first, so the registers take the
// next tile's loads at once and those stay in flight through this tile's classify AND its parse;
// the classify reads the lane's segment back from LDS.  A lane's LDS-table miss of tile t waits in registers (pd)
// and is stored to the cold list at the top of step t + 1, ahead of that step's loads, or after the loop.
// The loop's rare branches (seg_load_tail, classes_exact, the '\r' re-read, drain_rare, locate_code, a second header
// in a segment) are marked unlikely: the out-of-line calls among them clobber every caller-saved SGPR, and with
// the branches weighted evenly the register allocator kept the walk's uniforms (the buffer descriptor, ColdDest,
// te, ct, the range-end flags) in spill lanes and reloaded them with v_readlane / v_writelane on the path every
// tile takes; now the saves and reloads sit in the rare blocks, around the calls.
template <bool LIM>
__device__ __forceinline__ u64 walk_wave(ScanShared& sh, const ScanArgs& a0, u32 ct, u32 tb, u32 te, u64 L0,
                                         bool parse, int lane, u32 wid) {
    const ScanArgs& a = a0;
    u64 lines = 0;
    u32 done = *(const volatile lds_u32*)&sh.rq_tail[wid];
    SegRegs r;
    if (tb < te) seg_load(a, tb, r, lane);
    lds_u32x4* mine = (lds_u32x4*)(&sh.raw[wid][0]) + lane * (SEG / 16);
    const ColdDest cd = cold_dest(sh, a);  // once per walk
    ColdPend pd = {0ull, COLD_NONE};
    FR_WSTAMP_DECL
    for (u32 t = tb; t < te; ++t) {
#if defined(FR_STAMPS) && FR_STAMPS == 4
        FR_WSTAMP_RESET();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        FR_WSTAMP(0);
#endif
        // the previous tile's LDS-table misses: their cold-list indices are claimed here, ahead of the copy
        u32 ci;
        const bool cany = cold_flush_claim(sh, pd, ci);
        // the previous tile's parse is done with the LDS copy (program order)
#pragma unroll
        for (int k = 0; k < SEG / 16; ++k) {
            u32x4 v;
            v.x = r.v[k].x; v.y = r.v[k].y; v.z = r.v[k].z; v.w = r.v[k].w;
            mine[k] = v;
        }
        // ... and their stores go out ahead of the next tile's loads: the loop-top wait for those loads then has
        // no younger store to wait for
        cold_flush_store(sh, a, cd, pd, cany, ci);
        if (t + 1 < te) seg_load(a, t + 1, r, lane);
        // volatile: a real LDS read, one quarter of the segment at a time inside the classify
        const SegClass sc = seg_classify_src(a, t, [&](int k) {
            const u32x4 v = *(const volatile lds_u32x4*)&mine[k];
            return make_uint4(v.x, v.y, v.z, v.w);
        }, lane);
        FR_WSTAMP(1);
        if (sc.hi) rare_push(sh, a, (t - ct) * TSTEP + lane * SEG, 4u,
                             min((u32)min((u64)TSTEP, a.len - (u64)t * TSTEP) - lane * SEG, (u32)SEG), 0u);
        const u32 tail = *(const volatile lds_u32*)&sh.rq_tail[wid];
        if (__builtin_expect(tail != done, 0)) {  // uniform: the previous tile's rare events (and this tile's UTF-8 checks)
            drain_rare(sh, a, wid, done, tail, lane);
            done = tail;
        }
        sh.bsp[wid][lane] = sc.sp | sc.eol;  // token ends: ' ' or line end
        sh.bcol[wid][lane] = sc.col;
        sh.beol[wid][lane] = sc.eol;
        lds_fence();
        // (a speculation buffer that overflowed mid-walk, sh.spec_bad, is not checked per tile: the chunk is
        // redone exactly and everything its walk buffered is discarded, so parsing on is harmless; the check
        // was an LDS round trip per tile)
        FR_WSTAMP(2);
        if (parse && !(ABLATE & 1u)) parse_own_headers<LIM>(sh, a, t, ct, sc, L0 + lines, lane, wid, cd, pd);
        lines += sc.wtot;
        FR_WSTAMP(3);
    }
    FR_WSTAMP_FLUSH(te > tb ? te - tb : 0u);
    u32 ci;  // the last tile's misses: everything the walk buffers is in place when it returns
    const bool cany = cold_flush_claim(sh, pd, ci);
    cold_flush_store(sh, a, cd, pd, cany, ci);
    lds_fence();
    const u32 tail = *(const volatile lds_u32*)&sh.rq_tail[wid];
    if (tail != done) drain_rare(sh, a, wid, done, tail, lane);
    return lines;
}

// Tiles [tb, te) of chunk c.  Uniform: chunk_tiles each.  Ramped (ramp_g = G > 0, C = chunk_tiles,
// s = the ramp's smallest chunk): R_s(j) = s j + floor((C-s) j (j+1) / 2G) tiles precede ramp-up
// chunk j, so chunk j holds s + ~(C-s)(j+1)/G tiles and the G first chunks, all taken at once, finish
// in ticket order; mid_chunks full chunks follow; the last Gd = ramp_down_g chunks shrink the same way
// (over Gd chunks, smallest ramp_down_s), so every workgroup runs out of work at about the same time.  fr_api only ramps
// ranges of >= R_up(G) + R_down(G) + C tiles (ramp_prefix in fr_internal.h, shared with the host).
__device__ __forceinline__ u64 ramp_prefix(const Geom& g, u64 G, u64 j, u32 s0) {
    return ramp_tiles_before(g.chunk_tiles, G, s0, j);
}

// Run by the workgroup that finishes the launch's last chunk: the exact line prefix of every chunk
// (exclusive scan of the published counts), checked against the phase each committed speculative
// chunk guessed; writes the range's line total for the next launch.
__device__ __attribute__((noinline)) void verify_launch(ScanShared& sh, const ScanArgs& a, u32 n, u64 base_lines,
                                                       int tid) {
    const u32 per = (n + WG - 1) / WG;
    const u32 lo = min(tid * per, n), hi = min(lo + per, n);
    u64 sum = 0;
    for (u32 c = lo; c < hi; ++c) sum += (u32)agent_load(&a.chunk_info[c]);
    // block exclusive scan of the per-thread sums (the wave counts are free scratch here)
    u64 x = sum;
    const int lane = tid & 63, wid = tid >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) sh.wcount[wid] = x;
    __syncthreads();
    u64 before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const u64 v = sh.wcount[w];
        before += w < wid ? v : 0ull;
        total += v;
    }
    u64 run = base_lines + before + (x - sum);
    bool bad = false;
    for (u32 c = lo; c < hi; ++c) {
        const u64 info = agent_load(&a.chunk_info[c]);
        const u32 f = (u32)(info >> 32);
        if ((f & 1u) && ((f >> 1) & 3u) != (u32)(run & 3ull)) bad = true;
        run += (u32)info;
    }
    if (bad) atomicOr(&a.st->spec_fail, 1u);
    if (tid == 0) a.st->lines[a.par ^ 1u] = base_lines + total;
    __syncthreads();
}

__device__ __forceinline__ void chunk_bounds(const ScanArgs& a, const Geom& g, u32 c, u32& tb, u32& te) {
    if (a.ramp_g == 0) {
        tb = min(c * g.chunk_tiles, a.num_tiles);
        te = min(tb + g.chunk_tiles, a.num_tiles);
        return;
    }
    const u32 su = min(a.ramp_up_s, g.chunk_tiles), sd = min(a.ramp_down_s, g.chunk_tiles);
    const u64 G = a.ramp_g, Gd = g.down_g;
    const u64 rg = ramp_prefix(g, G, G, su), mid_end = (u64)a.num_tiles - ramp_prefix(g, Gd, Gd, sd);
    if (c < G) {
        tb = (u32)ramp_prefix(g, G, c, su);
        te = (u32)ramp_prefix(g, G, c + 1, su);
    } else if (c < G + g.mid_chunks) {
        const u64 b = rg + (u64)(c - G) * g.chunk_tiles;
        tb = (u32)b;
        te = (u32)min(b + g.chunk_tiles, mid_end);
    } else {
        const u64 j = c - G - g.mid_chunks;  // 0 .. Gd-1: shrinking
        tb = (u32)((u64)a.num_tiles - ramp_prefix(g, Gd, Gd - j, sd));
        te = (u32)((u64)a.num_tiles - ramp_prefix(g, Gd, Gd - j - 1, sd));
    }
}

#if defined(FR_STAMPS) && FR_STAMPS == 3  // diagnostic builds only: a timeline of every chunk and workgroup
constexpr u32 TRACE_CHUNKS = 1u << 14;  // per launch parity
constexpr u32 TRACE_WGS = 4096;
__device__ u64 g_chunk_trace[2 * TRACE_CHUNKS * 4];  // per ticket: {wg | xcc << 16 | tiles << 32, ticket, walked, committed}
__device__ u64 g_wg_trace[2 * TRACE_WGS * 2];        // per workgroup: {entry, exit} (s_memrealtime, 100 MHz)
__device__ __forceinline__ u32 xcc_id() {
    u32 x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
    return x & 0xFu;
}
extern "C" int fr_trace_read(u64* chunks, u64* wgs) {
    if (hipMemcpyFromSymbol(chunks, HIP_SYMBOL(g_chunk_trace), sizeof(g_chunk_trace)) != hipSuccess) return 1;
    if (hipMemcpyFromSymbol(wgs, HIP_SYMBOL(g_wg_trace), sizeof(g_wg_trace)) != hipSuccess) return 1;
    return 0;
}
extern "C" int fr_trace_clear() {
    static u64 zero[2 * TRACE_CHUNKS * 4];
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_chunk_trace), zero, sizeof(g_chunk_trace)) != hipSuccess) return 1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_wg_trace), zero, sizeof(g_wg_trace)) != hipSuccess) return 1;
    return 0;
}
#endif

#ifndef FR_OCC
#define FR_OCC 4  // workgroups (= waves per SIMD) per CU: ~39 KB of LDS per workgroup (the wave-tile copies
                  // and the LDS table) fit 4 in a CU's 160 KB; fr_api sizes the grid with chunk_occupancy()
#endif
// LIM: -s (a.max_records > 0), the launch's instance (launch_chunk_scan): the record limit's checks are not in the
// common instance's tile loop
template <bool LIM>
__global__ __launch_bounds__(WG, FR_OCC) void chunk_kernel(ScanArgs args) {
    // every helper reads the arguments where they lie (the kernarg segment): the out-of-line
    // helpers take them by reference without a scratch copy of the struct
    (void)args;
    const ScanArgs& a = *(const ScanArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ ScanShared sh;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const u32 wid = wave_id();  // wave-uniform: LDS addresses by wave stay scalar
    for (int i = tid; i < NS; i += WG) sh.ls[i] = LSlot{0, 0, 0xFFFFFFFFu};
    if (lane == 0) {
        sh.bsp[wid][SEGS] = sh.bsp[wid][SEGS + 1] = 0;
        sh.bcol[wid][SEGS] = sh.bcol[wid][SEGS + 1] = 0;
        sh.beol[wid][SEGS] = sh.beol[wid][SEGS + 1] = 0;
        sh.rq_tail[wid] = 0;
    }
    if (tid == 0) {
        sh.nkeys = 0;
        sh.created = 0;
        sh.flags = 0;
        sh.spec = 0;
        sh.spec_bad = 0;
        sh.ncold = 0;
        sh.nexo = 0;
        sh.err_off = 0xFFFFFFFFu;
        // a feed's fold statistics start at zero: nothing in this launch reads them, the aggregation
        // that updates them runs after it (instead of a memset dispatch ahead of the launch)
        if (a.zero_fold && blockIdx.x == 0) a.st->log_fold_max = a.st->log_fold_over = 0;
    }
#if defined(FR_STAMPS) && FR_STAMPS == 3
    if (tid == 0 && blockIdx.x < TRACE_WGS) g_wg_trace[(a.par * TRACE_WGS + blockIdx.x) * 2] = __builtin_amdgcn_s_memrealtime();
    u64 tl_t0 = 0;
#endif
    const u64 base_lines = a.st->lines[a.par];
    // the geometry: heavy when the previous launch said so (ramped launches that have a heavy set)
    const bool hv = a.num_chunks_h != 0 &&
                    __builtin_amdgcn_readfirstlane(__hip_atomic_load(&a.st->heavy[a.par], __ATOMIC_RELAXED,
                                                                     __HIP_MEMORY_SCOPE_AGENT)) != 0;
    const Geom g = hv ? Geom{a.chunk_tiles_h, a.mid_chunks_h, a.num_chunks_h, a.ramp_down_g_h}
                      : Geom{a.chunk_tiles, a.mid_chunks, a.num_chunks, a.ramp_down_g};
    constexpr bool limited = LIM;
#if defined(FR_STAMPS) && (FR_STAMPS == 1 || FR_STAMPS == 4)
    const u64 k0_ = __builtin_amdgcn_s_memtime();
#endif
    FR_STAMP_DECL
    for (;;) {
        if (tid == 0) {
            // every chunk goes by ticket, the first too: the chunk a look-back waits on is then always
            // held by a workgroup that is already running.  (Round 4 gave each workgroup its own index
            // as its first chunk; a resident workgroup could then wait on a chunk whose workgroup was not
            // dispatched yet -- a grid larger than the free CUs, or another process's kernels holding
            // them -- for a 0.2 % shorter launch head.)
            const u32 cn = atomicAdd(&a.st->ticket, 1u);
            sh.chunk = cn;
            if (cn < g.num_chunks) {  // the chunk's base for its offsets (published by the barrier)
                u32 tb0, te0;
                chunk_bounds(a, g, cn, tb0, te0);
                sh.cbase = (u64)tb0 * TSTEP;
            }
            sh.spec = 1u;  // pass 0 runs on guessed phases: side effects are buffered
        }
        __syncthreads();
        const u32 c = sh.chunk;
        FR_TRACE("w%d ticket %u of %u\n", (int)wid, c, g.num_chunks);
        if (c >= g.num_chunks) break;
        u32 tb, te;
        chunk_bounds(a, g, c, tb, te);
#if defined(FR_STAMPS) && FR_STAMPS == 3
        if (tid == 0) tl_t0 = __builtin_amdgcn_s_memrealtime();
#endif
        const u32 per = (te - tb + NW - 1) / NW;  // this wave's part of the chunk: [wb, we)
        const u32 wb = min(tb + wid * per, te), we = min(wb + per, te);
        // ---- pass 0: chunk 0's first wave starts at the range's exact line count; every other
        // wave guesses its phase (count only when unsure, and with -s or an exotic-only replay) --
        u64 L0 = 0;
        bool parse = false;
        FR_STAMP(3);
        if (wb < we) {
            if (c == 0 && wid == 0) {
                L0 = base_lines;
                parse = true;
            } else if (!limited && !a.exo_only) {
                const int P = guess_phase(sh, a, wb, lane, wid);
                parse = P >= 0;
                L0 = (u64)max(P, 0);
            }
        }
        FR_STAMP(0);
#if defined(FR_STAMPS) && FR_STAMPS == 1
        st_[7] += 1;
#endif
        // One walk site, several passes.  Pass 0 as above.  Then each wave's start follows from the
        // chunk start and the earlier waves' pass-0 counts: a wave that parsed on another phase (or a
        // buffer that overflowed) makes every wave redo; a wave that only counted walks again.  The
        // chunk start is exact (chunk 0, or a decoupled look-back) or, for a device feed, the first
        // wave's guess, committed at once (verify_launch checks it); a speculation buffer that
        // overflows on a guessed start sends the chunk to the look-back and an exact redo.
        bool run = wb < we, exact = true, force = false;
        u64 base = base_lines;
        for (int pass = 0;; ++pass) {
            FR_TRACE("w%d pass %d run %d [%u,%u) parse %d\n", (int)wid, pass, (int)run, wb, we, (int)parse);
            const u64 n = run ? walk_wave<LIM>(sh, a, tb, wb, we, L0, parse, lane, wid) : 0ull;
            FR_TRACE("w%d walked %llu\n", (int)wid, (unsigned long long)n);
            FR_STAMP(pass == 0 ? 1 : 4);
            if (pass == 0) {
                if (lane == 0) {
                    sh.wcount[wid] = n;
                    sh.wphase[wid] = run && parse ? (int)(L0 & 3ull) : -1;
                }
                __syncthreads();
                FR_STAMP(2);
                u64 total = 0;
#pragma unroll
                for (int w = 0; w < NW; ++w) total += sh.wcount[w];
                const int p0 = sh.wphase[0];
                const bool fast = a.spec_commit && c != 0 && p0 >= 0 && !uniform_flag(sh.spec_bad);
                if (tid == 0) {  // publish the chunk's line count
                    agent_store(&a.tiles[c], ((u64)(2u * a.epoch + (c == 0 ? 1u : 0u)) << 32) | (u32)total);
                    const u32 f = fast ? (1u | ((u32)p0 << 1)) : 0u;
                    agent_store(&a.chunk_info[c], ((u64)f << 32) | (u32)total);
                    // the sc1 (agent) stores drain before the count that signals them; verify_launch reads
                    // chunk_info with sc1 loads only (MI355X_MICROARCH.md, valid hand-off forms): no
                    // release fence, which would write back the XCD's L2 once per chunk
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    const u32 prev = __hip_atomic_fetch_add(&a.st->chunks_done, 1u, __ATOMIC_RELAXED,
                                                            __HIP_MEMORY_SCOPE_AGENT);
                    sh.last = prev == g.num_chunks - 1u;
                }
                exact = !fast;
                if (fast) {
                    base = (u64)p0;
                } else if (c != 0) {
                    if (wid == 0) {
                        const u64 ex = lookback(a, c, (u32)total, lane);
                        if (lane == 0) sh.tile_excl = ex;
                    }
                    __syncthreads();
                    base = base_lines + sh.tile_excl;
                }
            } else {
                __syncthreads();
                if (exact || !uniform_flag(sh.spec_bad)) break;
                // a speculation buffer overflowed on the guessed chunk start: look back, redo exactly
                u64 total = 0;
#pragma unroll
                for (int w = 0; w < NW; ++w) total += sh.wcount[w];
                if (wid == 0) {
                    const u64 ex = lookback(a, c, (u32)total, lane);
                    if (lane == 0) sh.tile_excl = ex;
                }
                __syncthreads();
                base = base_lines + sh.tile_excl;
                exact = true;
                force = true;
            }
            // plan the next pass from the pass-0 counts and phases (LDS: nothing held across the walk)
            u64 D = base;
            bool bad = force || uniform_flag(sh.spec_bad);
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const int pw = sh.wphase[w];
                if (w == (int)wid) L0 = D;
                if (pw >= 0 && (u64)pw != (D & 3ull)) bad = true;
                D += sh.wcount[w];
            }
            run = wb < we && (bad || sh.wphase[wid] < 0);
            parse = true;
            if (bad) discard_buffers(sh, tid);
            if (tid == 0) sh.spec = exact ? 0u : 1u;
            __syncthreads();
        }
        FR_TRACE("w%d commit\n", (int)wid);
        FR_STAMP(3);
#if defined(FR_STAMPS) && FR_STAMPS == 3
        const u64 tl_t1 = __builtin_amdgcn_s_memrealtime();
#endif
        commit_buffers(sh, a, tid, g, hv);  // starts and ends with a barrier: sh.last is visible
#if defined(FR_STAMPS) && FR_STAMPS == 3
        if (tid == 0 && c < TRACE_CHUNKS) {
            u64* e = &g_chunk_trace[(a.par * TRACE_CHUNKS + c) * 4];
            e[0] = (u64)blockIdx.x | ((u64)xcc_id() << 16) | ((u64)(te - tb) << 32);
            e[1] = tl_t0;
            e[2] = tl_t1;
            e[3] = __builtin_amdgcn_s_memrealtime();
        }
#endif
        FR_TRACE("w%d committed last %u\n", (int)wid, sh.last);
        if (sh.last) {  // once per launch: the acquire is cheap here (chunk_info is read with sc1 loads anyway)
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
            verify_launch(sh, a, g.num_chunks, base_lines, tid);
        }
        FR_STAMP(5);
    }
#if defined(FR_STAMPS) && FR_STAMPS == 1
    FR_STAMP_FLUSH(k0_);
#endif
#if defined(FR_STAMPS) && FR_STAMPS == 4
    if ((threadIdx.x & 63) == 0)
        atomicAdd((unsigned long long*)&a.st->stamp[5], (unsigned long long)(__builtin_amdgcn_s_memtime() - k0_));
#endif
#if defined(FR_STAMPS) && FR_STAMPS == 3
    if (tid == 0 && blockIdx.x < TRACE_WGS) g_wg_trace[(a.par * TRACE_WGS + blockIdx.x) * 2 + 1] = __builtin_amdgcn_s_memrealtime();
#endif
    __syncthreads();
    if (tid == 0) {
        if (sh.created) atomicAdd((unsigned long long*)&a.st->n_keys, (unsigned long long)sh.created);
        if (sh.flags & 1u) atomicOr(&a.st->nonascii, 1u);
        if (sh.flags & 2u) atomicOr(&a.st->utf8_bad, 1u);
        // every workgroup has taken its last ticket: the last one out zeroes the launch's counters
        // for the next launch (stream order makes the plain stores visible to it)
        if (atomicAdd(&a.st->exits, 1u) == gridDim.x - 1u) {
            a.st->ticket = 0;
            a.st->chunks_done = 0;
            a.st->exits = 0;
        }
    }
}

int chunk_occupancy() { return FR_OCC; }

hipError_t launch_chunk_scan(const ScanArgs& a, int grid, hipStream_t s) {
    if (a.max_records > 0) hipLaunchKernelGGL(chunk_kernel<true>, dim3(grid), dim3(WG), 0, s, a);
    else hipLaunchKernelGGL(chunk_kernel<false>, dim3(grid), dim3(WG), 0, s, a);
    return hipGetLastError();
}

}  // namespace fr
