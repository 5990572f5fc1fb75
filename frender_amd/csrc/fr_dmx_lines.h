// fr_dmx_lines.h — a routed record's lines, found by one wave: shared by the kernels that walk the routed bytes
// record by record (fr_dmx_stats.hip, fr_dmx_cycles.hip).
//
// A wave's 64 lanes cover 1 KiB of the routed bytes per step in aligned 16-byte loads (load16).  The record's (at
// most four) '\n' are found from per-lane SWAR masks (nl_mask16, the span's ends masked), a ballot of the lanes that
// have one, and the masks of those (at most four) lanes read into scalars: newlines_1step is straight-line code for
// a record inside one step, newlines a wave-uniform walk for a longer one.  The positions give the lines: split at
// '\n', the second piece is the sequence and the fourth the quality line (absent pieces are empty).
#pragma once
#include <hip/hip_runtime.h>

#include "fr_internal.h"

namespace fr {
namespace lines {

constexpr u32 STEP = 64 * 16;  // bytes a wave loads per step

__device__ __forceinline__ u32 eq4(u32 w, u32 rep) {  // exact byte equality -> bits 0..3
    const u32 t = w ^ rep;
    const u32 z = ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) & 0x80808080u;
    return __builtin_amdgcn_udot4(z >> 7, 0x08040201u, 0u, false);
}

__device__ __forceinline__ u32 nl_mask16(const uint4& v) {  // '\n' bytes of 16 -> bits 0..15
    return eq4(v.x, 0x0A0A0A0Au) | (eq4(v.y, 0x0A0A0A0Au) << 4) | (eq4(v.z, 0x0A0A0A0Au) << 8) |
           (eq4(v.w, 0x0A0A0A0Au) << 12);
}

__device__ __forceinline__ u32 eq_mask16(const uint4& v, u32 rep) {  // bytes of 16 equal to rep's byte -> bits 0..15
    return eq4(v.x, rep) | (eq4(v.y, rep) << 4) | (eq4(v.z, rep) << 8) | (eq4(v.w, rep) << 12);
}

__device__ __forceinline__ u32 either_mask16(const uint4& v, u32 rep_a, u32 rep_b) {  // equal to either of two bytes
    return eq_mask16(v, rep_a) | eq_mask16(v, rep_b);
}

// bits i of 0..15 with lo <= p + i < hi
__device__ __forceinline__ u32 span_mask(u64 p, u64 lo, u64 hi) {
    const u32 s = lo > p ? (u32)min(lo - p, (u64)16) : 0u;
    const u32 e = hi > p ? (u32)min(hi - p, (u64)16) : 0u;
    return e > s ? ((1u << e) - 1u) & ~((1u << s) - 1u) : 0u;
}

// the same in 32 bits: p, lo, hi relative to one origin, all below 2^31
__device__ __forceinline__ u32 span_mask32(u32 p, u32 lo, u32 hi) {
    const u32 s = (u32)min(max((int)lo - (int)p, 0), 16);
    const u32 e = (u32)min(max((int)hi - (int)p, 0), 16);
    return ((1u << e) - 1u) & ~((1u << s) - 1u);  // (empty when e <= s)
}

__device__ __forceinline__ u64 readlane64(u64 x, u32 l) {
    const u32 lo = __builtin_amdgcn_readlane((u32)x, l), hi = __builtin_amdgcn_readlane((u32)(x >> 32), l);
    return ((u64)hi << 32) | lo;
}

// the lane's 16 bytes of the step that starts at the 16-byte aligned offset a (zeros at and past end; the
// buffer has 16 bytes of slack past its last record)
__device__ __forceinline__ uint4 load16(const u8* buf, u64 a, u64 end, int lane) {
    const u64 p = a + (u64)lane * 16;
    return p < end ? *(const uint4*)(buf + p) : make_uint4(0u, 0u, 0u, 0u);
}

// a record that lies in one step (the usual one: up to 1 009 bytes): bytes [ro, re) of the step v0 holds, 16 per
// lane.  Straight-line code in 32 bits: the lanes that hold the record's (at most four) '\n' are at most four, so
// their 16-bit masks go side by side into one 64-bit scalar, in lane order, and its set bits, in order, are the
// record's '\n' in order.  Returns their count (at most 4); p: their positions in the step (an entry at or past the
// count is not to be used).
__device__ __forceinline__ u32 newlines_1step(u32 ro, u32 re, const uint4& v0, int lane, u32 (&p)[4]) {
    const u32 lb = (u32)lane * 16u;
    const u32 m = nl_mask16(v0) & span_mask32(lb, ro, re);
    u64 bal = __ballot(m != 0);
    u64 W = 0;
    u32 lanes = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const u32 ln = bal ? (u32)__builtin_ctzll(bal) : 0u;
        const u32 mm = __builtin_amdgcn_readlane(m, ln);
        W |= (u64)(bal ? mm : 0u) << (16 * t);
        lanes |= ln << (8 * t);
        bal &= bal - 1;
    }
    const u32 nnl = min((u32)__popcll(W), 4u);
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // (unrolled: p stays in registers)
        const u32 b = W ? (u32)__builtin_ctzll(W) : 0u;
        W &= W - 1;
        p[k] = ((lanes >> (8u * (b >> 4))) & 63u) * 16u + (b & 15u);
    }
    return nnl;
}

// one record of any length: bytes [o, o + L) of buf, v0 = load16 of its first step.  Returns the count of its '\n'
// (at most 4: a record is at most four lines); p0..p3: their positions from o.
__device__ __forceinline__ u32 newlines(const u8* buf, u64 o, u64 L, const uint4& v0, int lane, u64& p0, u64& p1,
                                        u64& p2, u64& p3) {
    const u64 a0 = o & ~15ull, end = o + L;
    const u64 nsteps = (end - a0 + STEP - 1) / STEP;
    u32 nnl = 0;
    u64 q0 = 0, q1 = 0, q2 = 0, q3 = 0;  // (locals, copied out at the end: they stay in registers)
    for (u64 st = 0; st < nsteps && nnl < 4; ++st) {
        const u64 a = a0 + st * STEP;
        const uint4 v = st == 0 ? v0 : load16(buf, a, end, lane);
        const u32 m = nl_mask16(v) & span_mask(a + (u64)lane * 16, o, end);
        u64 bal = __ballot(m != 0);
        while (bal && nnl < 4) {
            const u32 ln = (u32)__builtin_ctzll(bal);
            bal &= bal - 1;
            u32 mm = __builtin_amdgcn_readlane(m, ln);
            const u64 base = a + (u64)ln * 16 - o;  // (a bit below o is masked out: base + bit >= 0)
            while (mm && nnl < 4) {
                const u64 pos = base + (u32)__builtin_ctz(mm);
                mm &= mm - 1;
                if (nnl == 0) q0 = pos;
                else if (nnl == 1) q1 = pos;
                else if (nnl == 2) q2 = pos;
                else q3 = pos;
                ++nnl;
            }
        }
    }
    p0 = q0, p1 = q1, p2 = q2, p3 = q3;
    return nnl;
}

}  // namespace lines
}  // namespace fr
