// fr_dmx_stats.hip — the per-output table of `demux --stats`: reads, bases, quality bytes, bases >= Q30 and the
// quality byte sum of every destination and mate, taken over the routed records while they are resident in HBM.
//
// After fr_dmx_route the context holds both mates' records destination-major (out), every record's offset and
// length in partition order (o, l) and the sorted destination of every partition position (k_out).  Partition
// order is offset order, and equal destinations are contiguous in it.  dmx_stats_kernel gives every wave a
// contiguous range of partition positions; the wave walks its records one at a time, its 64 lanes over the
// record's bytes in aligned 16-byte loads (the span's ends masked):
//   pass 1  the record's (at most four) '\n': per-lane SWAR masks, a ballot of the lanes that have one, and the
//           masks of those (at most four) lanes read into scalars: straight-line code for a record inside one
//           1-KiB step, a wave-uniform walk for a longer one.  They give the sequence line's length by
//           subtraction and the quality line's span [qa, qb);
//   pass 2  only the quality span's bytes are summed: v_sad_u8 for the byte values, a SWAR compare and a
//           popcount for the bytes >= '?' (Phred+33 Q30).
// The sums stay in registers while the destination stays the same.  When it changes inside a wave's range the
// wave adds its five sums to the u64 accumulators in HBM (one atomic instruction, five lanes); the sums a wave
// holds at the end of its range go through LDS, where the workgroup's waves with the same destination are added
// first.  A destination that takes a whole window (Undetermined often takes most of one) therefore costs one
// atomic instruction per workgroup, not one per record.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/frender_amd.h"
#include "fr_dmx_lines.h"
#include "fr_internal.h"

namespace fr {
namespace {

constexpr int SWG = 256;            // lanes per workgroup
constexpr int SWAVES = SWG / 64;
constexpr int SPER = 16;            // records per wave before the grid gets another workgroup
constexpr int SGRID = 1024;         // workgroups per mate at the most: 4 per CU, and the bound on the atomic
                                    // instructions a destination that takes the whole window receives
constexpr int SF = 5;               // reads, bases, quality_bytes, q30_bases, quality_raw_sum
constexpr u32 SNONE = 0xFFFFFFFFu;  // no destination yet
using namespace lines;  // STEP, load16, span_mask*, readlane64, newlines_1step, newlines (fr_dmx_lines.h)

__device__ __forceinline__ u32 byte_mask(u32 nib) {  // bits 0..3 -> 0xFF per set bit
    return ((nib * 0x00204081u) & 0x01010101u) * 0xFFu;
}

__device__ __forceinline__ u64 wave_sum(u64 x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

struct Sums {
    u64 reads, bases, qbytes;  // wave-uniform
    u64 q30, qsum;             // per lane
};

// the five sums, one per lane 0..4 (all lanes call)
__device__ __forceinline__ u64 lane_field(const Sums& s, int lane) {
    const u64 q30 = wave_sum(s.q30), qsum = wave_sum(s.qsum);
    return lane == 0 ? s.reads : lane == 1 ? s.bases : lane == 2 ? s.qbytes : lane == 3 ? q30 : qsum;
}

__device__ __forceinline__ void add_field(u64* acc, u32 dest, int n_dest, int lane, u64 val) {
    if (lane < SF && dest < (u32)n_dest && val)
        atomicAdd((unsigned long long*)&acc[(u64)dest * SF + lane], (unsigned long long)val);
}

// the quality bytes among the lane's 16 (bm: their bits): their sum and the count of those >= 63 into s
__device__ __forceinline__ void add_quality(const uint4& v, u32 bm, Sums& s) {
    const u32 w[4] = {v.x & byte_mask(bm & 15u), v.y & byte_mask((bm >> 4) & 15u), v.z & byte_mask((bm >> 8) & 15u),
                      v.w & byte_mask(bm >> 12)};
    u32 sum = 0, ge = 0;  // 32-bit partial sums live for one step only: at most 16 x 255, then into 64 bits
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        sum = __builtin_amdgcn_sad_u8(w[q], 0u, sum);
        // unsigned byte >= 63: bit 7 of (low seven bits + 65), or bit 7 of the byte itself
        ge += __popc((((w[q] & 0x7F7F7F7Fu) + 0x41414141u) | w[q]) & 0x80808080u);
    }
    s.qsum += sum;
    s.q30 += ge;
}

// a record that lies in one step (the usual one: up to 1 009 bytes): bytes [ro, re) of the step v0 holds, 16 per
// lane; straight-line code in 32 bits (newlines_1step)
__device__ __forceinline__ void add_record_1step(u32 ro, u32 re, const uint4& v0, int lane, Sums& s) {
    u32 p[4];  // positions in the step (registers); an entry at or past nnl is not used
    const u32 nnl = newlines_1step(ro, re, v0, lane, p);
    s.reads += 1;
    s.bases += nnl >= 1 ? (nnl >= 2 ? p[1] : re) - (p[0] + 1u) : 0u;
    const u32 qa = nnl >= 3 ? p[2] + 1u : 0u, qb = nnl >= 3 ? (nnl >= 4 ? p[3] : re) : 0u;
    s.qbytes += qb - qa;
    add_quality(v0, span_mask32((u32)lane * 16u, qa, qb), s);
}

// one record of any length: bytes [o, o + L) of buf, v0 = load16 of its first step
__device__ __forceinline__ void add_record(const u8* buf, u64 o, u64 L, const uint4& v0, int lane, Sums& s) {
    const u64 a0 = o & ~15ull, end = o + L;
    // pass 1: the positions (from o) of the record's '\n'; a record is at most four lines
    u64 p0, p1, p2, p3;
    const u32 nnl = newlines(buf, o, L, v0, lane, p0, p1, p2, p3);
    s.reads += 1;
    if (nnl >= 1) s.bases += (nnl >= 2 ? p1 : L) - (p0 + 1);
    if (nnl < 3) return;
    // pass 2: the quality line, bytes [qa, qb) of buf
    const u64 qa = o + p2 + 1, qb = o + (nnl >= 4 ? p3 : L);
    s.qbytes += qb - qa;
    if (qb <= qa) return;
    for (u64 st = (qa - a0) / STEP; st <= (qb - 1 - a0) / STEP; ++st) {
        const u64 a = a0 + st * STEP;
        const uint4 v = st == 0 ? v0 : load16(buf, a, end, lane);
        add_quality(v, span_mask(a + (u64)lane * 16, qa, qb), s);
    }
}

// grid (workgroups, mates); wave w of a mate takes partition positions [w * per_wave, (w + 1) * per_wave).  mates is
// 2, or 1 for a single-end window, whose out2 / o2 / l2 are null and never read
__global__ __launch_bounds__(SWG) void dmx_stats_kernel(const u8* out1, const u8* out2, const u64* o1, const u64* l1,
                                                        const u64* o2, const u64* l2, const u32* __restrict__ dest,
                                                        u64 n, u32 per_wave, int n_dest, u64* acc) {
    __shared__ u64 wv[SWAVES][SF];
    __shared__ u32 wd[SWAVES];
    const int mate = blockIdx.y;
    const u8* buf = mate ? out2 : out1;
    const u64* off = mate ? o2 : o1;
    const u64* len = mate ? l2 : l1;
    u64* A = acc + (u64)mate * (u64)n_dest * SF;
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u64 wave = (u64)blockIdx.x * SWAVES + (u64)wid;
    const u64 j0 = min(wave * per_wave, n), j1 = min(j0 + per_wave, n);
    u32 cur = SNONE;
    Sums s{0, 0, 0, 0, 0};
    for (u64 b = j0; b < j1; b += 64) {
        // the next 64 records' length and destination: one coalesced load each, then lane reads; the records are
        // packed in partition order, so the first one's offset gives the others'
        const u32 cnt = (u32)min((u64)64, j1 - b);
        u64 ml = 0;
        u32 mk = 0;
        if ((u32)lane < cnt) {
            ml = len[b + lane];
            mk = dest[b + lane];
        }
        u64 o = off[b], L = readlane64(ml, 0);
        uint4 v0 = load16(buf, o & ~15ull, o + L, lane);
        for (u32 r = 0; r < cnt; ++r) {
            const u32 k = __builtin_amdgcn_readlane(mk, r);
            const u64 on = o + L;
            u64 Ln = 0;
            uint4 nxt = make_uint4(0u, 0u, 0u, 0u);
            if (r + 1 < cnt) {  // the next record's first step is in flight while this one is summed
                Ln = readlane64(ml, r + 1);
                nxt = load16(buf, on & ~15ull, on + Ln, lane);
            }
            if (k != cur) {  // the run of `cur` ends inside this wave's range
                if (cur != SNONE) add_field(A, cur, n_dest, lane, lane_field(s, lane));
                cur = k;
                s = Sums{0, 0, 0, 0, 0};
            }
            const u64 a0 = o & ~15ull;
            if (on - a0 <= STEP)
                add_record_1step((u32)(o - a0), (u32)(on - a0), v0, lane, s);
            else
                add_record(buf, o, L, v0, lane, s);
            o = on;
            L = Ln;
            v0 = nxt;
        }
    }
    // the runs still open at the ends of the waves' ranges: equal destinations are adjacent waves
    const u64 val = lane_field(s, lane);
    if (lane < SF) wv[wid][lane] = val;
    if (lane == 0) wd[wid] = cur;
    __syncthreads();
    if (wid == 0 && lane < SF) {
        u32 dc = wd[0];
        u64 a = wv[0][lane];
#pragma unroll
        for (int w = 1; w < SWAVES; ++w) {
            if (wd[w] == dc) {
                a += wv[w][lane];
            } else {
                add_field(A, dc, n_dest, lane, a);
                dc = wd[w];
                a = wv[w][lane];
            }
        }
        add_field(A, dc, n_dest, lane, a);
    }
}

}  // namespace

struct DmxStats {
    int device = 0;
    hipStream_t stream = nullptr;
    int n_dest = 0;
    u64* acc = nullptr;  // [2][n_dest][SF]
};

#define SK(x)                                                                  \
    do {                                                                       \
        hipError_t e_ = (x);                                                   \
        if (e_ != hipSuccess) {                                                \
            err = std::string(#x) + ": " + hipGetErrorString(e_);              \
            return FR_ERR_HIP;                                                 \
        }                                                                      \
    } while (0)

static u64 acc_bytes(int n_dest) { return (u64)2 * (u64)std::max(n_dest, 1) * SF * sizeof(u64); }

void dmx_stats_destroy(DmxStats* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    if (t->acc) (void)hipFree(t->acc);
    delete t;
}

int dmx_stats_begin(DmxStats** out, int device, hipStream_t stream, int n_dest, std::string& err) {
    if (n_dest < 0) return err = "fr_dmx_stats_begin: n_dest is negative", FR_ERR_INVALID;
    DmxStats* t = *out;
    if (!t || t->n_dest != n_dest) {
        dmx_stats_destroy(t);
        *out = t = new DmxStats();  // (freed by the owner's destroy if a step below fails)
        t->device = device;
        t->stream = stream;
        t->n_dest = n_dest;
        SK(hipMalloc((void**)&t->acc, acc_bytes(n_dest)));
    }
    SK(hipMemsetAsync(t->acc, 0, acc_bytes(n_dest), stream));
    return FR_OK;
}

int dmx_stats_n_dest(const DmxStats* t) { return t->n_dest; }

int dmx_stats_window(DmxStats* t, const u8* out1, const u8* out2, const u64* o1, const u64* l1, const u64* o2,
                     const u64* l2, const u32* dest, u64 n, std::string& err) {
    if (!n) return FR_OK;
    const u64 gx = std::max<u64>(1, std::min<u64>((n + SWAVES * SPER - 1) / (SWAVES * SPER), (u64)SGRID));
    const u64 per_wave = (n + gx * SWAVES - 1) / (gx * SWAVES);  // n < 2^32: fr_dmx_route's bound
    hipLaunchKernelGGL(dmx_stats_kernel, dim3((unsigned)gx, out2 ? 2 : 1), dim3(SWG), 0, t->stream, out1, out2, o1, l1,
                       o2, l2, dest, n, (u32)per_wave, t->n_dest, t->acc);
    SK(hipGetLastError());
    return FR_OK;
}

int dmx_stats_get(DmxStats* t, u64* out, std::string& err) {
    SK(hipStreamSynchronize(t->stream));
    if (t->n_dest) SK(hipMemcpy(out, t->acc, (u64)2 * t->n_dest * SF * sizeof(u64), hipMemcpyDeviceToHost));
    return FR_OK;
}

}  // namespace fr
