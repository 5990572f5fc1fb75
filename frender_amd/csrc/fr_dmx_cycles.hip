// fr_dmx_cycles.hip — the per-cycle table of `demux --cycle-stats`: for every destination, mate and 0-based cycle c
// (position in the line), the sequence line's bytes at c counted as A, C, G, T, N or other, and the quality line's
// bytes at c counted, counted when >= 63 (Phred+33 Q30) and summed; cycles at or past max_cycles share one tail
// bin.  Taken over the routed records while they are resident in HBM.
//
// After fr_dmx_route the context holds both mates' records destination-major (out), every record's offset and
// length in partition order (o, l) and the sorted destination of every partition position (k_out): partition order
// is offset order, and equal destinations are contiguous in it.  dmx_cycles_kernel gives every workgroup a
// contiguous range of partition positions and walks it run by run (a run: the range's positions with one
// destination, found by bisection).  Inside a run the eight waves take the records in turn; a wave finds its
// record's '\n' as dmx_stats_kernel does (fr_dmx_lines.h), then lane l takes cycles l, l + 64, ... of the sequence
// and of the quality line: one byte load per lane, coalesced over the wave, and ds_add_u32 into the workgroup's
// LDS accumulator u32 [9][max_cycles], whose rows are cycle-major so that a wave's lanes hit consecutive banks and
// never each other.  Cycles past max_cycles are summed per lane in 64-bit registers.  When the run ends (the
// destination changes, or the range ends) the workgroup adds the accumulator to the u64 sums in HBM -- the bins
// below the longest line the run has seen, the non-zero ones only -- and clears what it added.  So the atomics in
// HBM are per (workgroup, run, cycle seen, field), never per record or per byte.
//
// No 32-bit partial sum can overflow: between two flushes a bin below max_cycles gets at most one byte (<= 255) per
// record, and a workgroup's range is at most CMAXRANGE = 2^20 records (dmx_cycles_window sizes the grid so), hence
// a bin stays below 2^28.  The tail bin takes any number of bytes per record; it is 64 bits wide everywhere.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/frender_amd.h"
#include "fr_dmx_lines.h"
#include "fr_internal.h"

namespace fr {
namespace {

using namespace lines;

constexpr int CWG = 512;                // lanes per workgroup: eight waves share one accumulator
constexpr int CWAVES = CWG / 64;
constexpr int CF = 9;                   // A, C, G, T, N, other, quality_bytes, q30_bases, quality_raw_sum
constexpr int CPER = 128;               // records per workgroup before the grid gets another workgroup
constexpr int CGRID = 256;              // workgroups per mate (2 per CU in all), unless CMAXRANGE asks for more
constexpr u64 CMAXRANGE = 1ull << 20;   // records per workgroup at the most: 2^20 x 255 < 2^32
constexpr int CMAXCYCLES = 1024;

__device__ __forceinline__ u64 wave_sum(u64 x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

__device__ __forceinline__ u64 uniform64(u64 x) {
    const u32 lo = __builtin_amdgcn_readfirstlane((u32)x), hi = __builtin_amdgcn_readfirstlane((u32)(x >> 32));
    return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ u32 base_class(u32 b) {
    return b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : b == 'N' ? 4u : 5u;
}

// one record: the sequence line [sa, sb) and the quality line [qa, qb) of buf into bins (cycles below mc) and tail
// (past).  Lane l takes cycles l, l + 64, ... of both lines, 256 cycles per round: the round's (up to eight) byte
// loads are all in flight before the first is used, so a record of up to 256 cycles waits for memory once.
__device__ __forceinline__ void add_lines(const u8* buf, u64 sa, u64 sb, u64 qa, u64 qb, u32 mc, int lane, u32* bins,
                                          u64 (&tail)[CF]) {
    const u8 *sp = buf + sa, *qp = buf + qa;
    const u64 slen = sb - sa, qlen = qb - qa;
    for (u64 c0 = 0; c0 < max(slen, qlen); c0 += 256) {
        u32 sv[4], qv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const u64 c = c0 + (u64)(k * 64 + lane);
            sv[k] = c < slen ? (u32)sp[c] : 0u;
            qv[k] = c < qlen ? (u32)qp[c] : 0u;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const u64 c = c0 + (u64)(k * 64 + lane);
            if (c < slen) {
                const u32 cls = base_class(sv[k]);
                if (c < mc) {
                    atomicAdd(&bins[cls * mc + (u32)c], 1u);
                } else {
#pragma unroll
                    for (u32 f = 0; f < 6; ++f) tail[f] += cls == f;
                }
            }
            if (c < qlen) {
                const u32 b = qv[k];
                if (c < mc) {
                    atomicAdd(&bins[6 * mc + (u32)c], 1u);
                    if (b >= 63u) atomicAdd(&bins[7 * mc + (u32)c], 1u);
                    atomicAdd(&bins[8 * mc + (u32)c], b);
                } else {
                    tail[6] += 1;
                    tail[7] += b >= 63u;
                    tail[8] += b;
                }
            }
        }
    }
}

// grid (workgroups, mates); workgroup g of a mate takes partition positions [g * per_wg, (g + 1) * per_wg); mates is 2,
// or 1 for a single-end window, whose out2 / o2 / l2 are null and never read; dynamic LDS: u32 [CF][mc]
__global__ __launch_bounds__(CWG) void dmx_cycles_kernel(const u8* out1, const u8* out2, const u64* o1, const u64* l1,
                                                         const u64* o2, const u64* l2, const u32* __restrict__ dest,
                                                         u64 n, u32 per_wg, int n_dest, u32 mc, u64* acc) {
    extern __shared__ u32 bins[];  // [CF][mc]: row f, cycle c
    __shared__ u64 tail_s[CF];     // the cycles at and past mc
    __shared__ u32 seen_s;         // the run's longest line, at most mc
    const int mate = blockIdx.y;
    const u8* buf = mate ? out2 : out1;
    const u64* off = mate ? o2 : o1;
    const u64* len = mate ? l2 : l1;
    const u32 tid = threadIdx.x;
    const int lane = tid & 63;
    const u32 wid = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const u64 j0 = min((u64)blockIdx.x * per_wg, n), j1 = min(j0 + per_wg, n);
    for (u32 i = tid; i < CF * mc; i += CWG) bins[i] = 0u;
    if (tid < CF) tail_s[tid] = 0;
    if (tid == 0) seen_s = 0u;
    __syncthreads();
    u64 pos = j0;
    while (pos < j1) {
        // the run [pos, e): dest is sorted, so its end is found by bisection (the same loads in every lane)
        const u32 cur = (u32)__builtin_amdgcn_readfirstlane((int)dest[pos]);
        u64 lo = pos + 1, hi = j1;
        if ((u32)__builtin_amdgcn_readfirstlane((int)dest[j1 - 1]) == cur) lo = j1;  // (the usual one: to the end)
        while (lo < hi) {
            const u64 mid = lo + (hi - lo) / 2;
            const bool same = (u32)__builtin_amdgcn_readfirstlane((int)dest[mid]) == cur;
            lo = same ? mid + 1 : lo;
            hi = same ? hi : mid;
        }
        const u64 e = uniform64(lo);
        u32 wmax = 0;        // wave-uniform: the longest line of this wave's records, at most mc
        bool past = false;   // wave-uniform: a line went past mc
        u64 tail[CF] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        // wave w takes records pos + w, pos + w + 8, ...: 64 of them per batch, their offset and length loaded by the
        // lanes and read back one by one
        for (u64 b = pos + wid; b < e; b += 64 * CWAVES) {
            const u32 cnt = (u32)min((u64)64, (e - b + CWAVES - 1) / CWAVES);
            u64 mo = 0, ml = 0;
            if ((u32)lane < cnt) {
                mo = off[b + (u64)lane * CWAVES];
                ml = len[b + (u64)lane * CWAVES];
            }
            u64 o = readlane64(mo, 0), L = readlane64(ml, 0);
            uint4 v0 = load16(buf, o & ~15ull, o + L, lane);
            for (u32 r = 0; r < cnt; ++r) {
                u64 on = 0, Ln = 0;
                uint4 nxt = make_uint4(0u, 0u, 0u, 0u);
                if (r + 1 < cnt) {  // the next record's first step is in flight while this one is counted
                    on = readlane64(mo, r + 1);
                    Ln = readlane64(ml, r + 1);
                    nxt = load16(buf, on & ~15ull, on + Ln, lane);
                }
                const u64 a0 = o & ~15ull, end = o + L;
                u64 sa = 0, sb = 0, qa = 0, qb = 0;  // the sequence and the quality line (absent: empty)
                if (end - a0 <= STEP) {
                    u32 p[4];
                    const u32 nnl = newlines_1step((u32)(o - a0), (u32)(end - a0), v0, lane, p);
                    if (nnl >= 1) sa = a0 + p[0] + 1, sb = nnl >= 2 ? a0 + p[1] : end;
                    if (nnl >= 3) qa = a0 + p[2] + 1, qb = nnl >= 4 ? a0 + p[3] : end;
                } else {
                    u64 p0, p1, p2, p3;
                    const u32 nnl = newlines(buf, o, L, v0, lane, p0, p1, p2, p3);
                    if (nnl >= 1) sa = o + p0 + 1, sb = nnl >= 2 ? o + p1 : end;
                    if (nnl >= 3) qa = o + p2 + 1, qb = nnl >= 4 ? o + p3 : end;
                }
                const u64 longest = max(sb - sa, qb - qa);
                wmax = max(wmax, (u32)min(longest, (u64)mc));
                past = past || longest > mc;
                add_lines(buf, sa, sb, qa, qb, mc, lane, bins, tail);
                o = on;
                L = Ln;
                v0 = nxt;
            }
        }
        if (past) {  // (wave-uniform)
#pragma unroll
            for (int f = 0; f < CF; ++f) {
                const u64 t = wave_sum(tail[f]);
                if (lane == 0 && t) atomicAdd((unsigned long long*)&tail_s[f], (unsigned long long)t);
            }
        }
        if (lane == 0 && wmax) atomicMax(&seen_s, wmax);
        __syncthreads();
        // the run is counted: add the bins it touched to the sums in HBM and clear them
        const u32 seen = seen_s;
        const bool ok = cur < (u32)n_dest;  // a destination at or above n_dest is never written
        u64* A = acc + ((u64)mate * (u64)(ok ? n_dest : 0) + (ok ? cur : 0u)) * (u64)(mc + 1) * CF;
        __syncthreads();
        if (tid == 0) seen_s = 0u;
        for (u32 i = tid; i < seen * CF; i += CWG) {  // i = c * CF + f: consecutive lanes, consecutive words in HBM
            const u32 c = i / CF, f = i - c * CF;
            const u32 v = bins[f * mc + c];
            if (v) {
                bins[f * mc + c] = 0u;
                if (ok) atomicAdd((unsigned long long*)&A[i], (unsigned long long)v);
            }
        }
        if (tid < CF) {
            const u64 v = tail_s[tid];
            if (v) {
                tail_s[tid] = 0;
                if (ok) atomicAdd((unsigned long long*)&A[(u64)mc * CF + tid], (unsigned long long)v);
            }
        }
        __syncthreads();
        pos = e;
    }
}

}  // namespace

struct DmxCycles {
    int device = 0;
    hipStream_t stream = nullptr;
    int n_dest = 0;
    int max_cycles = 0;
    u64* acc = nullptr;  // [2][n_dest][max_cycles + 1][CF]
};

#define CK(x)                                                                  \
    do {                                                                       \
        hipError_t e_ = (x);                                                   \
        if (e_ != hipSuccess) {                                                \
            err = std::string(#x) + ": " + hipGetErrorString(e_);              \
            return FR_ERR_HIP;                                                 \
        }                                                                      \
    } while (0)

static u64 acc_words(int n_dest, int max_cycles) { return (u64)2 * (u64)n_dest * (u64)(max_cycles + 1) * CF; }

bool dmx_cycles_args_ok(int n_dest, int max_cycles) {
    return n_dest >= 0 && max_cycles >= 1 && max_cycles <= CMAXCYCLES;
}

void dmx_cycles_destroy(DmxCycles* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    if (t->acc) (void)hipFree(t->acc);
    delete t;
}

int dmx_cycles_begin(DmxCycles** out, int device, hipStream_t stream, int n_dest, int max_cycles, std::string& err) {
    if (!dmx_cycles_args_ok(n_dest, max_cycles))
        return err = "fr_dmx_cycles_begin: n_dest is negative or max_cycles is not in 1..1024", FR_ERR_INVALID;
    DmxCycles* t = *out;
    const u64 bytes = std::max<u64>(acc_words(n_dest, max_cycles), 1) * sizeof(u64);
    if (!t || t->n_dest != n_dest || t->max_cycles != max_cycles) {
        dmx_cycles_destroy(t);
        *out = t = new DmxCycles();  // (freed by the owner's destroy if a step below fails)
        t->device = device;
        t->stream = stream;
        t->n_dest = n_dest;
        t->max_cycles = max_cycles;
        CK(hipMalloc((void**)&t->acc, bytes));
    }
    CK(hipMemsetAsync(t->acc, 0, bytes, stream));
    return FR_OK;
}

int dmx_cycles_n_dest(const DmxCycles* t) { return t->n_dest; }
int dmx_cycles_max_cycles(const DmxCycles* t) { return t->max_cycles; }

int dmx_cycles_window(DmxCycles* t, const u8* out1, const u8* out2, const u64* o1, const u64* l1, const u64* o2,
                      const u64* l2, const u32* dest, u64 n, std::string& err) {
    if (!n) return FR_OK;
    u64 gx = std::max<u64>(1, std::min<u64>((n + CPER - 1) / CPER, (u64)CGRID));
    gx = std::max(gx, (n + CMAXRANGE - 1) / CMAXRANGE);  // n < 2^32 (fr_dmx_route's bound): at most 4096
    const u64 per_wg = (n + gx - 1) / gx;                // <= CMAXRANGE: the bound on a 32-bit bin
    const size_t lds = (size_t)CF * (size_t)t->max_cycles * sizeof(u32);
    hipLaunchKernelGGL(dmx_cycles_kernel, dim3((unsigned)gx, out2 ? 2 : 1), dim3(CWG), lds, t->stream, out1, out2, o1, l1,
                       o2, l2, dest, n, (u32)per_wg, t->n_dest, (u32)t->max_cycles, t->acc);
    CK(hipGetLastError());
    return FR_OK;
}

int dmx_cycles_get(DmxCycles* t, u64* out, std::string& err) {
    CK(hipStreamSynchronize(t->stream));
    const u64 words = acc_words(t->n_dest, t->max_cycles);
    if (words) CK(hipMemcpy(out, t->acc, words * sizeof(u64), hipMemcpyDeviceToHost));
    return FR_OK;
}

}  // namespace fr
