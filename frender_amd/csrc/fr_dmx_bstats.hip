// fr_dmx_bstats.hip — the index mismatch table of `demux -b --barcode-stats`: per destination, how many routed pairs
// fell into each (index-1 bin, index-2 bin), the bins being 0, 1, 2, 3 or more mismatches against the reference row,
// and none.  The classifier (fr_classify.hip, dmx_class_kernel<W, true>) and the host (fr_dmx_bstats_patch) leave
// one byte bin1 * 5 + bin2 per R2 record; this file adds a routed window's bytes to u64 counters in HBM.
//
// After fr_dmx_route the context holds the sorted destination of every partition position (k_out) and the pair
// that stands there (perm); equal destinations are contiguous.  dmx_bstats_kernel gives every wave a contiguous
// range of partition positions and takes them 64 at a time: destination and pair index in one coalesced load each,
// the pair's bin byte by a gather.  Inside the 64 a run of one destination is a ballot; within the run each bin
// that occurs is a ballot and a popcount, added to the register of lane `bin`.  The 25 lane registers stay with
// the wave while the destination stays the same.  When it changes inside the wave's range the wave adds its
// non-zero counts to HBM (one atomic instruction, at most 25 lanes on 200 contiguous bytes); the counts a wave
// holds at the end of its range go through LDS, where the workgroup's waves with the same destination are added
// first.  A destination and bin that take a whole window (Undetermined with none,none often take most of one)
// therefore cost one atomic per workgroup, not one per record, and nothing here is sized by n_dest: the same
// path serves a sheet of any size.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/frender_amd.h"
#include "fr_internal.h"

namespace fr {
namespace {

constexpr int BWG = 256;            // lanes per workgroup
constexpr int BWAVES = BWG / 64;
constexpr int BPER = 128;           // positions per wave before the grid gets another workgroup
constexpr int BGRID = 1024;         // workgroups at the most: the bound on the atomic instructions a destination
                                    // that takes the whole window receives
constexpr int NB = DMX_BINS;
constexpr u32 BNONE = 0xFFFFFFFFu;  // no destination yet
static_assert(NB <= 64, "one lane per bin");

// lane b < NB holds the count of bin b: the non-zero ones go to destination dest's counters
__device__ __forceinline__ void add_bins(u64* acc, u32 dest, int n_dest, int lane, u64 count) {
    if (lane < NB && dest < (u32)n_dest && count)
        atomicAdd((unsigned long long*)&acc[(u64)dest * NB + lane], (unsigned long long)count);
}

// wave w takes partition positions [w * per_wave, (w + 1) * per_wave)
__global__ __launch_bounds__(BWG) void dmx_bstats_kernel(const u32* __restrict__ dest, const u32* __restrict__ perm,
                                                         const u8* __restrict__ rec_bin, u64 n, u32 per_wave,
                                                         int n_dest, u64* acc) {
    __shared__ u64 wv[BWAVES][NB];
    __shared__ u32 wd[BWAVES];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u64 wave = (u64)blockIdx.x * BWAVES + (u64)wid;
    const u64 j0 = min(wave * per_wave, n), j1 = min(j0 + per_wave, n);
    u32 cur = BNONE;  // the open run's destination (wave-uniform)
    u64 count = 0;    // lane b < NB: the open run's records of bin b
    for (u64 b = j0; b < j1; b += 64) {
        const bool in = b + (u64)lane < j1;
        u32 k = BNONE, bin = DMX_NO_BIN;
        if (in) {
            k = dest[b + lane];
            bin = rec_bin[perm[b + lane]];
        }
        const bool counted = in && bin < (u32)NB;  // a byte past the bins is never counted
        u64 left = __ballot(in);
        while (left) {  // one turn per run of equal destinations among the 64
            const u32 kr = __builtin_amdgcn_readlane(k, __builtin_ctzll(left));
            const u64 run = __ballot(in && k == kr) & left;
            if (kr != cur) {  // the run of `cur` ends inside this wave's range
                add_bins(acc, cur, n_dest, lane, count);
                cur = kr;
                count = 0;
            }
            u64 rem = __ballot(counted) & run;
            while (rem) {  // one turn per bin that occurs in the run
                const u32 br = __builtin_amdgcn_readlane(bin, __builtin_ctzll(rem));
                const u64 m = __ballot(bin == br) & rem;
                if ((u32)lane == br) count += (u64)__popcll(m);
                rem &= ~m;
            }
            left &= ~run;
        }
    }
    // the runs still open at the ends of the waves' ranges: equal destinations are adjacent waves
    if (lane < NB) wv[wid][lane] = count;
    if (lane == 0) wd[wid] = cur;
    __syncthreads();
    if (wid == 0 && lane < NB) {
        u32 dc = wd[0];
        u64 a = wv[0][lane];
#pragma unroll
        for (int w = 1; w < BWAVES; ++w) {
            if (wd[w] == dc) {
                a += wv[w][lane];
            } else {
                add_bins(acc, dc, n_dest, lane, a);
                dc = wd[w];
                a = wv[w][lane];
            }
        }
        add_bins(acc, dc, n_dest, lane, a);
    }
}

}  // namespace

struct DmxBstats {
    int device = 0;
    hipStream_t stream = nullptr;
    int n_dest = 0;
    u64* acc = nullptr;  // [n_dest][5][5]
};

#define BK(x)                                                                  \
    do {                                                                       \
        hipError_t e_ = (x);                                                   \
        if (e_ != hipSuccess) {                                                \
            err = std::string(#x) + ": " + hipGetErrorString(e_);              \
            return FR_ERR_HIP;                                                 \
        }                                                                      \
    } while (0)

static u64 bstats_bytes(int n_dest) { return (u64)std::max(n_dest, 1) * NB * sizeof(u64); }

void dmx_bstats_destroy(DmxBstats* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    if (t->acc) (void)hipFree(t->acc);
    delete t;
}

int dmx_bstats_begin(DmxBstats** out, int device, hipStream_t stream, int n_dest, std::string& err) {
    if (n_dest < 0) return err = "fr_dmx_bstats_begin: n_dest is negative", FR_ERR_INVALID;
    DmxBstats* t = *out;
    if (!t || t->n_dest != n_dest) {
        dmx_bstats_destroy(t);
        *out = t = new DmxBstats();  // (freed by the owner's destroy if a step below fails)
        t->device = device;
        t->stream = stream;
        t->n_dest = n_dest;
        BK(hipMalloc((void**)&t->acc, bstats_bytes(n_dest)));
    }
    BK(hipMemsetAsync(t->acc, 0, bstats_bytes(n_dest), stream));
    return FR_OK;
}

int dmx_bstats_n_dest(const DmxBstats* t) { return t->n_dest; }

int dmx_bstats_window(DmxBstats* t, const u32* dest, const u32* perm, const u8* rec_bin, u64 n, std::string& err) {
    if (!n) return FR_OK;
    const u64 gx = std::max<u64>(1, std::min<u64>((n + BWAVES * BPER - 1) / (BWAVES * BPER), (u64)BGRID));
    const u64 per_wave = (n + gx * BWAVES - 1) / (gx * BWAVES);  // n < 2^32: fr_dmx_route's bound
    hipLaunchKernelGGL(dmx_bstats_kernel, dim3((unsigned)gx), dim3(BWG), 0, t->stream, dest, perm, rec_bin, n,
                       (u32)per_wave, t->n_dest, t->acc);
    BK(hipGetLastError());
    return FR_OK;
}

int dmx_bstats_get(DmxBstats* t, u64* out, std::string& err) {
    BK(hipStreamSynchronize(t->stream));
    if (t->n_dest) BK(hipMemcpy(out, t->acc, (u64)t->n_dest * NB * sizeof(u64), hipMemcpyDeviceToHost));
    return FR_OK;
}

}  // namespace fr
