// fr_table.hip — gfx950 kernels around the HBM table, everything but the tally (fr_kernels.hip):
//  table / order : maintenance, the launch log's aggregation, the first-occurrence-ordered merged table of
//                  frender.py:199-203 (radix sort or binning; the one user of rocprim), presence, multi-GPU merge
//  synth         : SYN-v1 records (frender_amd/synth.py), device side
#include <algorithm>
#include <cstring>  // (rocprim's headers use memset without including it)

#include <rocprim/rocprim.hpp>

#include "../../include/frender_amd.h"
#include "fr_internal.h"
#include "fr_table_dev.h"

namespace fr {

// ------------------------------------------------------------------------------------
// table maintenance
// ------------------------------------------------------------------------------------
__global__ void table_init_kernel(GSlot* slots, u64 n, DevState* st) {
    // fr_reset: the device state's reset image too (zero counters, no error offset), by workgroup 0 --
    // no upload dispatch behind this kernel
    if (st && blockIdx.x == 0) {
        static_assert(sizeof(DevState) % sizeof(u32) == 0 && offsetof(DevState, err_nospace) % sizeof(u32) == 0,
                      "DevState is written as 32-bit words");
        constexpr u32 E = (u32)(offsetof(DevState, err_nospace) / sizeof(u32));
        u32* w = (u32*)st;
        for (u32 i = threadIdx.x; i < (u32)(sizeof(DevState) / sizeof(u32)); i += blockDim.x)
            w[i] = (i == E || i == E + 1) ? 0xFFFFFFFFu : 0u;
    }
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        GSlot g;
        g.key = 0;
        g.count = 0;
        g.first = ~0ull;
        g.last_tag = 0;
        g.uidx = 0;
        slots[i] = g;
    }
}

hipError_t launch_table_init(GSlot* slots, u64 n, DevState* st, hipStream_t s) {
    const int grid = (int)std::min<u64>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(table_init_kernel, dim3(grid > 0 ? grid : 1), dim3(256), 0, s, slots, n, st);
    return hipGetLastError();
}

__device__ __forceinline__ bool last_block(u32* ctr);

// re-insert overflow entries (after the table has grown); presence is re-derived.  An entry whose probe
// window is still full goes on the (fresh) overflow list again: the grid's last workgroup reports how many did,
// straight into pinned host memory, and grow_table grows the table until none is left.  The counter is the
// aggregation's (zero between launches, and zero again afterwards).
__global__ void reinsert_kernel(Table t, DevState* st, const Overflow* src, u64 n, u64* left_out) {
    u32 made = 0;
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const Overflow o = src[i];
        made += global_insert(t, st, o.key, o.count, o.first, o.tag) ? 1u : 0u;
    }
    add_created(st, made);
    if (last_block(&st->log_red_done) && threadIdx.x == 0) {
        *left_out = __hip_atomic_load(&st->n_overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence_system();
    }
}

hipError_t launch_reinsert_overflow(Table t, DevState* st, const Overflow* src, u64 n, u64* left_out, hipStream_t s) {
    if (!n) return hipSuccess;
    const int grid = (int)std::min<u64>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(reinsert_kernel, dim3(grid), dim3(256), 0, s, t, st, src, n, left_out);
    return hipGetLastError();
}

// move every live slot of an old table into a bigger one (keeps count/first/last_tag)
__global__ void rehash_kernel(Table t, const GSlot* src, u64 nsrc) {
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < nsrc; i += (u64)gridDim.x * blockDim.x) {
        const GSlot g = src[i];
        if (!g.key) continue;
        u64 h = table_home(g.key, t.mask);
        for (;;) {
            const u64 old = atomicCAS((unsigned long long*)&t.slots[h].key, 0ull, (unsigned long long)g.key);
            if (old == 0) {
                t.slots[h].count = g.count;
                t.slots[h].first = g.first;
                t.slots[h].last_tag = g.last_tag;
                break;
            }
            h = (h + 1) & t.mask;
        }
    }
}

hipError_t launch_rehash(Table dst, const GSlot* src, u64 nsrc, hipStream_t s) {
    const int grid = (int)std::min<u64>((nsrc + 255) / 256, 8192);
    hipLaunchKernelGGL(rehash_kernel, dim3(grid), dim3(256), 0, s, dst, src, nsrc);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// launch-log aggregation: the tally kernel's logging commits append their (code, count, first) pairs to
// the launch log's parts (commit_buffers, fr_kernels.hip; log_bucket(code)) instead of inserting each into
// the HBM table (one dependent slot load plus memory-side atomics per pair).  After the launch one
// workgroup per part folds its codes in LDS and only the distinct codes reach the HBM table -- batched,
// with every slot load in flight at once, and with plain stores: the parts partition the codes.
// ------------------------------------------------------------------------------------
// this block is the last of the grid to pass here (counter ctr, reset for the next launch); every
// block's earlier global writes are visible to the last one
__device__ __forceinline__ bool last_block(u32* ctr) {
    __shared__ u32 last;
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        const u32 prev = atomicAdd(ctr, 1u);
        last = prev == gridDim.x - 1u;
        if (last) {
            *ctr = 0;
            __threadfence();
        }
    }
    __syncthreads();
    return last != 0;
}

constexpr int AGG_PROBE = 256;  // (64 let ~20 of a 7.4-GB launch's 11M entries overflow a fold at load 0.69)
constexpr int CLAIM_WORDS = 1024;  // a reduce workgroup's claim bitmap: home ranges of up to 32K slots (4 KB; tables of up to 16 Mi slots)
struct alignas(16) AggSlot {
    u64 key;
    u32 mino, cnt;  // min launch offset (logged launches are <= RANGE_FIRST_MAX: u32), records
};

// distinct (key, count, first, last tag) rows into the HBM table in rounds: every pending row's probe
// slot is loaded together, hits take fire-and-forget atomics, empty slots are claimed by CASes issued
// together (a lane waits for max-probe-depth round trips, not the sum over its rows)
// EXCL: no other thread touches these keys' slots while this kernel runs (log_reduce_kernel's parts
// partition the keys and nothing else updates the table): a found or claimed slot takes plain stores of
// the updated count / first / tag instead of three memory-side atomics.
// A reduce workgroup's claim zone: slots [lo, hi) of its part's home range (base = the range's
// first slot) that no other workgroup's probe can reach -- every insert gives up after GPROBE probes, so
// a key homed before the range reaches at most GPROBE - 1 slots into it.  There an empty slot is claimed
// through the workgroup's LDS bitmap and written with plain stores instead of a memory-side CAS (one
// round trip and one atomic fewer per new code); elsewhere CAS as usual.  bits == nullptr: no zone.
struct ClaimZone {
    u32* bits;
    u64 base, lo, hi;
};

template <int B, bool EXCL = false>
__device__ __forceinline__ u32 insert_rows(const Table& T, DevState* st, const u64 (&key)[B], const u32 (&cnt)[B],
                                           const u64 (&ord)[B], const u32 (&tag)[B], const bool (&valid)[B],
                                           const ClaimZone& cz = ClaimZone{nullptr, 0, 0, 0}) {
    u32 h[B];
    bool pend[B];
#pragma unroll
    for (int b = 0; b < B; ++b) {
        h[b] = (u32)table_home(key[b], T.mask);
        pend[b] = valid[b];
    }
    u32 made = 0;
    for (int round = 0; round < GPROBE; ++round) {
        bool any = false;
#pragma unroll
        for (int b = 0; b < B; ++b) any |= pend[b];
        if (!any) break;
        uint4 w0[B], w1[B];
#pragma unroll
        for (int b = 0; b < B; ++b)
            if (pend[b]) {
                const GSlot* sl = &T.slots[h[b]];
                w0[b] = *(const uint4*)sl;
                w1[b] = *((const uint4*)sl + 1);
            }
        bool cas[B];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            cas[b] = false;
            if (!pend[b]) continue;
            const u64 k = ((u64)w0[b].y << 32) | w0[b].x;
            if (k == key[b]) {
                GSlot* sl = &T.slots[h[b]];
                const u64 first = ((u64)w1[b].y << 32) | w1[b].x;
                if (EXCL) {
                    const u64 c = (((u64)w0[b].w << 32) | w0[b].z) + cnt[b];
                    const u64 f = min(first, ord[b]);
                    *((uint4*)sl) = make_uint4(w0[b].x, w0[b].y, (u32)c, (u32)(c >> 32));
                    *((uint4*)sl + 1) = make_uint4((u32)f, (u32)(f >> 32), max(w1[b].z, tag[b]), w1[b].w);
                } else {
                    atomicAdd((unsigned long long*)&sl->count, (unsigned long long)cnt[b]);
                    if (ord[b] < first) atomicMin((unsigned long long*)&sl->first, (unsigned long long)ord[b]);
                    if (w1[b].z < tag[b]) atomicMax(&sl->last_tag, tag[b]);
                }
                pend[b] = false;
            } else if (k == 0) {
                if (EXCL && cz.bits && h[b] >= cz.lo && h[b] < cz.hi) {
                    const u32 bit = (u32)(h[b] - cz.base), m = 1u << (bit & 31u);
                    if (!(atomicOr(&cz.bits[bit >> 5], m) & m)) {  // ours: the whole slot, plain stores
                        GSlot* sl = &T.slots[h[b]];
                        *((uint4*)sl) = make_uint4((u32)key[b], (u32)(key[b] >> 32), cnt[b], 0u);
                        *((uint4*)sl + 1) = make_uint4((u32)ord[b], (u32)(ord[b] >> 32), tag[b], w1[b].w);
                        made += 1;
                        pend[b] = false;
                    } else {  // another lane of this workgroup took it meanwhile
                        h[b] = (u32)((h[b] + 1ull) & T.mask);
                    }
                } else {
                    cas[b] = true;
                }
            } else {
                h[b] = (u32)((h[b] + 1ull) & T.mask);
            }
        }
        u64 old[B];
#pragma unroll
        for (int b = 0; b < B; ++b)
            if (cas[b]) old[b] = atomicCAS((unsigned long long*)&T.slots[h[b]].key, 0ull, (unsigned long long)key[b]);
#pragma unroll
        for (int b = 0; b < B; ++b) {
            if (!cas[b]) continue;
            if (old[b] == 0 || old[b] == key[b]) {
                GSlot* sl = &T.slots[h[b]];
                made += old[b] == 0 ? 1u : 0u;
                if (cz.bits && old[b] == 0 && h[b] >= cz.lo && h[b] < cz.hi) {  // (a fold overflow's claim)
                    const u32 bit = (u32)(h[b] - cz.base);
                    atomicOr(&cz.bits[bit >> 5], 1u << (bit & 31u));
                }
                if (EXCL && old[b] == 0) {  // claimed an initialised slot (count 0, first ~0, tag 0): ours alone
                    *((u64*)&sl->count) = cnt[b];
                    *((uint4*)sl + 1) = make_uint4((u32)ord[b], (u32)(ord[b] >> 32), tag[b], w1[b].w);
                } else {
                    atomicAdd((unsigned long long*)&sl->count, (unsigned long long)cnt[b]);
                    atomicMin((unsigned long long*)&sl->first, (unsigned long long)ord[b]);
                    atomicMax(&sl->last_tag, tag[b]);
                }
                pend[b] = false;
            } else {
                h[b] = (u32)((h[b] + 1ull) & T.mask);
            }
        }
    }
#pragma unroll
    for (int b = 0; b < B; ++b) {
        if (!pend[b]) continue;  // probe bound exceeded: the overflow list
        const u64 i = atomicAdd((unsigned long long*)&st->n_overflow, 1ull);
        if (i < T.ovf_cap) {
            Overflow o;
            o.key = key[b];
            o.count = cnt[b];
            o.first = ord[b];
            o.tag = tag[b];
            o.pad = 0;
            T.ovf[i] = o;
        } else {
            atomicOr(&st->cap_flags, 2u);
        }
    }
    return made;
}

// One workgroup per part of the log: the part (coalesced, eight entries in flight per thread)
// folded in LDS (records summed, min offset), then its distinct codes inserted into the HBM table with
// the launch's ordinal base and file tag.  The parts partition the codes, so found and claimed
// slots take plain stores (insert_rows EXCL).  The last workgroup empties the log for the next launch.
// RED_WG threads (round 6: 512, was 256): the fold's LDS table (64 KB) allows two workgroups per CU, and
// with 256 threads that left 2 waves per SIMD to cover the entry loads' and the inserts' round trips (1 024
// threads need 114 VGPRs: one workgroup per CU, and the 512 parts would run in two rounds).
#ifndef FR_RED_WG
#define FR_RED_WG 512
#endif
constexpr int RED_WG = FR_RED_WG;
constexpr int RED_FB = RED_WG >= 512 ? 4 : 8;  // distinct codes per thread per insert batch (4: <= 128 VGPRs, two workgroups per CU)
__device__ __forceinline__ void log_reduce_fold(Table t, DevState* st, const LogEntry* log, u32 scap, u32 file_tag,
                                                u64 ord0) {
    __shared__ AggSlot ls[AGG_LNS];
    __shared__ u32 zone_bits[CLAIM_WORDS];
    __shared__ u16 occ[AGG_LNS];  // the occupied slots of ls, listed for the inserts
    __shared__ u32 occ_n;
    u32 made = 0;
    for (int i = threadIdx.x; i < AGG_LNS; i += RED_WG) ls[i] = AggSlot{0, 0xFFFFFFFFu, 0};
    // this part's home range: slots [blockIdx.x n, (blockIdx.x + 1) n) of the table (table_home's top
    // bits are log_bucket's); its claim zone skips the first GPROBE slots
    const u64 nslots = t.mask + 1ull, rn = nslots >= (u64)LOG_NSUB ? nslots / LOG_NSUB : 0ull;
    ClaimZone cz{nullptr, 0, 0, 0};
    if (rn > 2ull * GPROBE && rn <= 32ull * CLAIM_WORDS && !(ABLATE & 2048u)) {
        cz = ClaimZone{zone_bits, (u64)blockIdx.x * rn, (u64)blockIdx.x * rn + GPROBE, (u64)(blockIdx.x + 1) * rn};
        for (u32 i = threadIdx.x; i < (u32)(rn / 32); i += RED_WG) zone_bits[i] = 0;
    }
    __syncthreads();
    const u32 n = min(st->log_scur[blockIdx.x], scap);
    const LogEntry* part = log + (u64)blockIdx.x * scap;
    // a first occurrence folds as v = its ordinal's offset / 4 - the launch base's (make_ord's rounding): 32 bits
    // for launches up to 16 GiB; the ordinal is tag | (base4 + v) << 2
    const u64 base4 = (ord0 & ((1ull << ORD_SHIFT) - 1ull)) >> 2, tagpart = ord0 & ~((1ull << ORD_SHIFT) - 1ull);
    u64 sink = 0;
    constexpr int LB = 8;  // entries per thread per batch; the next batch's loads fly during this one's fold
    const u32 nn = (ABLATE & 512u) ? 0u : n;  // 512: timing ablation
    // unconditional loads (a clamped index, the key zeroed past the end): exec-masked loads made the compiler wait
    // for every outstanding load (vmcnt(0)) right after issuing the next batch, so no batch flew during a fold
    LogEntry nx[LB];
    if (nn) {
#pragma unroll
        for (int q = 0; q < LB; ++q) nx[q] = part[min(threadIdx.x + q * RED_WG, nn - 1u)];
    }
    for (u32 i0 = threadIdx.x; i0 < nn; i0 += LB * RED_WG) {
        LogEntry ev[LB];
#pragma unroll
        for (int q = 0; q < LB; ++q) {
            ev[q] = nx[q];
            nx[q] = part[min(i0 + (LB + q) * RED_WG, nn - 1u)];  // (past the end: the last entry again, skipped)
        }
#pragma unroll
        for (int q = 0; q < LB; ++q) {
            const LogEntry e = ev[q];
            if (i0 + q * RED_WG >= nn || !e.key) continue;
            if (ABLATE & 1024u) {  // timing ablation: loads only
                sink ^= e.key;
                continue;
            }
            const u32 eoff = (u32)((((ord0 & ((1ull << ORD_SHIFT) - 1ull)) + log_off(e.oc)) >> 2) - base4);
            const u32 ecnt = log_cnt(e.oc);
            // the fold's slot and probe step (double hashing: a wave waits for its lanes' longest probe chain,
            // and linear probing's clusters at the fold's ~0.7 load made that chain long); two 32-bit
            // multiplies (a part's keys share mix64's top bits, not these)
            u32 h = (u32)e.key * 0x9E3779B1u ^ (u32)(e.key >> 32) * 0x85EBCA6Bu;
            const u32 hstep = ((h >> 7) & (AGG_LNS - 1)) | 1u;
            h = (h ^ (h >> 15)) & (AGG_LNS - 1);
            bool done = false;
            for (int pr = 0; pr < AGG_PROBE && !done; ++pr) {
                const AggSlot sl = ls[h];  // key, first and count in one LDS read
                u64 k = sl.key;
                u32 mino = sl.mino;
                if (k == 0) {
                    const u64 old = atomicCAS((unsigned long long*)&ls[h].key, 0ull, (unsigned long long)e.key);
                    k = old == 0 ? e.key : old;
                    mino = old == 0 ? 0xFFFFFFFFu : ls[h].mino;
                }
                if (k == e.key) {
                    atomicAdd(&ls[h].cnt, ecnt);  // (fire-and-forget LDS atomics: no wait in the fold's chain)
                    if (eoff < mino) atomicMin(&ls[h].mino, eoff);
                    done = true;
                    break;
                }
                h = (h + hstep) & (AGG_LNS - 1);
            }
            if (!done) {  // a full LDS table: this row goes in on its own
                const u64 key1[1] = {e.key};
                const u32 cnt1[1] = {ecnt};
                const u64 ord1[1] = {tagpart | ((base4 + eoff) << 2)};
                const u32 tag1[1] = {file_tag};
                const bool v1[1] = {true};
                made += insert_rows<1>(t, st, key1, cnt1, ord1, tag1, v1, cz);
                atomicAdd(&st->log_fold_over, 1u);  // the fold was full: the next feeds keep smaller logged launches
            }
        }
    }
    if (sink == 1) atomicAdd((unsigned long long*)&st->stamp[7], 1ull);  // keeps the ablation's loads
    __syncthreads();
    // the distinct codes into the table: the occupied slots listed first (LDS), then FB of them per thread in
    // flight -- one batch of probe loads covers RED_WG * FB codes, instead of one batch per FB slots scanned
    // (half of them empty at the fold's usual load)
    if (threadIdx.x == 0) occ_n = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < AGG_LNS; i += RED_WG)
        if (ls[i].key) occ[atomicAdd(&occ_n, 1u)] = (u16)i;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(&st->log_fold_max, occ_n);  // the feed's fullest fold (fr_feed_device's launch size)
    constexpr int FB = RED_FB;
    const u32 nocc = (ABLATE & 256u) ? 0u : occ_n;  // 256: timing ablation
    for (u32 i0 = threadIdx.x; i0 < nocc; i0 += FB * RED_WG) {
        u64 key[FB], ord[FB];
        u32 cnt[FB], tag[FB];
        bool v[FB];
#pragma unroll
        for (int b = 0; b < FB; ++b) {
            const u32 j = i0 + b * RED_WG;
            v[b] = j < nocc;
            const AggSlot e = v[b] ? ls[occ[j]] : AggSlot{0, 0, 0};
            key[b] = e.key;
            cnt[b] = e.cnt;
            ord[b] = tagpart | ((base4 + e.mino) << 2);
            tag[b] = file_tag;
        }
        made += insert_rows<FB, true>(t, st, key, cnt, ord, tag, v, cz);
    }
    add_created(st, made);
}

// mir: a device feed's last launch.  The grid's last workgroup mirrors the device state as this launch
// leaves it, and the feed's last byte, into the pinned host block: the host synchronises the stream and
// reads them there, without the copy dispatches (and the idle gaps around them) of a read-back.
__global__ __launch_bounds__(RED_WG) void log_reduce_kernel(Table t, DevState* st, const LogEntry* log, u32 scap,
                                                         u32 file_tag, u64 ord0, HostMirror* mir,
                                                         const u8* last_byte) {
    const bool logged = st->log_n != 0;  // (uniform; nobody changes it before every workgroup has read it)
    if (logged) log_reduce_fold(t, st, log, scap, file_tag, ord0);
    else if (!mir) return;
    // every workgroup has read log_n and its cursor: the last one empties the log
    if (last_block(&st->log_red_done)) {
        if (logged) {
            for (int i = threadIdx.x; i < LOG_NSUB; i += RED_WG)
                __hip_atomic_store(&st->log_scur[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (threadIdx.x == 0) __hip_atomic_store(&st->log_n, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // the state's words up to the log cursors, and the fold statistics behind them: the cursors, log_n
        // and log_red_done are zero after every aggregation (the host fills them in), so one wave's stores
        // carry the mirror.  Agent-scope loads: the other workgroups updated the counters with memory-side
        // atomics, ordered before this workgroup's turn by last_block's fences.
        if (mir && threadIdx.x < 64) {
            constexpr u32 HEAD = (u32)(offsetof(DevState, log_scur) / sizeof(u32));
            static_assert(offsetof(DevState, log_scur) % sizeof(u32) == 0 && HEAD <= 64, "one wave mirrors the state's head");
            const u32* src = (const u32*)st;
            u32* dst = (u32*)&mir->st;
            constexpr u32 LOGN = (u32)(offsetof(DevState, log_n) / sizeof(u32));  // (being zeroed above: not read)
            if (threadIdx.x < HEAD)
                dst[threadIdx.x] = (threadIdx.x == LOGN || threadIdx.x == LOGN + 1) ? 0u
                                   : __hip_atomic_load(src + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (threadIdx.x == 0) {
                mir->st.log_fold_max = __hip_atomic_load(&st->log_fold_max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                mir->st.log_fold_over = __hip_atomic_load(&st->log_fold_over, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                mir->last_byte = last_byte ? (u32)*last_byte : 0u;
            }
            __threadfence_system();
        }
    }
}

hipError_t launch_log_aggregate(Table t, DevState* st, const LogEntry* log, u32 scap, u32 file_tag, u64 file_offset,
                                HostMirror* mir, const u8* last_byte, hipStream_t s) {
    // reads log_n on the device and returns at once when no commit logged (none had ScanArgs::log_min pairs)
    const u64 ord0 = ((u64)file_tag << ORD_SHIFT) | file_offset;
    hipLaunchKernelGGL(log_reduce_kernel, dim3(LOG_NSUB), dim3(RED_WG), 0, s, t, st, log, scap, file_tag, ord0,
                       mir, last_byte);
    return hipGetLastError();  // log_reduce_kernel's last block emptied the log
}

// Stream compaction of table slots with one atomic per workgroup (single-address atomics
// serialise at ~11 ns each: a per-wave append over a 4 Mi-slot table costs ~0.8 ms).  Each
// workgroup owns a contiguous slot range: pass 1 counts its hits and reserves one output
// range, pass 2 re-reads the (L2-warm) range and writes hits in slot order.
constexpr int CWG = 256;

template <class Pred>
__device__ __forceinline__ u64 block_reserve(u64 lo, u64 hi, Pred pred, u64* counter, u32* red) {
    const int tid = threadIdx.x;
    u32 mine = 0;
    for (u64 i = lo + tid; i < hi; i += CWG) mine += pred(i) ? 1u : 0u;
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = mine;
    __syncthreads();
    if (tid == 0) {
        const u32 tot = red[0] + red[1] + red[2] + red[3];
        *(u64*)&red[4] = tot ? atomicAdd((unsigned long long*)counter, (unsigned long long)tot) : 0ull;
    }
    __syncthreads();
    return *(const u64*)&red[4];
}

// calls emit(out_index, slot_index) for every hit of [lo, hi), in slot order
template <class Pred, class Emit>
__device__ __forceinline__ void block_emit(u64 lo, u64 hi, u64 base, Pred pred, Emit emit, u32* wc) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    for (u64 b = lo; b < hi; b += CWG) {
        const u64 i = b + tid;
        const bool hit = i < hi && pred(i);
        const u64 m = __ballot(hit);
        if (lane == 0) wc[wid] = (u32)__popcll(m);
        __syncthreads();
        u32 before = 0, tot = 0;
        for (int w = 0; w < CWG / 64; ++w) {
            before += w < wid ? wc[w] : 0u;
            tot += wc[w];
        }
        if (hit) emit(base + before + (u64)__popcll(m & ((1ull << lane) - 1ull)), i);
        base += tot;
        __syncthreads();
    }
}

__device__ __forceinline__ void block_range(u64 n, u64& lo, u64& hi) {
    const u64 per = (n + gridDim.x - 1) / gridDim.x;
    lo = min(n, (u64)blockIdx.x * per);
    hi = min(n, lo + per);
}

__global__ __launch_bounds__(CWG) void compact_kernel(const GSlot* slots, u64 nslots, u64* keys, u64* counts,
                                                      u64* first, u32* pos, u64* counter) {
    __shared__ u32 red[8];
    u64 lo, hi;
    block_range(nslots, lo, hi);
    auto pred = [&](u64 i) { return slots[i].key != 0; };
    const u64 base = block_reserve(lo, hi, pred, counter, red);
    block_emit(lo, hi, base, pred, [&](u64 p, u64 i) {
        const GSlot g = slots[i];
        keys[p] = g.key;
        counts[p] = g.count;
        first[p] = g.first;
        pos[p] = (u32)p;
    }, red);
}

hipError_t launch_compact(const GSlot* slots, u64 nslots, u64* keys, u64* counts, u64* first, u32* pos,
                          u64* counter, hipStream_t s) {
    const int grid = (int)std::max<u64>(1, std::min<u64>((nslots + 4095) / 4096, 2048));
    hipLaunchKernelGGL(compact_kernel, dim3(grid), dim3(CWG), 0, s, slots, nslots, keys, counts, first, pos,
                       counter);
    return hipGetLastError();
}

hipError_t launch_order(const u64* first_in, const u32* pos_in, u64 n, u64* first_out, u32* perm_out, void* temp,
                        size_t* temp_bytes, int begin_bit, int end_bit, hipStream_t s) {
    return rocprim::radix_sort_pairs(temp, *temp_bytes, first_in, first_out, pos_in, perm_out, (size_t)n,
                                     (unsigned)begin_bit, (unsigned)end_bit, s);
}

__global__ void gather_kernel(const u32* perm, u64 n, const u64* keys, const u64* counts, u64* keys_o,
                              u64* counts_o, u32* rank) {
    for (u64 j = blockIdx.x * (u64)blockDim.x + threadIdx.x; j < n; j += (u64)gridDim.x * blockDim.x) {
        const u32 p = perm[j];
        keys_o[j] = keys[p];
        counts_o[j] = counts[p];
        rank[p] = (u32)j;
    }
}

hipError_t launch_gather(const u32* perm, u64 n, const u64* keys, const u64* counts, u64* keys_o, u64* counts_o,
                         u32* rank, hipStream_t s) {
    if (!n) return hipSuccess;
    const int grid = (int)std::min<u64>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(gather_kernel, dim3(grid), dim3(256), 0, s, perm, n, keys, counts, keys_o, counts_o, rank);
    return hipGetLastError();
}

__device__ __forceinline__ const GSlot* table_find(const GSlot* slots, u64 mask, u64 key) {
    u64 h = table_home(key, mask);
    for (u64 probe = 0; probe <= mask; ++probe) {
        const GSlot* s = &slots[h];
        if (s->key == key) return s;
        if (s->key == 0) return nullptr;
        h = (h + 1) & mask;
    }
    return nullptr;
}

// write each live slot's sorted index into slot.uidx (keys in sorted order)
__global__ void set_uidx_kernel(GSlot* slots, u64 mask, const u64* keys, u64 n) {
    for (u64 j = blockIdx.x * (u64)blockDim.x + threadIdx.x; j < n; j += (u64)gridDim.x * blockDim.x) {
        GSlot* s = const_cast<GSlot*>(table_find(slots, mask, keys[j]));
        if (s) s->uidx = (u32)j;
    }
}

hipError_t launch_set_uidx(GSlot* slots, u64 mask, const u64* keys, u64 n, hipStream_t s) {
    if (!n) return hipSuccess;
    const int grid = (int)std::min<u64>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(set_uidx_kernel, dim3(grid), dim3(256), 0, s, slots, mask, keys, n);
    return hipGetLastError();
}

__global__ void presence_map_kernel(const GSlot* slots, u64 mask, const Presence* pres, u64 n, u32* uidx,
                                    u32* file_idx, u64* snap) {
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const Presence p = pres[i];
        const GSlot* s = table_find(slots, mask, p.key);
        uidx[i] = s ? s->uidx : 0xFFFFFFFFu;
        file_idx[i] = (u32)(p.tc & ((1u << PRES_TAG_BITS) - 1u)) - 1u;
        snap[i] = p.tc >> PRES_TAG_BITS;
    }
}

// The presence pairs of a scan of one file (fr_finalize when fr_end_file deferred that file's scan):
// every finalized code, in final order, present in that file with its whole count -- what
// presence_scan_kernel + presence_map_kernel would give, without the two passes over the table.
__global__ void presence_one_file_kernel(const u64* counts, u64 n, u32 tag, u32* uidx, u32* file_idx, u64* snap) {
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        uidx[i] = (u32)i;
        file_idx[i] = tag - 1u;
        snap[i] = counts[i] & ((1ull << (64 - PRES_TAG_BITS)) - 1ull);
    }
}

hipError_t launch_presence_one_file(const u64* counts, u64 n, u32 tag, u32* uidx, u32* file_idx, u64* snap,
                                    hipStream_t s) {
    if (!n) return hipSuccess;
    const int grid = (int)std::min<u64>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(presence_one_file_kernel, dim3(grid), dim3(256), 0, s, counts, n, tag, uidx, file_idx, snap);
    return hipGetLastError();
}

hipError_t launch_presence_map(const GSlot* slots, u64 mask, const Presence* pres, u64 n, u32* uidx,
                               u32* file_idx, u64* snap, hipStream_t s) {
    if (!n) return hipSuccess;
    const int grid = (int)std::min<u64>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(presence_map_kernel, dim3(grid), dim3(256), 0, s, slots, mask, pres, n, uidx, file_idx, snap);
    return hipGetLastError();
}

// ---- first-occurrence order by binning (fr_finalize, one context's own ordinals) -------------
// An ordinal is a record start; records are four terminated lines, so two ordinals of one file
// are >= 4 bytes apart and a bin of 2^shift bytes holds at most 2^(shift-2) codes (twice that
// where a bin straddles two files).  Count per bin (each slot keeps its arrival index in uidx),
// exclusive scan, scatter by bin, then each code's rank inside its bin gives its final index: the
// table is read twice and nothing is sorted globally.
__device__ __forceinline__ u64 ord_bin(const BinMap& m, u64 ord) {
    const u64 tag = ord >> ORD_SHIFT, off = ord & ((1ull << ORD_SHIFT) - 1ull);
    return min(((tag - m.first_tag) * m.span + off) >> m.shift, m.nbins - 1ull);  // clamp: never out of bounds
}

// One slot (one 32-B sector) per lane, the whole table in one grid.  Every store here is a whole
// sector or part of a coalesced run: a random 4- or 8-B store is a partial-sector write, which HBM
// turns into a read-modify-write (the first version of these kernels stored into table slots and
// ran at half the speed).
__global__ __launch_bounds__(256) void fin_hist_kernel(const GSlot* slots, u64 n, BinMap m, u32* cnt, u32* arr) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 w0 = *(const uint4*)&slots[i];
    const uint4 w1 = *((const uint4*)&slots[i] + 1);
    u32 v = 0xFFFFFFFFu;
    if ((w0.x | w0.y) != 0u) v = atomicAdd(&cnt[ord_bin(m, ((u64)w1.y << 32) | w1.x)], 1u);
    arr[i] = v;  // arrival index in the bin (coalesced: every lane stores)
}

// each live slot's row {ordinal, key, count, slot} to its bin's run, one 32-B sector per row
__global__ __launch_bounds__(256) void fin_scatter_kernel(const GSlot* slots, u64 n, BinMap m, const u32* base,
                                                          const u32* arr, FinRow* rows, u32* cnt, u64* fin_out) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    // the bin counts' last reader (the scan) is done: zero them for the next fr_finalize, which then needs no
    // memset dispatch (a lane per slot: one round wherever the table has more slots than bins); and the scan's
    // last entry, the live-slot count fr_finalize checks, straight into pinned host memory
    for (u64 j = i; j <= m.nbins; j += (u64)gridDim.x * blockDim.x) cnt[j] = 0;
    if (i == 0 && fin_out) {
        *fin_out = base[m.nbins];
        __threadfence_system();
    }
    if (i >= n) return;
    const u32 k = arr[i];
    if (k == 0xFFFFFFFFu) return;
    const uint4 w0 = *(const uint4*)&slots[i];
    const uint4 w1 = *((const uint4*)&slots[i] + 1);
    const u64 first = ((u64)w1.y << 32) | w1.x;
    const u32 q = base[ord_bin(m, first)] + k;
    if (q < m.cap) {
        typedef u32 u32x4 __attribute__((ext_vector_type(4)));
        u32x4* d = (u32x4*)&rows[q];
        d[0] = u32x4{w1.x, w1.y, w0.x, w0.y};
        d[1] = u32x4{w0.z, w0.w, (u32)i, 0u};
    }
}

// final index = the bin's base + the codes of the bin with a smaller ordinal (ties: slot index,
// never met for one context's ordinals); the row goes there and the slot's uidx becomes that index
__global__ __launch_bounds__(256) void fin_rank_kernel(GSlot* slots, u64 nk, BinMap m, const u32* base,
                                                       const FinRow* rows, u64* keys_o, u64* counts_o, u64* first_o,
                                                       int set_uidx) {
    const u64 q = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (q >= nk) return;
    const FinRow row = rows[q];
    const u64 b = ord_bin(m, row.first);
    const u32 lo = base[b], hi = (u32)min((u64)base[b + 1], m.cap);
    u32 r = 0;
    for (u32 j = lo; j < hi; ++j) {
        const u64 fj = rows[j].first;
        r += (fj < row.first || (fj == row.first && rows[j].slot < row.slot)) ? 1u : 0u;
    }
    const u32 out = lo + r;
    if (out >= nk) return;  // only when the live count disagrees with n_keys (fr_finalize fails then)
    keys_o[out] = row.key;
    counts_o[out] = row.count;
    first_o[out] = row.first;
    if (set_uidx) slots[row.slot].uidx = out;  // read only by presence_map_kernel (a random partial-sector store)
}

static unsigned lane_grid(u64 n) { return (unsigned)std::max<u64>(1, (n + 255) / 256); }

hipError_t launch_fin_hist(const GSlot* slots, u64 nslots, const BinMap& m, u32* cnt, u32* arr, hipStream_t s) {
    hipLaunchKernelGGL(fin_hist_kernel, dim3(lane_grid(nslots)), dim3(256), 0, s, slots, nslots, m, cnt, arr);
    return hipGetLastError();
}

// exclusive scan of cnt[0, n) into base[0, n) (temp = nullptr: size query)
hipError_t launch_fin_scan(const u32* cnt, u32* base, u64 n, void* temp, size_t* temp_bytes, hipStream_t s) {
    return rocprim::exclusive_scan(temp, *temp_bytes, cnt, base, 0u, (size_t)n, rocprim::plus<u32>(), s);
}

hipError_t launch_fin_scatter(const GSlot* slots, u64 nslots, const BinMap& m, const u32* base, const u32* arr,
                              FinRow* rows, u32* cnt, u64* fin_out, hipStream_t s) {
    hipLaunchKernelGGL(fin_scatter_kernel, dim3(lane_grid(nslots)), dim3(256), 0, s, slots, nslots, m, base, arr, rows,
                       cnt, fin_out);
    return hipGetLastError();
}

hipError_t launch_fin_rank(GSlot* slots, u64 nk, const BinMap& m, const u32* base, const FinRow* rows, u64* keys_o,
                           u64* counts_o, u64* first_o, bool set_uidx, hipStream_t s) {
    if (!nk) return hipSuccess;
    hipLaunchKernelGGL(fin_rank_kernel, dim3(lane_grid(nk)), dim3(256), 0, s, slots, nk, m, base, rows, keys_o,
                       counts_o, first_o, set_uidx ? 1 : 0);
    return hipGetLastError();
}

// merge another GPU's compacted table into this one (count +, first min); presence of
// remote keys travels separately (fr_get_presence on each rank)
__global__ void merge_kernel(Table t, DevState* st, const u64* keys, const u64* counts, const u64* first, u64 n) {
    u32 made = 0;
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x)
        made += global_insert(t, st, keys[i], counts[i], first[i], 0u) ? 1u : 0u;
    add_created(st, made);
}

// the multi-GPU merge's send side: the finalized rows (key, count, first) partitioned by owner rank
// (owner = the top 24 bits of key * 0x9E3779B97F4A7C15 mod world, frender_amd/dist.py owner_of), row-major,
// owner blocks contiguous.  Pass 1 counts per owner (an LDS histogram per workgroup, one atomic per
// (workgroup, owner)); pass 2 gives each workgroup's rows of an owner a run claimed from that owner's cursor
// (cursors start at the owners' exclusive prefix).  Order inside a block is not fixed: the merge is commutative.
constexpr int PART_MAX = 1024;  // ranks
__device__ __forceinline__ u32 owner_rank(u64 key, u32 world) {
    return (u32)(((key * 0x9E3779B97F4A7C15ull) >> 40) & 0xFFFFFFull) % world;
}
__global__ __launch_bounds__(256) void part_count_kernel(const u64* keys, u64 n, u32 world, u64* counts) {
    __shared__ u32 h[PART_MAX];
    for (u32 i = threadIdx.x; i < world; i += 256) h[i] = 0;
    __syncthreads();
    for (u64 i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (u64)gridDim.x * 256ull) atomicAdd(&h[owner_rank(keys[i], world)], 1u);
    __syncthreads();
    for (u32 i = threadIdx.x; i < world; i += 256)
        if (h[i]) atomicAdd((unsigned long long*)&counts[i], (unsigned long long)h[i]);
}
__global__ __launch_bounds__(256) void part_scatter_kernel(const u64* keys, const u64* counts_in, const u64* first,
                                                          u64 n, u32 world, const u64* counts, u64* cursor, u64* rows) {
    __shared__ u32 h[PART_MAX];
    __shared__ u64 base[PART_MAX];
    for (u32 i = threadIdx.x; i < world; i += 256) h[i] = 0;
    __syncthreads();
    const u64 stride = (u64)gridDim.x * 256ull;
    for (u64 i = blockIdx.x * 256ull + threadIdx.x; i < n; i += stride) atomicAdd(&h[owner_rank(keys[i], world)], 1u);
    __syncthreads();
    if (threadIdx.x == 0) {  // cursors start at the exclusive prefix of the counts (the first claim of each sets it)
        u64 pre = 0;
        for (u32 r = 0; r < world; ++r) {
            base[r] = h[r] ? pre + atomicAdd((unsigned long long*)&cursor[r], (unsigned long long)h[r]) : 0ull;
            pre += counts[r];
            h[r] = 0;
        }
    }
    __syncthreads();
    for (u64 i = blockIdx.x * 256ull + threadIdx.x; i < n; i += stride) {
        const u64 k = keys[i];
        const u32 r = owner_rank(k, world);
        const u64 at = base[r] + atomicAdd(&h[r], 1u);
        rows[3 * at] = k;
        rows[3 * at + 1] = counts_in[i];
        rows[3 * at + 2] = first[i];
    }
}
// merge rows (key, count, first), row-major, into the table (count +, first min)
__global__ void merge_rows_kernel(Table t, DevState* st, const u64* rows, u64 n) {
    u32 made = 0;
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x)
        made += global_insert(t, st, rows[3 * i], rows[3 * i + 1], rows[3 * i + 2], 0u) ? 1u : 0u;
    add_created(st, made);
}
hipError_t launch_partition_rows(const u64* keys, const u64* counts_in, const u64* first, u64 n, u32 world,
                                 u64* counts, u64* cursor, u64* rows, hipStream_t s) {
    if (world < 1 || world > (u32)PART_MAX) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(counts, 0, 2ull * world * sizeof(u64), s);  // counts and cursors (adjacent)
    if (e != hipSuccess || !n) return e;
    const int grid = (int)std::min<u64>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(part_count_kernel, dim3(grid), dim3(256), 0, s, keys, n, world, counts);
    hipLaunchKernelGGL(part_scatter_kernel, dim3(grid), dim3(256), 0, s, keys, counts_in, first, n, world, counts,
                       cursor, rows);
    return hipGetLastError();
}
hipError_t launch_merge_rows(Table t, DevState* st, const u64* rows, u64 n, hipStream_t s) {
    if (!n) return hipSuccess;
    const int grid = (int)std::min<u64>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(merge_rows_kernel, dim3(grid), dim3(256), 0, s, t, st, rows, n);
    return hipGetLastError();
}

// per-file presence (R10) and the per-file distinct-code count (frender.py:175): after a
// file, exactly the slots whose last_tag is that file's tag hold a code seen in it.  Each pair keeps
// the code's running count (its per-file count is the difference to the code's previous pair).  A workgroup
// takes PS_K x 256 consecutive slots, one slot per lane per step with all the loads in flight
// together, reserves its output run with one atomic and writes its hits in slot order.
constexpr int PS_K = 16;
__global__ __launch_bounds__(CWG) void presence_scan_kernel(const GSlot* slots, u64 n, u32 tag, Presence* pres,
                                                            u64 cap, DevState* st) {
    __shared__ u32 wc[PS_K * (CWG / 64)];
    __shared__ u64 bbase;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const u64 b0 = (u64)blockIdx.x * (PS_K * CWG);
    u32 hits = 0;
#pragma unroll
    for (int k = 0; k < PS_K; ++k) {
        const u64 i = b0 + (u64)k * CWG + tid;
        if (i < n) {
            const uint2 key = *(const uint2*)&slots[i];
            const u32 lt = slots[i].last_tag;
            hits |= ((key.x | key.y) != 0u && lt == tag) ? (1u << k) : 0u;
        }
    }
    u64 m[PS_K];
#pragma unroll
    for (int k = 0; k < PS_K; ++k) {
        m[k] = __ballot((hits >> k) & 1u);
        if (lane == 0) wc[k * (CWG / 64) + wid] = (u32)__popcll(m[k]);
    }
    __syncthreads();
    if (tid == 0) {  // exclusive scan over (step, wave) = slot order, and the block's output run
        u32 run = 0;
        for (int j = 0; j < PS_K * (CWG / 64); ++j) {
            const u32 c = wc[j];
            wc[j] = run;
            run += c;
        }
        bbase = run ? atomicAdd((unsigned long long*)&st->n_presence, (unsigned long long)run) : 0ull;
    }
    __syncthreads();
    if (!hits) return;
    const u64 below = (1ull << lane) - 1ull;
#pragma unroll
    for (int k = 0; k < PS_K; ++k) {
        if ((hits >> k) & 1u) {
            const u64 kk = bbase + wc[k * (CWG / 64) + wid] + (u64)__popcll(m[k] & below);
            if (kk < cap) {
                const GSlot* sl = &slots[b0 + (u64)k * CWG + tid];
                pres[kk].key = sl->key;
                pres[kk].tc = (sl->count << PRES_TAG_BITS) | (u64)tag;  // count mod 2^44, file tag
            } else {
                atomicOr(&st->cap_flags, 1u);
            }
        }
    }
}

hipError_t launch_presence_scan(const GSlot* slots, u64 n, u32 tag, Presence* pres, u64 cap, DevState* st,
                                hipStream_t s) {
    const int grid = (int)std::max<u64>(1, (n + PS_K * CWG - 1) / (PS_K * CWG));
    hipLaunchKernelGGL(presence_scan_kernel, dim3(grid), dim3(CWG), 0, s, slots, n, tag, pres, cap, st);
    return hipGetLastError();
}

hipError_t launch_merge(Table t, DevState* st, const u64* keys, const u64* counts, const u64* first, u64 n,
                        hipStream_t s) {
    if (!n) return hipSuccess;
    const int grid = (int)std::min<u64>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(merge_kernel, dim3(grid), dim3(256), 0, s, t, st, keys, counts, first, n);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// SYN-v1 generator (byte-identical to frender_amd/synth.py generate_records)
// ------------------------------------------------------------------------------------
__device__ __forceinline__ u64 syn_h(u64 base, u64 r, u32 k) { return mix64(((r << 8) | k) ^ base); }

__global__ void synth_kernel(u8* out, u64 r0, u64 n, int R, u64 base, const u8* idx1, const u8* idx2, int S, int L1,
                             int L2) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 r = r0 + i;
    const int reclen = 36 + L1 + 1 + L2 + 1 + 2 * R + 4;
    u8* o = out + i * (u64)reclen;
    const char* ACGT = "ACGT";
    u8 idx[64];
    const u64 s = syn_h(base, r, 0) % (u64)S;
    for (int j = 0; j < L1; ++j) idx[j] = idx1[s * L1 + j];
    for (int j = 0; j < L2; ++j) idx[L1 + j] = idx2[s * L2 + j];
    if (syn_h(base, r, 1) % 10000ull < 200ull) {
        const u64 s2 = syn_h(base, r, 2) % (u64)S;
        for (int j = 0; j < L2; ++j) idx[L1 + j] = idx2[s2 * L2 + j];
    }
    if (syn_h(base, r, 3) % 10000ull < 100ull) {
        const u64 hj = syn_h(base, r, 4);
        for (int j = 0; j < L1 + L2; ++j) idx[j] = ACGT[(hj >> (2 * j)) & 3ull];
    }
    for (int j = 0; j < L1 + L2; ++j) {
        const u64 v = syn_h(base, r, 8 + j);
        const u64 p = v % 10000ull;
        if (p < 50ull) {
            const u8 c = idx[j];
            const u64 orig = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 0;
            idx[j] = ACGT[(orig + 1ull + (v >> 32) % 3ull) % 4ull];
        } else if (p < 70ull) {
            idx[j] = 'N';
        }
    }
    int pos = 0;
    const char* h0 = "@SYN:1:FCX:1:";
    for (int k = 0; k < 13; ++k) o[pos++] = h0[k];
    u64 v = (r / 10000000000ull) % 10000ull;
    for (int k = 3; k >= 0; --k) { o[pos + k] = '0' + (u8)(v % 10ull); v /= 10ull; }
    pos += 4;
    o[pos++] = ':';
    v = (r / 100000ull) % 100000ull;
    for (int k = 4; k >= 0; --k) { o[pos + k] = '0' + (u8)(v % 10ull); v /= 10ull; }
    pos += 5;
    o[pos++] = ':';
    v = r % 100000ull;
    for (int k = 4; k >= 0; --k) { o[pos + k] = '0' + (u8)(v % 10ull); v /= 10ull; }
    pos += 5;
    const char* h1 = " 1:N:0:";
    for (int k = 0; k < 7; ++k) o[pos++] = h1[k];
    for (int j = 0; j < L1; ++j) o[pos++] = idx[j];
    o[pos++] = '+';
    for (int j = 0; j < L2; ++j) o[pos++] = idx[L1 + j];
    o[pos++] = '\n';
    for (int w = 0; w < (R + 31) / 32; ++w) {
        const u64 hv = syn_h(base, r, 80 + w);
        for (int j = 32 * w; j < R && j < 32 * w + 32; ++j) o[pos + j] = ACGT[(hv >> (2 * (j - 32 * w))) & 3ull];
    }
    pos += R;
    o[pos++] = '\n';
    o[pos++] = '+';
    o[pos++] = '\n';
    for (int w = 0; w < (R + 7) / 8; ++w) {
        const u64 hv = syn_h(base, r, 100 + w);
        for (int j = 8 * w; j < R && j < 8 * w + 8; ++j) o[pos + j] = (u8)(((hv >> (8 * (j - 8 * w))) & 0xFFull) % 42ull) + 33;
    }
    pos += R;
    o[pos++] = '\n';
}

hipError_t launch_synth(u8* out, u64 r0, u64 n, int R, u64 seed, const u8* idx1, const u8* idx2, int S, int L1,
                        int L2, hipStream_t s) {
    if (!n) return hipSuccess;
    const u64 base = mix64(seed + 0x9E3779B97F4A7C15ull);
    const u64 grid = (n + 255) / 256;
    hipLaunchKernelGGL(synth_kernel, dim3((u32)grid), dim3(256), 0, s, out, r0, n, R, base, idx1, idx2, S, L1, L2);
    return hipGetLastError();
}

}  // namespace fr
