// fr_table_dev.h — device code of both kernel files: the tally (fr_kernels.hip) and the table kernels (fr_table.hip)
// insert into one HBM table and read one ablation switch.  Device-only: fr_gz.cpp includes fr_internal.h as plain C++.
#pragma once
#include "fr_internal.h"

namespace fr {

// Timing ablations exist only in experiment builds: scripts/build_exp.sh NAME
// "-DFR_ABLATE=<bits>" (1 no header parse, 2 no code encode, 4 no LDS insert, 8 no commit flush,
// 16 no cold-list entry stores after the context's third launch (the commits read the entries those left: wrong
// counts), 64 commit counts, 128 plain stores in the commit (wrong counts), 256/512/1024/2048 launch-log passes).
// The product build has FR_ABLATE = 0: every ablation branch folds away at compile time, and nothing
// read at run time (no environment variable, no kernel argument) can select one.
#ifndef FR_ABLATE
#define FR_ABLATE 0
#endif
constexpr u32 ABLATE = FR_ABLATE;

// Home slot of a key: the TOP bits of mix64(key).  A key's launch-log part (log_bucket) is the top bits of
// the same word, so in a table of >= LOG_NSUB slots each part owns one contiguous slot range and
// log_reduce_kernel's inserts stay inside it (DRAM-page and L2 locality instead of random lines).
__device__ __forceinline__ u64 table_home(u64 key, u64 mask) {
    return mask ? mix64(key) >> __builtin_clzll(mask) : 0ull;
}

// ------------------------------------------------------------------------------------
// HBM table insert: count add, first-occurrence min, last file tag (presence is derived per
// file by presence_scan_kernel).  One 32-B slot load decides; the count add is
// fire-and-forget and the min/max atomics run only when they can change the slot (a stale
// load only ever over-estimates `first` / under-estimates `last_tag`, so skipping is safe).
// Returns true when this call created the slot.  No global counters are touched here.
// ------------------------------------------------------------------------------------
__device__ inline bool global_insert(const Table& T, DevState* st, u64 key, u64 cnt, u64 ord, u32 tag) {
    u64 h = table_home(key, T.mask);
    for (int probe = 0; probe < GPROBE; ++probe) {
        GSlot* s = &T.slots[h];
        const uint4 w0 = *(const uint4*)s;
        const uint4 w1 = *((const uint4*)s + 1);
        u64 k = ((u64)w0.y << 32) | w0.x;
        u64 first = ((u64)w1.y << 32) | w1.x;
        u32 ltag = w1.z;
        bool created = false;
        if (k == 0) {
            const u64 old = atomicCAS((unsigned long long*)&s->key, 0ull, (unsigned long long)key);
            created = old == 0;
            k = created ? key : old;
            first = ~0ull;
            ltag = 0;
        }
        if (k == key) {
            atomicAdd((unsigned long long*)&s->count, (unsigned long long)cnt);
            if (ord < first) atomicMin((unsigned long long*)&s->first, (unsigned long long)ord);
            if (ltag < tag) atomicMax(&s->last_tag, tag);
            return created;
        }
        h = (h + 1) & T.mask;
    }
    const u64 i = atomicAdd((unsigned long long*)&st->n_overflow, 1ull);
    if (i < T.ovf_cap) {
        Overflow o;
        o.key = key;
        o.count = cnt;
        o.first = ord;
        o.tag = tag;
        o.pad = 0;
        T.ovf[i] = o;
    } else {
        atomicOr(&st->cap_flags, 2u);
    }
    return false;
}

// block-wide count of created slots -> one global add per wave
__device__ __forceinline__ void add_created(DevState* st, u32 mine) {
    u64 v = mine;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd((unsigned long long*)&st->n_keys, (unsigned long long)v);
}

}  // namespace fr
