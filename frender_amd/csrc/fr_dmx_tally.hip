// fr_dmx_tally.hip — the tally of `demux -b SHEET -n N --report`: the scan's count of every distinct code
// (tally_barcodes, frender.py:183-207, and scan_file's per-file table, :171-177), taken over the record keys
// the one-pass demux already has in HBM.
//
// In sheet mode dmx_index (fr_demux.hip) leaves every R2 record's fast key in rec_key; once fr_dmx_route has
// routed a window's first n_pairs records, dmx_tally_window counts exactly those keys into an open-addressing
// table in HBM (TSlot: key, total, first ordinal, reads in the current file pair).  A few sample codes take
// most of the reads, so a workgroup first accumulates (key, count, min record) in an LDS table and sends each
// occupied slot to HBM once, when its grid-stride loop is done; a key that finds no LDS slot within TLPROBE
// probes goes to HBM on its own.  At the end of a file pair dmx_tally_drain appends (key, file, cur) for every
// slot with cur > 0 to the presence list, adds cur to total and zeroes it: the reference's per-file tables,
// barcode_counter[basename][code], at one pass over the table per pair.  The host side below keeps the table at
// twice the keys it may hold after the next window (the count of distinct keys comes back with the syncs
// the demux makes anyway) and rebuilds it larger on the device otherwise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/frender_amd.h"
#include "fr_internal.h"

namespace fr {
namespace {

constexpr int TWG = 256;           // lanes per workgroup
constexpr int TNS = 1024;          // LDS slots per workgroup: 16 KiB (key 8, count 4, min record 4), so the 160 KiB
                                   // of a CU hold the 8 workgroups of 256 lanes its wave slots allow
constexpr int TLPROBE = 4;         // LDS probe bound before a key goes to HBM on its own
constexpr int TPER = 16;           // records per lane before the grid gets another workgroup: a workgroup's flush
                                   // (<= TNS HBM updates) stands against >= 4096 records
constexpr u64 TSLOTS_DEFAULT = 1ull << 16;
constexpr u64 TSLOTS_MIN = 64;
constexpr int TFILE_BITS = 19;     // file indices: (file + 1) << ORD_SHIFT stays below 2^63
constexpr u64 TREC_MAX = 1ull << ORD_SHIFT;  // records of one file pair

struct alignas(32) TSlot {         // one 32-B sector
    u64 key;                       // 0 = empty
    u64 total;                     // reads in the file pairs closed so far
    u64 first;                     // min ordinal, ~0 = none
    u64 cur;                       // reads in the current file pair
};

struct TPres {                     // one (code, file pair) entry: the reads of the code in that pair
    u64 key, file, reads;
};

struct TState {
    u64 n_keys;                    // occupied slots
    u64 n_pres;                    // presence entries claimed (may exceed the list's capacity: then full is set)
    u64 n_rows;                    // dmx_tally_rows' cursor
    u32 full;                      // a probe ran round the whole table, or the presence list was full
    u32 pad;
};

// count = sum into cur, first = min.  The probe is bounded by the table's size: a full table sets st->full
// (the host returns FR_ERR_CAPACITY) instead of spinning; the host keeps the table at most half full.
__device__ __forceinline__ void tally_upsert(TSlot* slots, u64 mask, TState* st, u64 key, u64 cnt, u64 ord) {
    u64 h = mix64(key) & mask;
    for (u64 p = 0; p <= mask; ++p) {
        u64 k = slots[h].key;  // a key never changes once set; a stale 0 is settled by the CAS
        if (k == 0) {
            k = atomicCAS((unsigned long long*)&slots[h].key, 0ull, (unsigned long long)key);
            if (k == 0) atomicAdd((unsigned long long*)&st->n_keys, 1ull);
        }
        if (k == 0 || k == key) {
            atomicAdd((unsigned long long*)&slots[h].cur, (unsigned long long)cnt);
            atomicMin((unsigned long long*)&slots[h].first, (unsigned long long)ord);
            return;
        }
        h = (h + 1) & mask;
    }
    atomicOr(&st->full, 1u);
}

__global__ __launch_bounds__(TWG) void dmx_tally_init(TSlot* slots, u64 n) {
    for (u64 i = blockIdx.x * (u64)TWG + threadIdx.x; i < n; i += (u64)gridDim.x * TWG)
        slots[i] = TSlot{0ull, 0ull, ~0ull, 0ull};
}

// records [0, n) of the window; record i's ordinal is ord0 + i (n < 2^32: fr_dmx_route's bound)
__global__ __launch_bounds__(TWG) void dmx_tally_window_kernel(const u64* __restrict__ rec_key, u64 n, u64 ord0,
                                                               TSlot* slots, u64 mask, TState* st) {
    __shared__ u64 lkey[TNS];
    __shared__ u32 lcnt[TNS];
    __shared__ u32 lmin[TNS];
    const int tid = threadIdx.x;
    for (int s = tid; s < TNS; s += TWG) {
        lkey[s] = 0ull;
        lcnt[s] = 0u;
        lmin[s] = ~0u;
    }
    __syncthreads();
    for (u64 i = blockIdx.x * (u64)TWG + tid; i < n; i += (u64)gridDim.x * TWG) {
        const u64 key = rec_key[i];
        // 0 marks a record dmx_index reported as FR_DMX_EXOTIC (the host counts those by string); no fast code
        // packs to 0: a code that gets a key is not empty and its symbols are 1..6
        if (key == 0) continue;
        u32 h = (u32)(mix64(key) >> 40) & (TNS - 1);  // (the HBM table takes the low bits)
        bool done = false;
#pragma unroll
        for (int p = 0; p < TLPROBE; ++p) {
            const u64 old = atomicCAS((unsigned long long*)&lkey[h], 0ull, (unsigned long long)key);
            if (old == 0 || old == key) {
                atomicAdd(&lcnt[h], 1u);
                atomicMin(&lmin[h], (u32)i);
                done = true;
                break;
            }
            h = (h + 1) & (TNS - 1);
        }
        if (!done) tally_upsert(slots, mask, st, key, 1, ord0 + i);
    }
    __syncthreads();
    for (int s = tid; s < TNS; s += TWG) {
        const u64 key = lkey[s];
        if (key) tally_upsert(slots, mask, st, key, lcnt[s], ord0 + lmin[s]);
    }
}

// `mine` lanes of the wave each claim one entry of a list whose cursor is *cursor: one atomic per wave
__device__ __forceinline__ u64 wave_claim(bool mine, u64* cursor) {
    const u64 m = __ballot(mine);
    if (!m) return 0;
    const int lane = threadIdx.x & 63, leader = __ffsll((unsigned long long)m) - 1;
    u64 base = 0;
    if (lane == leader) base = atomicAdd((unsigned long long*)cursor, (unsigned long long)__popcll(m));
    base = __shfl(base, leader, 64);
    return base + __popcll(m & ((1ull << lane) - 1ull));
}

// the end of file pair `file`: every slot with reads in it -> presence entry, cur into total
__global__ __launch_bounds__(TWG) void dmx_tally_drain(TSlot* slots, u64 nslots, u64 file, TPres* pres, u64 cap,
                                                       TState* st) {
    for (u64 b = blockIdx.x * (u64)TWG; b < nslots; b += (u64)gridDim.x * TWG) {  // wave-uniform trip count
        const u64 i = b + threadIdx.x;
        const u64 c = i < nslots ? slots[i].cur : 0ull;
        const u64 at = wave_claim(c != 0, &st->n_pres);
        if (!c) continue;
        if (at < cap) {
            pres[at] = TPres{slots[i].key, file, c};
            slots[i].total += c;
            slots[i].cur = 0;
        } else {
            atomicOr(&st->full, 1u);
        }
    }
}

// the occupied slots as int64 rows (key, count, first), in no fixed order (every pair is closed: count = total)
__global__ __launch_bounds__(TWG) void dmx_tally_rows(const TSlot* slots, u64 nslots, u64* rows, u64 cap, TState* st) {
    for (u64 b = blockIdx.x * (u64)TWG; b < nslots; b += (u64)gridDim.x * TWG) {
        const u64 i = b + threadIdx.x;
        const u64 key = i < nslots ? slots[i].key : 0ull;
        const u64 at = wave_claim(key != 0, &st->n_rows);
        if (!key) continue;
        if (at < cap) {
            rows[3 * at] = key;
            rows[3 * at + 1] = slots[i].total;
            rows[3 * at + 2] = slots[i].first;
        } else {
            atomicOr(&st->full, 1u);
        }
    }
}

// the rebuild: every occupied slot of src into the (initialised, larger) dst; keys are distinct
__global__ __launch_bounds__(TWG) void dmx_tally_rehash(const TSlot* src, u64 nsrc, TSlot* dst, u64 dmask, TState* st) {
    for (u64 i = blockIdx.x * (u64)TWG + threadIdx.x; i < nsrc; i += (u64)gridDim.x * TWG) {
        const TSlot s = src[i];
        if (!s.key) continue;
        u64 h = mix64(s.key) & dmask;
        bool placed = false;
        for (u64 p = 0; p <= dmask; ++p) {
            if (atomicCAS((unsigned long long*)&dst[h].key, 0ull, (unsigned long long)s.key) == 0ull) {
                dst[h].total = s.total;
                dst[h].first = s.first;
                dst[h].cur = s.cur;
                placed = true;
                break;
            }
            h = (h + 1) & dmask;
        }
        if (!placed) atomicOr(&st->full, 1u);
    }
}

int grid_over(u64 n, u64 per, int cap) {
    return (int)std::max<u64>(1, std::min<u64>((n + per - 1) / per, (u64)cap));
}

}  // namespace

struct DmxTally {
    int device = 0;
    hipStream_t stream = nullptr;
    int max_grid = 1024;           // CUs x 8 workgroups
    TSlot* slots = nullptr;
    u64 nslots = 0;
    TPres* pres = nullptr;
    u64 pres_cap = 0;
    TState* st = nullptr;          // device
    TState* h_st = nullptr;        // pinned: the state after the last kernel, copied behind it in stream order
    u64* rows = nullptr;           // dmx_tally_get's rows
    u64 rows_cap = 0;
    bool file_open = false;
    u64 file = 0;
    i64 last_file = -1;
};

#define TK(x)                                                                  \
    do {                                                                       \
        hipError_t e_ = (x);                                                   \
        if (e_ != hipSuccess) {                                                \
            err = std::string(#x) + ": " + hipGetErrorString(e_);              \
            return FR_ERR_HIP;                                                 \
        }                                                                      \
    } while (0)

static u64 pow2_from(u64 x, u64 from) {
    u64 p = from;
    while (p < x) p <<= 1;
    return p;
}

static int snapshot(DmxTally* t, std::string& err) {  // lands with the stream's next synchronisation
    TK(hipMemcpyAsync(t->h_st, t->st, sizeof(TState), hipMemcpyDeviceToHost, t->stream));
    return FR_OK;
}

static int check_full(DmxTally* t, std::string& err) {
    if (!t->h_st->full) return FR_OK;
    err = "fr_dmx_tally: the table or the presence list was full (the counts are not valid)";
    return FR_ERR_CAPACITY;
}

// the table rebuilt with `ns` slots (stream-ordered; the old one is freed once the rehash has run)
static int rebuild(DmxTally* t, u64 ns, std::string& err) {
    if (ns > (1ull << 40) / sizeof(TSlot)) return err = "fr_dmx_tally: more distinct codes than the table can hold", FR_ERR_CAPACITY;
    TSlot* fresh = nullptr;
    TK(hipMalloc((void**)&fresh, ns * sizeof(TSlot)));
    hipLaunchKernelGGL(dmx_tally_init, dim3(grid_over(ns, TWG, t->max_grid)), dim3(TWG), 0, t->stream, fresh, ns);
    TK(hipGetLastError());
    if (t->slots) {
        hipLaunchKernelGGL(dmx_tally_rehash, dim3(grid_over(t->nslots, TWG, t->max_grid)), dim3(TWG), 0, t->stream,
                           (const TSlot*)t->slots, t->nslots, fresh, ns - 1, t->st);
        TK(hipGetLastError());
        TK(hipStreamSynchronize(t->stream));
        TK(hipFree(t->slots));
    }
    t->slots = fresh;
    t->nslots = ns;
    return FR_OK;
}

void dmx_tally_destroy(DmxTally* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    void* p[] = {t->slots, t->pres, t->st, t->rows};
    for (void* x : p)
        if (x) (void)hipFree(x);
    if (t->h_st) (void)hipHostFree(t->h_st);
    delete t;
}

int dmx_tally_begin(DmxTally** out, int device, hipStream_t stream, u64 initial_slots, std::string& err) {
    dmx_tally_destroy(*out);
    *out = nullptr;
    DmxTally* t = new DmxTally();
    *out = t;  // (freed by the owner's destroy if a step below fails)
    t->device = device;
    t->stream = stream;
    int cus = 0;
    TK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    t->max_grid = std::max(cus, 1) * 8;
    TK(hipMalloc((void**)&t->st, sizeof(TState)));
    TK(hipHostMalloc((void**)&t->h_st, sizeof(TState), hipHostMallocDefault));
    *t->h_st = TState{};
    TK(hipMemsetAsync(t->st, 0, sizeof(TState), stream));
    t->pres_cap = 1024;
    TK(hipMalloc((void**)&t->pres, t->pres_cap * sizeof(TPres)));
    return rebuild(t, pow2_from(initial_slots ? initial_slots : TSLOTS_DEFAULT, TSLOTS_MIN), err);
}

// every entry the drain may append fits: one per occupied slot at the most
static int ensure_presence(DmxTally* t, std::string& err) {
    const u64 used = t->h_st->n_pres, need = used + t->h_st->n_keys;
    if (need <= t->pres_cap) return FR_OK;
    const u64 ncap = pow2_from(need + need / 2, t->pres_cap);
    TPres* fresh = nullptr;
    TK(hipMalloc((void**)&fresh, ncap * sizeof(TPres)));
    if (used) TK(hipMemcpyAsync(fresh, t->pres, used * sizeof(TPres), hipMemcpyDeviceToDevice, t->stream));
    TK(hipStreamSynchronize(t->stream));
    TK(hipFree(t->pres));
    t->pres = fresh;
    t->pres_cap = ncap;
    return FR_OK;
}

// close the open file pair: one synchronisation per pair (the exact state), then the drain
static int close_pair(DmxTally* t, std::string& err) {
    if (!t->file_open) return FR_OK;
    TK(hipStreamSynchronize(t->stream));
    if (int rc = check_full(t, err)) return rc;
    if (int rc = ensure_presence(t, err)) return rc;
    hipLaunchKernelGGL(dmx_tally_drain, dim3(grid_over(t->nslots, TWG, t->max_grid)), dim3(TWG), 0, t->stream, t->slots,
                       t->nslots, t->file, t->pres, t->pres_cap, t->st);
    TK(hipGetLastError());
    t->file_open = false;
    return snapshot(t, err);
}

int dmx_tally_file(DmxTally* t, i64 file_index, std::string& err) {
    if (file_index < 0 || file_index >= (1ll << TFILE_BITS) || file_index <= t->last_file)
        return err = "fr_dmx_tally_file: file indices increase from 0 and stay below 2^19", FR_ERR_INVALID;
    if (int rc = close_pair(t, err)) return rc;
    t->file = (u64)file_index;
    t->last_file = file_index;
    t->file_open = true;
    return FR_OK;
}

// The caller (fr_dmx_tally_window) has a successful fr_dmx_route of these n_pairs records behind it, and that
// call synchronised the stream after every earlier tally kernel and its state copy: *h_st is exact here.
int dmx_tally_window(DmxTally* t, const u64* rec_key, u64 n_pairs, u64 first_record, std::string& err) {
    if (!t->file_open) return err = "fr_dmx_tally_window: no fr_dmx_tally_file", FR_ERR_INVALID;
    if (!n_pairs) return FR_OK;
    if (n_pairs >= 0xFFFFFFFFull || first_record >= TREC_MAX || first_record + n_pairs > TREC_MAX)
        return err = "fr_dmx_tally_window: too many records in one file pair", FR_ERR_CAPACITY;
    if (int rc = check_full(t, err)) return rc;
    const u64 need = 2 * (t->h_st->n_keys + n_pairs);
    if (t->nslots < need)
        if (int rc = rebuild(t, pow2_from(need, t->nslots * 2), err)) return rc;
    const u64 ord0 = ((t->file + 1) << ORD_SHIFT) | first_record;
    hipLaunchKernelGGL(dmx_tally_window_kernel, dim3(grid_over(n_pairs, (u64)TWG * TPER, t->max_grid)), dim3(TWG), 0,
                       t->stream, rec_key, n_pairs, ord0, t->slots, t->nslots - 1, t->st);
    TK(hipGetLastError());
    return snapshot(t, err);
}

// everything closed and landed: the exact state in *h_st
static int settle(DmxTally* t, std::string& err) {
    if (int rc = close_pair(t, err)) return rc;
    TK(hipStreamSynchronize(t->stream));
    return check_full(t, err);
}

int dmx_tally_sizes(DmxTally* t, u64* n_unique, u64* n_presence, std::string& err) {
    if (int rc = settle(t, err)) return rc;
    *n_unique = t->h_st->n_keys;
    *n_presence = t->h_st->n_pres;
    return FR_OK;
}

int dmx_tally_rows_device(DmxTally* t, void* dev_rows, u64 cap, std::string& err) {
    if (int rc = settle(t, err)) return rc;
    const u64 n = t->h_st->n_keys;
    if (n > cap) return err = "fr_dmx_tally_rows_device: the buffer is too small", FR_ERR_CAPACITY;
    if (!n) return FR_OK;
    TK(hipMemsetAsync(&t->st->n_rows, 0, sizeof(u64), t->stream));
    hipLaunchKernelGGL(dmx_tally_rows, dim3(grid_over(t->nslots, TWG, t->max_grid)), dim3(TWG), 0, t->stream,
                       (const TSlot*)t->slots, t->nslots, (u64*)dev_rows, cap, t->st);
    TK(hipGetLastError());
    if (int rc = snapshot(t, err)) return rc;
    TK(hipStreamSynchronize(t->stream));
    if (t->h_st->full || t->h_st->n_rows != n) return err = "fr_dmx_tally: row count mismatch", FR_ERR_DEVICE;
    return FR_OK;
}

int dmx_tally_get(DmxTally* t, u64* keys, u64* counts, u64* first, u32* pres_unique, u32* pres_file, u64* pres_reads,
                  std::string& err) {
    if (int rc = settle(t, err)) return rc;
    const u64 n = t->h_st->n_keys, m = t->h_st->n_pres;
    if (n > 0xFFFFFFFFull) return err = "fr_dmx_tally_get: more than 2^32 distinct codes", FR_ERR_CAPACITY;
    if (n > t->rows_cap) {
        if (t->rows) TK(hipFree(t->rows));
        t->rows = nullptr;
        t->rows_cap = std::max<u64>(n + n / 4, 1024);
        TK(hipMalloc((void**)&t->rows, t->rows_cap * 3 * sizeof(u64)));
    }
    if (int rc = dmx_tally_rows_device(t, t->rows, t->rows_cap, err)) return rc;
    std::vector<u64> h(3 * n);
    if (n) TK(hipMemcpy(h.data(), t->rows, 3 * n * sizeof(u64), hipMemcpyDeviceToHost));
    std::unordered_map<u64, u32> where;
    where.reserve(n);
    for (u64 i = 0; i < n; ++i) {
        keys[i] = h[3 * i];
        counts[i] = h[3 * i + 1];
        first[i] = h[3 * i + 2];
        where.emplace(h[3 * i], (u32)i);
    }
    std::vector<TPres> p(m);
    if (m) TK(hipMemcpy(p.data(), t->pres, m * sizeof(TPres), hipMemcpyDeviceToHost));
    for (u64 j = 0; j < m; ++j) {
        const auto it = where.find(p[j].key);
        if (it == where.end()) return err = "fr_dmx_tally_get: a presence entry's code is not in the table", FR_ERR_DEVICE;
        pres_unique[j] = it->second;
        pres_file[j] = (u32)p[j].file;
        pres_reads[j] = p[j].reads;
    }
    return FR_OK;
}

}  // namespace fr
