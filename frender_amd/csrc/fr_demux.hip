// fr_demux.hip — SURVEY.md §8.1 row (f-1): `demux` (frender.py:733-814) on the GPU.
//
// The reference's hot loop walks R1/R2 record pairs in lockstep, takes the code after the last
// ':' of the R2 header line (frender.py:778), looks it up in the scan results and appends both
// records to the writer pair of the result's read type / sample (frender.py:779-810).  Here one
// pair of decoded files is resident in HBM and:
//   dmx_count  newline count per 16-KiB tile (HBM-bound streaming read)
//   scan       exclusive prefix of the tile counts (rocprim)
//   dmx_index  record starts (every 4th line start) and, for R2, the code -> destination lookup
//              in an open-addressing table of the results' fast codes; in sheet mode (fr_dmx_set_sheet)
//              the code's fast key instead, which dmx_class_kernel (fr_classify.hip) classifies against
//              the sample sheet and turns into the destination: no results, no scan pass
//   route      stable partition of the record pairs by destination (rocprim radix sort on the
//              destination, record index as payload), output offsets (rocprim scans) and a
//              gather-copy of both mates' record bytes into destination-major buffers
// With fr_dmx_tally_begin (sheet mode, `demux -b --report`) the routed records' keys are also counted: the kernels
// and their tables are fr_dmx_tally.hip's, the entry points at the end of this file check mode and call order.
// With fr_dmx_stats_begin (`demux --stats`) the routed records are also summed per destination (reads, bases, quality):
// fr_dmx_stats.hip's kernel over the routed bytes, entered the same way.
// With fr_dmx_cycles_begin (`demux --cycle-stats`) they are also counted per destination and cycle (bases by value,
// quality): fr_dmx_cycles.hip's kernel over the same bytes, entered the same way.
// With fr_dmx_bstats_begin (sheet mode, `demux -b --barcode-stats`) the classifier also leaves every record's index
// mismatch bins, and the routed records' are counted per destination: fr_dmx_bstats.hip's kernel over the partition
// order, entered the same way.
// The host inflates, normalises universal newlines (frender.py:776 reads in text mode), resolves
// the rare codes outside the fast alphabet, raises the reference's errors, and gzips each
// destination's bytes into its writer pair.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "../../include/frender_amd.h"
#include "fr_internal.h"

namespace fr {
namespace {

constexpr int DT = 16384;        // tile bytes
constexpr int DWG = 256;         // lanes per workgroup: 64 B each
constexpr int DSEG = DT / DWG;
constexpr int DHALO = 1024;      // bytes staged past the tile for headers that cross it
constexpr int DMAXSYM = MAXSYM;  // fast key: <= 21 symbols
constexpr u64 DMX_BATCH = 64;    // fr_dmx_records / fr_dmx_patch: from this many records on, whole-array copies

__device__ __forceinline__ u32 nl_mask4(u32 w) {  // exact '\n' bytes -> bits 0..3
    const u32 t = w ^ 0x0A0A0A0Au;
    const u32 z = ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) & 0x80808080u;
    return __builtin_amdgcn_udot4(z >> 7, 0x08040201u, 0u, false);
}

__device__ __forceinline__ u32 sym_byte(u32 c) {  // A1 C2 G3 T4 N5 +6, else 0
    switch (c) {
        case 'A': return 1;
        case 'C': return 2;
        case 'G': return 3;
        case 'T': return 4;
        case 'N': return 5;
        case '+': return 6;
        default: return 0;
    }
}

struct DmxTable {
    const u64* keys;  // 0 = empty
    const int32_t* vals;
    u64 mask;
};

__device__ __forceinline__ int32_t table_get(const DmxTable& t, u64 key) {
    if (!t.keys) return FR_DMX_MISSING;
    u64 h = mix64(key) & t.mask;
    for (;;) {
        const u64 k = t.keys[h];
        if (k == key) return t.vals[h];
        if (k == 0) return FR_DMX_MISSING;
        h = (h + 1) & t.mask;
    }
}

__global__ void dmx_table_insert(u64* keys, int32_t* vals, u64 mask, const u64* in_k, const int32_t* in_v, u64 n) {
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 key = in_k[i];
        u64 h = mix64(key) & mask;
        for (;;) {
            const u64 old = atomicCAS((unsigned long long*)&keys[h], 0ull, (unsigned long long)key);
            if (old == 0 || old == key) {
                vals[h] = in_v[i];
                break;
            }
            h = (h + 1) & mask;
        }
    }
}

// 64 bytes of lane `tid` of tile t (zeros past len) -> '\n' bitmap
__device__ __forceinline__ u64 lane_nl(const u8* buf, u64 len, u64 tile0, int tid) {
    const u64 base = tile0 + (u64)tid * DSEG;
    u64 m = 0;
    if (base + DSEG <= len) {
#pragma unroll
        for (int q = 0; q < DSEG / 16; ++q) {
            const uint4 v = *(const uint4*)(buf + base + q * 16);
            m |= (u64)(nl_mask4(v.x) | (nl_mask4(v.y) << 4) | (nl_mask4(v.z) << 8) | (nl_mask4(v.w) << 12)) << (16 * q);
        }
    } else if (base < len) {
        for (u64 j = 0; base + j < len; ++j) m |= (u64)(buf[base + j] == '\n') << j;
    }
    return m;
}

__global__ __launch_bounds__(DWG) void dmx_count(const u8* buf, u64 len, u32 ntiles, u32* tile_cnt) {
    __shared__ u32 ws[DWG / 64];
    for (u32 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        u32 c = __popcll(lane_nl(buf, len, (u64)t * DT, threadIdx.x));
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) tile_cnt[t] = ws[0] + ws[1] + ws[2] + ws[3];
        __syncthreads();
    }
}

__device__ __forceinline__ u32 eq_mask4(u32 w, u32 rep) {  // exact byte equality -> bits 0..3
    const u32 t = w ^ rep;
    const u32 z = ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) & 0x80808080u;
    return __builtin_amdgcn_udot4(z >> 7, 0x08040201u, 0u, false);
}

// fast key of the code bytes [s, s+n) in LDS: v_perm lookups 4 bytes per step (A1 C2 G3 T4 N5 +6);
// false when a byte is outside the fast alphabet
__device__ __forceinline__ bool encode_fast(const u8* lds, u32 s, u32 n, u64& key) {
    u64 kk = 0;
    u32 bad = 0;
    for (u32 k = 0; 4 * k < n; ++k) {
        const u32 p = s + 4 * k;
        const u32 lo = *(const u32*)(lds + (p & ~3u)), hi = *(const u32*)(lds + (p & ~3u) + 4);
        const u32 a = __builtin_amdgcn_alignbyte(hi, lo, p & 3u);
        const u32 idx = (a >> 1) & 0x07070707u;
        const u32 expect = __builtin_amdgcn_perm(0x4E002B00u, 0x47544341u, idx);
        const u32 sym = __builtin_amdgcn_perm(0x05000600u, 0x03040201u, idx);
        const u32 left = n - 4 * k;
        const u32 vm = left >= 4 ? 0xFFFFFFFFu : (0xFFFFFFFFu >> (32 - 8 * left));
        bad |= (expect ^ a) & vm;
        const u32 sv = sym & vm;
        kk |= (u64)((sv & 0x7u) | ((sv >> 5) & 0x38u) | ((sv >> 10) & 0x1C0u) | ((sv >> 15) & 0xE00u)) << (12 * k);
    }
    key = kk;
    return bad == 0;
}

// a fast key's destination: the table's answer, or in key mode (fr_dmx_set_sheet) the key itself for
// dmx_class_kernel, which replaces DMX_PENDING
template <bool KEY>
__device__ __forceinline__ int32_t key_dest(const DmxTable& tab, u64 key, u64& key_out) {
    if constexpr (KEY) {
        key_out = key;
        return DMX_PENDING;
    } else {
        return table_get(tab, key);
    }
}

// slow path: the header line runs past the staged bytes -> byte loop over global memory
template <bool KEY>
__device__ __noinline__ int32_t header_dest_global(const u8* buf, u64 len, u64 p, const DmxTable& tab, u64& key_out) {
    u64 e = p, lastc = ~0ull;
    while (e < len && buf[e] != '\n') {
        if (buf[e] == ':') lastc = e;
        ++e;
    }
    const u64 s = lastc == ~0ull ? p : lastc + 1;
    const u64 n = e - s;
    if (n == 0 || n > (u64)DMAXSYM) return FR_DMX_EXOTIC;
    u64 key = 0;
    for (u64 i = 0; i < n; ++i) {
        const u32 sy = sym_byte(buf[s + i]);
        if (!sy) return FR_DMX_EXOTIC;
        key |= (u64)sy << (3 * i);
    }
    return key_dest<KEY>(tab, key, key_out);
}

// the code of the header line starting at tile position q: the text after the line's last ':'
// up to its '\n' (frender.py:778) -> destination.  Word-at-a-time over the staged tile (LDS,
// zero-padded past lds_n); '\n' and ':' found with exact SWAR byte masks.
template <bool KEY>
__device__ __forceinline__ int32_t header_dest(const u8* buf, u64 len, u64 tile0, u32 q, const u8* lds, u32 lds_n,
                                               const DmxTable& tab, u64& key_out) {
    int lastc = -1, e = -1;
    u32 w = q & ~3u;
    u32 keep = (0xFu << (q & 3u)) & 0xFu;
    for (; w < lds_n; w += 4) {
        const u32 v = *(const u32*)(lds + w);
        u32 nl = eq_mask4(v, 0x0A0A0A0Au) & keep, col = eq_mask4(v, 0x3A3A3A3Au) & keep;
        keep = 0xFu;
        if (w + 4 > lds_n) {
            const u32 vm = (1u << (lds_n - w)) - 1u;
            nl &= vm;
            col &= vm;
        }
        if (nl) {
            const u32 b = __builtin_ctz(nl);
            col &= (1u << b) - 1u;
            if (col) lastc = (int)(w + 31u - __builtin_clz(col));
            e = (int)(w + b);
            break;
        }
        if (col) lastc = (int)(w + 31u - __builtin_clz(col));
    }
    if (e < 0) {
        if (tile0 + lds_n < len) return header_dest_global<KEY>(buf, len, tile0 + q, tab, key_out);
        e = (int)lds_n;  // the line ends with the data
    }
    const u32 s = lastc >= 0 ? (u32)lastc + 1u : q;
    const u32 n = (u32)e - s;
    if (n == 0 || n > (u32)DMAXSYM) return FR_DMX_EXOTIC;
    u64 key;
    if (!encode_fast(lds, s, n, key)) return FR_DMX_EXOTIC;
    return key_dest<KEY>(tab, key, key_out);
}

// KEY (fr_dmx_set_sheet's mode): no table; a record's fast key goes to rec_key and DMX_PENDING to rec_dest
template <bool KEY>
__global__ __launch_bounds__(DWG) void dmx_index(const u8* buf, u64 len, u32 ntiles, const u64* tile_base,
                                                 u64* rec_start, int32_t* rec_dest, DmxTable tab, u64* rec_key) {
    __shared__ __attribute__((aligned(16))) u8 lds[DT + DHALO + 32];  // +32: zero pad for word reads
    __shared__ u32 ws[DWG / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    for (u32 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const u64 tile0 = (u64)t * DT;
        const u32 lds_n = (u32)min((u64)(DT + DHALO), len - tile0);
        if (rec_dest) {
            for (u32 i = tid * 16; i < lds_n + 32; i += DWG * 16) {
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (i + 16 <= lds_n) {
                    v = *(const uint4*)(buf + tile0 + i);
                } else if (i < lds_n) {
                    u32 b[4] = {0u, 0u, 0u, 0u};
                    for (u32 j = i; j < lds_n; ++j) b[(j - i) >> 2] |= (u32)buf[tile0 + j] << (8 * ((j - i) & 3));
                    v = make_uint4(b[0], b[1], b[2], b[3]);
                }
                if (i < DT + DHALO + 32) *(uint4*)(lds + i) = v;
            }
        }
        const u64 m = lane_nl(buf, len, tile0, tid);
        const u32 c = __popcll(m);
        u32 x = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u32 y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63) ws[wid] = x;
        __syncthreads();
        u64 L = tile_base[t] + (x - c);
        for (int w = 0; w < wid; ++w) L += ws[w];
        // line start after each '\n' of this lane's segment: line index L + rank + 1
        u64 mm = m;
        while (mm) {
            const u32 j = __builtin_ctzll(mm);
            mm &= mm - 1;
            L += 1;
            const u64 p = tile0 + (u64)tid * DSEG + j + 1;
            if ((L & 3ull) == 0 && p < len) {
                rec_start[L >> 2] = p;
                if (rec_dest) {
                    u64 key = 0;
                    rec_dest[L >> 2] = header_dest<KEY>(buf, len, tile0, (u32)(p - tile0), lds, lds_n, tab, key);
                    if constexpr (KEY) rec_key[L >> 2] = key;
                }
            }
        }
        if (t == 0 && tid == 0 && len > 0) {  // the first line of the file
            rec_start[0] = 0;
            if (rec_dest) {
                u64 key = 0;
                rec_dest[0] = header_dest<KEY>(buf, len, tile0, 0u, lds, lds_n, tab, key);
                if constexpr (KEY) rec_key[0] = key;
            }
        }
        __syncthreads();
    }
}

// first[0]: the first record with a negative destination; first[1]: cleared when some destination is >= n_dest
// (a plain store of one value: no order among the writers is needed)
__global__ void dmx_first_error(const int32_t* dest, u64 n, int n_dest, unsigned long long* first) {
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const int32_t v = dest[i];
        if (v < 0)
            atomicMin(first, (unsigned long long)i);
        else if (v >= n_dest)
            first[1] = 0ull;
    }
}

__global__ void dmx_keys(const int32_t* dest, u64 n, u32* keys, u32* idx) {
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        keys[i] = (u32)dest[i];
        idx[i] = (u32)i;
    }
}

// lengths of both mates' records in partition order
__global__ void dmx_lengths(const u32* perm, u64 n, const u64* rs1, const u64* rs2, u64* len1, u64* len2) {
    for (u64 j = blockIdx.x * (u64)blockDim.x + threadIdx.x; j < n; j += (u64)gridDim.x * blockDim.x) {
        const u32 i = perm[j];
        len1[j] = rs1[i + 1] - rs1[i];
        len2[j] = rs2[i + 1] - rs2[i];
    }
}

// the same for the only mate there is (fr_dmx_set_mates(1))
__global__ void dmx_lengths1(const u32* perm, u64 n, const u64* rs, u64* len) {
    for (u64 j = blockIdx.x * (u64)blockDim.x + threadIdx.x; j < n; j += (u64)gridDim.x * blockDim.x) {
        const u32 i = perm[j];
        len[j] = rs[i + 1] - rs[i];
    }
}

// first partition position of every destination present (sorted keys: one boundary each, no atomics)
__global__ void dmx_bounds(const u32* sk, u64 n, u32* first) {
    for (u64 j = blockIdx.x * (u64)blockDim.x + threadIdx.x; j < n; j += (u64)gridDim.x * blockDim.x)
        if (j == 0 || sk[j] != sk[j - 1]) first[sk[j]] = (u32)j;
}

// byte offset of every destination's first record (n_dest entries, + the total at [n_dest])
__global__ void dmx_dest_offsets(const u32* first, int n_dest, u64 n, const u64* o1, const u64* l1, const u64* o2,
                                 const u64* l2, u64* off1, u64* off2) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d > n_dest) return;
    const u64 tot1 = o1[n - 1] + l1[n - 1], tot2 = o2[n - 1] + l2[n - 1];
    // an absent destination starts where the next present one does
    int e = d;
    while (e < n_dest && first[e] == 0xFFFFFFFFu) ++e;
    off1[d] = e < n_dest ? o1[first[e]] : tot1;
    off2[d] = e < n_dest ? o2[first[e]] : tot2;
}

// the same for the only mate there is (fr_dmx_set_mates(1))
__global__ void dmx_dest_offsets1(const u32* first, int n_dest, u64 n, const u64* o, const u64* l, u64* off) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d > n_dest) return;
    int e = d;
    while (e < n_dest && first[e] == 0xFFFFFFFFu) ++e;
    off[d] = e < n_dest ? o[first[e]] : o[n - 1] + l[n - 1];
}

// one wave per output record: a byte head up to the destination's 4-byte alignment, then
// aligned dword stores, each assembled from the two source dwords it straddles
// (v_alignbyte_b32), then a byte tail.  Source reads may run up to 3 bytes past the record
// inside the same aligned dword (allocations are 256-B granular).
__global__ void dmx_copy(const u32* perm, u64 n, const u64* rs, const u8* src, const u64* off, u8* dst) {
    const int lane = threadIdx.x & 63;
    const u64 waves = (u64)gridDim.x * (blockDim.x / 64);
    for (u64 j = blockIdx.x * (u64)(blockDim.x / 64) + (threadIdx.x >> 6); j < n; j += waves) {
        const u32 i = perm[j];
        const u64 s = rs[i], len = rs[i + 1] - s, o = off[j];
        const u64 head = min((u64)((4u - (u32)(o & 3u)) & 3u), len);
        if ((u64)lane < head) dst[o + lane] = src[s + lane];
        const u64 s1 = s + head, o1 = o + head, words = (len - head) >> 2;
        const u32 sh = (u32)(s1 & 3u);
        const u32* sw = (const u32*)(src + (s1 & ~3ull));
        u32* dw = (u32*)(dst + o1);
        for (u64 k = lane; k < words; k += 64) {
            const u32 lo = sw[k];
            const u32 hi = sh ? sw[k + 1] : 0u;
            dw[k] = sh ? __builtin_amdgcn_alignbyte(hi, lo, sh) : lo;
        }
        const u64 t0 = head + (words << 2);
        if (t0 + lane < len) dst[o + t0 + lane] = src[s + t0 + lane];
    }
}

int grid_for(u64 n, int per = 256, int cap = 8192) {
    return (int)std::max<u64>(1, std::min<u64>((n + per - 1) / per, (u64)cap));
}

}  // namespace
}  // namespace fr

using namespace fr;

fr_defl* fr_defl_create_on(int device, hipStream_t stream);

struct fr_dmx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // the mates of an input (fr_dmx_set_mates): 2, or 1 for a single-end file, whose only mate (0) is the code mate
    int n_mates = 2;
    int code_mate() const { return n_mates - 1; }
    // results table
    u64* tkeys = nullptr;
    int32_t* tvals = nullptr;
    u64 tmask = 0;
    // sheet mode (fr_dmx_set_sheet): the borrowed sheet and maps, the destinations, every R2 record's fast key
    bool key_mode = false;
    SheetArgs sheet{};
    NbrMap nbr{};
    int nsubs1 = 0, nsubs2 = 0;
    int32_t* row_dest = nullptr;
    DmxClassDest class_dest{};
    u64* rkey = nullptr;
    u64 rkey_cap = 0;
    u8* rbin = nullptr;  // every R2 record's mismatch bin byte (fr_dmx_bstats_begin; else never allocated)
    u64 rbin_cap = 0;
    bool rbin_loaded = false;  // the R2 window at hand was classified with the bin bytes
    // per mate: data, record starts (+ sentinel), destinations (R2)
    u8* data[2] = {nullptr, nullptr};
    u64 cap[2] = {0, 0};
    const u8* src[2] = {nullptr, nullptr};  // the bytes indexed: data[m] or a caller's device buffer
    u64 len[2] = {0, 0};
    u64* rs[2] = {nullptr, nullptr};
    u64 rs_cap[2] = {0, 0};
    u64 nrec[2] = {0, 0};
    int32_t* dest = nullptr;
    u64 dest_cap = 0;
    // route temporaries (grow-only) and outputs
    u32 *k_in = nullptr, *k_out = nullptr, *i_in = nullptr, *perm = nullptr, *first_pos = nullptr;
    u64 *l1 = nullptr, *l2 = nullptr, *o1 = nullptr, *o2 = nullptr, *off1 = nullptr, *off2 = nullptr;
    u64 c_k_in = 0, c_k_out = 0, c_i_in = 0, c_perm = 0, c_first = 0, c_l1 = 0, c_l2 = 0, c_o1 = 0, c_o2 = 0,
        c_off1 = 0, c_off2 = 0;
    void* tmp = nullptr;
    u64 c_tmp = 0;
    u32* cnt = nullptr;
    u64* base = nullptr;
    u64 c_cnt = 0, c_base = 0;
    unsigned long long* fe = nullptr;
    u64 c_fe = 0;
    u8* out[2] = {nullptr, nullptr};
    u64 out_cap[2] = {0, 0};
    u64 out_len[2] = {0, 0};
    std::vector<u64> hoff[2];  // destination offsets of the routed bytes (host copy)
    fr_defl* defl[2] = {nullptr, nullptr};  // the writers' compression (fr_deflate.hip), created on first use
    // the windows' tally (fr_dmx_tally_begin; fr_dmx_tally.hip), and the pairs the last fr_dmx_route routed that
    // no fr_dmx_tally_window has counted yet
    DmxTally* tally = nullptr;
    u64 routed_ok = 0;
    // the windows' statistics (fr_dmx_stats_begin; fr_dmx_stats.hip), and the pairs the last fr_dmx_route routed
    // that no fr_dmx_stats_window has added yet
    DmxStats* stats = nullptr;
    u64 stats_ok = 0;
    // the windows' per-cycle statistics (fr_dmx_cycles_begin; fr_dmx_cycles.hip), and the pairs the last fr_dmx_route
    // routed that no fr_dmx_cycles_window has added yet
    DmxCycles* cycles = nullptr;
    u64 cycles_ok = 0;
    // the windows' index mismatch table (fr_dmx_bstats_begin; fr_dmx_bstats.hip), and the pairs the last fr_dmx_route
    // routed that no fr_dmx_bstats_window has counted yet
    DmxBstats* bstats = nullptr;
    u64 bstats_ok = 0;
    // the windows' validation (fr_dmx_validate_begin; fr_dmx_validate.hip): the mates loaded since the last
    // fr_dmx_validate_window, and whether a window is queued whose result can be read
    DmxValidate* validate = nullptr;
    bool vloaded[2] = {false, false};
    bool vqueued = false;
    // the GPU reader of BGZF mates (fr_dmx_bgzf_open; fr_dmx_reader.hip): never created without that call
    DmxReader* reader = nullptr;
};

#define DK(x)                                                                  \
    do {                                                                       \
        hipError_t e_ = (x);                                                   \
        if (e_ != hipSuccess) {                                                \
            d->err = std::string(#x) + ": " + hipGetErrorString(e_);           \
            return FR_ERR_HIP;                                                 \
        }                                                                      \
    } while (0)

template <class T>
static hipError_t ensure(T** p, u64& cap, u64 n) {
    if (n <= cap && *p) return hipSuccess;
    if (*p) {
        hipError_t e = hipFree(*p);
        if (e != hipSuccess) return e;
        *p = nullptr;
    }
    cap = std::max<u64>(n + n / 4, 1024);
    return hipMalloc((void**)p, cap * sizeof(T));
}

// one-mate mode (fr_dmx_set_mates(1)) has no mate 1: the entry point `what` refuses it
static bool no_mate(fr_dmx* d, int mate, const char* what) {
    if (d->n_mates == 2 || mate != 1) return false;
    d->err = std::string(what) + ": there is no mate 1 in one-mate mode (fr_dmx_set_mates(1))";
    return true;
}

extern "C" {

fr_dmx* fr_dmx_create(int device) {
    fr_dmx* d = new fr_dmx();
    d->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess)
        d->err = "fr_dmx_create: no usable HIP device";
    return d;
}

void fr_dmx_destroy(fr_dmx* d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    if (d->stream) (void)hipStreamSynchronize(d->stream);
    void* p[] = {d->tkeys, d->tvals, d->data[0], d->data[1], d->rs[0], d->rs[1], d->dest, d->out[0], d->out[1],
                 d->k_in, d->k_out, d->i_in, d->perm, d->first_pos, d->l1, d->l2, d->o1, d->o2, d->off1, d->off2,
                 d->tmp, d->cnt, d->base, d->fe, d->row_dest, d->rkey, d->rbin};
    for (void* x : p)
        if (x) (void)hipFree(x);
    for (fr_defl* z : d->defl) fr_defl_destroy(z);
    dmx_tally_destroy(d->tally);
    dmx_stats_destroy(d->stats);
    dmx_cycles_destroy(d->cycles);
    dmx_bstats_destroy(d->bstats);
    dmx_validate_destroy(d->validate);
    dmx_reader_destroy(d->reader);
    if (d->stream) (void)hipStreamDestroy(d->stream);
    delete d;
}

const char* fr_dmx_last_error(const fr_dmx* d) { return d ? d->err.c_str() : "null context"; }

int fr_dmx_set_table(fr_dmx* d, const uint64_t* keys, const int32_t* vals, uint64_t n) {
    DK(hipSetDevice(d->device));
    d->key_mode = false;
    if (d->tkeys) DK(hipFree(d->tkeys));
    if (d->tvals) DK(hipFree(d->tvals));
    d->tkeys = nullptr;
    d->tvals = nullptr;
    u64 slots = 1024;
    while (slots < 2 * n) slots <<= 1;
    d->tmask = slots - 1;
    DK(hipMalloc(&d->tkeys, slots * 8));
    DK(hipMalloc(&d->tvals, slots * 4));
    DK(hipMemsetAsync(d->tkeys, 0, slots * 8, d->stream));
    if (n) {
        u64* k = nullptr;
        int32_t* v = nullptr;
        DK(hipMalloc(&k, n * 8));
        DK(hipMalloc(&v, n * 4));
        DK(hipMemcpyAsync(k, keys, n * 8, hipMemcpyHostToDevice, d->stream));
        DK(hipMemcpyAsync(v, vals, n * 4, hipMemcpyHostToDevice, d->stream));
        hipLaunchKernelGGL(dmx_table_insert, dim3(grid_for(n)), dim3(256), 0, d->stream, d->tkeys, d->tvals, d->tmask,
                           k, v, n);
        DK(hipGetLastError());
        DK(hipStreamSynchronize(d->stream));
        DK(hipFree(k));
        DK(hipFree(v));
    }
    return FR_OK;
}

int fr_dmx_set_sheet(fr_dmx* d, fr_ctx* ctx, int num_subs, const int32_t* row_dest, int n_rows,
                     const int32_t class_dest[4]) {
    return fr_dmx_set_sheet2(d, ctx, num_subs, num_subs, row_dest, n_rows, class_dest);
}

int fr_dmx_set_sheet2(fr_dmx* d, fr_ctx* ctx, int num_subs1, int num_subs2, const int32_t* row_dest, int n_rows,
                      const int32_t class_dest[4]) {
    if (!ctx || !class_dest || n_rows < 0 || (n_rows && !row_dest))
        return d->err = "fr_dmx_set_sheet[2]: null context or destinations", FR_ERR_INVALID;
    d->key_mode = false;
    int device = -1;
    SheetArgs sh{};
    NbrMap nm{};
    if (int rc = borrow_sheet(ctx, num_subs1, num_subs2, &device, &sh, &nm))
        return d->err = std::string("fr_dmx_set_sheet[2]: ") + fr_last_error(ctx), rc;
    if (device != d->device) return d->err = "fr_dmx_set_sheet[2]: the context is on another device", FR_ERR_INVALID;
    if (n_rows != std::max(sh.S, 0))
        return d->err = "fr_dmx_set_sheet[2]: n_rows differs from the sheet's rows", FR_ERR_INVALID;
    DK(hipSetDevice(d->device));
    DK(hipStreamSynchronize(d->stream));  // an earlier window may still read the old destinations
    if (d->row_dest) DK(hipFree(d->row_dest));
    d->row_dest = nullptr;
    DK(hipMalloc((void**)&d->row_dest, std::max(n_rows, 1) * sizeof(int32_t)));
    if (n_rows) DK(hipMemcpy(d->row_dest, row_dest, n_rows * sizeof(int32_t), hipMemcpyHostToDevice));
    for (int k = 0; k < 4; ++k) d->class_dest.v[k] = class_dest[k];
    d->sheet = sh;
    d->nbr = nm;
    d->nsubs1 = num_subs1;
    d->nsubs2 = num_subs2;
    d->key_mode = true;
    return FR_OK;
}

int fr_dmx_set_mates(fr_dmx* d, int n_mates) {
    if (n_mates != 1 && n_mates != 2) return d->err = "fr_dmx_set_mates: n_mates must be 1 or 2", FR_ERR_INVALID;
    if (n_mates == d->n_mates) return FR_OK;
    if (d->len[0] || d->len[1] || dmx_reader_is_open(d->reader, 0) || dmx_reader_is_open(d->reader, 1))
        return d->err = "fr_dmx_set_mates: a mate is loaded or a BGZF mate is open (the count changes between inputs, "
                        "with no window at hand)", FR_ERR_INVALID;
    DK(hipSetDevice(d->device));
    DK(hipStreamSynchronize(d->stream));
    d->n_mates = n_mates;
    d->nrec[0] = d->nrec[1] = 0;
    d->out_len[0] = d->out_len[1] = 0;
    d->routed_ok = d->stats_ok = d->cycles_ok = d->bstats_ok = 0;
    d->vloaded[0] = d->vloaded[1] = false;
    d->rbin_loaded = false;
    return FR_OK;
}

static int dmx_index_mate(fr_dmx* d, int mate, const u8* buf, u64 len, u64* n_records) {
    const bool code = mate == d->code_mate();  // the mate whose header carries the record's code
    d->src[mate] = buf;
    d->len[mate] = len;
    d->routed_ok = d->stats_ok = d->cycles_ok = d->bstats_ok = 0;
    d->vloaded[mate] = false;
    if (code) d->rbin_loaded = false;
    const u32 ntiles = (u32)((len + DT - 1) / DT);
    DK(ensure(&d->cnt, d->c_cnt, (u64)ntiles + 1));
    DK(ensure(&d->base, d->c_base, (u64)ntiles + 1));
    u64 nl = 0;
    if (ntiles) {
        hipLaunchKernelGGL(dmx_count, dim3(std::min<u32>(ntiles, 8192)), dim3(DWG), 0, d->stream, buf, len, ntiles,
                           d->cnt);
        DK(hipGetLastError());
        size_t tb = 0;
        DK(rocprim::exclusive_scan(nullptr, tb, d->cnt, d->base, (u64)0, (size_t)ntiles + 1, rocprim::plus<u64>(),
                                   d->stream));
        DK(ensure((u8**)&d->tmp, d->c_tmp, tb + 1));
        DK(hipMemsetAsync(d->cnt + ntiles, 0, 4, d->stream));
        DK(rocprim::exclusive_scan(d->tmp, tb, d->cnt, d->base, (u64)0, (size_t)ntiles + 1, rocprim::plus<u64>(),
                                   d->stream));
        DK(hipMemcpyAsync(&nl, d->base + ntiles, 8, hipMemcpyDeviceToHost, d->stream));  // total '\n'
    }
    u8 lastb = '\n';
    if (len) DK(hipMemcpyAsync(&lastb, buf + len - 1, 1, hipMemcpyDeviceToHost, d->stream));
    DK(hipStreamSynchronize(d->stream));
    const u64 lines = nl + ((len && lastb != '\n') ? 1 : 0);  // a last line without '\n'
    const u64 nrec = (lines + 3) / 4;
    DK(ensure(&d->rs[mate], d->rs_cap[mate], nrec + 1));
    if (code) DK(ensure(&d->dest, d->dest_cap, nrec + 1));
    d->nrec[mate] = nrec;
    *n_records = nrec;
    DK(hipMemcpyAsync(d->rs[mate] + nrec, &d->len[mate], 8, hipMemcpyHostToDevice, d->stream));  // sentinel
    if (ntiles && code && d->key_mode) {
        DK(ensure(&d->rkey, d->rkey_cap, nrec + 1));
        hipLaunchKernelGGL(dmx_index<true>, dim3(std::min<u32>(ntiles, 4096)), dim3(DWG), 0, d->stream, buf, len,
                           ntiles, d->base, d->rs[mate], d->dest, DmxTable{nullptr, nullptr, 0}, d->rkey);
        DK(hipGetLastError());
        if (d->bstats) DK(ensure(&d->rbin, d->rbin_cap, nrec + 1));
        DK(launch_dmx_classify(d->rkey, d->dest, nrec, d->sheet, d->nsubs1, d->nsubs2, d->nbr, d->row_dest,
                               d->class_dest, d->bstats ? d->rbin : nullptr, d->stream));
        d->rbin_loaded = d->bstats != nullptr;
    } else if (ntiles) {
        DmxTable tab{d->tkeys, d->tvals, d->tmask};
        hipLaunchKernelGGL(dmx_index<false>, dim3(std::min<u32>(ntiles, 4096)), dim3(DWG), 0, d->stream, buf, len,
                           ntiles, d->base, d->rs[mate], code ? d->dest : nullptr, tab, (u64*)nullptr);
        DK(hipGetLastError());
    }
    DK(hipStreamSynchronize(d->stream));
    d->vloaded[mate] = true;
    return FR_OK;
}

int fr_dmx_load(fr_dmx* d, int mate, const uint8_t* data, uint64_t len, uint64_t* n_records) {
    if (mate < 0 || mate > 1) return d->err = "mate must be 0 (R1) or 1 (R2)", FR_ERR_INVALID;
    if (no_mate(d, mate, "fr_dmx_load")) return FR_ERR_INVALID;
    DK(hipSetDevice(d->device));
    DK(ensure(&d->data[mate], d->cap[mate], len + 16));
    if (len) DK(hipMemcpyAsync(d->data[mate], data, len, hipMemcpyHostToDevice, d->stream));
    return dmx_index_mate(d, mate, d->data[mate], len, n_records);
}

int fr_dmx_load_parts(fr_dmx* d, int mate, const uint8_t* const* parts, const uint64_t* lens, int n_parts,
                      uint64_t* n_records) {
    if (mate < 0 || mate > 1 || n_parts < 0) return d->err = "mate must be 0 (R1) or 1 (R2)", FR_ERR_INVALID;
    if (no_mate(d, mate, "fr_dmx_load_parts")) return FR_ERR_INVALID;
    DK(hipSetDevice(d->device));
    u64 len = 0;
    for (int k = 0; k < n_parts; ++k) len += lens[k];
    DK(ensure(&d->data[mate], d->cap[mate], len + 16));
    u64 off = 0;
    for (int k = 0; k < n_parts; ++k) {
        if (lens[k]) DK(hipMemcpyAsync(d->data[mate] + off, parts[k], lens[k], hipMemcpyHostToDevice, d->stream));
        off += lens[k];
    }
    return dmx_index_mate(d, mate, d->data[mate], len, n_records);
}

int fr_dmx_load_device(fr_dmx* d, int mate, const uint8_t* dev_data, uint64_t len, uint64_t* n_records) {
    if (mate < 0 || mate > 1) return d->err = "mate must be 0 (R1) or 1 (R2)", FR_ERR_INVALID;
    if (no_mate(d, mate, "fr_dmx_load_device")) return FR_ERR_INVALID;
    if (((uintptr_t)dev_data & 15u) != 0) return d->err = "device data must be 16-byte aligned", FR_ERR_INVALID;
    DK(hipSetDevice(d->device));
    return dmx_index_mate(d, mate, dev_data, len, n_records);
}

int fr_dmx_records(fr_dmx* d, int mate, const uint64_t* recs, uint64_t n, uint64_t* starts, uint64_t* ends) {
    if (no_mate(d, mate, "fr_dmx_records")) return FR_ERR_INVALID;
    DK(hipSetDevice(d->device));
    std::vector<u64> all;
    for (u64 k = 0; k < n; ++k)
        if (recs[k] >= d->nrec[mate]) return d->err = "record index out of range", FR_ERR_INVALID;
    if (n >= DMX_BATCH) {  // many records (a file of lower-case codes: every one exotic): the whole array in one copy
        all.resize(d->nrec[mate] + 1);
        DK(hipMemcpy(all.data(), d->rs[mate], all.size() * 8, hipMemcpyDeviceToHost));
        for (u64 k = 0; k < n; ++k) {
            starts[k] = all[recs[k]];
            ends[k] = all[recs[k] + 1];
        }
        return FR_OK;
    }
    for (u64 k = 0; k < n; ++k) {
        u64 se[2];
        DK(hipMemcpy(se, d->rs[mate] + recs[k], 16, hipMemcpyDeviceToHost));
        starts[k] = se[0];
        ends[k] = se[1];
    }
    return FR_OK;
}

int fr_dmx_exotic(fr_dmx* d, uint64_t n_pairs, uint64_t* recs, uint64_t cap, uint64_t* n) {
    DK(hipSetDevice(d->device));
    n_pairs = std::min<u64>(n_pairs, d->nrec[d->code_mate()]);
    std::vector<int32_t> h(n_pairs);
    if (n_pairs) DK(hipMemcpy(h.data(), d->dest, n_pairs * 4, hipMemcpyDeviceToHost));
    u64 k = 0;
    for (u64 i = 0; i < n_pairs; ++i)
        if (h[i] == FR_DMX_EXOTIC) {
            if (k < cap) recs[k] = i;
            ++k;
        }
    *n = k;
    return FR_OK;
}

int fr_dmx_patch(fr_dmx* d, const uint64_t* recs, const int32_t* dest, uint64_t n) {
    DK(hipSetDevice(d->device));
    for (u64 k = 0; k < n; ++k)
        if (recs[k] >= d->nrec[d->code_mate()]) return d->err = "record index out of range", FR_ERR_INVALID;
    if (n >= DMX_BATCH) {  // many records: the whole array there and back, two copies
        std::vector<int32_t> all(d->nrec[d->code_mate()]);
        DK(hipMemcpy(all.data(), d->dest, all.size() * 4, hipMemcpyDeviceToHost));
        for (u64 k = 0; k < n; ++k) all[recs[k]] = dest[k];
        DK(hipMemcpy(d->dest, all.data(), all.size() * 4, hipMemcpyHostToDevice));
        return FR_OK;
    }
    for (u64 k = 0; k < n; ++k)
        DK(hipMemcpyAsync(d->dest + recs[k], dest + k, 4, hipMemcpyHostToDevice, d->stream));
    DK(hipStreamSynchronize(d->stream));
    return FR_OK;
}

int fr_dmx_route(fr_dmx* d, int n_dest, uint64_t n_pairs, int64_t* first_error, int32_t* error_val,
                 uint64_t* bytes_r1, uint64_t* bytes_r2) {
    DK(hipSetDevice(d->device));
    const bool paired = d->n_mates == 2;
    const u64 P = std::min<u64>({n_pairs, d->nrec[0], d->nrec[d->code_mate()]});
    if (P >= 0xFFFFFFFFull)
        return d->err = paired ? "too many records in one file pair" : "too many records in one file", FR_ERR_CAPACITY;
    *first_error = -1;
    *error_val = 0;
    d->routed_ok = d->stats_ok = d->cycles_ok = d->bstats_ok = 0;
    for (int k = 0; k < n_dest; ++k) bytes_r1[k] = bytes_r2[k] = 0;
    d->out_len[0] = d->out_len[1] = 0;
    d->hoff[0].assign((size_t)std::max(n_dest, 0) + 1, 0);
    d->hoff[1].assign((size_t)std::max(n_dest, 0) + 1, 0);
    if (!P) return FR_OK;
    DK(ensure(&d->fe, d->c_fe, 2));
    unsigned long long* fe = d->fe;
    DK(hipMemsetAsync(fe, 0xFF, 16, d->stream));
    hipLaunchKernelGGL(dmx_first_error, dim3(grid_for(P)), dim3(256), 0, d->stream, d->dest, P, n_dest, fe);
    DK(hipGetLastError());
    u64 fe_h[2] = {0, 0};  // {first negative destination, 0 when one is >= n_dest}
    DK(hipMemcpyAsync(fe_h, fe, 16, hipMemcpyDeviceToHost, d->stream));
    DK(hipStreamSynchronize(d->stream));
    const u64 first = fe_h[0];
    if (first != ~0ull) {
        int32_t v = 0;
        DK(hipMemcpy(&v, d->dest + first, 4, hipMemcpyDeviceToHost));
        *first_error = (int64_t)first;
        *error_val = v;
        return FR_OK;
    }
    // dmx_bounds indexes first_pos by the destination and the sort looks at its low bits only: refuse, route nothing
    if (fe_h[1] != ~0ull) return d->err = "fr_dmx_route: destination out of range", FR_ERR_INVALID;
    // stable partition by destination (temporaries cached in the context, grow-only)
    DK(ensure(&d->k_in, d->c_k_in, P));
    DK(ensure(&d->k_out, d->c_k_out, P));
    DK(ensure(&d->i_in, d->c_i_in, P));
    DK(ensure(&d->perm, d->c_perm, P));
    DK(ensure(&d->l1, d->c_l1, P));
    DK(ensure(&d->o1, d->c_o1, P));
    DK(ensure(&d->first_pos, d->c_first, (u64)std::max(n_dest, 1)));
    DK(ensure(&d->off1, d->c_off1, (u64)n_dest + 1));
    if (paired) {  // (one mate: nothing of mate 1's is allocated, scanned, copied or read back)
        DK(ensure(&d->l2, d->c_l2, P));
        DK(ensure(&d->o2, d->c_o2, P));
        DK(ensure(&d->off2, d->c_off2, (u64)n_dest + 1));
    }
    u32 *k_in = d->k_in, *k_out = d->k_out, *i_in = d->i_in, *perm = d->perm, *first_pos = d->first_pos;
    u64 *l1 = d->l1, *l2 = d->l2, *o1 = d->o1, *o2 = d->o2, *off1 = d->off1, *off2 = d->off2;
    DK(hipMemsetAsync(first_pos, 0xFF, (u64)std::max(n_dest, 1) * 4, d->stream));
    hipLaunchKernelGGL(dmx_keys, dim3(grid_for(P)), dim3(256), 0, d->stream, d->dest, P, k_in, i_in);
    DK(hipGetLastError());
    int bits = 1;
    while ((1 << bits) < n_dest) ++bits;
    size_t tb = 0;
    DK(rocprim::radix_sort_pairs(nullptr, tb, k_in, k_out, i_in, perm, (size_t)P, 0, (unsigned)bits, d->stream));
    size_t tb2 = 0;
    DK(rocprim::exclusive_scan(nullptr, tb2, l1, o1, (u64)0, (size_t)P, rocprim::plus<u64>(), d->stream));
    DK(ensure((u8**)&d->tmp, d->c_tmp, std::max<size_t>(std::max(tb, tb2), 1)));
    void* tmp = d->tmp;
    DK(rocprim::radix_sort_pairs(tmp, tb, k_in, k_out, i_in, perm, (size_t)P, 0, (unsigned)bits, d->stream));
    if (paired)
        hipLaunchKernelGGL(dmx_lengths, dim3(grid_for(P)), dim3(256), 0, d->stream, perm, P, d->rs[0], d->rs[1], l1, l2);
    else
        hipLaunchKernelGGL(dmx_lengths1, dim3(grid_for(P)), dim3(256), 0, d->stream, perm, P, d->rs[0], l1);
    DK(hipGetLastError());
    hipLaunchKernelGGL(dmx_bounds, dim3(grid_for(P)), dim3(256), 0, d->stream, k_out, P, first_pos);
    DK(hipGetLastError());
    DK(rocprim::exclusive_scan(tmp, tb2, l1, o1, (u64)0, (size_t)P, rocprim::plus<u64>(), d->stream));
    if (paired) {
        DK(rocprim::exclusive_scan(tmp, tb2, l2, o2, (u64)0, (size_t)P, rocprim::plus<u64>(), d->stream));
        hipLaunchKernelGGL(dmx_dest_offsets, dim3((n_dest + 256) / 256), dim3(256), 0, d->stream, first_pos, n_dest, P,
                           o1, l1, o2, l2, off1, off2);
    } else {
        hipLaunchKernelGGL(dmx_dest_offsets1, dim3((n_dest + 256) / 256), dim3(256), 0, d->stream, first_pos, n_dest, P,
                           o1, l1, off1);
    }
    DK(hipGetLastError());
    std::vector<u64> h1(n_dest + 1), h2(n_dest + 1, 0);
    DK(hipMemcpyAsync(h1.data(), off1, (n_dest + 1) * 8, hipMemcpyDeviceToHost, d->stream));
    if (paired) DK(hipMemcpyAsync(h2.data(), off2, (n_dest + 1) * 8, hipMemcpyDeviceToHost, d->stream));
    DK(hipStreamSynchronize(d->stream));
    for (int k = 0; k < n_dest; ++k) {
        bytes_r1[k] = h1[k + 1] - h1[k];
        bytes_r2[k] = h2[k + 1] - h2[k];
    }
    const u64 s1 = h1[n_dest], s2 = h2[n_dest];
    DK(ensure(&d->out[0], d->out_cap[0], s1 + 16));
    if (paired) DK(ensure(&d->out[1], d->out_cap[1], s2 + 16));
    const int cg = grid_for(P, 4, 16384);
    hipLaunchKernelGGL(dmx_copy, dim3(cg), dim3(256), 0, d->stream, perm, P, d->rs[0], d->src[0], o1, d->out[0]);
    DK(hipGetLastError());
    if (paired) {
        hipLaunchKernelGGL(dmx_copy, dim3(cg), dim3(256), 0, d->stream, perm, P, d->rs[1], d->src[1], o2, d->out[1]);
        DK(hipGetLastError());
    }
    DK(hipStreamSynchronize(d->stream));
    d->out_len[0] = s1;
    d->out_len[1] = s2;
    d->hoff[0] = h1;
    d->hoff[1] = h2;
    d->routed_ok = d->stats_ok = d->cycles_ok = P;
    d->bstats_ok = d->rbin_loaded ? P : 0;
    return FR_OK;
}

// ---- the windows' tally: mode and call order are checked here, the work is fr_dmx_tally.hip's
static int tally_ready(fr_dmx* d, const char* what) {
    if (d->key_mode && d->tally) return FR_OK;
    d->err = std::string(what) + (d->key_mode ? ": no fr_dmx_tally_begin" : ": sheet mode only (fr_dmx_set_sheet)");
    return FR_ERR_INVALID;
}

int fr_dmx_tally_begin(fr_dmx* d, uint64_t initial_slots) {
    if (!d->key_mode) return d->err = "fr_dmx_tally_begin: sheet mode only (fr_dmx_set_sheet)", FR_ERR_INVALID;
    DK(hipSetDevice(d->device));
    d->routed_ok = 0;
    return dmx_tally_begin(&d->tally, d->device, d->stream, initial_slots, d->err);
}

int fr_dmx_tally_file(fr_dmx* d, int64_t file_index) {
    if (int rc = tally_ready(d, "fr_dmx_tally_file")) return rc;
    DK(hipSetDevice(d->device));
    return dmx_tally_file(d->tally, file_index, d->err);
}

int fr_dmx_tally_window(fr_dmx* d, uint64_t n_pairs, uint64_t first_record) {
    if (int rc = tally_ready(d, "fr_dmx_tally_window")) return rc;
    if (n_pairs != d->routed_ok)
        return d->err = "fr_dmx_tally_window: n_pairs differs from the pairs the last fr_dmx_route routed (or they "
                        "are counted already)", FR_ERR_INVALID;
    DK(hipSetDevice(d->device));
    d->routed_ok = 0;
    return dmx_tally_window(d->tally, d->rkey, n_pairs, first_record, d->err);
}

int fr_dmx_tally_sizes(fr_dmx* d, uint64_t* n_unique, uint64_t* n_presence) {
    if (int rc = tally_ready(d, "fr_dmx_tally_sizes")) return rc;
    DK(hipSetDevice(d->device));
    return dmx_tally_sizes(d->tally, n_unique, n_presence, d->err);
}

int fr_dmx_tally_get(fr_dmx* d, uint64_t* keys, uint64_t* counts, uint64_t* first, uint32_t* pres_unique,
                     uint32_t* pres_file, uint64_t* pres_reads) {
    if (int rc = tally_ready(d, "fr_dmx_tally_get")) return rc;
    DK(hipSetDevice(d->device));
    return dmx_tally_get(d->tally, keys, counts, first, pres_unique, pres_file, pres_reads, d->err);
}

int fr_dmx_tally_rows_device(fr_dmx* d, void* dev_rows, uint64_t cap) {
    if (int rc = tally_ready(d, "fr_dmx_tally_rows_device")) return rc;
    DK(hipSetDevice(d->device));
    return dmx_tally_rows_device(d->tally, dev_rows, cap, d->err);
}

// ---- the windows' statistics: the call order is checked here, the work is fr_dmx_stats.hip's
int fr_dmx_stats_begin(fr_dmx* d, int n_dest) {
    DK(hipSetDevice(d->device));
    DK(hipStreamSynchronize(d->stream));  // an earlier window's sums may still be queued on the old accumulators
    d->stats_ok = 0;
    return dmx_stats_begin(&d->stats, d->device, d->stream, n_dest, d->err);
}

int fr_dmx_stats_window(fr_dmx* d, uint64_t n_pairs) {
    if (!d->stats) return d->err = "fr_dmx_stats_window: no fr_dmx_stats_begin", FR_ERR_INVALID;
    if (n_pairs != d->stats_ok)
        return d->err = "fr_dmx_stats_window: n_pairs differs from the pairs the last fr_dmx_route routed (or they "
                        "are added already)", FR_ERR_INVALID;
    if (d->hoff[0].size() > (size_t)dmx_stats_n_dest(d->stats) + 1)
        return d->err = "fr_dmx_stats_window: the last fr_dmx_route had more destinations than fr_dmx_stats_begin",
               FR_ERR_INVALID;
    DK(hipSetDevice(d->device));
    d->stats_ok = 0;
    if (d->n_mates == 1)  // the launch covers mate 0 alone: mate 1's half of the accumulators stays zero
        return dmx_stats_window(d->stats, d->out[0], nullptr, d->o1, d->l1, nullptr, nullptr, d->k_out, n_pairs, d->err);
    return dmx_stats_window(d->stats, d->out[0], d->out[1], d->o1, d->l1, d->o2, d->l2, d->k_out, n_pairs, d->err);
}

int fr_dmx_stats_get(fr_dmx* d, int n_dest, uint64_t* out) {
    if (!d->stats) return d->err = "fr_dmx_stats_get: no fr_dmx_stats_begin", FR_ERR_INVALID;
    if (n_dest != dmx_stats_n_dest(d->stats))
        return d->err = "fr_dmx_stats_get: n_dest differs from fr_dmx_stats_begin", FR_ERR_INVALID;
    DK(hipSetDevice(d->device));
    return dmx_stats_get(d->stats, out, d->err);
}

// ---- the windows' per-cycle statistics: the call order is checked here, the work is fr_dmx_cycles.hip's
int fr_dmx_cycles_begin(fr_dmx* d, int n_dest, int max_cycles) {
    if (!dmx_cycles_args_ok(n_dest, max_cycles))
        return d->err = "fr_dmx_cycles_begin: n_dest is negative or max_cycles is not in 1..1024", FR_ERR_INVALID;
    DK(hipSetDevice(d->device));
    DK(hipStreamSynchronize(d->stream));  // an earlier window's sums may still be queued on the old accumulators
    d->cycles_ok = 0;
    return dmx_cycles_begin(&d->cycles, d->device, d->stream, n_dest, max_cycles, d->err);
}

int fr_dmx_cycles_window(fr_dmx* d, uint64_t n_pairs) {
    if (!d->cycles) return d->err = "fr_dmx_cycles_window: no fr_dmx_cycles_begin", FR_ERR_INVALID;
    if (n_pairs != d->cycles_ok)
        return d->err = "fr_dmx_cycles_window: n_pairs differs from the pairs the last fr_dmx_route routed (or they "
                        "are added already)", FR_ERR_INVALID;
    if (d->hoff[0].size() > (size_t)dmx_cycles_n_dest(d->cycles) + 1)
        return d->err = "fr_dmx_cycles_window: the last fr_dmx_route had more destinations than fr_dmx_cycles_begin",
               FR_ERR_INVALID;
    DK(hipSetDevice(d->device));
    d->cycles_ok = 0;
    if (d->n_mates == 1)  // as fr_dmx_stats_window
        return dmx_cycles_window(d->cycles, d->out[0], nullptr, d->o1, d->l1, nullptr, nullptr, d->k_out, n_pairs,
                                 d->err);
    return dmx_cycles_window(d->cycles, d->out[0], d->out[1], d->o1, d->l1, d->o2, d->l2, d->k_out, n_pairs, d->err);
}

int fr_dmx_cycles_get(fr_dmx* d, int n_dest, int max_cycles, uint64_t* out) {
    if (!d->cycles) return d->err = "fr_dmx_cycles_get: no fr_dmx_cycles_begin", FR_ERR_INVALID;
    if (n_dest != dmx_cycles_n_dest(d->cycles) || max_cycles != dmx_cycles_max_cycles(d->cycles))
        return d->err = "fr_dmx_cycles_get: n_dest or max_cycles differs from fr_dmx_cycles_begin", FR_ERR_INVALID;
    DK(hipSetDevice(d->device));
    return dmx_cycles_get(d->cycles, out, d->err);
}

// ---- the windows' index mismatch table: mode and call order are checked here, the work is fr_dmx_bstats.hip's
int fr_dmx_bstats_begin(fr_dmx* d, int n_dest) {
    if (!d->key_mode) return d->err = "fr_dmx_bstats_begin: sheet mode only (fr_dmx_set_sheet)", FR_ERR_INVALID;
    DK(hipSetDevice(d->device));
    d->bstats_ok = 0;
    return dmx_bstats_begin(&d->bstats, d->device, d->stream, n_dest, d->err);
}

int fr_dmx_bstats_patch(fr_dmx* d, const uint64_t* recs, const uint8_t* bins, uint64_t n) {
    if (!d->bstats || !d->rbin_loaded)
        return d->err = d->n_mates == 2 ? "fr_dmx_bstats_patch: no R2 window loaded since fr_dmx_bstats_begin"
                                        : "fr_dmx_bstats_patch: no window loaded since fr_dmx_bstats_begin",
               FR_ERR_INVALID;
    DK(hipSetDevice(d->device));
    for (u64 k = 0; k < n; ++k)
        if (recs[k] >= d->nrec[d->code_mate()]) return d->err = "record index out of range", FR_ERR_INVALID;
    if (n >= DMX_BATCH) {  // many records: the whole array there and back, two copies
        std::vector<u8> all(d->nrec[d->code_mate()]);
        DK(hipMemcpy(all.data(), d->rbin, all.size(), hipMemcpyDeviceToHost));
        for (u64 k = 0; k < n; ++k) all[recs[k]] = bins[k];
        DK(hipMemcpy(d->rbin, all.data(), all.size(), hipMemcpyHostToDevice));
        return FR_OK;
    }
    for (u64 k = 0; k < n; ++k) DK(hipMemcpyAsync(d->rbin + recs[k], bins + k, 1, hipMemcpyHostToDevice, d->stream));
    DK(hipStreamSynchronize(d->stream));
    return FR_OK;
}

int fr_dmx_bstats_window(fr_dmx* d, uint64_t n_pairs) {
    if (!d->bstats) return d->err = "fr_dmx_bstats_window: no fr_dmx_bstats_begin", FR_ERR_INVALID;
    if (n_pairs != d->bstats_ok)
        return d->err = "fr_dmx_bstats_window: n_pairs differs from the pairs the last fr_dmx_route routed (or they "
                        "are counted already, or were classified before fr_dmx_bstats_begin)",
               FR_ERR_INVALID;
    if (d->hoff[0].size() > (size_t)dmx_bstats_n_dest(d->bstats) + 1)
        return d->err = "fr_dmx_bstats_window: the last fr_dmx_route had more destinations than fr_dmx_bstats_begin",
               FR_ERR_INVALID;
    DK(hipSetDevice(d->device));
    d->bstats_ok = 0;
    return dmx_bstats_window(d->bstats, d->k_out, d->perm, d->rbin, n_pairs, d->err);
}

int fr_dmx_bstats_get(fr_dmx* d, int n_dest, uint64_t* out) {
    if (!d->bstats) return d->err = "fr_dmx_bstats_get: no fr_dmx_bstats_begin", FR_ERR_INVALID;
    if (n_dest != dmx_bstats_n_dest(d->bstats))
        return d->err = "fr_dmx_bstats_get: n_dest differs from fr_dmx_bstats_begin", FR_ERR_INVALID;
    DK(hipSetDevice(d->device));
    return dmx_bstats_get(d->bstats, out, d->err);
}

// ---- the windows' validation: the call order is checked here, the work is fr_dmx_validate.hip's
int fr_dmx_validate_begin(fr_dmx* d) {
    DK(hipSetDevice(d->device));
    d->vqueued = false;
    return dmx_validate_begin(&d->validate, d->device, d->stream, d->err);
}

int fr_dmx_validate_window(fr_dmx* d, uint64_t n_pairs) {
    if (!d->validate) return d->err = "fr_dmx_validate_window: no fr_dmx_validate_begin", FR_ERR_INVALID;
    const int cm = d->code_mate();
    if (!d->vloaded[0] || !d->vloaded[cm])
        return d->err = cm ? "fr_dmx_validate_window: not both mates are loaded since the last fr_dmx_validate_window"
                           : "fr_dmx_validate_window: the mate is not loaded since the last fr_dmx_validate_window",
               FR_ERR_INVALID;
    if (n_pairs > std::min(d->nrec[0], d->nrec[cm]))
        return d->err = cm ? "fr_dmx_validate_window: n_pairs is beyond a mate's records"
                           : "fr_dmx_validate_window: n_pairs is beyond the mate's records", FR_ERR_INVALID;
    DK(hipSetDevice(d->device));
    // one mate: no second buffer, the kernel's instantiation that checks kinds 1-4 of mate 0 alone
    const int rc = cm ? dmx_validate_window(d->validate, d->src[0], d->src[1], d->rs[0], d->rs[1], n_pairs, d->err)
                      : dmx_validate_window(d->validate, d->src[0], nullptr, d->rs[0], nullptr, n_pairs, d->err);
    if (rc == FR_OK) {
        d->vloaded[0] = d->vloaded[1] = false;
        d->vqueued = true;
    }
    return rc;
}

int fr_dmx_validate_result(fr_dmx* d, int64_t* first_pair, int32_t* kind) {
    if (!d->validate || !d->vqueued)
        return d->err = "fr_dmx_validate_result: no fr_dmx_validate_window is queued", FR_ERR_INVALID;
    DK(hipSetDevice(d->device));
    return dmx_validate_result(d->validate, first_pair, kind, d->err);
}

int fr_dmx_validate_end(fr_dmx* d) {
    DK(hipSetDevice(d->device));
    dmx_validate_destroy(d->validate);  // (waits for the stream: a queued window still writes the word)
    d->validate = nullptr;
    d->vqueued = false;
    return FR_OK;
}

// ---- the GPU reader of BGZF mates: the arguments are checked here and a filled window is indexed here, the
// files, the staging and the window buffers are fr_dmx_reader.hip's
int fr_dmx_bgzf_open(fr_dmx* d, int mate, const char* path, uint64_t chunk_bytes, int* taken) {
    if (mate < 0 || mate > 1 || !taken) return d->err = "fr_dmx_bgzf_open: mate must be 0 (R1) or 1 (R2)", FR_ERR_INVALID;
    if (no_mate(d, mate, "fr_dmx_bgzf_open")) return FR_ERR_INVALID;
    return dmx_reader_open(&d->reader, d->device, d->stream, mate, path, chunk_bytes, taken, d->err);
}

int fr_dmx_bgzf_fill(fr_dmx* d, int mate, uint64_t keep_from, uint64_t want, uint64_t* n_records, uint64_t* len,
                     int* eof, int* handed_over, uint64_t* resume) {
    if (no_mate(d, mate, "fr_dmx_bgzf_fill")) return FR_ERR_INVALID;
    if (mate < 0 || mate > 1 || !dmx_reader_is_open(d->reader, mate))
        return d->err = "fr_dmx_bgzf_fill: no file is open for the mate (fr_dmx_bgzf_open)", FR_ERR_INVALID;
    const u8* win = nullptr;
    *n_records = 0;
    if (int rc = dmx_reader_fill(d->reader, mate, keep_from, want, &win, len, eof, handed_over, resume, d->err))
        return rc;
    if (*handed_over) {  // the carry alone, for fr_dmx_window_read: no records until the host loads its window
        d->src[mate] = win;
        d->len[mate] = *len;
        d->nrec[mate] = 0;
        d->routed_ok = d->stats_ok = d->cycles_ok = d->bstats_ok = 0;
        d->vloaded[mate] = false;
        if (mate == d->code_mate()) d->rbin_loaded = false;
        return FR_OK;
    }
    return dmx_index_mate(d, mate, win, *len, n_records);
}

int fr_dmx_bgzf_close(fr_dmx* d, int mate) {
    if (mate < 0 || mate > 1) return d->err = "fr_dmx_bgzf_close: mate must be 0 (R1) or 1 (R2)", FR_ERR_INVALID;
    if (no_mate(d, mate, "fr_dmx_bgzf_close")) return FR_ERR_INVALID;
    dmx_reader_close(d->reader, mate);
    return FR_OK;
}

int fr_dmx_bgzf_info(fr_dmx* d, int mate, double out[8]) {
    if (mate < 0 || mate > 1 || !out) return d->err = "fr_dmx_bgzf_info: mate must be 0 (R1) or 1 (R2)", FR_ERR_INVALID;
    if (no_mate(d, mate, "fr_dmx_bgzf_info")) return FR_ERR_INVALID;
    dmx_reader_info(d->reader, mate, out);
    return FR_OK;
}

int fr_dmx_window_read(fr_dmx* d, int mate, uint64_t start, uint64_t end, uint8_t* out) {
    if (mate < 0 || mate > 1) return d->err = "fr_dmx_window_read: mate must be 0 (R1) or 1 (R2)", FR_ERR_INVALID;
    if (no_mate(d, mate, "fr_dmx_window_read")) return FR_ERR_INVALID;
    if (start > end || end > d->len[mate] || (end > start && !d->src[mate]))
        return d->err = "fr_dmx_window_read: the span is not inside the mate's window", FR_ERR_INVALID;
    DK(hipSetDevice(d->device));
    if (end > start) DK(hipMemcpy(out, d->src[mate] + start, end - start, hipMemcpyDeviceToHost));
    return FR_OK;
}

// the routed bytes of a mate through its fr_defl: gzip streams (crc32 set) or BGZF member runs
static int dmx_deflate(fr_dmx* d, int mate, int n_dest, uint64_t* comp_bytes, uint32_t* crc32, bool bgzf) {
    if (mate < 0 || mate > 1) return d->err = "mate must be 0 (R1) or 1 (R2)", FR_ERR_INVALID;
    if (no_mate(d, mate, "fr_dmx_deflate")) return FR_ERR_INVALID;
    if (n_dest < 0 || (u64)n_dest + 1 != d->hoff[mate].size())
        return d->err = "fr_dmx_deflate: n_dest differs from the last fr_dmx_route", FR_ERR_INVALID;
    DK(hipSetDevice(d->device));
    if (!d->defl[mate]) {
        d->defl[mate] = fr_defl_create_on(d->device, d->stream);
        const char* e = fr_defl_last_error(d->defl[mate]);
        if (e && *e) return d->err = std::string("fr_dmx_deflate: ") + e, FR_ERR_HIP;
    }
    const int rc = bgzf ? fr_defl_run_bgzf(d->defl[mate], d->out[mate], d->hoff[mate].data(), n_dest, comp_bytes)
                        : fr_defl_run(d->defl[mate], d->out[mate], d->hoff[mate].data(), n_dest, comp_bytes, crc32);
    if (rc != FR_OK) d->err = std::string("fr_dmx_deflate: ") + fr_defl_last_error(d->defl[mate]);
    return rc;
}

int fr_dmx_deflate(fr_dmx* d, int mate, int n_dest, uint64_t* comp_bytes, uint32_t* crc32) {
    return dmx_deflate(d, mate, n_dest, comp_bytes, crc32, false);
}

int fr_dmx_deflate_bgzf(fr_dmx* d, int mate, int n_dest, uint64_t* comp_bytes) {
    return dmx_deflate(d, mate, n_dest, comp_bytes, nullptr, true);
}

int fr_dmx_fetch_deflated(fr_dmx* d, int mate, uint8_t* out, uint64_t len) {
    if (no_mate(d, mate, "fr_dmx_fetch_deflated")) return FR_ERR_INVALID;
    if (mate < 0 || mate > 1 || !d->defl[mate]) return d->err = "fr_dmx_fetch_deflated: bad mate or no fr_dmx_deflate", FR_ERR_INVALID;
    const int rc = fr_defl_fetch(d->defl[mate], out, len);
    if (rc != FR_OK) d->err = std::string("fr_dmx_fetch_deflated: ") + fr_defl_last_error(d->defl[mate]);
    return rc;
}

int fr_dmx_fetch(fr_dmx* d, int mate, uint8_t* out, uint64_t len) {
    if (no_mate(d, mate, "fr_dmx_fetch")) return FR_ERR_INVALID;
    if (mate < 0 || mate > 1 || len > d->out_len[mate]) return d->err = "fr_dmx_fetch: bad mate or length", FR_ERR_INVALID;
    DK(hipSetDevice(d->device));
    if (len) DK(hipMemcpy(out, d->out[mate], len, hipMemcpyDeviceToHost));
    return FR_OK;
}

}  // extern "C"
