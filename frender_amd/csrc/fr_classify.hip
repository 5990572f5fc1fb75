// fr_classify.hip — the Hamming classifier: frender.py:214-234 (Hamming), :237-291 (classes), :294-351 (rc).
//
//  classify_kernel     : one lane per unique code of a scan's table (fr_classify)
//  dmx_class_kernel    : one lane per R2 record of a demux window (fr_dmx_set_sheet), no rc, no sums
//  nbr_* kernels       : the sheet's neighbourhood maps both of them probe first
//  classify_cp_kernel  : the code-point fallback for codes outside the fast alphabet
//
// Both packed-key kernels take a code through the same steps: split at '+' (split_fast_key /
// split_wide_key), the length asserts (length_error), maps or exact row scan (class_code), the one class
// rule (class_rule).  Design notes: DESIGN.md §4.3, §4.4.
#include <algorithm>

#include "../../include/frender_amd.h"
#include "fr_internal.h"

namespace fr {

__device__ __forceinline__ int mism(u64 q, u64 s) {  // Hamming distance of two 3-bit packed strings
    const u64 x = q ^ s;
    return __popcll((x | (x >> 1) | (x >> 2)) & 0x1249249249249249ull);
}

constexpr int CLS_WG = 256;
constexpr int CLS_LDS_BYTES = 48 * 1024;  // dynamic LDS cap; the per-name rc sums may take half of it

__device__ __forceinline__ int mism32(u32 q, u32 s) {  // <= 10 symbols: 30 bits
    const u32 x = q ^ s;
    return __popc((x | (x >> 1) | (x >> 2)) & 0x09249249u);
}

template <typename W>
__device__ __forceinline__ int mism_w(W q, W s) {
    if constexpr (sizeof(W) == 4) return mism32(q, s);
    else return mism(q, s);
}

// R7/R8 for one code, the forward idx2 call and the rc(idx2) call side by side (idx1's matches are shared)
struct PairClass {
    int m1, m2, cls, row;  // first matching row of idx1 / idx2, class, the sample's row when demuxable
    int rm2, rcls, rrow;   // the same of the rc(idx2) call
};

// The class rule: from the first matching row of each list (m1, m2, rm2; -1 none), |M1 ∩ M2| (both, rboth)
// and its first row (r, rr).
__device__ __forceinline__ PairClass class_rule(int m1, int m2, int rm2, int both, int r, int rboth, int rr) {
    PairClass c;
    if (m1 >= 0 && m2 >= 0) {
        c.cls = both == 0 ? CLS_HOP : both == 1 ? CLS_DEMUX : CLS_AMBIG;
        c.row = both == 1 ? r : -1;
    } else {
        c.cls = CLS_UNDET;
        c.row = -1;
    }
    if (m1 >= 0 && rm2 >= 0) {
        c.rcls = rboth == 0 ? CLS_HOP : rboth == 1 ? CLS_DEMUX : CLS_AMBIG;
        c.rrow = rboth == 1 ? rr : -1;
    } else {
        c.rcls = CLS_UNDET;
        rm2 = -1;
        c.rrow = -1;
    }
    if (c.cls == CLS_UNDET) {  // pass A keeps matched_idx1 from the rc call (frender.py:319-323)
        if (c.rcls == CLS_UNDET) m1 = -1;
        m2 = -1;
    }
    c.m1 = m1;
    c.m2 = m2;
    c.rm2 = rm2;
    return c;
}

// The exact scan over every sheet row, forward idx2 and (RC) rc(idx2) in the same pass: the first matching
// row of each list, |M1 ∩ M2| and its first row.  The rows are read straight from the u64 sheet arrays in HBM:
// the row index is uniform, so every row arrives by scalar loads and the distance ops take it as a
// scalar operand (no LDS read per row), and the bookkeeping runs only on rows some lane matches
// (a code matches one or two rows of a well-separated sheet: the wave skips ~2/3 of the updates).
template <typename W, bool RC>
__device__ __forceinline__ PairClass class_pair_s(W q1, W q2, const u64* __restrict__ s1, const u64* __restrict__ s2,
                                                  const u64* __restrict__ s2rc, int S, int nsubs1, int nsubs2) {
    int m1 = -1, m2 = -1, rm2 = -1;
    int both = 0, r = -1, rboth = 0, rr = -1;
#pragma unroll 8
    for (int i = 0; i < S; ++i) {
        const bool a = mism_w<W>(q1, (W)s1[i]) <= nsubs1;
        const bool b = mism_w<W>(q2, (W)s2[i]) <= nsubs2;
        const bool c = RC && mism_w<W>(q2, (W)s2rc[i]) <= nsubs2;
        if (a || b || c) {
            m1 = (a && m1 < 0) ? i : m1;
            m2 = (b && m2 < 0) ? i : m2;
            r = (a && b && both == 0) ? i : r;
            both += (a && b) ? 1 : 0;
            rm2 = (c && rm2 < 0) ? i : rm2;
            rr = (a && c && rboth == 0) ? i : rr;
            rboth += (a && c) ? 1 : 0;
        }
    }
    return class_rule(m1, m2, rm2, both, r, rboth, rr);
}

// ------------------------------------------------------------------------------------
// classify neighbourhood maps (fr_internal.h NbrMap): a code is classified by three map probes and
// two pair probes instead of a scan over every sheet row
// ------------------------------------------------------------------------------------
__host__ __device__ inline u64 nbr_binom(int n, int k) {
    if (k < 0 || k > n) return 0;
    u64 r = 1;
    for (int j = 1; j <= k; ++j) r = r * (u64)(n - k + j) / (u64)j;
    return r;
}

u64 nbr_codes_per_row(int L, int nsubs) {
    u64 t = 0, p5 = 1;
    for (int d = 0; d <= nsubs && d <= L; ++d, p5 *= 5) t += nbr_binom(L, d) * p5;
    return t;
}

template <class SL>
__device__ __forceinline__ SL* nbr_claim(SL* t, u32 mask, u64 key) {  // the table has >= 2x free slots
    u32 h = (u32)mix64(key) & mask;
    for (;;) {
        const u64 prev = atomicCAS((unsigned long long*)&t[h].key, 0ull, (unsigned long long)key);
        if (prev == 0 || prev == key) return &t[h];
        h = (h + 1) & mask;
    }
}

// thread per (row, neighbour index t): t ranks (d, combination of d positions, d symbols in 1..5);
// substitutions equal to the row's own symbol are left to the smaller d that produces the same code
__global__ void nbr_insert_kernel(const u64* __restrict__ vals, const int32_t* __restrict__ canon, int S, int L,
                                  int nsubs, u64 T, NSlot* m, u32 mask) {
    const u64 g = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (g >= (u64)S * T) return;
    const int i = (int)(g / T);
    u64 t = g % T;
    if (canon[i] != i) return;  // one insertion per distinct value
    int d = 0;
    u64 p5 = 1;
    for (;; ++d, p5 *= 5) {
        const u64 nd = nbr_binom(L, d) * p5;
        if (t < nd) break;
        t -= nd;
    }
    u64 sub = t % p5, comb = t / p5;
    u64 v = vals[i];
    for (int k = d; k >= 1; --k) {  // colex unranking of the position set
        int c = k - 1;
        while (nbr_binom(c + 1, k) <= comb) ++c;
        comb -= nbr_binom(c, k);
        const u64 sy = sub % 5u + 1u;
        sub /= 5u;
        if (((v >> (3 * c)) & 7u) == sy) return;
        v = (v & ~(7ull << (3 * c))) | (sy << (3 * c));
    }
    NSlot* e = nbr_claim(m, mask, v | NBR_KEY);
    atomicMax(&e->vmin_c, ~(u32)i);
    atomicMax(&e->vmax1, (u32)i + 1u);
}

__global__ void nbr_pair_kernel(const int32_t* __restrict__ canon, int S, int rc, PSlot* p0, u32 m0, PSlot* p1,
                                u32 m1) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S) return;
    const u64 a = (u64)(u32)canon[i] << 32;
    PSlot* e = nbr_claim(p0, m0, a | (u32)canon[S + i] | NBR_KEY);
    atomicAdd(&e->cnt, 1u);
    atomicMax(&e->first_c, ~(u32)i);
    if (rc) {
        e = nbr_claim(p1, m1, a | (u32)canon[2 * S + i] | NBR_KEY);
        atomicAdd(&e->cnt, 1u);
        atomicMax(&e->first_c, ~(u32)i);
    }
}

hipError_t launch_nbr_build(const SheetArgs& sh, const int32_t* canon, int nsubs1, int nsubs2, int rc,
                            const NbrMap& nm, hipStream_t s) {
    const u64* vals[3] = {sh.i1, sh.i2, sh.i2rc};
    const int len[3] = {sh.L1u, sh.L2u, sh.L2u};
    for (int l = 0; l < (rc ? 3 : 2); ++l) {
        const int nsubs = l == 0 ? nsubs1 : nsubs2;  // the idx1 list at its radius, idx2 and rc(idx2) at theirs
        const u64 T = nbr_codes_per_row(len[l], nsubs);
        const u64 n = (u64)sh.S * T;
        hipLaunchKernelGGL(nbr_insert_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, s, vals[l], canon + l * sh.S,
                           sh.S, len[l], nsubs, T, nm.m[l], nm.mmask[l]);
    }
    hipLaunchKernelGGL(nbr_pair_kernel, dim3((u32)((sh.S + 255) / 256)), dim3(256), 0, s, canon, sh.S, rc, nm.p[0],
                       nm.pmask[0], nm.p[1], nm.pmask[1]);
    return hipGetLastError();
}

// one map probe chain from a slot already loaded (the caller issues the first loads of several chains
// together, so a code waits for one round trip per stage, not one per map)
__device__ __forceinline__ int nbr_resolve(const NSlot* __restrict__ t, u32 mask, u64 key, u32 h, NSlot e) {
    for (;;) {
        if (e.key == key) return ~e.vmin_c == e.vmax1 - 1u ? (int)~e.vmin_c : -2;
        if (e.key == 0) return -1;
        h = (h + 1) & mask;
        e = t[h];
    }
}

// nbr_find on the idx1, idx2 and (rc) rc(idx2) maps with the three first probes in flight together:
// per map the single row value near the code, -1 for none, -2 for several distinct values
__device__ __forceinline__ void nbr_find3(const NbrMap& nm, u64 q1, u64 q2, bool rc, int& a1, int& a2, int& a3) {
    const u64 k1 = q1 | NBR_KEY, k2 = q2 | NBR_KEY;
    const u32 h1 = (u32)mix64(k1) & nm.mmask[0], h2 = (u32)mix64(k2) & nm.mmask[1], h3 = (u32)mix64(k2) & nm.mmask[2];
    const NSlot e1 = nm.m[0][h1], e2 = nm.m[1][h2];
    const NSlot e3 = rc ? nm.m[2][h3] : NSlot{0, 0, 0};
    a1 = nbr_resolve(nm.m[0], nm.mmask[0], k1, h1, e1);
    a2 = nbr_resolve(nm.m[1], nm.mmask[1], k2, h2, e2);
    a3 = rc ? nbr_resolve(nm.m[2], nm.mmask[2], k2, h3, e3) : -1;
}

__device__ __forceinline__ void pair_resolve(const PSlot* __restrict__ t, u32 mask, u64 key, u32 h, PSlot e, int& both,
                                             int& r) {
    for (;;) {
        if (e.key == key) {
            both = (int)e.cnt;
            r = (int)~e.first_c;
            return;
        }
        if (e.key == 0) return;
        h = (h + 1) & mask;
        e = t[h];
    }
}

// class_pair_s's result from the map probes: the rows near q1 are exactly the rows holding value a1 (a
// single distinct value), so its first row is a1 and |M1 ∩ M2| is the pair count of (a1, a2).  The two
// pair maps' first probes are in flight together.
__device__ __forceinline__ PairClass class_pair_nbr(const NbrMap& nm, int a1, int a2, int a3) {
    int both = 0, r = -1, rboth = 0, rr = -1;
    const bool f0 = a1 >= 0 && a2 >= 0, f1 = a1 >= 0 && a3 >= 0;
    const u64 pk0 = ((u64)(u32)a1 << 32) | (u32)a2 | NBR_KEY, pk1 = ((u64)(u32)a1 << 32) | (u32)a3 | NBR_KEY;
    const u32 ph0 = (u32)mix64(pk0) & nm.pmask[0], ph1 = (u32)mix64(pk1) & nm.pmask[1];
    const PSlot p0 = f0 ? nm.p[0][ph0] : PSlot{0, 0, 0};
    const PSlot p1 = f1 ? nm.p[1][ph1] : PSlot{0, 0, 0};
    if (f0) pair_resolve(nm.p[0], nm.pmask[0], pk0, ph0, p0, both, r);
    if (f1) pair_resolve(nm.p[1], nm.pmask[1], pk1, ph1, p1, rboth, rr);
    return class_rule(a1, a2, a3, both, r, rboth, rr);
}

// ------------------------------------------------------------------------------------
// the per-code steps of classify_kernel and dmx_class_kernel
// ------------------------------------------------------------------------------------
// A fast key (symbols A1 C2 G3 T4 N5 '+'6, folded they equal the sheet's a1..n5) split at '+' like
// idx1, idx2 = code.split("+")[0:2] (frender.py:306), both halves packed 3 bits per letter like the sheet:
// false without a '+'.  single (a single-index sheet, uniform over the launch): the code is its idx1 alone,
// code.split("+")[0] -- every symbol without a '+' -- with n2 = 0, q2 = 0 whatever follows; always true.
__device__ __forceinline__ bool split_fast_key(u64 key, bool single, int& n1, int& n2, u64& q1, u64& q2) {
    // SWAR over the 21 3-bit groups: len = symbols before the first empty group; the '+'
    // groups (== 6) among them give p1, p2 (no per-symbol loop)
    constexpr u64 G0 = 0x1249249249249249ull & ((1ull << 63) - 1ull);  // bit 0 of each group
    const u64 nz = (key | (key >> 1) | (key >> 2)) & G0;                // groups holding a symbol
    const u64 empty = ~nz & G0;
    const int len = empty ? (int)(__builtin_ctzll(empty) / 3) : MAXSYM;
    const u64 x = key ^ (G0 * 6ull);                                    // '+' groups become 0
    u64 pm = ~(x | (x >> 1) | (x >> 2)) & G0;
    pm &= len < MAXSYM ? (1ull << (3 * len)) - 1ull : ~0ull;
    const int p1 = pm ? (int)(__builtin_ctzll(pm) / 3) : -1;
    pm &= pm - 1ull;
    const int p2 = pm ? (int)(__builtin_ctzll(pm) / 3) : MAXSYM;
    const bool plus = p1 >= 0;
    if (plus) {
        n1 = p1;
        const int e2 = p2 < len ? p2 : len;
        n2 = e2 - p1 - 1;
        q1 = n1 ? (key & ((1ull << (3 * n1)) - 1ull)) : 0ull;
        q2 = n2 ? ((key >> (3 * (p1 + 1))) & ((1ull << (3 * n2)) - 1ull)) : 0ull;
    }
    if (single) {
        if (!plus) {
            n1 = len;
            q1 = key;
        }
        n2 = 0;
        q2 = 0;
    }
    return plus || single;
}

// The same split of a wide key (fr_internal.h: more than 21 symbols): base-5 letters, the '+' position in
// bits 57-61 (WIDE_NOPLUS without one).  Either part of a wide key has at most 21 letters (wide_encode), so
// q1 always fits the packed form, with or without a '+'.
__device__ __forceinline__ bool split_wide_key(u64 key, bool single, int& n1, int& n2, u64& q1, u64& q2) {
    const u64 V = key & ((1ull << 57) - 1ull);
    const int pp = (int)((key >> 57) & 31u);
    int nl = 0;
    u64 off = 0, pw = 1;
    while (nl < WIDE_MAXN && off + pw <= V) {  // off = (5^nl - 1) / 4
        off += pw;
        pw *= 5;
        ++nl;
    }
    u64 D = V - off;
    const bool plus = pp != WIDE_NOPLUS;
    n1 = plus ? pp : nl;
    n2 = plus ? nl - pp : 0;
    for (int i = 0; i < nl; ++i) {
        const u64 sy = D % 5u + 1u;
        D /= 5u;
        if (i < n1) q1 |= sy << (3 * i);
        else q2 |= sy << (3 * (i - n1));
    }
    if (single) {
        n2 = 0;
        q2 = 0;
    }
    return plus || single;
}

// the length asserts (frender.py:227-229), idx1 list first: 1 idx1, 2 idx2, 0 none.  A single-index sheet's idx2
// entries are all empty (L2u = 0) and its codes split with n2 = 0: idx1's length alone decides.
__device__ __forceinline__ int length_error(const SheetArgs& sh, int n1, int n2) {
    if (sh.S > 0 && (sh.L1u == -2 || sh.L1u != n1)) return 1;
    if (sh.S > 0 && (sh.L2u == -2 || sh.L2u != n2)) return 2;
    return 0;
}

// One split code against the sheet: the maps when they are on, the exact row scan when they are off or a map
// answers -2 (the code lies near several distinct sheet values).  Without RC a3 stays -1.
template <typename W, bool RC>
__device__ __forceinline__ PairClass class_code(const SheetArgs& sh, const NbrMap& nm, u64 q1, u64 q2, int nsubs1,
                                                int nsubs2) {
    int a1 = -2, a2 = -2, a3 = -1;
    if (nm.on) nbr_find3(nm, q1, q2, RC, a1, a2, a3);
    if (a1 != -2 && a2 != -2 && a3 != -2) return class_pair_nbr(nm, a1, a2, a3);
    return class_pair_s<W, RC>((W)q1, (W)q2, sh.i1, sh.i2, sh.i2rc, sh.S, nsubs1, nsubs2);
}

// One lane per unique code; W is u32 when every sheet entry has <= 10 symbols, else u64.  The per-name rc
// sums live in dynamic LDS when they fit (names_in_lds), else they go to the global atomics.
template <typename W>
__global__ __launch_bounds__(CLS_WG) void classify_kernel(const u64* keys, const u64* counts, u64 n, SheetArgs sh,
                                                          int nsubs1, int nsubs2, int rc, ClassOut o, NbrMap nm,
                                                          int names_in_lds, u64* zero_next, u32 zero_n,
                                                          u64* err_flag) {
    extern __shared__ __attribute__((aligned(16))) u8 cls_lds[];
    // the error word + rc sums of the next fr_classify (the other of two alternating blocks): zeroed here,
    // so no call issues a memset dispatch for its own
    for (u64 i = blockIdx.x * (u64)CLS_WG + threadIdx.x; i < zero_n; i += (u64)gridDim.x * CLS_WG) zero_next[i] = 0;
    unsigned long long* lf = (unsigned long long*)cls_lds;
    unsigned long long* lr = lf + (names_in_lds ? sh.n_names : 0);
    if (rc && names_in_lds)
        for (int i = threadIdx.x; i < sh.n_names; i += CLS_WG) lf[i] = lr[i] = 0;
    __syncthreads();

    bool any_err = false;
    // grid-stride: the per-name sums stay in LDS over many codes (one flush per workgroup: the
    // flush's atomics all land on the same 2 x names addresses)
    for (u64 u = blockIdx.x * (u64)CLS_WG + threadIdx.x; u < n; u += (u64)gridDim.x * CLS_WG) {
        const u64 key = keys[u];
        int n1 = 0, n2 = 0;
        u64 q1 = 0, q2 = 0;
        const bool single = sh.single != 0;
        const bool plus = (key & WIDE_BIT) ? split_wide_key(key, single, n1, n2, q1, q2)
                                           : split_fast_key(key, single, n1, n2, q1, q2);
        const int err = plus ? length_error(sh, n1, n2) : 3;
        PairClass c = {-1, -1, CLS_UNDET, -1, -1, CLS_UNDET, -1};
        if (!err) {
            c = rc ? class_code<W, true>(sh, nm, q1, q2, nsubs1, nsubs2)
                   : class_code<W, false>(sh, nm, q1, q2, nsubs1, nsubs2);
            // both calls demuxable to different sample NAMES -> ambiguous (frender.py:336-349)
            if (rc && c.cls == CLS_DEMUX && c.rcls == CLS_DEMUX && sh.name[c.row] != sh.name[c.rrow]) {
                c.cls = CLS_AMBIG;
                c.row = -1;
                c.rcls = CLS_AMBIG;
                c.rrow = -1;
            }
        }
        if (err) {
            any_err = true;
            atomicMax((unsigned long long*)o.err_first, (unsigned long long)~u);  // = min u
            if (o.err_which) o.err_which[u] = err;
        } else if (o.err_which) {
            o.err_which[u] = 0;
        }
        o.m1[u] = (int16_t)c.m1;
        o.m2[u] = (int16_t)c.m2;
        o.cls[u] = (u8)c.cls;
        o.row[u] = (int16_t)c.row;
        if (rc) {
            o.rc_m2[u] = (int16_t)c.rm2;
            o.rc_cls[u] = (u8)c.rcls;
            o.rc_row[u] = (int16_t)c.rrow;
            // the record count only where a sum takes it (most codes are hops or undetermined)
            const u64 cnt = (c.cls == CLS_DEMUX || c.rcls == CLS_DEMUX) ? counts[u] : 0ull;
            if (c.cls == CLS_DEMUX) {
                const int nm = sh.name[c.row];
                if (names_in_lds) atomicAdd(&lf[nm], (unsigned long long)cnt);
                else atomicAdd((unsigned long long*)&o.rc_f[nm], (unsigned long long)cnt);
            }
            if (c.rcls == CLS_DEMUX) {
                const int nm = sh.name[c.rrow];
                if (names_in_lds) atomicAdd(&lr[nm], (unsigned long long)cnt);
                else atomicAdd((unsigned long long*)&o.rc_r[nm], (unsigned long long)cnt);
            }
        }
    }
    // pinned host memory (every lane that met an error stores the same value to the one address, once, after
    // its loop): the host reads the exact error word, kept by the atomicMax above, only when the flag is set
    if (any_err) *err_flag = 1;
    if (rc && names_in_lds) {
        __syncthreads();
        for (int i = threadIdx.x; i < sh.n_names; i += CLS_WG) {
            if (lf[i]) atomicAdd((unsigned long long*)&o.rc_f[i], lf[i]);
            if (lr[i]) atomicAdd((unsigned long long*)&o.rc_r[i], lr[i]);
        }
    }
}

// u32 distances when every sheet entry (and so every query that passes the length checks) has <= 10 symbols
static bool sheet_is_narrow(const SheetArgs& sh) {
    return sh.S > 0 && sh.L1u >= 0 && sh.L1u <= 10 && sh.L2u >= 0 && sh.L2u <= 10;
}

hipError_t launch_classify(const u64* keys, const u64* counts, u64 n, SheetArgs sh, int nsubs1, int nsubs2, int rc,
                           ClassOut o, const NbrMap& nm, u64* zero_next, u32 zero_n, u64* err_flag, hipStream_t s) {
    // (no codes: one workgroup still zeroes the next call's block)
    const size_t names_bytes = rc ? 2ull * 8 * sh.n_names : 0;
    const int names_in_lds = (rc && names_bytes <= CLS_LDS_BYTES / 2) ? 1 : 0;
    const size_t lds = (names_in_lds ? names_bytes : 0) + 16;
    const u64 grid = std::max<u64>(1, std::min<u64>((n + CLS_WG - 1) / CLS_WG, 2048));
    if (sheet_is_narrow(sh))
        hipLaunchKernelGGL(classify_kernel<u32>, dim3((u32)grid), dim3(CLS_WG), lds, s, keys, counts, n, sh, nsubs1,
                           nsubs2, rc, o, nm, names_in_lds, zero_next, zero_n, err_flag);
    else
        hipLaunchKernelGGL(classify_kernel<u64>, dim3((u32)grid), dim3(CLS_WG), lds, s, keys, counts, n, sh, nsubs1,
                           nsubs2, rc, o, nm, names_in_lds, zero_next, zero_n, err_flag);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// demux key mode (fr_dmx_set_sheet): one lane per R2 record of a window, classified from its fast key as
// classify_kernel classifies a unique code without rc, and turned into the record's destination at once.
// No LDS: a sheet of any size takes the same path and registers alone bound the occupancy.
//
// EMIT (fr_dmx_bstats_begin, `demux -b --barcode-stats`): the record's mismatch bins go to rec_bin[u] as well, one
// byte bin1 * 5 + bin2 (bins 0, 1, 2, 3 = three or more, 4 = none).  The reference row of either index comes from
// the PairClass at hand: the assigned row of a demuxable code, the first matching row of each list (m1, m2) of a
// hop or an ambiguous code, none of an undetermined one (class_rule leaves m1 = m2 = -1 there); a single-index
// sheet has no index 2.  The map path may name another row of equal value: the distance is the same.  A record
// this kernel skips or fails gets DMX_NO_BIN.  Without EMIT the kernel is the one it was, argument block included:
// rec_bin is a pack of one pointer with EMIT and of nothing without it.
// ------------------------------------------------------------------------------------
template <typename W>
__device__ __forceinline__ u32 mism_bin(W q, const u64* __restrict__ rows, int row) {
    return row < 0 ? 4u : (u32)min(mism_w<W>(q, (W)rows[row]), 3);
}

template <typename W, bool EMIT, typename... Bin>
__global__ __launch_bounds__(CLS_WG) void dmx_class_kernel(const u64* __restrict__ rec_key, int32_t* rec_dest, u64 n,
                                                           SheetArgs sh, int nsubs1, int nsubs2, NbrMap nm,
                                                           const int32_t* __restrict__ row_dest, DmxClassDest cd,
                                                           Bin... bin_out) {
    static_assert(sizeof...(Bin) == (EMIT ? 1 : 0), "one u8* with EMIT, nothing without");
    [[maybe_unused]] u8* rec_bin = nullptr;
    if constexpr (EMIT) rec_bin = (bin_out, ...);
    for (u64 u = blockIdx.x * (u64)CLS_WG + threadIdx.x; u < n; u += (u64)gridDim.x * CLS_WG) {
        if (rec_dest[u] != DMX_PENDING) {  // exotic: the host resolves it
            if constexpr (EMIT) rec_bin[u] = DMX_NO_BIN;
            continue;
        }
        int n1 = 0, n2 = 0;
        u64 q1 = 0, q2 = 0;
        int32_t d;
        u32 bin = DMX_NO_BIN;
        if (!split_fast_key(rec_key[u], sh.single != 0, n1, n2, q1, q2)) {
            d = FR_DMX_NOPLUS;
        } else if (const int err = length_error(sh, n1, n2)) {
            d = err == 1 ? FR_DMX_LEN1 : FR_DMX_LEN2;
        } else {
            const PairClass c = class_code<W, false>(sh, nm, q1, q2, nsubs1, nsubs2);
            d = c.cls == CLS_DEMUX   ? row_dest[c.row]
                : c.cls == CLS_HOP   ? cd.v[CLS_HOP]
                : c.cls == CLS_AMBIG ? cd.v[CLS_AMBIG]
                                     : cd.v[CLS_UNDET];
            if constexpr (EMIT) {
                const bool dm = c.cls == CLS_DEMUX;
                const u32 b1 = mism_bin<W>((W)q1, sh.i1, dm ? c.row : c.m1);
                const u32 b2 = sh.single ? 4u : mism_bin<W>((W)q2, sh.i2, dm ? c.row : c.m2);
                bin = b1 * 5u + b2;
            }
        }
        rec_dest[u] = d;
        if constexpr (EMIT) rec_bin[u] = (u8)bin;
    }
}

hipError_t launch_dmx_classify(const u64* rec_key, int32_t* rec_dest, u64 n, SheetArgs sh, int nsubs1, int nsubs2,
                               const NbrMap& nm, const int32_t* row_dest, DmxClassDest cd, u8* rec_bin, hipStream_t s) {
    if (!n) return hipSuccess;
    const u64 grid = std::max<u64>(1, std::min<u64>((n + CLS_WG - 1) / CLS_WG, 2048));
    const bool narrow = sheet_is_narrow(sh);
    auto go = [&](auto kernel, auto... bin_out) {
        hipLaunchKernelGGL(kernel, dim3((u32)grid), dim3(CLS_WG), 0, s, rec_key, rec_dest, n, sh, nsubs1, nsubs2, nm,
                           row_dest, cd, bin_out...);
    };
    if (rec_bin) narrow ? go(dmx_class_kernel<u32, true, u8*>, rec_bin) : go(dmx_class_kernel<u64, true, u8*>, rec_bin);
    else narrow ? go(dmx_class_kernel<u32, false>) : go(dmx_class_kernel<u64, false>);
    return hipGetLastError();
}

// generic classifier over case-folded code points (codes outside the fast alphabet): class_pair_s on strings
__device__ PairClass class_pair_cp(const u32* q1, int n1, const u32* q2, int n2, const u32* s1, const u32* s2,
                                   const u32* s2rc, int stride, int S, int nsubs1, int nsubs2, bool rc) {
    int m1 = -1, m2 = -1, rm2 = -1;
    int both = 0, r = -1, rboth = 0, rr = -1;
    for (int i = 0; i < S; ++i) {
        int d1 = 0, d2 = 0, d3 = 0;
        for (int k = 0; k < n1; ++k) d1 += q1[k] != s1[(u64)i * stride + k];
        for (int k = 0; k < n2; ++k) d2 += q2[k] != s2[(u64)i * stride + k];
        for (int k = 0; rc && k < n2; ++k) d3 += q2[k] != s2rc[(u64)i * stride + k];
        const bool a = d1 <= nsubs1, b = d2 <= nsubs2, c = rc && d3 <= nsubs2;
        m1 = (a && m1 < 0) ? i : m1;
        m2 = (b && m2 < 0) ? i : m2;
        r = (a && b && both == 0) ? i : r;
        both += (a && b) ? 1 : 0;
        rm2 = (c && rm2 < 0) ? i : rm2;
        rr = (a && c && rboth == 0) ? i : rr;
        rboth += (a && c) ? 1 : 0;
    }
    return class_rule(m1, m2, rm2, both, r, rboth, rr);
}

__global__ void classify_cp_kernel(int n, const u32* q1, const int32_t* q1len, const u32* q2, const int32_t* q2len,
                                   int stride, int S, const u32* s1, const int32_t* s1len, const u32* s2,
                                   const int32_t* s2len, const u32* s2rc, const int32_t* name, int nsubs1, int nsubs2,
                                   int rc, ClassOut o) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n) return;
    const int n1 = q1len[u], n2 = q2len[u];
    int err = 0;
    for (int i = 0; i < S && !err; ++i)
        if (s1len[i] != n1) err = 1;
    for (int i = 0; i < S && !err; ++i)
        if (s2len[i] != n2) err = 2;
    PairClass c = {-1, -1, CLS_UNDET, -1, -1, CLS_UNDET, -1};
    if (!err) {
        c = class_pair_cp(q1 + (u64)u * stride, n1, q2 + (u64)u * stride, n2, s1, s2, s2rc, stride, S, nsubs1, nsubs2,
                          rc != 0);
        if (rc && c.cls == CLS_DEMUX && c.rcls == CLS_DEMUX && name[c.row] != name[c.rrow]) {
            c.cls = c.rcls = CLS_AMBIG;
            c.row = c.rrow = -1;
        }
    }
    if (o.err_which) o.err_which[u] = err;
    o.m1[u] = (int16_t)c.m1;
    o.m2[u] = (int16_t)c.m2;
    o.cls[u] = (u8)c.cls;
    o.row[u] = (int16_t)c.row;
    if (rc) {
        o.rc_m2[u] = (int16_t)c.rm2;
        o.rc_cls[u] = (u8)c.rcls;
        o.rc_row[u] = (int16_t)c.rrow;
    }
}

hipError_t launch_classify_cp(int n, const u32* q1, const int32_t* q1len, const u32* q2, const int32_t* q2len,
                              int stride, int S, const u32* s1, const int32_t* s1len, const u32* s2,
                              const int32_t* s2len, const u32* s2rc, const int32_t* name, int nsubs1, int nsubs2,
                              int rc, ClassOut o, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(classify_cp_kernel, dim3((n + 127) / 128), dim3(128), 0, s, n, q1, q1len, q2, q2len, stride,
                       S, s1, s1len, s2, s2len, s2rc, name, nsubs1, nsubs2, rc, o);
    return hipGetLastError();
}

}  // namespace fr
