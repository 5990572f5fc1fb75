// fr_dmx_validate.hip — `demux --validate`: every record pair of a window is checked before it is routed, over the
// unrouted bytes while they are resident in HBM (src[0], src[1]) and the record starts the loader left (rs[0], rs[1],
// each with its sentinel).
//
// dmx_validate_kernel gives every wave one pair at a time, grid-strided.  Per mate the wave's 64 lanes load the
// record's first 1-KiB step in aligned 16-byte loads (lines::load16) and find its (at most four) '\n' with
// lines::newlines_1step, straight-line code, when the record lies in that step, with lines::newlines, the
// wave-uniform walk, when it is longer.  The positions are wave-uniform scalars, and so is everything that follows:
//   kinds 1-4 (R1), 5-8 (R2)  the count of '\n', two byte tests ('@', '+': read out of the step's registers with
//           readlane, no second load) and one subtraction (sequence against quality length);
//   kind 9  the name tokens: the header line's first space or tab and its last ':' come from per-lane SWAR masks and
//           a ballot, one pass over the header line's steps (one step for every usual header); a trailing /1 or /2 is
//           dropped; the two tokens, which sit at unrelated offsets mod 16, are compared with lane-per-byte loads (the
//           lines are in L2, just loaded), 64 bytes per round, as many rounds as the token is long;
//   kind 10 the codes, the text after the last ':' (the whole line without one), compared the same way.
// The first kind that applies is the pair's.  A wave that finds one does one 64-bit atomicMin of (pair << 8) | kind
// on the result word, which dmx_validate_window has reset to all-ones on the same stream; a clean window does no
// atomics and no stores.  No LDS, no scratch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/frender_amd.h"
#include "fr_dmx_lines.h"
#include "fr_internal.h"

namespace fr {
namespace {

constexpr int VWG = 256;  // lanes per workgroup
constexpr int VWAVES = VWG / 64;
constexpr int VGRID = 2048;  // workgroups at the most: 8 per CU, 32 waves per CU in flight
using namespace lines;  // STEP, load16, span_mask, eq_mask16, either_mask16, newlines_1step, newlines (fr_dmx_lines.h)

struct Rec {            // one mate's record: wave-uniform but v0
    u64 o, e;           // its bytes [o, e) of the mate's buffer
    u32 nnl;            // its '\n', at most 4
    u64 n0, n1, n2, n3; // their positions in the buffer (an entry at or past nnl is not to be used)
    uint4 v0;           // the lane's 16 bytes of the record's first step
};

__device__ __forceinline__ void parse(const u8* buf, u64 o, u64 e, int lane, Rec& r) {
    const u64 a0 = o & ~15ull;
    r.o = o;
    r.e = e;
    r.v0 = load16(buf, a0, e, lane);
    if (e - a0 <= STEP) {
        u32 p[4];
        r.nnl = newlines_1step((u32)(o - a0), (u32)(e - a0), r.v0, lane, p);
        r.n0 = a0 + p[0], r.n1 = a0 + p[1], r.n2 = a0 + p[2], r.n3 = a0 + p[3];
    } else {
        u64 p0, p1, p2, p3;
        r.nnl = newlines(buf, o, e - o, r.v0, lane, p0, p1, p2, p3);
        r.n0 = o + p0, r.n1 = o + p1, r.n2 = o + p2, r.n3 = o + p3;
    }
}

// the byte at pos of the record (o <= pos < e), wave-uniform: out of the first step's registers, or loaded
__device__ __forceinline__ u32 byte_at(const u8* buf, const Rec& r, u64 pos) {
    const u64 rel = pos - (r.o & ~15ull);
    u32 word;
    if (rel < STEP) {
        const u32 ln = (u32)rel >> 4, q = ((u32)rel >> 2) & 3u;
        const u32 x = __builtin_amdgcn_readlane(r.v0.x, ln), y = __builtin_amdgcn_readlane(r.v0.y, ln),
                  z = __builtin_amdgcn_readlane(r.v0.z, ln), w = __builtin_amdgcn_readlane(r.v0.w, ln);
        word = (q == 0 ? x : q == 1 ? y : q == 2 ? z : w) >> (8u * ((u32)rel & 3u));
    } else {
        word = __builtin_amdgcn_readfirstlane((u32)buf[pos]);
    }
    return word & 0xFFu;
}

// kinds 1-4 of one record, 0 for none
__device__ __forceinline__ u32 record_kind(const u8* buf, const Rec& r) {
    if (r.nnl < 3) return FR_DMX_V_TRUNCATED;
    if (byte_at(buf, r, r.o) != (u32)'@') return FR_DMX_V_HEADER;
    if (r.n2 == r.n1 + 1 || byte_at(buf, r, r.n1 + 1) != (u32)'+') return FR_DMX_V_SEPARATOR;
    const u64 seq = r.n1 - r.n0 - 1, qual = (r.nnl >= 4 ? r.n3 : r.e) - r.n2 - 1;
    return seq != qual ? FR_DMX_V_LENGTH : 0u;
}

// the header line [o, n0) of a record that passed kinds 1-4: name_end, its first space or tab (n0 without one), and
// code_start, the byte after its last ':' (o without one)
__device__ __forceinline__ void scan_header(const u8* buf, const Rec& r, int lane, u64& name_end, u64& code_start) {
    const u64 a0 = r.o & ~15ull;
    u64 sp = r.n0, cs = r.o;
    bool found = false;
    for (u64 a = a0; a < r.n0; a += STEP) {
        const uint4 v = a == a0 ? r.v0 : load16(buf, a, r.n0, lane);
        const u32 span = span_mask(a + (u64)lane * 16, r.o, r.n0);
        const u32 ms = either_mask16(v, 0x20202020u, 0x09090909u) & span;
        const u32 mc = eq_mask16(v, 0x3A3A3A3Au) & span;
        const u64 bs = __ballot(ms != 0), bc = __ballot(mc != 0);
        if (!found && bs) {
            const u32 ln = (u32)__builtin_ctzll(bs);
            sp = a + (u64)ln * 16 + (u32)__builtin_ctz(__builtin_amdgcn_readlane(ms, ln));
            found = true;
        }
        if (bc) {
            const u32 ln = 63u - (u32)__builtin_clzll(bc);
            cs = a + (u64)ln * 16 + (32u - (u32)__builtin_clz(__builtin_amdgcn_readlane(mc, ln)));
        }
    }
    name_end = sp;
    code_start = cs;
}

// bytes [s1, s1 + len) of b1 against [s2, s2 + len) of b2, a byte per lane and 64 per round
__device__ __forceinline__ bool same_bytes(const u8* b1, u64 s1, const u8* b2, u64 s2, u64 len, int lane) {
    for (u64 base = 0; base < len; base += 64) {
        const u64 i = base + (u64)lane;
        const bool d = i < len && b1[s1 + i] != b2[s2 + i];
        if (__ballot(d)) return false;
    }
    return true;
}

// the end of the name token [s, t): without its last two bytes when they are /1 or /2
__device__ __forceinline__ u64 strip_mate(const u8* buf, const Rec& r, u64 s, u64 t) {
    if (t - s < 2 || byte_at(buf, r, t - 2) != (u32)'/') return t;
    const u32 c = byte_at(buf, r, t - 1);
    return c == (u32)'1' || c == (u32)'2' ? t - 2 : t;
}

// grid-strided, one wave per pair: pair k is record k of rs1 (bytes of b1) with record k of rs2 (bytes of b2).
// PAIRED = false (a single-end window, fr_dmx_set_mates(1)): record k of rs1 alone, kinds 1-4; b2 and rs2 are null
// and never read
template <bool PAIRED>
__global__ __launch_bounds__(VWG) void dmx_validate_kernel(const u8* __restrict__ b1, const u8* __restrict__ b2,
                                                           const u64* __restrict__ rs1, const u64* __restrict__ rs2,
                                                           u64 n, unsigned long long* res) {
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u64 nw = (u64)gridDim.x * VWAVES;
    for (u64 k = (u64)blockIdx.x * VWAVES + (u64)wid; k < n; k += nw) {
        Rec A;
        parse(b1, rs1[k], rs1[k + 1], lane, A);
        u32 kind;
        if constexpr (PAIRED) {
            Rec B;
            parse(b2, rs2[k], rs2[k + 1], lane, B);
            kind = record_kind(b1, A);
            if (!kind) {
                kind = record_kind(b2, B);
                if (kind) kind += 4;
            }
            if (!kind) {
                u64 t1, c1, t2, c2;
                scan_header(b1, A, lane, t1, c1);
                scan_header(b2, B, lane, t2, c2);
                const u64 s1 = A.o + 1, s2 = B.o + 1;  // after the '@'
                t1 = strip_mate(b1, A, s1, t1);
                t2 = strip_mate(b2, B, s2, t2);
                if (t1 - s1 != t2 - s2 || !same_bytes(b1, s1, b2, s2, t1 - s1, lane))
                    kind = FR_DMX_V_NAME;
                else if (A.n0 - c1 != B.n0 - c2 || !same_bytes(b1, c1, b2, c2, A.n0 - c1, lane))
                    kind = FR_DMX_V_CODE;
            }
        } else {
            kind = record_kind(b1, A);
        }
        if (kind && lane == 0) atomicMin(res, (unsigned long long)((k << 8) | kind));
    }
}

}  // namespace

struct DmxValidate {
    int device = 0;
    hipStream_t stream = nullptr;
    unsigned long long* word = nullptr;  // (first violating pair << 8) | kind, all-ones for none
};

#define VK(x)                                                                  \
    do {                                                                       \
        hipError_t e_ = (x);                                                   \
        if (e_ != hipSuccess) {                                                \
            err = std::string(#x) + ": " + hipGetErrorString(e_);              \
            return FR_ERR_HIP;                                                 \
        }                                                                      \
    } while (0)

void dmx_validate_destroy(DmxValidate* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    if (t->word) (void)hipFree(t->word);
    delete t;
}

int dmx_validate_begin(DmxValidate** out, int device, hipStream_t stream, std::string& err) {
    if (*out) return FR_OK;
    DmxValidate* t = *out = new DmxValidate();  // (freed by the owner's destroy if the step below fails)
    t->device = device;
    t->stream = stream;
    VK(hipMalloc((void**)&t->word, sizeof(unsigned long long)));
    return FR_OK;
}

int dmx_validate_window(DmxValidate* t, const u8* b1, const u8* b2, const u64* rs1, const u64* rs2, u64 n,
                        std::string& err) {
    VK(hipMemsetAsync(t->word, 0xFF, sizeof(unsigned long long), t->stream));
    if (!n) return FR_OK;
    const u64 gx = std::min<u64>((n + VWAVES - 1) / VWAVES, (u64)VGRID);
    if (b2)
        hipLaunchKernelGGL(dmx_validate_kernel<true>, dim3((unsigned)gx), dim3(VWG), 0, t->stream, b1, b2, rs1, rs2, n,
                           t->word);
    else
        hipLaunchKernelGGL(dmx_validate_kernel<false>, dim3((unsigned)gx), dim3(VWG), 0, t->stream, b1, b2, rs1, rs2, n,
                           t->word);
    VK(hipGetLastError());
    return FR_OK;
}

int dmx_validate_result(DmxValidate* t, int64_t* first_pair, int32_t* kind, std::string& err) {
    unsigned long long w = ~0ull;
    VK(hipStreamSynchronize(t->stream));
    VK(hipMemcpy(&w, t->word, sizeof(w), hipMemcpyDeviceToHost));
    *first_pair = w == ~0ull ? -1 : (int64_t)(w >> 8);
    *kind = w == ~0ull ? 0 : (int32_t)(w & 0xFFu);
    return FR_OK;
}

}  // namespace fr
