// fr_dmx_reader.hip — `demux --gz-reader gpu`: a mate's BGZF file inflated on the GPU, window by window, into
// the buffer the demux indexes and routes from.
//
// The file is read in pieces of whole members (fr_dmx_reader_plan.h: whole_members) into one of two pinned
// buffers; while the GPU works on a piece -- and on everything the demux does with a window -- a host thread
// reads the next piece into the other buffer.  A piece goes to HBM compressed, and the members a window takes
// (plan_batch) decode with fr_inflate.hip's kernel, one wave each, straight to their place behind the carry:
// window + carry + the running decoded size.  A mate has two window buffers: the bytes after the last routed
// record (the carry) are copied from the old one to the front of the new one, so a carry of most of a window
// never overlaps itself, and the old window stays whole for whatever still reads it.  dmx_text_kernel then
// checks that the new bytes are 7-bit ASCII without '\r' -- text on which the reference's text-mode view is the
// raw bytes -- and the caller (fr_demux.hip) indexes the window in place.
//
// Anything else -- a header that is not plain BGZF, a member that does not decode to its trailer's size and
// CRC-32, a byte the text check flags, a read error -- hands the file over: the window keeps its carry only,
// and the host reader continues at the decoded offset `resume`, with its own error behaviour.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <future>
#include <string>
#include <vector>

#include "../../include/frender_amd.h"
#include "fr_dmx_reader_plan.h"
#include "fr_internal.h"

namespace fr {
namespace {

constexpr int TWG = 256;                 // lanes per workgroup
constexpr int TQ = 4;                    // 16-byte words per lane and step: 16 KiB per workgroup, dmx_count's tile
constexpr u64 CHUNK_DEFAULT = 32ull << 20;  // compressed bytes per piece: a launch's members should fill the inflater's grid
                                            // (4 waves per CU; at 8 MiB a level-1 piece held 235 members for 1024 slots)
constexpr u64 CHUNK_MAX = 256ull << 20;

// bit 7 of every byte of w that has bit 7 set or equals '\r'
__device__ __forceinline__ u32 text_bad4(u32 w) {
    const u32 t = w ^ 0x0D0D0D0Du;
    const u32 cr = ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) & 0x80808080u;  // exact zero bytes of t
    return (w & 0x80808080u) | cr;
}

// 0xFF in the bytes [lo, hi) of the dword whose first byte has index `at` in its 16-byte word
__device__ __forceinline__ u32 byte_range4(u32 at, u32 lo, u32 hi) {
    u32 m = 0;
#pragma unroll
    for (u32 j = 0; j < 4; ++j)
        if (at + j >= lo && at + j < hi) m |= 0xFFu << (8 * j);
    return m;
}

// *flag |= 1 when a byte of buf[a, b) has bit 7 set or is '\r'.  buf is 16-byte aligned and readable up to the
// 16-byte boundary at or after b: the loads cover the 16-byte hull of [a, b) and nothing else, the hull's bytes
// outside [a, b) are masked away (a larger earlier window leaves any bytes past b).  A streaming pass: 16-byte
// loads, adjacent lanes adjacent words, the lanes' findings ORed per wave (ballot) and per workgroup (LDS),
// at most one atomic per workgroup.
__global__ __launch_bounds__(TWG) void dmx_text_kernel(const u8* __restrict__ buf, u64 a, u64 b, u32* flag) {
    __shared__ u32 ws[TWG / 64];
    const u64 a0 = a & ~15ull;
    const u64 nwords = b > a ? (b - a0 + 15) >> 4 : 0;
    u32 bad = 0;
    for (u64 t = (u64)blockIdx.x * (TWG * TQ); t < nwords; t += (u64)gridDim.x * (TWG * TQ)) {
#pragma unroll
        for (int q = 0; q < TQ; ++q) {
            const u64 i = t + (u64)q * TWG + threadIdx.x;
            if (i >= nwords) continue;
            const u64 p = a0 + (i << 4);
            const uint4 v = *(const uint4*)(buf + p);
            u32 x = text_bad4(v.x), y = text_bad4(v.y), z = text_bad4(v.z), w = text_bad4(v.w);
            if (p < a || p + 16 > b) {  // the hull's first and last word
                const u32 lo = p < a ? (u32)(a - p) : 0u, hi = p + 16 > b ? (u32)(b - p) : 16u;
                x &= byte_range4(0, lo, hi);
                y &= byte_range4(4, lo, hi);
                z &= byte_range4(8, lo, hi);
                w &= byte_range4(12, lo, hi);
            }
            bad |= x | y | z | w;
        }
    }
    const u64 any = __ballot(bad != 0);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = any != 0;
    __syncthreads();
    if (threadIdx.x == 0 && (ws[0] | ws[1] | ws[2] | ws[3])) atomicOr(flag, 1u);
}

struct Piece {
    u8* h = nullptr;  // pinned
    u64 off = 0;      // file offset of h[0]: a member's first byte
    size_t n = 0, used = 0, count = 0;  // bytes read; bytes and number of its whole members
    bool bad = false, io_err = false;   // the bytes after `used` are not a member; the read failed
};

// bytes [off, off + n) of the file; false on an error or a short file
bool read_at(int fd, u8* dst, u64 off, size_t n) {
    size_t got = 0;
    while (got < n) {
        const ssize_t k = pread(fd, dst + got, n - got, (off_t)(off + got));
        if (k <= 0) return false;
        got += (size_t)k;
    }
    return true;
}

// the reader thread's job: the piece at file offset `off`, about `chunk` bytes, cut after its last whole member
void read_piece(int fd, u64 fsize, u64 off, u64 chunk, Piece* p) {
    p->off = off;
    p->n = p->used = p->count = 0;
    p->bad = p->io_err = false;
    size_t n = (size_t)std::min<u64>(chunk, fsize - off);
    if (!read_at(fd, p->h, off, n)) {
        p->io_err = true;
        return;
    }
    p->used = rdr::whole_members(p->h, n, off + n == fsize, &p->bad, &p->count);
    if (!p->count && !p->bad && off + n < fsize && n < rdr::MEMBER_MAX) {  // a piece smaller than its first member: up to one member more
        const size_t n2 = (size_t)std::min<u64>(rdr::MEMBER_MAX, fsize - off);
        if (!read_at(fd, p->h + n, off + n, n2 - n)) {
            p->io_err = true;
            return;
        }
        n = n2;
        p->used = rdr::whole_members(p->h, n, off + n == fsize, &p->bad, &p->count);
    }
    p->n = n;
}

struct Mate {
    bool open = false;
    int fd = -1;
    u64 fsize = 0, chunk = CHUNK_DEFAULT, hcap = 0;
    Piece pc[2];
    int cur = -1;  // the piece whose members are being decoded
    std::future<void> job;
    int job_slot = -1;  // the piece the reader thread fills (-1: none)
    std::vector<BgzfMember> ms;  // the current piece's members (offsets inside the piece)
    size_t mi = 0;               // the first one not decoded yet
    u8* d_in = nullptr;          // the current piece in HBM
    u64 c_d_in = 0;
    u8* win[2] = {nullptr, nullptr};
    u64 c_win[2] = {0, 0};
    int w = 0;                   // the window at hand
    u64 len = 0;
    u64 delivered = 0;           // decoded bytes of the file in the windows so far
    u64 fills = 0;               // fills of this file so far
    bool eof = false;
    // diagnostics, summed over the files of this mate
    double taken = 0, members = 0, batches = 0, handovers = 0, last_handover_fill = -1, infl_ms = 0, text_ms = 0,
           bytes = 0;
};

template <class T>
hipError_t grow(T** p, u64& cap, u64 n) {
    if (n <= cap && *p) return hipSuccess;
    if (*p) {
        hipError_t e = hipFree(*p);
        if (e != hipSuccess) return e;
        *p = nullptr;
    }
    cap = n + n / 4;
    return hipMalloc((void**)p, cap * sizeof(T));
}

}  // namespace

struct DmxReader {
    int device = 0;
    hipStream_t stream = nullptr;  // the demux's
    fr_infl* z = nullptr;
    u32* flag = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    Mate m[2];
    std::vector<u64> in_off, out_off;
    std::vector<u8> status;
    std::vector<u32> crc;
};

#define RK(x)                                                          \
    do {                                                               \
        hipError_t e_ = (x);                                           \
        if (e_ != hipSuccess) {                                        \
            err = std::string(#x) + ": " + hipGetErrorString(e_);      \
            return FR_ERR_HIP;                                         \
        }                                                              \
    } while (0)

static void stop_file(Mate& M) {
    if (M.job_slot >= 0 && M.job.valid()) M.job.wait();
    M.job_slot = -1;
    if (M.fd >= 0) close(M.fd);
    M.fd = -1;
    M.open = false;
    M.cur = -1;
    M.ms.clear();
    M.mi = 0;
}

static void start_job(Mate& M, int slot, u64 off) {
    Piece* p = &M.pc[slot];
    const int fd = M.fd;
    const u64 fsize = M.fsize, chunk = M.chunk;
    M.job = std::async(std::launch::async, [=]() { read_piece(fd, fsize, off, chunk, p); });
    M.job_slot = slot;
}

int dmx_reader_open(DmxReader** rp, int device, hipStream_t stream, int mate, const char* path, u64 chunk_bytes,
                    int* taken, std::string& err) {
    *taken = 0;
    RK(hipSetDevice(device));
    if (!*rp) {
        DmxReader* r = new DmxReader();
        r->device = device;
        r->stream = stream;
        *rp = r;
    }
    DmxReader* r = *rp;
    Mate& M = r->m[mate];
    if (M.open) return err = "fr_dmx_bgzf_open: the mate has a file open", FR_ERR_INVALID;
    const int fd = path ? open(path, O_RDONLY | O_CLOEXEC) : -1;
    if (fd < 0) return FR_OK;  // the host reader reports what is wrong with it
    struct stat sb;
    u8 head[18];
    bool bad = true;
    size_t count = 0;
    if (fstat(fd, &sb) != 0 || sb.st_size < 26 || !read_at(fd, head, 0, 18) ||
        (rdr::whole_members(head, 18, false, &bad, &count), bad)) {
        close(fd);
        return FR_OK;  // not a file whose first header is plain BGZF's
    }
    if (!r->z) {
        r->z = fr_infl_create(device);
        const char* e = fr_infl_last_error(r->z);
        if (e && *e) {
            err = std::string("fr_dmx_bgzf_open: ") + e;
            fr_infl_destroy(r->z);
            r->z = nullptr;
            close(fd);
            return FR_ERR_HIP;
        }
        RK(hipMalloc((void**)&r->flag, 4));
        RK(hipEventCreate(&r->e0));
        RK(hipEventCreate(&r->e1));
    }
    const u64 chunk = std::min<u64>(chunk_bytes ? chunk_bytes : CHUNK_DEFAULT, CHUNK_MAX);
    const u64 hcap = std::max<u64>(chunk, rdr::MEMBER_MAX);
    if (hcap > M.hcap) {
        for (Piece& p : M.pc) {
            if (p.h) (void)hipHostFree(p.h);
            p.h = nullptr;
        }
        M.hcap = 0;
        for (Piece& p : M.pc)
            if (hipHostMalloc((void**)&p.h, hcap, hipHostMallocDefault) != hipSuccess) {
                close(fd);
                return err = "fr_dmx_bgzf_open: pinned buffer", FR_ERR_HIP;
            }
        M.hcap = hcap;
    }
    M.fd = fd;
    M.fsize = (u64)sb.st_size;
    M.chunk = chunk;
    M.open = true;
    M.cur = -1;
    M.mi = 0;
    M.ms.clear();
    M.len = M.delivered = M.fills = 0;
    M.eof = false;
    M.taken += 1;
    start_job(M, 0, 0);  // the first piece is on its way while the caller opens the other mate
    *taken = 1;
    return FR_OK;
}

// the next piece becomes the current one: read (waited for), cut into members, uploaded; the one after it starts
// reading.  *ok = false: the file is handed over.  M.eof is set when no piece is left.
static int advance(DmxReader* r, Mate& M, bool* ok, std::string& err) {
    *ok = false;
    if (M.cur >= 0 && M.pc[M.cur].bad) return FR_OK;
    const u64 off = M.cur < 0 ? 0 : M.pc[M.cur].off + M.pc[M.cur].used;
    if (off >= M.fsize) {
        M.eof = true;
        *ok = true;
        return FR_OK;
    }
    if (M.job_slot < 0) start_job(M, M.cur < 0 ? 0 : M.cur ^ 1, off);
    M.job.wait();
    const int slot = M.job_slot;
    M.job_slot = -1;
    Piece& p = M.pc[slot];
    if (p.io_err || p.off != off || !p.count || !bgzf_member_table(p.h, p.used, M.ms) || M.ms.size() != p.count)
        return FR_OK;
    M.cur = slot;
    M.mi = 0;
    RK(grow(&M.d_in, M.c_d_in, (u64)p.used + 16));
    RK(hipMemcpyAsync(M.d_in, p.h, p.used, hipMemcpyHostToDevice, r->stream));
    RK(hipStreamSynchronize(r->stream));  // the inflater's stream reads it; the other pinned buffer is free
    if (!p.bad && p.off + p.used < M.fsize) start_job(M, slot ^ 1, p.off + p.used);
    *ok = true;
    return FR_OK;
}

int dmx_reader_fill(DmxReader* r, int mate, u64 keep_from, u64 want, const u8** win, u64* len, int* eof,
                    int* handed_over, u64* resume, std::string& err) {
    Mate& M = r->m[mate];
    if (!M.open) return err = "fr_dmx_bgzf_fill: no file is open for the mate", FR_ERR_INVALID;
    if (keep_from > M.len) return err = "fr_dmx_bgzf_fill: keep_from is beyond the window", FR_ERR_INVALID;
    RK(hipSetDevice(r->device));
    // Everything queued on the demux's stream that reads a window of this mate -- the validation, the route's
    // copies, the loader -- is complete before a byte of a window buffer changes (or the buffer is replaced).
    RK(hipStreamSynchronize(r->stream));
    const u64 carry = rdr::carry_len(M.len, keep_from);
    const int nw = M.w ^ 1;
    RK(grow(&M.win[nw], M.c_win[nw], rdr::window_capacity(carry, want)));
    u8* dst = M.win[nw];
    if (carry) RK(hipMemcpyAsync(dst, M.win[M.w] + keep_from, carry, hipMemcpyDeviceToDevice, r->stream));
    u64 have = carry, members = 0;
    double infl_ms = 0, text_ms = 0;
    bool ok = true;
    while (ok && have < want && !M.eof) {
        if (M.cur < 0 || M.mi == M.ms.size()) {
            if (int rc = advance(r, M, &ok, err)) return rc;
            if (!ok || M.eof) break;
        }
        const size_t left = M.ms.size() - M.mi;
        r->in_off.resize(2 * left);
        r->out_off.resize(left + 1);
        const size_t cnt = rdr::plan_batch(M.ms.data(), M.ms.size(), M.mi, have, want, r->in_off.data(), r->out_off.data());
        if (r->out_off[cnt] + rdr::SLACK > M.c_win[nw]) return err = "fr_dmx_bgzf_fill: a batch past the window's capacity", FR_ERR_DEVICE;
        r->status.resize(cnt);
        r->crc.resize(cnt);
        if (int rc = infl_run(r->z, M.d_in, r->in_off.data(), dst, r->out_off.data(), (int)cnt, r->status.data(),
                              r->crc.data(), 1))
            return err = std::string("fr_dmx_bgzf_fill: ") + fr_infl_last_error(r->z), rc;
        double ms = 0;
        if (fr_infl_kernel_info(r->z, nullptr, nullptr, &ms) == FR_OK) infl_ms += ms;
        for (size_t j = 0; j < cnt && ok; ++j)
            ok = r->status[j] == 0 && r->crc[j] == M.ms[M.mi + j].crc;
        M.mi += cnt;
        members += cnt;
        have = r->out_off[cnt];
    }
    if (ok && have > carry) {  // the new bytes are text whose text-mode view is the bytes themselves?
        u32 flag = 0;
        const u64 nwords = (have - (carry & ~15ull) + 15) >> 4;
        const u32 grid = (u32)std::max<u64>(1, std::min<u64>((nwords + TWG * TQ - 1) / (TWG * TQ), 2048));
        RK(hipMemsetAsync(r->flag, 0, 4, r->stream));
        RK(hipEventRecord(r->e0, r->stream));
        hipLaunchKernelGGL(dmx_text_kernel, dim3(grid), dim3(TWG), 0, r->stream, dst, carry, have, r->flag);
        RK(hipGetLastError());
        RK(hipEventRecord(r->e1, r->stream));
        RK(hipMemcpyAsync(&flag, r->flag, 4, hipMemcpyDeviceToHost, r->stream));
        RK(hipStreamSynchronize(r->stream));
        float ms = 0;
        RK(hipEventElapsedTime(&ms, r->e0, r->e1));
        text_ms = ms;
        ok = flag == 0;
    }
    RK(hipStreamSynchronize(r->stream));  // the carry is in place
    if (ok && M.cur >= 0 && M.mi == M.ms.size() && !M.pc[M.cur].bad && M.pc[M.cur].off + M.pc[M.cur].used >= M.fsize)
        M.eof = true;
    M.w = nw;
    M.infl_ms = infl_ms;
    M.text_ms = text_ms;
    *win = dst;
    *resume = M.delivered;
    if (!ok) {  // nothing of this batch is delivered: the window is its carry, the rest of the file the host's
        M.len = carry;
        M.handovers += 1;
        M.last_handover_fill = (double)M.fills;
        stop_file(M);
        *len = carry;
        *eof = 0;
        *handed_over = 1;
        return FR_OK;
    }
    M.len = have;
    M.delivered += have - carry;
    M.fills += 1;
    M.members += (double)members;
    M.batches += 1;
    M.bytes += (double)(have - carry);
    *len = have;
    *eof = M.eof ? 1 : 0;
    *handed_over = 0;
    *resume = M.delivered;
    return FR_OK;
}

bool dmx_reader_is_open(const DmxReader* r, int mate) { return r && r->m[mate].open; }

void dmx_reader_close(DmxReader* r, int mate) {
    if (r) stop_file(r->m[mate]);
}

void dmx_reader_destroy(DmxReader* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    for (Mate& M : r->m) {
        stop_file(M);
        for (Piece& p : M.pc)
            if (p.h) (void)hipHostFree(p.h);
        void* d[] = {M.d_in, M.win[0], M.win[1]};
        for (void* x : d)
            if (x) (void)hipFree(x);
    }
    if (r->flag) (void)hipFree(r->flag);
    if (r->e0) (void)hipEventDestroy(r->e0);
    if (r->e1) (void)hipEventDestroy(r->e1);
    if (r->z) fr_infl_destroy(r->z);
    delete r;
}

void dmx_reader_info(const DmxReader* r, int mate, double out[8]) {
    for (int k = 0; k < 8; ++k) out[k] = 0;
    out[4] = -1;
    if (!r) return;
    const Mate& M = r->m[mate];
    const double v[8] = {M.taken, M.members, M.batches, M.handovers, M.last_handover_fill, M.infl_ms, M.text_ms, M.bytes};
    for (int k = 0; k < 8; ++k) out[k] = v[k];
}

}  // namespace fr
