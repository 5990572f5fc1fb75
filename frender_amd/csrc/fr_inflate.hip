// fr_inflate.hip — inflate on the GPU: the decoder of fr_inflate_core.h, one wave per raw deflate stream
// of at most 64 KiB decoded (a BGZF member), and the C-ABI context around it (fr_infl_*); fr_feed_bgzf
// (fr_api.hip) decodes a whole BGZF file with it, straight into HBM.
//
// Serial Huffman decoding is latency-bound -- every symbol is a dependent table lookup -- so the rate
// comes from the members in flight, not from one member's speed.  A workgroup is one wave; waves take
// members by ticket, in file order.  The decode state is uniform over the wave (every lane runs the same
// scalar code: table lookups are same-address LDS reads), lane 0 writes shared state, and the lanes
// share the parallel parts: table fills, match copies (lane i copies byte i of a 64-byte step, i % dist
// for overlapping matches), stored blocks.  Per wave in LDS, 39,072 B in all, so four waves per CU: the
// 32-KiB back-reference window as a ring, the code tables (~4 KiB), 1 KiB of staged input, the 1-KiB
// CRC table and the lanes' CRC slices.  Every produced byte goes to the ring and to its final place in
// HBM; back-references read the ring only (LDS accesses of one wave are ordered, the same hand-off
// through global memory would need a fence per match).  After a member decoded, one fence, then
// its CRC-32: 64 lanes over 1 KiB each of the output, folded by the 1-KiB shift operator.
// Memory safety for any input bytes is the core's contract (fr_inflate_core.h); the kernel adds none of
// its own accesses except the platform's, which write out[pos .. pos + n) under the core's bounds.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/frender_amd.h"
#include "fr_inflate_core.h"
#include "fr_internal.h"

static_assert(FR_INFL_BTYPE == fri::INFL_BTYPE && FR_INFL_STORED == fri::INFL_STORED &&
                  FR_INFL_CODELEN == fri::INFL_CODELEN && FR_INFL_SYMBOL == fri::INFL_SYMBOL &&
                  FR_INFL_DIST == fri::INFL_DIST && FR_INFL_INPUT == fri::INFL_INPUT &&
                  FR_INFL_OVERRUN == fri::INFL_OVERRUN && FR_INFL_SHORT == fri::INFL_SHORT,
              "the header's reason codes are the core's");

namespace {

constexpr uint32_t WIN = 32768;  // the deflate window, the ring's size
constexpr uint32_t SUB = 1024;   // CRC slice of one lane
constexpr uint32_t STG = 1024;   // input bytes staged in LDS at a time

struct InflShared {
    uint8_t ring[WIN];
    fri::Tables T;
    alignas(16) uint8_t stg[STG];
    uint32_t crc_tab[256];
    uint32_t lane_v[64];
};
static_assert(sizeof(InflShared) <= 40 * 1024, "four waves per CU (160 KiB of LDS)");

// the core's platform on one wave: positions are below 65536, out holds the stream's out_len bytes
struct WaveP {
    uint8_t* ring;
    uint8_t* out;
    uint32_t lane;
    uint8_t* stg;
    // the stream's bytes [at, at + STG) into LDS, zeros from in_len on: the only reads of the compressed bytes
    // besides a stored block's copy, each checked against in_len
    __device__ const uint8_t* stage(const uint8_t* in, uint32_t in_len, uint32_t at, uint32_t* end) const {
        sync();
        for (uint32_t k = lane; k < STG; k += 64) stg[k] = at + k < in_len ? in[at + k] : (uint8_t)0;
        sync();
        *end = at + STG;
        return stg;
    }
    __device__ bool lane0() const { return lane == 0; }
    template <class F>
    __device__ void for_lanes(uint32_t n, F f) const {
        for (uint32_t i = lane; i < n; i += 64) f(i);
    }
    // LDS accesses of one wave execute in order; this keeps the compiler from moving them across
    __device__ void sync() const {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __device__ void put(uint32_t pos, uint8_t b) const {
        if (lane == 0) {
            ring[pos & (WIN - 1)] = b;
            out[pos] = b;
        }
        sync();
    }
    __device__ void copy_match(uint32_t pos, uint32_t d, uint32_t n) const {
        const uint32_t m = d >= 64 ? lane : lane % d;
        for (uint32_t base = 0; base < n; base += 64) {
            const bool on = base + lane < n;
            uint8_t b = 0;
            if (on) b = ring[(pos + base - d + m) & (WIN - 1)];
            sync();  // every lane has read before any lane writes
            if (on) {
                ring[(pos + base + lane) & (WIN - 1)] = b;
                out[pos + base + lane] = b;
            }
            sync();
        }
    }
    __device__ void copy_in(uint32_t pos, const uint8_t* src, uint32_t n) const {
        for (uint32_t i = lane; i < n; i += 64) {
            const uint8_t b = src[i];
            ring[(pos + i) & (WIN - 1)] = b;
            out[pos + i] = b;
        }
        sync();
    }
};

__global__ __launch_bounds__(64) void inflate_members(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                      uint8_t* out, const uint64_t* __restrict__ out_off,
                                                      uint32_t n_streams, uint32_t pairs, uint8_t* __restrict__ status,
                                                      uint32_t* __restrict__ crc_out, uint32_t* ticket,
                                                      const uint32_t* __restrict__ crc_shift) {
    __shared__ InflShared S;
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = lane; i < 256; i += 64) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        S.crc_tab[i] = c;
    }
    for (;;) {
        uint32_t s = 0;
        if (lane == 0) s = atomicAdd(ticket, 1u);
        s = __shfl(s, 0);
        if (s >= n_streams) break;
        // pairs: stream s is [in_off[2s], in_off[2s + 1]) (a BGZF file's members), else [in_off[s], in_off[s + 1])
        const uint64_t a = in_off[(uint64_t)s << pairs], oa = out_off[s];
        const uint32_t in_len = (uint32_t)(in_off[((uint64_t)s << pairs) + 1] - a), out_len = (uint32_t)(out_off[s + 1] - oa);  // host-checked
        uint8_t* o = out + oa;
        WaveP p{S.ring, o, lane, S.stg};
        uint32_t produced = 0;
        const uint8_t st = fri::inflate_stream(p, S.T, in + a, in_len, out_len, &produced);
        uint32_t crc = 0;
        if (st == fri::INFL_OK && out_len) {
            __threadfence();  // the lanes read bytes that other lanes stored
            const uint32_t nsub = (out_len + SUB - 1) / SUB;  // <= 64
            if (lane < nsub) {
                const uint32_t b0 = lane * SUB, b1 = min(out_len, b0 + SUB);
                uint32_t c = 0xFFFFFFFFu;
                for (uint32_t i = b0; i < b1; ++i) c = S.crc_tab[(c ^ o[i]) & 255] ^ (c >> 8);
                S.lane_v[lane] = ~c;
            }
            p.sync();
            if (lane == 0) {
                for (uint32_t k = 0; k < nsub; ++k) {
                    const uint32_t sl = min(SUB, out_len - k * SUB);
                    if (sl == SUB) {
                        crc = crc_shift[crc & 255] ^ crc_shift[256 + ((crc >> 8) & 255)] ^
                              crc_shift[512 + ((crc >> 16) & 255)] ^ crc_shift[768 + (crc >> 24)];
                    } else {
                        for (uint32_t q = 0; q < sl; ++q) crc = S.crc_tab[crc & 255] ^ (crc >> 8);
                    }
                    crc ^= S.lane_v[k];
                }
            }
        }
        if (lane == 0) {
            status[s] = st;
            crc_out[s] = crc;
        }
        p.sync();
    }
}

}  // namespace

struct fr_infl {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    int grid = 0;
    uint32_t *shift = nullptr, *ticket = nullptr, *crc = nullptr;
    uint64_t *in_off = nullptr, *out_off = nullptr;
    uint8_t *status = nullptr, *in = nullptr, *out = nullptr;
    uint8_t* h_in = nullptr;  // pinned: a BGZF file's bytes on their way to the device
    uint64_t c_crc = 0, c_in_off = 0, c_out_off = 0, c_status = 0, c_in = 0, c_out = 0, c_h_in = 0;
    uint64_t out_len = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;  // around the last run's kernel (fr_infl_kernel_info)
    bool timed = false;
    std::vector<fr::BgzfMember> ms;
    std::vector<uint64_t> h_in_off, h_out_off;
    std::vector<uint8_t> h_status;
    std::vector<uint32_t> h_crc;
};

#define IF(x)                                                        \
    do {                                                             \
        hipError_t e_ = (x);                                         \
        if (e_ != hipSuccess) {                                      \
            z->err = std::string(#x) + ": " + hipGetErrorString(e_); \
            return FR_ERR_HIP;                                       \
        }                                                            \
    } while (0)

// grow-only device buffers: they serve the next file (a free per file synchronises the device)
template <class T>
static hipError_t grow(T** p, uint64_t& cap, uint64_t n) {
    if (n <= cap && *p) return hipSuccess;
    if (*p) {
        hipError_t e = hipFree(*p);
        if (e != hipSuccess) return e;
        *p = nullptr;
    }
    cap = std::max<uint64_t>(n + n / 4, 1024);
    return hipMalloc((void**)p, cap * sizeof(T));
}

static int run_device(fr_infl* z, const uint8_t* dev_in, const uint64_t* in_off, uint8_t* dev_out,
                      const uint64_t* out_off, int n, uint8_t* status, uint32_t* crc32, int pairs = 0) {
    if (!z || !z->shift) return FR_ERR_HIP;
    if (n < 0 || (n && (!in_off || !out_off || !status || !crc32)))
        return z->err = "fr_infl_run: bad stream list", FR_ERR_INVALID;
    for (int s = 0; s < n; ++s) {
        const uint64_t a = in_off[(size_t)s << pairs], b = in_off[((size_t)s << pairs) + 1];
        if (b < a || out_off[s + 1] < out_off[s])
            return z->err = "fr_infl_run: offsets must not decrease", FR_ERR_INVALID;
        if (out_off[s + 1] - out_off[s] > fri::MAX_OUT || b - a > fri::MAX_IN)
            return z->err = "fr_infl_run: a stream decodes to at most 65536 bytes", FR_ERR_INVALID;
    }
    if (!n) return FR_OK;
    IF(hipSetDevice(z->device));
    const uint64_t n_in = pairs ? 2 * (uint64_t)n : (uint64_t)n + 1;
    IF(grow(&z->in_off, z->c_in_off, n_in));
    IF(grow(&z->out_off, z->c_out_off, (uint64_t)n + 1));
    IF(grow(&z->status, z->c_status, (uint64_t)n));
    IF(grow(&z->crc, z->c_crc, (uint64_t)n));
    IF(hipMemcpyAsync(z->in_off, in_off, n_in * 8, hipMemcpyHostToDevice, z->stream));
    IF(hipMemcpyAsync(z->out_off, out_off, ((uint64_t)n + 1) * 8, hipMemcpyHostToDevice, z->stream));
    IF(hipMemsetAsync(z->ticket, 0, 4, z->stream));
    const uint32_t g = (uint32_t)std::min<int64_t>(n, z->grid);
    IF(hipEventRecord(z->e0, z->stream));
    hipLaunchKernelGGL(inflate_members, dim3(g), dim3(64), 0, z->stream, dev_in, z->in_off, dev_out, z->out_off,
                       (uint32_t)n, (uint32_t)pairs, z->status, z->crc, z->ticket, z->shift);
    IF(hipGetLastError());
    IF(hipEventRecord(z->e1, z->stream));
    z->timed = true;
    IF(hipMemcpyAsync(status, z->status, (uint64_t)n, hipMemcpyDeviceToHost, z->stream));
    IF(hipMemcpyAsync(crc32, z->crc, (uint64_t)n * 4, hipMemcpyDeviceToHost, z->stream));
    IF(hipStreamSynchronize(z->stream));
    return FR_OK;
}

namespace fr {

// run_device for the other readers of this library (fr_dmx_reader.hip): fr_infl_run with the choice of `pairs`
int infl_run(fr_infl* z, const uint8_t* dev_in, const uint64_t* in_off, uint8_t* dev_out, const uint64_t* out_off, int n,
             uint8_t* status, uint32_t* crc32, int pairs) {
    return run_device(z, dev_in, in_off, dev_out, out_off, n, status, crc32, pairs);
}

// A whole BGZF file through the context: *ok = 1 with the decoded bytes on the device (16-byte aligned,
// 16 zero bytes past the end, valid until the context's next run) when every member decoded to its
// trailer's size and CRC-32; *ok = 0 when the file is not one the GPU reader takes or a member failed.
int infl_bgzf_file(fr_infl* z, const char* path, int* ok, const uint8_t** dev_out, uint64_t* out_len, uint64_t* members) {
    *ok = 0;
    if (!z || !z->shift) return FR_ERR_HIP;
    FILE* fp = fopen(path, "rb");
    if (!fp) return FR_OK;  // the host pool reports what is wrong with it
    uint64_t size = 0;
    if (fseek(fp, 0, SEEK_END) == 0) {
        const long t = ftell(fp);
        size = t > 0 ? (uint64_t)t : 0;
    }
    rewind(fp);
    if (!size || size > BGZF_MAX_IN) {
        fclose(fp);
        return FR_OK;
    }
    if (hipSetDevice(z->device) != hipSuccess) {
        fclose(fp);
        return z->err = "hipSetDevice failed", FR_ERR_HIP;
    }
    if (size > z->c_h_in) {
        if (z->h_in) (void)hipHostFree(z->h_in);
        z->h_in = nullptr;
        z->c_h_in = 0;
        if (hipHostMalloc((void**)&z->h_in, size + size / 4, hipHostMallocDefault) != hipSuccess) {
            fclose(fp);
            return z->err = "fr_feed_bgzf: pinned buffer", FR_ERR_HIP;
        }
        z->c_h_in = size + size / 4;
    }
    const bool read_ok = fread(z->h_in, 1, size, fp) == size;
    fclose(fp);
    if (!read_ok || !bgzf_member_table(z->h_in, size, z->ms)) return FR_OK;
    const size_t n = z->ms.size();
    if (n > 0x7FFFFFFFull) return FR_OK;
    // the file goes up in one copy; stream s is [in_off[2s], in_off[2s + 1]) of it (headers and trailers between)
    z->h_in_off.resize(2 * n);
    z->h_out_off.resize(n + 1);
    for (size_t s = 0; s < n; ++s) {
        const BgzfMember& m = z->ms[s];
        z->h_in_off[2 * s] = m.in_off;
        z->h_in_off[2 * s + 1] = m.in_off + m.in_len;
        z->h_out_off[s] = m.dst;
    }
    const uint64_t total = z->ms.back().dst + z->ms.back().isize;
    // a file whose buffers the device cannot hold is declined: the host pool decodes it in windows
    if (grow(&z->in, z->c_in, size + 16) != hipSuccess || grow(&z->out, z->c_out, total + 16) != hipSuccess) {
        (void)hipGetLastError();
        return FR_OK;
    }
    IF(hipMemcpyAsync(z->in, z->h_in, size, hipMemcpyHostToDevice, z->stream));
    z->h_out_off[n] = total;
    IF(hipMemsetAsync(z->out + total, 0, 16, z->stream));
    z->h_status.resize(n);
    z->h_crc.resize(n);
    z->out_len = 0;
    const int rc = run_device(z, z->in, z->h_in_off.data(), z->out, z->h_out_off.data(), (int)n, z->h_status.data(),
                              z->h_crc.data(), 1);
    if (rc) return rc;
    for (size_t s = 0; s < n; ++s)
        if (z->h_status[s] != 0 || z->h_crc[s] != z->ms[s].crc) return FR_OK;
    z->out_len = total;
    *ok = 1;
    *dev_out = z->out;
    *out_len = total;
    *members = n;
    return FR_OK;
}

}  // namespace fr

extern "C" {

fr_infl* fr_infl_create(int device) {
    fr_infl* z = new fr_infl();
    z->device = device;
    auto fail = [&](const char* m) {
        z->err = m;
        return z;
    };
    if (hipSetDevice(device) != hipSuccess) return fail("fr_infl_create: no usable HIP device");
    if (hipStreamCreateWithFlags(&z->stream, hipStreamNonBlocking) != hipSuccess) return fail("fr_infl_create: stream");
    if (hipEventCreate(&z->e0) != hipSuccess || hipEventCreate(&z->e1) != hipSuccess) return fail("fr_infl_create: events");
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
    z->grid = 4 * cus;  // the waves the LDS admits: every workgroup resident, members by ticket
    std::vector<uint32_t> t1k(1024);
    fr::crc_shift_table(SUB, t1k.data());
    if (hipMalloc(&z->shift, 4096) != hipSuccess ||
        hipMemcpy(z->shift, t1k.data(), 4096, hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc(&z->ticket, 4) != hipSuccess) {
        if (z->shift) (void)hipFree(z->shift);
        z->shift = nullptr;
        return fail("fr_infl_create: device allocation");
    }
    return z;
}

void fr_infl_destroy(fr_infl* z) {
    if (!z) return;
    (void)hipSetDevice(z->device);
    if (z->stream) (void)hipStreamSynchronize(z->stream);
    void* p[] = {z->shift, z->ticket, z->crc, z->in_off, z->out_off, z->status, z->in, z->out};
    for (void* x : p)
        if (x) (void)hipFree(x);
    if (z->h_in) (void)hipHostFree(z->h_in);
    if (z->e0) (void)hipEventDestroy(z->e0);
    if (z->e1) (void)hipEventDestroy(z->e1);
    if (z->stream) (void)hipStreamDestroy(z->stream);
    delete z;
}

const char* fr_infl_last_error(const fr_infl* z) { return z ? z->err.c_str() : "null context"; }

int fr_infl_run(fr_infl* z, const uint8_t* dev_in, const uint64_t* in_off, uint8_t* dev_out, const uint64_t* out_off,
                int n_streams, uint8_t* status, uint32_t* crc32) {
    return run_device(z, dev_in, in_off, dev_out, out_off, n_streams, status, crc32);
}

int fr_infl_run_host(fr_infl* z, const uint8_t* data, const uint64_t* in_off, const uint64_t* out_off, int n_streams,
                     uint8_t* status, uint32_t* crc32) {
    if (!z || !z->shift) return FR_ERR_HIP;
    if (n_streams < 0 || (n_streams && (!in_off || !out_off))) return z->err = "fr_infl_run_host: bad stream list", FR_ERR_INVALID;
    z->out_len = 0;
    if (!n_streams) return FR_OK;
    const uint64_t a = in_off[0], b = in_off[n_streams], total = out_off[n_streams];
    if (b < a) return z->err = "fr_infl_run_host: offsets must not decrease", FR_ERR_INVALID;
    IF(hipSetDevice(z->device));
    IF(grow(&z->in, z->c_in, b + 16));
    IF(grow(&z->out, z->c_out, total + 16));
    if (b > a) IF(hipMemcpyAsync(z->in + a, data + a, b - a, hipMemcpyHostToDevice, z->stream));
    IF(hipMemsetAsync(z->out, 0, total + 16, z->stream));
    const int rc = run_device(z, z->in, in_off, z->out, out_off, n_streams, status, crc32);
    if (rc == FR_OK) z->out_len = total;
    return rc;
}

int fr_infl_kernel_info(fr_infl* z, int* vgprs, int* lds_bytes, double* last_ms) {
    if (!z || !z->shift) return FR_ERR_HIP;
    IF(hipSetDevice(z->device));
    hipFuncAttributes at{};
    IF(hipFuncGetAttributes(&at, (const void*)inflate_members));
    if (vgprs) *vgprs = at.numRegs;
    if (lds_bytes) *lds_bytes = (int)at.sharedSizeBytes;
    if (last_ms) {
        float ms = 0;
        if (z->timed) IF(hipEventElapsedTime(&ms, z->e0, z->e1));  // the run synchronised its stream
        *last_ms = ms;
    }
    return FR_OK;
}

int fr_infl_fetch(fr_infl* z, uint8_t* out, uint64_t len) {
    if (!z || !z->shift) return FR_ERR_HIP;
    if (len > z->out_len) return z->err = "fr_infl_fetch: more bytes than the last run produced", FR_ERR_INVALID;
    IF(hipSetDevice(z->device));
    if (len) IF(hipMemcpy(out, z->out, len, hipMemcpyDeviceToHost));
    return FR_OK;
}

}  // extern "C"
