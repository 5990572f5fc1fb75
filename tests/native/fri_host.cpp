// Host build of the GPU inflate (frender_amd/csrc/fr_inflate_core.h): the kernel's decoder with the
// lanes of its wave as loops (fri::HostP).  tests/test_inflate_host.py checks its verdicts against zlib
// and runs the stand-alone program below (-DFRI_MAIN) over the whole corpus, corrupt streams included,
// under the address and undefined-behaviour sanitizers.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../frender_amd/csrc/fr_inflate_core.h"

extern "C" int fri_host_inflate(const uint8_t* in, uint64_t in_len, uint8_t* out, uint64_t out_len, uint64_t* produced) {
    if (in_len > fri::MAX_IN || out_len > fri::MAX_OUT) return fri::INFL_OVERRUN;
    static thread_local fri::Tables T;
    fri::HostP p{out};
    uint32_t n = 0;
    const uint8_t st = fri::inflate_stream(p, T, in, (uint32_t)in_len, (uint32_t)out_len, &n);
    if (produced) *produced = n;
    return st;
}

#ifdef FRI_MAIN
// corpus file: u32 count, then per stream u32 in_len, u32 out_len, in_len bytes.  Every stream is decoded
// from and into heap buffers of exactly in_len and out_len bytes, so the sanitizer sees any access past
// either.  Prints nothing; exit 0 when every stream returned a verdict.
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    uint64_t ok = 0;
    for (uint32_t s = 0; s < count; ++s) {
        uint32_t h[2];
        if (fread(h, 4, 2, f) != 2) return 2;
        if (h[0] > fri::MAX_IN || h[1] > fri::MAX_OUT) return 2;
        std::vector<uint8_t> in(h[0]), out(h[1]);
        if (h[0] && fread(in.data(), 1, h[0], f) != h[0]) return 2;
        uint64_t produced = 0;
        const int st = fri_host_inflate(in.data(), in.size(), out.data(), out.size(), &produced);
        if (produced > out.size()) return 3;
        ok += st == 0;
    }
    fclose(f);
    return ok <= count ? 0 : 3;
}
#endif
