// frp_host.cpp — the GPU reader's HIP-free arithmetic (frender_amd/csrc/fr_dmx_reader_plan.h) as a stand-alone
// program for the sanitizers (tests/test_demux_reader_host.py): a reader's fills are replayed on the host over
// member tables, every batch's offsets written through into exact-size heap buffers.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -o frp_main tests/native/frp_host.cpp && ./frp_main
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../frender_amd/csrc/fr_dmx_reader_plan.h"

using namespace fr::rdr;

struct M {
    size_t in_off, in_len;
    uint32_t isize;
};

static int fails = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                                     \
        }                                                                \
    } while (0)

// a file of members with the given decoded sizes, as a piece: headers as bgzip writes them, payload bytes of any
// value (the walk reads headers only)
static std::vector<uint8_t> file_of(const std::vector<uint32_t>& isize, std::vector<M>* ms) {
    std::vector<uint8_t> f;
    for (uint32_t n : isize) {
        const size_t body = 2 + n / 7, size = 18 + body + 8, pos = f.size();
        const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        f.insert(f.end(), head, head + 16);
        f.push_back((uint8_t)((size - 1) & 255));
        f.push_back((uint8_t)((size - 1) >> 8));
        f.insert(f.end(), body, (uint8_t)0xA5);
        for (int k = 0; k < 4; ++k) f.push_back(0);
        for (int k = 0; k < 4; ++k) f.push_back((uint8_t)(n >> (8 * k)));
        ms->push_back(M{pos + 18, body, n});
    }
    return f;
}

// every fill of a reader over the table: the window's bytes are counted per member, the carry is `keep` of a window
static void replay(const std::vector<uint32_t>& isize, uint64_t want, uint64_t keep_num, uint64_t keep_den) {
    std::vector<M> ms;
    const std::vector<uint8_t> f = file_of(isize, &ms);
    // the walk: every cut of the file finds whole members only, and a cut inside a member is not an error
    for (size_t n = 0; n <= f.size(); n += (n < 64 ? 1 : 37)) {
        std::vector<uint8_t> piece(f.begin(), f.begin() + n);  // exact size: a read past n is the sanitizer's
        bool bad = true;
        size_t count = 0;
        const size_t used = whole_members(piece.data(), n, false, &bad, &count);
        CHECK(!bad && used <= n && count <= ms.size());
        CHECK(used == (count ? ms[count - 1].in_off + ms[count - 1].in_len + 8 : 0));
        CHECK(count == ms.size() || n < ms[count].in_off + ms[count].in_len + 8);
        whole_members(piece.data(), n, true, &bad, &count);
        CHECK(bad == (used != n));
    }
    size_t mi = 0;
    uint64_t len = 0, keep_from = 0, total = 0, sum = 0;
    for (uint32_t n : isize) sum += n;
    std::vector<uint64_t> in_off(2 * ms.size() + 2), out_off(ms.size() + 1);
    for (int fill = 0; fill < 100000; ++fill) {
        const uint64_t carry = carry_len(len, keep_from);
        const uint64_t cap = window_capacity(carry, want);
        std::vector<uint8_t> window(cap);  // exact size
        const size_t cnt = plan_batch(ms.data(), ms.size(), mi, carry, want, in_off.data(), out_off.data());
        CHECK(out_off[0] == carry);
        for (size_t j = 0; j < cnt; ++j) {
            CHECK(in_off[2 * j] == ms[mi + j].in_off && in_off[2 * j + 1] - in_off[2 * j] == ms[mi + j].in_len);
            CHECK(in_off[2 * j + 1] + 8 <= f.size());
            CHECK(out_off[j + 1] - out_off[j] == ms[mi + j].isize);  // the members tile the window behind the carry
            CHECK(out_off[j] < want);                                // taken only below `want`
            if (ms[mi + j].isize) std::memset(window.data() + out_off[j], 1, ms[mi + j].isize);
        }
        CHECK(out_off[cnt] + SLACK <= cap);
        CHECK(mi + cnt == ms.size() || out_off[cnt] >= want);  // stopped by `want` or by the file's end
        if (carry >= want) CHECK(cnt == 0);
        for (uint64_t k = carry; k < out_off[cnt]; ++k) CHECK(window[k] == 1);
        mi += cnt;
        total += out_off[cnt] - carry;
        len = out_off[cnt];
        if (mi == ms.size()) break;
        keep_from = len - len * keep_num / keep_den;  // what the next window keeps
        if (carry_len(len, keep_from) >= want) want *= 2;  // the caller's doubling
    }
    CHECK(mi == ms.size() && total == sum);
}

int main() {
    CHECK(carry_len(10, 10) == 0 && carry_len(10, 0) == 10 && carry_len(0, 0) == 0 && carry_len(10, 3) == 7);
    replay({700}, 4096, 1, 2);                                     // one member
    replay({0}, 4096, 0, 1);                                       // only an empty member
    replay({0, 0, 997, 0, 997, 997, 0, 0, 12, 0}, 1500, 1, 3);     // empty members at every place
    replay({65280, 65280, 65280, 100}, 1000, 1, 10);               // `want` below a member
    replay({65536, 1, 65536}, 65536, 9, 10);                       // the format's largest members
    replay({997, 997, 997, 997, 997, 997, 997, 997}, 1200, 19, 20);  // the carry grows past `want`
    std::vector<uint32_t> many;
    for (int k = 0; k < 400; ++k) many.push_back((uint32_t)((k * 7919) % 1500));
    replay(many, 4096, 2, 3);
    // not a member: another flag, another extra field, a size below a member's frame, NUL padding at the end
    std::vector<M> ms;
    std::vector<uint8_t> f = file_of({100, 200}, &ms);
    const size_t second = ms[1].in_off - 18;
    for (int what = 0; what < 4; ++what) {
        std::vector<uint8_t> g = f;
        if (what == 0) g[second + 3] = 12;
        if (what == 1) g[second + 10] = 8;
        if (what == 2) g[second + 16] = 20, g[second + 17] = 0;
        if (what == 3) g.resize(second), g.insert(g.end(), 40, (uint8_t)0);
        bool bad = false;
        size_t count = 0;
        CHECK(whole_members(g.data(), g.size(), what == 3, &bad, &count) == second && bad && count == 1);
    }
    if (fails) return 1;
    std::puts("ok");
    return 0;
}
