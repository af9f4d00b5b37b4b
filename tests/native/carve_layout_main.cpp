// carve_layout_main.cpp -- the eight workspace layouts of the synchronous BLS and slasher calls, taken through carve.h alone
// and printed: one line per layout, "name region=offset ... total=bytes".  tests/test_carve_layout.py compiles this with the host
// compiler (AddressSanitizer, UBSan) and holds the lines to the up256 chains the calls were written with.
//
//   carve_layout_main PAIR_WORDS GT_WORDS GROUP_BYTES SLASH_ROW_BYTES SLASH_TABLE_BYTES < shapes
//
// The takes restate, in order and element type, the ones in engine_bls.cpp (pairing), engine_batch.cpp (batch),
// engine_sigverify.cpp (sums, locate, aggregate), engine_resident_verify.cpp (resident), engine_internal.h (res_points) and
// engine_slash.cpp (slash_rows); the sizes of the kernels' structs come in as arguments.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "carve.h"

using namespace posevo;

namespace {

template <size_t N> struct Blob { unsigned char b[N]; };  // an element of N bytes: G1Group, SlashRow, SlashTable

struct Line {
    Layout L;
    std::string text;
    template <typename T> Region<T> note(const char* name, const Region<T>& r)
    {
        text += std::string(" ") + name + "=" + std::to_string(r.off);
        return r;
    }
    template <typename T> Region<T> take(const char* name, size_t count) { return note(name, L.take<T>(count)); }
    template <typename T = uint8_t> Region<T> take_bytes(const char* name, size_t bytes) { return note(name, L.take_bytes<T>(bytes)); }
    void print(const char* layout) { printf("%s%s total=%zu\n", layout, text.c_str(), L.total()); }
};

template <size_t GROUP, size_t ROW, size_t TABLE> int run(size_t pair_words, size_t gt_words)
{
    char name[32];
    unsigned long long v[6];
    while (scanf("%31s", name) == 1) {
        Line l;
        if (!strcmp(name, "pairing")) {  // n_pairs n_groups out576
            if (scanf("%llu %llu %llu", &v[0], &v[1], &v[2]) != 3) return 2;
            const size_t rows = std::max<size_t>(1, v[0]), ng = v[1];
            l.take<uint8_t>("g1", 96 * rows);
            l.take<uint8_t>("g2", 192 * rows);
            l.take<uint32_t>("off", ng + 1);
            l.take<uint32_t>("ws", pair_words * rows);
            l.take<int32_t>("flag", rows);
            l.take<uint32_t>("gt", gt_words * ng);
            l.take<int32_t>("bad", ng);
            l.take<int32_t>("verdict", ng);
            l.take<uint8_t>("out", v[2] ? 576 * ng : 0);
        } else if (!strcmp(name, "batch")) {  // n chunk fan
            if (scanf("%llu %llu %llu", &v[0], &v[1], &v[2]) != 3) return 2;
            const size_t n = v[0], max_chunks = (n + v[1] - 1) / v[1], rows = n + max_chunks, lvl = (max_chunks + v[2] - 1) / v[2];
            l.take<uint8_t>("pk", 96 * n);
            l.take<uint8_t>("msg", 192 * n);
            l.take<uint8_t>("sig", 192 * n);
            l.take<uint64_t>("scal", n);
            l.take_bytes("neg", 256);
            l.take<int32_t>("status", n);
            l.take<uint32_t>("pkm", 24 * n);
            l.take<uint32_t>("msgm", 48 * n);
            l.take<uint32_t>("sigm", 48 * n);
            l.take<uint32_t>("live", n);
            l.take<uint32_t>("scaled", 96 * n);
            l.take<uint32_t>("ws", pair_words * rows);
            l.take<int32_t>("flag", rows);
            l.take<uint32_t>("off", max_chunks + 1);
            l.take<uint32_t>("gt", gt_words * max_chunks);
            l.take<uint32_t>("lvl0", gt_words * lvl);
            l.take<uint32_t>("lvl1", gt_words * lvl);
            l.take<int32_t>("bad", max_chunks);
            l.take_bytes<int32_t>("zero", 256);
            l.take<int32_t>("verdict", max_chunks);
            l.take<uint8_t>("out", 576);
        } else if (!strcmp(name, "sums")) {  // total n_groups partials2 partials1
            if (scanf("%llu %llu %llu %llu", &v[0], &v[1], &v[2], &v[3]) != 4) return 2;
            l.take<uint32_t>("index", v[0]);
            l.take<uint32_t>("signer", v[0]);
            l.take<uint64_t>("scal", v[0]);
            l.take<Blob<GROUP>>("gr2", v[1]);
            l.take<Blob<GROUP>>("gr1", v[1]);
            l.take<uint32_t>("part2", 96 * v[2]);
            l.take<uint32_t>("part1", 48 * v[3]);
            l.take<uint8_t>("pk", 96 * v[1]);
            l.take<uint8_t>("sig", 192 * v[1]);
        } else if (!strcmp(name, "locate")) {  // n_again
            if (scanf("%llu", &v[0]) != 1) return 2;
            l.take<uint32_t>("rows", 2 * v[0]);
            l.take<uint8_t>("be96", 96 * v[0]);
            l.take<uint8_t>("be192", 192 * v[0]);
        } else if (!strcmp(name, "aggregate")) {  // kept n_groups partials
            if (scanf("%llu %llu %llu", &v[0], &v[1], &v[2]) != 3) return 2;
            l.take<uint32_t>("keep", v[0]);
            l.take<Blob<GROUP>>("g", v[1]);
            l.take<uint32_t>("part", 96 * v[2]);
            l.take<uint8_t>("out", 192 * v[1]);
        } else if (!strcmp(name, "resident")) {  // n_groups n_in n_points point_of_row msg_in_place
            if (scanf("%llu %llu %llu %llu %llu", &v[0], &v[1], &v[2], &v[3], &v[4]) != 5) return 2;
            const size_t ng = v[0], por_bytes = v[3] ? 4 * v[1] : 0;
            const auto head = l.take_bytes("head", 256 + por_bytes);
            l.note("por", head.part<uint32_t>(256, por_bytes / 4));
            l.take<uint8_t>("msg", v[4] ? 0 : 192 * v[2]);
            l.take<uint32_t>("off", ng + 1);
            l.take<uint32_t>("ws", pair_words * 2 * ng);
            l.take<int32_t>("flag", 2 * ng);
            l.take<uint32_t>("gt", gt_words * ng);
            l.take<int32_t>("gbad", ng);
            l.take<int32_t>("fe", ng);
            l.take<uint32_t>("ident", ng);
            l.take<int32_t>("sub", ng);
            const auto out = l.take_bytes<uint32_t>("out", 64 + 4 * ng);
            l.note("verdict", out.part<int32_t>(64, ng));
            if (out.count != 16 + ng) return 3;
        } else if (!strcmp(name, "res_points")) {  // n
            if (scanf("%llu", &v[0]) != 1) return 2;
            const size_t rows = std::max<size_t>(v[0], 1);
            l.take<uint32_t>("pk", 48 * rows);
            l.take<uint32_t>("sig", 48 * rows);
            l.take<uint32_t>("bad", rows);
        } else if (!strcmp(name, "slash_rows")) {  // n_groups cand n_keys
            if (scanf("%llu %llu %llu", &v[0], &v[1], &v[2]) != 3) return 2;
            l.take<uint32_t>("err", 4);
            l.take<int32_t>("status", v[0]);
            l.take<uint32_t>("cslot", v[0]);
            l.take<uint32_t>("id", v[0]);
            l.take<Blob<ROW>>("rows", v[0]);
            l.take<uint32_t>("cand", v[1]);
            l.take<uint32_t>("cnt", v[2]);
            l.take<uint32_t>("start", v[2]);
            l.take<uint32_t>("cursor", v[2]);
            l.take<uint32_t>("list", v[0]);
            l.take<Blob<TABLE>>("tabs", 2);
        } else {
            return 2;
        }
        l.print(name);
    }
    // a zero-count region takes no space: its successor starts where it does; and the bound a transfer checks
    Layout L;
    L.take<uint8_t>(100);
    const auto empty = L.take<uint32_t>(0);
    const auto next = L.take<uint64_t>(5);
    printf("zero_count empty=%zu next=%zu\n", empty.off, next.off);
    printf("holds count=%d count_plus_1=%d empty_0=%d empty_1=%d\n", (int)next.holds(5), (int)next.holds(6), (int)empty.holds(0),
           (int)empty.holds(1));
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 6) return 2;
    const size_t pair_words = strtoull(argv[1], nullptr, 10), gt_words = strtoull(argv[2], nullptr, 10);
    // the struct sizes are template arguments (an element type has a fixed size): the ones kernels.h has today
    if (atoi(argv[3]) != 32 || atoi(argv[4]) != 32 || atoi(argv[5]) != 24) return 4;
    return run<32, 32, 24>(pair_words, gt_words);
}
