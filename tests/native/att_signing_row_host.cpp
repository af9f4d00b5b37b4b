// att_signing_row_host.cpp -- pos_evolution_amd/csrc/att_signing_row.h under a plain host compiler, as a program of its own
// (tests/test_att_signing_host.py).  stdin: fork_epoch (8 bytes little-endian) | domain_previous (32) | domain_current (32) |
// rows of 144 bytes (pe_attestation); stdout: per row hash_tree_root(AttestationData) | the signing root, 64 bytes, then
// Z[1] as the header states it (32 bytes).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../pos_evolution_amd/csrc/att_signing_row.h"

using namespace posevo;

static void put_words(const uint32_t w[8])
{
    unsigned char b[32];
    for (int k = 0; k < 8; ++k) {
        b[4 * k] = (unsigned char)(w[k] >> 24);
        b[4 * k + 1] = (unsigned char)(w[k] >> 16);
        b[4 * k + 2] = (unsigned char)(w[k] >> 8);
        b[4 * k + 3] = (unsigned char)w[k];
    }
    fwrite(b, 1, 32, stdout);
}

int main()
{
    std::vector<unsigned char> in;
    unsigned char buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), stdin)) > 0) in.insert(in.end(), buf, buf + got);
    if (in.size() < 72 || (in.size() - 72) % (4 * ATT_ROW_WORDS)) return 2;
    uint64_t fork_epoch;
    memcpy(&fork_epoch, in.data(), 8);
    AttDomains d;
    att_domains_load(fork_epoch, in.data() + 8, in.data() + 40, d);
    const size_t n = (in.size() - 72) / (4 * ATT_ROW_WORDS);
    for (size_t i = 0; i < n; ++i) {
        uint32_t row[ATT_ROW_WORDS], data_root[8], root[8];
        memcpy(row, in.data() + 72 + 4 * ATT_ROW_WORDS * i, sizeof(row));
        att_signing_root(row, d, data_root, root);
        put_words(data_root);
        put_words(root);
    }
    put_words(ATT_ZERO_NODE1);
    return 0;
}
