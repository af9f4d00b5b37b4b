// att_signing_kernels.hip -- the signing roots of attestation rows, for gfx950: the 32-byte messages
// pe_hash_to_g2 maps to H(m), from the rows where they lie.
//   k_att_signing_roots   one lane per root: row i of an array of rows, or row grp[g].rep of the resident aggregate's group g
// The rule is att_signing_row.h, the same text the host test compiles: nine sha256_64 per row through one copy of the hash in
// a loop.  Integer work, about 30 000 VALU operations against 128 bytes read and 32 written per lane; a row's words are read
// where the step that hashes them needs them, each once.  No LDS, no scratch (the Makefile keeps the compiler's resource
// report, tests/test_att_signing_host.py reads it).
#include <hip/hip_runtime.h>

#include "att_signing_row.h"
#include "kernels.h"

namespace posevo {

struct AttSigningArgs {
    const uint32_t* rows;   // n_rows rows of ATT_ROW_WORDS words
    uint32_t n_rows;
    const AttGroup* grp;    // nullable: root g is of row grp[g].rep, else of row g
    const AttPlan* plan;    // with grp: the group count, read here
    uint32_t n;             // roots; with grp: the host's upper bound of the groups
    AttDomains dom;
    uint32_t* out;          // 8 words per root, memory order
};

__global__ void __launch_bounds__(256)
k_att_signing_roots(const AttSigningArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t n = a.n;
    if (a.grp) {
        const uint32_t formed = a.plan->n_groups;
        n = formed < n ? formed : n;
    }
    if (i >= n) return;
    const uint32_t r = a.grp ? a.grp[i].rep : i;
    uint32_t root[8] = {};
    if (r < a.n_rows) att_signing_root(a.rows + (uint64_t)ATT_ROW_WORDS * r, a.dom, nullptr, root);
    uint32_t* dst = a.out + 8ull * i;
#pragma unroll
    for (int k = 0; k < 8; ++k) dst[k] = __builtin_bswap32(root[k]);
}

void launch_att_signing_roots(hipStream_t s, const void* rows, uint32_t n_rows, const AttGroup* grp, const AttPlan* plan,
                              uint32_t n, const AttDomains& dom, uint8_t* out_roots32)
{
    if (n == 0) return;
    AttSigningArgs a;
    a.rows = static_cast<const uint32_t*>(rows);
    a.n_rows = n_rows;
    a.grp = grp;
    a.plan = plan;
    a.n = n;
    a.dom = dom;
    a.out = reinterpret_cast<uint32_t*>(out_roots32);
    hipLaunchKernelGGL(k_att_signing_roots, dim3((n + 255) / 256), dim3(256), 0, s, a);
}

}  // namespace posevo
