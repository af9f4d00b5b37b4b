// slashbench.hip -- the slasher's scan kernel (slash_kernels.hip) on its own, under HIP events, at the configs[3] shape:
// 1 048 576 validators in 2048 committees of 512, one full row per committee, every validator attesting, a full history of
// H honest records behind it (steady state: every slot but the new epoch's holds a record).  H = 16, 64, 256 alone, then
// H = 64 beside a running k_g1_accumulate (the step's dominant kernel, set up as tools/accbench.hip does).
// It prints algorithmic bytes / time -- 8 H + 12 bytes per attesting validator, DESIGN 3 -- against the 6.29 TB/s that
// DESIGN 3 uses as the achievable HBM rate, and the shader clock of the run.  A measurement, not a test: no threshold.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I../pos_evolution_amd/csrc -I../include -o slashbench slashbench.hip
#include "../pos_evolution_amd/csrc/g1_kernels.hip"
#include "../pos_evolution_amd/csrc/slash_kernels.hip"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using namespace posevo;
#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

__global__ void k_clock(unsigned long long* out)   // shader cycles per 100 MHz tick over ~50 us
{
    const unsigned long long w0 = wall_clock64(), c0 = clock64();
    while (wall_clock64() - w0 < 5000) __builtin_amdgcn_s_sleep(8);
    out[0] = wall_clock64() - w0;
    out[1] = clock64() - c0;
}

int main()
{
    const uint32_t NC = 2048, SIZE = 512;
    const uint64_t NV = (uint64_t)NC * SIZE;
    const double ACHIEVABLE = 6.29e12;
    std::mt19937_64 rng(7);
    // a random partition: validator -> (committee, position)
    std::vector<uint32_t> perm(NV), inv_comm(NV), inv_pos(NV), crow_start(NC + 1), crow_list(NC);
    for (uint64_t i = 0; i < NV; ++i) perm[i] = (uint32_t)i;
    std::shuffle(perm.begin(), perm.end(), rng);
    for (uint64_t i = 0; i < NV; ++i) { inv_comm[perm[i]] = (uint32_t)(i / SIZE); inv_pos[perm[i]] = (uint32_t)(i % SIZE); }
    for (uint32_t c = 0; c <= NC; ++c) crow_start[c] = c;
    std::vector<SlashRow> rows(NC);
    for (uint32_t c = 0; c < NC; ++c) {
        crow_list[c] = c;
        rows[c] = SlashRow{c * (SIZE / 8), SIZE, 0, 0, c, {0, 0, 0}};
    }
    uint32_t *d_inv_comm, *d_inv_pos, *d_cs, *d_cl, *d_counter, *d_ev;
    uint8_t* d_bits;
    SlashRow* d_rows;
    SlashTable* d_tab;
    CHECK(hipMalloc(&d_inv_comm, 4 * NV));
    CHECK(hipMalloc(&d_inv_pos, 4 * NV));
    CHECK(hipMalloc(&d_cs, 4 * (NC + 1)));
    CHECK(hipMalloc(&d_cl, 4 * NC));
    CHECK(hipMalloc(&d_counter, 256));
    CHECK(hipMalloc(&d_ev, 24 * 4096));
    CHECK(hipMalloc(&d_bits, NV / 8));
    CHECK(hipMalloc(&d_rows, sizeof(SlashRow) * NC));
    CHECK(hipMalloc(&d_tab, sizeof(SlashTable)));
    CHECK(hipMemcpy(d_inv_comm, inv_comm.data(), 4 * NV, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_inv_pos, inv_pos.data(), 4 * NV, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_cs, crow_start.data(), 4 * (NC + 1), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_cl, crow_list.data(), 4 * NC, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_bits, 0xFF, NV / 8));
    const SlashTable tab{d_inv_comm, d_inv_pos, d_cs};
    CHECK(hipMemcpy(d_tab, &tab, sizeof(tab), hipMemcpyHostToDevice));

    // the accumulation beside which the last measurement runs (accbench's plan at k = 16)
    uint32_t *d_pts, *d_pts30, *d_mem, *d_lane, *d_wg;
    G1Group* d_groups;
    const uint32_t K = 16, tasks = SIZE / K, lb = 5, n_slots = NC << lb;
    {
        std::vector<uint32_t> pts((size_t)NV * G1_ROW_WORDS, 0);
        for (uint64_t i = 0; i < NV; ++i) {
            for (int k = 0; k < 24; ++k) pts[i * G1_ROW_WORDS + k] = (uint32_t)rng();
            pts[i * G1_ROW_WORDS + 11] &= 0x0fffffffu;
            pts[i * G1_ROW_WORDS + 23] &= 0x0fffffffu;
        }
        std::vector<G1Group> g(NC);
        for (uint32_t i = 0; i < NC; ++i) {
            g[i].member_start = i * SIZE; g[i].n_members = SIZE; g[i].bits_word = NONE32; g[i].slot_base = i << lb;
            g[i].n_tasks = tasks; g[i].k = K; g[i].log2_block = lb; g[i].out_base = i;
        }
        CHECK(hipMalloc(&d_pts, pts.size() * 4));
        CHECK(hipMalloc(&d_pts30, pts.size() * 4));
        CHECK(hipMalloc(&d_mem, 4 * NV));
        CHECK(hipMalloc(&d_lane, (size_t)G1_LANE_PARTIAL_BYTES * 131072 * 2));
        CHECK(hipMalloc(&d_wg, (size_t)G1X_WORDS * NC * 4 * 4));
        CHECK(hipMalloc(&d_groups, sizeof(G1Group) * NC));
        CHECK(hipMemcpy(d_pts, pts.data(), pts.size() * 4, hipMemcpyHostToDevice));
        CHECK(hipMemcpy(d_mem, perm.data(), 4 * NV, hipMemcpyHostToDevice));
        CHECK(hipMemcpy(d_groups, g.data(), sizeof(G1Group) * NC, hipMemcpyHostToDevice));
        launch_g1_table_s30(0, d_pts, d_pts30, NV);
        CHECK(hipDeviceSynchronize());
    }
    hipStream_t s_scan, s_acc;
    CHECK(hipStreamCreateWithFlags(&s_scan, hipStreamNonBlocking));
    CHECK(hipStreamCreateWithFlags(&s_acc, hipStreamNonBlocking));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    {
        unsigned long long *d_clk, clk[2];
        CHECK(hipMalloc(&d_clk, 16));
        for (int i = 0; i < 3; ++i) launch_g1_accumulate(0, d_pts30, d_mem, nullptr, d_groups, NC, n_slots, d_lane, d_wg, nullptr, nullptr);
        hipLaunchKernelGGL(k_clock, dim3(1), dim3(64), 0, 0, d_clk);
        CHECK(hipMemcpy(clk, d_clk, 16, hipMemcpyDeviceToHost));
        hipDeviceProp_t prop;
        CHECK(hipGetDeviceProperties(&prop, 0));
        printf("device %s, %d CUs, shader clock %.0f MHz (behind three accumulations)\n", prop.name, prop.multiProcessorCount,
               100.0 * (double)clk[1] / (double)clk[0]);
    }
    for (int pass = 0; pass < 4; ++pass) {
        const uint32_t H = pass == 0 ? 16 : pass == 1 ? 64 : pass == 2 ? 256 : 64;
        const bool beside = pass == 3;
        unsigned long long* d_rec;
        uint32_t* d_ids;
        CHECK(hipMalloc(&d_rec, 8ull * H * NV));
        CHECK(hipMalloc(&d_ids, 4ull * H * NV));
        // honest history: epoch e (slot e mod H) holds (source e - 1, target e) for every validator; epochs base - H + 1 .. base - 1
        const uint32_t base = 1000;
        {
            std::vector<unsigned long long> slot(NV);
            for (uint32_t e = base - H + 1; e < base; ++e) {
                std::fill(slot.begin(), slot.end(), ((unsigned long long)(e + 1) << 32) | (e - 1));
                CHECK(hipMemcpy(d_rec + (uint64_t)(e % H) * NV, slot.data(), 8 * NV, hipMemcpyHostToDevice));
            }
            CHECK(hipMemset(d_ids, 0, 4ull * H * NV));
        }
        std::vector<float> us;
        for (int rep = 0; rep < 12; ++rep) {
            // the new epoch's votes: target `base`, source base - 1, into the cleared slot of the epoch that left the window
            for (auto& r : rows) { r.source = base - 1; r.target = base; }
            CHECK(hipMemcpyAsync(d_rows, rows.data(), sizeof(SlashRow) * NC, hipMemcpyHostToDevice, s_scan));
            CHECK(hipMemsetAsync(d_rec + (uint64_t)(base % H) * NV, 0, 8 * NV, s_scan));
            CHECK(hipMemsetAsync(d_counter, 0, 4, s_scan));
            CHECK(hipStreamSynchronize(s_scan));
            SlashArgs a{};
            a.rows = d_rows; a.tables = d_tab; a.n_tables = 1; a.crow_list = d_cl; a.bits = d_bits;
            a.rec = d_rec; a.ids = d_ids; a.history = H; a.n_val = NV;
            a.counter = d_counter; a.evidence = d_ev; a.cap = 4096; a.flags = nullptr;
            if (beside) {
                for (int k = 0; k < 3; ++k)
                    launch_g1_accumulate(s_acc, d_pts30, d_mem, nullptr, d_groups, NC, n_slots, d_lane, d_wg, nullptr, nullptr);
            }
            CHECK(hipEventRecord(e0, s_scan));
            launch_slash_scan(s_scan, a);
            CHECK(hipEventRecord(e1, s_scan));
            CHECK(hipEventSynchronize(e1));
            CHECK(hipDeviceSynchronize());
            float t;
            CHECK(hipEventElapsedTime(&t, e0, e1));
            us.push_back(t * 1e3f);
            uint32_t found = 0;
            CHECK(hipMemcpy(&found, d_counter, 4, hipMemcpyDeviceToHost));
            if (found) { printf("unexpected evidence: %u\n", found); return 1; }
        }
        std::sort(us.begin(), us.end());
        const double bytes = (double)NV * (8.0 * H + 12.0);
        const double med = us[us.size() / 2];
        printf("k_slash_scan H=%3u %s: min %.1f med %.1f max %.1f us | %.0f MB algorithmic | %.2f TB/s at the median = %.2f of %.2f TB/s | floor %.0f us\n",
               H, beside ? "beside k_g1_accumulate" : "alone                 ", us.front(), med, us.back(), bytes / 1e6,
               bytes / med / 1e6, bytes / med / 1e6 / (ACHIEVABLE / 1e12), ACHIEVABLE / 1e12, bytes / ACHIEVABLE * 1e6);
        CHECK(hipFree(d_rec));
        CHECK(hipFree(d_ids));
    }
    return 0;
}
