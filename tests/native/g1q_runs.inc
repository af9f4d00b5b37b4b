// The lane and tree runs of the host harnesses (fp29_host.cpp, fp30_host.cpp) over the point formulas of
// pos_evolution_amd/csrc/g1_lazy.inc, written once.  Included after the harness's `using namespace` of its field form, so
// fq, g1q and the functions below them are that form's.  worst[0] / worst[1] (optional) receive the largest |limb| (all
// but the top limb) / |top limb| an accumulator coordinate held between adds: the bounds the products rely on.

static void track(const g1q& a, int32_t& worst_limb, int32_t& worst_top)
{
    const fq* cs[4] = {&a.x, &a.y, &a.zz, &a.zzz};
    for (const fq* c : cs) {
        for (int i = 0; i < FQ_N - 1; ++i) {
            const int32_t v = c->l[i] < 0 ? -c->l[i] : c->l[i];
            if (v > worst_limb) worst_limb = v;
        }
        const int32_t t = c->l[FQ_N - 1] < 0 ? -c->l[FQ_N - 1] : c->l[FQ_N - 1];
        if (t > worst_top) worst_top = t;
    }
}
// a registry row (x, y as 12-word Montgomery values of the 32-bit form, all zero = no point) in the field form
static bool row_of(const uint32_t* row, fq& qx, fq& qy)
{
    uint32_t any = 0;
    for (int k = 0; k < 24; ++k) any |= row[k];
    fq_from_mont32(qx, row);
    fq_from_mont32(qy, row + 12);
    return any != 0;
}

// One lane's run: n registry rows added into an empty accumulator in order with the complete mixed add; out = the 48 XYZZ
// words.
static void lane_run(const uint32_t* rows24, int n, uint32_t* out48, int32_t* worst)
{
    g1q acc;
    g1q_set_inf(acc);
    int32_t wl = 0, wt = 0;
    for (int j = 0; j < n; ++j) {
        fq qx, qy;
        const bool any = row_of(rows24 + 24 * j, qx, qy);
        g1q_add_affine(acc, qx, qy, !any);
        track(acc, wl, wt);
    }
    if (worst) { worst[0] = wl; worst[1] = wt; }
    g1q_to_words32(out48, acc);
}

// The same run the way k_g1_accumulate does it: first point as the accumulator (g1q_set_first), every later one through the
// general body alone (g1q_madd_fast); a same-x case only raises the flag and the run is then redone by the complete add.
// *took_slow_path says which way the run went.
static void lane_run_kernel_way(const uint32_t* rows24, int n, uint32_t* out48, int32_t* worst, int* took_slow_path)
{
    g1q acc;
    g1q_set_inf(acc);
    bool exc = false;
    int32_t wl = 0, wt = 0;
    for (int j = 0; j < n; ++j) {
        fq qx, qy;
        if (!row_of(rows24 + 24 * j, qx, qy)) continue;
        if (acc.inf) g1q_set_first(acc, qx, qy);
        else g1q_madd_fast(acc, qx, qy, exc);
        if (exc) break;  // the kernel's lane goes on over garbage; nothing of it is used
        track(acc, wl, wt);
    }
    *took_slow_path = exc ? 1 : 0;
    if (worst) { worst[0] = wl; worst[1] = wt; }
    if (exc) {
        lane_run(rows24, n, out48, nullptr);
        return;
    }
    g1q_to_words32(out48, acc);
}

// k_g1_accumulate + k_g1_tree at the level of their formulas: lanes of k rows each accumulate the kernel's way, and the lanes'
// accumulators -- handed over as they are, lazy limbs and all, all limbs zero for infinity -- are reduced pairwise, level by
// level, with the complete add g1q_add.  out = the 48 words k_g1_finish reads; worst covers the tree's adds.
static void tree_run(const uint32_t* rows24, int n, int k, uint32_t* out48, int32_t* worst)
{
    const int lanes = (n + k - 1) / k;
    g1q* acc = new g1q[lanes > 0 ? lanes : 1];
    for (int l = 0; l < lanes; ++l) {
        const int cnt = (l + 1) * k <= n ? k : n - l * k;
        g1q a;
        g1q_set_inf(a);
        bool exc = false;
        for (int j = 0; j < cnt; ++j) {
            fq qx, qy;
            if (!row_of(rows24 + 24 * (l * k + j), qx, qy)) continue;
            if (a.inf) g1q_set_first(a, qx, qy);
            else g1q_madd_fast(a, qx, qy, exc);
        }
        if (exc) {  // the kernel's second run of the lane
            g1q_set_inf(a);
            for (int j = 0; j < cnt; ++j) {
                fq qx, qy;
                const bool any = row_of(rows24 + 24 * (l * k + j), qx, qy);
                g1q_add_affine(a, qx, qy, !any);
            }
        }
        if (a.inf) g1q_set_inf(a);  // all limbs zero: what the hand-over writes for an empty lane
        acc[l] = a;
    }
    int32_t wl = 0, wt = 0;
    for (int m = lanes; m > 1; m = (m + 1) / 2) {
        for (int i = 0; i < m / 2; ++i) {
            g1q a = acc[2 * i];
            a.inf = fq_limbs_zero(a.zz);  // the tree learns "infinity" from the limbs, not from a flag
            g1q b = acc[2 * i + 1];
            b.inf = fq_limbs_zero(b.zz);
            a.affine = b.affine = false;
            g1q_add(a, b);
            if (a.inf) g1q_set_inf(a);
            acc[i] = a;
            track(a, wl, wt);
        }
        if (m & 1) acc[m / 2] = acc[m - 1];
    }
    if (worst) { worst[0] = wl; worst[1] = wt; }
    if (lanes == 0) {
        for (int w = 0; w < 48; ++w) out48[w] = 0;
    } else {
        g1q r = acc[0];
        r.inf = fq_limbs_zero(r.zz);
        g1q_to_words32(out48, r);
    }
    delete[] acc;
}
