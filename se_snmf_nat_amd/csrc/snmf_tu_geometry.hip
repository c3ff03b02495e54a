// snmf_tu_geometry.hip -- the kernels and launch geometry of a plan (struct PlanGeometry, snmf_internal.h): host code only, a pure
// function of snmf_params, the device's compute-unit count and the plan-creation switches.
#include "snmf_internal.h"
#include "snmf_generic.h"

// The switches that steer plan creation.  Each selects the plain form of a fast path, against which the tests compare it; they
// are read on every plan creation (tests change them between the plans of one process).
namespace {
struct Switches {
    bool hstep_rp;     // SNMF_HSTEP_RP=0: the barrier-phased k_hstep instead of the role pipelines and k_hstep_sf / k_hstep_sr
    bool hstep_split;  // SNMF_HSTEP_SPLIT=0: every tile whole (no split last round, no shared last tiles)
    bool wstats_nl;    // SNMF_WSTATS_NL set to anything but 4: k_wstats without loader waves (so no k_wstats_sf / k_wstats_sr)
    bool wstats_xg;    // SNMF_WSTATS_XG=0: k_wstats' extra row at the top of the tile instead of behind P3's first W loads (k_wstats_xg)
    bool iter_sf;      // SNMF_ITER_SF=0: two launches instead of k_iter_sf
    bool gram_p;       // SNMF_GRAM_P=0: the Euclidean P without the Gram matrix
    int no_small;      // SNMF_NO_SMALL: 1 = no persistent kernel at all (the plan loop), 2 = no register-resident frame kernel
    bool hfold;        // SNMF_HFOLD=0: the H-only loop folds its objective with k_reduce
};
int env_int(const char* name, int unset) {
    const char* e = getenv(name);
    return e ? atoi(e) : unset;
}
Switches read_switches() {
    Switches s;
    s.hstep_rp = env_int("SNMF_HSTEP_RP", 1) != 0;
    s.hstep_split = env_int("SNMF_HSTEP_SPLIT", 1) != 0;
    s.wstats_nl = env_int("SNMF_WSTATS_NL", 4) == 4;
    s.wstats_xg = env_int("SNMF_WSTATS_XG", 1) != 0;
    s.iter_sf = env_int("SNMF_ITER_SF", 1) != 0;
    s.gram_p = env_int("SNMF_GRAM_P", 1) != 0;
    s.no_small = env_int("SNMF_NO_SMALL", 0);
    s.hfold = env_int("SNMF_HFOLD", 1) != 0;
    return s;
}
}  // namespace

int plan_geometry(const snmf_params* pp, int n_cu, PlanGeometry* g) {
    SN_TRY(validate_params(pp));
    const snmf_params& p = *pp;
    const Switches sw = read_switches();
    *g = PlanGeometry{};
    const int F = p.F, T = p.T, r = p.r;
    // masks (src/sparse_nmf.m:142-148, :176-179)
    int n_h = 0, n_w = 0;
    SN_TRY(read_update_masks(pp, &n_h, &n_w, nullptr));
    g->upd_h = n_h > 0;
    g->upd_w = n_w > 0;
    g->bm = (p.beta == 1.0) ? BM_KL : (p.beta == 2.0 ? BM_EUC : BM_GEN);
    g->n_mat = g->bm == BM_KL ? 1 : 2;

    // row geometry (see snmf_kernels.h): F = 32*nf + 1 (257, 513, ...) -> extra-row mode
    g->xr = (F % 32 == 1 && F > 32) ? 1 : 0;
    g->nf = g->xr ? F / 32 : (int)roundup(F, 32) / 32;
    g->Fm = 32 * g->nf;
    g->Fp = g->Fm + 4 * g->xr;
    g->Fq = g->Fm + 8 * g->xr;
    g->rp = (int)roundup(r, 32);
    g->Tp = (int)roundup(T + 32, 64);  // >= 32 zero columns of slack: a 32-frame tile may start at any frame
    g->nk = g->rp / 32;
    g->ldh = g->rp + 4;
    g->ldr = g->Fq + 4;
    // k_hstep geometry: prefer two 4-wave workgroups per CU on 32-frame tiles (their phases
    // de-synchronise and keep the matrix pipe fed); otherwise one 8-wave workgroup per CU on the
    // widest tile whose H image + ratio image fit the 160 KiB LDS.
    const size_t per_col = (size_t)(g->ldh + g->ldr) * 4;
    const size_t lds_cap = 160 * 1024;  // gfx950: 160 KiB per CU, one workgroup may take all of it
    const size_t lds_extra = (size_t)g->rp * 4 + 128;  // extra row of W + the roles' progress slots (6 signals x 4 waves) + the split tile's flag
    const size_t lds1 = 32 * per_col + lds_extra, lds2 = 64 * per_col + lds_extra;
    if (2 * lds1 - lds_extra <= lds_cap) { g->NWH = 8; g->NT = 1; g->NLH = 4; }  // double-buffered
    else if (lds2 <= lds_cap && g->Tp / 64 >= n_cu) { g->NWH = 8; g->NT = 2; }
    else if (lds1 <= lds_cap) { g->NWH = 8; g->NT = 1; }
    else if (16 * per_col + lds_extra <= lds_cap) {
        // the H image + ratio image of 32 frames do not fit (F + r > 1272, e.g. the reference's exemplar setting
        // R_x = R_d = 500 at F = 513, settings/bak_IS16_results/initial_setting_Exemplar.m:47-48): 16-frame tiles
        g->NWH = 8; g->NT = 1; g->TTH = 16;
    } else {
        // F + r beyond what a 16-frame tile's H block + ratio image take of the LDS (~2540): the out-of-envelope path
        g->generic = true;
        g->NWH = 8; g->NT = 1; g->TTH = 16;
    }
    g->hstep_rp = sw.hstep_rp;
    // A workgroup with a single tile has nothing to pipeline: the role pipelines' hand-offs then only add latency (C1,
    // 257 x 2000 r = 40, 63 tiles: k_hstep 16.9 us against k_hstep_rp 18.5), so such problems take the barrier-phased kernel
    if ((T + 31) / 32 <= n_cu) g->hstep_rp = false;
    // F = 513 (9..16 row tiles): two whole tile buffers do not fit, but two H blocks + ONE ratio image do -- k_hstep_rh
    // pipelines on half tiles.  One pair of column tiles per wave of its P2 team: rp <= 256.
    g->lds_rh = std::max<size_t>(((size_t)2 * 32 * g->ldh + (size_t)32 * g->ldr + g->rp) * 4 + 160, 2 * kMaxNW * 64 * sizeof(double));
    g->rh = g->hstep_rp && g->NLH != 4 && g->bm == BM_KL && g->nf >= 9 && g->nf <= 16 && g->rp <= 256 && g->lds_rh <= lds_cap;
    // r = 97..100 on 16 row tiles (the reference's R = 100 at F = 513): P2 cut over the contraction, the 1..4 real columns of
    // the fourth column tile as 4x4x1 MFMAs on the same ratio fragments (k_hstep_rh<OBJ, LXH>); needs 52 KB more LDS for the waves' partial tiles
    {
        const size_t lx = g->lds_rh + 4 * 3 * 1024 * 4 + 4 * 64 * 16;  // the B waves' partial tiles + partial leftover columns
        g->rh_lxh = (g->rh && g->nf == 16 && g->nk == 4 && r > 96 && r <= 100 && lx <= lds_cap) ? 1 : 0;
        if (g->rh_lxh) g->lds_rh = lx;
        // r = 193..200 on 16 row tiles (R_x + R_d = 200 at F = 513, run_basis_DNMF.m:40): seven column tiles -> the B waves work
        // in pairs over three full tiles each, cut in two over the contraction (k_hstep_rh<OBJ, 2>); 29 KB more LDS
        const size_t lx2 = g->lds_rh + (size_t)(4 * 6 * 256 + 4 * 64 * 4 + g->rp) * 4;
        if (g->rh && !g->rh_lxh && g->nf == 16 && g->nk == 7 && r > 192 && r <= 200 && lx2 <= lds_cap) {
            g->rh_lxh = 2;
            g->lds_rh = lx2;
        }
    }
    g->lds_h = std::max<size_t>(g->NLH ? 2 * lds1 - lds_extra : (g->NT == 1 ? (size_t)g->TTH * per_col + lds_extra : lds2),
                                 2 * kMaxNW * 64 * sizeof(double));
    // one or two column tiles (r <= 64) on the double-buffered role pipeline: P2 cut over the contraction (k_hstep_rp<., CUT>):
    // 32 KB of partial tiles + 1 ./ dph + two more signals behind the buffers
    {
        const size_t more = 32 + (size_t)4 * g->nk * 1024 * 4 + (size_t)g->rp * 4;
        const bool shape_ok = g->NLH == 4 && g->NWH == 8 && g->bm == BM_KL && g->nk <= 2 && g->nf >= 4;
        // (rp_cut = 2: the PAIR form -- two column tiles, 8 KB of partials -- where the four-way form's 32 KB do not fit: 513 rows, r = 33..64)
        const size_t more2 = 32 + (size_t)2048 * 4 + (size_t)g->rp * 4;
        g->rp_cut = !shape_ok ? 0 : g->lds_h + more <= lds_cap ? 1 : (g->nk == 2 && g->lds_h + more2 <= lds_cap) ? 2 : 0;
        if (g->rp_cut) g->lds_h += g->rp_cut == 2 ? more2 : more;
    }
    g->lds_mdi = std::max<size_t>(lds1, 2 * kMaxNW * 64 * sizeof(double));  // MDI pass: (NW=8, NT=1, NL=0)
    g->grid_mdi = std::max(1, std::min(g->Tp / 32, n_cu));
    const int n_tiles_h = g->Tp / (g->TTH * g->NT);
    // without loaders the NT == 1 kernels are register-bounded for two workgroups per CU
    int wg_per_cu = (g->lds_h * 2 <= lds_cap && g->NT == 1 && !g->NLH) ? 2 : 1;
    g->grid_h = std::max(1, std::min(n_tiles_h, n_cu * wg_per_cu));
    // k_hstep_rp: only tiles that hold a frame (the pad tiles of both H buffers are zero and stay zero), and the last
    // PARTIAL round split by rows over the workgroups that would idle through it (snmf_kernels.h, "the split last round"):
    // 4 parts per tile when 4 * (tiles of that round) workgroups exist, else 2, else the round stays whole.
    // SNMF_HSTEP_SPLIT=0 keeps every tile in the pipeline (tests compare the two).
    {
        const int G = n_cu;
        g->rp_tiles = (T + 31) / 32;
        g->rp_full = g->rp_tiles;
        g->rp_grid = std::max(1, std::min(g->rp_tiles, G));  // (k_hstep_rh launches on the same grid)
        g->rp_S = 0;
        // (k_hstep_rh splits by CONTIGUOUS row tiles within a half: 16 row tiles only, F = 505..513)
        if ((g->NLH == 4 || (g->rh && g->nf == 16)) && !g->rp_cut && sw.hstep_split) {
            // (only a partial round BEHIND whole ones: a problem of fewer tiles than workgroups is latency-bound, and there
            //  the split's extra steps -- partial stores, the arrival counter, the finishing pass -- cost more than the
            //  shorter MFMA loops save: C1, 257 x 2000 r = 40, ran 23.3 k iterations/s split against 26.7 k whole)
            const int full = (g->rp_tiles / G) * G, R = g->rp_tiles - full;
            int S = (full > 0 && R > 0) ? (4 * R <= G ? 4 : (2 * R <= G ? 2 : 0)) : 0;
            while (S > g->nf) S >>= 1;
            if (S >= 2) {
                g->rp_S = S;
                g->rp_full = full;
                g->rp_grid = G;
            }
        }
    }
    // At most two row tiles and eight column tiles (the Mel solves, r <= 256): a tile per WAVE, nothing handed between waves
    // (snmf_smallf.h).  Follows SNMF_HSTEP_RP (tests compare against the barrier-phased kernels).
    {
        g->lds_sf = ((size_t)g->nf * g->rp * 32 + (size_t)g->nk * g->Fq * 32 + 2 * (size_t)g->rp) * 4 + 2 * 8 * sizeof(double);
        g->sf = g->bm == BM_KL && g->upd_h && !g->xr && g->nf <= 2 && g->nk <= 8 && g->lds_sf <= lds_cap && !g->generic &&
                sw.hstep_rp;
        g->sf_grid = std::max(1, std::min((T + 31) / 32, n_cu));
        // the shared last tile: when the partial wave level behind the whole ones is the FIRST on its SIMDs (level 0 or 4 of 8: any other
        // level runs beside whole tiles of the same round on other SIMDs and sharing it would not end the launch earlier).  SNMF_HSTEP_SPLIT=0
        // keeps every tile whole, like the split last round of k_hstep_rp.
        {
            const int nw = 8 * g->sf_grid, R = g->rp_tiles % nw, wfull = R / g->sf_grid, xb = R % g->sf_grid;
            const size_t more = (size_t)g->nf * 16384 + 16;
            g->sf_share = 0;
            g->sf_nfull = g->rp_tiles;
            // (not for the full updates that snmf_plan_run fuses into k_iter_sf: the step API's two launches -- the sharded loop -- stay
            //  bit for bit what the fused launch computes with every tile whole, tests/test_gpu_parity.py::test_fused_small_f_iteration_equals_the_two_launches;
            //  k_iter_sf shares a chunk's remainder tile in its own way, isf_share)
            const bool isf_shape = g->upd_h && g->upd_w && g->nf == 2 && g->nk >= 3 && g->nk <= 4;
            if (g->sf && !isf_shape && xb > 0 && (wfull == 0 || wfull == 4) && g->nk >= 2 && g->lds_sf + more <= lds_cap && sw.hstep_split) {
                g->sf_share = xb;
                g->sf_nfull = g->rp_tiles - xb;
                g->lds_sf += more;
            }
        }
    }
    // k_wstats geometry: 4-wave workgroups, each wave owns one 32-row tile x NKT 32-column tiles of
    // the statistics in registers.  NKT <= 8 (128 accumulator VGPRs): two workgroups per CU.
    if (g->nk <= 4) { g->NKT = 4; g->WPS = 2; }
    else if (g->nk <= 8) { g->NKT = 8; g->WPS = 2; }
    else { g->NKT = 16; g->WPS = 1; }
    // (eight consumer waves, two per SIMD, for narrow statistics over at least eight row tiles: see the kernel)
    g->NWB = (g->NKT == 4 && g->nf >= 8) ? 8 : 4;
    g->n_kg = (g->nk + g->NKT - 1) / g->NKT;
    g->n_fg = (g->nf + g->NWB - 1) / g->NWB;
    // H image of k_wstats: rows padded to whole NKT-tile groups (branch-free P4, see the kernel)
    g->ldhw = std::max(g->rp, 32 * g->NKT * g->n_kg) + 4;  // (NKT = 4: always 132 -- k_wstats<4, ...> has it as a compile-time constant)
    if (((size_t)32 * g->ldhw + (size_t)32 * 32 * g->NWB) * 4 + (size_t)g->rp * 4 + 320 > lds_cap && g->NKT == 16)
        g->TTW = 16;  // large r: 16-frame tiles (the 32-frame H + V images do not fit the LDS)
    const int n_tiles_w = (T + g->TTW - 1) / g->TTW;  // tiles that hold a frame (an all-padding tile adds exact zeros: skipped)
    {
        // loaders + double buffering when the accumulators allow 2 waves per SIMD and LDS has room; the loader waves
        // stage only the row group's 32 * NWB columns of V (the kernel's ldv), so F = 513 fits as well
        const size_t buf_ld = ((size_t)g->TTW * g->ldhw + (size_t)g->TTW * 32 * g->NWB) * 4;
        g->NLW = (g->WPS == 2 && 2 * buf_ld + (size_t)g->rp * 4 + 512 + (size_t)g->NWB * std::min(g->rp, 256) * 4 <= lds_cap) ? 4 : 0;
        // (loader waves pay from the second tile of a workgroup on; with one tile each -- C1: 63 tiles -- the synchronous
        //  4-wave geometry is faster: 12.7 us against 16.4)
        if (n_tiles_w <= n_cu / std::max(1, ((g->nf + 3) / 4) * g->n_kg)) g->NLW = 0;
        if (!sw.wstats_nl) g->NLW = 0;
        size_t buf = buf_ld;
        if (!g->NLW && g->NWB == 8) {  // the eight-consumer geometry exists with loader waves only
            g->NWB = 4;
            g->n_fg = (g->nf + g->NWB - 1) / g->NWB;
            buf = ((size_t)g->TTW * g->ldhw + (size_t)g->TTW * 32 * g->NWB) * 4;
        }
        // (the fixed-order sums at the end of the kernel use [4][rp] floats / one double per thread of the same memory)
        // (+ ready/done slots + the extra row's V values [2][32] + the consumers' partial extra rows of the slab, NK <= 8)
        const size_t gxs = g->NKT <= 8 ? (size_t)g->NWB * std::min(g->rp, 256) * 4 : 0;
        // a THIRD tile buffer where it fits (r <= 128 at F = 513, C2's geometry): the loader waves then stage two tiles ahead
        // and the consumers stop waiting for `ready` (k_wstats)
        const size_t tail = (size_t)g->rp * 4 + 512 + gxs;  // extra row of W, progress slots + the extra row's V values, gxs
        // (every loader geometry of a gfx950 LDS takes the third buffer: nbw = 2 is not chosen for any shape)
        g->nbw = g->NLW ? 2 : 1;
        if (g->NLW && 3 * buf_ld + tail <= lds_cap) g->nbw = 3;
        g->lds_w = std::max<size_t>(std::max<size_t>((g->NLW ? g->nbw * buf_ld : buf) + tail,
                                                      (size_t)std::max(4, g->NWB) * g->rp * 4),
                                     (size_t)(g->NWB + g->NLW) * 64 * sizeof(double));
    }
    // Fewer row tiles than consumer waves (F = 64, a Mel spectrogram: two): the consumer waves form teams that take the chunk's
    // tiles in turn (StepArgs::til) instead of leaving half the SIMDs without an MFMA wave.  Needs the loader geometry (the
    // teams' partial statistics meet in the tile buffers at the end), one row group, one kappa-group, no extra row.
    // (k_wstats_sf below takes every shape this admits, so no plan launches the teams: til = 1 in the end)
    g->til = 1;
    if (g->NLW && g->TTW == 32 && !g->xr && g->n_fg == 1 && g->n_kg == 1 && g->upd_w && g->NKT == 4 && g->bm == BM_KL) {
        int til = 1;
        while (til * 2 * g->nf <= g->NWB) til *= 2;
        const size_t per_wave = (size_t)(g->NKT * 16 + 8) * 64 * 4;
        while (til > 1 && (size_t)(til - 1) * (g->NWB / til) * per_wave > g->lds_w) til /= 2;
        g->til = til;
    }
    // ... and the KL statistics of the same shapes (r <= 128) through k_wstats_sf; needs the loader geometry, so follows SNMF_WSTATS_NL
    // (tests compare against the synchronously staging kernels)
    {
        const int ncl = 8 / std::max(1, g->nf);
        g->lds_wsf = ((size_t)(ncl - 1) * g->nf * g->nk * 1024 + (size_t)ncl * g->rp) * 4 + 8 * sizeof(double) + 64;
        g->wsf = g->bm == BM_KL && g->upd_w && !g->xr && g->nf <= 2 && g->nk <= 4 && g->TTW == 32 && g->n_kg == 1 && g->n_fg == 1 &&
                  g->NLW && !g->generic && g->lds_wsf <= lds_cap;
        if (g->wsf) g->til = 1;
        g->wsf_share = g->wsf && g->nf == 2 && g->nk >= 2 && !(g->upd_h && g->nk >= 3) && sw.hstep_split;  // (not the shapes of k_iter_sf: see sf_share)
    }
    // ... and, for FULL updates of those shapes, both half-steps in one launch (k_iter_sf; the run loop only: the step API keeps
    // the two launches, between which a multi-rank caller sums nothing but could).  SNMF_ITER_SF=0 keeps two launches.
    {
        const int ncl = 4;  // SIMD pairs (H wave + W wave) per workgroup = chunk lanes of k_wstats_sf at two row tiles
        // (images, 1 ./ dph and lambda, ncl + 1 hand-off buffers, 16 progress words, the H waves' fp64 objective sums and the W waves' row sums per lane)
        const size_t body = ((size_t)g->nf * g->rp * 32 + (size_t)g->nk * g->Fq * 32 + 2 * (size_t)g->rp + (size_t)(ncl + 1) * 32 * (32 * g->nk + 4) + 16) * 4 + (size_t)ncl * 64 * 2 * sizeof(double) + (size_t)ncl * 64 * 4 * 4;
        const size_t tail = ((size_t)ncl * g->nf * g->nk * 1024 + (size_t)ncl * g->rp) * 4 + 2 * ncl * sizeof(double);
        g->lds_isf = std::max(body, tail) + 64;
        g->isf = g->sf && g->wsf && g->nf == 2 && g->nk >= 3 && g->upd_h && g->upd_w && g->lds_isf <= lds_cap && sw.iter_sf;
    }
    // Small rank on tall spectrograms (r <= 32 on 3..16 row tiles; the reference's R = 20 / 10 / 30 at F = 513): a tile per workgroup
    // cut by ROW TILES over its eight waves, every operand straight into the MFMA layouts (snmf_smallr.h).  Follow SNMF_HSTEP_RP /
    // SNMF_WSTATS_NL like the other fast paths (tests compare against the plain kernels).
    {
        const bool shape = g->bm == BM_KL && g->nf >= 3 && g->nf <= 16 && g->nk == 1 && !g->generic && g->TTW == 32 && g->TTH == 32;
        g->lds_sr = sr_hstep_lds_bytes(g->nk, g->Fq, g->rp);
        g->sr = shape && g->upd_h && g->hstep_rp && g->lds_sr <= lds_cap;
        g->sr_grid = std::max(1, std::min((T + 31) / 32, n_cu));
        g->lds_wsr = sr_wstats_lds_bytes(g->rp);
        g->wsr = shape && g->upd_w && g->NLW;
        if (g->wsr) {  // one workgroup per frame chunk carries every row tile: no row groups
            g->n_fg = 1;
            g->n_kg = 1;
            g->til = 1;
        }
    }
    const int wg_w = g->NLW ? 1 : g->WPS;  // workgroups per CU
    g->n_chunks = std::max(1, std::min(n_tiles_w, n_cu * wg_w / std::max(1, g->n_fg * g->n_kg)));
    // Two row groups, only group 0 carries the extra row: deal the workgroups out so that both finish together.
    // Relative cost x of the extra row per tile: ~2.1 k cycles at rp = 256 against 21 k for the two MFMA loops (phase
    // stamps; a sweep of the split point on C2 had its optimum where this x puts it: 131..135 chunks for group 0,
    // k_wstats 0.2573 -> 0.2481 ms, profiles/r02_experiments.md).
    // (Round 7 stamps on C2: 1.61 k of 21.2 k cycles per group-0 tile, x = 0.083; k_wstats_xg hides part of the row under P3's
    //  first W loads -- 1.15 k, see below -- and keeps this x: at C2 131 : 125 is the optimum for every x > 0 (24 tiles + rows
    //  against 25 tiles; any other deal gives a group 25 tiles + rows or 27 tiles), and a plan's deal decides its chunks' fp32
    //  sums, which stay what they were.)
    g->n_ch1 = 0;
    if (g->xr && g->n_fg >= 2 && g->n_kg == 1 && g->NLW && g->upd_w && n_tiles_w >= 4 * g->n_chunks) {
        const int tot = g->n_fg * g->n_chunks, ng1 = g->n_fg - 1;  // group 0: n0 workgroups, every other group n1
        // (the row is shared by the group's NWB waves.  Round 4 re-measured it with phase stamps at 513 x 72000, r = 100 -- a group-0
        //  tile takes 12 % longer per wave -- and swept x over 0.065 .. 0.22: the split this model picks (x = 0.065 there) is within
        //  0.5 % of the best one, larger x loses 4 % to the tile-count quantisation)
        const double x = (600.0 + 6.0 * g->rp) / (82.0 * (g->rp / 2 + 16 * g->nk)) * 4.0 / g->NWB;
        auto n1_of = [&](int n0) { return (tot - n0) / ng1; };
        auto cost = [&](int n0) {
            return std::max(std::ceil((double)n_tiles_w / n0) * (1.0 + x), std::ceil((double)n_tiles_w / n1_of(n0)));
        };
        int best = g->n_chunks;
        for (int n0 = g->n_chunks + 1; n0 <= g->n_chunks + g->n_chunks / 4 && n1_of(n0) >= 1; ++n0)
            if (cost(n0) < cost(best) - 1e-9) best = n0;
        if (best != g->n_chunks) {
            g->n_ch1 = n1_of(best);
            g->n_chunks = best;
        }
    }
    // The extra row of the KL statistics of FULL updates on the NK = 8, 4 + 4-wave loader geometry with at most two row groups (the
    // headline) runs behind P3's first W-fragment loads (k_wstats_xg); four-group plans, the statistics launch of a W-only solve
    // (it also sums the objective) and every other instantiation keep it at the top of the tile.  SNMF_WSTATS_XG=0: there as well
    // -- describe() then says so; the default text is the one the recorded plans pin.
    {
        const bool shape = g->xr && g->bm == BM_KL && g->upd_w && g->upd_h && g->NKT == 8 && g->NWB == 4 && g->NLW == 4 && g->TTW == 32 &&
                           g->n_fg <= 2 && g->n_kg == 1 && !g->wsr;
        g->wxg = shape && sw.wstats_xg;
        g->wxg_off = shape && !sw.wstats_xg;
    }
    // start-up stagger (cycles) of the second half of each grid: about half a tile period when two
    // workgroups share a CU.
    {
        const int mf_h = (g->nf + g->NWH - 1) / g->NWH * g->NT * (g->rp / 2) +
                         (g->nk + g->NWH - 1) / g->NWH * g->NT * (g->Fq / 2);
        g->stagger_h = (g->grid_h > n_cu) ? mf_h * 64 : 0;
    }
    if (g->lds_w > lds_cap && g->upd_w) g->generic = true;  // r too large for k_wstats' H image
    if (g->bm == BM_EUC && g->NKT == 16 && g->TTW == 32 && g->upd_w) {
        // Q = V * H^T of the Euclidean W step needs no Lam', so nothing is recomputed when the statistics' columns are cut
        // into 256-wide kappa-groups: the NK = 16 geometry (256 accumulator registers, no room for loader waves, 116
        // spilled VGPRs) is replaced for this launch by <8,4,4,2> with double-buffered LDS-DMA staging
        g->kq_kg = (g->nk + 7) / 8;
        g->kq_chunks = std::max(1, std::min(std::min(n_tiles_w, g->n_chunks), n_cu / std::max(1, g->n_fg * g->kq_kg)));
        g->kq_lds = (size_t)2 * 32 * (260 + 32 * 4) * 4 + (size_t)g->rp * 4 + 512 + (size_t)4 * 256 * 4;
    }
    // Euclidean full updates: P through the Gram matrix (launch_gram_p) wherever it is the cheaper form (2 r^2 T against
    // 4 F T r; W-only solves take their objective from the P launch's Lam' and keep it)
    // SNMF_GRAM_P=0 opts out: P = max(W*H, flr)*H' is then formed from the Lam' pass exactly as src/sparse_nmf.m:228-233 writes
    // it (the two forms differ only where W*H sits below the 1e-9 floor, by at most flr * sum(h) per entry: include/snmf.h)
    if (g->bm == BM_EUC && g->upd_w && g->upd_h && g->TTW == 32 && r < 2 * F && sw.gram_p) {
        g->gram_p = true;
        const int nfg_g = (g->rp / 32 + g->NWB - 1) / g->NWB;
        g->gram_chunks = g->kq_kg ? g->kq_chunks
                                    : std::max(1, std::min(n_tiles_w, n_cu * (g->NLW ? 1 : g->WPS) / std::max(1, nfg_g)));
    }
    // k_wstats keeps the row sums of H (KL) and the extra row of the slab (F = 32n+1) in per-thread registers: 1024 columns
    if (g->rp > 4 * g->NWB * 64 && g->upd_w && (g->bm == BM_KL || g->xr)) g->generic = true;

    g->lds_wfin = (size_t)9 * g->n_mat * g->Fp * sizeof(double);
    g->wfin = g->upd_w && g->lds_wfin + 12 * 1024 <= lds_cap;
    // very few columns (r <= 32: the reference's R = 20 / 10 / 30): cut every column's rows into slices, a workgroup each (k_wfin,
    // gridDim.y): r * S workgroups of at least eight 16-byte cells each.  Measured (513 x 72000): r = 10 W-only 13 824 -> 14 474 it/s,
    // r = 20 7 615 -> 7 744; from r = 100 up the gather costs what the wider read saves (a11 17.3 -> 17.4 us, Mel 11.3 -> 12.5), so
    // those keep one workgroup per column.
    {
        int S = r <= 32 ? std::max(1, std::min(8, n_cu / std::max(1, r))) : 1;
        while (S > 1 && (g->Fp / 4 + S - 1) / S < 8) --S;
        g->wfin_S = g->wfin ? S : 1;
    }

    // persistent single-launch path for the online shape (H-only, at most one 32-frame tile)
    {
        const size_t need = ((size_t)32 * (g->ldh + g->ldr) + ((g->rp + 3) & ~3)) * 4 + 2 * 512 * sizeof(double);
        g->small_ok = g->upd_h && !g->upd_w && need <= lds_cap;   // shape admits the persistent kernel
        g->small = g->small_ok && T <= 32 && sw.no_small != 1;
        g->lds_small = need;
        // one frame per solve: register-resident dictionary (k_hsolve_frame), F <= 64*FB + 1, r <= 8*KB
        if (g->small_ok && sw.no_small == 0) {
            static const int fbs[2] = {4, 8}, kbs[2] = {16, 25};
            for (int fi = 0; fi < 2 && !g->frame_fb; ++fi)
                for (int ki = 0; ki < 2 && !g->frame_fb; ++ki)
                    if (F <= 64 * fbs[fi] + 1 && r <= 8 * kbs[ki]) {
                        g->frame_fb = fbs[fi];
                        g->frame_kb = kbs[ki];
                    }
            if (g->frame_fb) {
                const int Fm2 = 64 * g->frame_fb, RB = 8 * g->frame_kb, nv = g->bm == BM_KL ? 1 : 2;
                g->lds_frame = (size_t)(40 + 4 * RB + 3 * (Fm2 + 4) + 8 * Fm2 + nv * 16 * (RB + 1)) * 4;
                if (g->lds_frame > lds_cap) g->frame_fb = g->frame_kb = 0;
            }
        }
    }
    if (g->generic) {
        // none of the fused geometries applies; contractions over the frames are split into chunks of kGChunkT frames,
        // whose slabs k_reduce adds like the fast path's
        g->hstep_rp = g->rh = false;
        g->rh_lxh = 0;
        g->rp_S = 0;
        g->kq_kg = 0;
        g->gram_p = false;
        g->n_ch1 = 0;
        g->wxg = g->wxg_off = false;
        g->small_ok = g->small = false;
        g->frame_fb = g->frame_kb = 0;
        g->wfin = false;
        g->n_fg = g->n_kg = 1;
        g->n_chunks = (T + kGChunkT - 1) / kGChunkT;
        g->grid_h = g->grid_mdi = kGBlocks;
    }
    g->fold_obj = g->upd_h && !g->upd_w && !g->generic && sw.hfold;
    // k_iter_sf where its grid is the statistics' chunk grid and k_wfin finishes the W step (snmf_plan_run)
    g->isf = g->isf && g->wfin && g->n_chunks == g->sf_grid;
    g->isf_share = g->isf && sw.hstep_split;
    // the kernel of the H-update launches (objective-only launches run the k_hstep of the geometry, MDI plans their own pass)
    if (!g->upd_h || g->generic) g->hupd = HUPD_PLAIN;
    else if (g->sr) g->hupd = HUPD_SR;
    else if (g->sf) g->hupd = HUPD_SF;
    else if (g->rh) g->hupd = HUPD_RH;
    else if (g->NWH == 8 && g->NLH == 4 && g->hstep_rp && g->bm == BM_KL) g->hupd = HUPD_RP;
    else g->hupd = HUPD_PLAIN;
    return SNMF_OK;
}

void describe_geometry(const PlanGeometry& g, const snmf_params& p, int n_cu, bool mdi, char* buf, size_t n) {
    if (g.generic) {
        snprintf(buf, n, "F=%d T=%d r=%d beta=%g | out-of-envelope path (intermediates in HBM: k_g_gemm / k_g_ratio / k_g_hupd, %d frame splits) | n_cu=%d",
                 p.F, p.T, p.r, p.beta, g.n_chunks, n_cu);
        return;
    }
    const HUpd h = mdi ? HUPD_PLAIN : g.hupd;  // (an MDI plan's H updates are its Lam pass: k_hstep)
    char hs[256];
    switch (h) {
    case HUPD_SR:
        snprintf(hs, sizeof hs, "k_hstep_sr (a tile per workgroup cut by row tiles over 8 waves, operands straight into the MFMA layouts, partial numerators meet in LDS; %d tiles, grid %d)", g.rp_tiles, g.sr_grid);
        break;
    case HUPD_SF:
        if (g.isf)
            snprintf(hs, sizeof hs, "k_iter_sf (H step + W statistics of a full update in ONE launch, 4 SIMD pairs of an H wave and a W wave per workgroup%s; %d tiles, grid %d; step API: k_hstep_sf)", g.isf_share ? ", a chunk's single remainder tile shared by the four pairs" : "", g.rp_tiles, g.n_chunks);
        else
            snprintf(hs, sizeof hs, "k_hstep_sf (a tile per wave from first load to last store, 8 waves per workgroup; %d tiles, the last %d shared by four waves each, grid %d)", g.rp_tiles, g.sf_share, g.sf_grid);
        break;
    case HUPD_RH:
        snprintf(hs, sizeof hs, "k_hstep_rh (4 P1 + 4 P2 + 4 loader waves on half tiles%s; %d of %d tiles pipelined, last round split %d ways, grid %d)",
                 g.rh_lxh == 1 ? ", P2 cut four ways over the contraction + leftover columns as 4x4x1 MFMAs" : (g.rh_lxh == 2 ? ", P2 in wave pairs cut over the contraction + leftover columns as 4x4x1 MFMAs" : ""), g.rp_full, g.rp_tiles, g.rp_S, g.rp_grid);
        break;
    case HUPD_RP:
        snprintf(hs, sizeof hs, "k_hstep_rp (4 P1 + 4 P2 + 4 loader waves%s; %d of %d tiles pipelined, last round split %d ways, grid %d)",
                 g.rp_cut == 2 ? ", P2 in wave pairs cut over the contraction" : g.rp_cut ? ", P2 cut four ways over the contraction" : "", g.rp_full, g.rp_tiles, g.rp_S, g.rp_grid);
        break;
    case HUPD_PLAIN:
        if (mdi)  // (launch_hstep_mdi_b: k_hstep<8, 1, 0, ., ., ., MDI = true> on every 32-frame tile of Tp, pad tiles included)
            snprintf(hs, sizeof hs, "k_hstep (MDI pass: 8 waves on 32-frame tiles, synchronous staging, V re-imputed in place; %d tiles)", g.Tp / 32);
        else
            snprintf(hs, sizeof hs, "k_hstep");
        break;
    }
    // (a masked plan launches its own pass: grid_mdi workgroups of 512 threads with lds_mdi, whatever the geometry's k_hstep is)
    const int grid = mdi ? g.grid_mdi : h == HUPD_SR ? g.sr_grid : h == HUPD_SF ? g.sf_grid : (h == HUPD_RH || h == HUPD_RP) ? g.rp_grid : g.grid_h;
    const int threads = (mdi || h == HUPD_SR || h == HUPD_SF) ? 512 : h == HUPD_RH ? 768 : (g.NWH + g.NLH) * 64;
    const size_t lds = mdi ? g.lds_mdi : h == HUPD_SR ? g.lds_sr : h == HUPD_SF ? g.lds_sf : h == HUPD_RH ? g.lds_rh : g.lds_h;
    const char* wkind = g.gram_p ? ", P = W*(H*H') through the Gram matrix"
                        : g.wsr  ? ", k_wstats_sr: statistics rows per wave, operands straight into the MFMA layouts"
                        : g.wsf  ? (g.wsf_share ? ", k_wstats_sf: a tile per wave, a single remainder tile shared by the eight waves" : ", k_wstats_sf: a tile per wave")
                        : g.til > 1 ? (g.til == 2 ? ", 2 consumer teams take the tiles in turn" : ", 4+ consumer teams take the tiles in turn")
                        : g.wxg_off ? ", extra row at the top of the tile (SNMF_WSTATS_XG=0)"
                                    : "";
    const char* wfinish = g.wfin    ? "k_wfin"
                          : g.upd_w ? "k_reduce + k_wapply"
                          : (g.fold_obj && !mdi) ? "none (objective fold + convergence test on the H step's last workgroup)"
                                                 : "none (objective fold + convergence test: k_reduce)";
    snprintf(buf, n,
             "F=%d T=%d r=%d beta=%g | Fm=%d(+%d VALU row) rp=%d Tp=%d | hstep: %s, tile=%d frames, grid=%d x %d thr, lds=%zu B | "
             "wstats: NK=%d waves=%d+%d grid=(%d chunks,%d fgroups,%d kgroups; group-1 chunks %d) lds=%zu B%s | W finish (run loop): %s | n_cu=%d",
             p.F, p.T, p.r, p.beta, g.Fm, g.xr, g.rp, g.Tp, hs, mdi ? 32 : g.TTH * g.NT, grid, threads, lds, g.NKT, g.NWB, g.NLW, g.n_chunks, g.n_fg,
             g.n_kg, g.n_ch1 ? g.n_ch1 : g.n_chunks, g.lds_w, wkind, wfinish, n_cu);
}

extern "C" int snmf_plan_geometry_describe(const snmf_params* p, int32_t n_cu, char* buf, size_t buflen) {
    if (!buf) return fail(SNMF_ERR_INVALID, "NULL argument");
    if (n_cu <= 0) return fail(SNMF_ERR_INVALID, "n_cu must be positive (got %d)", (int)n_cu);
    PlanGeometry g;
    SN_TRY(plan_geometry(p, n_cu, &g));
    describe_geometry(g, *p, n_cu, false, buf, buflen);
    return SNMF_OK;
}
