// gangfit_fifo_minfrag_chain.inc — the LDS-resident chain kernel of the minimal-fragmentation packers, as text: gangfit_fifo_minfrag.inc
// includes it once per narrow form, with
//   GF_MINFRAG_CHAIN_KERNEL   the kernel's name: fit_fifo_minfrag_lds_kernel (exact form), fit_fifo_minfrag_lds_floor_kernel (floored form)
//   GF_MINFRAG_CHAIN_FLOOR    false / true: the table holds floor(value / unit) and frem its remainders ([3][n_slots]; gangfit_floor_units.h)
// for the reason gangfit_fifo_zoned_chain.inc gives.  Only the zones' averages (ZONED) read frem: the launcher instantiates the
// floored kernel for ZONED = true alone, and plain minimal-fragmentation runs the exact form's kernel on the floored table.
// RES: the whole table is in LDS (lds_slots >= n_slots, decided by the launcher): the global-tail branch of every slot access
// compiles away (NarrowHybridView::resident).
template <bool ZONED, bool RES, int NWV>
__global__ __launch_bounds__(kWave* NWV) void GF_MINFRAG_CHAIN_KERNEL(
    NodeTable T, NarrowTable NT, ZoneTable Z, const int64_t* __restrict__ sched, uint32_t lds_slots, uint32_t n_apps,
    uint32_t n_shapes /* shape ids per role: rows of the capacity matrix */, uint32_t n_idx /* <= n_shapes: those with chunk-index rows in LDS */,
    const gf_app* __restrict__ apps, const NApp* __restrict__ napps,
    const int32_t* __restrict__ wide_needed, gf_result* __restrict__ results, uint32_t* __restrict__ exec_nodes,
    uint32_t* __restrict__ spill, uint64_t spill_stride, int32_t* __restrict__ chain_failed_at, int32_t* capmat,
    int32_t* hist /* [n_cand][n_shapes][kMfBins] counts, then the first-position table of the same shape (every row is written
                     in full when its shape's matrix row is filled); nullptr = block-cooperative passes only */,
    ChainCkpt ck, ScanStats* __restrict__ stats, const int64_t* __restrict__ frem) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (*wide_needed) return;  // some request has no scaled form: fit_fifo_generic_kernel (guarded the other way) runs
    constexpr uint32_t NW = NWV, BLOCK = kWave * NW;
    const uint32_t tid = threadIdx.x;
    const int lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t nc = T.n_chunks;
    const uint32_t n_zone_cand = ZONED ? Z.n_zones : 0u;
    const uint32_t n_cand = ZONED ? n_zone_cand : 1u;  // host guarantees n_cand <= 16
    const uint32_t n_views = n_zone_cand + 1;
    const size_t hist_words = (size_t)n_cand * n_shapes * kMfBins;  // the first-position table follows the histograms

    // ---- LDS carve
    size_t off = 0;
    lds_u8* stage = (lds_u8*)smem;
    off += (size_t)kMfStage * (sizeof(gf_app) + sizeof(NApp));
    lds_mfshared* sh = (lds_mfshared*)(smem + off);
    off += (sizeof(MfShared) + 15) & ~(size_t)15;
    lds_u64* lmasks = (lds_u64*)(smem + off);  // [n_views][2][nc]
    off += 16 * (size_t)nc * n_views;
    lds_i32* lcm = (lds_i32*)(smem + off);
    off += 12 * (size_t)nc;
    lds_i32* lruns = (lds_i32*)(smem + off);   // [n_cand][2 = application parity][2][kZRunMax]
    off += 2 * 8 * (size_t)kZRunMax * n_cand;
    lds_u32* chunk_cnt = (lds_u32*)(smem + off);
    off += 4 * (size_t)nc;
    lds_u32* chunk_pre = (lds_u32*)(smem + off);
    off += 4 * (size_t)nc;
    off = (off + 7) & ~(size_t)7;
    lds_u64* chunk_msk = (lds_u64*)(smem + off);
    off += 8 * (size_t)nc;
    lds_i32* fillh = (lds_i32*)(smem + off);  // [n_cand][2][256]: counts, first positions of the matrix row being filled
    off += 2048 * (size_t)n_cand;
    const uint32_t nw = (nc + 63u) / 64u;
    lds_u64* sbx = (lds_u64*)(smem + off);
    off += 8 * (size_t)n_views * n_idx * nw;
    lds_u64* sbd = (lds_u64*)(smem + off);
    off += 8 * (size_t)n_views * n_idx * nw;
    off = (off + 15) & ~(size_t)15;
    lds_i32* ltab = (lds_i32*)(smem + off);

    for (uint32_t i = tid; i < nc; i += BLOCK) {
        for (uint32_t v = 0; v < n_zone_cand; ++v) {
            lmasks[(size_t)(2 * v) * nc + i] = Z.xmask[(size_t)v * Z.stride + i];
            lmasks[(size_t)(2 * v + 1) * nc + i] = Z.dmask[(size_t)v * Z.stride + i];
        }
        lmasks[(size_t)(2 * n_zone_cand) * nc + i] = T.xmask[i];
        lmasks[(size_t)(2 * n_zone_cand + 1) * nc + i] = T.dmask[i];
        lcm[i] = NT.cmax[i];
        lcm[nc + i] = NT.cmax[nc + i];
        lcm[2 * nc + i] = NT.cmax[2 * (size_t)nc + i];
    }
    for (uint32_t s = tid; s < lds_slots; s += BLOCK) {
        ltab[s] = NT.cpu[s];
        ltab[lds_slots + s] = NT.mem[s];
        ltab[2 * lds_slots + s] = NT.gpu[s];
    }
    for (uint32_t i = tid; i < n_views * n_idx * nw; i += BLOCK) {
        const uint32_t word = i % nw;
        const uint32_t bits = nc - word * 64u;
        const uint64_t v = bits >= 64u ? ~0ull : ((1ull << bits) - 1ull);
        sbx[i] = v;
        sbd[i] = v;
    }
    for (uint32_t i = tid; i < 16 * kMaxShapes; i += BLOCK) sh->total_cap[i / kMaxShapes][i % kMaxShapes] = INT32_MAX;
    for (uint32_t i = tid; i < 512 * n_cand; i += BLOCK) fillh[i] = (i & 256u) ? kMfNoPos : 0;
    if (tid == 0) {
        sh->row_ready = 0ull;
        sh->row_big = 0ull;
    }
    if (tid == 0) {
        sh->n_shape_x = 0;
        sh->n_shape_d = 0;
        sh->pl_seq = 0xFFFFFFFFu;
        sh->pl_done = 0;
        sh->pl_target = 0;
    }
    __syncthreads();
    // the helper wavefronts of the histogram path: up to four that evaluate no candidate view (none with 16 candidates)
    const uint32_t hw = (hist != nullptr && capmat != nullptr && n_cand < NW) ? n_cand : NW;
    const uint32_t n_help = hw < NW ? ((NW - hw) < kMfHelpers ? (NW - hw) : kMfHelpers) : 0u;
    // ... and one more that writes the winner's result and expands its runs to ExecutorNodes behind the end-of-application
    // barrier: global stores are acknowledged ~2 us after they are issued and memory operations of a wavefront return in
    // order, so a winner that stored its own placement would find its next loads (histograms, matrix rows) queued behind
    // those stores.  The run lists alternate with the application's parity: the winner's next decision writes the other one.
    const uint32_t ewv = hw + n_help < NW ? hw + n_help : NW;  // NW = none: the winner stores its own placement

    auto view_of = [&](uint32_t v) {
        NarrowHybridView V;
        V.lcpu = ltab;
        V.lmem = ltab + lds_slots;
        V.lgpu = ltab + 2 * lds_slots;
        V.lds_slots = lds_slots;
        V.cpu = (glb_i32*)NT.cpu;
        V.mem = (glb_i32*)NT.mem;
        V.gpu = (glb_i32*)NT.gpu;
        V.cmax_cpu = lcm;
        V.cmax_mem = lcm + nc;
        V.cmax_gpu = lcm + 2 * nc;
        V.xm = lmasks + (size_t)(2 * v) * nc;
        V.dm = lmasks + (size_t)(2 * v + 1) * nc;
        V.n_chunks = nc;
        V.resident = RES;
        return V;
    };
    const NarrowHybridView plain = view_of(n_zone_cand);
    const int64_t unit[3] = {NT.unit[0], NT.unit[1], NT.unit[2]};
    const bool tail_in_global = lds_slots < T.n_slots;
    uint32_t xpar = 0;

    // The matrix / histogram patch of one commit, by one wavefront: lane = shape (every filled row); entry(i, slot, run) names
    // the i-th touched slot and whether it was a run's node (it lost one executor request e) or the lone driver's (it lost the
    // driver request d).  Every touched slot lies in `view` (the winner's zone; the plain view without zones).  The capacity a
    // slot had is recomputed from what the commit subtracted, not read back (a dependent L2 round trip per slot).
    auto patch_commit = [&](uint32_t view, uint32_t n, auto entry, int32_t e0, int32_t e1, int32_t e2, int32_t d0, int32_t d1,
                            int32_t d2) {
        const uint32_t nshape = sh->n_shape_x;
        const unsigned long long rdy = sh->row_ready, big = sh->row_big;
        const bool mine = (uint32_t)lane < nshape && ((rdy >> lane) & 1ull) != 0ull;
        NAppR q{};
        if (mine) {
            q.exe0 = sh->shape_x[lane][0];
            q.exe1 = sh->shape_x[lane][1];
            q.exe2 = sh->shape_x[lane][2];
            q.mag0 = sh->shape_xm[lane][0];
            q.mag1 = sh->shape_xm[lane][1];
            q.mag2 = sh->shape_xm[lane][2];
            q.msh = narrow_shift(q.exe0) | (narrow_shift(q.exe1) << 8) | (narrow_shift(q.exe2) << 16);
        }
        const bool hmine = mine && hist != nullptr && ((big >> lane) & 1ull) == 0ull;
        int32_t* hrow = hist != nullptr ? hist + ((size_t)view * n_shapes + (uint32_t)lane) * kMfBins : nullptr;
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t s;
            bool run;
            entry(i, s, run);  // wave-uniform
            int32_t a0, a1, a2;
            plain.load32(s, a0, a1, a2);
            const bool xc = s < T.n_x && plain.xcand(s);
            int32_t cap = 0;
            if (xc && nfits_exe(a0, a1, a2, q)) cap = ncap_full3(a0, a1, a2, q);
            if (hmine && xc) {
                const int32_t b0 = a0 + (run ? e0 : d0), b1 = a1 + (run ? e1 : d1), b2 = a2 + (run ? e2 : d2);
                int32_t old = 0;
                if (nfits_exe(b0, b1, b2, q)) old = ncap_full3(b0, b1, b2, q);
                if (old != cap) {  // capacities only fall: old < kMfBins covers cap
                    if (old > 0) __hip_atomic_fetch_add(&hrow[old], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (cap > 0) {
                        __hip_atomic_fetch_add(&hrow[cap], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_fetch_min(&hrow[hist_words + cap], (int32_t)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
            }
            if (mine) __hip_atomic_store(&capmat[(size_t)lane * T.n_slots + s], cap, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    };

    int32_t failed_at = -1;
    uint32_t a = 0;
    unsigned long long ph[6] = {0, 0, 0, 0, 0, 0};
    unsigned long long xvis = 0;  // slots the histogram path's walks looked at (this wavefront)
    unsigned long long tph = stats != nullptr ? __builtin_readcyclecounter() : 0ull;
    const unsigned long long t0_cycles = tph;
    const unsigned long long t0_real = wall_clock64();
    for (; a < n_apps; ++a) {
        if ((a % kMfStage) == 0) {
            const uint32_t n_stage = (n_apps - a) < (uint32_t)kMfStage ? (n_apps - a) : (uint32_t)kMfStage;
            const uint32_t words = n_stage * (uint32_t)(sizeof(gf_app) / 4);
            const uint32_t* gw = reinterpret_cast<const uint32_t*>(apps + a);
            const uint32_t* gn = reinterpret_cast<const uint32_t*>(napps + a);
            lds_u32* sw = (lds_u32*)stage;
            lds_u32* sn = (lds_u32*)(stage + (size_t)kMfStage * sizeof(gf_app));
            for (uint32_t i = tid; i < words; i += BLOCK) {
                sw[i] = gw[i];
                sn[i] = gn[i];
            }
            __syncthreads();
            // checkpoint (ChainCkpt): the TABLE before application a — every earlier commit ended before its application's
            // closing barrier; matrix rows, histograms and pending patches are derived state a resumed chain rebuilds
            if (chain_ckpt_due(ck, a) && wave != 0) chain_ckpt_dump(plain, T.n_slots, chain_ckpt_slot(ck, a, T.n_slots), tid, BLOCK);
            if (wave == 0) {
                uint32_t nx = sh->n_shape_x, nd = sh->n_shape_d;
                zshapes_assign((lds_u32*)sn, n_stage, sh->shape_x, sh->shape_d, nx, nd, n_shapes, lane,
                               [&](bool drv, uint32_t id, int32_t v0, int32_t v1, int32_t v2) {
                                   if (!drv) {  // the commit patch divides by every registered executor shape (lane = shape)
                                       uint32_t m0, m1, m2, l0, l1, l2;
                                       narrow_magic(v0, m0, l0);
                                       narrow_magic(v1, m1, l1);
                                       narrow_magic(v2, m2, l2);
                                       if (lane == 0) {
                                           sh->shape_xm[id][0] = m0;
                                           sh->shape_xm[id][1] = m1;
                                           sh->shape_xm[id][2] = m2;
                                       }
                                   }
                                   if (id < n_idx)
                                       zshape_rows_init(drv ? sbd : sbx, lmasks, lcm, nc, nw, n_views, n_idx, id, drv, v0, v1, v2, lane);
                               });
                if (lane == 0) {
                    sh->n_shape_x = nx;
                    sh->n_shape_d = nd;
                }
            }
            __syncthreads();
        }
        gf_app w;
        {
            const lds_i64* rec = (const lds_i64*)(stage + (size_t)(a % kMfStage) * sizeof(gf_app));
            w.drv[0] = rec[0];
            w.drv[1] = rec[1];
            w.drv[2] = rec[2];
            w.exe[0] = rec[3];
            w.exe[1] = rec[4];
            w.exe[2] = rec[5];
            const int64_t kf = rec[6];
            w.k = (int32_t)(uint32_t)kf;
            w.flags = (uint32_t)((uint64_t)kf >> 32);
            w.exec_off = (uint64_t)rec[7];
        }
        const NAppR app = read_staged_napp(
            (const lds_u4*)(stage + (size_t)kMfStage * sizeof(gf_app) + (size_t)(a % kMfStage) * sizeof(NApp)));
        const int64_t K = app.k;
        const bool last = (a + 1 == n_apps);
        const uint32_t par = a & 1u;

        // ---- the helper wavefront applies the patch the previous application's commit left behind
        if (wave >= hw && wave < hw + n_help && sh->pl_seq == a) {
            const uint32_t k = wave - hw, n = sh->pl_n;
            const uint32_t mine_n = n > k ? (n - k + n_help - 1) / n_help : 0u;  // entries k, k + n_help, ...
            if (mine_n != 0)
                patch_commit(sh->pl_view, mine_n, [&](uint32_t i, uint32_t& slot, bool& run) {
                    const uint32_t e = sh->pl_slot[k + i * n_help];
                    slot = e & 0x7FFFFFFFu;
                    run = (e >> 31) != 0;
                }, sh->pl_req[0], sh->pl_req[1], sh->pl_req[2], sh->pl_req[3], sh->pl_req[4], sh->pl_req[5]);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every store and atomic of the patch has been performed
            if (lane == 0) __hip_atomic_fetch_add((uint32_t*)&sh->pl_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        // ---- the capacity-matrix row of this executor shape: filled on first use (every slot of the plain executor order,
        //      nothing reserved), by all wavefronts
        const int32_t* caprow = nullptr;
        if (capmat != nullptr && app.shape_x != kNoShape) {
            int32_t* row = capmat + (size_t)app.shape_x * T.n_slots;
            if (((sh->row_ready >> (app.shape_x & 63u)) & 1ull) == 0ull) {  // workgroup-uniform
                for (uint32_t cc = wave; cc < nc; cc += NW) {
                    const uint32_t j = cc * kWave + (uint32_t)lane;
                    int32_t cap = 0;
                    if (j < T.n_x && ((plain.xm[cc] >> lane) & 1ull)) {
                        int32_t a0, a1, a2;
                        plain.load32(j, a0, a1, a2);
                        if (nfits_exe(a0, a1, a2, app)) cap = ncap_full3(a0, a1, a2, app);
                    }
                    if (j < T.n_slots) row[j] = cap;
                    if (hist != nullptr) {
                        // histogram + first positions of the candidate view that holds the slot, in LDS (one atomic per slot on
                        // the global bins would pile thousands onto the hot ones); written out below
                        if (__ballot(cap >= kMfBins) != 0) {
                            if (lane == 0) atomicOr((unsigned long long*)&sh->row_big, 1ull << (app.shape_x & 63u));
                            continue;
                        }
                        if (cap > 0) {
                            for (uint32_t v = 0; v < n_cand; ++v) {
                                const uint32_t view = ZONED ? v : n_zone_cand;
                                if ((lmasks[(size_t)(2 * view) * nc + cc] >> lane) & 1ull) {
                                    __hip_atomic_fetch_add(&fillh[512 * v + (uint32_t)cap], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                                    __hip_atomic_fetch_min(&fillh[512 * v + 256 + (uint32_t)cap], (int32_t)j, __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_WORKGROUP);
                                }
                            }
                        }
                    }
                }
                if (hist != nullptr) {
                    __syncthreads();
                    for (uint32_t i = tid; i < 512 * n_cand; i += BLOCK) {
                        const uint32_t v = i >> 9, bin = i & 255u;
                        const bool pos = (i & 256u) != 0;
                        hist[(pos ? hist_words : 0) + ((size_t)v * n_shapes + app.shape_x) * kMfBins + bin] = fillh[i];
                        fillh[i] = pos ? kMfNoPos : 0;  // ready for the next row
                    }
                }
                // the whole workgroup sits on one CU and shares its L1: workgroup scope orders these stores for every reader
                // (an agent-scope fence writes back and invalidates the XCD's L2 — every later load of the chain would miss)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __syncthreads();
                if (tid == 0) sh->row_ready |= 1ull << (app.shape_x & 63u);
                lds_barrier();
            }
            caprow = row;
        }
        GF_TICK(stats != nullptr, ph, tph, 0)
        // one wavefront per candidate view, from the histograms (workgroup-uniform)
        const bool use_hist = hist != nullptr && caprow != nullptr && ((sh->row_big >> (app.shape_x & 63u)) & 1ull) == 0ull;
        if (use_hist) {
            if (wave < n_cand) {
                const uint32_t c = wave;
                const uint32_t view = ZONED ? c : n_zone_cand;
                ZView ZV;
                ZV.V = view_of(view);
                ZV.xrow = app.shape_x < n_idx ? sbx + ((size_t)view * n_idx + app.shape_x) * nw : nullptr;
                ZV.drow = app.shape_d < n_idx ? sbd + ((size_t)view * n_idx + app.shape_d) * nw : nullptr;
                ZV.caprow = caprow;
                RunList R;
                R.l_slot = lruns + ((size_t)c * 2 + par) * 2 * kZRunMax;
                R.l_cnt = R.l_slot + kZRunMax;
                R.g_slot = spill + (size_t)(2 * c) * spill_stride + app.exec_off;
                R.g_cnt = spill + (size_t)(2 * c + 1) * spill_stride + app.exec_off;
                uint32_t ds = 0, nruns = 0;
                int32_t* hrow = hist + ((size_t)c * n_shapes + app.shape_x) * kMfBins;
                const bool feasible = mf_hist_decide(ZV, hrow, hrow + hist_words, T.n_d, T.n_x, app, R, sh, c, lane, ds, nruns, xvis,
                                                     sh->pl_seq == a && sh->pl_view == c);
                GF_TICK(stats != nullptr, ph, tph, 1)
                if (feasible && nruns > kZRunMax && ewv < NW)  // spilled runs (global stores): the emitting helper reads them
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                double mx = 0.0;
                if (ZONED && feasible) {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // the runs were stored by other lanes of this wave
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    mx = wave_runs_avg_max<false, true, GF_MINFRAG_CHAIN_FLOOR>(ZV.V, unit, sched, T.n_slots, w, ds, R, nruns, 0u, lane, nullptr,
                                                                                        nullptr, frem);
                }
                if (lane == 0) {
                    sh->feas[c] = feasible ? 1 : 0;
                    sh->ds[c] = ds;
                    sh->nruns[c] = nruns;
                    sh->mx[c] = mx;
                }
            }
        } else {
        // ---- the candidate views, one after the other, each by the whole workgroup.  Commits of the histogram path patch
        //      the matrix without a release (the committing wavefront is the only reader of what it writes there): publish them
        if (hist != nullptr) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __syncthreads();
        }
        for (uint32_t c = 0; c < n_cand; ++c) {
            const uint32_t view = ZONED ? c : n_zone_cand;
            ZView ZV;
            ZV.V = view_of(view);
            ZV.xrow = app.shape_x < n_idx ? sbx + ((size_t)view * n_idx + app.shape_x) * nw : nullptr;
            ZV.drow = app.shape_d < n_idx ? sbd + ((size_t)view * n_idx + app.shape_d) * nw : nullptr;
            ZV.caprow = caprow;
            RunList R;
            R.l_slot = lruns + ((size_t)c * 2 + par) * 2 * kZRunMax;
            R.l_cnt = R.l_slot + kZRunMax;
            R.g_slot = spill + (size_t)(2 * c) * spill_stride + app.exec_off;
            R.g_cnt = spill + (size_t)(2 * c + 1) * spill_stride + app.exec_off;
            uint32_t ds = 0, nruns = 0;
            const bool feasible = mf_block_decide<NWV>(ZV, T.n_d, T.n_x, nc, app, R, chunk_cnt, chunk_pre, chunk_msk, sh, c, wave, lane, tid,
                                                  xpar, ds, nruns);
            if (wave == 0) {
                if (feasible && nruns > kZRunMax && ewv < NW)  // thread 0's spilled runs: the emitting helper reads them
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                double mx = 0.0;
                if (ZONED && feasible) {
                    // the runs were stored by thread 0 (this wave) or published by the barriers of the level walk
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    mx = wave_runs_avg_max<false, true, GF_MINFRAG_CHAIN_FLOOR>(ZV.V, unit, sched, T.n_slots, w, ds, R, nruns, 0u, lane, nullptr,
                                                                                        nullptr, frem);
                }
                if (lane == 0) {
                    sh->feas[c] = feasible ? 1 : 0;
                    sh->ds[c] = ds;
                    sh->nruns[c] = nruns;
                    sh->mx[c] = mx;
                }
            }
        }
        }
        GF_TICK(stats != nullptr, ph, tph, 2)
        lds_barrier();
        GF_TICK(stats != nullptr, ph, tph, 3)
        // ---- chooseBestResult (single_az.go:75-97) / the plain result
        int32_t best;
        {
            int32_t f = 0;
            double m = 0.0;
            if (lane < 16) {
                f = sh->feas[lane];
                m = sh->mx[lane];
            }
            best = ZONED ? zoned_choose_best(f, m, n_cand, lane) : (read_lane(f, 0) ? 0 : -1);
        }
        const bool feasible = best >= 0;
        bool stop = false;
        if (last) {
            stop = true;
        } else if (!feasible && !(app.flags & GF_APP_SKIPPABLE)) {
            failed_at = (int32_t)a;
            stop = true;
        }
        // the histogram path: the winner's own wavefront emits, commits and patches — what it patches (matrix entries of
        // its zone's slots, its view's histograms and first positions) is read by no other wavefront of that path
        const bool defer = feasible && ewv < NW;  // the helper stores the result and the placement behind the barrier
        uint32_t e_ds = 0, e_nruns = 0;
        if (defer && wave == ewv) {  // (the next decisions overwrite these two)
            e_ds = sh->ds[best];
            e_nruns = sh->nruns[best];
        }
        if (wave == ((use_hist && feasible) ? (uint32_t)best : 0u)) {
            const uint32_t my_ds = feasible ? sh->ds[best] : 0u;
            const uint32_t my_nruns = feasible ? sh->nruns[best] : 0u;
            if (!defer && lane == 0) {
                gf_result r;
                r.has_capacity = feasible ? 1 : 0;
                r.driver_node = feasible ? my_ds : GF_NO_NODE;  // SLOT id: zoned_translate_kernel maps it
                r.exec_len = feasible ? (uint32_t)K : 0u;
                r.evaluated = 1;
                results[a] = r;
            }
            if (feasible) {
                RunList R;
                R.l_slot = lruns + ((size_t)best * 2 + par) * 2 * kZRunMax;
                R.l_cnt = R.l_slot + kZRunMax;
                R.g_slot = spill + (size_t)(2 * best) * spill_stride + app.exec_off;
                R.g_cnt = spill + (size_t)(2 * best + 1) * spill_stride + app.exec_off;
                if (my_nruns > kZRunMax) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                uint32_t* dst = exec_nodes + app.exec_off;
                int64_t base = 0;
                bool driver_hosts_exec = false;
                for (uint32_t b = 0; b < my_nruns; b += kWave) {
                    const uint32_t i = b + lane;
                    uint32_t s = 0, c = 0;
                    if (i < my_nruns) R.load(i, s, c);
                    if (!defer) {
                        const int32_t incl = wave_inclusive_scan((int32_t)c);
                        emit_runs(dst, base + (int64_t)(incl - (int32_t)c), (int32_t)c, s, lane);  // SLOT ids
                        base += read_lane(incl, kWave - 1);
                    }
                    if (!last && c > 0) plain.sub32(s, app.exe0, app.exe1, app.exe2);  // sparkpods.go:139-146
                    if (__ballot(c > 0 && s == my_ds)) driver_hosts_exec = true;
                }
                if (!last && !driver_hosts_exec && lane == 0) plain.sub32(my_ds, app.drv0, app.drv1, app.drv2);
                GF_TICK(stats != nullptr, ph, tph, 4)
                if (!last && capmat != nullptr) {
                    // the subtractions above are this wavefront's own LDS writes (in order); a workgroup fence here would also
                    // wait for the placement stores just issued
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    if (use_hist && hw < NW && my_nruns <= kZRunMax) {
                        // hand the patch to the helper wavefront: it runs next to the next application's staging and driver
                        // searches; only a decision on THIS view waits for it
                        for (uint32_t i = lane; i < my_nruns; i += kWave) {
                            uint32_t s2, c2;
                            R.load(i, s2, c2);
                            sh->pl_slot[i] = s2 | 0x80000000u;
                        }
                        if (lane == 0) {
                            uint32_t n = my_nruns;
                            if (!driver_hosts_exec) sh->pl_slot[n++] = my_ds;
                            sh->pl_n = n;
                            sh->pl_view = (uint32_t)best;
                            sh->pl_req[0] = app.exe0;
                            sh->pl_req[1] = app.exe1;
                            sh->pl_req[2] = app.exe2;
                            sh->pl_req[3] = app.drv0;
                            sh->pl_req[4] = app.drv1;
                            sh->pl_req[5] = app.drv2;
                            sh->pl_target += n_help;  // every helper reports, with or without a slot of its own
                            sh->pl_seq = a + 1;
                        }
                    } else {
                        const uint32_t n = my_nruns + (driver_hosts_exec ? 0u : 1u);
                        patch_commit((uint32_t)best, n, [&](uint32_t i, uint32_t& slot, bool& run) {
                            uint32_t c2 = 1;
                            slot = my_ds;
                            run = i < my_nruns;
                            if (run) R.load(i, slot, c2);  // wave-uniform index: broadcast reads
                        }, app.exe0, app.exe1, app.exe2, app.drv0, app.drv1, app.drv2);
                        if (!use_hist) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // for every wavefront's loads
                    }
                }
            }
        }
        if (tail_in_global)
            __syncthreads();
        else
            lds_barrier();
        GF_TICK(stats != nullptr, ph, tph, 5)
        if (defer && wave == ewv) {
            if (lane == 0) {
                gf_result r;
                r.has_capacity = 1;
                r.driver_node = e_ds;  // SLOT id: zoned_translate_kernel maps it
                r.exec_len = (uint32_t)K;
                r.evaluated = 1;
                results[a] = r;
            }
            RunList E;
            E.l_slot = lruns + ((size_t)best * 2 + par) * 2 * kZRunMax;
            E.l_cnt = E.l_slot + kZRunMax;
            E.g_slot = spill + (size_t)(2 * best) * spill_stride + app.exec_off;  // per application: never reused
            E.g_cnt = spill + (size_t)(2 * best + 1) * spill_stride + app.exec_off;
            if (e_nruns > kZRunMax) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            uint32_t* dst = exec_nodes + app.exec_off;
            int64_t base = 0;
            for (uint32_t b = 0; b < e_nruns; b += kWave) {
                const uint32_t i = b + lane;
                uint32_t s2 = 0, c2 = 0;
                if (i < e_nruns) E.load(i, s2, c2);
                const int32_t incl = wave_inclusive_scan((int32_t)c2);
                emit_runs(dst, base + (int64_t)(incl - (int32_t)c2), (int32_t)c2, s2, lane);  // SLOT ids
                base += read_lane(incl, kWave - 1);
            }
        }
        if (stop) {
            ++a;
            break;
        }
    }
    if (tid == 0 && stats != nullptr) {  // wave 0: stage + row fill | decide | efficiency | barrier | select + emit + commit | patch + barrier
        stats->fifo_shader_cycles = __builtin_readcyclecounter() - t0_cycles;
        stats->fifo_realtime_ticks = wall_clock64() - t0_real;
        for (int i = 0; i < 6; ++i) stats->fifo_phase_cycles[i] = ph[i];
    }
    if (lane == 0 && stats != nullptr && xvis != 0) atomicAdd(&stats->exec_slots_visited, xvis);
    chain_mark_not_evaluated<BLOCK>(results, a, n_apps, tid);
    __syncthreads();
    const bool tip = RES && ck.tip != nullptr;  // (ChainCkpt::tip: the table this chain ended with, for the next Filter)
    for (uint32_t s = tid; s + 1 < T.n_slots; s += BLOCK) {
        int32_t b0, b1, b2;
        plain.load32(s, b0, b1, b2);
        T.cpu[s] = (int64_t)b0 * unit[0];
        T.mem[s] = (int64_t)b1 * unit[1];
        T.gpu[s] = (int64_t)b2 * unit[2];
        if (tip) chain_tip_store(ck, T.n_slots, s, b0, b1, b2);
    }
    if (tip && tid == 0) {  // the sentinel slot, as the snapshot has it (the loop above leaves it out)
        int32_t b0, b1, b2;
        plain.load32(T.n_slots - 1u, b0, b1, b2);
        chain_tip_store(ck, T.n_slots, T.n_slots - 1u, b0, b1, b2);
    }
    if (tid == 0 && chain_failed_at != nullptr) *chain_failed_at = failed_at;
}
