// gangfit_fifo_zoned_chain.inc — the LDS-resident chain kernel of the zone-aware tightly-pack packers, as text: gangfit_fifo_zoned.inc
// includes it once per narrow form, with
//   GF_ZONED_CHAIN_KERNEL   the kernel's name: fit_fifo_zoned_lds_kernel (exact form), fit_fifo_zoned_lds_floor_kernel (floored form)
//   GF_ZONED_CHAIN_FLOOR    false / true: the table holds floor(value / unit) and frem its remainders ([3][n_slots]; gangfit_floor_units.h)
// Text, not a template parameter or a shared body: the exact form's kernels are then compiled from the very lines they always were —
// as a body inlined into two kernels, the same lines came out with other spill counts in every instance (tools/kernel_resources.py).
// Every integer decision is the same on both forms; only the averages (wave_runs_avg_max) take the remainders in, and the
// residuals the epilogue writes are completed behind the kernel (floor_residual_kernel).  frem is not read by the exact form.
// RES: the whole table is in LDS (lds_slots >= n_slots, decided by the launcher).
template <bool AZ_AWARE, int NW, bool RES>
__global__ __launch_bounds__(kWave* NW) void GF_ZONED_CHAIN_KERNEL(
    NodeTable T, NarrowTable NT, ZoneTable Z, const int64_t* __restrict__ sched, uint32_t lds_slots, uint32_t n_apps,
    uint32_t n_shapes, const gf_app* __restrict__ apps, const NApp* __restrict__ napps,
    const int32_t* __restrict__ wide_needed,
    gf_result* __restrict__ results, uint32_t* __restrict__ exec_nodes, uint32_t* __restrict__ spill, uint64_t spill_stride,
    int32_t* __restrict__ chain_failed_at, ChainCkpt ck, ScanStats* __restrict__ stats, const int64_t* __restrict__ frem) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (*wide_needed) return;  // some request has no scaled form: fit_fifo_generic_kernel (guarded the other way) runs
    constexpr uint32_t BLOCK = kWave * NW;
    const uint32_t tid = threadIdx.x;
    const int lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t nc = T.n_chunks;
    const uint32_t n_zone_cand = Z.n_zones;
    const uint32_t n_cand = n_zone_cand + (AZ_AWARE ? 1u : 0u);  // host guarantees n_cand <= NW
    const uint32_t n_views = n_zone_cand + 1;                     // + the plain view (commit, az-aware candidate)

    // ---- LDS carve (ZonedLds, gangfit_chain_lds.h)
    const chain_lds::ZonedLds L = chain_lds::zoned_lds(lds_slots, nc, n_views, NW, n_shapes);
    lds_u8* stage = (lds_u8*)(smem + L.stage);    // gf_app [kZStage]
    lds_u8* nstage = (lds_u8*)(smem + L.nstage);  // NApp [kZStage]
    typedef __attribute__((address_space(3))) ZonedShared lds_zshared;  // typed: ds_* accesses, no flat/vmcnt waits
    lds_zshared* sh = (lds_zshared*)(smem + L.shared);
    lds_u64* lmasks = (lds_u64*)(smem + L.lmasks);  // [n_views][2][nc]: x then d
    lds_i32* lcm = (lds_i32*)(smem + L.lcm);
    lds_i32* lruns = (lds_i32*)(smem + L.lruns);    // [NW][2 = application parity][2][kZRunMax]: two lists per wavefront
    const uint32_t nw = (nc + 63u) / 64u;           // 64-bit words per shape row
    lds_u64* sbx = (lds_u64*)(smem + L.sbx);        // [n_views][n_shapes][nw] executor-shape index
    lds_u64* sbd = (lds_u64*)(smem + L.sbd);        // [n_views][n_shapes][nw] driver-shape index
    lds_i32* ltab = (lds_i32*)(smem + L.ltab);      // [3][lds_slots]

    // ---- stage tables
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
    for (uint32_t i = tid; i < n_views * n_shapes * nw; i += BLOCK) {  // every chunk may host every shape until a scan says otherwise
        const uint32_t word = i % nw;
        const uint32_t bits = nc - word * 64u;
        const uint64_t v = bits >= 64u ? ~0ull : ((1ull << bits) - 1ull);
        sbx[i] = v;
        sbd[i] = v;
    }
    for (uint32_t i = tid; i < 17 * kMaxShapes; i += BLOCK) sh->total_cap[i / kMaxShapes][i % kMaxShapes] = INT32_MAX;
    if (tid == 0) {
        sh->n_shape_x = 0;
        sh->n_shape_d = 0;
        sh->commit_done = 0;
    }
    __syncthreads();

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
    RunList R;
    const int64_t unit[3] = {NT.unit[0], NT.unit[1], NT.unit[2]};
    const bool tail_in_global = lds_slots < T.n_slots;
    // A wavefront without a candidate view expands the winner's runs to ExecutorNodes (stores only, nothing reads them in
    // this kernel) while the other wavefronts commit, stage and decide the next application.  It reads the winner's own
    // list: the lists alternate with the application's parity, so this one is not written again before the barrier of
    // the next application — which the helper only reaches when it is done.
    const uint32_t ew = n_cand < (uint32_t)NW ? n_cand : (uint32_t)NW;  // NW = none: the winner expands its own runs
    // ONE barrier per application for the zone views: every node sits in exactly one zone, so the winner's commit only
    // changes slots that the winner's own wavefront reads (program order), and the other views go straight on to the
    // next application.  The plain view of az-aware reads every slot: its wavefront waits for the helper's commit exactly as
    // the winner's does (commit_done); a second barrier for everybody only publishes the commit where there is no helper
    // (sixteen views) or the table has a global tail.
    const bool kCommitBarrier = AZ_AWARE && (tail_in_global || ew >= (uint32_t)NW);

    int32_t failed_at = -1;
    uint32_t a = 0;
    bool wait_commit = false;  // this wavefront won the previous application and the helper is subtracting its usage
    unsigned long long ph[6] = {0, 0, 0, 0, 0, 0};
    unsigned long long tph = stats != nullptr ? __builtin_readcyclecounter() : 0ull;
    const unsigned long long t0_cycles = tph;
    const unsigned long long t0_real = wall_clock64();
    for (; a < n_apps; ++a) {
        if ((a % kZStage) == 0) {  // refill the staged app records
            // without the commit barrier a wavefront may still be behind the previous application's decision barrier
            // (commit, expansion): nothing of the staging area or the shape rows is rewritten before it is here too
            if (!kCommitBarrier && a != 0) lds_barrier();
            const uint32_t n_stage = (n_apps - a) < (uint32_t)kZStage ? (n_apps - a) : (uint32_t)kZStage;
            const uint32_t words = n_stage * (uint32_t)(sizeof(gf_app) / 4);
            const uint32_t* gw = reinterpret_cast<const uint32_t*>(apps + a);
            const uint32_t* gn = reinterpret_cast<const uint32_t*>(napps + a);
            lds_u32* sw = (lds_u32*)stage;
            lds_u32* sn = (lds_u32*)nstage;
            for (uint32_t i = tid; i < words; i += BLOCK) {
                sw[i] = gw[i];
                sn[i] = gn[i];
            }
            __syncthreads();
            // checkpoint (ChainCkpt): every commit of the applications before `a` has been performed and published (the
            // barriers above), nothing commits before the barrier below — the other wavefronts dump the table meanwhile
            if (chain_ckpt_due(ck, a) && wave != 0) chain_ckpt_dump(plain, T.n_slots, chain_ckpt_slot(ck, a, T.n_slots), tid, BLOCK);
            if (wave == 0) {  // shape ids of the staged requests (NApp words 14 / 15 = {shape_x, shape_d})
                uint32_t nx = sh->n_shape_x, nd = sh->n_shape_d;
                zshapes_assign((lds_u32*)sn, n_stage, sh->shape_x, sh->shape_d, nx, nd, n_shapes, lane,
                               [&](bool drv, uint32_t id, int32_t v0, int32_t v1, int32_t v2) {
                                   zshape_rows_init(drv ? sbd : sbx, lmasks, lcm, nc, nw, n_views, n_shapes, id, drv, v0, v1, v2, lane);
                               });
                if (lane == 0) {
                    sh->n_shape_x = nx;
                    sh->n_shape_d = nd;
                }
            }
            __syncthreads();
        }
        // app records from LDS: the wide one for true quantities, the narrow one for the scaled decision
        gf_app w;
        {
            const lds_i64* rec = (const lds_i64*)(stage + (size_t)(a % kZStage) * sizeof(gf_app));
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
        NAppR app = read_staged_napp((const lds_u4*)(nstage + (size_t)(a % kZStage) * sizeof(NApp)));
        // what steers the control flow as scalars (every lane read the same record): tests on them are scalar compares, not a
        // vector compare handed over to a branch
        app.k = (int32_t)uniform32((uint32_t)app.k);
        app.flags = uniform32(app.flags);
        app.shape_x = uniform32(app.shape_x);
        app.shape_d = uniform32(app.shape_d);
        const int64_t K = app.k;
        const bool last = (a + 1 == n_apps);
        const uint32_t par = a & 1u;
        R.l_slot = lruns + ((size_t)wave * 2 + par) * 2 * kZRunMax;
        R.l_cnt = R.l_slot + kZRunMax;
        R.l_dummy = (lds_i32*)(smem + L.spare_words);  // shared by all views: nobody reads them
        R.g_slot = spill + (size_t)(2 * wave) * spill_stride + app.exec_off;
        R.g_cnt = spill + (size_t)(2 * wave + 1) * spill_stride + app.exec_off;

        GF_TICK(stats != nullptr, ph, tph, 0)
        if (wait_commit) {  // the helper's commit of the previous application ran next to this staging
            while (__hip_atomic_load(&sh->commit_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != a)
                __builtin_amdgcn_s_sleep(1);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            wait_commit = false;
        }
        // ---- one wavefront per candidate view: SparkBinPack (binpack.go:60-87) with tightly-pack, runs in LDS
        uint32_t my_nruns = 0, my_ds = 0, my_on_ds = 0;
        bool my_feasible = false;
        if (wave < n_cand) {
            const bool zone_view = wave < n_zone_cand;
            ZView ZV;
            ZV.V = zone_view ? view_of(wave) : plain;
            const uint32_t view = zone_view ? wave : n_zone_cand;
            ZV.xrow = app.shape_x != kNoShape ? sbx + ((size_t)view * n_shapes + app.shape_x) * nw : nullptr;
            ZV.drow = app.shape_d != kNoShape ? sbd + ((size_t)view * n_shapes + app.shape_d) * nw : nullptr;
            const NarrowHybridView& V = ZV.V;
            bool feasible = false;
            const bool indexed = app.shape_x != kNoShape;
            const bool hopeless = indexed && K > 0 && (int64_t)sh->total_cap[wave][app.shape_x] < K;
            const int64_t p0 = hopeless ? -1 : nwave_first_driver(ZV, T.n_d, app, lane);
            if (p0 >= 0) {
                my_ds = (uint32_t)p0;
                if (K == 0) {
                    feasible = true;
                } else {
                    const int64_t S_d = nwave_tight_runs(ZV, T.n_x, app, my_ds, R, my_nruns, my_on_ds, lane);
                    if (S_d >= K) {
                        feasible = true;
                    } else {  // the first fitting candidate's node is where the executors were needed (wave_fallback)
                        int64_t S = S_d;
                        if (my_ds < T.n_x && V.xcand(my_ds)) {
                            int32_t a0, a1, a2;
                            V.load32(my_ds, a0, a1, a2);
                            S = S_d + ncap3(a0, a1, a2, app) - ncap3(a0 - app.drv0, a1 - app.drv1, a2 - app.drv2, app);
                        }
                        if (S < K && indexed && lane == 0) sh->total_cap[wave][app.shape_x] = (int32_t)S;
                        if (S >= K) {
                            const int64_t p1 = nwave_next_feasible_driver(ZV, T.n_d, T.n_x, app, (uint32_t)p0 + 1, S, lane);
                            if (p1 >= 0) {
                                my_ds = (uint32_t)p1;
                                feasible = nwave_tight_runs(ZV, T.n_x, app, my_ds, R, my_nruns, my_on_ds, lane) >= K;
                            }
                        }
                    }
                }
            }
            GF_TICK(stats != nullptr, ph, tph, 1)
            double mx = 0.0, me = 0.0;
            my_feasible = feasible;
            if (feasible && zone_view) {
                if (my_nruns > kZRunMax) {  // spilled runs were written by other lanes of this wave
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                }
                mx = wave_runs_avg_max<true, false, GF_ZONED_CHAIN_FLOOR>(V, unit, sched, T.n_slots, w, my_ds, R, my_nruns, my_on_ds, lane, nullptr,
                                                                                  &me, frem);
            }
            if (lane == 0) {
                sh->feas[par][wave] = feasible ? 1 : 0;
                sh->ds[par][wave] = my_ds;
                sh->nruns[par][wave] = my_nruns;
                sh->mx[par][wave] = mx;
                sh->me[par][wave] = me;
            }
            if (feasible && my_nruns > kZRunMax && ew < (uint32_t)NW)  // spilled runs (global): the helper reads them
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        }
        GF_TICK(stats != nullptr, ph, tph, 2)
        lds_barrier();
        GF_TICK(stats != nullptr, ph, tph, 3)
        // ---- chooseBestResult (single_az.go:75-97), evaluated identically by every wave
        int32_t best;
        {
            int32_t f = 0;
            double m = 0.0, e = 0.0;
            if (lane < 16) {
                f = sh->feas[par][lane];
                m = sh->mx[par][lane];
                e = sh->me[par][lane];
            }
            best = zoned_choose_bounded(f, m, e, n_zone_cand, lane);
            if (GF_RARE(best == kChooseUndecided)) {
                // the bounds do not separate the candidates (ties between zones with equal nodes, an unbounded candidate): the
                // reference's own sums, one more barrier — every wavefront reaches the same verdict from the same published values
                if (wave < n_zone_cand && my_feasible) {
                    const NarrowHybridView VZ = view_of(wave);
                    const double mxe = wave_runs_avg_max<true, true, GF_ZONED_CHAIN_FLOOR>(VZ, unit, sched, T.n_slots, w, my_ds, R, my_nruns, my_on_ds,
                                                                                                    lane, nullptr, nullptr, frem);
                    if (lane == 0) sh->mxe[par][wave] = mxe;
                }
                lds_barrier();
                if (lane < 16) m = sh->mxe[par][lane];  // (only read where f says the candidate is feasible)
                best = zoned_choose_best(f, m, n_zone_cand, lane);
            }
            if (AZ_AWARE && best < 0 && read_lane(f, (int)n_zone_cand)) best = (int32_t)n_zone_cand;  // az_aware_pack_tightly.go:33-37
        }
        const bool feasible = best >= 0;
        bool stop = false;
        if (last) {
            stop = true;
        } else if (!feasible && !(app.flags & GF_APP_SKIPPABLE)) {  // resource.go:249-251
            failed_at = (int32_t)a;
            stop = true;
        }
        const bool defer = feasible && ew < (uint32_t)NW;  // the helper commits, stores the result and expands the runs
        if (wave == (feasible ? (uint32_t)best : 0u)) {
            // (with a helper the winner issues no global store at all: stores are acknowledged ~2 us later and the memory
            //  operations of a wavefront return in order — its next loads would queue behind them)
            if (!defer && lane == 0) {
                gf_result r;
                r.has_capacity = feasible ? 1 : 0;
                r.driver_node = feasible ? my_ds : GF_NO_NODE;  // SLOT id: zoned_translate_kernel maps it
                r.exec_len = feasible ? (uint32_t)K : 0u;
                r.evaluated = 1;
                results[a] = r;
            }
            if (defer) {
                wait_commit = !last;  // the helper commits (below) while this wavefront stages the next application
            } else if (feasible) {
                if (my_nruns > kZRunMax) {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                }
                // without a helper: commit the winner's usage (sparkpods.go:139-146) and expand its runs in the same walk
                uint32_t* dst = exec_nodes + app.exec_off;
                int64_t base = 0;
                bool driver_hosts_exec = false;
                for (uint32_t b = 0; b < my_nruns; b += kWave) {
                    const uint32_t i = b + lane;
                    uint32_t s = 0, c = 0;
                    if (i < my_nruns) R.load(i, s, c);
                    const int32_t incl = wave_inclusive_scan((int32_t)c);
                    emit_runs(dst, base + (int64_t)(incl - (int32_t)c), (int32_t)c, s, lane);  // SLOT ids
                    base += read_lane(incl, kWave - 1);
                    if (!last && c > 0) plain.sub32(s, app.exe0, app.exe1, app.exe2);
                    if (__ballot(c > 0 && s == my_ds)) driver_hosts_exec = true;
                }
                if (!last && !driver_hosts_exec && lane == 0) plain.sub32(my_ds, app.drv0, app.drv1, app.drv2);
                if (!kCommitBarrier && tail_in_global) {
                    // slots of the global tail were written by the lanes that hold their runs and are read back by lane
                    // (slot & 63) of this same wavefront in its next scan
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                }
            }
        }
        // az-aware without the second barrier: the plain view reads the winner's slots too, and when the PLAIN placement wins
        // (no single zone fits, az_aware_pack_tightly.go:33-37) its commit touches every zone's slots
        if (AZ_AWARE && !kCommitBarrier && defer && wave < n_cand && (wave == n_zone_cand || best == (int32_t)n_zone_cand))
            wait_commit = !last;
        RunList E;  // the winner's run list as the helper reads it
        uint32_t e_nruns = 0, e_ds = 0;
        if (defer && wave == ew) {
            e_nruns = sh->nruns[par][best];
            e_ds = sh->ds[par][best];
            E.l_slot = lruns + ((size_t)best * 2 + par) * 2 * kZRunMax;
            E.l_cnt = E.l_slot + kZRunMax;
            E.g_slot = spill + (size_t)(2 * best) * spill_stride + app.exec_off;  // the winner's spill area (per app: never reused)
            E.g_cnt = spill + (size_t)(2 * best + 1) * spill_stride + app.exec_off;
            if (e_nruns > kZRunMax) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            if (!last) {
                // commit the winner's usage (sparkpods.go:139-146): one executor request per distinct node, the driver request
                // only if no executor landed on the driver's node — before anything else, the winner's wavefront waits for it
                if (RES && e_nruns < (uint32_t)kWave) {
                    // The usual case in one pass without a masked-out lane or a read: lane i < e_nruns takes one executor
                    // request off its run's node, lane e_nruns the driver request off the driver's node unless a run sits
                    // there, the others nothing — as LDS atomics without a return value (a plain read-modify-write is a round
                    // trip, and lanes that must not write would have to be masked out).
                    const bool is_run = (uint32_t)lane < e_nruns;
                    const uint32_t i = is_run ? (uint32_t)lane : 0u;
                    uint32_t s2 = (uint32_t)E.l_slot[i];
                    const uint32_t c2 = (uint32_t)E.l_cnt[i];
                    const bool hosts = __ballot(is_run && c2 > 0 && s2 == e_ds) != 0;
                    const bool is_drv = (uint32_t)lane == e_nruns && !hosts;
                    s2 = is_run ? s2 : e_ds;
                    const bool hit = is_run && c2 > 0;
                    const int32_t q0 = hit ? app.exe0 : (is_drv ? app.drv0 : 0), q1 = hit ? app.exe1 : (is_drv ? app.drv1 : 0),
                                  q2 = hit ? app.exe2 : (is_drv ? app.drv2 : 0);
                    __hip_atomic_fetch_add(&plain.lcpu[s2], -q0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_add(&plain.lmem[s2], -q1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_add(&plain.lgpu[s2], -q2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                } else {
                    bool driver_hosts_exec = false;
                    for (uint32_t b = 0; b < e_nruns; b += kWave) {
                        const uint32_t i = b + lane;
                        uint32_t s2 = 0, c2 = 0;
                        if (i < e_nruns) E.load(i, s2, c2);
                        if (c2 > 0) plain.sub32(s2, app.exe0, app.exe1, app.exe2);
                        if (__ballot(c2 > 0 && s2 == e_ds)) driver_hosts_exec = true;
                    }
                    if (!driver_hosts_exec && lane == 0) plain.sub32(e_ds, app.drv0, app.drv1, app.drv2);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                if (lane == 0) __hip_atomic_store(&sh->commit_done, a + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        GF_TICK(stats != nullptr, ph, tph, 4)
        if (kCommitBarrier) {
            if (tail_in_global)
                __syncthreads();  // commits to the global tail of the table must be visible to the next app's scans
            else
                lds_barrier();
        }
        GF_TICK(stats != nullptr, ph, tph, 5)
        if (defer && wave == ew) {
            if (lane == 0) {
                gf_result r;
                r.has_capacity = 1;
                r.driver_node = e_ds;  // SLOT id: zoned_translate_kernel maps it
                r.exec_len = (uint32_t)K;
                r.evaluated = 1;
                results[a] = r;
            }
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
    chain_mark_not_evaluated<BLOCK>(results, a, n_apps, tid);
    __syncthreads();
    // residuals back to the wide working table (gf_residual_get reads it): value = scaled value * unit
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
    // wave 0: stage | decide | efficiency | barrier | select+emit+commit | barrier
    if (tid == 0 && stats != nullptr) chain_write_clocks(stats, t0_cycles, t0_real, ph);
}
