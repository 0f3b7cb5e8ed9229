// reuse_impl.hpp -- the driver of the reusing and recording steps (the plan itself: step_plan.hpp).  Included
// by pyipm_newton.hip in front of its factorisation driver: a kernel is launched from the unit that defines it.
#pragma once
static SchedOpts sched_opts(const Ctx* ctx) { return {ctx->group, ctx->tail_group, ctx->tail_group_user, ctx->skip_zeros != 0, ctx->lookahead, ctx->group_chain != 0}; }
// The PX_HDR doubles in front of the two snapshots by name.  First: the statistics at the boundary behind the prefix, the
// assembly's maximum.  Second: the record in front of the lambda_e groups (set aside there by a recording step), their own.
struct SnapHeaders { DevStats* at_boundary; unsigned long long* asm_max; DevStats* before_lam_e; DevStats* of_lam_e; };
static_assert(sizeof(DevStats) <= PX_HDR_SECOND * sizeof(double) && PX_HDR >= 2 * PX_HDR_SECOND, "a snapshot's header holds two records");
static SnapHeaders snap_headers(const Ctx* ctx) {
    double* const a = ctx->snap.get(); double* const b = ctx->snap_e.get();
    return SnapHeaders{(DevStats*)a, a ? (unsigned long long*)(a + PX_HDR_SECOND) : nullptr, (DevStats*)b, b ? (DevStats*)(b + PX_HDR_SECOND) : nullptr};
}
// the launches of the two copy kernels: dst[rows x cols] := src; the square behind column c0 of the storage to (save) or from B
static int copy_cols(Ctx* ctx, double* dst, int64_t ldd, const double* src, int64_t lds, int64_t rows, int64_t cols) {
    hipLaunchKernelGGL(k_copy_cols, dim3((unsigned)cols, (unsigned)((rows + 2047) / 2048)), dim3(256), 0, ctx->stream, dst, ldd, src, lds, rows, cols);
    PYIPM_KCHECK(); return 0;
}
static int copy_square(Ctx* ctx, double* B, int64_t c0, bool save) {
    const int64_t ne = ctx->g.Npad - c0;
    hipLaunchKernelGGL(k_copy_square, dim3((unsigned)ne, (unsigned)((ne + 2047) / 2048)), dim3(256), 0, ctx->stream, ctx->A, ctx->g.Npad, B, ne, c0, save ? 1 : 0);
    PYIPM_KCHECK(); return 0;
}
// The first snapshot, saved or restored along the plan's ranges (c_end > 0, restoring: only the columns in front of c_end)
static int prefix_copy(Ctx* ctx, const StepPlan& plan, bool save, int64_t c_end = 0) {
    const Geo& g = ctx->g;
    if (plan.snap_doubles > ctx->snap.capacity()) { ctx->err = "prefix snapshot: buffer too small"; return PYIPM_E_BADARG; }
    const SnapHeaders hdr = snap_headers(ctx); const hipMemcpyKind dd = hipMemcpyDeviceToDevice;
    if (save) {
        PYIPM_HIP(hipMemcpyAsync(hdr.at_boundary, ctx->dstats, sizeof(DevStats), dd, ctx->stream));
        PYIPM_HIP(hipMemcpyAsync(hdr.asm_max, ctx->anorm, sizeof(unsigned long long), dd, ctx->stream));
    } else {
        PYIPM_HIP(hipMemcpyAsync(ctx->anorm, hdr.asm_max, sizeof(unsigned long long), dd, ctx->stream));
    }
    for (int k = 0; k < plan.nranges; ++k) {
        const PxRange& r = plan.ranges[k];
        const int64_t rows = g.Npad - r.c0, cols = (c_end > 0 && c_end < r.c1 ? c_end : r.c1) - r.c0;
        if (cols <= 0) continue;
        double* a = ctx->A + r.c0 + r.c0 * g.Npad; double* b = ctx->snap.get() + r.off;     // (single rank: local = global columns)
        const int rc = save ? copy_cols(ctx, b, rows, a, g.Npad, rows, cols) : copy_cols(ctx, a, g.Npad, b, rows, rows, cols); if (rc) return rc;
    }
    return 0;
}
static double* lam_e_w(const Ctx* ctx, const LamE& e, int64_t c) { return ctx->snap_e.get() + PX_HDR + (c - e.cS) * (ctx->g.Npad - e.cE); }
static double* lam_e_square(const Ctx* ctx, const LamE& e) { return lam_e_w(ctx, e, e.cE); }
// K source columns from global column src_c0 on (L at Lop; -S at W, whose first row is global row w_row0 <= cE: row r of column
// k at W[(r - w_row0) + k ldw]) applied to the 128-row diagonal blocks of the columns [cE, Npad): k_update<64> (the instance of
// the narrow bulk launches) over a list of those tiles.  k_update addresses its W operand by global row; the address of "row 0"
// it is handed is computed on integers (a pointer in front of the buffer is never formed; no tile of the list reads there).
static int diag_update(Ctx* ctx, hipStream_t st, const double* Lop, const double* W, int64_t w_row0, int64_t ldw, int K, int64_t src_c0,
                       int64_t cE) {
    const double* const Wop = reinterpret_cast<const double*>(reinterpret_cast<uintptr_t>(W) - (uintptr_t)w_row0 * sizeof(double));
    const Geo& g = ctx->g; const int64_t nrt = (g.Npad - cE) / BM;
    if (nrt <= 0 || K <= 0) return 0;
    if (ctx->diag_tiles_n != nrt) {
        ctx->diag_tiles_host.clear();
        for (int64_t r = 0; r < nrt; ++r) for (int h = 0; h < BM / 64; ++h)
            ctx->diag_tiles_host.push_back((unsigned)r | ((unsigned)(r * (BM / 64) + h) << 16));
        PYIPM_HIP(ctx->diag_tiles.reserve(ctx->diag_tiles_host.size()));
        PYIPM_HIP(hipMemcpyAsync(ctx->diag_tiles.get(), ctx->diag_tiles_host.data(), ctx->diag_tiles_host.size() * sizeof(unsigned),
                                 hipMemcpyHostToDevice, st));
        ctx->diag_tiles_n = nrt;
    }
    UpdGeo u;
    u.row_begin = cE; u.Npad = g.Npad; u.first_lp = cE / g.nb; u.sub0 = 0;
    u.nb = g.nb; u.world = 1; u.rank = 0; u.nrt = (int)nrt; u.nct = (int)(nrt * (BM / 64));
    u.prio = 0; u.rt_min0 = 0; u.rt_step = 0; u.dbg = ctx->dbg_buf; u.ks_cstride = 0;
    active_ranges(ctx, src_c0, src_c0 + K, &u.a0, &u.a1, &u.b0, &u.b1);
    u.tiles = ctx->diag_tiles.get();
    hipLaunchKernelGGL((k_update<64, true, 8>), dim3((unsigned)ctx->diag_tiles_host.size()), dim3(512), 0, st, ctx->A, g.Npad, Lop, g.Npad,
                       Wop, ldw, K, u);
    PYIPM_KCHECK(); return 0;
}
// all columns of group grp (complete; L in the storage, -S at W as above) applied to those diagonal blocks, on the main stream
static int diag_update_group(Ctx* ctx, int64_t grp, const double* W, int64_t w_row0, int64_t ldw, int64_t cE) {
    const Geo& g = ctx->g;
    const int64_t p0 = ctx->sched.first(grp), p1 = ctx->sched.first(grp + 1) - 1, c0 = g.panel_c0(p0);
    return diag_update(ctx, ctx->stream, ctx->A + g.local_c0(p0) * g.Npad, W, w_row0, ldw, (int)(g.panel_c0(p1) + g.panel_w(p1) - c0), c0, cE);
}

// The plan of the step the fused entry point runs now.  Reuse applies to the full form on one rank with a lookahead schedule and
// at least one group inside the x block; everything else is a full step.
static StepPlan prefix_mode(Ctx* ctx, double delta, double delta_c) {
    const Geo& g = ctx->g; Held& h = ctx->held;
    if (!ctx->reuse_x || g.world != 1 || ctx->batched || ctx->provider_only || (ctx->condensed && g.mi > 0) || !ctx->lookahead ||
        h.storage_exported) return StepPlan();                 // (a holder of the storage pointer may write into the x columns at any time)
    const SchedOpts o = sched_opts(ctx); const GroupSched sc = plan_groups(g, o);
    auto plan = [&](int kind, bool lam_e) { return make_step_plan(g, sc, o, kind, lam_e, false, false); };
    const StepPlan rec = plan(PX_RECORD, ctx->reuse_lam_e != 0);
    if (rec.kind == PX_FULL) return rec;
    if (h.px_valid && delta == h.px_delta && delta_c == h.px_delta_c && rec.gB == h.px_rec.gB && rec.cB == h.px_rec.cB && ctx->snap)
        return plan(PX_REUSE, rec.e.ok && rec.e == h.px_rec.e && ctx->snap_e.capacity() >= rec.snap_e_doubles);
    // the first factorisation of these blocks records; a later one only with the shifts of the one before it (a shift loop
    // changes them every time and never gets as far as reusing)
    if (!h.px_record || (h.px_steps > 0 && (delta != h.px_last_delta || delta_c != h.px_last_delta_c))) return StepPlan();
    auto room = [&](DevBuf<double>& buf, size_t doubles) {           // is there room for a snapshot?  (a new buffer is poisoned on request)
        if (buf.capacity() >= doubles) return true;
        if (buf.reserve(doubles) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (getenv("PYIPM_POISON_WORKSPACE")) (void)hipMemsetAsync(buf, 0xFF, doubles * sizeof(double), ctx->stream);
        return true;
    };
    if (!room(ctx->snap, rec.snap_doubles)) { ctx->reuse_x = 0; return StepPlan(); }                 // none: the handle goes on without the feature
    if (rec.e.ok && !room(ctx->snap_e, rec.snap_e_doubles)) { ctx->reuse_lam_e = 0; return plan(PX_RECORD, false); }   // none for the second one: the first level alone
    return rec;
}
// The assembly of a reusing step (events 2 and 3 around it): the slack columns from the staged vectors, the rest from the snapshot;
// columns [0, cB) keep L of the prefix.  With the lambda_e groups kept: of the first snapshot the columns in front of cS and the
// diagonal blocks behind cE, of the second one everything else behind cE; the columns [cS, cE) keep L.
static int reassemble_slack(Ctx* ctx, const StepPlan& plan) {
    const Geo& g = ctx->g; const LamE& e = plan.e;
    PYIPM_HIP(hipEventRecord(ctx->ev[2], ctx->stream));
    int rc = prefix_copy(ctx, plan, false, e.ok ? e.cS : 0); if (rc) return rc;
    if (e.ok) {
        const PxRange* last = plan.nranges ? &plan.ranges[plan.nranges - 1] : nullptr;
        if (!last || last->c0 > e.cE || last->c1 != g.Npad) { ctx->err = "prefix snapshot: the lambda_i columns are not in its last range"; return PYIPM_E_BADARG; }
        const int64_t ne = g.Npad - e.cE, s0 = last->c0;
        hipLaunchKernelGGL(k_copy_diag_blocks, dim3((unsigned)ne), dim3(64), 0, ctx->stream, ctx->A, g.Npad,
                           (const double*)(ctx->snap.get() + last->off), g.Npad - s0, s0, e.cE, ne);
        PYIPM_KCHECK();
        rc = copy_square(ctx, lam_e_square(ctx, e), e.cE, false); if (rc) return rc;
    }
    if (g.mi > 0) {
        const int zip = (ctx->keep_zeros && !ctx->held.storage_exported && ctx->held.zeros_clean) ? 1 : 0;
        const int64_t lc0 = g.n / 16 * 16;
        const dim3 grid((unsigned)((g.Npad + 511) / 512), (unsigned)((g.n + g.mi - lc0 + 15) / 16));
        hipLaunchKernelGGL(k_assemble, grid, dim3(256), 0, ctx->stream, ctx->A, g.Npad, g, ctx->d2L, ctx->ld_d2L,
                           ctx->Je, ctx->ld_Je, ctx->Ji, ctx->ld_Ji, ctx->s, ctx->lda, ctx->eps, ctx->delta, ctx->delta_c, ctx->anorm, 0, 0,
                           zip, lc0, 0, g.n, g.n + g.mi);
        PYIPM_KCHECK();
    }
    PYIPM_HIP(hipEventRecord(ctx->ev[3], ctx->stream));
    ctx->held.prefix_reassembled(); ctx->held.assemble_timed();
    return 0;
}

// The assembly of a step or of pyipm_newton_assemble, with the decision what the factorisation behind it does (Held::plan).
// Every entry point that looks at the storage as a matrix in between completes a reusing assembly first (G_STORAGE, storage_whole).
int assemble_planned(Ctx* ctx, double delta, double delta_c) {
    if (!ctx->held.have_blocks || !ctx->held.have_vectors || ctx->provider_only) return assemble_timed(ctx, delta, delta_c);   // (its refusals)
    ctx->held.step_begun();
    const StepPlan plan = prefix_mode(ctx, delta, delta_c);
    const int rc = plan.kind == PX_REUSE ? reassemble_slack(ctx, plan) : assemble_timed(ctx, delta, delta_c); if (rc) return rc;
    ctx->held.assembly_planned(ctx->held.cond_active ? StepPlan() : plan);
    return 0;
}
// ... and its factorisation, with the bookkeeping of what was recorded or reused.
int factor_planned(Ctx* ctx, pyipm_factor_stats* stats, bool fuse) {
    const StepPlan plan = ctx->held.assembled ? ctx->held.plan : StepPlan();
    const double delta = ctx->delta, delta_c = ctx->delta_c;
    const int rc = factor_dispatch(ctx, stats, fuse, plan.kind);
    if (rc) { ctx->held.prefix_dropped(); ctx->held.plan = StepPlan(); return rc; }       // a failed factorisation: the next one runs in full
    ctx->held.step_factored(plan, delta, delta_c);
    ctx->last_step_kind = plan.kind; ctx->n_recorded += plan.kind == PX_RECORD; ctx->n_reused += plan.kind == PX_REUSE;
    return 0;
}
int storage_whole(Ctx* ctx) {
    if (ctx->held.partial()) { const int rc = assemble_timed(ctx, ctx->delta, ctx->delta_c); if (rc) return rc; }
    ctx->held.prefix_dropped();
    return 0;
}
