// esc_pod_grow.hip — the host runtime's fourth file (esc_ctx.h): esc_pods_grow, the pod classes
// grown on the device when they fill, and esc_pods_room.
//
// The plan is the host's alone (plan_pod_grow, esc_pod_layout.h, from the class table, the free
// counts and the batch's arrivals: no pass over the pods).  The new replica 0 is built beside
// the resident one — the K blocks by k_kb_regrow, the C arrays by device-to-device copies of the
// old prefix and the staged tail — and swapped in after the call's one wait; the other replicas
// are then copied from it and the K1 plan and touch tables re-derived.  Pod ids, classes,
// positions, the placement and the occupancy words stay as they are.
#include "esc_ctx.h"

using namespace esc;

namespace {

double grow_clock() {
    timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}
// The last esc_pods_grow of this thread (ms): host plan, buffers + staged upload, k_kb_regrow to
// the wait, the C copies to the call's wait, other replicas, work re-plan + touch; then the bytes
// k_kb_regrow wrote and (measurement library) the ms of a plain device-to-device copy of the OLD K
// array made in the same call, for the probe's comparison.  The product library has no wait
// between the kernel and the C copies: there part 2 holds both and part 3 is 0.
thread_local double g_grow_ms[8];

// The buffers a grow builds beside replica 0; after the swap they hold the old ones.  Released
// on every way out.
struct GrowBufs {
    PodBuf b;
    uint8_t* blob = nullptr;
    ~GrowBufs() {
        b.release();
        dfree(blob);
    }
};

// The checks of esc_pods_grow and its plan; nothing is touched.
int32_t grow_plan(esc_ctx* c, const int64_t* ids, const esc_pod_soa* p, PodGrowPlan& P) {
    if (!c) return ESC_E_INVAL;
    const int64_t n = p ? p->n_pods : 0;
    if (n < 0 || (n > 0 && (!ids || !p->flags || !p->cpu0 || !p->mem0 || !p->pair0))) return ESC_E_INVAL;
    if (!c->has_device) return ESC_E_NODEV;
    if (!c->pods_loaded || c->stale) return ESC_E_STATE;
    // the batch classified as upsert_plan does (batch_shape, k_needs_pos, c_keeps_slot);
    // departures are not credited, as there
    std::vector<int64_t> arr(POD_CLASS_IDS, 0);
    int64_t arr_c = 0;
    if (n > 0) {
        BatchShape sh;
        if (int32_t rc = batch_shape(c, ids, p, sh)) return rc;
        for (int64_t i = 0; i < n; ++i) {
            const int sid = sh.sid[i];
            const uint32_t f = p->flags[i];
            if (sid >= 0) {
                const int ci = c->h_cls_of[sid];
                if (ci < 0 || k_needs_pos(c, ids[i], ci)) ++arr[sid];
                continue;
            }
            if (c_keeps_slot(c, ids[i], f)) continue;
            if (!c_room(CS_FLAGS, f)) return ESC_E_LIMIT;    // no spare slot holds it: a reload, as before
            ++arr_c;
        }
    }
    std::vector<int64_t> k_free(c->h_cls.size());
    for (size_t i = 0; i < k_free.size(); ++i) k_free[i] = (int64_t)c->cls_free[i].size();
    PodGrowIn in;
    in.cls = &c->h_cls;
    in.cls_of = &c->h_cls_of;
    in.k_free = k_free.data();
    in.arr = arr.data();
    in.f = c->spare_frac;
    in.c_tiles = c->c_tiles;
    in.live_c = c->live_c_pods;
    in.arr_c = arr_c;
    for (int64_t d : c->c_free) in.free_cs += c_room(c->h_cflags[d], CS_FLAGS) ? 1 : 0;
    in.xc_end = c->h_xc_base[c->c_tiles];
    in.xp_end = c->h_xp_base[c->c_tiles];
    return plan_pod_grow(P, in);
}

// Frees, re-allocates and fills from replica 0 the buffers of replica r that a grow changed.
int32_t grow_replica(esc_ctx* c, int r, const PodGrowPlan& P, int64_t npad, int64_t nxc, int64_t nxp) {
    const PodBuf& a = c->pods[0];
    PodBuf& b = c->pods[r];
    auto remake = [&](auto*& dst, const auto* src, int64_t count) -> hipError_t {
        using T = std::remove_pointer_t<std::remove_reference_t<decltype(dst)>>;
        dfree(dst);
        if (hipError_t e = dalloc(&dst, (size_t)std::max<int64_t>(count, 1)); e != hipSuccess) return e;
        return count ? hipMemcpyAsync(dst, src, (size_t)count * sizeof(T), hipMemcpyDeviceToDevice, c->stream) : hipSuccess;
    };
    if (P.k_changed) {
        dfree(b.kb);
        HIP_TRY(dalloc(&b.kb, (size_t)std::max<int64_t>(P.kb_words, 4)));
        if (P.kb_words) HIP_TRY(hipMemcpyAsync(b.kb, a.kb, (size_t)P.kb_words * 4, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(remake(b.cls, a.cls, (int64_t)c->h_cls.size()));   // (the swap took the plan's table)
    }
    if (P.c_changed) {
        HIP_TRY(remake(b.flags, a.flags, npad)); HIP_TRY(remake(b.cpu0, a.cpu0, npad));
        HIP_TRY(remake(b.mem0, a.mem0, npad)); HIP_TRY(remake(b.pair0, a.pair0, npad));
        HIP_TRY(remake(b.xc_cpu, a.xc_cpu, nxc)); HIP_TRY(remake(b.xc_mem, a.xc_mem, nxc));
        HIP_TRY(remake(b.xp, a.xp, nxp));
        HIP_TRY(remake(b.xc_base, a.xc_base, P.c_tiles + 1)); HIP_TRY(remake(b.xp_base, a.xp_base, P.c_tiles + 1));
    }
    return ESC_OK;
}

int32_t grow_one(esc_ctx* c, PodGrowPlan& P, double t0) {
    for (double& x : g_grow_ms) x = 0;
    if (!P.k_changed && !P.c_changed) return ESC_OK;          // room enough already
    if (c->pods.empty()) return ESC_E_STATE;
    hipSetDevice(c->device);
    HIP_TRY(hipStreamSynchronize(c->stream));
    hipStream_t st = c->stream;
    const PodBuf& old = c->pods[0];
    const int64_t old_kb_words = c->n_cls ? c->h_cls.back().kb0 + (c->h_cls.back().t1 - c->h_cls.back().t0) *
                                                                       (int64_t)c->h_cls.back().wt * KB_UNIT : 0;
    const int64_t npad0 = c->c_tiles * CTILE, npad = P.c_tiles * CTILE;
    const int64_t xc_end = c->h_xc_base[c->c_tiles], xp_end = c->h_xp_base[c->c_tiles];
    const int64_t nxc = xc_end + (int64_t)P.xc_cpu.size(), nxp = xp_end + (int64_t)P.xp.size();
    std::vector<uint32_t> xc_base(c->h_xc_base), xp_base(c->h_xp_base);
    xc_base.insert(xc_base.end(), P.xc_base.begin(), P.xc_base.end());
    xp_base.insert(xp_base.end(), P.xp_base.begin(), P.xp_base.end());
    // ---- one staged copy: the regrow table, the templates, the class table, the C tail (the
    // error word, zero, at its end)
    struct Part { const void* p; size_t bytes, at; };
    enum { S_TAB, S_TMPL, S_CLS, S_FLAGS, S_CPU0, S_MEM0, S_PAIR0, S_XCC, S_XCM, S_XP, S_XCB, S_XPB, S_N };
    Part parts[S_N] = {{P.moves.data(), P.moves.size() * sizeof(KbRegrowCls), 0},
                       {P.tmpl.data(), P.tmpl.size() * 4, 0},
                       {P.cls.data(), P.cls.size() * sizeof(PodClass), 0},
                       {P.c_flags.data(), P.c_flags.size() * 4, 0},
                       {P.c_cpu0.data(), P.c_cpu0.size() * 4, 0},
                       {P.c_mem0.data(), P.c_mem0.size() * 8, 0},
                       {P.c_pair0.data(), P.c_pair0.size() * 4, 0},
                       {P.xc_cpu.data(), P.xc_cpu.size() * 8, 0},
                       {P.xc_mem.data(), P.xc_mem.size() * 8, 0},
                       {P.xp.data(), P.xp.size() * 4, 0},
                       {xc_base.data(), xc_base.size() * 4, 0},
                       {xp_base.data(), xp_base.size() * 4, 0}};
    size_t bytes = 0;
    for (int k = 0; k < S_N; ++k) {
        if (!P.k_changed && k <= S_CLS) parts[k].bytes = 0;
        if (!P.c_changed && k >= S_FLAGS) parts[k].bytes = 0;
        parts[k].at = bytes;
        bytes += (parts[k].bytes + 255) & ~(size_t)255;
    }
    const size_t err_at = bytes;
    bytes += 256;
    std::vector<uint8_t> stage(bytes, 0);
    for (const Part& q : parts)
        if (q.bytes) std::memcpy(stage.data() + q.at, q.p, q.bytes);
    g_grow_ms[0] = (grow_clock() - t0) * 1e3;
    t0 = grow_clock();
    // ---- the new replica 0, beside the resident one
    GrowBufs B;
    PodBuf& nb = B.b;
    HIP_TRY(dalloc(&B.blob, bytes));
    if (P.k_changed) {
        HIP_TRY(dalloc(&nb.kb, (size_t)std::max<int64_t>(P.kb_words, 4)));
        HIP_TRY(dalloc(&nb.cls, P.cls.size()));
    }
    if (P.c_changed) {
        HIP_TRY(dalloc(&nb.flags, (size_t)npad)); HIP_TRY(dalloc(&nb.cpu0, (size_t)npad));
        HIP_TRY(dalloc(&nb.mem0, (size_t)npad)); HIP_TRY(dalloc(&nb.pair0, (size_t)npad));
        HIP_TRY(dalloc(&nb.xc_cpu, (size_t)nxc)); HIP_TRY(dalloc(&nb.xc_mem, (size_t)nxc));
        HIP_TRY(dalloc(&nb.xp, (size_t)nxp));
        HIP_TRY(dalloc(&nb.xc_base, (size_t)P.c_tiles + 1)); HIP_TRY(dalloc(&nb.xp_base, (size_t)P.c_tiles + 1));
    }
    HIP_TRY(hipMemcpyAsync(B.blob, stage.data(), bytes, hipMemcpyHostToDevice, st));
#if ESC_MEASURE
    HIP_TRY(hipStreamSynchronize(st));                       // (the probe's split: the upload's end)
#endif
    g_grow_ms[1] = (grow_clock() - t0) * 1e3;
    t0 = grow_clock();
    uint32_t* d_err = reinterpret_cast<uint32_t*>(B.blob + err_at);
    auto staged = [&](void* dst, int k) -> hipError_t {      // a staged table to its own buffer
        return parts[k].bytes ? hipMemcpyAsync(dst, B.blob + parts[k].at, parts[k].bytes, hipMemcpyDeviceToDevice, st)
                              : hipSuccess;
    };
    // ---- the K blocks to their new tile ranges
    if (P.k_changed) {
        KbRegrow R{};
        R.old_kb = old.kb;
        R.tmpl = reinterpret_cast<const uint32_t*>(B.blob + parts[S_TMPL].at);
        R.new_kb = nb.kb;
        R.tab = reinterpret_cast<const KbRegrowCls*>(B.blob + parts[S_TAB].at);
        R.old_words = old_kb_words;
        R.tmpl_words = (int64_t)P.tmpl.size();
        R.new_words = P.kb_words;
        R.n_cls = (int32_t)P.moves.size();
        R.err = d_err;
        HIP_TRY(launch_kb_regrow(R, P.k_tiles, st));
        HIP_TRY(staged(nb.cls, S_CLS));
    }
#if ESC_MEASURE
    HIP_TRY(hipStreamSynchronize(st));                       // (the probe's split: the kernel's end)
    g_grow_ms[2] = (grow_clock() - t0) * 1e3;
    if (P.k_changed && old_kb_words > 0) {                   // the same old array by hipMemcpy, into scratch
        uint32_t* tmp = nullptr;
        if (dalloc(&tmp, (size_t)old_kb_words) == hipSuccess) {
            t0 = grow_clock();
            hipMemcpyAsync(tmp, old.kb, (size_t)old_kb_words * 4, hipMemcpyDeviceToDevice, st);
            hipStreamSynchronize(st);
            g_grow_ms[7] = (grow_clock() - t0) * 1e3;
        }
        dfree(tmp);
    }
    t0 = grow_clock();
#endif
    g_grow_ms[6] = P.k_changed ? (double)P.kb_words * 4 : 0;
    // ---- the C arrays: the old prefix device to device, the tail from the staged arrays
    if (P.c_changed) {
        auto prefix = [&](void* dst, const void* src, int64_t count, int width) -> hipError_t {
            return count ? hipMemcpyAsync(dst, src, (size_t)count * width, hipMemcpyDeviceToDevice, st) : hipSuccess;
        };
        HIP_TRY(prefix(nb.flags, old.flags, npad0, 4)); HIP_TRY(prefix(nb.cpu0, old.cpu0, npad0, 4));
        HIP_TRY(prefix(nb.mem0, old.mem0, npad0, 8)); HIP_TRY(prefix(nb.pair0, old.pair0, npad0, 4));
        HIP_TRY(prefix(nb.xc_cpu, old.xc_cpu, xc_end, 8)); HIP_TRY(prefix(nb.xc_mem, old.xc_mem, xc_end, 8));
        HIP_TRY(prefix(nb.xp, old.xp, xp_end, 4));
        HIP_TRY(staged(nb.flags + npad0, S_FLAGS)); HIP_TRY(staged(nb.cpu0 + npad0, S_CPU0));
        HIP_TRY(staged(nb.mem0 + npad0, S_MEM0)); HIP_TRY(staged(nb.pair0 + npad0, S_PAIR0));
        HIP_TRY(staged(nb.xc_cpu + xc_end, S_XCC)); HIP_TRY(staged(nb.xc_mem + xc_end, S_XCM));
        HIP_TRY(staged(nb.xp + xp_end, S_XP));
        HIP_TRY(staged(nb.xc_base, S_XCB)); HIP_TRY(staged(nb.xp_base, S_XPB));
    }
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));                       // the call's one wait before the swap
    if (err) return fail_fmt(ESC_E_HIP, "pods grow: the K blocks do not fit the mirrors' plan (%u)", err);
#if ESC_MEASURE
    g_grow_ms[3] = (grow_clock() - t0) * 1e3;
    if (c->fail_grow > 0) {                                  // injected (esc_debug_fail_grow)
        --c->fail_grow;
        return fail_fmt(ESC_E_HIP, "pods grow: injected failure before the swap");
    }
#else
    g_grow_ms[2] = (grow_clock() - t0) * 1e3;
#endif
    t0 = grow_clock();
    // ---- the swap: replica 0 and every mirror
    PodBuf& b0 = c->pods[0];
    if (P.k_changed) {
        std::swap(b0.kb, nb.kb); std::swap(b0.cls, nb.cls);
        const size_t n_cls = P.cls.size();
        c->cls_free.resize(n_cls);
        for (size_t i = 0; i < n_cls; ++i) {
            const auto [lo, hi] = P.k_new[i];
            if (hi <= lo) continue;
            // old free positions keep priority (taken from the back); the new ones follow, ascending
            std::vector<int64_t> fr;
            fr.reserve((size_t)(hi - lo) + c->cls_free[i].size());
            for (int64_t q = hi - 1; q >= lo; --q) fr.push_back(q);
            fr.insert(fr.end(), c->cls_free[i].begin(), c->cls_free[i].end());
            c->cls_free[i].swap(fr);
        }
        c->h_cls.swap(P.cls);
        c->h_cls_of.swap(P.cls_of);
        c->k_tiles = P.k_tiles;
        c->k_weight = P.k_weight;
        c->n_cls = (int32_t)n_cls;
    }
    if (P.c_changed) {
        std::swap(b0.flags, nb.flags); std::swap(b0.cpu0, nb.cpu0); std::swap(b0.mem0, nb.mem0);
        std::swap(b0.pair0, nb.pair0); std::swap(b0.xc_cpu, nb.xc_cpu); std::swap(b0.xc_mem, nb.xc_mem);
        std::swap(b0.xp, nb.xp); std::swap(b0.xc_base, nb.xc_base); std::swap(b0.xp_base, nb.xp_base);
        c->h_cflags.insert(c->h_cflags.end(), P.c_flags.begin(), P.c_flags.end());
        c->h_cused.resize((size_t)npad, 0);
        c->h_xc_base.swap(xc_base);
        c->h_xp_base.swap(xp_base);
        // the old free slots keep priority (taken from the back); the new ones follow, ascending
        std::vector<int64_t> fr(P.c_free.rbegin(), P.c_free.rend());
        fr.insert(fr.end(), c->c_free.begin(), c->c_free.end());
        c->c_free.swap(fr);
        c->c_tiles = P.c_tiles;
    }
    const bool had_work = c->work_ready;
    drop_graphs(c);
    c->sel_valid = c->rm_valid = c->tot_dec = false;
    // ---- after the swap a failure leaves replicas or the work set behind: stale, as a failed
    // pod event does
    const uint32_t was = c->stale;
    c->stale |= STALE_PODS;
    for (int r = 1; r < (int)c->pods.size(); ++r)
        if (int32_t rc = grow_replica(c, r, P, npad, nxc, nxp)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    g_grow_ms[4] = (grow_clock() - t0) * 1e3;
    t0 = grow_clock();
    release_work(c);                                         // the K1 plan and the touch tables follow the tiles
    if (had_work)
        if (int32_t rc = ensure_work(c)) return rc;
    g_grow_ms[5] = (grow_clock() - t0) * 1e3;
    c->stale = was;
    return ESC_OK;
}

}  // namespace

namespace esc {
int32_t pods_grow_check(esc_ctx* c, const int64_t* ids, const esc_pod_soa* p) {
    PodGrowPlan P;
    return grow_plan(c, ids, p, P);
}
}  // namespace esc

extern "C" {

int32_t esc_pods_grow(esc_ctx* c, const int64_t* ids, const esc_pod_soa* p) {
    if (c && c->multi) return esc::multi_pods_grow(c, ids, p);
    const double t0 = grow_clock();
    PodGrowPlan P;
    if (int32_t rc = grow_plan(c, ids, p, P)) return rc;
    return grow_one(c, P, t0);
}

int32_t esc_pods_room(const esc_ctx* c, int64_t* k_capacity, int64_t* k_free, int64_t* c_free, int64_t* per_class) {
    if (c && c->multi) {
        int64_t cap = 0, kf = 0, cf = 0;
        if (per_class) std::fill(per_class, per_class + POD_CLASS_IDS, (int64_t)-1);
        std::vector<int64_t> pc(POD_CLASS_IDS);
        for (int i = 0; esc::multi_sub(c, i); ++i) {
            int64_t a = 0, b = 0, d = 0;
            if (int32_t rc = esc_pods_room(esc::multi_sub(c, i), &a, &b, &d, pc.data())) return rc;
            cap += a; kf += b; cf += d;
            if (per_class)
                for (int id = 0; id < POD_CLASS_IDS; ++id)
                    if (pc[id] >= 0) per_class[id] = std::max<int64_t>(per_class[id], 0) + pc[id];
        }
        if (k_capacity) *k_capacity = cap;
        if (k_free) *k_free = kf;
        if (c_free) *c_free = cf;
        return ESC_OK;
    }
    if (!c) return ESC_E_INVAL;
    if (!c->has_device) return ESC_E_NODEV;
    if (!c->pods_loaded) return ESC_E_STATE;
    if (k_capacity) *k_capacity = c->k_tiles * TILE;
    if (k_free) {
        *k_free = 0;
        for (const auto& fr : c->cls_free) *k_free += (int64_t)fr.size();
    }
    if (c_free) *c_free = (int64_t)c->c_free.size();
    if (per_class)
        for (int id = 0; id < POD_CLASS_IDS; ++id)
            per_class[id] = c->h_cls_of[id] < 0 ? -1 : (int64_t)c->cls_free[c->h_cls_of[id]].size();
    return ESC_OK;
}

#if ESC_MEASURE
// The parts of this thread's last esc_pods_grow (ms; g_grow_ms above), and the injected failure
// before the swap for the next n calls (measurement library only; not in the header;
// scripts/pods_grow_probe.py, tests/pods_grow_child.py).
int32_t esc_debug_grow_times(double* ms, int32_t n) {
    if (!ms || n < 0) return ESC_E_INVAL;
    for (int32_t k = 0; k < n && k < 8; ++k) ms[k] = g_grow_ms[k];
    return ESC_OK;
}
int32_t esc_debug_fail_grow(esc_ctx* c, int32_t n) {
    if (!c || c->multi) return ESC_E_INVAL;
    c->fail_grow = std::max(0, n);
    return ESC_OK;
}
#endif

}  // extern "C"
