// esc_pod_compact.hip — the host runtime's fifth file (esc_ctx.h): esc_pods_compact, the pod
// side re-laid on the device, esc_pods_slack and esc_pod_where.
//
// The call runs in two halves so that a multi-device context can build every device's new K
// section before it swaps any.  compact_build: the K-holdable C slots are listed from the host
// mirrors and classified on the device (k_pc_classify; the first wait, only when there are
// any), the classes re-cut by plan_pod_compact (esc_pod_layout.h), every old K position and
// re-homed slot keyed and stable-sorted (k_pc_keys + the LSD passes), the new tiles gathered
// (k_pc_move) beside the resident ones and the old -> new map copied back; then the call's one
// wait, the error word and a read-only pass over the pod ids that checks the map against the
// mirrors.  compact_commit: the swap, the mirrors remapped in one threaded pass, the vacated C
// slots freed in place (k_pc_cfree), the other replicas copied, the K1 plan and the touch tables
// re-derived and the re-homed pods' PodRefs rewritten.
//
// Peak extra device memory, all released when the call returns: the new K array (kb_words * 4
// B), the map (4 B per old K position and candidate), the sort's two element arrays (2 x 8 B per
// old K position and candidate) and its histogram (<= 512 KB), the free-slot bitmap (1 bit per
// old K position) and the staged tables (the class tables, one free tile per class, the
// candidates' 12 B each).  The old K array is freed after the swap.
#include "esc_ctx.h"

using namespace esc;

namespace {

double pc_clock() {
    timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}
// The last esc_pods_compact of this thread (ms): 0 candidates + classify, 1 plan + buffers +
// staged upload, 2 keys + sort, 3 move kernel, 4 map download + the wait, 5 host check + remap,
// 6 C slots freed + other replicas, 7 work re-plan + touch + PodRefs; 8 the bytes the move
// kernel wrote, 9 (measurement library) a plain device-to-device copy of as many bytes of the
// OLD K array in the same call; 10 the sort's launches.  The product library has no wait between
// the kernels: there part 4 holds 2-4.
thread_local double g_pc_ms[12];

struct CompactJob {
    PodCompactPlan P;
    PodCompactDev D{};
    std::vector<uint32_t> cand;                   // K-holdable C slots, ascending
    std::vector<int32_t> cand_id, cand_cls;       // the device's class id, the plan's class index
    std::vector<uint32_t> map;                    // [old K slots + candidates] the device's map
    std::vector<int64_t> old_t0;                  // the old classes' first tiles
    int64_t nk_old = 0, old_kb_words = 0;
    esc_pods_compact_report rep{};
    // device
    uint32_t* new_kb = nullptr;
    PodClass* new_cls = nullptr;
    uint8_t *blob0 = nullptr, *blob = nullptr;
    uint32_t *d_map = nullptr, *hist = nullptr, *tot = nullptr;
    uint64_t* elems[2] = {nullptr, nullptr};
    ~CompactJob() {
        dfree(new_kb); dfree(new_cls); dfree(blob0); dfree(blob); dfree(d_map); dfree(hist); dfree(tot);
        dfree(elems[0]); dfree(elems[1]);
    }
};

int32_t compact_check(const esc_ctx* c) {
    if (!c) return ESC_E_INVAL;
    if (!c->has_device) return ESC_E_NODEV;
    if (!c->pods_loaded || c->stale || c->pods.empty()) return ESC_E_STATE;
    return ESC_OK;
}

// The K-holdable pods in C slots by the host's counts (c_slot_parked), ascending.
void parked_slots(const esc_ctx* c, std::vector<uint32_t>* out, int64_t* count) {
    const int64_t npad = c->c_tiles * CTILE;
    std::vector<char> fr((size_t)npad, 0);
    for (int64_t d : c->c_free) fr[(size_t)d] = 1;
    int64_t n = 0;
    for (int64_t d = 0; d < npad; ++d)
        if (!fr[(size_t)d] && c_slot_parked(c->h_cflags[d], c->h_cused[d])) {
            ++n;
            if (out) out->push_back((uint32_t)d);
        }
    if (count) *count = n;
}

// One pass over the pod ids with the device's map: checks it against the mirrors (apply false:
// every live K pod and every re-homed pod has a position inside its class's live range) or
// writes pod_cls / pod_pos (apply true).  moved: pods whose position or section changed;
// rehomed_ids: the pods that left the C section.
int32_t remap_pods(esc_ctx* c, CompactJob& J, bool apply, int64_t* moved, std::vector<int64_t>* rehomed_ids) {
    const int64_t n = (int64_t)c->pod_cls.size();
    const int T = n >= (1 << 16) ? host_threads() : 1;
    std::vector<int32_t> cand_of((size_t)(c->c_tiles * CTILE), -1);
    for (size_t j = 0; j < J.cand.size(); ++j) cand_of[J.cand[j]] = (int32_t)j;
    std::vector<int64_t> mv((size_t)T, 0), bad((size_t)T, 0);
    std::vector<std::vector<int64_t>> rh((size_t)T);
    par_chunks(n, T, [&](int t, int64_t lo, int64_t hi) {
        for (int64_t id = lo; id < hi; ++id) {
            const int32_t ci = c->pod_cls[id];
            if (ci == -2) continue;
            if (ci >= 0) {
                const int64_t q = c->pod_pos[id];
                const uint32_t nq = J.map[(size_t)(J.old_t0[ci] * TILE + q)];
                if (nq == NONE || (int64_t)nq >= J.P.live[ci]) { ++bad[t]; continue; }
                if ((int64_t)nq != q) ++mv[t];
                if (apply) c->pod_pos[id] = nq;
                continue;
            }
            const int32_t j = cand_of[(size_t)c->pod_pos[id]];
            if (j < 0 || J.cand_cls[j] < 0) continue;
            const uint32_t nq = J.map[(size_t)(J.nk_old + j)];
            if (nq == NONE || (int64_t)nq >= J.P.live[J.cand_cls[j]]) { ++bad[t]; continue; }
            ++mv[t];
            rh[t].push_back(id);
            if (apply) {
                c->pod_cls[id] = J.cand_cls[j];
                c->pod_pos[id] = nq;
            }
        }
    });
    int64_t m = 0, b = 0, r = 0;
    for (int t = 0; t < T; ++t) { m += mv[t]; b += bad[t]; r += (int64_t)rh[t].size(); }
    if (b || r != J.P.rehomed) return fail_fmt(ESC_E_HIP, "pods compact: the device's map does not fit the mirrors (%lld pods)", (long long)(b ? b : r - J.P.rehomed));
    if (moved) *moved = m;
    if (rehomed_ids)
        for (auto& v : rh) rehomed_ids->insert(rehomed_ids->end(), v.begin(), v.end());
    return ESC_OK;
}

int32_t compact_build(esc_ctx* c, CompactJob& J) {
    for (double& x : g_pc_ms) x = 0;
    double t0 = pc_clock();
    if (int32_t rc = compact_check(c)) return rc;
    hipSetDevice(c->device);
    HIP_TRY(hipStreamSynchronize(c->stream));
    hipStream_t st = c->stream;
    const PodBuf& old = c->pods[0];
    PodCompactDev& D = J.D;
    J.nk_old = c->k_tiles * TILE;
    J.old_kb_words = c->n_cls ? c->h_cls.back().kb0 + (c->h_cls.back().t1 - c->h_cls.back().t0) *
                                                           (int64_t)c->h_cls.back().wt * KB_UNIT : 0;
    for (const PodClass& k : c->h_cls) J.old_t0.push_back(k.t0);
    parked_slots(c, &J.cand, nullptr);
    const int64_t n_cand = (int64_t)J.cand.size(), n_el = J.nk_old + n_cand;
    const int64_t nbk = pod_buckets(c->pod_sort, c->gi.n_gp);
    if (n_el >= (int64_t)0xFFFFFFFF) return ESC_E_LIMIT;
    D.old = pod_dev(c, 0);
    D.old.seg = nullptr; D.old.wg_cols = nullptr; D.old.wg_off = nullptr;
    D.n_xc = c->h_xc_base[c->c_tiles];
    D.n_xp = c->h_xp_base[c->c_tiles];
    D.old_words = J.old_kb_words;
    D.n_cand = n_cand;
    D.n_gp = c->gi.n_gp;
    D.pod_sort = c->pod_sort;
    D.nbk = nbk;
    // ---- classify the candidates (the host cannot: it holds no pod's values or pairs)
    J.cand_id.assign((size_t)n_cand, -1);
    std::vector<int64_t> arr(POD_CLASS_IDS, 0);
    if (n_cand) {
        const size_t ids_at = ((size_t)n_cand * 4 + 255) & ~(size_t)255, used_at = 2 * ids_at, err_at = 3 * ids_at;
        std::vector<uint32_t> used((size_t)n_cand);
        for (int64_t j = 0; j < n_cand; ++j) used[(size_t)j] = c->h_cused[J.cand[(size_t)j]];
        HIP_TRY(dalloc(&J.blob0, err_at + 256));
        HIP_TRY(hipMemsetAsync(J.blob0, 0, err_at + 256, st));
        HIP_TRY(hipMemcpyAsync(J.blob0, J.cand.data(), (size_t)n_cand * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(J.blob0 + used_at, used.data(), (size_t)n_cand * 4, hipMemcpyHostToDevice, st));
        D.cand = reinterpret_cast<const uint32_t*>(J.blob0);
        D.cand_used = reinterpret_cast<const uint32_t*>(J.blob0 + used_at);
        D.cand_id = reinterpret_cast<int32_t*>(J.blob0 + ids_at);
        D.err = reinterpret_cast<uint32_t*>(J.blob0 + err_at);
        HIP_TRY(launch_pc_classify(D, st));
        uint32_t err = 0;
        HIP_TRY(hipMemcpyAsync(J.cand_id.data(), D.cand_id, (size_t)n_cand * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&err, D.err, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (err) return fail_fmt(ESC_E_HIP, "pods compact: a C slot lies outside the C arrays (%u)", err);
        for (int32_t& id : J.cand_id) {
            if (id >= POD_CLASS_IDS || (id >= 0 && !pod_class_holdable(id))) id = -1;
            if (id >= 0) ++arr[id];
        }
    }
    g_pc_ms[0] = (pc_clock() - t0) * 1e3;
    t0 = pc_clock();
    // ---- the plan
    std::vector<int64_t> k_free(c->h_cls.size());
    for (size_t i = 0; i < k_free.size(); ++i) k_free[i] = (int64_t)c->cls_free[i].size();
    PodCompactIn in;
    in.cls = &c->h_cls;
    in.cls_of = &c->h_cls_of;
    in.k_free = k_free.data();
    in.arr = arr.data();
    in.f = c->spare_frac;
    in.c_tiles = c->c_tiles;
    PodCompactPlan& P = J.P;
    if (int32_t rc = plan_pod_compact(P, in)) return rc;
    const int64_t n_cls = (int64_t)P.cls.size();
    if ((n_cls + 1) * nbk >= (int64_t)0xFFFFFFFF) return ESC_E_LIMIT;       // the sort's 32-bit keys
    J.cand_cls.assign((size_t)n_cand, -1);
    for (int64_t j = 0; j < n_cand; ++j)
        if (J.cand_id[j] >= 0) J.cand_cls[j] = P.cls_of[J.cand_id[j]];
    std::vector<uint32_t> free_bits((size_t)((J.nk_old + 31) / 32) + 1, 0);
    for (size_t i = 0; i < c->cls_free.size(); ++i)
        for (int64_t q : c->cls_free[i]) {
            const int64_t s = J.old_t0[i] * TILE + q;
            free_bits[(size_t)(s >> 5)] |= 1u << (s & 31);
        }
    J.rep.rehomed = P.rehomed;
    J.rep.classes_created = P.created;
    J.rep.k_tiles_before = P.tiles_before;
    J.rep.k_tiles_after = P.k_tiles;
    J.rep.k1_bytes_before = P.k1_bytes_before;
    J.rep.k1_bytes_after = P.k1_bytes_after;
    J.rep.c_free_before = (int64_t)c->c_free.size();
    J.rep.c_free_after = J.rep.c_free_before + P.rehomed;
    // ---- one staged copy: the candidates' classes, the class tables, the free tiles, the free
    // bitmap (the error word, zero, at its end)
    struct Part { const void* p; size_t bytes, at; };
    enum { S_CCLS, S_CLS, S_TAB, S_TMPL, S_FREE, S_N };
    Part parts[S_N] = {{J.cand_cls.data(), J.cand_cls.size() * 4, 0},
                       {P.cls.data(), P.cls.size() * sizeof(PodClass), 0},
                       {P.tab.data(), P.tab.size() * sizeof(PcCls), 0},
                       {P.tmpl.data(), P.tmpl.size() * 4, 0},
                       {free_bits.data(), free_bits.size() * 4, 0}};
    size_t bytes = 0;
    for (Part& q : parts) {
        q.at = bytes;
        bytes += (q.bytes + 255) & ~(size_t)255;
    }
    const size_t err_at = bytes;
    bytes += 256;
    std::vector<uint8_t> stage(bytes, 0);
    for (const Part& q : parts)
        if (q.bytes) std::memcpy(stage.data() + q.at, q.p, q.bytes);
    HIP_TRY(dalloc(&J.blob, bytes));
    HIP_TRY(dalloc(&J.new_kb, (size_t)std::max<int64_t>(P.kb_words, 4)));
    HIP_TRY(dalloc(&J.new_cls, (size_t)std::max<int64_t>(n_cls, 1)));
    HIP_TRY(dalloc(&J.d_map, (size_t)std::max<int64_t>(n_el, 1)));
    HIP_TRY(dalloc(&J.elems[0], (size_t)std::max<int64_t>(n_el, 1)));
    HIP_TRY(dalloc(&J.elems[1], (size_t)std::max<int64_t>(n_el, 1)));
    HIP_TRY(dalloc(&J.hist, std::max(sort_hist_words(std::max<int64_t>(n_el, 1)), sort_hist_words(1) * 4)));
    HIP_TRY(dalloc(&J.tot, 256));
    HIP_TRY(hipMemcpyAsync(J.blob, stage.data(), bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(J.d_map, 0xFF, (size_t)std::max<int64_t>(n_el, 1) * 4, st));
    if (n_cls) HIP_TRY(hipMemcpyAsync(J.new_cls, J.blob + parts[S_CLS].at, parts[S_CLS].bytes, hipMemcpyDeviceToDevice, st));
    D.cand_cls = reinterpret_cast<const int32_t*>(J.blob + parts[S_CCLS].at);
    D.cls = reinterpret_cast<const PodClass*>(J.blob + parts[S_CLS].at);
    D.tab = reinterpret_cast<const PcCls*>(J.blob + parts[S_TAB].at);
    D.tmpl = reinterpret_cast<const uint32_t*>(J.blob + parts[S_TMPL].at);
    D.tmpl_words = (int64_t)P.tmpl.size();
    D.free_bits = reinterpret_cast<const uint32_t*>(J.blob + parts[S_FREE].at);
    D.n_cls = (int32_t)n_cls;
    D.k_tiles = P.k_tiles;
    D.kb = J.new_kb;
    D.kb_words = P.kb_words;
    D.map_k = J.d_map;
    D.map_c = J.d_map + J.nk_old;
    D.err = reinterpret_cast<uint32_t*>(J.blob + err_at);
#if ESC_MEASURE
    HIP_TRY(hipStreamSynchronize(st));
#endif
    g_pc_ms[1] = (pc_clock() - t0) * 1e3;
    t0 = pc_clock();
    // ---- the order, the move
    const int key_bits = bit_width((uint64_t)(n_cls * nbk));
    int sorted = 0;
    HIP_TRY(launch_pc_order(D, J.elems, J.hist, J.tot, key_bits, &sorted, st));
    g_pc_ms[10] = 1 + 3 * (double)((std::max(key_bits, 1) + 7) / 8);
#if ESC_MEASURE
    HIP_TRY(hipStreamSynchronize(st));
    g_pc_ms[2] = (pc_clock() - t0) * 1e3;
    t0 = pc_clock();
#endif
    HIP_TRY(launch_pc_move(D, J.elems[sorted], st));
#if ESC_MEASURE
    HIP_TRY(hipStreamSynchronize(st));
    g_pc_ms[3] = (pc_clock() - t0) * 1e3;
    {                                                        // as many bytes of the old array by hipMemcpy
        const int64_t w = std::min(J.old_kb_words, P.kb_words);
        uint32_t* tmp = nullptr;
        if (w > 0 && dalloc(&tmp, (size_t)w) == hipSuccess) {
            t0 = pc_clock();
            hipMemcpyAsync(tmp, old.kb, (size_t)w * 4, hipMemcpyDeviceToDevice, st);
            hipStreamSynchronize(st);
            g_pc_ms[9] = (pc_clock() - t0) * 1e3;
            g_pc_ms[11] = (double)w * 4;
        }
        dfree(tmp);
    }
    t0 = pc_clock();
#endif
    (void)old;
    g_pc_ms[8] = (double)P.kb_words * 4;
    J.map.assign((size_t)std::max<int64_t>(n_el, 1), NONE);
    uint32_t err = 0;
    if (n_el) HIP_TRY(hipMemcpyAsync(J.map.data(), J.d_map, (size_t)n_el * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&err, D.err, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));                       // the call's one wait before the swap
    g_pc_ms[4] = (pc_clock() - t0) * 1e3;
    t0 = pc_clock();
    if (err) return fail_fmt(ESC_E_HIP, "pods compact: the snapshot does not fit the mirrors' plan (%u)", err);
#if ESC_MEASURE
    if (c->fail_compact > 0) {                               // injected (esc_debug_fail_compact)
        --c->fail_compact;
        return fail_fmt(ESC_E_HIP, "pods compact: injected failure before the swap");
    }
#endif
    if (int32_t rc = remap_pods(c, J, false, &J.rep.moved, nullptr)) return rc;
    g_pc_ms[5] = (pc_clock() - t0) * 1e3;
    return ESC_OK;
}

int32_t compact_commit(esc_ctx* c, CompactJob& J) {
    double t0 = pc_clock();
    hipSetDevice(c->device);
    hipStream_t st = c->stream;
    PodCompactPlan& P = J.P;
    PodBuf& b0 = c->pods[0];
    // ---- the swap: replica 0 and every mirror
    std::swap(b0.kb, J.new_kb);
    std::swap(b0.cls, J.new_cls);
    std::vector<int64_t> rehomed_ids;
    if (int32_t rc = remap_pods(c, J, true, nullptr, &rehomed_ids)) {   // (checked before the swap: never expected)
        c->stale |= STALE_PODS;
        return rc;
    }
    const size_t n_cls = P.cls.size();
    c->h_cls.swap(P.cls);
    c->h_cls_of.swap(P.cls_of);
    c->cls_free.assign(n_cls, {});
    for (size_t i = 0; i < n_cls; ++i)                       // as the load lists them: the lowest taken first
        for (int64_t q = P.k_free[i].second - 1; q >= P.k_free[i].first; --q) c->cls_free[i].push_back(q);
    c->k_tiles = P.k_tiles;
    c->k_weight = P.k_weight;
    c->n_cls = (int32_t)n_cls;
    for (int64_t j = (int64_t)J.cand.size() - 1; j >= 0; --j) {   // descending: the lowest slot is taken first again
        const int32_t ci = J.cand_cls[j];
        if (ci < 0) continue;
        const int64_t d = J.cand[j];
        c->live_xc -= c->h_cused[d] & 0xFFFF;
        c->live_xp -= c->h_cused[d] >> 16;
        c->h_cused[d] = 0;
        c->h_cflags[d] = c_slot_freed(c->h_cflags[d]);
        c->c_free.push_back(d);
        --c->live_c_pods;
        const PodClass& k = c->h_cls[ci];
        c->live_xc += kb_nrec(k);
        c->live_xp += k.nxp;
        if (k.packed) ++c->live_pk_pods;
        if (k.packed == 2) { ++c->live_p8_pods; c->live_p8_xp += k.nxp; }
        if (kb_inert(k)) { ++c->live_inert_pods; c->live_inert_xp += k.nxp; }
    }
    g_pc_ms[5] += (pc_clock() - t0) * 1e3;
    t0 = pc_clock();
    const bool had_work = c->work_ready;
    drop_graphs(c);
    c->sel_valid = c->rm_valid = c->tot_dec = false;
    // ---- after the swap a failure leaves replicas, C slots or the work set behind: stale, as a
    // failed pod event does
    const uint32_t was = c->stale;
    c->stale |= STALE_PODS;
    for (int r = 0; r < (int)c->pods.size(); ++r) {
        PodBuf& b = c->pods[r];
        if (r > 0) {
            dfree(b.kb);
            HIP_TRY(dalloc(&b.kb, (size_t)std::max<int64_t>(P.kb_words, 4)));
            if (P.kb_words) HIP_TRY(hipMemcpyAsync(b.kb, b0.kb, (size_t)P.kb_words * 4, hipMemcpyDeviceToDevice, st));
            dfree(b.cls);
            HIP_TRY(dalloc(&b.cls, std::max<size_t>(n_cls, 1)));
            if (n_cls) HIP_TRY(hipMemcpyAsync(b.cls, b0.cls, n_cls * sizeof(PodClass), hipMemcpyDeviceToDevice, st));
        }
        if (P.rehomed) HIP_TRY(launch_pc_cfree(J.D, b.flags, b.xc_cpu, b.xc_mem, b.xp, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    g_pc_ms[6] = (pc_clock() - t0) * 1e3;
    t0 = pc_clock();
    release_work(c);                                         // the K1 plan and the touch tables follow the tiles
    if (had_work)
        if (int32_t rc = ensure_work(c)) return rc;
    // a parked pod's PodRef named its C slot's pairs (a spare slot's room makes it indirect)
    if (c->placed && !rehomed_ids.empty())
        if (int32_t rc = refresh_podrefs(c, rehomed_ids)) return rc;
    g_pc_ms[7] = (pc_clock() - t0) * 1e3;
    c->stale = was;
    return ESC_OK;
}

void add_report(esc_pods_compact_report& a, const esc_pods_compact_report& b) {
    a.rehomed += b.rehomed; a.classes_created += b.classes_created;
    a.k_tiles_before += b.k_tiles_before; a.k_tiles_after += b.k_tiles_after;
    a.k1_bytes_before += b.k1_bytes_before; a.k1_bytes_after += b.k1_bytes_after;
    a.moved += b.moved; a.c_free_before += b.c_free_before; a.c_free_after += b.c_free_after;
}

}  // namespace

extern "C" {

int32_t esc_pods_compact(esc_ctx* c, esc_pods_compact_report* out) {
    esc_pods_compact_report rep{};
    if (c && c->multi) {
        size_t k = 0;                                            // one job per device context
        while (esc::multi_sub(c, (int)k)) ++k;
        std::vector<CompactJob> jobs(k);
        if (int32_t rc = esc::multi_pods_compact(
                c, jobs.data(), [](esc_ctx* s, int i, void* j) { return compact_build(s, static_cast<CompactJob*>(j)[i]); },
                [](esc_ctx* s, int i, void* j) { return compact_commit(s, static_cast<CompactJob*>(j)[i]); }))
            return rc;
        for (const CompactJob& j : jobs) add_report(rep, j.rep);
        if (out) *out = rep;
        return ESC_OK;
    }
    CompactJob J;
    if (int32_t rc = compact_build(c, J)) return rc;
    if (int32_t rc = compact_commit(c, J)) return rc;
    if (out) *out = J.rep;
    return ESC_OK;
}

int32_t esc_pods_slack(const esc_ctx* c, int64_t* k_tiles, int64_t* k_tiles_rule, int64_t* parked) {
    if (c && c->multi) return esc::multi_pods_slack(c, k_tiles, k_tiles_rule, parked);
    if (!c) return ESC_E_INVAL;
    if (!c->has_device) return ESC_E_NODEV;
    if (!c->pods_loaded || (c->stale & STALE_PODS)) return ESC_E_STATE;   // (stale: the mirrors may be half-written)
    if (k_tiles) *k_tiles = c->k_tiles;
    if (k_tiles_rule) {
        *k_tiles_rule = 0;
        for (size_t i = 0; i < c->h_cls.size(); ++i) {
            const int64_t live = (c->h_cls[i].t1 - c->h_cls[i].t0) * TILE - (int64_t)c->cls_free[i].size();
            *k_tiles_rule += (live + pod_spare(live, c->spare_frac) + TILE - 1) / TILE;
        }
    }
    if (parked) parked_slots(c, nullptr, parked);
    return ESC_OK;
}

int32_t esc_pod_where(const esc_ctx* c, int64_t id, int32_t* class_id, int64_t* pos) {
    if (c && c->multi) return esc::multi_pod_where(c, id, class_id, pos);
    if (!c || id < 0) return ESC_E_INVAL;
    if (!c->has_device) return ESC_E_NODEV;
    if (!c->pods_loaded) return ESC_E_STATE;
    int32_t cid = -2;
    int64_t q = -1;
    if (id < (int64_t)c->pod_cls.size() && c->pod_cls[id] != -2) {
        const int32_t ci = c->pod_cls[id];
        q = c->pod_pos[id];
        cid = -1;
        if (ci >= 0)
            for (int k = 0; k < POD_CLASS_IDS; ++k)
                if (c->h_cls_of[k] == ci) cid = k;
    }
    if (class_id) *class_id = cid;
    if (pos) *pos = q;
    return ESC_OK;
}

#if ESC_MEASURE
// The parts of this thread's last esc_pods_compact (g_pc_ms above), and the injected failure
// before the swap for the next n calls (measurement library only; not in the header;
// scripts/pods_compact_probe.py, tests/pods_compact_child.py).
int32_t esc_debug_pods_compact_times(double* ms, int32_t n) {
    if (!ms || n < 0) return ESC_E_INVAL;
    for (int32_t k = 0; k < n && k < 12; ++k) ms[k] = g_pc_ms[k];
    return ESC_OK;
}
int32_t esc_debug_fail_compact(esc_ctx* c, int32_t n) {
    if (!c || c->multi) return ESC_E_INVAL;
    c->fail_compact = std::max(0, n);
    return ESC_OK;
}
#endif

}  // extern "C"
