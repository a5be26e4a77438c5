// esc_pod_audit.hip — the host runtime's sixth file (esc_ctx.h): esc_audit_pods, the read-only
// audit of the resident pod side, and the measurement library's
// esc_debug_poke_pods.
//
// Every check is uploads and kernels on the context's stream and one report read back at the
// call's last wait.  The host tables (the id map, the free-slot bitmap, the C mirrors, the run
// table, the run positions' slots) go up in bounded chunks through the context's pinned staging
// buffer, two halves of PSTAGE_HALF bytes used in turn: a half is refilled only after the copy
// and the kernels that read its last chunk are done (an event per half), so a table that fits
// one half costs no wait of its own.  Device scratch: one chunk buffer per half, the two slot
// bitmaps and the host's class table; all freed on every way out.
#include "esc_ctx.h"

using namespace esc;

namespace {

#if ESC_MEASURE
// This thread's last REPLICA pass (measurement library: scripts/pod_audit_probe.py turns them
// into a bandwidth): the bytes of one replica it compared (each is read from two replicas) and
// the time between an event in front of its first launch and one behind its last.
thread_local int64_t g_paud_replica_bytes = 0;
thread_local float g_paud_replica_ms = 0;
#endif
void paud_bad(esc_audit_check& k, int64_t id) {
    ++k.n_bad;
    if (k.first_bad < 0 || id < k.first_bad) k.first_bad = id;
}

int64_t kb_words_of(const esc_ctx* c) {
    int64_t w = 0;
    for (const PodClass& k : c->h_cls) w = std::max(w, k.kb0 + (k.t1 - k.t0) * (int64_t)k.wt * KB_UNIT);
    return w;
}

// COUNT: the nine live counters from the class table, the free lists' lengths and the C slots'
// counts (the order is the header's).
void audit_count(const esc_ctx* c, esc_audit_check& x) {
    int64_t v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < c->h_cls.size(); ++i) {
        const PodClass& k = c->h_cls[i];
        const int64_t live = (k.t1 - k.t0) * TILE - (i < c->cls_free.size() ? (int64_t)c->cls_free[i].size() : 0);
        v[0] += live;
        v[2] += live * (int64_t)kb_nrec(k);
        v[3] += live * (int64_t)k.nxp;
        if (k.packed) v[4] += live;
        if (k.packed == 2) { v[5] += live; v[6] += live * (int64_t)k.nxp; }
        if (kb_inert(k)) { v[7] += live; v[8] += live * (int64_t)k.nxp; }
    }
    int64_t c_live = -(int64_t)c->c_free.size();             // the C slots with room, less the free ones
    for (size_t d = 0; d < c->h_cflags.size(); ++d) {
        if (c->h_cflags[d] != ESC_PF_DAEMONSET) ++c_live;
        if (d < c->h_cused.size()) { v[2] += c->h_cused[d] & 0xFFFF; v[3] += c->h_cused[d] >> 16; }
    }
    v[0] += c_live;
    v[1] = c_live;
    const int64_t have[9] = {c->live_pods, c->live_c_pods, c->live_xc, c->live_xp, c->live_pk_pods,
                             c->live_p8_pods, c->live_p8_xp, c->live_inert_pods, c->live_inert_xp};
    x.n_checked = 9;
    for (int k = 0; k < 9; ++k)
        if (v[k] != have[k]) paud_bad(x, k);
}

int32_t audit_pods_one(esc_ctx* c, uint32_t checks, esc_pod_audit_report* out) {
    if (!c || !out || (checks >> ESC_PAUD_N)) return ESC_E_INVAL;
    if (!c->has_device) return ESC_E_NODEV;
    if (!c->pods_loaded || c->stale || c->pods.empty()) return ESC_E_STATE;
    if (!checks) checks = (1u << ESC_PAUD_N) - 1;
    std::memset(out, 0, sizeof *out);
    for (esc_audit_check& k : out->check) k.first_bad = -1;
    uint32_t skip = 0;
    if (!c->placed || !c->d_refs || !c->d_nrun_off || !c->d_nrun_len) skip |= 1u << ESC_PAUD_PODREF;
    if (c->pods.size() < 2) skip |= 1u << ESC_PAUD_REPLICA;
    out->skipped = checks & skip;
    out->ran = checks & ~skip;
    const uint32_t run = out->ran;
    auto on = [&](int k) { return (run >> k) & 1u; };
    esc_audit_check host[ESC_PAUD_N];                        // what the host finds, merged at the end
    for (esc_audit_check& k : host) k = esc_audit_check{0, 0, -1};
    if (on(ESC_PAUD_COUNT)) audit_count(c, host[ESC_PAUD_COUNT]);

    hipSetDevice(c->device);
    hipStream_t st = c->stream;
    if (int32_t rc = pstage_ensure(c)) return rc;
    const int64_t n_cls = (int64_t)c->h_cls.size(), kt = c->k_tiles, ct = c->c_tiles, npad = ct * CTILE;
    const int64_t kslots = kt * TILE, n_slots = kslots + npad;
    // The sizes every offset is compared with are the host's, cut to the device allocations' own
    // (the host's mirrors are under suspicion too): a host size past its allocation is a mismatch
    // of the check that reads the array, and nothing is read past the allocation.
    const PodBuf& b0 = c->pods[0];
    const int64_t ct_dev = std::min({dev_bytes_from(b0.flags) / 4 / CTILE, dev_bytes_from(b0.cpu0) / 4 / CTILE,
                                     dev_bytes_from(b0.pair0) / 4 / CTILE, dev_bytes_from(b0.mem0) / 8 / CTILE,
                                     dev_bytes_from(b0.xc_base) / 4 - 1, dev_bytes_from(b0.xp_base) / 4 - 1});
    const bool c_ok = (int64_t)c->h_cflags.size() == npad && (int64_t)c->h_cused.size() == npad &&
                      (int64_t)c->h_xc_base.size() == ct + 1 && (int64_t)c->h_xp_base.size() == ct + 1 && ct_dev >= ct;
    PodAuditScratch S;
#if ESC_MEASURE
    struct Timers {                                          // REPLICA's event pair, destroyed on every way out
        hipEvent_t e[2] = {nullptr, nullptr};
        ~Timers() { for (hipEvent_t x : e) if (x) hipEventDestroy(x); }
        hipEvent_t& operator[](int i) { return e[i]; }
    } rt;
#endif
    Stager G{c, st};
    PodAuditDev A{};
    A.P = pod_dev(c, 0);
    A.P.seg = nullptr; A.P.wg_cols = nullptr; A.P.wg_off = nullptr;
    A.P.c_tiles = std::min(ct, std::max<int64_t>(ct_dev, 0));
    A.P.n_cls = (int32_t)std::min<int64_t>(c->n_cls, dev_bytes_from(b0.cls) / (int64_t)sizeof(PodClass));
    A.kb_words = std::min(kb_words_of(c), dev_bytes_from(b0.kb) / 4);
    A.n_xc = c_ok ? std::min<int64_t>({(int64_t)c->h_xc_base[ct], dev_bytes_from(b0.xc_cpu) / 8, dev_bytes_from(b0.xc_mem) / 8}) : 0;
    A.n_xp = c_ok ? std::min<int64_t>((int64_t)c->h_xp_base[ct], dev_bytes_from(b0.xp) / 4) : 0;
    if (A.kb_words < kb_words_of(c) || A.P.n_cls < c->n_cls) paud_bad(host[ESC_PAUD_KSLOT], 0);
    if (c_ok && (A.n_xc < (int64_t)c->h_xc_base[ct] || A.n_xp < (int64_t)c->h_xp_base[ct])) paud_bad(host[ESC_PAUD_CSLOT], 0);
    A.n_slots = n_slots;
    A.n_gp = c->gi.n_gp;
    int64_t* h_rep = reinterpret_cast<int64_t*>(c->h_pstage + 2 * PSTAGE_HALF);
    for (int k = 0; k < ESC_PAUD_N; ++k) {
        h_rep[k * AW_K + AW_CHECKED] = h_rep[k * AW_K + AW_BAD] = 0;
        h_rep[k * AW_K + AW_FIRST] = INT64_MAX;
    }
    HIP_TRY(S.get(&A.rep, (size_t)ESC_PAUD_N * AW_K));
    HIP_TRY(hipMemcpyAsync(A.rep, h_rep, (size_t)ESC_PAUD_N * AW_K * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(S.get(&G.dev[0], PSTAGE_HALF));
    HIP_TRY(S.get(&G.dev[1], PSTAGE_HALF));
    // (the report words above left the pinned buffer before its next write: the same stream,
    // and they are rewritten only by the download behind every kernel)

    // ---- the host's class table and the classes' first tiles, resident for MAP and KSLOT
    PodClass* d_hcls = nullptr;
    uint32_t* d_t0 = nullptr;
    if (on(ESC_PAUD_MAP) || on(ESC_PAUD_KSLOT)) {
        HIP_TRY(S.get(&d_hcls, (size_t)std::max<int64_t>(n_cls, 1)));
        HIP_TRY(S.get(&d_t0, (size_t)std::max<int64_t>(n_cls, 1)));
        if (int32_t rc = G.next()) return rc;
        const size_t t0_at = ((size_t)n_cls * sizeof(PodClass) + 255) & ~(size_t)255;
        uint32_t* t0s = reinterpret_cast<uint32_t*>(G.host() + t0_at);
        for (int64_t i = 0; i < n_cls; ++i) t0s[i] = (uint32_t)std::min<int64_t>(std::max<int64_t>(c->h_cls[i].t0, 0), kt);
        if (n_cls) std::memcpy(G.host(), c->h_cls.data(), (size_t)n_cls * sizeof(PodClass));
        if (int32_t rc = G.send(d_hcls, 0, (size_t)n_cls * sizeof(PodClass))) return rc;
        if (n_cls) HIP_TRY(hipMemcpyAsync(d_t0, t0s, (size_t)n_cls * 4, hipMemcpyHostToDevice, st));
        if (int32_t rc = G.done()) return rc;
    }
    // ---- the free bitmap: the classes' free positions, the free C slots and the C tiles' padding
    if (on(ESC_PAUD_MAP) || on(ESC_PAUD_KSLOT) || on(ESC_PAUD_CSLOT)) {
        esc_audit_check& x = host[ESC_PAUD_MAP];             // (counted only when MAP runs)
        std::vector<uint32_t> fb((size_t)(n_slots / 32) + 1, 0);
        auto mark = [&](int64_t s) {
            if (fb[(size_t)(s >> 5)] & (1u << (s & 31))) paud_bad(x, s);   // named twice
            fb[(size_t)(s >> 5)] |= 1u << (s & 31);
        };
        for (size_t i = 0; i < c->cls_free.size() && (int64_t)i < n_cls; ++i) {
            const PodClass& k = c->h_cls[i];
            const bool cls_ok = k.t0 >= 0 && k.t0 <= k.t1 && k.t1 <= kt;
            for (int64_t q : c->cls_free[i]) {
                if (!cls_ok || q < 0 || q >= (k.t1 - k.t0) * TILE) paud_bad(x, cls_ok ? k.t0 * TILE : 0);
                else mark(k.t0 * TILE + q);
            }
        }
        for (int64_t d : c->c_free) {
            if (d < 0 || d >= npad) paud_bad(x, kslots);
            else mark(kslots + d);
        }
        for (int64_t d = 0; d < npad && c_ok; ++d)
            if (c->h_cflags[d] == ESC_PF_DAEMONSET) fb[(size_t)((kslots + d) >> 5)] |= 1u << ((kslots + d) & 31);
        uint32_t* d_free = nullptr;
        HIP_TRY(S.get(&d_free, fb.size()));
        HIP_TRY(S.get(&A.map_bits, fb.size()));
        HIP_TRY(hipMemsetAsync(A.map_bits, 0, fb.size() * 4, st));
        for (size_t at = 0; at < fb.size() * 4; at += PSTAGE_HALF) {
            const size_t bytes = std::min(PSTAGE_HALF, fb.size() * 4 - at);
            if (int32_t rc = G.next()) return rc;
            std::memcpy(G.host(), reinterpret_cast<const uint8_t*>(fb.data()) + at, bytes);
            if (int32_t rc = G.send(reinterpret_cast<uint8_t*>(d_free) + at, 0, bytes)) return rc;
            if (int32_t rc = G.done()) return rc;
        }
        A.free_bits = d_free;
    }
    // ---- MAP
    if (on(ESC_PAUD_MAP)) {
        const int64_t n = (int64_t)std::min(c->pod_cls.size(), c->pod_pos.size());
        if (c->pod_cls.size() != c->pod_pos.size()) paud_bad(host[ESC_PAUD_MAP], n_slots + n);
        constexpr int64_t CH = 1 << 18;                      // pods per chunk: 1 MiB of classes, 2 MiB of positions
        constexpr size_t POS_AT = (size_t)CH * 4;
        for (int64_t i0 = 0; i0 < n; i0 += CH) {
            const int64_t m = std::min(CH, n - i0);
            if (int32_t rc = G.next()) return rc;
            std::memcpy(G.host(), c->pod_cls.data() + i0, (size_t)m * 4);
            std::memcpy(G.host() + POS_AT, c->pod_pos.data() + i0, (size_t)m * 8);
            if (int32_t rc = G.send(nullptr, 0, (size_t)m * 4)) return rc;
            if (int32_t rc = G.send(nullptr, POS_AT, (size_t)m * 8)) return rc;
            HIP_TRY(launch_paud_map(A, reinterpret_cast<const int32_t*>(G.chunk()), reinterpret_cast<const int64_t*>(G.chunk() + POS_AT),
                                    i0, m, d_hcls, (int32_t)n_cls, st));
            if (int32_t rc = G.done()) return rc;
        }
        HIP_TRY(launch_paud_map_cmp(A, st));
    }
    // ---- KSLOT
    if (on(ESC_PAUD_KSLOT)) {
        if (c->n_cls != (int32_t)n_cls) paud_bad(host[ESC_PAUD_KSLOT], 0);
        const int64_t m = std::min<int64_t>(n_cls, A.P.n_cls);
        HIP_TRY(launch_paud_words(A, ESC_PAUD_KSLOT, reinterpret_cast<const uint32_t*>(A.P.cls),
                                  reinterpret_cast<const uint32_t*>(d_hcls), m * (int64_t)(sizeof(PodClass) / 4), d_t0,
                                  (int)(sizeof(PodClass) / 4), TILE, st));
        A.P.n_cls = (int32_t)m;
        HIP_TRY(launch_paud_kslot(A, st));
    }
    // ---- CSLOT
    if (on(ESC_PAUD_CSLOT)) {
        esc_audit_check& x = host[ESC_PAUD_CSLOT];
        bool asc = c_ok;
        for (int64_t t = 0; t < ct && asc; ++t)              // the offsets ascend (their end is the arrays' size)
            if (c->h_xc_base[t] > c->h_xc_base[t + 1] || c->h_xp_base[t] > c->h_xp_base[t + 1]) { asc = false; paud_bad(x, t * CTILE); }
        if (!c_ok) paud_bad(x, 0);
        constexpr int64_t CT = 4096;                         // tiles per chunk: 1 MiB of flags, 1 MiB of counts
        constexpr size_t USED_AT = (size_t)CT * CTILE * 4, XC_AT = 2 * USED_AT, XP_AT = XC_AT + (size_t)(CT + 64) * 4;
        for (int64_t t0 = 0; t0 < ct && asc; t0 += CT) {
            const int64_t m = std::min(CT, ct - t0);
            if (int32_t rc = G.next()) return rc;
            std::memcpy(G.host(), c->h_cflags.data() + t0 * CTILE, (size_t)m * CTILE * 4);
            std::memcpy(G.host() + USED_AT, c->h_cused.data() + t0 * CTILE, (size_t)m * CTILE * 4);
            std::memcpy(G.host() + XC_AT, c->h_xc_base.data() + t0, (size_t)(m + 1) * 4);
            std::memcpy(G.host() + XP_AT, c->h_xp_base.data() + t0, (size_t)(m + 1) * 4);
            if (int32_t rc = G.send(nullptr, 0, (size_t)m * CTILE * 4)) return rc;
            if (int32_t rc = G.send(nullptr, USED_AT, (size_t)m * CTILE * 4)) return rc;
            if (int32_t rc = G.send(nullptr, XC_AT, (size_t)(m + 1) * 4)) return rc;
            if (int32_t rc = G.send(nullptr, XP_AT, (size_t)(m + 1) * 4)) return rc;
            const uint8_t* d = G.chunk();
            HIP_TRY(launch_paud_cslot(A, t0, m, reinterpret_cast<const uint32_t*>(d), reinterpret_cast<const uint32_t*>(d + USED_AT),
                                      reinterpret_cast<const uint32_t*>(d + XC_AT), reinterpret_cast<const uint32_t*>(d + XP_AT), st));
            if (int32_t rc = G.done()) return rc;
        }
    }
    // ---- PODREF
    if (on(ESC_PAUD_PODREF)) {
        esc_audit_check& x = host[ESC_PAUD_PODREF];
        const int64_t NC = (int64_t)c->h_run_len.size(), total = (int64_t)c->h_run_pod.size();
        const int64_t np = (int64_t)c->pod_cls.size();
        bool runs_ok = (int64_t)c->h_run_off.size() == NC + 1 && NC == c->rm_nodes && c->h_pod_rpos.size() == c->h_pod_node.size() &&
                       dev_bytes_from(c->d_nrun_off) >= (NC + 1) * 4 && dev_bytes_from(c->d_nrun_len) >= NC * 4 &&
                       (NC == 0 || dev_bytes_from(c->d_refs) >= (int64_t)c->h_run_off[NC] * (int64_t)sizeof(PodRef));
        if (!runs_ok) paud_bad(x, 0);
        for (int64_t j = 0; j < NC && runs_ok; ++j)
            if (c->h_run_off[j] > c->h_run_off[j + 1] || c->h_run_len[j] > c->h_run_off[j + 1] - c->h_run_off[j] ||
                (int64_t)c->h_run_off[j + 1] > total) {
                paud_bad(x, std::min<int64_t>(c->h_run_off[j], total));
                runs_ok = false;
            }
        const int64_t n_refs = runs_ok && NC ? c->h_run_off[NC] : 0;
        // the pod -> position map names the position that names the pod, inside its node's run
        // (both passes over the pods are random reads of the mirrors: threaded, each thread's
        // finds merged — counts and a minimum, so the report does not depend on the split)
        const int T = host_threads();
        std::vector<esc_audit_check> part((size_t)T, esc_audit_check{0, 0, -1});
        auto merge = [&] {
            for (esc_audit_check& k : part) {
                x.n_bad += k.n_bad;
                if (k.n_bad && (x.first_bad < 0 || k.first_bad < x.first_bad)) x.first_bad = k.first_bad;
                k = esc_audit_check{0, 0, -1};
            }
        };
        if (runs_ok)
            par_chunks((int64_t)c->h_pod_rpos.size(), T, [&](int t, int64_t lo, int64_t hi) {
                for (int64_t id = lo; id < hi; ++id) {
                    const int64_t r = c->h_pod_rpos[id];
                    if (r < 0) continue;
                    const uint32_t j = c->h_pod_node[id];
                    if (r >= n_refs || c->h_run_pod[r] != (int32_t)id || (int64_t)j >= NC || r < (int64_t)c->h_run_off[j] ||
                        r >= (int64_t)c->h_run_off[j] + c->h_run_len[j])
                        paud_bad(part[t], std::min(r, total));
                }
            });
        merge();
        // the run table against the device's
        constexpr int64_t CN = 1 << 18;                      // nodes per chunk
        constexpr size_t LEN_AT = (size_t)(CN + 64) * 4;
        for (int64_t j0 = 0; j0 < NC && runs_ok; j0 += CN) {
            const int64_t m = std::min(CN, NC - j0);
            if (int32_t rc = G.next()) return rc;
            std::memcpy(G.host(), c->h_run_off.data() + j0, (size_t)(m + 1) * 4);
            std::memcpy(G.host() + LEN_AT, c->h_run_len.data() + j0, (size_t)m * 4);
            if (int32_t rc = G.send(nullptr, 0, (size_t)(m + 1) * 4)) return rc;
            if (int32_t rc = G.send(nullptr, LEN_AT, (size_t)m * 4)) return rc;
            const uint32_t* off = reinterpret_cast<const uint32_t*>(G.chunk());
            HIP_TRY(launch_paud_words(A, ESC_PAUD_PODREF, c->d_nrun_off + j0, off, m + (j0 + m == NC ? 1 : 0), off, 1, 1, st));
            HIP_TRY(launch_paud_words(A, ESC_PAUD_PODREF, c->d_nrun_len + j0, reinterpret_cast<const uint32_t*>(G.chunk() + LEN_AT),
                                      m, off, 1, 1, st));
            if (int32_t rc = G.done()) return rc;
        }
        // every position's pod by its present slot
        constexpr int64_t CR = 1 << 19;                      // run positions per chunk (2 MiB of slots)
        for (int64_t r0 = 0; r0 < n_refs; r0 += CR) {
            const int64_t m = std::min(CR, n_refs - r0);
            if (int32_t rc = G.next()) return rc;
            uint32_t* slot = reinterpret_cast<uint32_t*>(G.host());
            par_chunks(m, T, [&](int t, int64_t lo, int64_t hi) {
                for (int64_t i = lo; i < hi; ++i) {
                    const int64_t r = r0 + i, id = c->h_run_pod[r];
                    slot[i] = NONE;
                    if (id < 0) continue;
                    int64_t s = -1;
                    if (id < np && id < (int64_t)c->h_pod_rpos.size() && c->h_pod_rpos[id] == r && c->pod_cls[id] != -2) {
                        const int32_t ci = c->pod_cls[id];
                        const int64_t q = c->pod_pos[id];
                        if (ci == -1 && q >= 0 && q < npad) s = kslots + q;
                        else if (ci >= 0 && ci < n_cls && q >= 0 && q < (c->h_cls[ci].t1 - c->h_cls[ci].t0) * TILE) s = c->h_cls[ci].t0 * TILE + q;
                    }
                    if (s < 0 || s >= n_slots) paud_bad(part[t], r);   // a position that names no live pod's slot
                    else slot[i] = (uint32_t)s;
                }
            });
            merge();
            if (int32_t rc = G.send(nullptr, 0, (size_t)m * 4)) return rc;
            HIP_TRY(launch_paud_podref(A, c->d_refs, n_refs, reinterpret_cast<const uint32_t*>(G.chunk()), r0, m, st));
            if (int32_t rc = G.done()) return rc;
        }
    }
    // ---- REPLICA
    if (on(ESC_PAUD_REPLICA)) {
        const PodBuf& a = c->pods[0];
        const int64_t n_big = c->n_big;
#if ESC_MEASURE
        g_paud_replica_bytes = 0;
        g_paud_replica_ms = 0;
        if (hipEventCreate(&rt[0]) == hipSuccess && hipEventCreate(&rt[1]) == hipSuccess) hipEventRecord(rt[0], st);
#endif
        for (int r = 1; r < (int)c->pods.size(); ++r) {
            const PodBuf& b = c->pods[r];
            struct Arr { const void *x, *y; int64_t n; int esz; };
            const Arr arrs[12] = {{a.kb, b.kb, A.kb_words, 4},         {a.flags, b.flags, npad, 4},
                                  {a.cpu0, b.cpu0, npad, 4},           {a.pair0, b.pair0, npad, 4},
                                  {a.xp, b.xp, A.n_xp, 4},             {a.xc_base, b.xc_base, ct + 1, 4},
                                  {a.xp_base, b.xp_base, ct + 1, 4},   {a.big, b.big, n_big, 4},
                                  {a.mem0, b.mem0, npad, 8},           {a.xc_cpu, b.xc_cpu, A.n_xc, 8},
                                  {a.xc_mem, b.xc_mem, A.n_xc, 8},     {a.cls, b.cls, (int64_t)c->n_cls * (int64_t)(sizeof(PodClass) / 8), 8}};
            for (int k = 0; k < 12; ++k) {
                const Arr& q = arrs[k];
                if (q.n <= 0 || !q.x || !q.y) continue;
                const int64_t code = (int64_t)r << 56 | (int64_t)k << 48;
                const int64_t n = std::min({q.n, dev_bytes_from(q.x) / q.esz, dev_bytes_from(q.y) / q.esz});
                if (n < q.n) paud_bad(host[ESC_PAUD_REPLICA], code | n);       // an array shorter than the host's size for it
                HIP_TRY(launch_paud_replica(A, q.x, q.y, n * q.esz, q.esz, code, st));
#if ESC_MEASURE
                g_paud_replica_bytes += n * q.esz;
#endif
            }
        }
    }
#if ESC_MEASURE
    if (on(ESC_PAUD_REPLICA) && rt[1]) hipEventRecord(rt[1], st);
#endif
    HIP_TRY(hipMemcpyAsync(h_rep, A.rep, (size_t)ESC_PAUD_N * AW_K * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
#if ESC_MEASURE
    if (on(ESC_PAUD_REPLICA) && rt[1]) hipEventElapsedTime(&g_paud_replica_ms, rt[0], rt[1]);
#endif
    for (int k = 0; k < ESC_PAUD_N; ++k) {
        if (!on(k)) continue;
        esc_audit_check& x = out->check[k];
        x.n_checked = h_rep[k * AW_K + AW_CHECKED] + host[k].n_checked;
        x.n_bad = h_rep[k * AW_K + AW_BAD] + host[k].n_bad;
        x.first_bad = h_rep[k * AW_K + AW_BAD] ? h_rep[k * AW_K + AW_FIRST] : -1;
        if (host[k].n_bad && (x.first_bad < 0 || host[k].first_bad < x.first_bad)) x.first_bad = host[k].first_bad;
    }
    return ESC_OK;
}

}  // namespace

extern "C" {

int32_t esc_audit_pods(esc_ctx* c, uint32_t checks, esc_pod_audit_report* out) {
    if (c && c->multi) return esc::multi_audit_pods(c, checks, out);
    return audit_pods_one(c, checks, out);
}

#if ESC_MEASURE
// Corruption injection for esc_audit_pods (measurement library only; not in the header;
// tests/pod_audit_child.py): one word of the pod side made wrong, so that a test can show the
// matching check sees it.  As with esc_debug_poke only VALUE words are reachable: no kernel
// uses one of them as an address, index, offset, length or loop bound.  K words are written to
// every replica (REPLICA stays clean) except by target 8.
//   0 free K position `index` (a device slot) of a packed or packed small class: its word made
//     a live-looking pod, no pair, cpu = value (1 .. 2^14 - 1).  The pod pass reads the word's
//     cpu and mem as addends and its pair field as a slot only after comparing it with the
//     slot count (KP8_PAIR_NONE / KP_PAIR_NONE is above every count); kb_head returns values.
//   1 live pod at device slot `index` of a non-inert packed small class: daemonset and
//     blocks-default bits set.  Bits 62-63 are tested, never added or indexed with.
//   2 live default-blocking pod at slot `index` of an inert class: pair0 = value, a group pair.
//     No pass streams an inert class; podref_of and esc_pods_compact read pair0 as a value that
//     is compared with the pair count before it selects a bucket or a slot.
//   3 the host's live_p8_pods += value (a counter esc_stream_bytes reads; no device word).
//   4 live unbound K pod `index` (a pod id): pod_cls = -2 on the host only.  -2 is the value
//     every reader of the map tests first (absent); the slot is not put on a free list.
//   5 live C slot `index`: h_cflags ^ ESC_PF_STATIC on the host only (never a count: the
//     counts are the slot's room, which sizes prefix sums).
//   6 parked pod in C slot `index` with more pair room than pairs: the first pair past its
//     count = value in every replica.  A pair is matched against group pairs, never an index.
//   7 run position `index` that holds a pod: its PodRef's pair0 = value (never `flags`: the
//     indirect bit makes p[0] / p[1] an offset and a length).
//   8 live packed small pod at slot `index`: its cpu field = value in replica 1 only.
// Everything else is ESC_E_INVAL.
int32_t esc_debug_poke_pods(esc_ctx* c, int32_t what, int64_t index, int64_t value) {
    if (!c || c->multi || index < 0) return ESC_E_INVAL;
    if (!c->has_device) return ESC_E_NODEV;
    if (!c->pods_loaded || c->stale || c->pods.empty()) return ESC_E_STATE;
    hipSetDevice(c->device);
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int64_t kslots = c->k_tiles * TILE, npad = c->c_tiles * CTILE;
    // the class index of K slot s and whether the host lists its position as free
    auto k_class = [&](int64_t s) -> int {
        if (s >= kslots) return -1;
        for (size_t i = 0; i < c->h_cls.size(); ++i)
            if (s / TILE >= c->h_cls[i].t0 && s / TILE < c->h_cls[i].t1) return (int)i;
        return -1;
    };
    auto k_is_free = [&](int ci, int64_t s) {
        const int64_t q = s - c->h_cls[ci].t0 * TILE;
        return std::find(c->cls_free[ci].begin(), c->cls_free[ci].end(), q) != c->cls_free[ci].end();
    };
    auto c_live = [&](int64_t d) {
        return d < npad && c->h_cflags[d] != ESC_PF_DAEMONSET && std::find(c->c_free.begin(), c->c_free.end(), d) == c->c_free.end();
    };
    auto word64_at = [&](int ci, int64_t s) { return kb_block(c->h_cls[ci], s / TILE) / 2 + kb_pos64(s % TILE); };
    auto rd64 = [&](int r, int64_t at, uint64_t* w) {
        return hipMemcpy(w, reinterpret_cast<uint64_t*>(c->pods[r].kb) + at, 8, hipMemcpyDeviceToHost);
    };
    auto wr64 = [&](int r, int64_t at, uint64_t w) {
        return hipMemcpy(reinterpret_cast<uint64_t*>(c->pods[r].kb) + at, &w, 8, hipMemcpyHostToDevice);
    };
    uint64_t w = 0;
    switch (what) {
    case 0: {
        const int ci = k_class(index);
        if (ci < 0 || !c->h_cls[ci].packed || !k_is_free(ci, index) || value < 1 || value > (int64_t)KP8_CPU_MASK) return ESC_E_INVAL;
        const PodClass& k = c->h_cls[ci];
        for (int r = 0; r < (int)c->pods.size(); ++r) {
            if (k.packed == 2) {
                HIP_TRY(wr64(r, word64_at(ci, index), (uint64_t)value | (uint64_t)KP8_PAIR_NONE << KP8_PAIR_SHIFT));
            } else {
                const uint32_t w0 = KP_PAIR_NONE;
                const int64_t blk = kb_block(k, index / TILE);
                HIP_TRY(hipMemcpy(c->pods[r].kb + blk + index % TILE, &w0, 4, hipMemcpyHostToDevice));
                HIP_TRY(wr64(r, (blk + KP_CM0) / 2 + kb_pos64(index % TILE), kp_val(value, 0)));
            }
        }
        return ESC_OK;
    }
    case 1: case 2: case 8: {
        const int ci = k_class(index);
        if (ci < 0 || c->h_cls[ci].packed != 2 || k_is_free(ci, index)) return ESC_E_INVAL;
        const bool inert = kb_inert(c->h_cls[ci]);
        const int64_t at = word64_at(ci, index);
        HIP_TRY(rd64(0, at, &w));
        if (what == 1) {
            if (inert) return ESC_E_INVAL;
            w |= KP8_DS | KP8_NODEF;
        } else if (what == 2) {
            if (!inert || !(w & KP8_NODEF) || (w & KP8_DS) || value < 0 || value >= (int64_t)c->gi.n_gp) return ESC_E_INVAL;
            w = (w & ~((uint64_t)KP8_PAIR_NONE << KP8_PAIR_SHIFT)) | (uint64_t)value << KP8_PAIR_SHIFT;
        } else {
            if (c->pods.size() < 2 || value < 0 || value > (int64_t)KP8_CPU_MASK || (uint64_t)value == (w & KP8_CPU_MASK)) return ESC_E_INVAL;
            HIP_TRY(wr64(1, at, (w & ~KP8_CPU_MASK) | (uint64_t)value));
            return ESC_OK;
        }
        for (int r = 0; r < (int)c->pods.size(); ++r) HIP_TRY(wr64(r, at, w));
        return ESC_OK;
    }
    case 3:
        if (value == 0) return ESC_E_INVAL;
        c->live_p8_pods += value;
        return ESC_OK;
    case 4:
        if (index >= (int64_t)c->pod_cls.size() || c->pod_cls[index] < 0) return ESC_E_INVAL;
        if (c->placed && index < (int64_t)c->h_pod_rpos.size() && c->h_pod_rpos[index] >= 0) return ESC_E_INVAL;
        c->pod_cls[index] = -2;
        return ESC_OK;
    case 5:
        if (!c_live(index)) return ESC_E_INVAL;
        c->h_cflags[index] ^= ESC_PF_STATIC;
        return ESC_OK;
    case 6: {
        if (!c_live(index) || value < 0 || value >= (int64_t)NONE) return ESC_E_INVAL;
        const uint32_t np = c->h_cused[index] >> 16, room = pf_xpair(c->h_cflags[index]);
        if (np >= room) return ESC_E_INVAL;
        int64_t po = c->h_xp_base[index / CTILE];
        for (int64_t d = index / CTILE * CTILE; d < index; ++d) po += pf_xpair(c->h_cflags[d]);
        if (po + room > (int64_t)c->h_xp_base[c->c_tiles]) return ESC_E_INVAL;
        const uint32_t v = (uint32_t)value;
        for (PodBuf& b : c->pods) HIP_TRY(hipMemcpy(b.xp + po + np, &v, 4, hipMemcpyHostToDevice));
        return ESC_OK;
    }
    case 7: {
        if (!c->placed || !c->d_refs || index >= (int64_t)c->h_run_pod.size() || c->h_run_pod[index] < 0 || value < 0 ||
            value > (int64_t)NONE)
            return ESC_E_INVAL;
        const uint32_t v = (uint32_t)value;
        HIP_TRY(hipMemcpy(&c->d_refs[index].pair0, &v, 4, hipMemcpyHostToDevice));
        return ESC_OK;
    }
    default:
        return ESC_E_INVAL;
    }
}
int64_t esc_debug_pod_audit_bytes(void) { return g_paud_replica_bytes; }
double esc_debug_pod_audit_replica_ms(void) { return (double)g_paud_replica_ms; }
// The device slot of live pod `id` by the host's map (what the poke targets above and the
// report's first_bad are numbered in), -1 for an absent id; host only.
int64_t esc_debug_pod_slot(const esc_ctx* c, int64_t id) {
    if (!c || c->multi || !c->pods_loaded || id < 0 || id >= (int64_t)c->pod_cls.size() || c->pod_cls[id] == -2) return -1;
    const int32_t ci = c->pod_cls[id];
    if (ci >= (int32_t)c->h_cls.size()) return -1;
    return ci >= 0 ? c->h_cls[ci].t0 * TILE + c->pod_pos[id] : c->k_tiles * TILE + c->pod_pos[id];
}
// The 4-byte element of the K blocks that holds the low half of K slot `slot`'s first 8-byte
// word (a packed small pod's cpu field: REPLICA's element index for target 8), -1 outside K.
int64_t esc_debug_k_word(const esc_ctx* c, int64_t slot) {
    if (!c || c->multi || !c->pods_loaded || slot < 0) return -1;
    for (const PodClass& k : c->h_cls)
        if (slot / TILE >= k.t0 && slot / TILE < k.t1) return (kb_block(k, slot / TILE) / 2 + kb_pos64(slot % TILE)) * 2;
    return -1;
}
#endif

}  // extern "C"
