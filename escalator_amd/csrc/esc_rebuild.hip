// esc_rebuild.hip — the node-side rebuild on the device, the node table's
// compaction in front of it (§8l), and esc_audit with the measurement library's esc_debug_poke.
#include <functional>

#include "esc_ctx.h"

using namespace esc;

namespace {

// The buffers a rebuild builds beside the resident ones.  The swap exchanges them with the
// context's, so whatever this holds when it goes out of scope — the new buffers of a rebuild
// that failed, the old ones of one that succeeded, the scratch of both — is released.
struct RebuildBufs {
    NodeDerived nb;                               // entries, pieces, spans, rows, gnode, xl, xl_off, trk_start
    uint32_t *ne_off = nullptr, *ne_pos = nullptr, *e_pair = nullptr, *occ = nullptr, *occ_local = nullptr;
    uint32_t *nn_off = nullptr, *nn_list = nullptr, *rm_off = nullptr, *rm_list = nullptr;
    uint8_t* blob = nullptr;                      // the staged layout tables
    uint64_t* elems[2] = {nullptr, nullptr};
    uint32_t *hist = nullptr, *tot = nullptr;
    ~RebuildBufs() {
        nb.release();
        dfree(ne_off); dfree(ne_pos); dfree(e_pair); dfree(occ); dfree(occ_local);
        dfree(nn_off); dfree(nn_list); dfree(rm_off); dfree(rm_list);
        dfree(blob); dfree(elems[0]); dfree(elems[1]); dfree(hist); dfree(tot);
    }
};

// Seconds since the first call (the probe's split of a rebuild, esc_debug_rebuild_times).
double rebuild_clock() {
    timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}
thread_local double g_rebuild_ms[6];              // host layout, upload, kernels, mirrors, occupancy, age index

// The node table a rebuild derives the node side from: the resident one (esc_nodes_rebuild), or
// the one a compaction built beside it (esc_nodes_compact), whose `commit` makes it the
// resident one at the swap.  The extra labels are always the resident words: a compacted
// table's xl_off holds its nodes' OLD offsets.
struct NodeSrc {
    uint32_t* flags = nullptr;                                // device columns, [n_cap]
    const uint32_t *label0 = nullptr, *xl_off = nullptr;
    const int64_t *cpu = nullptr, *mem = nullptr;
    int64_t n_nodes = 0, n_cap = 0, min_free_xl = 0;
    const std::vector<uint32_t> *nflags = nullptr, *hlabel0 = nullptr, *hxl_off = nullptr;   // their mirrors
    const std::vector<int64_t> *ncpu = nullptr, *nmem = nullptr;
    const std::vector<uint64_t>* trk = nullptr;
    std::function<void()> commit;                             // nothing in it fails
};

NodeSrc resident_src(esc_ctx* c) {
    NodeSrc S;
    S.flags = c->nodes.flags; S.label0 = c->nodes.label0; S.xl_off = c->nodes.d.xl_off;
    S.cpu = c->nodes.cpu; S.mem = c->nodes.mem;
    S.n_nodes = c->n_nodes; S.n_cap = c->n_cap;
    S.nflags = &c->h_nflags; S.hlabel0 = &c->h_label0; S.hxl_off = &c->h_xl_off;
    S.ncpu = &c->h_ncpu; S.nmem = &c->h_nmem; S.trk = &c->h_trk;
    return S;
}

int32_t nodes_rebuild_from(esc_ctx* c, const NodeSrc& S) {
    const uint32_t n_gp = c->gi.n_gp;
    const int32_t G = c->gi.G;
    const int64_t N = S.n_nodes, NC = S.n_cap;
    const double sf = c->spare_frac;
    const std::vector<uint32_t>&s_flags = *S.nflags, &s_label0 = *S.hlabel0, &s_xl_off = *S.hxl_off;
    const std::vector<int64_t>&s_cpu = *S.ncpu, &s_mem = *S.nmem;
    if ((int64_t)s_flags.size() < NC || (int64_t)s_label0.size() < NC || (int64_t)s_xl_off.size() < NC ||
        (int64_t)s_cpu.size() < NC || (int64_t)s_mem.size() < NC || (int64_t)c->pair_live.size() != (int64_t)n_gp)
        return ESC_E_STATE;
    hipSetDevice(c->device);
    HIP_TRY(hipStreamSynchronize(c->stream));
    double t0 = rebuild_clock();
    for (double& x : g_rebuild_ms) x = 0;
    // ---- the layout, from the host's counts alone
    // the tracker index and bit first: the entries carry the bit
    std::vector<uint32_t> trk_start((size_t)std::max<int64_t>(NC, 1), NONE);
    for (int64_t k = (int64_t)S.trk->size() - 1; k >= 0; --k) {
        const uint64_t j = (*S.trk)[k] >> 32;
        if ((int64_t)j >= N) return fail_hip(hipErrorUnknown, "nodes rebuild: tracker mirror");
        trk_start[j] = (uint32_t)k;
    }
    std::vector<uint32_t> nflags(s_flags.begin(), s_flags.begin() + NC);
    std::vector<uint32_t> ne_off((size_t)NC + 1, 0), xl_off((size_t)std::max<int64_t>(NC, 1), 0);
    uint64_t m = 0, xw = 0;
    uint32_t max_pair = 0;
    bool pk_ok = true;
    for (int64_t i = 0; i < NC; ++i) {
        ne_off[i] = (uint32_t)m;
        xl_off[i] = (uint32_t)xw;
        uint32_t& f = nflags[i];
        if (i >= N || (f & ESC_NF_ABSENT)) continue;
        f = (f & ~ESC_NF_TRACKED) | (trk_start[i] != NONE ? ESC_NF_TRACKED : 0u);
        pk_ok = pk_ok && entry_cpu_packs(s_cpu[i]);
        if (s_label0[i] == NONE) continue;
        const uint32_t nx = nf_xlbl(f);
        if ((uint64_t)s_xl_off[i] + nx > c->h_xl.size()) return fail_hip(hipErrorUnknown, "nodes rebuild: label mirror");
        max_pair = std::max(max_pair, nx ? c->h_xl[s_xl_off[i] + nx - 1] : s_label0[i]);
        m += 1 + nx;
        xw += nx;
        if (m >= 0xFFFFFFFFull) return ESC_E_LIMIT;
    }
    ne_off[NC] = (uint32_t)m;
    const int64_t M = (int64_t)m;
    // the extra labels, compacted to the live nodes' words
    std::vector<uint32_t> h_xl((size_t)xw);
    for (int64_t i = 0; i < N; ++i) {
        if ((nflags[i] & ESC_NF_ABSENT) || s_label0[i] == NONE) continue;
        const uint32_t nx = nf_xlbl(nflags[i]);
        std::copy_n(c->h_xl.begin() + s_xl_off[i], nx, h_xl.begin() + xl_off[i]);
    }
    const int64_t xl_cap = std::max(label_words((int64_t)xw, sf), (int64_t)xw + S.min_free_xl);
    // group pairs: live entries sorted by node (start: where a pair's begin among the sorted
    // elements), then their spare ones; the entries of pairs no group selects follow all of
    // them as one run (pair NONE: nothing reads a piece of such a pair).  This rank's share
    // stays inside the kept owner bounds.  The ranges, pieces, spans and list offsets are
    // plan_node_layout's (esc_node_layout.h), as at a load.
    std::vector<uint32_t> start((size_t)n_gp + 1);
    uint64_t s_acc = 0;
    for (uint32_t q = 0; q < n_gp; ++q) {
        if (c->pair_live[q] < 0) return fail_hip(hipErrorUnknown, "nodes rebuild: pair mirror");
        start[q] = (uint32_t)s_acc;
        s_acc += (uint64_t)c->pair_live[q];
    }
    start[n_gp] = (uint32_t)s_acc;
    if ((int64_t)s_acc > M) return fail_hip(hipErrorUnknown, "nodes rebuild: pair mirror");
    NodeLayout L;
    if (const int32_t rc = plan_node_layout(L, c->pair_live, sf, {TailRun{NONE, (uint64_t)M - s_acc}}, c->q_lo, c->q_hi,
                                            pk_ok, c->gi.gpair.data(), G))
        return rc;
    const int64_t E = L.n_entries, n_pieces = L.n_pieces;
    const uint64_t spare_total = (uint64_t)(E - M);
    // ---- one staged copy of every table (the error word, zero, at its end)
    struct Part { const std::vector<uint32_t>* v; size_t at; };
    Part parts[] = {{&ne_off, 0}, {&xl_off, 0}, {&trk_start, 0}, {&start, 0}, {&L.pair_lo, 0}, {&L.piece_off, 0},
                    {&L.piece_pair, 0}, {&L.pp_off, 0}, {&L.span_off, 0}, {&L.span_e, 0}, {&L.list_off, 0}};
    enum { P_NE, P_XLO, P_TRK, P_START, P_LO, P_POFF, P_PPAIR, P_PP, P_SOFF, P_SE, P_LIST, P_N };
    size_t bytes = 0;
    for (Part& p : parts) { p.at = bytes; bytes += (p.v->size() * 4 + 255) & ~(size_t)255; }
    const size_t err_at = bytes;
    bytes += 256;
    std::vector<uint8_t> stage(bytes, 0);
    for (const Part& p : parts)
        if (!p.v->empty()) std::memcpy(stage.data() + p.at, p.v->data(), p.v->size() * 4);
    g_rebuild_ms[0] = (rebuild_clock() - t0) * 1e3;
    t0 = rebuild_clock();
    // ---- the new buffers, beside the resident ones
    RebuildBufs B;
    NodeDerived& b = B.nb;
    const size_t Ez = (size_t)std::max<int64_t>(E, 1), Pz = (size_t)std::max<int64_t>(n_pieces, 1);
    const bool reap = c->d_e_pair != nullptr;     // esc_load_placement's per-entry buffers exist
    HIP_TRY(dalloc(&B.blob, bytes));
    HIP_TRY(dalloc(&b.e_flags, Ez)); HIP_TRY(dalloc(&b.e_node, Ez)); HIP_TRY(dalloc(&b.e_cpu, Ez));
    HIP_TRY(dalloc(&b.e_mem, Ez)); HIP_TRY(dalloc(&b.e_pk, Ez));
    HIP_TRY(dalloc(&b.piece_off, L.piece_off.size())); HIP_TRY(dalloc(&b.piece_pair, Pz));
    HIP_TRY(dalloc(&b.pp_off, L.pp_off.size())); HIP_TRY(dalloc(&b.span_off, L.span_off.size()));
    HIP_TRY(dalloc(&b.span_e, L.span_e.size())); HIP_TRY(dalloc(&b.rows, Pz * NR_K));
    HIP_TRY(dalloc(&b.gnode, (size_t)G));
    HIP_TRY(dalloc(&b.xl, (size_t)xl_cap)); HIP_TRY(dalloc(&b.xl_off, xl_off.size()));
    HIP_TRY(dalloc(&b.trk_start, trk_start.size()));
    HIP_TRY(dalloc(&B.ne_off, ne_off.size())); HIP_TRY(dalloc(&B.ne_pos, Ez));
    HIP_TRY(dalloc(&B.nn_off, (size_t)G)); HIP_TRY(dalloc(&B.nn_list, std::max<uint32_t>(L.list_off[G], 1)));
    if (reap) {
        HIP_TRY(dalloc(&B.e_pair, Ez)); HIP_TRY(dalloc(&B.occ, 2 * Ez));
        if (c->d_occ_local) HIP_TRY(dalloc(&B.occ_local, 2 * Ez));
        HIP_TRY(dalloc(&B.rm_off, (size_t)G)); HIP_TRY(dalloc(&B.rm_list, std::max<uint32_t>(L.list_off[G], 1)));
    }
    HIP_TRY(dalloc(&B.elems[0], (size_t)M)); HIP_TRY(dalloc(&B.elems[1], (size_t)M));
    HIP_TRY(dalloc(&B.hist, std::max(sort_hist_words(std::max<int64_t>(M, 1)), sort_hist_words(1) * 4)));
    HIP_TRY(dalloc(&B.tot, 256));
    hipStream_t st = c->stream;
    HIP_TRY(hipMemcpyAsync(B.blob, stage.data(), bytes, hipMemcpyHostToDevice, st));
    auto view = [&](int k) { return reinterpret_cast<uint32_t*>(B.blob + parts[k].at); };
    auto keep = [&](uint32_t* dst, int k, size_t words) -> hipError_t {   // a table the snapshot keeps: its own buffer
        return words ? hipMemcpyAsync(dst, view(k), words * 4, hipMemcpyDeviceToDevice, st) : hipSuccess;
    };
    HIP_TRY(keep(B.ne_off, P_NE, ne_off.size())); HIP_TRY(keep(b.xl_off, P_XLO, xl_off.size()));
    HIP_TRY(keep(b.trk_start, P_TRK, trk_start.size())); HIP_TRY(keep(b.piece_off, P_POFF, L.piece_off.size()));
    HIP_TRY(keep(b.piece_pair, P_PPAIR, L.piece_pair.size())); HIP_TRY(keep(b.pp_off, P_PP, L.pp_off.size()));
    HIP_TRY(keep(b.span_off, P_SOFF, L.span_off.size())); HIP_TRY(keep(b.span_e, P_SE, L.span_e.size()));
    HIP_TRY(keep(B.nn_off, P_LIST, (size_t)G));
    if (reap) HIP_TRY(keep(B.rm_off, P_LIST, (size_t)G));
#if ESC_MEASURE
    HIP_TRY(hipStreamSynchronize(st));                       // (the probe's split: the upload's end)
    g_rebuild_ms[1] = (rebuild_clock() - t0) * 1e3;
    t0 = rebuild_clock();
#endif
    // ---- list, sort, place
    RebuildDev R{};
    R.flags = S.flags; R.label0 = S.label0; R.xl_off = S.xl_off; R.xl = c->nodes.d.xl;
    R.cpu = S.cpu; R.mem = S.mem;
    R.n_cap = NC; R.xl_len = c->xl_used;
    R.ne_off = view(P_NE); R.xl_off_new = view(P_XLO); R.trk_start = view(P_TRK); R.start = view(P_START);
    R.pair_lo = view(P_LO); R.piece_off = view(P_POFF); R.piece_pair = view(P_PPAIR);
    R.n_pieces = n_pieces; R.n_elems = M; R.n_entries = E; R.xl_new_cap = xl_cap;
    R.n_gp = n_gp; R.spare_total = (uint32_t)spare_total;
    R.xl_new = b.xl; R.e_flags = b.e_flags; R.e_node = b.e_node; R.e_pair = B.e_pair; R.e_cpu = b.e_cpu;
    R.e_mem = b.e_mem; R.e_pk = b.e_pk; R.ne_pos = B.ne_pos;
    R.err = reinterpret_cast<uint32_t*>(B.blob + err_at);
    HIP_TRY(launch_nodes_rebuild(R, B.elems, B.hist, B.tot, bit_width(max_pair), st));
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, R.err, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));                       // the build's wait
    if (err) return fail_fmt(ESC_E_HIP, "nodes rebuild: the node table does not fit the mirrors' layout (%u)", err);
    g_rebuild_ms[2] = (rebuild_clock() - t0) * 1e3;
    t0 = rebuild_clock();
    // ---- host mirrors: entry -> node in one copy, the map, allNodes[0] of every group
    std::vector<uint32_t> h_e_node((size_t)E), ne_pos((size_t)M);
    if (E) HIP_TRY(hipMemcpy(h_e_node.data(), b.e_node, (size_t)E * 4, hipMemcpyDeviceToHost));
    if (M) HIP_TRY(hipMemcpy(ne_pos.data(), B.ne_pos, (size_t)M * 4, hipMemcpyDeviceToHost));
    std::vector<GroupNode> gn((size_t)G);
    for (int32_t g = 0; g < G; ++g) {
        const uint32_t q = c->gi.gpair[g];
        const bool any = L.pair_next[q] > L.pair_lo[q];
        const uint32_t first = any ? h_e_node[L.pair_lo[q]] : NONE;      // sorted by node: the lowest
        if (any && (int64_t)first >= N) return fail_hip(hipErrorUnknown, "nodes rebuild: entry mirror");
        gn[g] = group_node(L, q, first, any ? s_cpu[first] : 0, any ? s_mem[first] : 0);
    }
    if (G) HIP_TRY(hipMemcpy(b.gnode, gn.data(), gn.size() * sizeof(GroupNode), hipMemcpyHostToDevice));
    g_rebuild_ms[3] = (rebuild_clock() - t0) * 1e3;
    // ---- the swap: nothing below fails before the snapshot is whole again
    drop_graphs(c);                                          // captured steps hold the old buffers
    if (S.commit) S.commit();                                // a compacted table becomes the resident one
    std::swap(c->nodes.d, B.nb);
    std::swap(c->d_ne_off, B.ne_off); std::swap(c->d_ne_pos, B.ne_pos);
    std::swap(c->d_nn_off, B.nn_off); std::swap(c->d_nn_list, B.nn_list);
    if (reap) {
        std::swap(c->d_e_pair, B.e_pair); std::swap(c->d_occ, B.occ); std::swap(c->d_occ_local, B.occ_local);
        std::swap(c->d_rm_off, B.rm_off); std::swap(c->d_rm_list, B.rm_list);
        c->h_rm_off = L.list_off;
    }
    commit_layout(c, L, pk_ok);
    c->h_nn_new.clear();
    c->h_e_node.swap(h_e_node);
    ne_off.resize((size_t)N + 1);                            // the host map covers the nodes so far (adds append)
    c->ne_off.swap(ne_off);
    c->ne_pos.swap(ne_pos);
    c->ne_dev_nodes = N;                                     // the device copy is the one just built
    c->ne_dev_pos = M;
    std::copy(nflags.begin(), nflags.end(), c->h_nflags.begin());
    std::copy(xl_off.begin(), xl_off.begin() + NC, c->h_xl_off.begin());
    c->h_xl.swap(h_xl);
    c->xl_used = c->n_xl = (int64_t)xw;
    c->xl_cap = xl_cap;
    c->h_gnode.swap(gn);
    c->sel_valid = c->rm_valid = c->nn_valid = false;
    c->sorted = false;
    // ---- what is recounted over the new entries: a failure from here on leaves the node
    // side stale (the occupancy words) or the orderings refused (the age index), as after a load
    t0 = rebuild_clock();
    if (reap && c->placed)
        if (int32_t rc = occ_recount(c)) { c->stale |= STALE_NODES; return rc; }
    g_rebuild_ms[4] = (rebuild_clock() - t0) * 1e3;
    t0 = rebuild_clock();
    release_sort(c);                                         // a fresh index: regions sized from the live counts
    const int32_t rc = build_age_index(c);
    g_rebuild_ms[5] = (rebuild_clock() - t0) * 1e3;
    return rc;
}

// ------------------------------------------------------------------- compaction
// The buffers a compaction builds beside the resident table; after the swap they hold the old
// ones.  Released on every way out.
struct CompactBufs {
    uint32_t *flags = nullptr, *label0 = nullptr, *xl_off = nullptr, *nrun_off = nullptr, *nrun_len = nullptr;
    int64_t *cpu = nullptr, *mem = nullptr, *created = nullptr, *inst = nullptr, *taint_s = nullptr;
    uint8_t *no_delete = nullptr, *blob = nullptr;
    int32_t* trk_node = nullptr;
    PodRef* refs = nullptr;
    ~CompactBufs() {
        dfree(flags); dfree(label0); dfree(xl_off); dfree(nrun_off); dfree(nrun_len);
        dfree(cpu); dfree(mem); dfree(created); dfree(inst); dfree(taint_s);
        dfree(no_delete); dfree(blob); dfree(trk_node); dfree(refs);
    }
};
thread_local double g_compact_ms[5];              // host plan, buffers + upload, gather + run move, host mirror remap,
                                                  // and of the remap the O(pods) pass alone

int32_t nodes_compact_one(esc_ctx* c, int64_t min_free_slots, int64_t min_free_xl_words, int64_t* new_index, int64_t cap) {
    const int64_t N0 = c->n_nodes;
    if (cap < N0) return ESC_E_LIMIT;
    if (!c->d_inst || (int64_t)c->h_nflags.size() < N0 || (int64_t)c->h_label0.size() < N0 || (int64_t)c->h_created.size() != N0 ||
        c->node_lo != 0 || c->node_hi != N0)
        return ESC_E_STATE;
    const bool facts = c->d_taint_s && c->d_no_delete;       // esc_load_placement's per-node facts exist
    const bool runs = c->placed && c->d_refs && c->d_nrun_off && c->d_nrun_len;
    if (runs && ((int64_t)c->h_run_off.size() < N0 + 1 || (int64_t)c->h_run_len.size() < N0)) return ESC_E_STATE;
    hipSetDevice(c->device);
    HIP_TRY(hipStreamSynchronize(c->stream));
    double t0 = rebuild_clock();
    for (double& x : g_compact_ms) x = 0;
    // ---- the plan, from the host's mirrors alone
    CompactPlan P;
    if (const int32_t rc = plan_node_compact(P, c->h_nflags.data(), c->h_label0.data(), N0, c->spare_frac, min_free_slots,
                                             min_free_xl_words, runs ? c->h_run_off.data() : nullptr,
                                             runs ? c->h_run_len.data() : nullptr, runs ? c->h_run_pod.data() : nullptr))
        return rc;
    const int64_t L = P.n_live, NC = P.n_cap;
    const int64_t refs_old = runs ? (int64_t)c->h_run_off.back() : 0;
    const int64_t refs_new = runs ? (int64_t)P.run_off[NC] : 0;
    std::vector<uint64_t> trk(c->h_trk);                     // monotone map: stays sorted
    std::vector<int32_t> trk_node((size_t)std::max<int64_t>(c->trk_cap, 1), 0);
    if ((int64_t)trk.size() > c->trk_cap) return ESC_E_STATE;
    for (size_t k = 0; k < trk.size(); ++k) {
        const uint64_t j = trk[k] >> 32;
        if ((int64_t)j >= N0 || P.new_of[j] == NONE) return fail_hip(hipErrorUnknown, "nodes compact: tracker mirror");
        trk[k] = ((uint64_t)P.new_of[j] << 32) | (uint32_t)trk[k];
        trk_node[k] = (int32_t)P.new_of[j];
    }
    // ---- one staged copy of the plan's tables (the error word, zero, at its end)
    static_assert(sizeof(RunMove) == 12, "k_run_move reads a move as three words");
    struct Part { const void* p; size_t bytes, at; };
    Part parts[] = {{P.src_of.data(), P.src_of.size() * 4, 0}, {P.moves.data(), P.moves.size() * sizeof(RunMove), 0},
                    {P.run_off.data(), P.run_off.size() * 4, 0}, {P.run_len.data(), P.run_len.size() * 4, 0},
                    {trk_node.data(), trk_node.size() * 4, 0}};
    enum { C_SRC, C_MOVES, C_ROFF, C_RLEN, C_TRK };
    size_t bytes = 0;
    for (Part& q : parts) { q.at = bytes; bytes += (q.bytes + 255) & ~(size_t)255; }
    const size_t err_at = bytes;
    bytes += 256;
    std::vector<uint8_t> stage(bytes, 0);
    for (const Part& q : parts)
        if (q.bytes) std::memcpy(stage.data() + q.at, q.p, q.bytes);
    g_compact_ms[0] = (rebuild_clock() - t0) * 1e3;
    t0 = rebuild_clock();
    // ---- the new table, beside the resident one
    CompactBufs B;
    const size_t NCz = (size_t)std::max<int64_t>(NC, 1);
    HIP_TRY(dalloc(&B.blob, bytes));
    HIP_TRY(dalloc(&B.flags, NCz)); HIP_TRY(dalloc(&B.label0, NCz)); HIP_TRY(dalloc(&B.xl_off, NCz));
    HIP_TRY(dalloc(&B.cpu, NCz)); HIP_TRY(dalloc(&B.mem, NCz)); HIP_TRY(dalloc(&B.created, NCz));
    HIP_TRY(dalloc(&B.inst, NCz)); HIP_TRY(dalloc(&B.trk_node, trk_node.size()));
    if (facts) { HIP_TRY(dalloc(&B.taint_s, NCz)); HIP_TRY(dalloc(&B.no_delete, NCz)); }
    if (runs) {
        HIP_TRY(dalloc(&B.refs, (size_t)std::max<int64_t>(refs_new, 1)));
        HIP_TRY(dalloc(&B.nrun_off, (size_t)NC + 1)); HIP_TRY(dalloc(&B.nrun_len, NCz));
    }
    hipStream_t st = c->stream;
    HIP_TRY(hipMemcpyAsync(B.blob, stage.data(), bytes, hipMemcpyHostToDevice, st));
    auto view = [&](int k) { return reinterpret_cast<uint32_t*>(B.blob + parts[k].at); };
    auto keep = [&](void* dst, int k) -> hipError_t {         // a table the snapshot keeps: its own buffer
        return parts[k].bytes ? hipMemcpyAsync(dst, view(k), parts[k].bytes, hipMemcpyDeviceToDevice, st) : hipSuccess;
    };
    HIP_TRY(keep(B.trk_node, C_TRK));
    if (runs) { HIP_TRY(keep(B.nrun_off, C_ROFF)); HIP_TRY(keep(B.nrun_len, C_RLEN)); }
#if ESC_MEASURE
    HIP_TRY(hipStreamSynchronize(st));                       // (the probe's split: the upload's end)
    g_compact_ms[1] = (rebuild_clock() - t0) * 1e3;
    t0 = rebuild_clock();
#endif
    // ---- gather the table, move the runs
    CompactDev D{};
    D.flags = c->nodes.flags; D.label0 = c->nodes.label0; D.xl_off = c->nodes.d.xl_off;
    D.cpu = c->nodes.cpu; D.mem = c->nodes.mem; D.created = c->nodes.created; D.inst = c->d_inst;
    D.taint_s = facts ? c->d_taint_s : nullptr; D.no_delete = facts ? c->d_no_delete : nullptr;
    D.n_old = N0;
    D.src_of = view(C_SRC); D.n_new = NC;
    D.moves = view(C_MOVES); D.n_moves = runs ? (int64_t)P.moves.size() : 0;
    D.flags_new = B.flags; D.label0_new = B.label0; D.xl_off_new = B.xl_off;
    D.cpu_new = B.cpu; D.mem_new = B.mem; D.created_new = B.created; D.inst_new = B.inst;
    D.taint_new = B.taint_s; D.nd_new = B.no_delete;
    D.refs_old = reinterpret_cast<const uint32_t*>(c->d_refs); D.refs_new = reinterpret_cast<uint32_t*>(B.refs);
    D.refs_old_words = refs_old * 5; D.refs_new_words = refs_new * 5;
    D.err = reinterpret_cast<uint32_t*>(B.blob + err_at);
    HIP_TRY(launch_nodes_compact(D, st));
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, D.err, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));                       // the call's one wait before the rebuild's
    if (err) return fail_fmt(ESC_E_HIP, "nodes compact: the node table does not fit the mirrors' plan (%u)", err);
    g_compact_ms[2] = (rebuild_clock() - t0) * 1e3;
    t0 = rebuild_clock();
    // ---- the new table's mirrors, beside the resident ones (a mirror that disagrees with the
    // table is reported, not repaired: they are permuted, never re-read)
    std::vector<uint32_t> nflags(NCz, ESC_NF_ABSENT), label0(NCz, NONE), xl_off(NCz, 0);
    std::vector<int64_t> ncpu(NCz, 0), nmem(NCz, 0), created((size_t)L);
    for (int64_t i = 0; i < L; ++i) {
        const uint32_t s = P.src_of[i];
        nflags[i] = c->h_nflags[s]; label0[i] = c->h_label0[s]; xl_off[i] = c->h_xl_off[s];
        ncpu[i] = c->h_ncpu[s]; nmem[i] = c->h_nmem[s]; created[i] = c->h_created[s];
    }
    std::vector<int32_t> run_pod;
    if (runs) {
        run_pod.assign((size_t)std::max<int64_t>(refs_new, 1), -1);
        for (const RunMove& m : P.moves) std::copy_n(c->h_run_pod.begin() + m.src, m.len, run_pod.begin() + m.dst);
    }
    g_compact_ms[3] = (rebuild_clock() - t0) * 1e3;
    // ---- the rebuild over the new table; its swap makes the table the resident one
    bool swapped = false;
    NodeSrc S;
    S.flags = B.flags; S.label0 = B.label0; S.xl_off = B.xl_off; S.cpu = B.cpu; S.mem = B.mem;
    S.n_nodes = L; S.n_cap = NC; S.min_free_xl = min_free_xl_words;
    S.nflags = &nflags; S.hlabel0 = &label0; S.hxl_off = &xl_off; S.ncpu = &ncpu; S.nmem = &nmem; S.trk = &trk;
    S.commit = [&]() {
        const double t1 = rebuild_clock();
        NodeBuf& b = c->nodes;
        std::swap(b.flags, B.flags); std::swap(b.label0, B.label0); std::swap(b.cpu, B.cpu); std::swap(b.mem, B.mem);
        std::swap(b.created, B.created); std::swap(b.trk_node, B.trk_node); std::swap(c->d_inst, B.inst);
        if (facts) {
            std::swap(c->d_taint_s, B.taint_s); std::swap(c->d_no_delete, B.no_delete);
            c->rm_nodes = NC;
        }
        if (runs) {
            // every bound pod follows its node's run; the pods of dead runs come out unbound
            const double t2 = rebuild_clock();
            const std::vector<uint32_t>& old_off = c->h_run_off;
            par_chunks((int64_t)c->h_pod_node.size(), host_threads(), [&](int, int64_t lo, int64_t hi) {
                for (int64_t i = lo; i < hi; ++i) {
                    const uint32_t j = c->h_pod_node[i];
                    if (j == NONE) continue;
                    const uint32_t nj = (int64_t)j < N0 ? P.new_of[j] : NONE;
                    c->h_pod_node[i] = nj;
                    c->h_pod_rpos[i] = nj == NONE ? -1 : c->h_pod_rpos[i] - (int64_t)old_off[j] + (int64_t)P.run_off[nj];
                }
            });
            g_compact_ms[4] = (rebuild_clock() - t2) * 1e3;
            std::swap(c->d_refs, B.refs); std::swap(c->d_nrun_off, B.nrun_off); std::swap(c->d_nrun_len, B.nrun_len);
            c->h_run_off.swap(P.run_off); c->h_run_len.swap(P.run_len); c->h_run_pod.swap(run_pod);
        }
        c->h_nflags.swap(nflags); c->h_label0.swap(label0); c->h_xl_off.swap(xl_off);
        c->h_ncpu.swap(ncpu); c->h_nmem.swap(nmem); c->h_created.swap(created); c->h_trk.swap(trk);
        c->n_nodes = L; c->n_cap = NC;
        c->node_lo = 0; c->node_hi = L;
        swapped = true;
        g_compact_ms[3] += (rebuild_clock() - t1) * 1e3;
    };
    const int32_t rc = nodes_rebuild_from(c, S);
    if (swapped)
        for (int64_t j = 0; j < N0; ++j) new_index[j] = P.new_of[j] == NONE ? -1 : (int64_t)P.new_of[j];
    return rc;
}

}  // namespace

extern "C" {

int32_t esc_nodes_rebuild(esc_ctx* c) {
    if (c && c->multi) return esc::multi_nodes_rebuild(c);
    if (!c) return ESC_E_INVAL;
    if (!c->has_device) return ESC_E_NODEV;
    if (!c->nodes_loaded || c->stale) return ESC_E_STATE;
    return nodes_rebuild_from(c, resident_src(c));
}

int32_t esc_nodes_compact(esc_ctx* c, int64_t min_free_slots, int64_t min_free_xl_words, int64_t* new_index, int64_t cap) {
    if (c && c->multi) return esc::multi_nodes_compact(c, min_free_slots, min_free_xl_words, new_index, cap);
    if (!c || min_free_slots < 0 || min_free_xl_words < 0 || cap < 0 || (cap > 0 && !new_index)) return ESC_E_INVAL;
    if (!c->has_device) return ESC_E_NODEV;
    if (!c->nodes_loaded || c->stale) return ESC_E_STATE;
    return nodes_compact_one(c, min_free_slots, min_free_xl_words, new_index, cap);
}

int32_t esc_nodes_room(const esc_ctx* c, int64_t* free_slots, int64_t* free_xl_words) {
    if (c && c->multi) return esc_nodes_room(esc::multi_sub(c, 0), free_slots, free_xl_words);
    if (!c) return ESC_E_INVAL;
    if (!c->has_device) return ESC_E_NODEV;
    if (!c->nodes_loaded) return ESC_E_STATE;
    if (free_slots) *free_slots = c->n_cap - c->n_nodes;
    if (free_xl_words) *free_xl_words = c->xl_cap - c->xl_used;
    return ESC_OK;
}

#if ESC_MEASURE
// The last esc_nodes_rebuild of this thread, split (ms): host layout, upload, list + sort +
// place, mirror download, occupancy recount, age-index build (measurement library only; not
// in the header; scripts/rebuild_probe.py).
int32_t esc_debug_rebuild_times(double* ms, int32_t n) {
    if (!ms || n < 0) return ESC_E_INVAL;
    for (int32_t k = 0; k < n && k < 6; ++k) ms[k] = g_rebuild_ms[k];
    return ESC_OK;
}

// The last esc_nodes_compact of this thread before its rebuild part (ms): host plan, buffers and
// upload, gather + run move to the wait, host mirror remap, the remap's O(pods) pass alone;
// esc_debug_rebuild_times has the rest
// (scripts/compact_probe.py).
int32_t esc_debug_compact_times(double* ms, int32_t n) {
    if (!ms || n < 0) return ESC_E_INVAL;
    for (int32_t k = 0; k < n && k < 5; ++k) ms[k] = g_compact_ms[k];
    return ESC_OK;
}
#endif

}  // extern "C"

// ------------------------------------------------------------------- audit
namespace {

// Device scratch of one audit, freed on every way out.
struct AuditScratch {
    std::vector<void*> bufs;
    ~AuditScratch() { for (void* p : bufs) hipFree(p); }
    template <class T>
    hipError_t get(T** p, size_t n) {
        const hipError_t e = dalloc(p, n);
        if (e == hipSuccess) bufs.push_back(*p);
        return e;
    }
};

void audit_bad(esc_audit_check& k, int64_t id) {
    ++k.n_bad;
    if (k.first_bad < 0 || id < k.first_bad) k.first_bad = id;
}

// TOUCH on the host (the tables are small): every column the recount `fresh` finds touched is
// in the maintained bitmap h_touch, every workgroup's device list holds exactly its bitmap row's
// columns, and the destinations are the columns' ranges handed out in workgroup order — what
// touch_upload derives from the bitmap.  An offender is a (workgroup, column) pair, counted once.
void audit_touch(const esc_ctx* c, const std::vector<uint32_t>& fresh, const std::vector<uint2>& cols,
                 const std::vector<uint32_t>& wg_off, const std::vector<uint32_t>& col_rows, esc_audit_check& k) {
    const int64_t nblk = c->nblk, tw = c->touch_tw, n_col = slot_stride(c) / FC_COL;
    std::vector<uint64_t> bad;
    auto key = [](int64_t b, int64_t col) { return ((uint64_t)b << 32) | (uint64_t)(uint32_t)col; };
    auto kept = [&](int64_t b, int64_t col) { return (c->h_touch[b * tw + (col >> 5)] >> (col & 31)) & 1u; };
    std::vector<uint32_t> seen(n_col, 0), stamp(n_col, 0);
    for (int64_t b = 0; b < nblk; ++b) {
        for (int64_t w = 0; w < tw; ++w)
            for (uint32_t x = fresh[b * tw + w]; x; x &= x - 1) {
                const int64_t col = w * 32 + __builtin_ctz(x);
                if (col >= n_col) continue;
                ++k.n_checked;
                if (!kept(b, col)) bad.push_back(key(b, col));
            }
        const int64_t cnt = std::min<int64_t>(wg_off[b], n_col);
        if ((int64_t)wg_off[b] > n_col) bad.push_back(key(b, 0xFFFFFFFFll));
        for (int64_t i = 0; i < cnt; ++i) {
            const uint2 e = cols[b * n_col + i];
            if ((int64_t)e.x >= n_col) { bad.push_back(key(b, e.x)); continue; }
            if (stamp[e.x] == (uint32_t)b + 1 || !kept(b, e.x) || e.y != col_rows[e.x] + seen[e.x]) bad.push_back(key(b, e.x));
            if (stamp[e.x] != (uint32_t)b + 1) ++seen[e.x];
            stamp[e.x] = (uint32_t)b + 1;
        }
        for (int64_t w = 0; w < tw; ++w)
            for (uint32_t x = c->h_touch[b * tw + w]; x; x &= x - 1) {
                const int64_t col = w * 32 + __builtin_ctz(x);
                if (col < n_col && stamp[col] != (uint32_t)b + 1) bad.push_back(key(b, col));
            }
    }
    for (int64_t col = 0; col < n_col; ++col)                  // the columns' ranges (K3 reads them)
        if (col_rows[col + 1] - col_rows[col] != seen[col] || (col == 0 && col_rows[0] != 0)) bad.push_back(key(nblk, col));
    std::sort(bad.begin(), bad.end());
    bad.erase(std::unique(bad.begin(), bad.end()), bad.end());
    for (uint64_t x : bad) audit_bad(k, (int64_t)x);
}

}  // namespace

extern "C" {

int32_t esc_audit(esc_ctx* c, uint32_t checks, esc_audit_report* out) {
    if (c && c->multi) return esc::multi_audit(c, checks, out);
    if (!c || !out || (checks >> ESC_AUD_N)) return ESC_E_INVAL;
    if (!c->has_device) return ESC_E_NODEV;
    if (!c->nodes_loaded || c->stale) return ESC_E_STATE;
    if (!checks) checks = (1u << ESC_AUD_N) - 1;
    std::memset(out, 0, sizeof *out);
    for (esc_audit_check& k : out->check) k.first_bad = -1;
    // a check whose derived state is not resident is skipped: the occupancy words come with a
    // placement, the regions with a valid age index, the touch tables with the first step's
    // static K1 plan
    uint32_t skip = 0;
    if (!c->placed || !c->d_e_pair || !c->d_occ) skip |= 1u << ESC_AUD_OCC;
    if (!(c->age_built && c->age_ok && !c->h_pcap.empty() && c->d_g_memb)) skip |= 1u << ESC_AUD_REGION;
    if (!c->pods_loaded || !c->work_ready || !c->touch_on || !c->d_k1seg || c->pods.empty()) skip |= 1u << ESC_AUD_TOUCH;
    out->skipped = checks & skip;
    out->ran = checks & ~skip;
    const uint32_t run = out->ran;
    auto on = [&](int k) { return (run >> k) & 1u; };
    hipSetDevice(c->device);
    hipStream_t st = c->stream;
    const GroupDev g = group_dev(c);
    const NodeDev n = node_dev(c);
    const int32_t G = c->gi.G;
    const uint32_t n_gp = c->gi.n_gp;
    const int64_t E = c->n_entries, NC = c->n_cap;
    AuditScratch S;
    AuditDev a{};
    std::vector<int64_t> rep((size_t)ESC_AUD_N * AW_K, 0);
    for (int k = 0; k < ESC_AUD_N; ++k) rep[(size_t)k * AW_K + AW_FIRST] = INT64_MAX;
    HIP_TRY(S.get(&a.rep, rep.size()));
    HIP_TRY(hipMemcpyAsync(a.rep, rep.data(), rep.size() * 8, hipMemcpyHostToDevice, st));
    a.n_cap = NC;
    a.n_entries = E;
    a.e_pair = c->placed ? c->d_e_pair : nullptr;
    std::vector<uint32_t> pair_cnt(std::max<uint32_t>(n_gp, 1), 0), memb_cnt((size_t)std::max<int32_t>(G, 1), 0);
    std::vector<uint32_t> own;                                  // the groups whose node side this rank owns
    for (int32_t q = 0; q < G; ++q)
        if (owns_group(c, (uint32_t)q)) own.push_back((uint32_t)q);
    if (on(ESC_AUD_ENTRY)) {
        if (int32_t rc = ensure_ne_dev(c)) return rc;           // (the lazily uploaded map, re-sent when out of date)
        a.ne_off = c->d_ne_off;
        a.ne_pos = c->d_ne_pos;
        a.ne_len = (int64_t)c->ne_pos.size();
        HIP_TRY(S.get(&a.pair_cnt, pair_cnt.size()));
        HIP_TRY(hipMemsetAsync(a.pair_cnt, 0, pair_cnt.size() * 4, st));
        HIP_TRY(launch_audit_entries(n, g, a, st));
        HIP_TRY(launch_audit_node_entries(n, g, a, st));
        HIP_TRY(hipMemcpyAsync(pair_cnt.data(), a.pair_cnt, pair_cnt.size() * 4, hipMemcpyDeviceToHost, st));
    }
    if (on(ESC_AUD_FIRST) && !own.empty()) {
        uint32_t* d_own = nullptr;
        HIP_TRY(S.get(&d_own, own.size()));
        HIP_TRY(hipMemcpyAsync(d_own, own.data(), own.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(launch_audit_first(n, g, GroupList{d_own, (int32_t)own.size(), 0}, a, st));
    }
    if (on(ESC_AUD_REGION) && G > 0) {
        uint32_t *d_ps = nullptr, *d_pl = nullptr;
        HIP_TRY(S.get(&d_ps, (size_t)G + 1));
        HIP_TRY(S.get(&d_pl, (size_t)G));
        HIP_TRY(S.get(&a.memb_cnt, memb_cnt.size()));
        HIP_TRY(hipMemcpyAsync(d_ps, c->h_pstart.data(), ((size_t)G + 1) * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_pl, c->h_plen.data(), (size_t)G * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(a.memb_cnt, 0, memb_cnt.size() * 4, st));
        HIP_TRY(launch_audit_regions(n, g, d_ps, d_pl, c->d_g_memb, a, st));
        HIP_TRY(hipMemcpyAsync(memb_cnt.data(), a.memb_cnt, memb_cnt.size() * 4, hipMemcpyDeviceToHost, st));
    }
    if (on(ESC_AUD_OCC) && E > 0) {
        // K6 into scratch through a view of the placement that points there, then the compare
        uint32_t* fresh = nullptr;
        HIP_TRY(S.get(&fresh, (size_t)(2 * E)));
        RemovalDev r = occ_dev(c);
        const uint32_t* kept = r.occ_pair;
        r.occ_pair = fresh;
        r.occ_def = fresh + E;
        HIP_TRY(launch_occupancy(n, g, r, st));
        HIP_TRY(launch_audit_occ(n, g, a, fresh, kept, st));
    }
    std::vector<uint32_t> t_fresh, t_off, t_rows;
    std::vector<uint2> t_cols;
    if (on(ESC_AUD_TOUCH)) {
        const int64_t n_col = slot_stride(c) / FC_COL;
        t_fresh.assign((size_t)c->nblk * c->touch_tw, 0);
        t_off.assign((size_t)c->nblk, 0);
        t_rows.assign((size_t)n_col + 1, 0);
        t_cols.assign((size_t)c->nblk * n_col, make_uint2(0, 0));
        uint32_t* d_bits = nullptr;
        HIP_TRY(S.get(&d_bits, t_fresh.size()));
        HIP_TRY(launch_touch(pod_dev(c, 0), g, c->nblk, c->touch_tw, d_bits, st));
        HIP_TRY(hipMemcpyAsync(t_fresh.data(), d_bits, t_fresh.size() * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(t_off.data(), c->d_wg_off, t_off.size() * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(t_rows.data(), c->d_col_rows, t_rows.size() * 4, hipMemcpyDeviceToHost, st));
        if (!t_cols.empty())
            HIP_TRY(hipMemcpyAsync(t_cols.data(), c->d_wg_cols, t_cols.size() * sizeof(uint2), hipMemcpyDeviceToHost, st));
    }
    if (on(ESC_AUD_TRACKER)) HIP_TRY(launch_audit_tracker(n, g, a, st));
    std::vector<uint32_t> m_flags, m_label0;
    std::vector<int64_t> m_cpu, m_mem;
    if (on(ESC_AUD_MIRROR) && NC > 0) {
        m_flags.resize(NC); m_label0.resize(NC); m_cpu.resize(NC); m_mem.resize(NC);
        HIP_TRY(hipMemcpyAsync(m_flags.data(), c->nodes.flags, NC * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(m_label0.data(), c->nodes.label0, NC * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(m_cpu.data(), c->nodes.cpu, NC * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(m_mem.data(), c->nodes.mem, NC * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(rep.data(), a.rep, rep.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < ESC_AUD_N; ++k) {
        esc_audit_check& x = out->check[k];
        x.n_checked = rep[(size_t)k * AW_K + AW_CHECKED];
        x.n_bad = rep[(size_t)k * AW_K + AW_BAD];
        x.first_bad = x.n_bad ? rep[(size_t)k * AW_K + AW_FIRST] : -1;
    }
    if (on(ESC_AUD_ENTRY))                                      // per-pair live counts against the host's
        for (uint32_t q = 0; q < n_gp; ++q)
            if ((int64_t)pair_cnt[q] != c->pair_live[q]) audit_bad(out->check[ESC_AUD_ENTRY], c->pair_lo[q]);
    if (on(ESC_AUD_REGION))                                     // a group's live memberships = its pair's live entries
        for (uint32_t q : own)
            if ((int64_t)memb_cnt[q] != c->pair_live[c->gi.gpair[q]]) audit_bad(out->check[ESC_AUD_REGION], c->h_pstart[q]);
    if (on(ESC_AUD_TOUCH)) audit_touch(c, t_fresh, t_cols, t_off, t_rows, out->check[ESC_AUD_TOUCH]);
    if (on(ESC_AUD_MIRROR)) {
        esc_audit_check& x = out->check[ESC_AUD_MIRROR];
        x.n_checked = NC;
        for (int64_t j = 0; j < NC; ++j)
            if (m_flags[j] != c->h_nflags[j] || m_cpu[j] != c->h_ncpu[j] || m_mem[j] != c->h_nmem[j] ||
                m_label0[j] != c->h_label0[j])
                audit_bad(x, j);
    }
    return ESC_OK;
}

#if ESC_MEASURE
// Corruption injection (measurement library only; not in the header; tests/audit_child.py): one
// derived word made wrong, so that a test can show the matching audit check sees it.  Only
// VALUE words are reachable — no kernel uses one of them as an address, index, offset, length
// or loop bound — so a poke changes numbers, never where a kernel reads or writes:
//   0 entry `index`: its UNSCHED / TAINTED bits ^= value (1..3)   1 entry: e_cpu (and the packed copy) = value
//   2 region word `index`: UNSCHED / TAINTED / TRACKED of its nibble ^= value (1..7)
//   3 region words `index`, `index` + 1 swapped (two memberships of one group)
//   4 occupancy word `index` of [2][n_entries] = value       5 touch bitmap: workgroup `index`, set column `value` cleared
//   6 node `index`: ESC_NF_TRACKED flipped in the device node table only
//   7 group `index`: GroupNode::first_cpu = value            8 node `index`: the host mirror h_ncpu = value
//   9 deleted slot `index`: ESC_NF_ABSENT cleared in the host mirror h_nflags only (esc_nodes_compact
//     then plans a source the table calls absent; k_node_gather reports it)
// Everything else is ESC_E_INVAL.
int32_t esc_debug_poke(esc_ctx* c, int32_t what, int64_t index, int64_t value) {
    if (!c || c->multi || index < 0) return ESC_E_INVAL;
    if (!c->has_device) return ESC_E_NODEV;
    if (!c->nodes_loaded || c->stale) return ESC_E_STATE;
    hipSetDevice(c->device);
    HIP_TRY(hipStreamSynchronize(c->stream));
    auto live_entry = [&](int64_t e) {                         // an entry of a group pair whose node is live
        return e < c->n_entries && c->h_e_node[e] != NONE && !(c->h_nflags[c->h_e_node[e]] & ESC_NF_ABSENT) &&
               entry_pair(c, (uint32_t)e) != NONE;
    };
    // the owned group whose live memberships hold region word i (h_pstart / h_plen), or -1
    auto region_group = [&](int64_t i) -> int32_t {
        if (!(c->age_built && c->age_ok) || c->h_pstart.empty()) return -1;
        for (int32_t q = 0; q < c->gi.G; ++q)
            if (owns_group(c, (uint32_t)q) && i >= c->h_pstart[q] && i < (int64_t)c->h_pstart[q] + c->h_plen[q]) return q;
        return -1;
    };
    uint32_t w = 0, w2 = 0;
    switch (what) {
    case 0:
        if (!live_entry(index) || value < 1 || value > 3) return ESC_E_INVAL;
        HIP_TRY(hipMemcpy(&w, c->nodes.d.e_flags + index, 4, hipMemcpyDeviceToHost));
        w ^= (uint32_t)value;
        HIP_TRY(hipMemcpy(c->nodes.d.e_flags + index, &w, 4, hipMemcpyHostToDevice));
        return ESC_OK;
    case 1:
        if (!live_entry(index) || !entry_cpu_packs(value)) return ESC_E_INVAL;
        w = (uint32_t)value;
        HIP_TRY(hipMemcpy(c->nodes.d.e_cpu + index, &value, 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(reinterpret_cast<uint32_t*>(c->nodes.d.e_pk + index) + 1, &w, 4, hipMemcpyHostToDevice));
        return ESC_OK;
    case 2:
        if (region_group(index) < 0 || value < 1 || value > 7) return ESC_E_INVAL;
        HIP_TRY(hipMemcpy(&w, c->d_g_memb + index, 4, hipMemcpyDeviceToHost));
        w ^= (uint32_t)value << MEMB_FLAG_SHIFT;
        HIP_TRY(hipMemcpy(c->d_g_memb + index, &w, 4, hipMemcpyHostToDevice));
        return ESC_OK;
    case 3:
        if (region_group(index) < 0 || region_group(index) != region_group(index + 1)) return ESC_E_INVAL;
        HIP_TRY(hipMemcpy(&w, c->d_g_memb + index, 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&w2, c->d_g_memb + index + 1, 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(c->d_g_memb + index, &w2, 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->d_g_memb + index + 1, &w, 4, hipMemcpyHostToDevice));
        return ESC_OK;
    case 4: {
        uint32_t* o = c->d_occ_local ? c->d_occ_local : c->d_occ;
        if (!c->placed || !o || index >= 2 * c->n_entries || value < 0 || value > (int64_t)0xFFFFFFFF) return ESC_E_INVAL;
        if (!live_entry(index % c->n_entries)) return ESC_E_INVAL;   // a word K7 reads
        w = (uint32_t)value;
        HIP_TRY(hipMemcpy(o + index, &w, 4, hipMemcpyHostToDevice));
        return ESC_OK;
    }
    case 5:
        if (!c->touch_on || index >= c->nblk || value < 0 || value >= slot_stride(c) / FC_COL) return ESC_E_INVAL;
        if (!((c->h_touch[(size_t)index * c->touch_tw + (size_t)(value >> 5)] >> (value & 31)) & 1u)) return ESC_E_INVAL;
        c->h_touch[(size_t)index * c->touch_tw + (size_t)(value >> 5)] &= ~(1u << (value & 31));
        return ESC_OK;
    case 6:
        if (index >= c->n_nodes || (c->h_nflags[index] & ESC_NF_ABSENT)) return ESC_E_INVAL;
        HIP_TRY(hipMemcpy(&w, c->nodes.flags + index, 4, hipMemcpyDeviceToHost));
        w ^= ESC_NF_TRACKED;
        HIP_TRY(hipMemcpy(c->nodes.flags + index, &w, 4, hipMemcpyHostToDevice));
        return ESC_OK;
    case 7:
        if (index >= c->gi.G) return ESC_E_INVAL;
        HIP_TRY(hipMemcpy(&c->nodes.d.gnode[index].first_cpu, &value, 8, hipMemcpyHostToDevice));
        return ESC_OK;
    case 8:
        if (index >= c->n_nodes || (c->h_nflags[index] & ESC_NF_ABSENT)) return ESC_E_INVAL;
        c->h_ncpu[index] = value;
        return ESC_OK;
    case 9:
        if (index >= c->n_nodes || !(c->h_nflags[index] & ESC_NF_ABSENT)) return ESC_E_INVAL;
        c->h_nflags[index] &= ~ESC_NF_ABSENT;
        return ESC_OK;
    default:
        return ESC_E_INVAL;
    }
}
#endif

}  // extern "C"
