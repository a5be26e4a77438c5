// esc_ctx.h — the context behind the C ABI, private to the host runtime's files:
//   esc_runtime.hip   the context, the decision step, the loaders, the ordering, the events,
//                     reaping
//   esc_rebuild.hip   the device rebuild of the node side, the node table's compaction, the audit
//   esc_pod_grow.hip  the pod classes grown on the device (esc_pods_grow, esc_pods_room)
//   esc_pod_compact.hip  the pod side re-laid on the device (esc_pods_compact, esc_pods_slack,
//                     esc_pod_where)
//   esc_pod_audit.hip  the pod side's read-only audit (esc_audit_pods)
//   esc_pod_verify.hip  the resident pods compared with a caller's batch (esc_pods_verify,
//                     esc_pods_live_ids) and its kernel
//   esc_node_verify.hip  the resident nodes compared with a caller's batch (esc_nodes_verify,
//                     esc_nodes_live_ids) and its kernel; the compare rule is esc_node_verify.h
// Everything else (esc_multi.hip, esc_list.hip, the packer, the generator) sees esc_ctx as
// opaque.  Helpers that cross a file are declared at the end, each defined in the file of its
// subsystem; the small ones are inline here.
#pragma once

#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <new>
#include <thread>
#include <type_traits>
#include <string>
#include <vector>

#include "esc_internal.h"
#include "esc_kernels.h"
#include "esc_multi.h"
#include "esc_node_layout.h"
#include "esc_pod_layout.h"

#ifndef ESC_MEASURE
#define ESC_MEASURE 0   // 1: the measurement library (Makefile ABLATIONS=1) reads its knobs
#endif

namespace esc {

constexpr int MAX_STAGES = 10;
constexpr int32_t HTOT_MAX_GROUPS = 1024;   // K4 writes the totals records to host memory (<= 104 KB)

#define HIP_TRY(x)                                              \
    do {                                                        \
        hipError_t e_ = (x);                                    \
        if (e_ != hipSuccess) return fail_hip(e_, #x);          \
    } while (0)

template <class T>
hipError_t dalloc(T** p, size_t n) {
    *p = nullptr;
    if (n == 0) n = 1;
    return hipMalloc(reinterpret_cast<void**>(p), n * sizeof(T));
}

// A device copy of a host vector.
template <class T>
hipError_t dcopy(T** p, const std::vector<T>& v) {
    const hipError_t e = dalloc(p, v.size());
    return e != hipSuccess || v.empty() ? e : hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

template <class T>
void dfree(T*& p) {
    if (p) hipFree(p);
    p = nullptr;
}

struct PodBuf {
    uint32_t* kb = nullptr;                      // K blocks (tile-major K section)
    uint32_t *flags = nullptr, *cpu0 = nullptr, *pair0 = nullptr, *xp = nullptr, *xc_base = nullptr,
             *xp_base = nullptr, *big = nullptr;
    int64_t *mem0 = nullptr, *xc_cpu = nullptr, *xc_mem = nullptr;
    PodClass* cls = nullptr;
    void release() {
        dfree(kb); dfree(flags); dfree(cpu0); dfree(pair0); dfree(xp); dfree(xc_base); dfree(xp_base); dfree(big);
        dfree(mem0); dfree(xc_cpu); dfree(xc_mem); dfree(cls);
    }
};

// What is derived from the node table and the layout (esc_node_layout.h): the buffers a
// rebuild builds anew and swaps in as one (esc_nodes_rebuild).
struct NodeDerived {
    // pair-major entries, pieces, K2 rows
    uint32_t *e_flags = nullptr, *e_node = nullptr, *piece_off = nullptr, *piece_pair = nullptr, *pp_off = nullptr;
    uint32_t* span_off = nullptr;                // K2 waves' piece ranges
    uint32_t* span_e = nullptr;                  // and their entry ranges
    int64_t *e_cpu = nullptr, *e_mem = nullptr, *rows = nullptr;
    uint4* e_pk = nullptr;                       // the entries packed 16 B each (NodeDev::e_pk)
    GroupNode* gnode = nullptr;
    // the extra labels (compacted by a rebuild), their offsets and the tracker's per-node index
    uint32_t *xl = nullptr, *xl_off = nullptr, *trk_start = nullptr;
    void release() {
        dfree(gnode);
        dfree(e_flags); dfree(e_node); dfree(piece_off); dfree(piece_pair); dfree(pp_off); dfree(span_off); dfree(span_e);
        dfree(e_cpu); dfree(e_mem); dfree(rows); dfree(e_pk);
        dfree(xl); dfree(xl_off); dfree(trk_start);
    }
};

struct NodeBuf {
    // node table (snapshot order), tracker by (node, group)
    uint32_t *flags = nullptr, *label0 = nullptr;
    int64_t *cpu = nullptr, *mem = nullptr, *created = nullptr;
    int32_t *trk_node = nullptr, *trk_group = nullptr;
    NodeDerived d;
    void release() {
        dfree(flags); dfree(label0); dfree(cpu); dfree(mem);
        dfree(created); dfree(trk_node); dfree(trk_group);
        d.release();
    }
};

constexpr uint32_t STALE_PODS = 1, STALE_NODES = 2;

}  // namespace esc

struct esc_ctx {
    int device = -1, rank = 0, world = 1;
    bool has_device = false;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int cu_count = 0;
    esc::GroupIndex gi;
    std::vector<esc::GroupParams> params;
    // device group tables
    uint8_t* d_dry = nullptr;
    esc::GroupParams* d_params = nullptr;
    uint32_t *d_gpair = nullptr, *d_node_code = nullptr, *d_code_list = nullptr;
    uint32_t* d_gslot = nullptr;
    // snapshot
    std::vector<esc::PodBuf> pods;
    int n_replicas = 1, cur = 0;
    int64_t k_weight = 0;
    int64_t n_pods = 0, k_tiles = 0, c_tiles = 0, n_xc = 0, n_xp = 0, pod_offset = 0, n_big = 0;
    int32_t n_cls = 0;
    bool pods_loaded = false;
    esc::NodeBuf nodes;
    int64_t n_nodes = 0, n_xl = 0, n_trk = 0, node_lo = 0, node_hi = 0;
    int64_t n_entries = 0, n_pieces = 0, pc_lo = 0, pc_hi = 0, node_bytes = 0, n_spans = 0;
    int64_t ts_min = 0, ts_max = 0;
    bool nodes_loaded = false;
    // every node's allocatable cpu is in [0, 2^32): K2 reads the packed 16-B entries (node
    // events that break it switch K2 back to the three entry arrays, dropping the graphs)
    bool e_pk_ok = false;
    uint32_t q_lo = 0, q_hi = 0;                              // the group pairs this rank owns (§7)
    std::vector<uint32_t> q_bounds;                           // every rank's first owned pair, + n_gp
    std::vector<int64_t> pair_live;                           // group pair -> live node entries
    // work
    int nblk = 0;
    uint64_t* d_pod_part = nullptr;
    uint32_t *d_col_off = nullptr, *d_col_groups = nullptr;   // K3: groups by pod slot column
    int k3_ablate = 0;                                        // ESC_K3_ABLATE (timing-only knob)
    bool tail_trace = false;                                  // ESC_TAIL_TRACE (measurement library)
    uint64_t* d_ttrace = nullptr;                             // tail + node-groups block timestamps
    int64_t ttrace_cap = 0, ttrace_tail = 0, ttrace_ng = 0;   // words; blocks of the last traced step
    int64_t* d_wide_pod = nullptr;
    int64_t* d_k1seg = nullptr;                               // K1 work plan [nblk][K1_SEGS][2]
    // Compact K1 flush: the pod-slot columns each workgroup's share touches
    // (bitmap of touch_tw u32 per workgroup, kept current by pod upserts), as per-workgroup
    // {column, entry} lists and per-column entry ranges on the device.
    bool touch_on = false;
    bool full_flush = false;                                  // ESC_K1_FULL_FLUSH=1 (measurement knob)
    int touch_tw = 0;
    std::vector<uint32_t> h_touch;
    std::vector<std::array<int64_t, 3>> h_tile_wg;            // {first tile, end tile, workgroup}, sorted
    uint32_t* d_touch = nullptr;
    uint2* d_wg_cols = nullptr;
    uint32_t* d_wg_off = nullptr;
    uint32_t* d_col_rows = nullptr;
    std::vector<double> k1_share;                             // calibrated K1 shares (esc_k1_calibrate)
    uint64_t* d_k1_trace = nullptr;                           // K1 per-workgroup timestamps (esc_k1_trace)
    int64_t* d_trk_acc = nullptr;                             // [G][TA_K] dry-mode tracked sums
    int64_t* d_pwords = nullptr;                              // active exchange buffer [world * own_cap][PW_K]
    int64_t* own_pwords = nullptr;                            // the context-owned one
    int64_t* d_nwords = nullptr;                              // [G][NW_K] node words (exact for owned groups),
                                                              // right after own_pwords (one allocation)
    // Owner-major exchange rows: group g's pod words at row h_xs[g] = owner *
    // own_cap + its index among the owner's groups, so one ncclReduceScatter hands every
    // owner the exact sums of its own groups; h_own = this rank's groups (ascending).
    int32_t own_cap = 0, own_first = 0;
    bool own_seq = true;                                      // h_own is own_first + i
    std::vector<uint32_t> h_own, h_xs;
    uint32_t *d_own = nullptr, *d_xs = nullptr;
    esc_group_decision* d_dec = nullptr;                     // full records (device)
    esc::DecCompact* d_cdec = nullptr;                        // compact records (device; no zero-copy)
    esc::DecCompact* h_cdec = nullptr;                        // compact records (pinned host)
    esc::DecCompact* h_cdec_dev = nullptr;                    // device view of h_cdec (zero-copy)
    bool zero_copy = true;                                    // K3/K4 write compact decisions to h_cdec
    bool order_in_step = false;                               // K5 ordering inside every decision
    // selections delivered with the decision (esc_set_selections, SelOut): K4 writes every
    // decided group's taint / untaint nodes into h_sel (pinned, zero-copy) as [header, nodes]
    // runs, their offsets into the compact records
    int32_t sel_slack = -1, sel_group_cap = 0;
    uint32_t *h_sel = nullptr, *h_sel_dev = nullptr;
    int64_t sel_words = 0;
    // the last decision enqueued was given a selection target (sel_out): esc_selections reads
    // h_cdec[].sel / h_sel only then.  Cleared by everything that changes or drops the target
    // (esc_set_selections, esc_set_order_in_step, release_sort) and when h_cdec is allocated.
    bool sel_valid = false;
    bool want_metrics = false;                                // K4 also writes the gauges
    esc_group_metrics* d_metrics = nullptr;
    int64_t* bound_pwords = nullptr;                          // caller-bound exchange buffer
    int64_t bound_words = 0;                                  // its size: xw_count when bound
    void* comm = nullptr;                                     // RCCL communicator (esc_comm_init)
    bool work_ready = false;
    // An informer-event batch that failed after its first write (a HIP error mid-apply)
    // leaves host mirrors and device arrays half-updated: decisions and reaping are refused
    // (ESC_E_STATE) until the snapshot is reloaded (STALE_PODS: esc_load_pods, STALE_NODES:
    // esc_load_nodes).  ADVICE r4.
    uint32_t stale = 0;
    // world > 1: a shard step's node groups run with K4 after the exchange (esc_decide); a
    // reduce not followed by a decide leaves them pending (the tail's tracker sums unread)
    bool ng_pending = false;
    bool force_wide = false;
    int k1_variant = 0;                                       // ESC_K1_VARIANT (measurement knob)
    int k1_threads = 0;                                       // ESC_K1_THREADS (measurement knob); 0: 512
    // K pods of a class are laid out in order of pair0 / pod_sort (0: input order), so that a
    // K1 workgroup's share touches few pod-slot columns; ESC_POD_SORT
    uint32_t pod_sort = esc::FC_COL; // one K3 column per bucket (exact pair order serialises K1's LDS atomics: 0.65 ms)
    // graph
    bool use_graph = false;
    std::vector<hipGraphExec_t> graphs;                       // esc_run: whole decision (world 1)
    std::vector<hipGraphExec_t> rgraphs;                      // esc_reduce: the shard's step (world > 1)
    // timing
    bool timing = false;
    hipEvent_t ev[esc::MAX_STAGES] = {};
    hipEvent_t k1t_ev[2] = {};                                // esc_k1_time's own pair (stage events stay readable)
    double stage_ms[esc::MAX_STAGES] = {};
    int n_stage_ev = 0;
    bool pending = false;
    // K5 ordering: the age index (built at load) and the per-decision partition
    uint64_t* d_mkeys[2] = {nullptr, nullptr};               // index build: (group | creation offset)
    uint32_t* d_mvals[2] = {nullptr, nullptr};               //              (node | flags << 28)
    int64_t mcap = 0;                                         // their capacity (memberships)
    bool age_built = false;
    bool age_ok = false;                                      // the last build succeeded (its regions are valid)
    uint32_t *d_hist = nullptr, *d_tot = nullptr;
    // The index's small tables live in ONE allocation, filled by ONE upload per build
    // (build_age_index): sorted starts d_seg, region starts / lengths, chunk tables, the
    // listing's status words, the error word and listed total, the groups' tie flags.
    uint8_t* d_itab = nullptr;
    size_t itab_cap = 0;
    uint32_t *d_total = nullptr, *d_ierr = nullptr;           // (views into d_itab)
    uint32_t* d_g_tie = nullptr;                              // [G] equal creation times in the group (RegionSink::tie)
    uint64_t* d_lstat = nullptr;                              // single-pass listing status words
    int64_t* d_seg = nullptr;
    int64_t n_memb = 0;
    int order_src = 0;
    // group order of the memberships (per-decision 3-way split by class inside each group)
    uint32_t* d_g_memb = nullptr;                             // K5 regions: membership words
    uint32_t *d_grp_off = nullptr, *d_gch_off = nullptr;
    uint64_t* d_ostat = nullptr;                              // k_ord_split status words (x2)
    int ord_parity = 0;                                       // which status array the next ordering uses
    // A look-back that gave up (k_ord_split, OrdFail) sets the pinned word h_oerr; the host
    // reads it after its stream waits: esc_sync reports it once as ESC_E_ORDER and clears it,
    // and esc_group_order refuses (ESC_E_ORDER) until the next ordering is enqueued.
    uint32_t *h_oerr = nullptr, *h_oerr_dev = nullptr;
    bool ord_failed = false;
    // fault injection, measurement library only (esc_debug_*: tests/test_gpu_faults.py): the
    // next n ordering / listing launches give up their look-back at once, the next n event
    // patch applications fail after their host-side writes
    int lb_fail_order = 0, lb_fail_list = 0, fail_patches = 0;
    int fail_grow = 0;                                        // the next n esc_pods_grow fail before their swap
    int fail_compact = 0;                                     // the next n esc_pods_compact fail before their swap
    uint32_t *d_pstart = nullptr, *d_plen = nullptr;
    uint32_t* d_ord = nullptr;                                // K5 output, in the group regions
    esc::OrdChunk* d_pchunks = nullptr;                       // packed chunks of small groups
    int64_t n_pchunks = 0, n_psmall = 0;                      // all / those <= ORD_PCHUNK (first)
    std::vector<uint32_t> h_pstart, h_plen;                   // group regions: start, memberships
    std::vector<uint32_t> h_pcap;                             // every group's region capacity (owned or not)
    std::vector<uint32_t> h_gch_off;                          // group -> its split chunks (big groups)
    int64_t n_gpad = 0;                                       // padded group-order length
    esc::OrdChunk* d_chunks = nullptr;
    int64_t n_chunks = 0;
    uint64_t sort_div = 1;
    int sort_R = 1;
    bool age_exact = false;                                   // this snapshot needs the exact 64-bit keys
    bool sorted = false;
    std::vector<int64_t> h_created;                           // [lo, hi) creation times (tie order)
    // node informer events (§8f rank 1): capacity and host mirrors for in-place add / delete
    int64_t n_cap = 0, xl_used = 0, xl_cap = 0, age_n = -1;
    std::vector<uint32_t> h_label0, h_xl_off, h_xl;           // node labels (pair ids)
    std::vector<uint32_t> h_e_node;                           // pair-major entry -> node (NONE: spare)
    std::vector<uint32_t> pair_next, pair_end;                // group pair -> next spare entry, range end
    std::vector<uint32_t> pair_lo;                            // group pair -> its first entry
    std::vector<uint32_t> h_gn;                               // group regions' nodes (lazy mirror of d_g_memb)
    // per-function drop-ins: the list reducer (esc_list.hip); esc_order_by_creation runs
    // on a one-group list context
    esc_ctx* list_ctx = nullptr;
    esc::ListReducer* lred = nullptr;
    // single-process multi-device context (esc_ctx_create_multi): every call dispatches to
    // its per-device contexts (esc_multi.hip); null for a per-device context
    esc::esc_multi_state* multi = nullptr;
    // incremental snapshot (§8f rank 1): where each loaded pod lives, free K slots
    double spare_frac = 0.0;                                  // esc_set_spare
    esc::hvec<int32_t> pod_cls;                               // by pod id: K class index, -1 C, -2 absent
    esc::hvec<int64_t> pod_pos;                               // K: position in its class; C: C-array index (slot
                                                              // k_tiles * 256 + it: a grown K section moves no C pod)
    std::vector<std::vector<int64_t>> cls_free;               // per K class: free positions
    std::vector<esc::PodClass> h_cls;
    std::vector<int> h_cls_of;                                // signature id -> class index (-1: none)
    std::vector<uint32_t> h_cflags;                           // C-section flags (deletes keep the counts)
    std::vector<int64_t> c_free;                              // free C slots (C-array index), room in h_cflags
    std::vector<uint32_t> h_cused;                            // a C slot's pod's own records | pairs << 16
    std::vector<uint32_t> h_xc_base, h_xp_base;               // C tiles' record / pair offsets
    int64_t live_pods = 0, live_xc = 0, live_xp = 0;
    int64_t live_c_pods = 0;                    // of them in C slots (their own, or parked there by a full class)
    int64_t live_pk_pods = 0;                   // of them in packed K classes (either size; no records there)
    int64_t live_p8_pods = 0, live_p8_xp = 0;   // of them in packed small K classes, their extra pairs
    int64_t live_inert_pods = 0, live_inert_xp = 0;   // of those in inert classes (K1 streams none of them)
    int64_t c_tiles_loaded = 0;                 // C tiles of loaded pods (the spare C tiles excluded)
    // node state mirrors for esc_nodes_update
    std::vector<uint32_t> h_nflags;
    std::vector<int64_t> h_ncpu, h_nmem;
    std::vector<uint32_t> ne_off, ne_pos;                     // node -> its pair-major entry positions
    // The reaping occupancy words, maintained by pod / node events once esc_load_placement
    // counted them (K6 no longer runs per call): d_occ at one rank; with several ranks the
    // maintained local words are d_occ_local and d_occ is the exchange buffer.
    uint32_t* d_occ_local = nullptr;
    uint32_t* d_ne_off = nullptr;                             // device copies of ne_off / ne_pos
    uint32_t* d_ne_pos = nullptr;
    int64_t ne_dev_nodes = -1, ne_dev_pos = -1;
    std::vector<esc::GroupNode> h_gnode;
    // dry-mode taintTracker mirror (§8f rank 4): (node << 32 | group), sorted, unique
    std::vector<uint64_t> h_trk;
    int64_t trk_cap = 0;                                      // device capacity of trk_node/_group
    // scale-down reaping (§8f rank 2): pods bound to nodes, per-node taint times
    bool placed = false;                                      // pod binding current
    bool node_removal = false;                                // taint times / no-delete loaded
    esc::PodRef* d_refs = nullptr;
    uint32_t* d_e_pair = nullptr;
    uint32_t *d_nrun_off = nullptr, *d_nrun_len = nullptr, *d_occ = nullptr, *d_rm_off = nullptr,
             *d_rm_list = nullptr;                             // d_occ: [2][n_entries] (pair, default)
    // host mirror of the placement: runs per node (capacity offsets, lengths), the pod at
    // each run position, each pod's node and run position (pod events keep them current)
    std::vector<uint32_t> h_run_off, h_run_len, h_pod_node;
    std::vector<int32_t> h_run_pod;
    std::vector<int64_t> h_pod_rpos;
    int64_t *d_taint_s = nullptr, *d_soft = nullptr, *d_hard = nullptr;
    uint8_t* d_no_delete = nullptr;
    esc::RmRec* d_rm_out = nullptr;
    std::vector<uint32_t> h_rm_off;                           // [G + 1]
    esc::RmRec* h_rm = nullptr;                               // K7 results (pinned copy)
    uint8_t* h_istage = nullptr;                              // age-index build uploads (pinned)
    size_t istage_cap = 0;
    uint8_t* h_pstage = nullptr;                              // esc_audit_pods' staging (pinned; two halves + the
    hipEvent_t pstage_ev[2] = {};                             // report), made at the first call; a half's last use
    int64_t* h_words = nullptr;                               // esc_results' pod + node words (pinned)
    size_t words_cap = 0;
    // Small contexts (G <= HTOT_MAX_GROUPS): K4 writes every decided group's totals record
    // straight to pinned host memory with its decision (<= 104 KB over PCIe), so esc_results
    // copies nothing; tot_dec = the last enqueued step decided (the records are current).
    esc_group_totals* h_tot = nullptr;
    esc_group_totals* h_tot_dev = nullptr;
    bool tot_dec = false;
    std::vector<int64_t> h_soft, h_hard;                      // grace periods last uploaded
    bool rm_valid = false;                                    // esc_try_remove results current
    int64_t rm_nodes = -1;                                    // node count the reaping buffers are sized for
    // newly registered nodes (calculateNewNodeMetrics, controller.go:157-189): the per-node
    // instantiation time belongs to the node table (esc_load_nodes: every slot unknown)
    int64_t *d_inst = nullptr, *d_nn_since = nullptr;         // [n_cap], [G]
    uint32_t *d_nn_off = nullptr, *d_nn_list = nullptr;       // list offsets per group (as h_rm_off), the lists
    esc_new_nodes* d_nn_out = nullptr;                        // [G]
    std::vector<uint32_t> h_nn_off;                           // [G + 1]
    std::vector<int64_t> h_nn_new;                            // [G] n_new of the last eval (list lengths)
    bool nn_valid = false;                                    // esc_new_nodes_eval results current
};

namespace esc {

inline int bit_width(uint64_t v) {
    int b = 0;
    while (v) { ++b; v >>= 1; }
    return b;
}

// A node's allocatable cpu fits K2's packed entry (NodeDev::e_pk).
inline bool entry_cpu_packs(int64_t cpu) { return cpu >= 0 && cpu <= (int64_t)0xFFFFFFFF; }

// K1 partial row stride: the pod slots (one per group pair + the default filter's)
// rounded up to whole K3 columns.
inline int64_t slot_stride(const esc_ctx* c) { return ((int64_t)c->gi.n_gp + 1 + FC_COL - 1) / FC_COL * FC_COL; }

// Does this rank own group g's node side (its pair in [q_lo, q_hi))?
inline bool owns_group(const esc_ctx* c, uint32_t g) {
    const uint32_t q = c->gi.gpair[g];
    return q >= c->q_lo && q < c->q_hi;
}

// the group pair of pair-major entry e (NONE: a pair no group uses)
inline uint32_t entry_pair(const esc_ctx* c, uint32_t e) {
    const uint32_t n_gp = c->gi.n_gp;
    if (!n_gp || e >= c->pair_end[n_gp - 1]) return NONE;
    const uint32_t q = (uint32_t)(std::upper_bound(c->pair_lo.begin(), c->pair_lo.end(), e) - c->pair_lo.begin()) - 1;
    return e < c->pair_end[q] ? q : NONE;
}

// Host threads for the load-time layout passes: ESC_HOST_THREADS, else OMP_NUM_THREADS (the
// GPU box sets 16, its CPU share per GPU), else min(16, hardware threads).
inline int host_threads() {
    int n = 0;
    for (const char* e : {"ESC_HOST_THREADS", "OMP_NUM_THREADS"})
        if (const char* v = std::getenv(e)) { n = std::atoi(v); if (n > 0) break; }
    if (n <= 0) n = std::min<int>(16, std::max(1u, std::thread::hardware_concurrency()));
    return std::max(1, std::min(n, 64));
}

// f(t, lo, hi) over T contiguous chunks of [0, n), one host thread each (in order for T = 1)
template <class F>
void par_chunks(int64_t n, int T, F&& f) {
    if (T <= 1 || n < 4096) {
        f(0, (int64_t)0, n);
        return;
    }
    std::vector<std::thread> th;
    th.reserve(T);
    for (int t = 0; t < T; ++t) th.emplace_back([&, t] { f(t, n * t / T, n * (t + 1) / T); });
    for (auto& x : th) x.join();
}

// ---- esc_runtime.hip
// Sets esc_strerror's text for `code` (ESC_E_HIP, ESC_E_COMM) and returns the code.
int32_t fail_fmt(int32_t code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
GroupDev group_dev(const esc_ctx* c);
PodDev pod_dev(const esc_ctx* c, int replica);
NodeDev node_dev(const esc_ctx* c);
void drop_graphs(esc_ctx* c);
void release_sort(esc_ctx* c);
int32_t build_age_index(esc_ctx* c);
void commit_layout(esc_ctx* c, NodeLayout& L, bool pk_ok);
RemovalDev occ_dev(const esc_ctx* c);
int32_t ensure_ne_dev(esc_ctx* c);
int32_t occ_recount(esc_ctx* c);
void release_work(esc_ctx* c);
int32_t ensure_work(esc_ctx* c);
// Rewrites the PodRefs of the bound pods among ids from their present slots (esc_pods_compact:
// the pods that left the C section).
int32_t refresh_podrefs(esc_ctx* c, std::vector<int64_t>& ids);
// A pod event batch as esc_pods_upsert and esc_pods_grow both read it: validated, each pod's
// first record / extra pair in the batch and its class id (pod_class_id).
struct BatchShape {
    std::vector<int64_t> rof, pof;
    std::vector<int16_t> sid;
};
int32_t batch_shape(const esc_ctx* c, const int64_t* ids, const esc_pod_soa* p, BatchShape& b);
// Does batch pod `id`, bound for K class ci, need a new position there (no: it is in ci already)?
inline bool k_needs_pos(const esc_ctx* c, int64_t id, int ci) {
    return !(id < (int64_t)c->pod_cls.size() && c->pod_cls[id] == ci);
}
// Does batch pod `id` with flags f, bound for the C section, stay in its own C slot?
inline bool c_keeps_slot(const esc_ctx* c, int64_t id, uint32_t f) {
    return id < (int64_t)c->pod_cls.size() && c->pod_cls[id] == -1 && c_room(c->h_cflags[c->pod_pos[id]], f);
}

// ---- the pinned staging buffer of the read-only passes (esc_audit_pods, esc_pods_verify): two
// halves of PSTAGE_HALF bytes used in turn and a report's words behind them, kept on the context
constexpr size_t PSTAGE_HALF = size_t(4) << 20;
constexpr size_t PSTAGE_REP = 4096;                      // the report's words behind the halves
inline int32_t pstage_ensure(esc_ctx* c) {
    if (c->h_pstage) return ESC_OK;                      // (the buffer last: it marks the three as made)
    for (hipEvent_t& e : c->pstage_ev)
        if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->h_pstage), 2 * PSTAGE_HALF + PSTAGE_REP));
    return ESC_OK;
}
// The bytes from p to the end of the device allocation p lies in, as the runtime recorded it
// (0: not a device allocation).  An allocation may be rounded up past what was asked for; it is
// the bound that keeps a read inside mapped memory whatever the host mirrors say.
inline int64_t dev_bytes_from(const void* p) {
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (!p || hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) return 0;
    return (int64_t)size - (int64_t)(static_cast<const char*>(p) - static_cast<const char*>(base));
}

// Device scratch of one call, freed on every way out.
struct PodAuditScratch {
    std::vector<void*> bufs;
    ~PodAuditScratch() { for (void* p : bufs) hipFree(p); }
    template <class T>
    hipError_t get(T** p, size_t n) {
        const hipError_t e = dalloc(p, n);
        if (e == hipSuccess) bufs.push_back(*p);
        return e;
    }
};

// The staging halves in turn.  next(): the half to fill (after its last use is over);
// send(dst, bytes): the half's first bytes to device memory dst (null: the half's own chunk
// buffer); done(): everything enqueued so far is the half's last use.
struct Stager {
    esc_ctx* c;
    hipStream_t st;
    uint8_t* dev[2] = {nullptr, nullptr};
    bool used[2] = {false, false};
    int h = 1;
    uint8_t* host() const { return c->h_pstage + (size_t)h * PSTAGE_HALF; }
    uint8_t* chunk() const { return dev[h]; }
    int32_t next() {
        h ^= 1;
        if (used[h]) HIP_TRY(hipEventSynchronize(c->pstage_ev[h]));
        return ESC_OK;
    }
    int32_t send(void* dst, size_t at, size_t bytes) {
        if (bytes) HIP_TRY(hipMemcpyAsync(dst ? dst : dev[h] + at, host() + at, bytes, hipMemcpyHostToDevice, st));
        return ESC_OK;
    }
    int32_t done() {
        HIP_TRY(hipEventRecord(c->pstage_ev[h], st));
        used[h] = true;
        return ESC_OK;
    }
};

}  // namespace esc
