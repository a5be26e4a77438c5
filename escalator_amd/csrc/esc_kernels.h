// esc_kernels.h — device-side argument blocks and launch wrappers (esc_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "esc_common.h"
#include "esc_kblock.h"

namespace esc {

// Device view of a pod shard.  Two sections, made at load (esc_load_pods; sums are
// order-independent):
//  - K: pods with at most 3 extra container records and at most 3 extra pairs, grouped by
//    record signature into 256-pod tiles, each tile one contiguous block (kb: esc_kblock.h);
//  - C: the others, in 64-pod tiles (1 per lane) in their own SoA arrays (flags .. pair0
//    indexed from the C section's start), whose extra records are contiguous per tile
//    (xc_base / xp_base into xc_cpu / xc_mem / xp).
// Pod slot numbering (the host's and the reaping's): K pod s of tile t = t * 256 + s, C pod
// i = k_tiles * 256 + i.  Padding pods carry ESC_PF_DAEMONSET.
struct PodDev {
    const uint32_t* kb;        // K blocks
    const uint32_t* flags;     // C section
    const uint32_t* cpu0;
    const int64_t*  mem0;
    const uint32_t* pair0;
    const int64_t*  xc_cpu;
    const int64_t*  xc_mem;
    const uint32_t* xp;
    const PodClass* cls;       // [n_cls] K classes, in tile order
    const uint32_t* xc_base;   // [c_tiles + 1] extra-container offset of each C tile
    const uint32_t* xp_base;   // [c_tiles + 1] extra-pair offset
    // K1 work plan (ensure_work): per workgroup up to K1_SEGS runs of one
    // class, {t0 | class << 48, t1} (t1 == 0: unused), balanced in work weight, at most two
    // class boundaries per workgroup.  Null: plan_k1 could not place every class; K1 then
    // walks equal weight ranges per workgroup and flushes whole rows.
    const int64_t* seg;
    // Compact K1 flush: workgroup b writes only the pod-slot columns its share
    // touches, wg_cols[b * n_col + i] = {column, destination} for i < wg_off[b] (n_col = the
    // columns of a partial row), each destination a 64-word partial (32 cpu|count words, 32
    // mem words) that K3 finds through FoldPlan::col_rows.  Null: every row flushed whole (no
    // static plan).
    const uint2* wg_cols;
    const uint32_t* wg_off;
    int32_t n_cls;
    int64_t k_tiles;           // K section: pods [0, k_tiles * 256)
    int64_t k_weight;          // total work weight of the K tiles (K1 splits it evenly)
    int64_t c_tiles;           // C section: pods [k_tiles * 256, + c_tiles * 64)
};

// Device view of the node snapshot.
//
// Two layouts of the same records, both resident on every rank:
//  - the node table in snapshot order: flags, label pairs, allocatable, creation time.
//    The K5 age index is listed from it (nodes [lo, hi) = the whole table), keeping the
//    memberships of this rank's groups; K3 reads allNodes[0]'s capacity.
//  - the pair-major entries: one entry per (label pair, node), sorted by (pair, node)
//    at load (e_flags / e_cpu / e_mem / e_node).  NewNodeLabelFilterFunc
//    (node_group.go:278) is "(K_g, V_g) in the node's label pairs", so a group's members
//    are exactly the entries of its pair, in snapshot order.  K2 reduces the entries per
//    piece (a run of entries of one pair that crosses no multiple of PIECE_ALIGN entries:
//    K2's spans of whole pieces come out full); this rank reduces the pieces
//    [pc_lo, pc_hi) of the pairs [q_lo, q_hi) it owns.  K3 joins each group to its pair's
//    pieces.
// (PIECE_ALIGN, NODE_PIECE, NODE_SPAN and GroupNode: esc_common.h, shared with the host's
// layout plan, esc_node_layout.h.)
struct NodeDev {
    const GroupNode* gnode;    // [G] per-group facts fixed by the snapshot
    const uint32_t* flags;
    const uint32_t* label0;
    const int64_t*  cpu;
    const int64_t*  mem;
    const int64_t*  created;
    const uint32_t* xl;
    const uint32_t* xl_off;    // [n_nodes] offset of each node's extra labels
    const int32_t*  trk_node;  // dry-mode tracker, sorted by (node, group)
    const int32_t*  trk_group;
    const uint32_t* trk_start; // [n_nodes] first tracker entry of a tracked node
    int64_t n_trk;
    int64_t lo, hi;            // K5's node range
    // pair-major entries
    const uint32_t* e_flags;
    const int64_t*  e_cpu;
    const int64_t*  e_mem;
    // the same entries as one 16-B record each (flags, cpu as u32, mem lo, mem hi) when every
    // node's allocatable cpu is in [0, 2^32) (checked at load and by every node event; null
    // otherwise): K2 streams one load per entry instead of three, 16 B instead of 20
    const uint4*    e_pk;
    const uint32_t* e_node;    // snapshot index of the entry's node
    const uint32_t* piece_off; // [n_pieces + 1] entry offsets
    const uint32_t* piece_pair;// [n_pieces]
    const uint32_t* pp_off;    // [n_gp + 1]: pieces of group pair q are [pp_off[q], pp_off[q+1])
    // K2 work: span w = this rank's group-pair pieces [span_off[w], span_off[w + 1]), at
    // most NODE_SPAN entries of whole pieces, one wave per span
    const uint32_t* span_off;  // [n_spans + 1]
    const uint32_t* span_e;    // [n_spans + 1] the spans' entry bounds (piece_off[span_off[w]])
    int64_t n_pieces, pc_lo, pc_hi, n_spans;
    // the group pairs this rank owns: their pieces [pc_lo, pc_hi) are its K2
    // work, their groups' memberships its K5 age index; [0, n_gp) with one rank
    uint32_t q_lo, q_hi;
};

// K2 output row per piece (int64 words, stored word-major: rows[word * n_pieces + piece]).
// Sums travel split lo32 / hi (arithmetic) so they add without wrapping; counts are
// packed 21 bits each (a piece has <= NODE_PIECE entries).
enum NodeRow : int {
    NR_UCPU_LO = 0, NR_UCPU_HI, NR_UMEM_LO, NR_UMEM_HI,    // untainted members (wet classes)
    NR_ACPU_LO, NR_ACPU_HI, NR_AMEM_LO, NR_AMEM_HI,        // every member (dry mode)
    NR_COUNTS,                                             // unt | taint << 21 | cord << 42
    NR_K
};
constexpr int NR_CNT_BITS = 21;
constexpr uint64_t NR_CNT_MASK = (uint64_t(1) << NR_CNT_BITS) - 1;

struct GroupDev {
    const uint8_t*  dry;
    const GroupParams* params;
    const uint32_t* gpair;     // [G] group -> its pair id (K3 joins pod slots / node pieces to groups)
    const uint32_t* node_code; // [n_gp] pair id -> group code (K5)
    const uint32_t* code_list; // CODE_MULTI lists: [count, g...]
    const uint32_t* gslot;     // [G] the group's pod slot: its pair, or n_gp for the default group
    const uint32_t* xs;        // [G] the group's row of the exchanged pod words (owner-major)
    esc_group_metrics* metrics; // [G] gauges written by K4, or null (esc_set_metrics)
    esc_group_totals* htot;    // [G] totals written by K4 with the decision (pinned host memory,
                               // small contexts: esc_results then copies nothing), or null
    int64_t sp;                // K1 partial row stride: pod slots rounded up to FC_COL
    uint32_t n_gp;             // pod slots: pair ids [0, n_gp) + the default filter's slot n_gp
    int32_t G;
    uint32_t default_group;    // NONE when no group is named "default"
};

// Wide (exact, any-range) pod accumulators: global int64 atomics, one row per pod slot.
// K3 reads them and resets a non-zero row (every reader of a slot is in one K3 workgroup).
enum WidePod : int { WP_CPU_LO = 0, WP_CPU_HI, WP_MEM_LO, WP_MEM_HI, WP_CNT, WP_K };
// Per dry-mode group: the tracked members' count and split sums (K2 adds, K3 resets).
enum TrkAcc : int { TA_CNT = 0, TA_CPU_LO, TA_CPU_HI, TA_MEM_LO, TA_MEM_HI, TA_K };

// variant: 0 = the product K1 (one static share per workgroup); 7 = the product kernel without
// the plan (PodDev::seg null: the weight-range walk and the full-row flush, exact); 3-6,
// 9-13 = timing ablations (3-6 exact; 9-13 wrong results), present in the measurement
// library only.  The variant is chosen by ESC_K1_VARIANT, which only the measurement
// library reads (scripts/k1_variants.py).
// threads: the workgroup's width.  512 is the product's (8 waves with up to 256 VGPRs, up to 3
// K tiles in flight per wave); 1024 (16 waves with 128 VGPRs; the same share, LDS and results)
// exists in the measurement library only (ESC_K1_THREADS), anything else is refused.
struct DecCompact;
// K1 diagnostics.  trace: per workgroup 8 words (esc_k1_trace; the share calibration reads words
// 0-1): s_memrealtime (100 MHz) at start, after the K tiles, after the C tiles, after the
// flush; HW_ID, XCC_ID.
struct K1Diag {
    uint64_t* trace;
};
// Selections delivered with the decision (esc_set_selections; controller.go:367-383): K4
// also writes, for every group it decides with delta < 0 (and the taint clamp passed) the
// first min(n_to_taint + slack, group_cap) untainted nodes oldest first (taintOldestN's walk,
// scale_down.go:171-205), with delta > 0 the first min(delta + slack, group_cap) tainted
// nodes newest first (untaintNewestN, scale_up.go:118-163; equal creation times by ascending
// index, the ordering's tie rule), copied from the ordering of the same decision into the
// pinned buffer `out` — a block's groups as one contiguous run of [header, nodes...] words
// at the block's own slot (blockIdx.x * 64 * (group_cap + 1): no reservation across blocks)
// — and the run's offset into the compact record's `sel` field.  Header: count | which << 28
// (1 taint, 2 untaint) | SEL_CUT (more wanted than group_cap: the nodes are the walk's first
// ones) | SEL_TIE (a run of equal creation times longer than SEL_TIE_MAX: the nodes are not
// used; in both cases the host continues with esc_group_order).
struct SelOut {
    const uint32_t* ord;       // K5 output: every group's segments
    const int64_t* seg;        // [4G] segment bounds (K5)
    const uint32_t* tie;       // [G] RegionSink::tie: only these groups' untaint lists need the
                               // tie rule (the others copy their segment's prefix as it stands)
    uint32_t* out;             // device view of the pinned selection buffer; null: no selections
    int64_t cap_words;         // out's size (a block whose run does not fit gets SEL_OVERFLOW)
    int32_t slack, group_cap;
};
constexpr uint32_t SEL_NONE = 0xFFFFFFFFu, SEL_OVERFLOW = 0xFFFFFFFEu;   // DecCompact::sel without a run
constexpr uint32_t SEL_COUNT_MASK = (1u << 28) - 1, SEL_CUT = 1u << 30, SEL_TIE = 1u << 31;
constexpr int SEL_TIE_MAX = 64;
// k_node_groups' decision target: null dec = the node words only (a reduce that was never
// decided, esc_reduce).
struct NGDecide {
    const int64_t* pwords;
    esc_group_decision* dec;
    DecCompact* cdec;
    SelOut sel;
    uint64_t* trace = nullptr;         // measurement library: per block {start, end} (esc_debug_tail_trace)
};
// The groups a launch of k_node_groups covers: ids[i] for i < n, or, with null
// ids, the contiguous run first + i (a rank's owned groups).
struct GroupList {
    const uint32_t* ids;
    int32_t n;
    int32_t first;
};
hipError_t launch_pod_reduce(const PodDev& p, const GroupDev& g, int32_t g0, int32_t gw, int nblk, int variant,
                             int threads, uint64_t* part, int64_t* wide, const K1Diag& diag, hipStream_t st);
hipError_t launch_pod_bigtiles(const PodDev& p, const GroupDev& g, const uint32_t* tiles, int64_t n_big,
                               int64_t* wide, hipStream_t st);
// Compact decision record (32 B) that K3 / K4 write to pinned host memory each decision
// instead of the ABI's 64-B esc_group_decision: esc_results rebuilds the full record on the
// host (the cached capacity from its node mirror: allNodes[0]'s allocatable when the group
// has nodes, else the state's, controller.go:207-211) and copies the full record, which
// the kernels also keep in device memory, for a group whose delta or n_to_taint leaves int32.
struct DecCompact {
    double cpu_pct, mem_pct;
    int32_t delta, n_to_taint;
    uint8_t status, branch, taint_status, wide;
    uint32_t sel;              // word offset of the group's selection run (SelOut), or SEL_NONE / SEL_OVERFLOW
};
static_assert(sizeof(DecCompact) == 32, "compact decision is 2 x 16 B");

// K2b + K4 (k_node_groups): the listed groups' final node words from K2's piece rows, then
// (nd.dec != null) their decisions (K4) from the pod words at rows xs[g] (or g).
// Peer exchange of a multi-device context (esc_ctx_create_multi): dst[i] = sum of src[k][i]
// over the n_src buffers (peer-mapped device memory), int64 or uint32 words.
hipError_t launch_peer_sum64(const int64_t* const* src, int n_src, int64_t* dst, int64_t n, hipStream_t st);
hipError_t launch_peer_sum32(const uint32_t* const* src, int n_src, uint32_t* dst, int64_t n, hipStream_t st);
hipError_t launch_node_groups(const GroupDev& g, const NodeDev& n, const GroupList& list, const int64_t* node_rows,
                              int64_t* trk_acc, int64_t* nwords, const NGDecide& nd, hipStream_t st);
// K3 fold (a role of k_step_tail): the K1 partials of FC_COL pod slots per block.
constexpr int FC_COL = 32;             // pod slots per K3 column (a 256-B piece of each K1 row)
struct FoldPlan {
    const uint64_t* part;              // K1 partials: row b = cc[sp], mem[sp] at part + 2 * sp * b
    int nblk;                          // K1 rows
    int64_t sp;                        // slots per partial row, a multiple of FC_COL
    int64_t n_col;                     // columns (grid)
    const uint32_t* col_off;           // [n_col + 1] the column's groups in col_groups
    const uint32_t* col_groups;        // group ids ordered by pod slot, then id
    const uint32_t* col_rows;          // compact flush: [n_col + 1] partial entries of each column (null: nblk rows)
    int ablate;                        // ESC_K3_ABLATE (timing-only knob)
    uint64_t* trace = nullptr;         // measurement library: per block {start, end, role} (esc_debug_tail_trace)
};
// The pod-slot columns each K1 workgroup's share touches (compact flush): bitmap words of
// tw u32 per workgroup, from the same work plan as K1 (daemonset pods skipped: they add
// nothing; the default filter's column always).
hipError_t launch_touch(const PodDev& p, const GroupDev& g, int nblk, int tw, uint32_t* bits, hipStream_t st);
struct OrdChunk;
// The step's tail in one launch (esc_kernels.hip k_step_tail): the K3 fold into the pod
// words, K2's dry-mode tracker entries (+ its piece rows when `spans`) and,
// with n_small > 0, the K5 ordering of the packed small-group chunks [0, n_small).
// the tail's K2 span blocks (K2_WAVES spans each) and dry-mode tracker blocks for this node view
constexpr int K2_WAVES = 4;
int64_t tail_span_blocks(const NodeDev& n);
int64_t tail_trk_blocks(const NodeDev& n);
hipError_t launch_step_tail(const GroupDev& g, const NodeDev& n, const FoldPlan& f, bool spans, int64_t* wide_pod,
                            int64_t* pwords, int64_t* rows, int64_t* trk_acc, const OrdChunk* chunks, int64_t n_small,
                            const uint32_t* grp_off, const uint32_t* g_memb,
                            uint32_t* vals, int64_t* seg, hipStream_t st);
hipError_t launch_wide_pods(const PodDev& p, const GroupDev& g, int64_t* wide, hipStream_t st);
// §8f rank 2: a loaded pod as seen by NodePodsRemaining, listed per node (runs in
// node order).  p[0..2]: the pod's extra pairs (NONE-padded); a C pod with more than 3
// has POD_REF_INDIRECT in flags and p[0] = offset, p[1] = count into xp.
struct PodRef {
    uint32_t flags, pair0, p[3];
};
constexpr uint32_t POD_REF_INDIRECT = 1u << 31;
// K7's per-group record on the device (esc_removal widened on the host)
struct RmRec {
    uint32_t n_candidates, n_delete;
    int64_t pods_remaining;
};
struct RemovalDev {
    const int64_t* taint_s;    // [n_nodes] escalator-taint time (INT64_MIN: none / unparsable)
    const uint8_t* no_delete;  // [n_nodes]
    const uint32_t* e_pair;    // [n_entries] pair of each pair-major entry
    int64_t n_entries;
    const uint32_t* nrun_off;  // [n_nodes + 1] runs of PodRef per node (capacity)
    const uint32_t* nrun_len;  // [n_nodes] PodRefs in each run
    const PodRef* refs;
    const uint32_t* xp;        // C-pod extra pairs (indirect refs)
    uint32_t* occ_pair;        // [entries] group pods on the node, by the entry's pair
    uint32_t* occ_def;         // [entries] default-filter pods on the node
    const int64_t* soft_ns;    // [G]
    const int64_t* hard_ns;    // [G]
    const uint32_t* rm_off;    // [G] offset of each group's deletable-node list
    uint32_t* rm_list;
    RmRec* out;                // [G]
    int64_t now_ns;
};
hipError_t launch_podref_fill(const PodDev& p, const uint32_t* run_slot, const uint32_t* run_pos, int64_t n, PodRef* refs,
                              hipStream_t st);
// K6: the occupancy words of every live pair-major entry (esc_load_placement; pod and node
// events then keep them current through launch_occ_delta instead of a recount per call).
hipError_t launch_occupancy(const NodeDev& n, const GroupDev& g, const RemovalDev& r, hipStream_t st);
// The occupancy change of n PodRef placements: the PodRef at run position pos[i], on node
// node[i], added (sign +1) to or removed (-1) from the words of the node's entries
// (ne_off / ne_pos: node -> its entry positions).
hipError_t launch_occ_delta(const GroupDev& g, const RemovalDev& r, const uint32_t* ne_off, const uint32_t* ne_pos,
                            const uint32_t* pos, const uint32_t* node, int64_t n, int sign, hipStream_t st);
hipError_t launch_try_remove(const NodeDev& n, const GroupDev& g, const RemovalDev& r, hipStream_t st);  // K7

struct PatchTargets {          // k_patch destinations: 4-byte arrays 0-5, 8-byte arrays 6-11, 2-byte 12-13
    uint32_t* u32[6];
    int64_t* i64[6];
    uint16_t* u16[2];
};
hipError_t launch_patch(const PatchTargets& t, const uint64_t* where, const uint64_t* what, int64_t n, hipStream_t st);
// esc_nodes_facts: node ids[i]'s taint time and no-delete byte, one event per thread (ids unique).
hipError_t launch_node_facts(int64_t* taint_s, uint8_t* no_delete, const int64_t* ids, const int64_t* ev_taint,
                             const uint8_t* ev_nd, int64_t n, hipStream_t st);

// calculateNewNodeMetrics (controller.go:157-189) for every group: k_new_nodes, one wave per
// group over its pair's entries (K7's walk).  A list word is the node's snapshot index, with
// NN_UNKNOWN set when its instantiation time is unknown (node indices are < 2^28, MEMB_NODE_MASK).
constexpr uint32_t NN_UNKNOWN = 1u << 31;
constexpr int64_t NN_BUCKET_NS = 60ll * 1000000000ll;   // metrics.go:190: bounds 60, 120, ..., 1740 s
struct NewNodesDev {
    const int64_t* inst_ns;    // [node-table capacity] instantiation time, Unix ns (INT64_MIN: unknown)
    const int64_t* since;      // [G] lastScaleOut (INT64_MIN: zero time; INT64_MAX: group not evaluated)
    const uint32_t* list_off;  // [G] offset of each group's new-node list (its pair's entry capacity)
    uint32_t* list;
    esc_new_nodes* out;        // [G]
};
hipError_t launch_new_nodes(const NodeDev& n, const GroupDev& g, const NewNodesDev& w, hipStream_t st);
// esc_nodes_instantiated / esc_nodes_delete: inst_ns[ids[i]] = ev_inst[i], or INT64_MIN for
// every listed id when ev_inst is null; one event per thread (ids unique).
hipError_t launch_node_inst(int64_t* inst_ns, const int64_t* ids, const int64_t* ev_inst, int64_t n, hipStream_t st);

// esc_audit: read-only checks of the derived state against its primary tables.  Every check
// adds to its row of `rep` ([ESC_AUD_N][AW_K] int64, AW_FIRST preset to INT64_MAX): counts
// summed and the lowest offending id, reduced per wave, then one relaxed agent-scope atomic per
// wave and word — a deterministic report.  A derived word may be wrong, so every index read
// from one is bounds-checked before it is used (n_cap, n_entries, ne_len, n_trk).
enum AuditWord : int { AW_CHECKED = 0, AW_BAD, AW_FIRST, AW_K };
struct AuditDev {
    int64_t* rep;
    uint32_t* pair_cnt;        // [n_gp] live entries found per group pair (the host compares pair_live)
    uint32_t* memb_cnt;        // [G] live memberships found per region
    int64_t n_cap;             // node-table capacity (slots of flags / cpu / mem / label0 / trk_start)
    int64_t n_entries;
    const uint32_t* e_pair;    // [n_entries] pair of each entry (with a placement), or null
    const uint32_t* ne_off;    // node -> entries map: [n_cap + 1]
    const uint32_t* ne_pos;
    int64_t ne_len;            // words of ne_pos
};
// ENTRY, forward: one block per group pair over its entry range (K7's walk, four waves wide).
hipError_t launch_audit_entries(const NodeDev& n, const GroupDev& g, const AuditDev& a, hipStream_t st);
// ENTRY, reverse: one thread per node slot through the node -> entries map.
hipError_t launch_audit_node_entries(const NodeDev& n, const GroupDev& g, const AuditDev& a, hipStream_t st);
// FIRST: one wave per listed group over its pair's entries (k_try_remove's walk).
hipError_t launch_audit_first(const NodeDev& n, const GroupDev& g, const GroupList& list, const AuditDev& a,
                              hipStream_t st);
// REGION: one block per group over its region [pstart[g], pstart[g + 1]) with plen[g] memberships.
hipError_t launch_audit_regions(const NodeDev& n, const GroupDev& g, const uint32_t* pstart, const uint32_t* plen,
                                const uint32_t* g_memb, const AuditDev& a, hipStream_t st);
// OCC: the recounted words (`fresh`, [2][n_entries]) against the maintained ones over the live entries.
hipError_t launch_audit_occ(const NodeDev& n, const GroupDev& g, const AuditDev& a, const uint32_t* fresh,
                            const uint32_t* kept, hipStream_t st);
// TRACKER: one thread per node slot and per tracker entry.
hipError_t launch_audit_tracker(const NodeDev& n, const GroupDev& g, const AuditDev& a, hipStream_t st);

// esc_audit_pods: the pod side's read-only checks.  `rep` is [ESC_PAUD_N][AW_K]
// as esc_audit's; P is replica 0 (seg / wg_cols / wg_off unused).  Every offset derived from a
// device word or a host mirror is compared with its array's size before it indexes.
struct PodAuditDev {
    PodDev P;
    int64_t kb_words, n_xc, n_xp;      // sizes of P.kb (u32 words), P.xc_cpu / xc_mem, P.xp
    int64_t n_slots;                   // k_tiles * 256 + c_tiles * 64 (a multiple of 32)
    uint32_t* map_bits;                // [n_slots / 32] slots the id map names (zeroed by the host)
    const uint32_t* free_bits;         // [n_slots / 32] slots the free lists name (+ C padding)
    int64_t* rep;
    uint32_t n_gp;
};
// MAP, part 1.  Pod ids [id0, id0 + n): their class index (-1 C, -2 absent) and position, the
// host's class table (n_cls of them) for the tile ranges.
hipError_t launch_paud_map(const PodAuditDev& a, const int32_t* cls, const int64_t* pos, int64_t id0, int64_t n,
                           const PodClass* hcls, int32_t n_cls, hipStream_t st);
// MAP, part 2: every slot in exactly one of the two bitmaps.
hipError_t launch_paud_map_cmp(const PodAuditDev& a, hipStream_t st);
// KSLOT: one workgroup per K tile.
hipError_t launch_paud_kslot(const PodAuditDev& a, hipStream_t st);
// CSLOT: one wave per C tile of [t0, t0 + nt); hflags / hused: the host's flags and counts of
// those tiles' slots, hxc / hxp: the host's offsets [nt + 1] from tile t0.
hipError_t launch_paud_cslot(const PodAuditDev& a, int64_t t0, int64_t nt, const uint32_t* hflags, const uint32_t* hused,
                             const uint32_t* hxc, const uint32_t* hxp, hipStream_t st);
// PODREF: run positions [r0, r0 + n), slot[i] the device slot of the pod bound there (NONE: no
// pod); n_refs: PodRefs in refs.
hipError_t launch_paud_podref(const PodAuditDev& a, const PodRef* refs, int64_t n_refs, const uint32_t* slot, int64_t r0,
                              int64_t n, hipStream_t st);
// n words of a device table against the host's copy of them; a difference at word i is reported
// to `check` as ids[i / per] * mul when ids is given (the host's id of that row), else as i.
hipError_t launch_paud_words(const PodAuditDev& a, int check, const uint32_t* dev, const uint32_t* host, int64_t n,
                             const uint32_t* ids, int per, int64_t mul, hipStream_t st);
// REPLICA: n_bytes of arrays x (replica 0) and y compared 16 B per lane, esz-byte elements
// (4 or 8); code = replica << 56 | array << 48.  The check's n_checked grows by the elements
// the kernel loaded and compared (n_bytes / esz).
hipError_t launch_paud_replica(const PodAuditDev& a, const void* x, const void* y, int64_t n_bytes, int esz, int64_t code,
                               hipStream_t st);


// Ordering (K5), see esc_kernels.hip: the age index (once per snapshot) and the per-decision
// (group, class) partition.
size_t sort_hist_words(int64_t n);   // digit-histogram words one LSD pass over n keys needs
struct OrdChunk {               // K5 per-decision chunk: memberships [start, end) of one group
    uint32_t start, end, group, pad;   // a packed chunk: its first group, and pad = how many
};                                     // groups [group, group + pad) it covers (<= ORD_GCAP)
constexpr uint32_t ORD_CHUNK_DRY = 2u;   // OrdChunk::pad bit of a split chunk: its group is in dry mode
constexpr uint32_t ORD_GCAP = 512;       // groups a packed chunk covers at most (empty ones included)
#ifndef ESC_ORD_CHUNK
#define ESC_ORD_CHUNK 4096         // (timing builds may override)
#endif
constexpr int ORD_CHUNK = ESC_ORD_CHUNK;   // memberships per K5 chunk (three-pass default)
// Every group owns a region of the group-order arrays: its memberships oldest first, then
// padding (the round-up to whole 16-B quads and the spare slots node additions take,
// DESIGN.md §4) — MEMB_PAD_WORD, class 3 from the word alone.  The packed orderings find a
// quad's group from the chunk's region starts (round 6: no group word per slot).
constexpr uint32_t MEMB_PAD = 0x80000000u;   // (a group word's padding bit: ord_class)
// A group region's membership word (g_memb, 4 B): node | the low four flag bits of the node
// as the per-decision split reads them (UNSCHED, TAINTED, TRACKED resolved for the group,
// ABSENT) << MEMB_FLAG_SHIFT — the age index's sort value, kept as is.  One 4-B word per
// membership is all the split reads besides the chunk (round 3 read node, flags and a class
// byte: 9 B).  Nodes < 2^28.  Padding: node 0, ABSENT.
constexpr uint32_t MEMB_FLAG_SHIFT = 28, MEMB_NODE_MASK = (1u << MEMB_FLAG_SHIFT) - 1;
constexpr uint32_t MEMB_PAD_WORD = ESC_NF_ABSENT << MEMB_FLAG_SHIFT;
inline uint32_t memb_word(uint32_t node, uint32_t flags) { return node | ((flags & 0xFu) << MEMB_FLAG_SHIFT); }
// Small groups (region <= ORD_CHUNK) are packed whole into chunks ordered in one pass:
// chunks [0, n_small) of groups with regions <= ORD_PCHUNK, packed up to ORD_PCHUNK
// memberships (more, shorter blocks), then chunks of up to ORD_CHUNK.
constexpr int ORD_PCHUNK = 1024;
hipError_t launch_order_packed(const NodeDev& nd, const OrdChunk* chunks, int64_t n_chunks, int64_t n_small,
                               const uint32_t* grp_off, const uint8_t* dry, const uint32_t* g_memb,
                               uint32_t* vals, int64_t* seg, hipStream_t st);
// Fills the padding of every group's region (after its `len` memberships) with MEMB_PAD_WORD
// and sets the ordering's segment starts (seg[4g + k] = pstart[g], seg[4G] = pstart[G]).
hipError_t launch_region_pad(const uint32_t* pstart, const uint32_t* plen, int32_t G, uint32_t* g_memb, int64_t* seg,
                             hipStream_t st);
// The age index (load time): memberships listed in one pass (per-tile counts, decoupled
// look-back: status = memb_status_words(n) u64 words, zeroed by the caller) with
// (group << R | creation offset) keys and (node | flags) values, LSD-sorted, then written
// into the groups' padded regions; *total = the listed count.
size_t memb_status_words(int64_t n);
// The age index's destination: every group's padded region (k_rs_scatter<FINAL>).
struct RegionSink {
    const int64_t* seg;        // sorted start of group g's memberships (host-computed)
    const uint32_t* pstart;    // region start of group g
    const uint32_t* plen;      // memberships of group g
    uint32_t* g_memb;          // region words (MEMB_FLAG_SHIFT)
    uint32_t* err;             // bit 0: a membership fell outside its group's count; bit 1: a
                               // coarse-key run too long for k_age_fix (rebuild exact)
    int32_t G;
    int R;                     // the group's shift in the key (key = group << R | time bits)
    int fix;                   // coarse keys: the final pass also writes the sorted keys and
                               // k_age_fix reads them — 1 (time bits were dropped): it orders each
                               // run of equal keys exactly and flags the groups with equal times;
                               // 2 (the keys are exact): it only flags the groups of equal-key runs
    uint32_t spins;            // the listing's look-back bound (LOOKBACK_SPINS; err bit 0 on a give-up)
    uint32_t* tie;             // [G] nonzero: two of the group's members share a creation time (the
                               // selections resolve such ties, SelOut); zeroed by the host first
};
// coarse_shift < 0: exact 64-bit keys (group << R | offset); >= 0: 32-bit coarse keys
// (group << (32 - gbits) | offset >> coarse_shift) + the run fix-up (S.R = 32 - gbits).
hipError_t launch_age_sort(const NodeDev& nd, const GroupDev& g, uint64_t* status, uint32_t* total, int64_t n_memb,
                           int64_t cap, int64_t ts_min, uint64_t div, int R, int gbits, int coarse_shift,
                           uint64_t* keys[2], uint32_t* vals[2], uint32_t* hist, uint32_t* tot, const RegionSink& S,
                           hipStream_t st);
// esc_nodes_rebuild: the pair-major entries, the node -> entries map and the compacted extra
// labels re-derived from the resident node table.  The HOST fixes the layout from its counts
// (every pointer marked "layout" below is host-made and uploaded); the device supplies the
// values.  k_entry_fill writes every entry of every piece as a spare one, k_pair_list lists
// one (pair << 32 | node) element per label of every live node at ne_off[node] + j, the
// k_rs_* passes sort the elements by pair alone (stable: nodes stay ascending inside a pair),
// k_entry_place puts sorted element k at its entry.  No kernel waits on another workgroup.
// A pair, node, count or offset that does not fit the layout sets *err and indexes nothing.
struct RebuildDev {
    // the resident node table (read; `flags` also gets its tracker bit set from trk_start)
    uint32_t* flags;
    const uint32_t *label0, *xl_off, *xl;
    const int64_t *cpu, *mem;
    int64_t n_cap, xl_len;                 // table slots; words of xl
    // layout
    const uint32_t* ne_off;                // [n_cap + 1] node -> first element / map slot
    const uint32_t* xl_off_new;            // [n_cap] node -> first word of xl_new
    const uint32_t* trk_start;             // [n_cap] the tracker list's first entry per node
    const uint32_t* start;                 // [n_gp + 1] group pair -> first sorted element
    const uint32_t* pair_lo;               // [n_gp] group pair -> first entry
    const uint32_t *piece_off, *piece_pair;
    int64_t n_pieces, n_elems, n_entries, xl_new_cap;
    uint32_t n_gp, spare_total;            // spare entries of all group pairs (ids >= n_gp sit behind them)
    // built
    uint32_t* xl_new;
    uint32_t *e_flags, *e_node, *e_pair;   // e_pair: null without a placement
    int64_t *e_cpu, *e_mem;
    uint4* e_pk;
    uint32_t* ne_pos;                      // [n_elems]
    uint32_t* err;
};
// elems[2]: n_elems 8-B elements each; hist: sort_hist_words(n_elems); tot: 256 words;
// pair_bits: bits of the largest resident pair id (one 8-bit pass per started byte).
hipError_t launch_nodes_rebuild(const RebuildDev& r, uint64_t* elems[2], uint32_t* hist, uint32_t* tot, int pair_bits,
                                hipStream_t st);
// esc_nodes_compact: the live nodes gathered into a new table in the host's order (k_node_gather,
// one thread per new slot) and every live node's PodRefs moved to its re-cut run (k_run_move,
// one wave per non-empty run).  Everything marked "plan" is host-made and uploaded; nothing is
// written in place.  A source slot or a run that does not fit the buffers sets *err (the
// rebuild's error word) and indexes nothing.
struct CompactDev {
    // the old table and its per-node facts (read); taint_s / no_delete: null without a placement
    const uint32_t *flags, *label0, *xl_off;
    const int64_t *cpu, *mem, *created, *inst, *taint_s;
    const uint8_t* no_delete;
    int64_t n_old;                         // old n_nodes: the slots a source may name
    // plan
    const uint32_t* src_of;                // [n_new] old slot of every new one (NONE: free)
    int64_t n_new;                         // the new capacity
    const uint32_t* moves;                 // [n_moves][3] old PodRef offset, new offset, length
    int64_t n_moves;
    // built
    uint32_t *flags_new, *label0_new, *xl_off_new;   // xl_off_new: the OLD offsets, by new slot
    int64_t *cpu_new, *mem_new, *created_new, *inst_new, *taint_new;
    uint8_t* nd_new;
    const uint32_t* refs_old;              // the PodRef buffers as 4-byte words
    uint32_t* refs_new;
    int64_t refs_old_words, refs_new_words;
    uint32_t* err;
};
hipError_t launch_nodes_compact(const CompactDev& c, hipStream_t st);
// esc_pods_grow: the K blocks moved to the re-cut classes' tile ranges (k_kb_regrow, one
// workgroup per new tile; KbRegrowCls: esc_kblock.h).  Sizes in u32 words; every source and
// destination block is checked against them and a violation sets bits of *err.
struct KbRegrow {
    const uint32_t* old_kb;
    const uint32_t* tmpl;              // the classes' free tiles (KbRegrowCls::tmpl)
    uint32_t* new_kb;
    const KbRegrowCls* tab;
    int64_t old_words, tmpl_words, new_words;
    int32_t n_cls;
    uint32_t* err;
};
hipError_t launch_kb_regrow(const KbRegrow& r, int64_t n_tiles, hipStream_t st);
// esc_pods_compact: the K-holdable C slots classified (k_pc_classify), every
// old K position and re-homed slot keyed (class, bucket) with its source as the element's low
// word (k_pc_keys) and stable-sorted by the key (the age index's LSD passes), the new tiles
// gathered in that order (k_pc_move, one workgroup per new tile), the vacated C slots freed in
// place after the swap (k_pc_cfree).  `old` is the resident replica; sizes in elements.  A
// source, a class or a block that does not fit its buffer sets bits of *err and is not indexed.
struct PodCompactDev {
    PodDev old;
    int64_t n_xc, n_xp;                // sizes of old.xc_cpu / xc_mem and old.xp
    int64_t old_words;                 // old.kb, in u32 words
    const uint32_t* free_bits;         // [ceil(old.k_tiles * 256 / 32)] bit set: the old K slot is free
    const uint32_t* cand;              // [n_cand] the K-holdable C slots (C-array index), ascending
    const uint32_t* cand_used;         // [n_cand] the host's count of the pod's own records | pairs << 16 (h_cused)
    int32_t* cand_id;                  // [n_cand] k_pc_classify: class id (pod_class_id), -1: stays
    const int32_t* cand_cls;           // [n_cand] the host's: new class index, -1: stays
    int64_t n_cand;
    uint32_t n_gp, pod_sort;
    int64_t nbk;                       // buckets per class (pod_buckets)
    // the re-cut K section
    const PodClass* cls;               // [n_cls] the new class table
    const PcCls* tab;                  // [n_cls]
    const uint32_t* tmpl;              // the classes' free tiles
    int64_t tmpl_words;
    int32_t n_cls;
    int64_t k_tiles;                   // new K tiles
    uint32_t* kb;                      // the new K blocks
    int64_t kb_words;
    uint32_t* map_k;                   // [old.k_tiles * 256] old slot -> new position in its class (NONE: free)
    uint32_t* map_c;                   // [n_cand] re-homed slot -> its position (NONE: stays)
    uint32_t* err;
};
hipError_t launch_pc_classify(const PodCompactDev& d, hipStream_t st);
// elems[2]: old.k_tiles * 256 + n_cand 8-B elements each; hist: sort_hist_words of that count;
// tot: 256 words; key_bits: bits of n_cls * nbk.  *sorted: the buffer that holds the order.
hipError_t launch_pc_order(const PodCompactDev& d, uint64_t* elems[2], uint32_t* hist, uint32_t* tot, int key_bits,
                           int* sorted, hipStream_t st);
hipError_t launch_pc_move(const PodCompactDev& d, const uint64_t* sorted, hipStream_t st);
// The C arrays of one replica (written in place): the re-homed slots become free ones.
hipError_t launch_pc_cfree(const PodCompactDev& d, uint32_t* flags, int64_t* xc_cpu, int64_t* xc_mem, uint32_t* xp,
                           hipStream_t st);
// The bounded waits of the decoupled look-backs (k_ord_split, k_memb_keys): HIP does not
// promise dispatch order, so a chunk never waits unboundedly on one that was not dispatched.
// A chunk that waited `spins` probes gives up: it publishes a FAILED status word (never an
// inclusive prefix it could not compute; its successors fail in turn instead of waiting),
// writes none of its output and sets *err (k_ord_split: a pinned host word the runtime reads
// after its stream wait and reports as ESC_E_ORDER, then clears).
constexpr uint32_t LOOKBACK_SPINS = 1u << 22;
struct OrdFail {
    uint32_t* err;             // device view of a pinned host word: set to 1 by a give-up
    uint32_t spins;            // LOOKBACK_SPINS (smaller in measurement builds' tests)
};
// The split groups' ordering in one pass (k_ord_split): ostat = 2 * n_chunks + 1 u64 words,
// zeroed when the chunk table is made: two arrays of status words used by alternate
// decisions (par = 0, 1: a decision clears its chunks' words of the other).
// Output layout of every group (split and packed): untainted forward from the region start,
// tainted newest first backward from the region end; seg[4g..4g+3] = start, start +
// untainted, end - tainted, end.
hipError_t launch_order(const NodeDev& n, const OrdChunk* chunks, int64_t n_chunks, const uint32_t* gch_off,
                        const uint32_t* grp_off, const uint32_t* g_memb, uint64_t* ostat, int par, uint32_t* vals,
                        int64_t* seg, const OrdFail& fail, hipStream_t st);

}  // namespace esc
