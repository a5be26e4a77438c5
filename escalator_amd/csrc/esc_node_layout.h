// esc_node_layout.h — the node side's layout, derived once.
//
// esc_load_nodes and esc_nodes_rebuild lay the pair-major entries out from the same counts,
// and everything downstream (K2, k_node_groups, k_entry_fill, the audit, the event patches)
// rests on their agreeing: the rules live here and nowhere else.  So do the capacity rule of
// the placement's runs (esc_load_placement, esc_nodes_compact) and the compaction's plan.
// Host only, plain C++17, no HIP header: tests/node_layout_check.cpp and
// tests/node_compact_check.cpp build it with the host compiler.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "esc_common.h"

namespace esc {

// Capacity rules (esc_set_spare's fraction f; no spare room at f = 0): the spare entries behind
// a group pair's live ones, the node-table slots for n nodes, the extra-label words for w in use.
inline int64_t spare_entries(int64_t live, double f) { return f > 0 ? (int64_t)std::ceil((double)live * f) + 4 : 0; }
inline int64_t table_slots(int64_t n, double f) { return n + (f > 0 ? (int64_t)std::ceil((double)n * f) + 64 : 0); }
inline int64_t label_words(int64_t w, double f) { return w + (f > 0 ? (int64_t)std::ceil((double)w * f) + 256 : 0); }

// Entries behind the group pairs: `len` consecutive entries of one pair no group selects.
struct TailRun { uint32_t pair; uint64_t len; };

struct NodeLayout {
    // group pair q: entries [pair_lo, pair_end), the live ones first, spare from pair_next on
    std::vector<uint32_t> pair_lo, pair_next, pair_end;
    // piece p: entries [piece_off[p], piece_off[p + 1]) of pair piece_pair[p]; group pair q's
    // pieces are [pp_off[q], pp_off[q + 1])
    std::vector<uint32_t> piece_off, piece_pair, pp_off;   // [n_pieces + 1], [n_pieces], [n_gp + 1]
    int64_t n_pieces = 0, n_entries = 0;
    int64_t pc_lo = 0, pc_hi = 0;                          // this rank's pieces
    std::vector<uint32_t> span_off, span_e;                // K2's spans: piece and entry bounds
    int64_t node_bytes = 0;                                // what K2 streams per decision
    std::vector<uint32_t> list_off;                        // [G + 1] new-node / removal lists
};

// The layout of `live[q]` entries per group pair (each followed by spare_entries of spare
// room) and the tail runs behind them, for the rank that owns the group pairs [q_lo, q_hi).
// ESC_E_LIMIT when the entries or a group's list offset do not fit 32 bits.
inline int32_t plan_node_layout(NodeLayout& L, const std::vector<int64_t>& live, double f,
                                const std::vector<TailRun>& tail, uint32_t q_lo, uint32_t q_hi, bool pk_ok,
                                const uint32_t* gpair, int32_t G) {
    const uint32_t n_gp = (uint32_t)live.size();
    L = NodeLayout();
    L.pair_lo.resize(n_gp); L.pair_next.resize(n_gp); L.pair_end.resize(n_gp);
    uint64_t E = 0;
    for (uint32_t q = 0; q < n_gp; ++q) {
        L.pair_lo[q] = (uint32_t)E;
        L.pair_next[q] = (uint32_t)(E + (uint64_t)live[q]);
        E += (uint64_t)(live[q] + spare_entries(live[q], f));
        if (E >= 0xFFFFFFFFull) return ESC_E_LIMIT;
        L.pair_end[q] = (uint32_t)E;
    }
    const uint64_t tail_lo = E;
    for (const TailRun& r : tail) {
        E += r.len;
        if (E >= 0xFFFFFFFFull) return ESC_E_LIMIT;
    }
    L.n_entries = (int64_t)E;
    // Pieces: runs of entries of one pair that cross no multiple of PIECE_ALIGN entries, so
    // K2's spans (whole pieces, <= NODE_SPAN entries) come out full (cut only at
    // pairs they averaged 72 % of NODE_SPAN at config 4); a pair cut in two is summed from both
    // rows by k_node_groups, as any multi-piece pair.
    auto cut = [&L](uint64_t a, uint64_t z, uint32_t pair) {
        while (a < z) {
            L.piece_off.push_back((uint32_t)a);
            L.piece_pair.push_back(pair);
            a = std::min<uint64_t>(z, (a / PIECE_ALIGN + 1) * PIECE_ALIGN);
        }
    };
    L.pp_off.resize((size_t)n_gp + 1);
    for (uint32_t q = 0; q < n_gp; ++q) {
        L.pp_off[q] = (uint32_t)L.piece_pair.size();
        cut(L.pair_lo[q], L.pair_end[q], q);
    }
    L.pp_off[n_gp] = (uint32_t)L.piece_pair.size();
    uint64_t a = tail_lo;
    for (const TailRun& r : tail) {
        cut(a, a + r.len, r.pair);
        a += r.len;
    }
    L.n_pieces = (int64_t)L.piece_pair.size();
    L.piece_off.push_back((uint32_t)E);
    // This rank's share: the pieces of the group pairs it owns.  The algorithmic bytes K2
    // streams over them per decision: per piece its pair and offset, per entry 16 B packed
    // (flags, cpu, memory in one record) or 20 B (the three arrays).
    L.pc_lo = L.pp_off[q_lo];
    L.pc_hi = L.pp_off[q_hi];
    const int64_t entries = (int64_t)L.piece_off[L.pc_hi] - L.piece_off[L.pc_lo];
    L.node_bytes = 8 * (L.pc_hi - L.pc_lo) + (pk_ok ? 16 : 20) * entries;
    // K2 spans: consecutive whole pieces, <= NODE_SPAN entries (or one larger piece) and
    // <= 63 pieces per wave
    L.span_off.assign(1, (uint32_t)L.pc_lo);
    int64_t acc = 0, np = 0;
    for (int64_t p = L.pc_lo; p < L.pc_hi; ++p) {
        const int64_t len = (int64_t)L.piece_off[p + 1] - L.piece_off[p];
        if (acc > 0 && (acc + len > NODE_SPAN || np == 63)) { L.span_off.push_back((uint32_t)p); acc = 0; np = 0; }
        acc += len;
        ++np;
    }
    if (L.pc_hi > L.pc_lo) L.span_off.push_back((uint32_t)L.pc_hi);
    L.span_e.resize(L.span_off.size());
    for (size_t w = 0; w < L.span_off.size(); ++w) L.span_e[w] = L.piece_off[L.span_off[w]];
    // a group's new-node and removal lists hold at most its pair's entry capacity
    L.list_off.assign((size_t)G + 1, 0);
    for (int32_t g = 0; g < G; ++g) {
        const uint32_t q = gpair[g];
        const uint64_t end = (uint64_t)L.list_off[g] + (L.pair_end[q] - L.pair_lo[q]);
        if (end >= 0xFFFFFFFFull) return ESC_E_LIMIT;
        L.list_off[g + 1] = (uint32_t)end;
    }
    return ESC_OK;
}

// Group facts fixed by a layout: this rank's pieces of the group's pair q (empty when another
// rank owns it) and allNodes[0] (controller.go:207-211) = the pair's first live entry's node
// (`first`, the lowest node index; NONE: the pair has no live entry) with its allocatable.
inline GroupNode group_node(const NodeLayout& L, uint32_t q, uint32_t first, int64_t cpu, int64_t mem) {
    GroupNode x;
    x.plo = std::max<int64_t>(L.pp_off[q], L.pc_lo);
    x.phi = std::max<int64_t>(std::min<int64_t>(L.pp_off[q + 1], L.pc_hi), x.plo);
    const bool any = first != NONE;
    x.first = any ? (int64_t)first : INT64_MAX;
    x.first_cpu = any ? cpu : 0;
    x.first_mem = any ? mem : 0;
    return x;
}

// ---- the placement's runs of PodRefs (esc_load_placement, esc_nodes_compact)
// Room for pods bound later (esc_set_spare's fraction f; none at f = 0): a slot of the node
// table gets its own count with the spare fraction on top, and at least the mean pods per live
// node with the spare fraction on top (run_cap_new) — what a lightly loaded node, or a free
// slot with no node yet, gets; the scheduler fills those.
inline uint64_t run_cap_new(int64_t bound, int64_t live, double f) {
    return f > 0 ? (uint64_t)std::ceil((double)bound / (double)std::max<int64_t>(live, 1) * (1.0 + f)) + 4 : 0;
}
inline uint64_t run_capacity(uint64_t len, bool in_table, uint64_t cap_new, double f) {
    const uint64_t own = len + (f > 0 ? (uint64_t)std::ceil((double)len * f) + 2 : 0);
    return in_table ? std::max(own, cap_new) : cap_new;
}
// The runs' offsets off[n_slots + 1] from their lengths: slots [0, n_table) hold nodes, the
// rest are free.  ESC_E_LIMIT when the PodRefs do not fit 32-bit offsets.
inline int32_t plan_runs(std::vector<uint32_t>& off, const uint32_t* len, int64_t n_slots, int64_t n_table, int64_t bound,
                         int64_t live, double f) {
    const uint64_t cap_new = run_cap_new(bound, live, f);
    off.assign((size_t)n_slots + 1, 0);
    uint64_t at = 0;
    for (int64_t j = 0; j < n_slots; ++j) {
        at += run_capacity(j < n_table ? len[j] : 0, j < n_table, cap_new, f);
        if (at >= 0xFFFFFFFFull) return ESC_E_LIMIT;
        off[j + 1] = (uint32_t)at;
    }
    return ESC_OK;
}

// ---- esc_nodes_compact: the live nodes renumbered densely, in ascending old
// index, into a table with fresh capacity, and the placement's runs re-cut for the new table.
constexpr int64_t NODE_INDEX_LIMIT = (int64_t)1 << 28;    // the age index's node field (MEMB_NODE_MASK)
struct RunMove { uint32_t src, dst, len; };                // PodRef offsets in the old and new buffer
struct CompactPlan {
    std::vector<uint32_t> new_of;                          // [old n_nodes] new index (NONE: absent)
    std::vector<uint32_t> src_of;                          // [n_cap] old index (NONE: a free slot)
    int64_t n_live = 0, n_cap = 0, xl_words = 0, xl_cap = 0;
    // with a placement: the new runs, the non-empty live runs' moves, the pods of dead runs
    std::vector<uint32_t> run_off, run_len;                // [n_cap + 1], [n_cap]
    std::vector<RunMove> moves;
    std::vector<int32_t> unbind;
    int64_t bound = 0;                                     // pods bound to live nodes
};
// nflags / label0: the mirrors of the old table's n_nodes slots.  run_off / run_len / run_pod:
// the placement's mirror (null without one).  ESC_E_INVAL for a negative minimum, ESC_E_LIMIT
// when the new table reaches NODE_INDEX_LIMIT slots or the labels or PodRefs 32-bit offsets.
inline int32_t plan_node_compact(CompactPlan& P, const uint32_t* nflags, const uint32_t* label0, int64_t n_nodes, double f,
                                 int64_t min_free_slots, int64_t min_free_xl_words, const uint32_t* run_off,
                                 const uint32_t* run_len, const int32_t* run_pod) {
    P = CompactPlan();
    if (min_free_slots < 0 || min_free_xl_words < 0 || n_nodes < 0) return ESC_E_INVAL;
    P.new_of.assign((size_t)n_nodes, NONE);
    for (int64_t j = 0; j < n_nodes; ++j) {
        if (nflags[j] & ESC_NF_ABSENT) continue;
        P.new_of[j] = (uint32_t)P.n_live++;
        if (label0[j] != NONE) P.xl_words += nf_xlbl(nflags[j]);
    }
    const int64_t L = P.n_live;
    if (min_free_slots >= NODE_INDEX_LIMIT || min_free_xl_words >= (int64_t)0xFFFFFFFF) return ESC_E_LIMIT;
    P.n_cap = std::max(table_slots(L, f), L + min_free_slots);
    P.xl_cap = std::max(label_words(P.xl_words, f), P.xl_words + min_free_xl_words);
    if (P.n_cap >= NODE_INDEX_LIMIT || P.xl_cap >= (int64_t)0xFFFFFFFF) return ESC_E_LIMIT;
    P.src_of.assign((size_t)P.n_cap, NONE);
    for (int64_t j = 0; j < n_nodes; ++j)
        if (P.new_of[j] != NONE) P.src_of[P.new_of[j]] = (uint32_t)j;
    if (!run_off) return ESC_OK;
    P.run_len.assign((size_t)std::max<int64_t>(P.n_cap, 1), 0);
    for (int64_t j = 0; j < n_nodes; ++j) {
        if (P.new_of[j] != NONE) {
            P.run_len[P.new_of[j]] = run_len[j];
            P.bound += run_len[j];
        } else {
            for (uint32_t k = 0; k < run_len[j]; ++k) P.unbind.push_back(run_pod[run_off[j] + k]);
        }
    }
    if (const int32_t rc = plan_runs(P.run_off, P.run_len.data(), P.n_cap, L, P.bound, L, f)) return rc;
    for (int64_t j = 0; j < n_nodes; ++j)
        if (P.new_of[j] != NONE && run_len[j]) P.moves.push_back(RunMove{run_off[j], P.run_off[P.new_of[j]], run_len[j]});
    return ESC_OK;
}

}  // namespace esc
