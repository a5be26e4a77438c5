// esc_pod_layout.h — the pod side's capacity rules and the plan of esc_pods_grow (DESIGN.md §3,
// §8n).
//
// esc_load_pods gives every K class `live + spare` positions in whole 256-pod tiles and a few
// spare C tiles; esc_pods_upsert fills them in place; esc_pods_grow re-cuts the classes' tile
// ranges on the device when they are full.  What the three must agree on lives here: the class of
// a pod, the room of a C slot, the spare rule, the cut of tile ranges from capacities, a free
// tile's bytes and a spare C tile's arrays.  Host only, plain C++17, no HIP header:
// tests/pod_grow_check.cpp builds it with the host compiler.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "esc_common.h"
#include "esc_kblock.h"

namespace esc {

// A kb_write_pod / kb_write_free put into a host copy of K blocks.
inline void put_kb(uint32_t* kb, int width, int64_t at, uint64_t v) {
    if (width == 8) reinterpret_cast<int64_t*>(kb)[at] = (int64_t)v;
    else if (width == 4) kb[at] = (uint32_t)v;
    else reinterpret_cast<uint16_t*>(kb)[at] = (uint16_t)v;
}

// Spare C slots (esc_load_pods with esc_set_spare, esc_pods_grow): room per slot, slots per
// 64-pod tile.
constexpr int CS_SLOTS = 16, CS_XREG = 4, CS_XINIT = 2, CS_REC = CS_XREG + CS_XINIT + 1, CS_XP = 6;
static_assert(CS_SLOTS * CS_REC <= 128 && CS_SLOTS * CS_XP <= 128, "a spare C tile stays on K1's C path");
constexpr uint32_t CS_FLAGS = ESC_PF_DAEMONSET | ESC_PF_HAS_OVH | (uint32_t)CS_XREG << ESC_PF_XREG_SHIFT |
                              (uint32_t)CS_XINIT << ESC_PF_XINIT_SHIFT | (uint32_t)CS_XP << ESC_PF_XPAIR_SHIFT;

// (pod_inert and pod_class_id, the one definition of a pod's class, are in esc_kblock.h: the
// device classifies re-homed pods by the same body, esc_pods_compact.)

// Does C slot room `cf` (counts of a slot's flags) hold a pod with flags f?  Its records
// and pairs take the slot's first positions of each kind, the rest stay neutral.
inline bool c_room(uint32_t cf, uint32_t f) {
    return pf_xreg(f) <= pf_xreg(cf) && pf_xinit(f) <= pf_xinit(cf) && (!(f & ESC_PF_HAS_OVH) || (cf & ESC_PF_HAS_OVH)) &&
           pf_xpair(f) <= pf_xpair(cf);
}

// The spare positions behind x live pods of a K class (esc_set_spare's fraction f).
inline int64_t pod_spare(int64_t x, double f) { return f > 0 ? std::max<int64_t>(1, (int64_t)((double)x * f)) : 0; }
// The spare C slots beside n pods of the C section.
inline int64_t c_spare(int64_t n, double f) { return f > 0 ? std::max<int64_t>(CS_SLOTS, (int64_t)std::ceil((double)n * f)) : 0; }

// The class of id `id` (pod_class_id), its tile range and offsets unset.
inline PodClass pod_class_of_id(int id) {
    const int sig = id % POD_SIG_IDS;
    PodClass k;
    std::memset(&k, 0, sizeof k);
    k.nxp = (uint32_t)(sig % 4);
    k.ovh = (uint32_t)((sig / 4) % 2);
    k.xinit = (uint32_t)((sig / 8) % 4);
    k.xreg = (uint32_t)(sig / 32);
    const bool inert = id >= POD_INERT_ID0;               // the packed small tile, a kind of its own
    k.packed = inert ? 2u : (uint32_t)(id / POD_SIG_IDS);
    const uint32_t R = k.xreg + k.xinit + k.ovh;
    k.kind = inert ? K_KIND_INERT + k.nxp : k_kind(R, k.nxp, k.packed);
    k.wt = k_tile_weight(R, k.nxp, k.packed);
    return k;
}

// Class ids in the load's table order: packed small, packed, plain, then the inert classes, so
// that K1 streams the packed classes first and the inert ones move no other class's range.
inline int pod_class_order(int ord) {
    const int blk = ord / POD_SIG_IDS;
    return (blk < 3 ? 2 - blk : 3) * POD_SIG_IDS + ord % POD_SIG_IDS;
}
// Can the K layout hold class id at all?  Plain: every signature of at most 3 records; the
// packed and inert classes: the 4 without records.
inline bool pod_class_holdable(int id) {
    const int sig = id % POD_SIG_IDS;
    return id < POD_SIG_IDS ? (sig / 32) + ((sig / 8) % 4) + ((sig / 4) % 2) <= 3 : sig < 4;
}

// Cuts the classes' tile ranges from their tile counts, in class-index order: t0 / t1, kb0 and
// w0 ascend.  Returns the K section's tiles; kb_words / weight: its block words and work weight.
// An inert class has real tiles and block words and no weight (kb_k1_wt): K1's walks split the
// weight, so none of them reaches its tiles.
inline int64_t cut_pod_classes(std::vector<PodClass>& cls, const std::vector<int64_t>& tiles, int64_t& kb_words,
                               int64_t& weight) {
    int64_t kt = 0;
    kb_words = weight = 0;
    for (size_t i = 0; i < cls.size(); ++i) {
        PodClass& k = cls[i];
        k.t0 = kt;
        k.t1 = kt + tiles[i];
        k.kb0 = kb_words;
        k.w0 = weight;
        kt += tiles[i];
        weight += tiles[i] * (int64_t)kb_k1_wt(k);
        kb_words += tiles[i] * (int64_t)k.wt * KB_UNIT;
    }
    return kt;
}

// A free tile of class k at dst (k.wt * KB_UNIT words), as esc_load_pods writes every tile before
// it places the pods: zeroed, every slot a freed one, no pairs.
inline void write_free_tile(const PodClass& k, uint32_t* dst) {
    const int64_t words = (int64_t)k.wt * KB_UNIT;
    std::memset(dst, 0, (size_t)words * 4);
    for (int64_t sl = 0; sl < TILE; ++sl)
        kb_write_free(k, 0, sl, [&](int width, int64_t at, uint64_t v) { put_kb(dst, width, at, v); });
    if (!k.packed) std::fill(dst + KB_PAIR0, dst + KB_PAIR0 + TILE, NONE);
    const int64_t x0 = kb_xp_row0(k, 0);              // no pairs (u32 or u16 NONE)
    std::fill(dst + x0, dst + x0 + kb_xp_words(k), NONE);
}

// What esc_pods_grow knows before it plans: the resident classes, their free positions, the
// batch's arrivals and the C section's counts.
struct PodGrowIn {
    const std::vector<PodClass>* cls = nullptr;
    const std::vector<int>* cls_of = nullptr;     // [POD_CLASS_IDS] class id -> class index, -1: none
    const int64_t* k_free = nullptr;              // [classes] free positions
    const int64_t* arr = nullptr;                 // [POD_CLASS_IDS] batch pods that need a new position, by class id
    double f = 0;                                 // esc_set_spare
    int64_t c_tiles = 0;                          // C tiles resident
    int64_t live_c = 0;                           // pods in C slots
    int64_t arr_c = 0;                            // batch pods that need a free C slot
    int64_t free_cs = 0;                          // free C slots with at least a spare slot's room
    uint32_t xc_end = 0, xp_end = 0;              // xc_base[c_tiles], xp_base[c_tiles]
};

struct PodGrowPlan {
    bool k_changed = false, c_changed = false;
    // K section: the new class table (old indices kept, created classes behind them)
    std::vector<PodClass> cls;
    std::vector<int> cls_of;
    std::vector<KbRegrowCls> moves;               // [classes] k_kb_regrow's table
    std::vector<uint32_t> tmpl;                   // the free tiles of the classes that gain tiles
    std::vector<std::pair<int64_t, int64_t>> k_new;   // [classes] new free positions [first, second)
    int64_t k_tiles = 0, k_weight = 0, kb_words = 0;
    // C section: the appended spare tiles (arrays cover the new tiles' slots / records alone)
    int64_t c_tiles = 0, c_new = 0;
    std::vector<uint32_t> c_flags, c_cpu0, c_pair0;   // [c_new * CTILE]
    std::vector<int64_t> c_mem0;
    std::vector<int64_t> xc_cpu, xc_mem;          // [c_new * CS_SLOTS * CS_REC + 1]: from the old padding element on
    std::vector<uint32_t> xp;                     // [c_new * CS_SLOTS * CS_XP + 1]
    std::vector<uint32_t> xc_base, xp_base;       // [c_new] the bases of tiles old c_tiles + 1 .. c_tiles (their ends)
    std::vector<int64_t> c_free;                  // the new free C slots (C-array index), ascending
};

// The plan (the rule of include/escalator_hip.h, esc_pods_grow).  ESC_E_LIMIT when the C record
// offsets or the pod slots leave 32 bits.
inline int32_t plan_pod_grow(PodGrowPlan& P, const PodGrowIn& in) {
    P = PodGrowPlan();
    const std::vector<PodClass>& old = *in.cls;
    P.cls = old;
    P.cls_of = *in.cls_of;
    const size_t n_old = old.size();
    std::vector<int64_t> arr_cls(n_old, 0);
    for (int id = 0; id < POD_CLASS_IDS; ++id) {
        if (in.arr[id] <= 0) continue;
        int ci = P.cls_of[id];
        if (ci < 0) {                                  // (a context loaded without spare room)
            ci = P.cls_of[id] = (int)P.cls.size();
            P.cls.push_back(pod_class_of_id(id));
            arr_cls.push_back(0);
        }
        arr_cls[ci] += in.arr[id];
    }
    const size_t n = P.cls.size();
    std::vector<int64_t> tiles(n), was(n);
    for (size_t i = 0; i < n; ++i) {
        was[i] = i < n_old ? old[i].t1 - old[i].t0 : 0;
        const int64_t live = i < n_old ? was[i] * TILE - in.k_free[i] : 0;
        const int64_t want = live + arr_cls[i] + pod_spare(live + arr_cls[i], in.f);
        tiles[i] = std::max(was[i], (want + TILE - 1) / TILE);
        P.k_changed |= tiles[i] != was[i];
    }
    P.k_tiles = cut_pod_classes(P.cls, tiles, P.kb_words, P.k_weight);
    P.moves.resize(n);
    P.k_new.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const PodClass& k = P.cls[i];
        KbRegrowCls m{};
        m.t0 = k.t0; m.t1 = k.t1;
        m.old_kb0 = i < n_old ? old[i].kb0 : 0;
        m.old_tiles = was[i];
        m.new_kb0 = k.kb0;
        m.wt = k.wt;
        m.tmpl = -1;
        if (tiles[i] > was[i]) {
            m.tmpl = (int64_t)P.tmpl.size();
            P.tmpl.resize(P.tmpl.size() + (size_t)k.wt * KB_UNIT);
            write_free_tile(k, P.tmpl.data() + m.tmpl);
        }
        P.moves[i] = m;
        P.k_new[i] = {was[i] * TILE, tiles[i] * TILE};
    }
    // C section
    const int64_t want_cs = in.arr_c + (in.f > 0 ? c_spare(in.live_c + in.arr_c, in.f) : 0);
    P.c_new = (std::max<int64_t>(0, want_cs - in.free_cs) + CS_SLOTS - 1) / CS_SLOTS;
    P.c_tiles = in.c_tiles + P.c_new;
    P.c_changed = P.c_new > 0;
    const int64_t xc_dev = (int64_t)in.xc_end + P.c_new * CS_SLOTS * CS_REC + 1;
    const int64_t xp_dev = (int64_t)in.xp_end + P.c_new * CS_SLOTS * CS_XP + 1;
    if (xc_dev >= (int64_t)0xFFFFFFFF || xp_dev >= (int64_t)0xFFFFFFFF) return ESC_E_LIMIT;
    if (P.k_tiles * TILE + P.c_tiles * CTILE >= (int64_t)0xFFFFFFFF) return ESC_E_LIMIT;   // a PodRef's source slot
    if (P.c_new) {
        const size_t slots = (size_t)P.c_new * CTILE;
        P.c_flags.assign(slots, ESC_PF_DAEMONSET);
        P.c_cpu0.assign(slots, 0);
        P.c_pair0.assign(slots, NONE);
        P.c_mem0.assign(slots, 0);
        P.xc_cpu.assign((size_t)(P.c_new * CS_SLOTS * CS_REC + 1), 0);
        P.xc_mem = P.xc_cpu;
        P.xp.assign((size_t)(P.c_new * CS_SLOTS * CS_XP + 1), NONE);
        uint64_t oc = 0;
        for (int64_t t = 0; t < P.c_new; ++t) {
            for (int l = 0; l < CS_SLOTS; ++l) {
                P.c_flags[(size_t)t * CTILE + l] = CS_FLAGS;
                for (int k = 0; k < CS_REC; ++k) {       // neutral records: 0 added, init keys absent
                    const bool init = k >= CS_XREG && k < CS_XREG + CS_XINIT;
                    P.xc_cpu[oc + k] = P.xc_mem[oc + k] = init ? INT64_MIN : 0;
                }
                oc += CS_REC;
                P.c_free.push_back((in.c_tiles + t) * CTILE + l);
            }
            P.xc_base.push_back((uint32_t)(in.xc_end + (uint64_t)(t + 1) * CS_SLOTS * CS_REC));
            P.xp_base.push_back((uint32_t)(in.xp_end + (uint64_t)(t + 1) * CS_SLOTS * CS_XP));
        }
    }
    return ESC_OK;
}

// ---- esc_pods_compact
// The bucket of a pod inside its class (esc_load_pods' step 4): pair0 / pod_sort, NONE and the
// pairs no group selects last; one bucket when pod_sort == 0.
inline int64_t pod_buckets(uint32_t pod_sort, uint32_t n_gp) { return pod_sort ? (int64_t)(n_gp / pod_sort) + 2 : 1; }
inline int64_t pod_bucket(uint32_t pair0, uint32_t pod_sort, uint32_t n_gp) {
    return pod_sort ? (pair0 < n_gp ? (int64_t)(pair0 / pod_sort) : pod_buckets(pod_sort, n_gp) - 1) : 0;
}
// Is the C slot with flags cf live and its pod K-holdable by the host's counts (h_cused: the
// pod's own records | pairs << 16)?  A slot whose flags are the daemonset bit alone is padding.
inline bool c_slot_parked(uint32_t cf, uint32_t used) { return cf != ESC_PF_DAEMONSET && (used & 0xFFFF) <= 3 && (used >> 16) <= 3; }
// The flags a re-homed pod leaves behind in its C slot, as esc_pods_delete leaves them: free
// (daemonset-flagged), the counts kept as the slot's room.
inline uint32_t c_slot_freed(uint32_t cf) { return cf | ESC_PF_DAEMONSET; }

// What esc_pods_compact knows before it plans: the resident classes, their free positions and
// the re-homed pods by class id (the device's classification of the K-holdable C slots).
struct PodCompactIn {
    const std::vector<PodClass>* cls = nullptr;
    const std::vector<int>* cls_of = nullptr;     // [POD_CLASS_IDS] class id -> class index, -1: none
    const int64_t* k_free = nullptr;              // [classes] free positions
    const int64_t* arr = nullptr;                 // [POD_CLASS_IDS] re-homed pods, by class id
    double f = 0;                                 // esc_set_spare
    int64_t c_tiles = 0;                          // C tiles resident (they stay)
};

struct PodCompactPlan {
    // the new class table: old indices kept, created classes behind them in ascending class id
    std::vector<PodClass> cls;
    std::vector<int> cls_of;
    std::vector<int64_t> live;                    // [classes] live pods after the re-homing
    std::vector<PcCls> tab;                       // [classes] k_pc_move's table
    std::vector<uint32_t> tmpl;                   // the free tile of every class that has tiles
    std::vector<std::pair<int64_t, int64_t>> k_free;   // [classes] the free positions [first, second)
    int created = 0;
    int64_t rehomed = 0;
    int64_t k_tiles = 0, k_weight = 0, kb_words = 0;
    int64_t tiles_before = 0, k1_bytes_before = 0, k1_bytes_after = 0;
};

// The plan (the rule of include/escalator_hip.h, esc_pods_compact): tiles_i = ceil((live_i +
// s(live_i)) / 256) with the load's s; a class may shrink, grow or (f = 0) drop to no tile.
// ESC_E_LIMIT when the pod slots leave 32 bits.
inline int32_t plan_pod_compact(PodCompactPlan& P, const PodCompactIn& in) {
    P = PodCompactPlan();
    const std::vector<PodClass>& old = *in.cls;
    P.cls = old;
    P.cls_of = *in.cls_of;
    const size_t n_old = old.size();
    std::vector<int64_t> arr_cls(n_old, 0);
    for (int id = 0; id < POD_CLASS_IDS; ++id) {
        if (in.arr[id] <= 0) continue;
        int ci = P.cls_of[id];
        if (ci < 0) {
            ci = P.cls_of[id] = (int)P.cls.size();
            P.cls.push_back(pod_class_of_id(id));
            arr_cls.push_back(0);
            ++P.created;
        }
        arr_cls[ci] += in.arr[id];
        P.rehomed += in.arr[id];
    }
    const size_t n = P.cls.size();
    std::vector<int64_t> tiles(n);
    P.live.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const int64_t was = i < n_old ? old[i].t1 - old[i].t0 : 0;
        P.live[i] = (i < n_old ? was * TILE - in.k_free[i] : 0) + arr_cls[i];
        tiles[i] = (P.live[i] + pod_spare(P.live[i], in.f) + TILE - 1) / TILE;
        P.tiles_before += was;
        if (i < n_old) P.k1_bytes_before += was * (int64_t)kb_k1_wt(old[i]) * 512;
    }
    P.k_tiles = cut_pod_classes(P.cls, tiles, P.kb_words, P.k_weight);
    P.k1_bytes_after = P.k_weight * 512;
    if (P.k_tiles * TILE + in.c_tiles * CTILE >= (int64_t)0xFFFFFFFF) return ESC_E_LIMIT;   // a PodRef's source slot
    P.tab.resize(n);
    P.k_free.resize(n);
    int64_t at = 0;
    for (size_t i = 0; i < n; ++i) {
        const PodClass& k = P.cls[i];
        PcCls m{};
        m.start = at;
        m.live = P.live[i];
        m.tmpl = -1;
        if (tiles[i] > 0) {
            m.tmpl = (int64_t)P.tmpl.size();
            P.tmpl.resize(P.tmpl.size() + (size_t)k.wt * KB_UNIT);
            write_free_tile(k, P.tmpl.data() + m.tmpl);
        }
        at += P.live[i];
        P.tab[i] = m;
        P.k_free[i] = {P.live[i], tiles[i] * TILE};
    }
    return ESC_OK;
}

}  // namespace esc
