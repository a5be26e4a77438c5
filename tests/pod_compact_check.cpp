// pod_compact_check — stand-alone check of the plan of esc_pods_compact (plan_pod_compact,
// esc_pod_layout.h) and of the class rule the device shares with the host (pod_class_id /
// pod_inert, esc_kblock.h).
//
// Every class table is planned twice: by plan_pod_compact, and naively here — the tile counts from
// the rule of include/escalator_hip.h written out again, the ranges summed one by one, the free
// tiles compared with write_free_tile's.  Hand-written tables pin the edges (a class without live
// pods keeps one tile at spare > 0 and none at spare 0, re-homed pods that overflow a class, a
// created class, the 32-bit limit); a few thousand random tables follow.  Exit status 0: every
// check held (tests/test_pod_compact_host.py builds it with the host compiler and the address and
// undefined-behaviour sanitizers).
#include <cstdio>
#include <random>
#include <string>

#include "esc_pod_layout.h"

using namespace esc;

namespace {

int g_failed = 0, g_checked = 0;
std::string g_case;

#define CHECK(x)                                                                         \
    do {                                                                                 \
        ++g_checked;                                                                     \
        if (!(x)) {                                                                      \
            if (++g_failed <= 40) std::fprintf(stderr, "FAILED %s: %s (line %d)\n", g_case.c_str(), #x, __LINE__); \
        }                                                                                \
    } while (0)

struct World {
    std::vector<int> ids;                          // class ids in table order
    std::vector<int64_t> tiles, k_free;
    std::vector<int64_t> arr = std::vector<int64_t>(POD_CLASS_IDS, 0);
    double f = 0;
    int64_t c_tiles = 0;
};

std::vector<PodClass> table_of(const World& W, std::vector<int>& cls_of) {
    std::vector<PodClass> cls;
    cls_of.assign(POD_CLASS_IDS, -1);
    for (size_t i = 0; i < W.ids.size(); ++i) {
        cls_of[W.ids[i]] = (int)i;
        cls.push_back(pod_class_of_id(W.ids[i]));
    }
    int64_t kb = 0, w = 0;
    cut_pod_classes(cls, W.tiles, kb, w);
    return cls;
}

int64_t naive_spare(int64_t x, double f) {
    if (!(f > 0)) return 0;
    const int64_t s = (int64_t)((double)x * f);
    return s < 1 ? 1 : s;
}

int32_t run(const World& W, PodCompactPlan& P, std::vector<PodClass>& old, std::vector<int>& cls_of) {
    old = table_of(W, cls_of);
    PodCompactIn in;
    in.cls = &old;
    in.cls_of = &cls_of;
    in.k_free = W.k_free.data();
    in.arr = W.arr.data();
    in.f = W.f;
    in.c_tiles = W.c_tiles;
    return plan_pod_compact(P, in);
}

void check_world(const World& W) {
    PodCompactPlan P;
    std::vector<PodClass> old;
    std::vector<int> cls_of;
    const int32_t rc = run(W, P, old, cls_of);
    CHECK(rc == ESC_OK);
    if (rc) return;
    // the classes: old indices kept, the created ones behind them in ascending class id
    std::vector<int> ids = W.ids;
    int created = 0;
    int64_t rehomed = 0;
    for (int id = 0; id < POD_CLASS_IDS; ++id) {
        rehomed += W.arr[id];
        if (W.arr[id] > 0 && cls_of[id] < 0) { ids.push_back(id); ++created; }
    }
    CHECK(P.created == created && P.rehomed == rehomed);
    CHECK(P.cls.size() == ids.size() && P.live.size() == ids.size() && P.tab.size() == ids.size() && P.k_free.size() == ids.size());
    if (P.cls.size() != ids.size()) return;
    int64_t t = 0, kb = 0, w = 0, at = 0, before = 0, bytes_before = 0;
    for (size_t i = 0; i < ids.size(); ++i) {
        const PodClass ref = pod_class_of_id(ids[i]);
        const PodClass& k = P.cls[i];
        CHECK(P.cls_of[ids[i]] == (int)i);
        CHECK(k.xreg == ref.xreg && k.xinit == ref.xinit && k.ovh == ref.ovh && k.nxp == ref.nxp && k.kind == ref.kind &&
              k.wt == ref.wt && k.packed == ref.packed);
        const int64_t was = i < W.ids.size() ? W.tiles[i] : 0;
        const int64_t live = (i < W.ids.size() ? was * 256 - W.k_free[i] : 0) + W.arr[ids[i]];
        const int64_t tiles = (live + naive_spare(live, W.f) + 255) / 256;
        CHECK(P.live[i] == live);
        CHECK(k.t0 == t && k.t1 == t + tiles && k.kb0 == kb && k.w0 == w);      // ascending ranges
        CHECK(P.k_free[i].first == live && P.k_free[i].second == tiles * 256);
        CHECK(P.tab[i].start == at && P.tab[i].live == live);
        const bool inert = ids[i] >= POD_INERT_ID0;
        if (tiles > 0) {
            std::vector<uint32_t> free_tile((size_t)ref.wt * 128);
            write_free_tile(ref, free_tile.data());
            CHECK(P.tab[i].tmpl >= 0 && (P.tab[i].tmpl & 3) == 0 && P.tab[i].tmpl + (int64_t)free_tile.size() <= (int64_t)P.tmpl.size());
            if (P.tab[i].tmpl >= 0 && P.tab[i].tmpl + (int64_t)free_tile.size() <= (int64_t)P.tmpl.size())
                CHECK(std::equal(free_tile.begin(), free_tile.end(), P.tmpl.begin() + P.tab[i].tmpl));
        } else {
            CHECK(P.tab[i].tmpl == -1);
            CHECK(!(W.f > 0));                                                   // only at spare 0
        }
        if (W.f > 0) CHECK(tiles >= 1);
        t += tiles;
        kb += tiles * (int64_t)ref.wt * 128;
        w += inert ? 0 : tiles * (int64_t)ref.wt;
        at += live;
        before += was;
        bytes_before += inert ? 0 : was * (int64_t)ref.wt * 512;
    }
    for (int id = 0; id < POD_CLASS_IDS; ++id)
        if (std::find(ids.begin(), ids.end(), id) == ids.end()) CHECK(P.cls_of[id] == -1);
    CHECK(P.k_tiles == t && P.kb_words == kb && P.k_weight == w);
    CHECK(P.tiles_before == before && P.k1_bytes_before == bytes_before && P.k1_bytes_after == w * 512);
}

World hand(std::vector<int> ids, std::vector<int64_t> tiles, std::vector<int64_t> k_free, double f) {
    World W;
    W.ids = std::move(ids);
    W.tiles = std::move(tiles);
    W.k_free = std::move(k_free);
    W.f = f;
    W.c_tiles = 3;
    return W;
}

constexpr uint32_t DS = ESC_PF_DAEMONSET, ST = ESC_PF_STATIC, SEL = ESC_PF_HAS_SEL, AFF = ESC_PF_AFF_BLOCK;
uint32_t flags(uint32_t bits, uint32_t np, uint32_t xr = 0, uint32_t xi = 0, uint32_t ov = 0) {
    return bits | (ov ? ESC_PF_HAS_OVH : 0u) | xr << ESC_PF_XREG_SHIFT | xi << ESC_PF_XINIT_SHIFT | np << ESC_PF_XPAIR_SHIFT;
}

struct Pod {
    const char* name;
    uint32_t f, cpu0;
    int64_t mem0;
    uint32_t pair0;
    std::vector<uint32_t> xp;
    std::vector<int64_t> xc_cpu, xc_mem;
    bool inert;
    int id;
};

}  // namespace

int main() {
    // ---- hand-written tables
    g_case = "shrink";
    {   // 4 tiles, 513 live at spare 0 -> 3; 2 tiles, 255 live -> 1; 2 tiles, 257 live -> 2
        World W = hand({256, 257, 128}, {4, 2, 2}, {4 * 256 - 513, 2 * 256 - 255, 2 * 256 - 257}, 0.0);
        check_world(W);
        PodCompactPlan P; std::vector<PodClass> old; std::vector<int> of;
        CHECK(run(W, P, old, of) == ESC_OK);
        CHECK(P.cls[0].t1 - P.cls[0].t0 == 3 && P.cls[1].t1 - P.cls[1].t0 == 1 && P.cls[2].t1 - P.cls[2].t0 == 2);
        CHECK(P.k_tiles == 6 && P.tiles_before == 8);
    }
    g_case = "no live pods";
    {   // spare > 0: one tile stays; spare 0: none, the class keeps its index
        World W = hand({256, 0, 384}, {3, 2, 2}, {3 * 256, 2 * 256, 2 * 256}, 0.25);
        check_world(W);
        PodCompactPlan P; std::vector<PodClass> old; std::vector<int> of;
        CHECK(run(W, P, old, of) == ESC_OK && P.k_tiles == 3);
        W.f = 0.0;
        check_world(W);
        CHECK(run(W, P, old, of) == ESC_OK && P.k_tiles == 0 && P.cls.size() == 3 && P.cls_of[0] == 1 && P.kb_words == 0);
        CHECK(P.tmpl.empty());
    }
    g_case = "grow by re-homed pods";
    {   // one tile, 250 live, 10 re-homed at spare 0.25: 260 + 65 -> 2 tiles
        World W = hand({256, 1}, {1, 1}, {6, 256}, 0.25);
        W.arr[256] = 10;
        check_world(W);
        PodCompactPlan P; std::vector<PodClass> old; std::vector<int> of;
        CHECK(run(W, P, old, of) == ESC_OK && P.cls[0].t1 == 2 && P.live[0] == 260 && P.rehomed == 10 && P.created == 0);
    }
    g_case = "created classes";
    {   // ids the table lacks: behind the old classes, ascending; an inert one among them
        World W = hand({258, 128}, {1, 1}, {0, 1}, 0.0);
        W.arr[385] = 3; W.arr[33] = 300; W.arr[128] = 2; W.arr[2] = 1;
        check_world(W);
        PodCompactPlan P; std::vector<PodClass> old; std::vector<int> of;
        CHECK(run(W, P, old, of) == ESC_OK && P.created == 3 && P.cls.size() == 5);
        CHECK(P.cls_of[258] == 0 && P.cls_of[128] == 1 && P.cls_of[2] == 2 && P.cls_of[33] == 3 && P.cls_of[385] == 4);
        CHECK(P.cls[3].t1 - P.cls[3].t0 == 2 && P.cls[1].t1 - P.cls[1].t0 == 2);          // 300 -> 2 tiles; 255 + 2 -> 2
        CHECK(kb_inert(P.cls[4]) && P.k_weight == P.cls[4].w0);                          // the inert class weighs nothing
    }
    g_case = "a fresh cut";
    {   // the load's table order (inert classes last) is what the plan keeps
        std::vector<int> ids;
        for (int ord = 0; ord < POD_CLASS_IDS; ++ord) {
            const int id = pod_class_order(ord);
            if (pod_class_holdable(id) && (id < POD_INERT_ID0 || id == 384)) ids.push_back(id);
        }
        CHECK(ids.size() == 73 && ids.back() == 384 && ids.front() == 256);
        World W = hand(ids, std::vector<int64_t>(73, 2), std::vector<int64_t>(73, 300), 0.02);
        check_world(W);
    }
    g_case = "limit";
    {
        World W = hand({256}, {(int64_t)1 << 24}, {0}, 0.0);                             // 2^32 pod slots
        PodCompactPlan P; std::vector<PodClass> old; std::vector<int> of;
        CHECK(run(W, P, old, of) == ESC_E_LIMIT);
        W.tiles[0] = ((int64_t)1 << 24) - 1;                                             // 2^32 - 256 + 192 slots: one below
        W.c_tiles = 3;
        CHECK(run(W, P, old, of) == ESC_OK);
        W.c_tiles = 4;                                                                   // 2^32 exactly
        CHECK(run(W, P, old, of) == ESC_E_LIMIT);
        W.c_tiles = 3;
        W.arr[256] = 64;                                                                 // the re-homed pods push a tile over
        W.f = 0.0;
        CHECK(run(W, P, old, of) == ESC_E_LIMIT);
    }
    // ---- random tables
    std::mt19937_64 rng(20260101);
    std::vector<int> holdable;
    for (int id = 0; id < POD_CLASS_IDS; ++id)
        if (pod_class_holdable(id)) holdable.push_back(id);
    CHECK(holdable.size() == 76);
    for (int it = 0; it < 3000; ++it) {
        g_case = "random " + std::to_string(it);
        World W;
        W.f = (it % 3 == 0) ? 0.0 : (double)(rng() % 400) / 1000.0;
        W.c_tiles = (int64_t)(rng() % 50);
        std::vector<int> pool = holdable;
        std::shuffle(pool.begin(), pool.end(), rng);
        const size_t n = 1 + rng() % 20;
        for (size_t i = 0; i < n; ++i) {
            const int64_t tiles = (int64_t)(rng() % 6);
            W.ids.push_back(pool[i]);
            W.tiles.push_back(tiles);
            W.k_free.push_back(tiles ? (int64_t)(rng() % (uint64_t)(tiles * 256 + 1)) : 0);
        }
        for (size_t i = 0; i < 6; ++i)
            if (rng() % 2) W.arr[pool[rng() % 30]] += (int64_t)(rng() % 700);
        check_world(W);
    }
    // ---- the class rule, over the edges of tests/inert_class_check.cpp: the body the device shares
    g_case = "class rule";
    const uint32_t N_GP = 6, NONE_ = NONE;
    const std::vector<Pod> pods = {
        {"daemonset, no pair", flags(DS, 0), 100, 1 << 20, NONE_, {}, {}, {}, true, 384},
        {"daemonset with a group pair", flags(DS | SEL, 0), 100, 1 << 20, 2, {}, {}, {}, true, 384},
        {"daemonset, group pair among extras", flags(DS | SEL, 2), 100, 1 << 20, 1, {3, 9}, {}, {}, true, 386},
        {"static", flags(ST, 0), 100, 1 << 20, NONE_, {}, {}, {}, true, 384},
        {"selector, last group pair", flags(SEL, 0), 100, 1 << 20, N_GP - 1, {}, {}, {}, false, 256},
        {"selector, first non-group pair", flags(SEL, 0), 100, 1 << 20, N_GP, {}, {}, {}, true, 384},
        {"affinity only", flags(AFF, 0), 100, 1 << 20, NONE_, {}, {}, {}, true, 384},
        {"no filter bit, no pairs", flags(0, 0), 100, 1 << 20, NONE_, {}, {}, {}, false, 256},
        {"one group pair, three non-group extras", flags(SEL, 3), 100, 1 << 20, 3, {7, 8, 9}, {}, {}, false, 259},
        {"four non-group pairs", flags(SEL, 3), 100, 1 << 20, 6, {7, 8, 9}, {}, {}, true, 387},
        {"group pair0, a non-group extra", flags(SEL | AFF, 1), 100, 1 << 20, 0, {N_GP}, {}, {}, false, 257},
        {"static with a group pair", flags(ST | SEL, 0), 100, 1 << 20, 0, {}, {}, {}, false, 256},
        {"daemonset, 12-B request", flags(DS, 0), 100, (int64_t)1 << 34, NONE_, {}, {}, {}, true, 128},
        {"daemonset, plain", flags(DS, 1), 100, (int64_t)1 << 44, NONE_, {9}, {}, {}, true, 1},
        {"static, record folds to 12 B", flags(ST, 0, 1), 1 << 13, 5, NONE_, {}, {1 << 13}, {5}, true, 128},
        {"static, record folds to 8 B", flags(ST, 0, 1), 100, 5, NONE_, {}, {100}, {5}, true, 384},
        {"daemonset, four records", flags(DS, 0, 4), 1, 1, NONE_, {}, {1, 1, 1, 1}, {1, 1, 1, 1}, true, -1},
        {"four extra pairs", flags(SEL, 4), 1, 1, 0, {1, 2, 3, 4}, {}, {}, false, -1},
        {"plain, 2 regular + 1 init + overhead", flags(SEL, 0, 2, 1, 1), 1, 1, 0, {}, {1, 1, 1, 1}, {1, 1, 1, 1}, false, -1},
        {"plain, 1 regular + 1 init + overhead", flags(SEL, 1, 1, 1, 1), 1 << 20, 1, 0, {1}, {1, INT64_MIN, 1}, {1, INT64_MIN, 1},
         false, ((1 * 4 + 1) * 2 + 1) * 4 + 1},
        {"an init key absent folds", flags(SEL, 0, 0, 1), 100, 5, 0, {}, {INT64_MIN}, {7}, false, 256},
    };
    for (const Pod& p : pods) {
        const bool inert = pod_inert(p.f, p.pair0, p.xp.empty() ? nullptr : p.xp.data(), N_GP);
        const int id = pod_class_id(p.f, p.cpu0, p.mem0, p.pair0, p.xc_cpu.empty() ? nullptr : p.xc_cpu.data(),
                                    p.xc_mem.empty() ? nullptr : p.xc_mem.data(), p.xp.empty() ? nullptr : p.xp.data(), N_GP);
        if (inert != p.inert || id != p.id) std::fprintf(stderr, "%s: inert %d, class id %d\n", p.name, (int)inert, id);
        CHECK(inert == p.inert);
        CHECK(id == p.id);
    }
    CHECK(pod_class_id(flags(DS, 0), 100, 1 << 20, NONE_, nullptr, nullptr, nullptr, KP8_PAIR_NONE) == 128);
    // ---- the small helpers of the call
    g_case = "helpers";
    CHECK(pod_buckets(32, 10016) == 315 && pod_buckets(32, 20480) == 642 && pod_buckets(0, 999) == 1);
    CHECK(pod_bucket(0, 32, 96) == 0 && pod_bucket(95, 32, 96) == 2 && pod_bucket(96, 32, 96) == 4 && pod_bucket(NONE, 32, 96) == 4);
    CHECK(pod_bucket(31, 32, 96) == 0 && pod_bucket(32, 32, 96) == 1 && pod_bucket(7, 0, 96) == 0 && pod_bucket(NONE, 0, 96) == 0);
    CHECK(!c_slot_parked(ESC_PF_DAEMONSET, 0) && c_slot_parked(CS_FLAGS & ~ESC_PF_DAEMONSET, 0));
    CHECK(c_slot_parked(CS_FLAGS, 3 | 3 << 16) && !c_slot_parked(CS_FLAGS, 4) && !c_slot_parked(CS_FLAGS, 4 << 16));
    CHECK(c_slot_freed(CS_FLAGS & ~ESC_PF_DAEMONSET) == CS_FLAGS);
    std::printf("%d checks held, %d failed\n", g_checked - g_failed, g_failed);
    return g_failed ? 1 : 0;
}
