// pod_grow_check — stand-alone check of the plan of esc_pods_grow (plan_pod_grow,
// esc_pod_layout.h).
//
// Every generated class table is planned twice: by plan_pod_grow, and naively here — the
// capacities from the rule of include/escalator_hip.h written out again, the tile ranges summed
// one by one, a free tile's words written from the block layout's description
// instead of through kb_write_free, the spare C tiles slot by slot.  Every field must agree.
// Tables past the limits are given to the plan alone and must be refused.  Exit status 0: every
// check held (tests/test_pod_grow_host.py builds it with the host compiler and the address and
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

// A resident pod side: class ids in table order, tiles and free positions per class, the C counts.
struct World {
    std::vector<int> ids;
    std::vector<int64_t> tiles, k_free;
    std::vector<int64_t> arr = std::vector<int64_t>(POD_CLASS_IDS, 0);
    double f = 0;
    int64_t c_tiles = 0, live_c = 0, arr_c = 0, free_cs = 0;
    uint32_t xc_end = 0, xp_end = 0;
};

// the signature of a class id, written out: np | init << 3 ... as pod_class_id composes it
void sig_of(int id, uint32_t& xreg, uint32_t& xinit, uint32_t& ovh, uint32_t& nxp, uint32_t& packed) {
    packed = (uint32_t)(id / 128);
    const int sig = id % 128;
    nxp = (uint32_t)(sig & 3);
    ovh = (uint32_t)((sig >> 2) & 1);
    xinit = (uint32_t)((sig >> 3) & 3);
    xreg = (uint32_t)(sig >> 5);
}
uint32_t naive_wt(int id) {
    uint32_t xr, xi, ov, np, pk;
    sig_of(id, xr, xi, ov, np, pk);
    if (pk == 2) return 4 + np;
    if (pk == 1) return 2 * (3 + np);
    return 2 * (5 + 4 * (xr + xi + ov) + np);
}
// a free tile of class id, from the layout's description
std::vector<uint32_t> naive_free_tile(int id) {
    uint32_t xr, xi, ov, np, pk;
    sig_of(id, xr, xi, ov, np, pk);
    std::vector<uint32_t> w((size_t)naive_wt(id) * 128, 0);
    if (pk == 2) {
        const uint64_t v = (uint64_t(1) << 62) | (uint64_t(1) << 63) | (uint64_t(0x3FFF) << 48);
        for (int s = 0; s < 256; ++s) { w[2 * s] = (uint32_t)v; w[2 * s + 1] = (uint32_t)(v >> 32); }
        for (size_t k = 512; k < w.size(); ++k) w[k] = 0xFFFFFFFFu;         // u16 rows: 0xFFFF each
    } else if (pk == 1) {
        for (int s = 0; s < 256; ++s) w[s] = (ESC_PF_DAEMONSET << 28) | 0x0FFFFFFFu;
        for (size_t k = 768; k < w.size(); ++k) w[k] = 0xFFFFFFFFu;
    } else {
        const size_t R = xr + xi + ov;
        for (int s = 0; s < 256; ++s) { w[s] = ESC_PF_DAEMONSET; w[1024 + s] = 0xFFFFFFFFu; }
        for (size_t k = 1280 + 1024 * R; k < w.size(); ++k) w[k] = 0xFFFFFFFFu;
    }
    return w;
}

std::vector<PodClass> table_of(const World& W, std::vector<int>& cls_of) {
    std::vector<PodClass> cls;
    cls_of.assign(POD_CLASS_IDS, -1);
    int64_t kt = 0, kb = 0, kw = 0;
    for (size_t i = 0; i < W.ids.size(); ++i) {
        PodClass k = pod_class_of_id(W.ids[i]);
        k.t0 = kt; k.t1 = kt + W.tiles[i]; k.kb0 = kb; k.w0 = kw;
        kt += W.tiles[i]; kb += W.tiles[i] * (int64_t)k.wt * 128; kw += W.tiles[i] * (int64_t)k.wt;
        cls_of[W.ids[i]] = (int)i;
        cls.push_back(k);
    }
    return cls;
}

void check_world(const World& W, const std::string& name) {
    g_case = name;
    std::vector<int> cls_of;
    const std::vector<PodClass> cls = table_of(W, cls_of);
    PodGrowIn in;
    in.cls = &cls; in.cls_of = &cls_of; in.k_free = W.k_free.data(); in.arr = W.arr.data(); in.f = W.f;
    in.c_tiles = W.c_tiles; in.live_c = W.live_c; in.arr_c = W.arr_c; in.free_cs = W.free_cs;
    in.xc_end = W.xc_end; in.xp_end = W.xp_end;
    PodGrowPlan P;
    const int32_t rc = plan_pod_grow(P, in);
    // ---- naive: the classes (created ones behind the old, ascending id), their tiles
    std::vector<int> ids = W.ids;
    for (int id = 0; id < POD_CLASS_IDS; ++id)
        if (W.arr[id] > 0 && cls_of[id] < 0) ids.push_back(id);
    const size_t n = ids.size(), n_old = W.ids.size();
    std::vector<int64_t> tiles(n);
    bool k_changed = false;
    for (size_t i = 0; i < n; ++i) {
        const int64_t was = i < n_old ? W.tiles[i] : 0;
        const int64_t live = i < n_old ? was * 256 - W.k_free[i] : 0;
        const int64_t x = live + W.arr[ids[i]];
        const int64_t s = W.f > 0 ? std::max<int64_t>(1, (int64_t)std::floor((double)x * W.f)) : 0;
        tiles[i] = std::max(was, (x + s + 255) / 256);
        k_changed |= tiles[i] != was;
    }
    int64_t kt = 0;
    for (int64_t t : tiles) kt += t;
    // ---- naive: the C tail
    const int64_t sp = W.f > 0 ? std::max<int64_t>(16, (int64_t)std::ceil((double)(W.live_c + W.arr_c) * W.f)) : 0;
    const int64_t want_cs = W.arr_c + sp;
    const int64_t c_new = want_cs > W.free_cs ? (want_cs - W.free_cs + 15) / 16 : 0;
    const int64_t xc_dev = (int64_t)W.xc_end + c_new * 16 * 7 + 1, xp_dev = (int64_t)W.xp_end + c_new * 16 * 6 + 1;
    const bool limit = xc_dev >= 0xFFFFFFFFll || xp_dev >= 0xFFFFFFFFll ||
                       kt * 256 + (W.c_tiles + c_new) * 64 >= 0xFFFFFFFFll;
    CHECK(rc == (limit ? ESC_E_LIMIT : ESC_OK));
    if (rc || limit) return;
    CHECK(P.k_changed == k_changed);
    CHECK(P.c_changed == (c_new > 0));
    CHECK(P.cls.size() == n && P.moves.size() == n && P.k_new.size() == n);
    if (P.cls.size() != n || P.moves.size() != n || P.k_new.size() != n) return;
    int64_t t0 = 0, kb0 = 0, w0 = 0;
    for (size_t i = 0; i < n; ++i) {
        const PodClass& k = P.cls[i];
        const KbRegrowCls& m = P.moves[i];
        uint32_t xr, xi, ov, np, pk;
        sig_of(ids[i], xr, xi, ov, np, pk);
        const uint32_t wt = naive_wt(ids[i]);
        // kept indices and signatures; ascending ranges cut in class-index order
        CHECK(P.cls_of[ids[i]] == (int)i);
        CHECK(k.xreg == xr && k.xinit == xi && k.ovh == ov && k.nxp == np && k.packed == pk && k.wt == wt);
        CHECK(k.kind == (pk ? 16 + (pk - 1) * 4 + np : (xr + xi + ov) * 4 + np));
        if (i < n_old) CHECK(k.kind == cls[i].kind && k.wt == cls[i].wt && k.packed == cls[i].packed);
        CHECK(k.t0 == t0 && k.t1 == t0 + tiles[i] && k.kb0 == kb0 && k.w0 == w0);
        CHECK(k.t1 - k.t0 >= (i < n_old ? W.tiles[i] : 0));
        CHECK(m.t0 == k.t0 && m.t1 == k.t1 && m.new_kb0 == k.kb0 && m.wt == wt);
        CHECK(m.old_tiles == (i < n_old ? W.tiles[i] : 0));
        if (i < n_old) CHECK(m.old_kb0 == cls[i].kb0);
        // the new free positions: the gained tiles' slots, nothing else
        CHECK(P.k_new[i].first == m.old_tiles * 256 && P.k_new[i].second == tiles[i] * 256);
        // capacity holds the live pods, the arrivals and the spare rule
        const int64_t live = i < n_old ? W.tiles[i] * 256 - W.k_free[i] : 0;
        CHECK(tiles[i] * 256 - live >= W.arr[ids[i]] + (W.f > 0 ? 1 : 0));
        if (tiles[i] > m.old_tiles) {
            const std::vector<uint32_t> want = naive_free_tile(ids[i]);
            CHECK(m.tmpl >= 0 && (m.tmpl % 4) == 0 && m.tmpl + (int64_t)want.size() <= (int64_t)P.tmpl.size());
            if (m.tmpl >= 0 && m.tmpl + (int64_t)want.size() <= (int64_t)P.tmpl.size())
                CHECK(std::equal(want.begin(), want.end(), P.tmpl.begin() + m.tmpl));
            // and equal to what the load's step writes through the layout's own functions
            std::vector<uint32_t> own(want.size(), 0xA5A5A5A5u);
            write_free_tile(k, own.data());
            CHECK(own == want);
        } else {
            CHECK(m.tmpl == -1);
        }
        t0 += tiles[i]; kb0 += tiles[i] * (int64_t)wt * 128; w0 += tiles[i] * (int64_t)wt;
    }
    CHECK(P.k_tiles == t0 && P.kb_words == kb0 && P.k_weight == w0);
    for (int id = 0; id < POD_CLASS_IDS; ++id)
        if (std::find(ids.begin(), ids.end(), id) == ids.end()) CHECK(P.cls_of[id] == -1);
    // ---- the C tail
    CHECK(P.c_new == c_new && P.c_tiles == W.c_tiles + c_new);
    CHECK((int64_t)P.c_flags.size() == c_new * 64 && P.c_cpu0.size() == P.c_flags.size() &&
          P.c_mem0.size() == P.c_flags.size() && P.c_pair0.size() == P.c_flags.size());
    CHECK((int64_t)P.xc_cpu.size() == (c_new ? c_new * 112 + 1 : 0) && P.xc_mem.size() == P.xc_cpu.size());
    CHECK((int64_t)P.xp.size() == (c_new ? c_new * 96 + 1 : 0));
    CHECK((int64_t)P.xc_base.size() == c_new && (int64_t)P.xp_base.size() == c_new);
    CHECK((int64_t)P.c_free.size() == c_new * 16);
    if ((int64_t)P.c_flags.size() != c_new * 64 || (int64_t)P.xc_cpu.size() != (c_new ? c_new * 112 + 1 : 0) ||
        (int64_t)P.c_free.size() != c_new * 16 || (int64_t)P.xc_base.size() != c_new)
        return;
    const uint32_t cs_flags = ESC_PF_DAEMONSET | ESC_PF_HAS_OVH | 4u << ESC_PF_XREG_SHIFT | 2u << ESC_PF_XINIT_SHIFT |
                              6u << ESC_PF_XPAIR_SHIFT;
    for (int64_t t = 0; t < c_new; ++t) {
        for (int l = 0; l < 64; ++l) {
            const size_t d = (size_t)(t * 64 + l);
            CHECK(P.c_flags[d] == (l < 16 ? cs_flags : ESC_PF_DAEMONSET));
            CHECK(P.c_cpu0[d] == 0 && P.c_mem0[d] == 0 && P.c_pair0[d] == 0xFFFFFFFFu);
            if (l < 16) {
                CHECK(P.c_free[(size_t)(t * 16 + l)] == (W.c_tiles + t) * 64 + l);
                for (int k = 0; k < 7; ++k) {
                    const int64_t v = (k == 4 || k == 5) ? INT64_MIN : 0;
                    CHECK(P.xc_cpu[(size_t)((t * 16 + l) * 7 + k)] == v && P.xc_mem[(size_t)((t * 16 + l) * 7 + k)] == v);
                }
            }
        }
        CHECK(P.xc_base[(size_t)t] == W.xc_end + (uint32_t)((t + 1) * 112));
        CHECK(P.xp_base[(size_t)t] == W.xp_end + (uint32_t)((t + 1) * 96));
    }
    if (c_new) CHECK(P.xc_cpu.back() == 0 && P.xc_mem.back() == 0);          // the one padding element
    for (uint32_t q : P.xp) CHECK(q == 0xFFFFFFFFu);
    // the slots appended hold the arrivals and the spare rule
    CHECK(W.free_cs + c_new * 16 >= want_cs);
}

}  // namespace

int main() {
    // ---- hand-written
    {   // the issue's full class: 300 packed-small pods at spare 0.25 (375 -> 2 tiles), 400 arrive
        World W;
        W.ids = {256, 257, 258, 259, 128, 0};
        W.tiles = {2, 1, 1, 1, 1, 1};
        W.k_free = {212, 255, 255, 255, 255, 255};
        W.arr[256] = 400;
        W.f = 0.25;
        W.c_tiles = 1; W.free_cs = 16; W.xc_end = 112; W.xp_end = 96;
        check_world(W, "full class");
        W.arr[256] = 0;
        check_world(W, "nothing to do");
        W.arr_c = 40; W.live_c = 3;
        check_world(W, "C arrivals");
    }
    {   // loaded without spare: a class created by the grow, odd weights, the heaviest plain class
        World W;
        W.ids = {257, 259};
        W.tiles = {1, 2};
        W.k_free = {1, 0};
        W.arr[257] = 1; W.arr[259] = 513;
        W.arr[128 + 3] = 257;            // 12-B packed, 3 pairs
        W.arr[3 * 32 + 3] = 257;         // R = 3 regular, 3 pairs: wt 40
        W.arr[128 + 2] = 1;              // 12-B packed, 2 pairs
        W.arr_c = 17;
        check_world(W, "no spare");
    }
    {   // limits: record offsets and pod slots past 32 bits
        World W;
        W.ids = {256};
        W.tiles = {1};
        W.k_free = {0};
        W.f = 0.5; W.arr_c = 1; W.c_tiles = 1; W.xc_end = 0xFFFFFFFFu - 100;
        check_world(W, "xc limit");
        W.xc_end = 0; W.xp_end = 0xFFFFFFFFu - 96;
        check_world(W, "xp limit");
        W.xp_end = 0; W.arr[256] = 0xFFFFFFFFll;
        check_world(W, "slot limit");
        W.arr[256] = 0; W.c_tiles = 0xFFFFFFFFll / 64;
        check_world(W, "slot limit C");
    }
    // ---- random class tables
    std::mt19937_64 rng(0x9E3779B97F4A7C15ull);
    auto rnd = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
    const double fracs[] = {0.0, 0.0, 0.01, 0.25, 0.5, 1.0, 4.0};
    for (int it = 0; it < 4000; ++it) {
        World W;
        W.f = fracs[rnd(0, 6)];
        std::vector<int> all;
        for (int id = 0; id < POD_CLASS_IDS; ++id) {
            uint32_t xr, xi, ov, np, pk;
            sig_of(id, xr, xi, ov, np, pk);
            if (pk > 2 || (pk ? id % 128 >= 4 : xr + xi + ov > 3)) continue;
            all.push_back(id);
        }
        // table order as the load's: small, packed, plain; a subset when no spare was asked
        std::vector<int> order;
        for (int pk = 2; pk >= 0; --pk)
            for (int id : all)
                if (id / 128 == pk && (W.f > 0 || rnd(0, 3) == 0)) order.push_back(id);
        for (int id : order) {
            const int64_t t = rnd(1, it % 7 == 0 ? 40 : 3);
            W.ids.push_back(id);
            W.tiles.push_back(t);
            W.k_free.push_back(rnd(0, 2) == 0 ? 0 : rnd(0, t * 256));
        }
        for (int k = (int)rnd(0, 6); k > 0; --k) {
            const int id = all[(size_t)rnd(0, (int64_t)all.size() - 1)];
            if (W.f > 0 && std::find(order.begin(), order.end(), id) == order.end()) continue;
            const int64_t sizes[] = {1, 255, 256, 257, 1000, 5000};
            W.arr[id] = sizes[rnd(0, 5)];
        }
        W.c_tiles = rnd(0, 50);
        W.live_c = rnd(0, W.c_tiles * 64);
        W.arr_c = rnd(0, 3) == 0 ? rnd(0, 300) : 0;
        W.free_cs = rnd(0, 2) == 0 ? 0 : rnd(0, 64);
        W.xc_end = (uint32_t)rnd(0, 100000);
        W.xp_end = (uint32_t)rnd(0, 100000);
        check_world(W, "random " + std::to_string(it));
    }
    std::printf("%d checks held, %d failed\n", g_checked - g_failed, g_failed);
    return g_failed ? 1 : 0;
}
