// Stand-alone host check of the inert classes (escalator_amd/csrc/esc_pod_layout.h),
// built by tests/test_inert_host.py with the host compiler under AddressSanitizer and UBSan:
//  - pod_inert / pod_class_id over hand-built pods at every edge of the definition;
//  - the class cut: inert classes last, real tiles and block words, no K1 weight, and every other
//    class's t0 / kb0 / w0 equal to the cut of the same pods without the inert ones;
//  - plan_pod_grow grows and creates an inert class by the load's rule and leaves the weight alone.
#include <cstdio>
#include <string>
#include <vector>

#include "esc_pod_layout.h"

using namespace esc;

namespace {

int g_checked = 0, g_failed = 0;
#define CHECK(x)                                                                          \
    do {                                                                                  \
        ++g_checked;                                                                      \
        if (!(x) && ++g_failed <= 40) std::fprintf(stderr, "FAILED: %s (line %d)\n", #x, __LINE__); \
    } while (0)

constexpr uint32_t N_GP = 5;
constexpr uint32_t DS = ESC_PF_DAEMONSET, ST = ESC_PF_STATIC, SEL = ESC_PF_HAS_SEL, AFF = ESC_PF_AFF_BLOCK;

uint32_t flags(uint32_t bits, uint32_t nxp, uint32_t xreg = 0) {
    return bits | nxp << ESC_PF_XPAIR_SHIFT | xreg << ESC_PF_XREG_SHIFT;
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

// the load's class table for per-id pod counts at spare fraction f, as esc_load_pods cuts it
std::vector<PodClass> load_table(const std::vector<int64_t>& cnt, double f, std::vector<int>& cls_of, int64_t& kb_words,
                                 int64_t& weight, int64_t& k_tiles) {
    std::vector<PodClass> cls;
    std::vector<int64_t> tiles;
    cls_of.assign(POD_CLASS_IDS, -1);
    for (int ord = 0; ord < POD_CLASS_IDS; ++ord) {
        const int id = pod_class_order(ord);
        if (!cnt[id] && !(f > 0 && id < POD_INERT_ID0 && pod_class_holdable(id))) continue;
        cls_of[id] = (int)cls.size();
        cls.push_back(pod_class_of_id(id));
        tiles.push_back((cnt[id] + pod_spare(cnt[id], f) + TILE - 1) / TILE);
    }
    k_tiles = cut_pod_classes(cls, tiles, kb_words, weight);
    return cls;
}

}  // namespace

int main() {
    const uint32_t NONE_ = NONE;
    // ---- the definition, one pod just inside and one just outside every edge
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
        // inert but outside the packed small block: where it is today
        {"daemonset, 12-B request", flags(DS, 0), 100, (int64_t)1 << 34, NONE_, {}, {}, {}, true, 128},
        {"daemonset, plain", flags(DS, 1), 100, (int64_t)1 << 44, NONE_, {9}, {}, {}, true, 1},
        {"static, record folds to 12 B", flags(ST, 0, 1), 1 << 13, 5, NONE_, {}, {1 << 13}, {5}, true, 128},
        {"static, record folds to 8 B", flags(ST, 0, 1), 100, 5, NONE_, {}, {100}, {5}, true, 384},
        {"daemonset, four records", flags(DS, 0, 4), 1, 1, NONE_, {}, {1, 1, 1, 1}, {1, 1, 1, 1}, true, -1},
    };
    for (const Pod& p : pods) {
        const bool inert = pod_inert(p.f, p.pair0, p.xp.empty() ? nullptr : p.xp.data(), N_GP);
        const int id = pod_class_id(p.f, p.cpu0, p.mem0, p.pair0, p.xc_cpu.empty() ? nullptr : p.xc_cpu.data(),
                                    p.xc_mem.empty() ? nullptr : p.xc_mem.data(), p.xp.empty() ? nullptr : p.xp.data(), N_GP);
        if (inert != p.inert || id != p.id) std::fprintf(stderr, "%s: inert %d, class id %d\n", p.name, (int)inert, id);
        CHECK(inert == p.inert);
        CHECK(id == p.id);
    }
    // a context too wide for the packed small block has no inert classes either
    CHECK(pod_class_id(flags(DS, 0), 100, 1 << 20, NONE_, nullptr, nullptr, nullptr, KP8_PAIR_NONE) == 128);
    // ---- an inert class: the packed small tile, a kind of its own, no K1 weight
    for (int np = 0; np < 4; ++np) {
        const PodClass a = pod_class_of_id(POD_INERT_ID0 + np), b = pod_class_of_id(2 * POD_SIG_IDS + np);
        CHECK(a.packed == 2 && a.nxp == (uint32_t)np && a.xreg + a.xinit + a.ovh == 0 && a.wt == b.wt && a.wt == 4u + np);
        CHECK(a.kind == K_KIND_INERT + np && a.kind != b.kind && a.kind >= 24);
        CHECK(kb_inert(a) && !kb_inert(b) && kb_k1_wt(a) == 0 && kb_k1_wt(b) == b.wt);
        CHECK(pod_class_holdable(POD_INERT_ID0 + np));
        std::vector<uint32_t> ta((size_t)a.wt * KB_UNIT, 1u), tb(ta.size(), 2u);
        write_free_tile(a, ta.data());
        write_free_tile(b, tb.data());
        CHECK(ta == tb);                                   // the same free tile, word for word
    }
    CHECK(!pod_class_holdable(POD_INERT_ID0 + 4));
    {   // every class id in the table order exactly once, the inert ones last
        std::vector<int> seen(POD_CLASS_IDS, 0);
        for (int ord = 0; ord < POD_CLASS_IDS; ++ord) {
            const int id = pod_class_order(ord);
            CHECK(id >= 0 && id < POD_CLASS_IDS);
            if (id >= 0 && id < POD_CLASS_IDS) ++seen[id];
            CHECK((id >= POD_INERT_ID0) == (ord >= 3 * POD_SIG_IDS));
        }
        for (int v : seen) CHECK(v == 1);
    }
    // ---- the cut: with and without the inert pods, at the tile edges
    for (double f : {0.0, 0.25}) {
        for (int64_t n : {255, 256, 257}) {
            std::vector<int64_t> cnt(POD_CLASS_IDS, 0);
            cnt[256] = n; cnt[257] = 3; cnt[259] = 700; cnt[128] = 40; cnt[131] = n; cnt[0] = 5; cnt[99] = 300;
            std::vector<int64_t> with = cnt;
            for (int np = 0; np < 4; ++np) with[POD_INERT_ID0 + np] = n + np;
            std::vector<int> of_a, of_b;
            int64_t kb_a, w_a, t_a, kb_b, w_b, t_b;
            const std::vector<PodClass> A = load_table(cnt, f, of_a, kb_a, w_a, t_a);
            const std::vector<PodClass> B = load_table(with, f, of_b, kb_b, w_b, t_b);
            CHECK(B.size() == A.size() + 4 && w_a == w_b);
            for (size_t i = 0; i < A.size() && i < B.size(); ++i) {
                CHECK(A[i].t0 == B[i].t0 && A[i].t1 == B[i].t1 && A[i].kb0 == B[i].kb0 && A[i].w0 == B[i].w0);
                CHECK(A[i].kind == B[i].kind && !kb_inert(B[i]));
            }
            int64_t t = t_a, kb = kb_a;
            for (int np = 0; np < 4; ++np) {
                const size_t i = A.size() + np;
                if (i >= B.size()) break;
                const PodClass& k = B[i];
                const int64_t tiles = (n + np + pod_spare(n + np, f) + TILE - 1) / TILE;
                CHECK(of_b[POD_INERT_ID0 + np] == (int)i && kb_inert(k) && k.nxp == (uint32_t)np);
                CHECK(k.t0 == t && k.t1 == t + tiles && k.kb0 == kb && k.w0 == w_a);   // real storage, no weight
                t += tiles;
                kb += tiles * (int64_t)k.wt * KB_UNIT;
            }
            CHECK(t_b == t && kb_b == kb);
            // an inert class without pods is not made by the load, spare room or not
            for (int np = 0; np < 4; ++np) CHECK(of_a[POD_INERT_ID0 + np] == -1);
            // ---- the grow: a full inert class, and one the context lacks
            auto free_of = [](const std::vector<PodClass>& cls, const std::vector<int>& of, const std::vector<int64_t>& n_of) {
                std::vector<int64_t> fr(cls.size(), 0);
                for (int id = 0; id < POD_CLASS_IDS; ++id)
                    if (of[id] >= 0) fr[of[id]] = (cls[of[id]].t1 - cls[of[id]].t0) * TILE - n_of[id];
                return fr;
            };
            const std::vector<int64_t> k_free = free_of(B, of_b, with);
            std::vector<int64_t> arr(POD_CLASS_IDS, 0);
            arr[POD_INERT_ID0] = 400;
            PodGrowIn in;
            in.cls = &B; in.cls_of = &of_b; in.k_free = k_free.data(); in.arr = arr.data(); in.f = f;
            PodGrowPlan P;
            CHECK(plan_pod_grow(P, in) == ESC_OK);
            const size_t ci = (size_t)of_b[POD_INERT_ID0];
            const int64_t want = n + 400 + pod_spare(n + 400, f);
            CHECK(P.k_changed && P.cls.size() == B.size() && P.k_weight == w_b);
            CHECK(P.cls[ci].t1 - P.cls[ci].t0 == (want + TILE - 1) / TILE && kb_inert(P.cls[ci]));
            CHECK(P.k_new[ci].first == (B[ci].t1 - B[ci].t0) * TILE && P.k_new[ci].second == (P.cls[ci].t1 - P.cls[ci].t0) * TILE);
            for (size_t i = 0; i < B.size(); ++i) {
                if (i != ci) CHECK(P.cls[i].t1 - P.cls[i].t0 == B[i].t1 - B[i].t0);
                CHECK(P.cls[i].w0 == B[i].w0 && P.cls[i].kind == B[i].kind);
                if (i <= ci) CHECK(P.cls[i].t0 == B[i].t0 && P.cls[i].kb0 == B[i].kb0);
            }
            const std::vector<int64_t> free_a = free_of(A, of_a, cnt);
            std::vector<int64_t> arr2(POD_CLASS_IDS, 0);
            arr2[POD_INERT_ID0 + 2] = 257;
            PodGrowIn in2;
            in2.cls = &A; in2.cls_of = &of_a; in2.k_free = free_a.data(); in2.arr = arr2.data(); in2.f = f;
            PodGrowPlan Q;
            CHECK(plan_pod_grow(Q, in2) == ESC_OK);
            CHECK(Q.cls.size() == A.size() + 1 && Q.cls_of[POD_INERT_ID0 + 2] == (int)A.size() && Q.k_weight == w_a);
            if (Q.cls.size() == A.size() + 1) {
                const PodClass& k = Q.cls.back();
                CHECK(kb_inert(k) && k.nxp == 2 && k.packed == 2 && k.t0 == t_a && k.kb0 == kb_a && k.w0 == w_a);
                CHECK(k.t1 - k.t0 == (257 + pod_spare(257, f) + TILE - 1) / TILE);
                CHECK(Q.moves.back().tmpl >= 0 && Q.moves.back().wt == k.wt && Q.moves.back().old_tiles == 0);
            }
        }
    }
    {   // every pod inert: tiles and words, no weight at all
        std::vector<int64_t> cnt(POD_CLASS_IDS, 0);
        cnt[POD_INERT_ID0] = 600;
        std::vector<int> of;
        int64_t kb, w, t;
        const std::vector<PodClass> A = load_table(cnt, 0.0, of, kb, w, t);
        CHECK(A.size() == 1 && t == 3 && w == 0 && kb == 3 * 4 * KB_UNIT && A[0].w0 == 0);
    }
    std::printf("%d checks held, %d failed\n", g_checked - g_failed, g_failed);
    return g_failed ? 1 : 0;
}
