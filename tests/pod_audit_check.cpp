// CPU check of the re-derivation esc_audit_pods' KSLOT check runs on the device (kb_pod_class,
// escalator_amd/csrc/esc_kblock.h): a pod written into the class the rule chose for it
// (pod_class_id -> kb_write_pod) reads back (kb_head / kb_rec / kb_pair) and re-classifies to
// that class's id, for every class the K layout can hold, in contexts on both sides of the
// packed small format's pair limit.  Values are drawn from the edges of every range the rule
// tests — 2^14 - 1 m, 2^34 - 1 B, 2^20 - 1, 2^44 - 1, pair ids around the group-pair count,
// 0xFFFF, 2^14 - 1 and 2^28 - 1 — and from random ones.  Also: what the words of a free tile
// re-derive to, per class.  Stand-alone; built by tests/test_pod_audit_host.py with the host
// compiler under AddressSanitizer and UBSan.
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
#include <vector>

#include "esc_pod_layout.h"

using namespace esc;

static long held = 0, failed = 0;
#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (cond) ++held;                                       \
        else { if (++failed <= 20) { std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } \
    } while (0)

static const uint32_t CPU_EDGES[] = {0, 1, (1u << 14) - 2, (1u << 14) - 1, 1u << 14, (1u << 20) - 2, (1u << 20) - 1, 1u << 20, 0xFFFFFFFFu};
static const int64_t MEM_EDGES[] = {0, 1, (int64_t(1) << 34) - 2, (int64_t(1) << 34) - 1, int64_t(1) << 34, (int64_t(1) << 44) - 2,
                                    (int64_t(1) << 44) - 1, int64_t(1) << 44, -1, INT64_MAX};
static const int64_t REC_CPU_EDGES[] = {0, 1, (1 << 14) - 1, 1 << 14, (1 << 20) - 2, (1 << 20) - 1, 1 << 20, -1, INT64_MAX};
static const uint32_t OWN_FLAGS[] = {0, ESC_PF_DAEMONSET, ESC_PF_STATIC, ESC_PF_HAS_SEL, ESC_PF_AFF_BLOCK,
                                     ESC_PF_DAEMONSET | ESC_PF_STATIC, ESC_PF_STATIC | ESC_PF_AFF_BLOCK};

template <class T, size_t N>
static T pick(std::mt19937_64& g, const T (&v)[N]) { return v[g() % N]; }

static uint32_t pick_pair(std::mt19937_64& g, uint32_t n_gp) {
    const uint32_t edges[] = {0, n_gp - 1, n_gp, n_gp + 1, 0xFFFEu, 0xFFFFu, 0x10000u, (1u << 14) - 2, (1u << 14) - 1, 1u << 14,
                              (1u << 28) - 2, (1u << 28) - 1, 1u << 28, NONE - 1, NONE};
    return g() % 4 ? pick(g, edges) : (uint32_t)(g() % (2 * (uint64_t)n_gp + 2));
}

// One tile of class id, every slot free (as esc_load_pods writes it before it places the pods).
static PodClass one_tile(int id, std::vector<uint32_t>& tile) {
    PodClass k = pod_class_of_id(id);
    k.t0 = 0; k.t1 = 1; k.kb0 = 0;
    tile.assign((size_t)k.wt * KB_UNIT, 0);
    write_free_tile(k, tile.data());
    return k;
}

int main() {
    std::mt19937_64 g(0xE5CA1A7E0000A0D1ull);
    std::set<int> holdable, reached;
    for (int id = 0; id < POD_CLASS_IDS; ++id)
        if (pod_class_holdable(id)) holdable.insert(id);
    CHECK(holdable.size() == 76, "%zu holdable class ids", holdable.size());
    for (int id : holdable) {                                       // the class's fields give its id back
        const PodClass k = pod_class_of_id(id);
        CHECK(kb_class_id(k) == id, "kb_class_id %d of class id %d", kb_class_id(k), id);
    }
    {                                                               // fields no class has
        PodClass k = pod_class_of_id(5);
        k.nxp = 4;
        CHECK(kb_class_id(k) == -1, "nxp 4");
        k = pod_class_of_id(2 * POD_SIG_IDS);
        k.xreg = 1;
        CHECK(kb_class_id(k) == -1, "a packed class with records");
        k = pod_class_of_id(3);
        k.packed = 3;
        CHECK(kb_class_id(k) == -1, "packed 3");
    }

    std::vector<uint32_t> tile;
    const uint32_t n_gps[] = {1, 16382, 16383};
    long pods = 0;
    for (uint32_t n_gp : n_gps)
        for (uint32_t xr = 0; xr <= 3; ++xr)
            for (uint32_t xi = 0; xr + xi <= 3; ++xi)
                for (uint32_t ov = 0; xr + xi + ov <= 3 && ov <= 1; ++ov)
                    for (uint32_t np = 0; np <= 3; ++np)
                        for (int rep = 0; rep < 2500; ++rep) {
                            const uint32_t f = pick(g, OWN_FLAGS) | (ov ? ESC_PF_HAS_OVH : 0u) | xr << ESC_PF_XREG_SHIFT |
                                               xi << ESC_PF_XINIT_SHIFT | np << ESC_PF_XPAIR_SHIFT;
                            const uint32_t cpu0 = g() % 3 ? pick(g, CPU_EDGES) : (uint32_t)(g() % (1u << 21));
                            const int64_t mem0 = g() % 3 ? pick(g, MEM_EDGES) : (int64_t)(g() % (uint64_t(1) << 45));
                            const uint32_t pair0 = pick_pair(g, n_gp);
                            int64_t xc[3] = {0, 0, 0}, xm[3] = {0, 0, 0};
                            uint32_t xp[3] = {NONE, NONE, NONE};
                            const uint32_t R = xr + xi + ov;
                            const bool small = g() % 2;            // keep half of the pods inside the packed ranges
                            for (uint32_t k = 0; k < R; ++k) {
                                const bool init = k >= xr && k < xr + xi;
                                xc[k] = small ? (int64_t)(g() % 5000) : pick(g, REC_CPU_EDGES);
                                xm[k] = small ? (int64_t)(g() % (uint64_t(1) << 32)) : pick(g, MEM_EDGES);
                                if (init && g() % 4 == 0) xc[k] = INT64_MIN;
                                if (init && g() % 4 == 0) xm[k] = INT64_MIN;
                            }
                            for (uint32_t k = 0; k < np; ++k) xp[k] = pick_pair(g, n_gp);
                            const int id = pod_class_id(f, cpu0, mem0, pair0, R ? xc : nullptr, R ? xm : nullptr, np ? xp : nullptr, n_gp);
                            CHECK(id >= 0 && holdable.count(id), "class id %d of a K pod", id);
                            if (id < 0 || !holdable.count(id)) continue;
                            reached.insert(id);
                            const PodClass C = one_tile(id, tile);
                            const int64_t s = (int64_t)(g() % TILE);
                            kb_write_pod(C, 0, s, f, cpu0, mem0, pair0, xc, xm, xp,
                                         [&](int width, int64_t at, uint64_t v) { put_kb(tile.data(), width, at, v); });
                            CPodRec r;
                            const int back = kb_pod_class(C, tile.data(), 0, s, n_gp, r);
                            CHECK(back == id, "n_gp %u flags %#x cpu0 %u mem0 %lld pair0 %u: wrote class %d, read back %d", n_gp, f, cpu0,
                                  (long long)mem0, pair0, id, back);
                            ++pods;
                        }
    for (int id : holdable) CHECK(reached.count(id), "class id %d never reached", id);

    // A free tile's slots.  Where the context has packed small classes they re-derive to the
    // inert class of the tile's pair count, else to the packed class of that count: to their own
    // class only in an inert class and in a packed class of a context without packed small ones
    // (there a free slot is the words of a live daemonset pod of zero request).
    const uint32_t n_gps_free[] = {1, 16382, 16383, 20480};
    for (uint32_t n_gp : n_gps_free)
        for (int id : holdable) {
            const bool p8 = n_gp < KP8_PAIR_NONE;
            if (id >= 2 * POD_SIG_IDS && !p8) continue;             // no packed small or inert class in such a context
            const PodClass C = one_tile(id, tile);
            for (int64_t s : {0, 1, 127, 255}) {
                CPodRec r;
                const int back = kb_pod_class(C, tile.data(), 0, s, n_gp, r);
                const bool own = kb_inert(C) || (C.packed == 1 && !p8);
                if (own) CHECK(back == id, "free slot of class %d (n_gp %u) read back %d", id, n_gp, back);
                else CHECK(back != id, "free slot of class %d (n_gp %u) re-derives to its own class", id, n_gp);
                if (C.packed) CHECK(back == (int)(C.nxp | (p8 ? POD_INERT_ID0 : POD_SIG_IDS)), "free slot of class %d read back %d", id, back);
            }
        }
    std::printf("%ld pods round-tripped over %zu classes\n", pods, reached.size());
    std::printf("%ld checks held, %ld failed\n", held, failed);
    return failed ? 1 : 0;
}
