// CPU check of the compare esc_pods_verify runs on the device (kb_pod_same / c_pod_same,
// escalator_amd/csrc/esc_kblock.h): the writers' own walks with a put that reads and compares.
// For every class the K layout can hold, and for C slots of several rooms: random pods written
// with kb_write_pod / c_write_pod compare equal at every slot 0..255 (all four s % 4 cases of
// kb_pos64), differ after every single-field change the class stores (cpu +-1, mem +-1, pair0,
// each extra pair, each record's cpu and mem, an init key present <-> absent), and a change to
// slot s leaves slots s - 1 and s + 1 equal.  The lossy encodings compare as stored: a packed
// class keeps the fold of the records, a packed small class one blocks-default bit and no pair
// past its field.  Stand-alone; built by tests/test_pod_verify_host.py with the host compiler
// under AddressSanitizer and UBSan.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "esc_pod_layout.h"

using namespace esc;

static long held = 0, failed = 0;
#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (cond) ++held;                                       \
        else { if (++failed <= 20) { std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } \
    } while (0)

struct Pod {
    uint32_t f, cpu0, pair0;
    int64_t mem0;
    int64_t xc[8], xm[8];
    uint32_t xp[8];
};

// ------------------------------------------------------------------ K classes
static bool k_same(const PodClass& C, const std::vector<uint32_t>& kb, int64_t s, const Pod& p) {
    return kb_pod_same(C, kb.data(), 0, s, p.f, p.cpu0, p.mem0, p.pair0, p.xc, p.xm, p.xp);
}
static void k_write(const PodClass& C, std::vector<uint32_t>& kb, int64_t s, const Pod& p) {
    kb_write_pod(C, 0, s, p.f, p.cpu0, p.mem0, p.pair0, p.xc, p.xm, p.xp,
                 [&](int width, int64_t at, uint64_t v) { put_kb(kb.data(), width, at, v); });
}

// A pod of class C with every value strictly inside the ranges the class stores exactly, so
// that +-1 and another pair are representable: no daemonset bit (a packed small daemonset pod
// stores no pair), a packed class's pods without records (their fold is checked on its own).
static Pod k_pod(const PodClass& C, std::mt19937_64& g) {
    Pod p{};
    const uint32_t own[] = {0, ESC_PF_STATIC, ESC_PF_HAS_SEL, ESC_PF_AFF_BLOCK};
    p.f = own[g() % 4] | C.nxp << ESC_PF_XPAIR_SHIFT;
    if (!C.packed) p.f |= C.xreg << ESC_PF_XREG_SHIFT | C.xinit << ESC_PF_XINIT_SHIFT | (C.ovh ? ESC_PF_HAS_OVH : 0u);
    const uint64_t cpu_hi = C.packed == 2 ? KP8_CPU_MASK : (C.packed ? KP_CPU_ABSENT - 1 : 0xFFFFFFFFull);
    const uint64_t mem_hi = C.packed == 2 ? KP8_MEM_MASK : (C.packed ? KP_MEM_ABSENT - 1 : (uint64_t)INT64_MAX);
    p.cpu0 = (uint32_t)(1 + g() % (cpu_hi - 1));
    p.mem0 = (int64_t)(1 + g() % (mem_hi - 1));
    const uint32_t pair_hi = C.packed == 2 ? KP8_PAIR_NONE - 1 : (C.packed ? KP_PAIR_NONE - 1 : NONE - 1);
    p.pair0 = (uint32_t)(g() % pair_hi);
    for (uint32_t k = 0; k < C.nxp; ++k) p.xp[k] = (uint32_t)(g() % (C.packed == 2 ? KP8_XP_NONE - 1 : NONE - 1));
    for (uint32_t k = 0; k < kb_nrec(C) && !C.packed; ++k) {
        p.xc[k] = (int64_t)(g() % (uint64_t(1) << 40)) + 1;
        p.xm[k] = (int64_t)(g() % (uint64_t(1) << 50)) + 1;
    }
    return p;
}

static void k_class_checks(int id, std::mt19937_64& g) {
    PodClass C = pod_class_of_id(id);
    C.t0 = 0; C.t1 = 1; C.kb0 = 0;
    std::vector<uint32_t> kb((size_t)C.wt * KB_UNIT, 0);
    write_free_tile(C, kb.data());
    std::vector<Pod> pods(TILE);
    for (int64_t s = 0; s < TILE; ++s) { pods[s] = k_pod(C, g); k_write(C, kb, s, pods[s]); }
    for (int64_t s = 0; s < TILE; ++s) CHECK(k_same(C, kb, s, pods[s]), "class %d slot %lld: the written pod differs", id, (long long)s);
    const uint32_t R = C.packed ? 0 : kb_nrec(C);
    for (int64_t s = 0; s < TILE; ++s) {
        const Pod& p = pods[s];
        std::vector<Pod> changed;
        auto with = [&](auto&& edit) { Pod q = p; edit(q); changed.push_back(q); };
        with([](Pod& q) { q.cpu0 += 1; });
        with([](Pod& q) { q.cpu0 -= 1; });
        with([](Pod& q) { q.mem0 += 1; });
        with([](Pod& q) { q.mem0 -= 1; });
        with([](Pod& q) { q.pair0 = q.pair0 ? q.pair0 - 1 : 1; });
        for (uint32_t k = 0; k < C.nxp; ++k) with([k](Pod& q) { q.xp[k] = q.xp[k] ? q.xp[k] - 1 : 1; });
        for (uint32_t k = 0; k < R; ++k) {
            with([k](Pod& q) { q.xc[k] += 1; });
            with([k](Pod& q) { q.xm[k] -= 1; });
            if (k >= C.xreg && k < C.xreg + C.xinit) {       // an init key present <-> absent
                with([k](Pod& q) { q.xc[k] = INT64_MIN; });
                with([k](Pod& q) { q.xm[k] = INT64_MIN; });
            }
        }
        for (size_t j = 0; j < changed.size(); ++j) CHECK(!k_same(C, kb, s, changed[j]), "class %d slot %lld change %zu compares equal", id, (long long)s, j);
        // the same the other way round: the slot rewritten, the old pod offered; its neighbours stay
        if (s % 37 == 0 || s == 255) {
            for (size_t j = 0; j < changed.size(); ++j) {
                k_write(C, kb, s, changed[j]);
                CHECK(!k_same(C, kb, s, p) && k_same(C, kb, s, changed[j]), "class %d slot %lld rewritten %zu", id, (long long)s, j);
                if (s > 0) CHECK(k_same(C, kb, s - 1, pods[s - 1]), "class %d: slot %lld's write reached slot s - 1", id, (long long)s);
                if (s + 1 < TILE) CHECK(k_same(C, kb, s + 1, pods[s + 1]), "class %d: slot %lld's write reached slot s + 1", id, (long long)s);
            }
            k_write(C, kb, s, p);
        }
    }
    if (C.packed) {
        // the stored form decides.  A packed class keeps the fold: two regular containers with
        // the same total compare equal to the one-container pod, another total differs.
        const int64_t s = 77;
        Pod p = pods[s];
        p.cpu0 = 1000; p.mem0 = 4096;
        k_write(C, kb, s, p);
        Pod q = p;
        q.f |= 1u << ESC_PF_XREG_SHIFT;
        q.cpu0 = 400; q.xc[0] = 600; q.mem0 = 96; q.xm[0] = 4000;
        CHECK(k_same(C, kb, s, q), "class %d: a split with the same request differs", id);
        q.xc[0] = 601;
        CHECK(!k_same(C, kb, s, q), "class %d: a split with another request compares equal", id);
    }
    if (C.packed == 2) {
        // one blocks-default bit for static / has-selector / affinity; pair0 past the 14-bit
        // field and extra pairs past 16 bits are all "none"
        const int64_t s = 130;
        Pod p = pods[s];
        p.f = (p.f & ~KP_POD_FLAGS) | ESC_PF_STATIC;
        p.pair0 = 20000;
        for (uint32_t k = 0; k < C.nxp; ++k) p.xp[k] = 0x10000u + k;
        k_write(C, kb, s, p);
        Pod q = p;
        q.f = (q.f & ~KP_POD_FLAGS) | ESC_PF_HAS_SEL;
        q.pair0 = 30000;
        for (uint32_t k = 0; k < C.nxp; ++k) q.xp[k] = 0x20000u + k;
        CHECK(k_same(C, kb, s, q), "class %d: the one blocks-default bit / the none pairs differ", id);
        q.f &= ~KP_POD_FLAGS;
        CHECK(!k_same(C, kb, s, q), "class %d: blocks-default cleared compares equal", id);
        q = p;
        q.f |= ESC_PF_DAEMONSET;
        CHECK(!k_same(C, kb, s, q), "class %d: the daemonset bit compares equal", id);
    } else if (C.packed == 1) {
        const int64_t s = 130;
        Pod p = pods[s], q = p;
        q.f = (q.f & ~KP_POD_FLAGS) | ((p.f & ESC_PF_STATIC) ? ESC_PF_HAS_SEL : ESC_PF_STATIC);
        CHECK(!k_same(C, kb, s, q), "class %d: the packed class keeps the pod's four bits", id);
    }
}

// ------------------------------------------------------------------ C slots
struct CArrs {
    std::vector<uint32_t> flags, cpu0, pair0, xp;
    std::vector<int64_t> mem0, xc_cpu, xc_mem;
};
static void c_write(CArrs& A, uint32_t cf, int64_t d, int64_t ro, int64_t po, const Pod& p) {
    c_write_pod(cf, d, ro, po, p.f, p.cpu0, p.mem0, p.pair0, p.xc, p.xm, p.xp, [&](int arr, int64_t at, uint64_t v) {
        switch (arr) {
        case CA_FLAGS: A.flags.at((size_t)at) = (uint32_t)v; break;
        case CA_CPU0: A.cpu0.at((size_t)at) = (uint32_t)v; break;
        case CA_MEM0: A.mem0.at((size_t)at) = (int64_t)v; break;
        case CA_PAIR0: A.pair0.at((size_t)at) = (uint32_t)v; break;
        case CA_XC_CPU: A.xc_cpu.at((size_t)at) = (int64_t)v; break;
        case CA_XC_MEM: A.xc_mem.at((size_t)at) = (int64_t)v; break;
        default: A.xp.at((size_t)at) = (uint32_t)v; break;
        }
    });
}
static bool c_same(const CArrs& A, uint32_t cf, int64_t d, int64_t ro, int64_t po, const Pod& p) {
    return c_pod_same(cf, d, ro, po, p.f, p.cpu0, p.mem0, p.pair0, p.xc, p.xm, p.xp, [&](int arr, int64_t at) -> uint64_t {
        switch (arr) {
        case CA_FLAGS: return A.flags.at((size_t)at);
        case CA_CPU0: return A.cpu0.at((size_t)at);
        case CA_MEM0: return (uint64_t)A.mem0.at((size_t)at);
        case CA_PAIR0: return A.pair0.at((size_t)at);
        case CA_XC_CPU: return (uint64_t)A.xc_cpu.at((size_t)at);
        case CA_XC_MEM: return (uint64_t)A.xc_mem.at((size_t)at);
        default: return A.xp.at((size_t)at);
        }
    });
}

static void c_room_checks(uint32_t rr, uint32_t ri, uint32_t rv, uint32_t rp, std::mt19937_64& g) {
    const uint32_t room = rr << ESC_PF_XREG_SHIFT | ri << ESC_PF_XINIT_SHIFT | (rv ? ESC_PF_HAS_OVH : 0u) | rp << ESC_PF_XPAIR_SHIFT;
    const int64_t nrec = rr + ri + rv, n = TILE;
    CArrs A;
    A.flags.assign(n, room | ESC_PF_DAEMONSET); A.cpu0.assign(n, 0); A.pair0.assign(n, NONE); A.mem0.assign(n, 0);
    A.xc_cpu.assign((size_t)(n * nrec), -7); A.xc_mem.assign((size_t)(n * nrec), -7); A.xp.assign((size_t)(n * rp), 12345);
    std::vector<Pod> pods(n);
    std::vector<uint32_t> cfs(n);
    for (int64_t d = 0; d < n; ++d) {
        Pod p{};
        const uint32_t xr = (uint32_t)(g() % (rr + 1)), xi = (uint32_t)(g() % (ri + 1)), ov = rv ? (uint32_t)(g() % 2) : 0;
        const uint32_t np = (uint32_t)(g() % (rp + 1));
        const uint32_t own[] = {0, ESC_PF_STATIC, ESC_PF_HAS_SEL | ESC_PF_AFF_BLOCK, ESC_PF_DAEMONSET};
        p.f = own[g() % 4] | xr << ESC_PF_XREG_SHIFT | xi << ESC_PF_XINIT_SHIFT | (ov ? ESC_PF_HAS_OVH : 0u) | np << ESC_PF_XPAIR_SHIFT;
        p.cpu0 = (uint32_t)(1 + g() % 0xFFFFFFF0u);
        p.mem0 = (int64_t)(g() % (uint64_t(1) << 60)) + 1;
        p.pair0 = (uint32_t)(g() % 1000);
        for (uint32_t k = 0; k < np; ++k) p.xp[k] = p.pair0 + 1 + k * 3 + (uint32_t)(g() % 3);
        for (uint32_t k = 0; k < xr + xi + ov; ++k) { p.xc[k] = (int64_t)(g() % 100000) + 1; p.xm[k] = (int64_t)(g() % (uint64_t(1) << 40)) + 1; }
        CHECK(c_room(room, p.f), "the pod fits its room");
        pods[d] = p;
        cfs[d] = A.flags[d];                                  // the slot's flags before the write: its room
        c_write(A, cfs[d], d, d * nrec, d * rp, p);
    }
    for (int64_t d = 0; d < n; ++d) {
        const Pod& p = pods[d];
        // (the room is the counts of the flags; the slot's own bits are rewritten from the pod)
        const uint32_t cf = A.flags[d];
        CHECK(cf == ((cfs[d] & ~KP_POD_FLAGS) | (p.f & KP_POD_FLAGS)), "slot %lld flags", (long long)d);
        CHECK(c_same(A, cf, d, d * nrec, d * rp, p), "room (%u %u %u %u) slot %lld: the written pod differs", rr, ri, rv, rp, (long long)d);
        const uint32_t xr = pf_xreg(p.f), xi = pf_xinit(p.f), nc = pf_xctr(p.f), np = pf_xpair(p.f);
        std::vector<Pod> changed;
        auto with = [&](auto&& edit) { Pod q = p; edit(q); changed.push_back(q); };
        with([](Pod& q) { q.cpu0 += 1; });
        with([](Pod& q) { q.cpu0 -= 1; });
        with([](Pod& q) { q.mem0 += 1; });
        with([](Pod& q) { q.mem0 -= 1; });
        with([](Pod& q) { q.pair0 += 1; });
        with([](Pod& q) { q.f ^= ESC_PF_STATIC; });
        for (uint32_t k = 0; k < np; ++k) with([k](Pod& q) { q.xp[k] += 1; });
        for (uint32_t k = 0; k < nc; ++k) {
            with([k](Pod& q) { q.xc[k] += 1; });
            with([k](Pod& q) { q.xm[k] -= 1; });
            if (k >= xr && k < xr + xi) {
                with([k](Pod& q) { q.xc[k] = INT64_MIN; });
                with([k](Pod& q) { q.xm[k] = INT64_MIN; });
            }
        }
        for (size_t j = 0; j < changed.size(); ++j)
            CHECK(!c_same(A, cf, d, d * nrec, d * rp, changed[j]), "room (%u %u %u %u) slot %lld change %zu compares equal", rr, ri, rv, rp, (long long)d, j);
        // the neutral remainder is compared: one word of it made wrong, then put back
        if (np < rp) {
            uint32_t& w = A.xp[(size_t)(d * rp + np)];
            CHECK(w == NONE, "a pair past the pod's is NONE");
            w = 5;
            CHECK(!c_same(A, cf, d, d * nrec, d * rp, p), "a pair in the neutral remainder compares equal");
            w = NONE;
        }
        if (xi < ri) {
            int64_t& w = A.xc_cpu[(size_t)(d * nrec + rr + xi)];
            CHECK(w == INT64_MIN, "an init key past the pod's is absent");
            w = 0;
            CHECK(!c_same(A, cf, d, d * nrec, d * rp, p), "an init key in the neutral remainder compares equal");
            w = INT64_MIN;
        }
        if (xr < rr) {
            int64_t& w = A.xc_mem[(size_t)(d * nrec + xr)];
            CHECK(w == 0, "a regular record past the pod's is 0");
            w = 1;
            CHECK(!c_same(A, cf, d, d * nrec, d * rp, p), "a record in the neutral remainder compares equal");
            w = 0;
        }
        if (d % 41 == 0 && !changed.empty()) {               // a rewrite of slot d leaves its neighbours
            for (size_t j = 0; j < changed.size(); ++j) {
                c_write(A, cf, d, d * nrec, d * rp, changed[j]);
                if (d > 0) CHECK(c_same(A, A.flags[d - 1], d - 1, (d - 1) * nrec, (d - 1) * rp, pods[d - 1]), "slot %lld's write reached d - 1", (long long)d);
                if (d + 1 < n) CHECK(c_same(A, A.flags[d + 1], d + 1, (d + 1) * nrec, (d + 1) * rp, pods[d + 1]), "slot %lld's write reached d + 1", (long long)d);
            }
            c_write(A, cf, d, d * nrec, d * rp, p);
        }
    }
}

int main() {
    std::mt19937_64 g(0xE5CA1A7E0000B0D2ull);
    int classes = 0;
    for (int id = 0; id < POD_CLASS_IDS; ++id)
        if (pod_class_holdable(id)) { k_class_checks(id, g); ++classes; }
    const uint32_t rooms[][4] = {{(uint32_t)CS_XREG, (uint32_t)CS_XINIT, 1, (uint32_t)CS_XP}, {5, 0, 0, 0}, {0, 0, 0, 4}, {2, 1, 1, 3}, {0, 4, 0, 7}};
    for (const auto& r : rooms) c_room_checks(r[0], r[1], r[2], r[3], g);
    std::printf("%d classes, %zu rooms\n", classes, sizeof rooms / sizeof rooms[0]);
    std::printf("%ld checks held, %ld failed\n", held, failed);
    return failed ? 1 : 0;
}
