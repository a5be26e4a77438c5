// node_compact_check — stand-alone check of the node-table compaction plan
// (plan_node_compact, plan_runs: esc_node_layout.h).
//
// Every generated table is planned twice: by plan_node_compact, and naively here — the live
// slots listed one by one, the capacities from the rules written out again, the runs cut the
// way esc_load_placement cut them before the rule was a function.  Every field must agree.
// Tables past the limits are given to the plan alone and must be refused.  Exit status 0: every
// check held (tests/test_node_compact.py builds it with the host compiler and the address and
// undefined-behaviour sanitizers).
#include <cstdio>
#include <random>
#include <string>

#include "esc_node_layout.h"

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

struct Table {
    std::vector<uint32_t> flags, label0, run_off, run_len;
    std::vector<int32_t> run_pod;
};

// A table of `absent.size()` slots; live slot j carries j % 4 extra labels (none without a
// first label, every 5th slot) and a run of len(j) pods with 3 spare positions behind it.
template <class Len>
Table make_table(const std::vector<bool>& absent, Len len) {
    Table t;
    const size_t n = absent.size();
    int32_t pod = 0;
    t.run_off.push_back(0);
    for (size_t j = 0; j < n; ++j) {
        const bool bare = j % 5 == 4;
        t.flags.push_back((absent[j] ? ESC_NF_ABSENT : 0u) | (bare ? 0u : (uint32_t)(j % 4) << ESC_NF_XLBL_SHIFT) | (j & 3u));
        t.label0.push_back(bare ? NONE : (uint32_t)(j % 7));
        const uint32_t l = len(j);
        t.run_len.push_back(l);
        for (uint32_t k = 0; k < l; ++k) t.run_pod.push_back(pod++);
        for (int k = 0; k < 3; ++k) t.run_pod.push_back(-1);
        t.run_off.push_back((uint32_t)t.run_pod.size());
    }
    return t;
}

// esc_load_placement's capacity rule as it stood before plan_runs.
std::vector<uint32_t> former_runs(const std::vector<uint32_t>& cnt, int64_t NC, int64_t N, int64_t bound, int64_t live, double f) {
    const uint64_t cap_new = f > 0 ? (uint64_t)std::ceil((double)bound / (double)std::max<int64_t>(live, 1) * (1.0 + f)) + 4 : 0;
    std::vector<uint32_t> off((size_t)NC + 1, 0);
    for (int64_t j = 0; j < NC; ++j) {
        const uint32_t c = j < N ? cnt[j] : 0;
        const uint64_t own = c + (f > 0 ? (uint64_t)std::ceil(c * f) + 2 : 0);
        const uint64_t cap = j >= N ? cap_new : std::max(own, cap_new);
        off[j + 1] = off[j] + (uint32_t)cap;
    }
    return off;
}

void check_table(const std::string& name, const Table& t, double f, int64_t min_slots, int64_t min_xl, bool placed) {
    g_case = name;
    const int64_t n = (int64_t)t.flags.size();
    CompactPlan P;
    const int32_t rc = plan_node_compact(P, t.flags.data(), t.label0.data(), n, f, min_slots, min_xl,
                                         placed ? t.run_off.data() : nullptr, placed ? t.run_len.data() : nullptr,
                                         placed ? t.run_pod.data() : nullptr);
    CHECK(rc == ESC_OK);
    if (rc != ESC_OK) return;
    // the naive recomputation
    std::vector<uint32_t> live;
    int64_t w = 0;
    for (int64_t j = 0; j < n; ++j)
        if (!(t.flags[j] & ESC_NF_ABSENT)) {
            live.push_back((uint32_t)j);
            if (t.label0[j] != NONE) w += (t.flags[j] >> ESC_NF_XLBL_SHIFT) & ESC_PF_CNT_MASK;
        }
    const int64_t L = (int64_t)live.size();
    const int64_t spare_slots = f > 0 ? (int64_t)std::ceil((double)L * f) + 64 : 0;
    const int64_t spare_xl = f > 0 ? (int64_t)std::ceil((double)w * f) + 256 : 0;
    const int64_t n_cap = L + std::max(spare_slots, min_slots), xl_cap = w + std::max(spare_xl, min_xl);
    CHECK(P.n_live == L && P.n_cap == n_cap && P.xl_words == w && P.xl_cap == xl_cap);
    CHECK(P.n_cap - L >= min_slots && P.xl_cap - w >= min_xl);
    CHECK((int64_t)P.new_of.size() == n && (int64_t)P.src_of.size() == n_cap);
    if ((int64_t)P.new_of.size() != n || (int64_t)P.src_of.size() != n_cap) return;
    for (int64_t j = 0, k = 0; j < n; ++j) {
        const bool a = t.flags[j] & ESC_NF_ABSENT;
        CHECK(P.new_of[j] == (a ? NONE : (uint32_t)k));      // dense, ascending in the old index
        if (!a) ++k;
    }
    for (int64_t i = 0; i < n_cap; ++i) CHECK(P.src_of[i] == (i < L ? live[i] : NONE));
    if (!placed) {
        CHECK(P.run_off.empty() && P.moves.empty() && P.unbind.empty());
        return;
    }
    std::vector<uint32_t> cnt((size_t)n_cap, 0);
    std::vector<int32_t> dead;
    int64_t bound = 0;
    for (int64_t j = 0; j < n; ++j) {
        if (!(t.flags[j] & ESC_NF_ABSENT)) { bound += t.run_len[j]; continue; }
        for (uint32_t k = 0; k < t.run_len[j]; ++k) dead.push_back(t.run_pod[t.run_off[j] + k]);
    }
    for (int64_t i = 0; i < L; ++i) cnt[i] = t.run_len[live[i]];
    const std::vector<uint32_t> off = former_runs(cnt, n_cap, L, bound, L, f);
    CHECK(P.bound == bound && P.unbind == dead && P.run_off == off);
    CHECK((int64_t)P.run_len.size() == std::max<int64_t>(n_cap, 1));
    size_t m = 0;
    for (int64_t i = 0; i < n_cap; ++i) {
        CHECK(P.run_len[i] == cnt[i]);
        CHECK(off[i + 1] - off[i] >= cnt[i]);                  // a run holds what it held
        if (f > 0 && i < L) CHECK(off[i + 1] - off[i] >= cnt[i] + 2);   // and takes another pod
        if (!cnt[i]) continue;
        CHECK(m < P.moves.size());
        if (m >= P.moves.size()) return;
        CHECK(P.moves[m].src == t.run_off[live[i]] && P.moves[m].dst == off[i] && P.moves[m].len == cnt[i]);
        ++m;
    }
    CHECK(m == P.moves.size());
}

std::vector<bool> pattern(size_t n, int kind) {
    std::vector<bool> a(n, false);
    for (size_t j = 0; j < n; ++j) switch (kind) {
        case 0: break;                                         // no absent slot
        case 1: a[j] = true; break;                            // every slot absent
        case 2: a[j] = j < n / 3; break;                       // an absent run at the start
        case 3: a[j] = j >= n / 3 && j < 2 * n / 3; break;     // in the middle
        case 4: a[j] = j >= n - n / 3; break;                  // at the end
        case 5: a[j] = j % 2 == 0; break;                      // alternating, first absent
        case 6: a[j] = j % 2 == 1; break;
        default: a[j] = (j * 2654435761u >> 7) % 3 == 0;
    }
    return a;
}

void limits() {
    g_case = "limits";
    CompactPlan P;
    const std::vector<uint32_t> f3(3, 0), l3(3, 1);
    CHECK(plan_node_compact(P, f3.data(), l3.data(), 3, 0.0, -1, 0, nullptr, nullptr, nullptr) == ESC_E_INVAL);
    CHECK(plan_node_compact(P, f3.data(), l3.data(), 3, 0.0, 0, -1, nullptr, nullptr, nullptr) == ESC_E_INVAL);
    // the age index's node field: a table of 2^28 slots is refused, nothing materialised
    CHECK(plan_node_compact(P, f3.data(), l3.data(), 3, 0.0, ((int64_t)1 << 28) - 3, 0, nullptr, nullptr, nullptr) == ESC_E_LIMIT);
    CHECK(P.src_of.empty());
    CHECK(plan_node_compact(P, f3.data(), l3.data(), 3, 0.5, (int64_t)1 << 28, 0, nullptr, nullptr, nullptr) == ESC_E_LIMIT);
    CHECK(plan_node_compact(P, f3.data(), l3.data(), 3, 0.0, INT64_MAX, 0, nullptr, nullptr, nullptr) == ESC_E_LIMIT);
    CHECK(plan_node_compact(P, f3.data(), l3.data(), 3, 0.0, 0, INT64_MAX, nullptr, nullptr, nullptr) == ESC_E_LIMIT);
    CHECK(plan_node_compact(P, f3.data(), l3.data(), 3, 0.0, 0, (int64_t)0xFFFFFFFF - 1, nullptr, nullptr, nullptr) == ESC_OK);
    CHECK(plan_node_compact(P, f3.data(), l3.data(), 3, 0.0, 1000, 0, nullptr, nullptr, nullptr) == ESC_OK && P.n_cap == 1003);
    // PodRefs past 32-bit offsets: two live runs of 2^31 (no dead run: no pod is listed)
    const std::vector<uint32_t> f2(2, 0), l2(2, 1), off{0, 0x80000000u, 0xFFFFFFFFu};
    std::vector<uint32_t> len{0x80000000u, 0x7FFFFFFFu};
    CHECK(plan_node_compact(P, f2.data(), l2.data(), 2, 0.0, 0, 0, off.data(), len.data(), nullptr) == ESC_E_LIMIT);
    len[1] = 0x7FFFFFFEu;
    CHECK(plan_node_compact(P, f2.data(), l2.data(), 2, 0.0, 0, 0, off.data(), len.data(), nullptr) == ESC_OK);
    CHECK(P.run_off.size() == 3 && P.run_off[2] == 0xFFFFFFFEu && P.moves.size() == 2 && P.bound == (int64_t)0xFFFFFFFEll);
    len[0] = len[1] = 0x60000000u;                            // the spare fraction takes them past it
    CHECK(plan_node_compact(P, f2.data(), l2.data(), 2, 0.5, 0, 0, off.data(), len.data(), nullptr) == ESC_E_LIMIT);
}

void run_rule() {
    g_case = "run rule";
    std::mt19937_64 rng(12345);
    for (int it = 0; it < 400; ++it) {
        const int64_t N = (int64_t)(rng() % 40), NC = N + (int64_t)(rng() % 9);
        const double f = it % 4 == 0 ? 0.0 : (double)(rng() % 200) / 100.0;
        std::vector<uint32_t> cnt((size_t)NC, 0);
        int64_t bound = 0, live = 0;
        for (int64_t j = 0; j < N; ++j) {
            cnt[j] = (uint32_t)(rng() % 3 == 0 ? 0 : rng() % 500);
            bound += cnt[j];
            live += rng() % 5 != 0;
        }
        std::vector<uint32_t> off;
        CHECK(plan_runs(off, cnt.data(), NC, N, bound, live, f) == ESC_OK);
        CHECK(off == former_runs(cnt, NC, N, bound, live, f));
    }
}

}  // namespace

int main() {
    limits();
    run_rule();
    const uint32_t lens[] = {0, 1, 63, 64, 65, 300};
    for (size_t n : {(size_t)0, (size_t)1, (size_t)6, (size_t)255, (size_t)256, (size_t)257, (size_t)383, (size_t)384,
                     (size_t)385, (size_t)600})
        for (int kind = 0; kind < 8; ++kind)
            for (double f : {0.0, 0.25}) {
                const std::vector<bool> a = pattern(n, kind);
                const Table t = make_table(a, [&](size_t j) { return lens[(j * 7 + kind) % 6]; });
                // each minimum below the spare rule's room, above it, and zero
                for (int64_t ms : {(int64_t)0, (int64_t)5, (int64_t)1000})
                    for (int64_t mx : {(int64_t)0, (int64_t)8, (int64_t)5000})
                        for (bool placed : {false, true})
                            check_table("n=" + std::to_string(n) + " kind=" + std::to_string(kind) + " f=" + std::to_string(f) +
                                            " ms=" + std::to_string(ms) + " mx=" + std::to_string(mx) + (placed ? " placed" : ""),
                                        t, f, ms, mx, placed);
            }
    // L at 255, 256 and 257 behind absent slots
    for (size_t L : {(size_t)255, (size_t)256, (size_t)257}) {
        std::vector<bool> a(L + 300, false);
        for (size_t j = 0; j < 300; ++j) a[j] = true;
        check_table("300 absent then " + std::to_string(L), make_table(a, [](size_t j) { return (uint32_t)(j % 3); }), 0.5, 0, 0, true);
    }
    std::printf("%d checks held, %d failed\n", g_checked - g_failed, g_failed);
    return g_failed ? 1 : 0;
}
