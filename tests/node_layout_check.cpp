// node_layout_check — stand-alone check of the node-side layout plan (esc_node_layout.h).
//
// Every case is laid out twice: by plan_node_layout, from the counts alone, and the way
// esc_load_nodes did before the plan existed — the (pair, node) list materialised with its
// spare entries, sorted, scanned for piece starts (the first entry, a pair change, a multiple
// of PIECE_ALIGN) and pp_off found by lower bound.  Every field must agree.  Counts past the
// 32-bit limits are given to the plan alone (nothing is materialised) and must be refused.
// Exit status 0: every check held (tests/test_node_layout.py builds it with the host compiler
// and the address and undefined-behaviour sanitizers).
#include <cstdio>
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

// The former layout of esc_load_nodes, from the materialised entries.
struct Former {
    std::vector<uint32_t> pair_lo, pair_next, pair_end, piece_off, piece_pair, pp_off, span_off, span_e, list_off;
    std::vector<uint32_t> e_node;
    int64_t n_pieces = 0, n_entries = 0, pc_lo = 0, pc_hi = 0, node_bytes = 0;
};

Former former_layout(const std::vector<int64_t>& live, double sf, const std::vector<TailRun>& tail, uint32_t q_lo,
                     uint32_t q_hi, bool pk_ok, const std::vector<uint32_t>& gpair) {
    Former F;
    const uint32_t n_gp = (uint32_t)live.size();
    std::vector<uint64_t> ent;
    uint32_t node = 0;
    for (uint32_t q = 0; q < n_gp; ++q)
        for (int64_t k = 0; k < live[q]; ++k) ent.push_back(((uint64_t)q << 32) | node++);
    for (const TailRun& r : tail)
        for (uint64_t k = 0; k < r.len; ++k) ent.push_back(((uint64_t)r.pair << 32) | node++);
    for (uint32_t q = 0; q < n_gp && sf > 0; ++q) {
        const int64_t sp = (int64_t)std::ceil((double)live[q] * sf) + 4;
        for (int64_t k = 0; k < sp; ++k) ent.push_back(((uint64_t)q << 32) | 0xFFFFFFFFull);
    }
    std::sort(ent.begin(), ent.end());
    const int64_t E = (int64_t)ent.size();
    F.e_node.resize((size_t)E);
    for (int64_t k = 0; k < E; ++k) {
        const uint32_t q = (uint32_t)(ent[k] >> 32);
        if (k == 0 || q != F.piece_pair.back() || k % PIECE_ALIGN == 0) {
            F.piece_off.push_back((uint32_t)k);
            F.piece_pair.push_back(q);
        }
        F.e_node[k] = (uint32_t)ent[k];
    }
    F.n_entries = E;
    F.n_pieces = (int64_t)F.piece_pair.size();
    F.piece_off.push_back((uint32_t)E);
    F.pp_off.resize((size_t)n_gp + 1);
    for (uint32_t q = 0; q <= n_gp; ++q)
        F.pp_off[q] = (uint32_t)(std::lower_bound(F.piece_pair.begin(), F.piece_pair.end(), q) - F.piece_pair.begin());
    F.pc_lo = F.pp_off[q_lo];
    F.pc_hi = F.pp_off[q_hi];
    const int64_t per_entry = pk_ok ? 16 : 20;
    for (int64_t p = F.pc_lo; p < F.pc_hi; ++p) {
        F.node_bytes += 8;
        if (F.piece_pair[p] < n_gp) F.node_bytes += per_entry * (int64_t)(F.piece_off[p + 1] - F.piece_off[p]);
    }
    F.span_off.assign(1, (uint32_t)F.pc_lo);
    {
        int64_t p_end = F.pc_lo, acc = 0;
        while (p_end < F.pc_hi && F.piece_pair[p_end] < n_gp) ++p_end;
        int64_t np = 0;
        for (int64_t p = F.pc_lo; p < p_end; ++p) {
            const int64_t len = (int64_t)F.piece_off[p + 1] - F.piece_off[p];
            if (acc > 0 && (acc + len > NODE_SPAN || np == 63)) { F.span_off.push_back((uint32_t)p); acc = 0; np = 0; }
            acc += len;
            ++np;
        }
        if (p_end > F.pc_lo) F.span_off.push_back((uint32_t)p_end);
    }
    F.span_e.resize(F.span_off.size());
    for (size_t w = 0; w < F.span_off.size(); ++w) F.span_e[w] = F.piece_off[F.span_off[w]];
    F.list_off.assign(gpair.size() + 1, 0);
    for (size_t g = 0; g < gpair.size(); ++g) {
        const uint32_t q = gpair[g];
        F.list_off[g + 1] = F.list_off[g] + (F.piece_off[F.pp_off[q + 1]] - F.piece_off[F.pp_off[q]]);
    }
    F.pair_lo.resize(n_gp);
    F.pair_next.resize(n_gp);
    F.pair_end.resize(n_gp);
    for (uint32_t q = 0; q < n_gp; ++q) {
        const uint32_t a = F.piece_off[F.pp_off[q]], z = F.piece_off[F.pp_off[q + 1]];
        F.pair_end[q] = z;
        F.pair_lo[q] = a;
        F.pair_next[q] = a + (uint32_t)live[q];
    }
    return F;
}

void check_case(const std::string& name, const std::vector<int64_t>& live, double sf, const std::vector<TailRun>& tail,
                uint32_t q_lo, uint32_t q_hi, bool pk_ok, const std::vector<uint32_t>& gpair) {
    g_case = name + " f=" + std::to_string(sf) + " q=[" + std::to_string(q_lo) + "," + std::to_string(q_hi) + ") pk=" +
             std::to_string((int)pk_ok) + " tail=" + std::to_string(tail.size());
    NodeLayout L;
    const int32_t rc = plan_node_layout(L, live, sf, tail, q_lo, q_hi, pk_ok, gpair.data(), (int32_t)gpair.size());
    CHECK(rc == ESC_OK);
    if (rc != ESC_OK) return;
    const Former F = former_layout(live, sf, tail, q_lo, q_hi, pk_ok, gpair);
    CHECK(L.pair_lo == F.pair_lo);
    CHECK(L.pair_next == F.pair_next);
    CHECK(L.pair_end == F.pair_end);
    CHECK(L.piece_off == F.piece_off);
    CHECK(L.piece_pair == F.piece_pair);
    CHECK(L.pp_off == F.pp_off);
    CHECK(L.n_pieces == F.n_pieces);
    CHECK(L.n_entries == F.n_entries);
    CHECK(L.pc_lo == F.pc_lo && L.pc_hi == F.pc_hi);
    CHECK(L.span_off == F.span_off);
    CHECK(L.span_e == F.span_e);
    CHECK(L.node_bytes == F.node_bytes);
    CHECK(L.list_off == F.list_off);
    // the pieces: whole, of one pair, inside one alignment block, at most NODE_PIECE entries
    CHECK((int64_t)L.piece_off.size() == L.n_pieces + 1 && (int64_t)L.piece_pair.size() == L.n_pieces);
    for (int64_t p = 0; p < L.n_pieces; ++p) {
        const uint32_t a = L.piece_off[p], z = L.piece_off[p + 1];
        CHECK(a < z && z - a <= (uint32_t)NODE_PIECE && a / PIECE_ALIGN == (z - 1) / PIECE_ALIGN);
    }
    // the spans: whole pieces covering [pc_lo, pc_hi) exactly, <= 63 pieces, <= NODE_SPAN
    // entries unless a single piece is larger
    CHECK(!L.span_off.empty() && L.span_off.front() == (uint32_t)L.pc_lo);
    CHECK(L.pc_hi > L.pc_lo ? L.span_off.back() == (uint32_t)L.pc_hi : L.span_off.size() == 1);
    for (size_t w = 0; w + 1 < L.span_off.size(); ++w) {
        const uint32_t a = L.span_off[w], z = L.span_off[w + 1];
        CHECK(a < z && z - a <= 63);
        CHECK(z - a == 1 || L.piece_off[z] - L.piece_off[a] <= (uint32_t)NODE_SPAN);
        CHECK(L.span_e[w] == L.piece_off[a] && L.span_e[w + 1] == L.piece_off[z]);
    }
    // every group's facts: its pair's pieces clipped to this rank's, allNodes[0] = the pair's
    // first entry unless that one is spare
    for (size_t g = 0; g < gpair.size(); ++g) {
        const uint32_t q = gpair[g], p0 = F.pp_off[q], p1 = F.pp_off[q + 1];
        const bool any = p1 > p0 && F.e_node[F.piece_off[p0]] != NONE;
        const uint32_t first = L.pair_next[q] > L.pair_lo[q] ? F.e_node[L.pair_lo[q]] : NONE;
        const GroupNode x = group_node(L, q, first, 1000 + (int64_t)first, 2000 + (int64_t)first);
        int64_t plo = std::max<int64_t>(p0, F.pc_lo), phi = std::min<int64_t>(p1, F.pc_hi);
        if (phi < plo) phi = plo;
        CHECK(x.plo == plo && x.phi == phi);
        CHECK(any == (first != NONE));
        CHECK(x.first == (any ? (int64_t)F.e_node[F.piece_off[p0]] : INT64_MAX));
        CHECK(x.first_cpu == (any ? 1000 + x.first : 0) && x.first_mem == (any ? 2000 + x.first : 0));
    }
}

// A case over both spare settings, both entry formats, every tail and every owned pair range.
void sweep(const std::string& name, const std::vector<int64_t>& live, const std::vector<uint32_t>& gpair,
           bool every_range) {
    const uint32_t n_gp = (uint32_t)live.size();
    const std::vector<std::vector<TailRun>> tails = {
        {},                                                   // nothing behind the group pairs
        {{n_gp + 3, 300}},                                    // one non-group pair
        {{n_gp, 1}, {n_gp + 1, 255}, {n_gp + 7, 513}, {n_gp + 8, 2}},
        {{NONE, 0}},                                          // a rebuild's single run, empty
        {{NONE, 777}},                                        // and with entries
    };
    for (double sf : {0.0, 0.02, 0.5})
        for (size_t t = 0; t < tails.size(); ++t)
            for (int pk = 0; pk < 2; ++pk) {
                if (!every_range) {
                    check_case(name, live, sf, tails[t], 0, n_gp, pk != 0, gpair);
                    continue;
                }
                for (uint32_t lo = 0; lo <= n_gp; ++lo)
                    for (uint32_t hi = lo; hi <= n_gp; ++hi) check_case(name, live, sf, tails[t], lo, hi, pk != 0, gpair);
            }
}

std::vector<uint32_t> one_group_per_pair(size_t n_gp) {
    std::vector<uint32_t> g(n_gp);
    for (size_t q = 0; q < n_gp; ++q) g[q] = (uint32_t)q;
    return g;
}

void expect_limit(const std::string& name, const std::vector<int64_t>& live, double sf, const std::vector<TailRun>& tail,
                  const std::vector<uint32_t>& gpair, int32_t want) {
    g_case = name;
    NodeLayout L;
    const uint32_t n_gp = (uint32_t)live.size();
    CHECK(plan_node_layout(L, live, sf, tail, 0, n_gp, true, gpair.data(), (int32_t)gpair.size()) == want);
}

}  // namespace

int main() {
    // the capacity rules
    g_case = "capacity rules";
    CHECK(spare_entries(100, 0.02) == 6 && spare_entries(101, 0.02) == 7 && spare_entries(0, 0.5) == 4);
    CHECK(spare_entries(100, 0.0) == 0 && spare_entries(0, 0.0) == 0);
    CHECK(table_slots(1000, 0.02) == 1000 + 20 + 64 && table_slots(0, 0.02) == 64 && table_slots(1000, 0.0) == 1000);
    CHECK(label_words(1000, 0.02) == 1000 + 20 + 256 && label_words(0, 0.02) == 256 && label_words(7, 0.0) == 7);

    // an empty table, with and without groups; every pair empty
    sweep("no pairs", {}, {}, true);
    sweep("one empty pair", {0}, {0}, true);
    sweep("every pair empty", {0, 0, 0, 0, 0}, {0, 1, 2, 3, 4}, true);
    // pair lengths around the alignment, singly and back to back: cuts fall at, just before and
    // just after a multiple inside a pair and at a pair boundary
    const std::vector<int64_t> lens = {1, 255, 256, 257, 600, 1025};
    for (int64_t a : lens) {
        sweep("single " + std::to_string(a), {a}, {0}, true);
        for (int64_t b : lens) {
            sweep("pair " + std::to_string(a) + "+" + std::to_string(b), {a, b}, {0, 1}, true);
            sweep("around an empty pair " + std::to_string(a) + "+0+" + std::to_string(b), {a, 0, b}, {0, 1, 2}, false);
        }
    }
    sweep("all lengths", lens, one_group_per_pair(lens.size()), true);
    sweep("all lengths, reversed", {1025, 600, 257, 256, 255, 1}, one_group_per_pair(lens.size()), true);
    // two groups sharing a pair, a pair no group selects, groups out of pair order
    sweep("shared pair", {300, 5, 257}, {0, 0, 2}, true);
    sweep("groups out of order", {10, 256, 0, 1025}, {3, 1, 1, 0, 2, 3}, true);
    // 64 and more one-entry pieces in a row: the 63-piece limit of a span (no spare room, so a
    // piece is one entry), and beside longer pieces
    {
        std::vector<int64_t> ones(70, 1), mixed(200, 1);
        for (size_t q = 0; q < mixed.size(); q += 67) mixed[q] = 250;
        for (const std::vector<int64_t>& v : {std::vector<int64_t>(64, 1), ones, std::vector<int64_t>(127, 1), mixed}) {
            const std::vector<uint32_t> gp = one_group_per_pair(v.size());
            for (double sf : {0.0, 0.02})
                for (const std::vector<TailRun>& t : {std::vector<TailRun>{}, std::vector<TailRun>{{NONE, 5}}}) {
                    const uint32_t n = (uint32_t)v.size();
                    check_case("one-entry pieces " + std::to_string(v.size()), v, sf, t, 0, n, true, gp);
                    check_case("one-entry pieces " + std::to_string(v.size()), v, sf, t, 1, n, false, gp);
                    check_case("one-entry pieces " + std::to_string(v.size()), v, sf, t, 3, n - 2, true, gp);
                    check_case("one-entry pieces " + std::to_string(v.size()), v, sf, t, n / 2, n / 2, true, gp);
                }
        }
    }
    // counts past the 32-bit limits (given to the plan alone): the entry total through the live
    // counts, the spare room and the tail, and a list offset through groups sharing a pair
    expect_limit("entry total: one pair", {0xFFFFFFFFll}, 0.0, {}, {0}, ESC_E_LIMIT);
    expect_limit("entry total: several pairs", {0x7FFFFFFFll, 0x7FFFFFFFll, 1}, 0.0, {}, {}, ESC_E_LIMIT);
    expect_limit("entry total: spare room", {0xFFFFFFF0ll}, 0.5, {}, {}, ESC_E_LIMIT);
    expect_limit("entry total: an empty pair's spare room", {0xFFFFFFF3ll, 0}, 1e-9, {}, {}, ESC_E_LIMIT);
    expect_limit("entry total: tail", {100}, 0.0, {{NONE, 0xFFFFFFFFull - 100}}, {0}, ESC_E_LIMIT);
    expect_limit("entry total: several tail runs", {100}, 0.0, {{1, 0x80000000ull}, {2, 0x80000000ull}}, {0}, ESC_E_LIMIT);
    expect_limit("list offset under the limit", {0x10000000ll}, 0.0, {}, std::vector<uint32_t>(15, 0), ESC_OK);
    expect_limit("list offset", {0x10000000ll}, 0.0, {}, std::vector<uint32_t>(16, 0), ESC_E_LIMIT);

    if (g_failed) {
        std::fprintf(stderr, "node layout check: %d of %d checks FAILED\n", g_failed, g_checked);
        return 1;
    }
    std::printf("node layout check: %d checks held\n", g_checked);
    return 0;
}
