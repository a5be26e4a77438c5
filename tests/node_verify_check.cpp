// CPU check of the compare esc_nodes_verify runs on the device (nv_compare,
// escalator_amd/csrc/esc_node_verify.h), over a node table this program fills itself.  Nodes with
// 0, 1, 2 and 255 extra labels sit between neighbours whose every word would differ: an equal node
// gives 0, every single-field change gives exactly its own bit, ESC_NF_TRACKED on either side gives
// 0, an absent slot gives ABSENT alone, a fact left out of the mask is neither compared nor read,
// and the reader is only ever asked for the node's own id and its own label words (the arrays are
// exactly as long as the table, so AddressSanitizer sees any read past them).  Stand-alone; built
// by tests/test_node_verify_host.py with the host compiler under AddressSanitizer and UBSan.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "esc_node_verify.h"

using namespace esc;

static long held = 0, failed = 0;
#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (cond) ++held;                                       \
        else { if (++failed <= 20) { std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } \
    } while (0)

struct Table {
    std::vector<uint32_t> flags, label0, xl;
    std::vector<int64_t> cpu, mem, created, taint_s, inst;
    std::vector<uint8_t> no_delete;
};

// What one compare asked the reader for.
struct Reads {
    long n[NV_XL + 1] = {};
    long foreign = 0;          // reads at another index than the node's id / its label words
};

static uint32_t compare(const Table& T, const NvNode& v, const std::vector<uint32_t>& xl, Reads& R) {
    const uint32_t nx = nf_xlbl(v.flags);
    return nv_compare(v, xl.data(), [&](int col, int64_t at) -> uint64_t {
        ++R.n[col];
        if (col == NV_XL ? (at < (int64_t)v.xl_dev || at >= (int64_t)v.xl_dev + nx) : at != (int64_t)v.id) ++R.foreign;
        switch (col) {
        case NV_FLAGS: return T.flags.at((size_t)at);
        case NV_LABEL0: return T.label0.at((size_t)at);
        case NV_CPU: return (uint64_t)T.cpu.at((size_t)at);
        case NV_MEM: return (uint64_t)T.mem.at((size_t)at);
        case NV_CREATED: return (uint64_t)T.created.at((size_t)at);
        case NV_TAINT_S: return (uint64_t)T.taint_s.at((size_t)at);
        case NV_NO_DELETE: return T.no_delete.at((size_t)at);
        case NV_INST: return (uint64_t)T.inst.at((size_t)at);
        default: return T.xl.at((size_t)at);
        }
    });
}

static uint32_t run(const Table& T, const NvNode& v, const std::vector<uint32_t>& xl) {
    Reads R;
    const uint32_t st = compare(T, v, xl, R);
    CHECK(R.foreign == 0, "node %u: %ld reads outside its own words", v.id, R.foreign);
    return st;
}

int main() {
    const uint32_t counts[4] = {0, 1, 2, 255};
    const uint8_t ALL = NV_M_TAINT | NV_M_NODEL | NV_M_INST;
    // slots 1, 3, 5, 7 hold the nodes; 0, 2, 4, 6, 8 the neighbours; 9 is absent
    const int N = 10;
    Table T;
    T.flags.assign(N, ESC_NF_UNSCHED | ESC_NF_TAINTED | 7u << ESC_NF_XLBL_SHIFT);
    T.label0.assign(N, 0x7000000u);
    T.cpu.assign(N, -11); T.mem.assign(N, -12); T.created.assign(N, -13); T.taint_s.assign(N, -14); T.inst.assign(N, -15);
    T.no_delete.assign(N, 0);
    std::vector<NvNode> nodes;
    std::vector<std::vector<uint32_t>> labels;
    for (int k = 0; k < 4; ++k) {
        const uint32_t id = 1 + 2 * (uint32_t)k, nx = counts[k];
        for (int j = 0; j < 3; ++j) T.xl.push_back(0x6000000u + (uint32_t)T.xl.size());   // neighbours' words
        NvNode v{};
        v.id = id;
        v.flags = (k & 1 ? ESC_NF_UNSCHED : 0u) | (k & 2 ? ESC_NF_TAINTED : 0u) | nx << ESC_NF_XLBL_SHIFT;
        v.label0 = 10 + (uint32_t)k;
        v.cpu = 4000 + k; v.mem = (int64_t(8) << 30) + k; v.created = 1700000000000000000ll + k;
        v.taint_s = k == 0 ? INT64_MIN : 1700000000 + k;
        v.no_delete = (uint8_t)(k & 1);
        v.inst = k == 1 ? INT64_MIN : 1690000000000000000ll + k;
        v.mask = ALL;
        v.xl_dev = (uint32_t)T.xl.size();
        std::vector<uint32_t> xl;
        for (uint32_t j = 0; j < nx; ++j) xl.push_back(100 + 3 * j + (uint32_t)k);
        T.xl.insert(T.xl.end(), xl.begin(), xl.end());
        T.flags[id] = v.flags; T.label0[id] = v.label0; T.cpu[id] = v.cpu; T.mem[id] = v.mem; T.created[id] = v.created;
        T.taint_s[id] = v.taint_s; T.no_delete[id] = v.no_delete; T.inst[id] = v.inst;
        nodes.push_back(v);
        labels.push_back(xl);
    }
    for (int j = 0; j < 3; ++j) T.xl.push_back(0x6000000u + (uint32_t)T.xl.size());
    T.flags[9] = ESC_NF_ABSENT;

    for (int k = 0; k < 4; ++k) {
        const NvNode v = nodes[(size_t)k];
        const std::vector<uint32_t>& xl = labels[(size_t)k];
        const uint32_t nx = counts[k];
        CHECK(run(T, v, xl) == 0, "node %d equal", k);
        {   // all eight columns are read once, every label word once
            Reads R;
            compare(T, v, xl, R);
            for (int c = 0; c < NV_XL; ++c) CHECK(R.n[c] == 1, "node %d column %d read %ld times", k, c, R.n[c]);
            CHECK(R.n[NV_XL] == (long)nx, "node %d: %ld label reads", k, R.n[NV_XL]);
        }
        // --- the batch side changed, one field at a time
        NvNode w = v;
        w.flags ^= ESC_NF_UNSCHED; CHECK(run(T, w, xl) == ESC_NV_STATUS, "unsched %d", k);
        w = v; w.flags ^= ESC_NF_TAINTED; CHECK(run(T, w, xl) == ESC_NV_STATUS, "tainted %d", k);
        w = v; w.cpu += 1; CHECK(run(T, w, xl) == ESC_NV_STATUS, "cpu %d", k);
        w = v; w.cpu ^= int64_t(1) << 40; CHECK(run(T, w, xl) == ESC_NV_STATUS, "cpu high %d", k);
        w = v; w.mem -= 1; CHECK(run(T, w, xl) == ESC_NV_STATUS, "mem %d", k);
        w = v; w.label0 += 1; CHECK(run(T, w, xl) == ESC_NV_SHAPE, "label0 %d", k);
        w = v; w.created += 1; CHECK(run(T, w, xl) == ESC_NV_SHAPE, "created %d", k);
        w = v; w.created ^= int64_t(1) << 62; CHECK(run(T, w, xl) == ESC_NV_SHAPE, "created high %d", k);
        w = v; w.taint_s = v.taint_s == INT64_MIN ? 5 : INT64_MIN; CHECK(run(T, w, xl) == ESC_NV_FACTS, "taint time %d", k);
        w = v; w.taint_s = v.taint_s == INT64_MIN ? INT64_MIN + 1 : v.taint_s + 1; CHECK(run(T, w, xl) == ESC_NV_FACTS, "taint time + 1 %d", k);
        w = v; w.no_delete = !v.no_delete; CHECK(run(T, w, xl) == ESC_NV_FACTS, "no-delete 0 <-> 1 %d", k);
        w = v; w.inst = v.inst == INT64_MIN ? 7 : v.inst - 1; CHECK(run(T, w, xl) == ESC_NV_INST, "inst %d", k);
        {   // the label count, one more and one fewer: SHAPE, and no label word is read
            std::vector<uint32_t> more = xl;
            more.push_back(0x5000000u);
            for (int d = -1; d <= 1; d += 2) {
                if ((d < 0 && nx == 0) || (d > 0 && nx == 255)) continue;
                w = v; w.flags = (v.flags & ~(0xFFu << ESC_NF_XLBL_SHIFT)) | (nx + d) << ESC_NF_XLBL_SHIFT;
                Reads R;
                CHECK(compare(T, w, more, R) == ESC_NV_SHAPE, "count %+d node %d", d, k);
                CHECK(R.n[NV_XL] == 0 && R.foreign == 0, "count %+d node %d read %ld label words", d, k, R.n[NV_XL]);
            }
        }
        if (nx) {   // the first, the middle and the last label word
            for (uint32_t at : {0u, nx / 2, nx - 1}) {
                std::vector<uint32_t> x = xl;
                x[at] += 1;
                CHECK(run(T, v, x) == ESC_NV_SHAPE, "label word %u node %d", at, k);
            }
        }
        // --- the table side changed (the device is what drifts), one word at a time
        Table U = T;
        U.flags[v.id] ^= ESC_NF_UNSCHED; CHECK(run(U, v, xl) == ESC_NV_STATUS, "dev unsched %d", k);
        U = T; U.mem[v.id] += 1; CHECK(run(U, v, xl) == ESC_NV_STATUS, "dev mem %d", k);
        U = T; U.label0[v.id] = ESC_NONE; CHECK(run(U, v, xl) == ESC_NV_SHAPE, "dev label0 %d", k);
        U = T; U.inst[v.id] = INT64_MIN + 2; CHECK(run(U, v, xl) == ESC_NV_INST, "dev inst %d", k);
        if (nx) { U = T; U.xl[v.xl_dev + nx - 1] ^= 1; CHECK(run(U, v, xl) == ESC_NV_SHAPE, "dev last label %d", k); }
        // no-delete is compared as != 0: 1 <-> 7 is no difference, 0 <-> 7 is
        U = T; U.no_delete[v.id] = v.no_delete ? 7 : 0; CHECK(run(U, v, xl) == 0, "no-delete 1 <-> 7 %d", k);
        w = v; w.no_delete = v.no_delete ? 7 : 0; CHECK(run(T, w, xl) == 0, "batch no-delete 1 <-> 7 %d", k);
        U = T; U.no_delete[v.id] = v.no_delete ? 0 : 7; CHECK(run(U, v, xl) == ESC_NV_FACTS, "no-delete 0 <-> 7 %d", k);
        // ESC_NF_TRACKED belongs to the context: flipped on either side it is no difference
        U = T; U.flags[v.id] ^= ESC_NF_TRACKED; CHECK(run(U, v, xl) == 0, "dev tracked %d", k);
        w = v; w.flags ^= ESC_NF_TRACKED; CHECK(run(T, w, xl) == 0, "batch tracked %d", k);
        // several kinds at once are or-ed
        U = T; U.cpu[v.id] -= 3; U.created[v.id] += 9; U.taint_s[v.id] ^= 4; U.inst[v.id] ^= 8;
        CHECK(run(U, v, xl) == (ESC_NV_SHAPE | ESC_NV_STATUS | ESC_NV_FACTS | ESC_NV_INST), "all four %d", k);
        U = T; U.flags[v.id] ^= ESC_NF_TAINTED; U.no_delete[v.id] = !v.no_delete;
        CHECK(run(U, v, xl) == (ESC_NV_STATUS | ESC_NV_FACTS), "status and facts %d", k);
        // an absent slot: ABSENT alone, whatever else differs
        U = T; U.flags[v.id] |= ESC_NF_ABSENT; U.cpu[v.id] += 1; U.label0[v.id] += 1; U.inst[v.id] += 1;
        {
            Reads R;
            CHECK(compare(U, v, xl, R) == ESC_NV_ABSENT, "absent %d", k);
            CHECK(R.n[NV_XL] == 0 && R.foreign == 0, "absent %d read label words", k);
        }
        // a fact left out of the mask is neither compared nor read
        const struct { uint8_t bit; int col; } facts[3] = {{NV_M_TAINT, NV_TAINT_S}, {NV_M_NODEL, NV_NO_DELETE}, {NV_M_INST, NV_INST}};
        for (const auto& f : facts) {
            U = T; U.taint_s[v.id] += 1; U.no_delete[v.id] = !v.no_delete; U.inst[v.id] += 1;
            w = v; w.mask = (uint8_t)(ALL & ~f.bit);
            Reads R;
            const uint32_t st = compare(U, w, xl, R);
            const uint32_t want = f.bit == NV_M_INST ? ESC_NV_FACTS : (ESC_NV_FACTS | ESC_NV_INST);
            CHECK(st == want, "mask without %d node %d: %u", f.bit, k, st);
            CHECK(R.n[f.col] == 0 && R.foreign == 0, "masked column %d read", f.col);
        }
        U = T; U.taint_s[v.id] += 1; U.no_delete[v.id] = !v.no_delete; U.inst[v.id] += 1;
        w = v; w.mask = 0;
        {
            Reads R;
            CHECK(compare(U, w, xl, R) == 0, "no facts %d", k);
            CHECK(R.n[NV_TAINT_S] + R.n[NV_NO_DELETE] + R.n[NV_INST] == 0, "no facts %d read facts", k);
        }
        w = v; w.mask = NV_M_TAINT; U = T; U.no_delete[v.id] = !v.no_delete; CHECK(run(U, w, xl) == 0, "taint alone %d", k);
        // what the host decides before the launch
        {
            w = v; w.mask = NV_M_ABSENT; w.id = 1u << 30;
            Reads R;
            CHECK(compare(T, w, xl, R) == ESC_NV_ABSENT, "preset absent %d", k);
            long reads = 0;
            for (long c : R.n) reads += c;
            CHECK(reads == 0, "preset absent %d read %ld words", k, reads);
            w = v; w.mask = ALL | NV_M_NO_XL; w.xl_dev = 1u << 30;
            Reads Q;
            CHECK(compare(T, w, xl, Q) == ESC_NV_SHAPE, "preset shape %d", k);
            CHECK(Q.n[NV_XL] == 0, "preset shape %d read label words", k);
            w = v; w.mask = NV_M_INST | NV_M_FACTS;
            Reads P;
            CHECK(compare(T, w, xl, P) == ESC_NV_FACTS, "preset facts %d", k);
            CHECK(P.n[NV_TAINT_S] + P.n[NV_NO_DELETE] == 0, "preset facts %d read facts", k);
        }
    }
    {   // slot 9 is absent in the table
        NvNode v = nodes[0];
        v.id = 9;
        CHECK(run(T, v, labels[0]) == ESC_NV_ABSENT, "the absent slot");
    }
    std::printf("%ld checks held, %ld failed; %d nodes, label counts 0 1 2 255\n", held, failed, 4);
    return failed ? 1 : 0;
}
