// esc_node_verify.hip — the host runtime's eighth file (esc_ctx.h): esc_nodes_verify, the
// read-only compare of a batch of nodes with the resident node table and its per-node facts
// (DESIGN.md §8t), its kernel, and esc_nodes_live_ids.
//
// The batch is checked once on the host (ids, label counts, a bitmap over the table's slots for
// repeated ids), every node's place is taken from the host mirrors and compared with the device
// allocations' recorded sizes, and the batch goes up in chunks through the context's pinned
// staging buffer (esc_audit_pods' two halves): per node one NvNode (esc_node_verify.h) and its
// label words, then one launch per chunk with one lane per node.  The status bytes come back
// through the same half; a half is refilled only after its chunk's bytes are back (an event per
// half).  Device scratch: one chunk buffer per half and the report's words; freed on every way
// out.
#include "esc_ctx.h"
#include "esc_node_verify.h"

using namespace esc;

namespace {

enum NvWord : int { NW_ABSENT = 0, NW_SHAPE, NW_STATUS, NW_FACTS, NW_INST, NW_FIRST, NW_N };

struct NodeVerifyDev {
    const uint32_t *flags, *label0, *xl;
    const int64_t *cpu, *mem, *created, *taint_s, *inst;
    const uint8_t* no_delete;
    int64_t* rep;              // [NW_N]: five sums and a minimum (preset to INT64_MAX)
};

__device__ __forceinline__ int64_t nv_wave_min(int64_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int64_t w = (int64_t)__shfl_xor((unsigned long long)v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}

// One lane per node of the chunk: the lane's record, then nv_compare over the table's columns
// gathered at the record's id (ascending in a resync, so neighbouring lanes share cache lines).
// Every status byte has one writer.  The counts and the lowest bad index are reduced per wave
// (ballots and a shuffle minimum), then per block in LDS; one thread adds the block's sums and
// takes its minimum with one relaxed agent-scope 64-bit atomic per report word that has
// something to add.
__global__ __launch_bounds__(256) void k_nodes_verify(NodeVerifyDev D, const NvNode* __restrict__ nodes,
                                                      const uint32_t* __restrict__ xl, uint8_t* __restrict__ stat, int64_t i0,
                                                      int32_t m) {
    __shared__ uint32_t s_cnt[4][5];
    __shared__ int64_t s_first[4];
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    uint32_t st = 0;
    if (i < m) {
        const NvNode v = nodes[i];
        st = nv_compare(v, xl + v.xl_at, [&](int col, int64_t at) -> uint64_t {
            switch (col) {
            case NV_FLAGS: return (uint64_t)D.flags[at];
            case NV_LABEL0: return (uint64_t)D.label0[at];
            case NV_CPU: return (uint64_t)D.cpu[at];
            case NV_MEM: return (uint64_t)D.mem[at];
            case NV_CREATED: return (uint64_t)D.created[at];
            case NV_TAINT_S: return (uint64_t)D.taint_s[at];
            case NV_NO_DELETE: return (uint64_t)D.no_delete[at];
            case NV_INST: return (uint64_t)D.inst[at];
            default: return (uint64_t)D.xl[at];
            }
        });
        stat[i] = (uint8_t)st;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t cnt[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) cnt[k] = (uint32_t)__popcll(__ballot((st >> k) & 1u));
    const int64_t first = nv_wave_min(st ? i0 + i : INT64_MAX);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k) s_cnt[wave][k] = cnt[k];
        s_first[wave] = first;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t f = INT64_MAX;
        for (int w = 0; w < 4; ++w) f = s_first[w] < f ? s_first[w] : f;
        for (int k = 0; k < 5; ++k) {
            const uint32_t c = s_cnt[0][k] + s_cnt[1][k] + s_cnt[2][k] + s_cnt[3][k];
            if (c) __hip_atomic_fetch_add(D.rep + k, (int64_t)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (f != INT64_MAX) __hip_atomic_fetch_min(D.rep + NW_FIRST, f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
static_assert(ESC_NV_ABSENT == 1 && ESC_NV_SHAPE == 2 && ESC_NV_STATUS == 4 && ESC_NV_FACTS == 8 && ESC_NV_INST == 16,
              "the report words are the status bits in order");

size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

const esc_nodes_verify_report NV_ZERO = {0, 0, 0, 0, 0, 0, -1, 0};

int32_t verify_one(esc_ctx* c, const int64_t* ids, const esc_node_soa* s, const int64_t* taint_s, const uint8_t* no_delete,
                   const int64_t* inst_ns, uint8_t* status_out, esc_nodes_verify_report* out) {
    if (!c || !out || !s || s->n_nodes < 0 ||
        (s->n_nodes > 0 && (!ids || !s->flags || !s->label0 || !s->cpu || !s->mem || !s->created_ns)))
        return ESC_E_INVAL;
    if (s->n_trk != 0 || s->n_xl < 0 || (s->n_xl > 0 && !s->xl_pair)) return ESC_E_INVAL;
    if (!c->has_device) return ESC_E_NODEV;
    if (!c->nodes_loaded || (c->stale & STALE_NODES)) return ESC_E_STATE;
    if ((taint_s || no_delete) && (!c->node_removal || !c->d_taint_s || !c->d_no_delete)) return ESC_E_STATE;
    const int64_t n = s->n_nodes;
    if (n == 0) {
        *out = NV_ZERO;
        return ESC_OK;
    }
    // The batch, once: ids in [0, 2^31), each named once (a bitmap over the table's slots; the
    // few ids past it, which no slot can hold, are sorted), and every node's first label word.
    const int64_t n_cap = c->n_cap;
    std::vector<int64_t> xo((size_t)n + 1);
    {
        std::vector<uint64_t> seen((size_t)(n_cap + 63) / 64, 0);
        std::vector<int64_t> past;
        int64_t sx = 0;
        for (int64_t i = 0; i < n; ++i) {
            const int64_t id = ids[i];
            if (id < 0 || id >= (int64_t)0x7FFFFFFF) return ESC_E_INVAL;
            if (id < n_cap) {
                uint64_t& w = seen[(size_t)(id >> 6)];
                if (w >> (id & 63) & 1) return ESC_E_INVAL;
                w |= uint64_t(1) << (id & 63);
            } else {
                past.push_back(id);
            }
            xo[(size_t)i] = sx;
            sx += nf_xlbl(s->flags[i]);
            if (sx > s->n_xl) return ESC_E_INVAL;
        }
        xo[(size_t)n] = sx;
        std::sort(past.begin(), past.end());
        if (std::adjacent_find(past.begin(), past.end()) != past.end()) return ESC_E_INVAL;
    }

    hipSetDevice(c->device);
    hipStream_t st = c->stream;
    if (int32_t rc = pstage_ensure(c)) return rc;
    // The sizes every place is compared with: the host's, cut to the device allocations' own.
    const NodeBuf& b = c->nodes;
    const bool mirrors = (int64_t)c->h_xl_off.size() >= n_cap;
    const int64_t slots = !mirrors ? 0 : std::min({n_cap, dev_bytes_from(b.flags) / 4, dev_bytes_from(b.label0) / 4,
                                                   dev_bytes_from(b.cpu) / 8, dev_bytes_from(b.mem) / 8,
                                                   dev_bytes_from(b.created) / 8, dev_bytes_from(c->d_inst) / 8});
    const int64_t xl_words = std::min(c->xl_cap, dev_bytes_from(b.d.xl) / 4);
    const bool facts = taint_s || no_delete;
    const int64_t fact_slots = !facts ? 0 : std::min({c->rm_nodes, dev_bytes_from(c->d_taint_s) / 8, dev_bytes_from(c->d_no_delete)});
    const uint8_t want = (uint8_t)((taint_s ? NV_M_TAINT : 0) | (no_delete ? NV_M_NODEL : 0) | (inst_ns ? NV_M_INST : 0));

    PodAuditScratch S;
    Stager G{c, st};
    NodeVerifyDev D{};
    D.flags = b.flags; D.label0 = b.label0; D.xl = b.d.xl;
    D.cpu = b.cpu; D.mem = b.mem; D.created = b.created;
    D.taint_s = c->d_taint_s; D.no_delete = c->d_no_delete; D.inst = c->d_inst;
    int64_t* h_rep = reinterpret_cast<int64_t*>(c->h_pstage + 2 * PSTAGE_HALF);
    for (int k = 0; k < NW_N; ++k) h_rep[k] = k == NW_FIRST ? INT64_MAX : 0;
    HIP_TRY(S.get(&D.rep, (size_t)NW_N));
    HIP_TRY(hipMemcpyAsync(D.rep, h_rep, (size_t)NW_N * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(S.get(&G.dev[0], PSTAGE_HALF));
    HIP_TRY(S.get(&G.dev[1], PSTAGE_HALF));

    struct Pending { int64_t i0 = 0, m = 0; size_t at = 0; } pend[2];
    auto harvest = [&](int h) {
        if (status_out && pend[h].m)
            std::memcpy(status_out + pend[h].i0, c->h_pstage + (size_t)h * PSTAGE_HALF + pend[h].at, (size_t)pend[h].m);
        pend[h].m = 0;
    };
    const int T = host_threads();
    for (int64_t i0 = 0; i0 < n;) {
        // the chunk: as many nodes as one half holds (records, label words, status bytes)
        int64_t i1 = i0;
        size_t bytes = 64;
        while (i1 < n) {
            const size_t add = sizeof(NvNode) + 1 + 4 * (size_t)(xo[(size_t)i1 + 1] - xo[(size_t)i1]);
            if (bytes + add > PSTAGE_HALF) break;
            bytes += add;
            ++i1;
        }
        if (i1 == i0) return ESC_E_LIMIT;                    // (never: one node is at most 1.1 KB)
        const int64_t m = i1 - i0, q0 = xo[(size_t)i0], nq = xo[(size_t)i1] - q0;
        const size_t xl_at = up16((size_t)m * sizeof(NvNode)), st_at = xl_at + up16((size_t)nq * 4);
        if (int32_t rc = G.next()) return rc;
        harvest(G.h);
        uint8_t* hb = G.host();
        NvNode* hp = reinterpret_cast<NvNode*>(hb);
        if (nq) std::memcpy(hb + xl_at, s->xl_pair + q0, (size_t)nq * 4);
        par_chunks(m, T, [&](int, int64_t lo, int64_t hi) {
            for (int64_t k = lo; k < hi; ++k) {
                const int64_t i = i0 + k, id = ids[i];
                const uint32_t nx = nf_xlbl(s->flags[i]);
                NvNode v{};
                v.id = (uint32_t)id;
                v.flags = s->flags[i] & NV_FLAG_BITS;
                v.label0 = s->label0[i];
                v.xl_at = (uint32_t)(xo[(size_t)i] - q0);
                v.cpu = s->cpu[i]; v.mem = s->mem[i]; v.created = s->created_ns[i];
                v.taint_s = taint_s ? taint_s[i] : INT64_MIN;
                v.no_delete = no_delete ? (uint8_t)(no_delete[i] != 0) : 0;
                v.inst = inst_ns ? inst_ns[i] : INT64_MIN;
                v.mask = want;
                if (id >= slots) {
                    v.mask = NV_M_ABSENT;
                } else {
                    v.xl_dev = c->h_xl_off[(size_t)id];
                    if ((int64_t)v.xl_dev + nx > xl_words) v.mask |= NV_M_NO_XL;
                    if (facts && id >= fact_slots) v.mask = (uint8_t)((v.mask & ~(NV_M_TAINT | NV_M_NODEL)) | NV_M_FACTS);
                }
                hp[k] = v;
            }
        });
        if (int32_t rc = G.send(nullptr, 0, (size_t)m * sizeof(NvNode))) return rc;
        if (int32_t rc = G.send(nullptr, xl_at, (size_t)nq * 4)) return rc;
        uint8_t* d = G.chunk();
        hipLaunchKernelGGL(k_nodes_verify, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, D, reinterpret_cast<const NvNode*>(d),
                           reinterpret_cast<const uint32_t*>(d + xl_at), d + st_at, i0, (int32_t)m);
        HIP_TRY(hipGetLastError());
        if (status_out) HIP_TRY(hipMemcpyAsync(hb + st_at, d + st_at, (size_t)m, hipMemcpyDeviceToHost, st));
        pend[G.h].i0 = i0; pend[G.h].m = m; pend[G.h].at = st_at;
        if (int32_t rc = G.done()) return rc;
        i0 = i1;
    }
    HIP_TRY(hipMemcpyAsync(h_rep, D.rep, (size_t)NW_N * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    harvest(0);
    harvest(1);
    *out = NV_ZERO;
    out->n_checked = n;
    out->n_absent = h_rep[NW_ABSENT];
    out->n_shape = h_rep[NW_SHAPE];
    out->n_status = h_rep[NW_STATUS];
    out->n_facts = h_rep[NW_FACTS];
    out->n_inst = h_rep[NW_INST];
    out->first_bad = h_rep[NW_FIRST] == INT64_MAX ? -1 : h_rep[NW_FIRST];
    return ESC_OK;
}

}  // namespace

extern "C" {

int32_t esc_nodes_verify(esc_ctx* c, const int64_t* ids, const esc_node_soa* nodes, const int64_t* taint_s, const uint8_t* no_delete,
                         const int64_t* inst_ns, uint8_t* status_out, esc_nodes_verify_report* out) {
    if (c && c->multi) return esc::multi_nodes_verify(c, ids, nodes, taint_s, no_delete, inst_ns, status_out, out);
    return verify_one(c, ids, nodes, taint_s, no_delete, inst_ns, status_out, out);
}

int32_t esc_nodes_live_ids(const esc_ctx* c, int64_t* ids_out, int64_t cap, int64_t* n_out) {
    if (c && c->multi) return esc_nodes_live_ids(esc::multi_sub(c, 0), ids_out, cap, n_out);
    if (!c || !n_out || cap < 0 || (cap > 0 && !ids_out)) return ESC_E_INVAL;
    if (!c->nodes_loaded) return ESC_E_STATE;
    int64_t k = 0;
    const int64_t n = std::min<int64_t>(c->n_nodes, (int64_t)c->h_nflags.size());
    for (int64_t id = 0; id < n; ++id) {
        if (c->h_nflags[(size_t)id] & ESC_NF_ABSENT) continue;
        if (k < cap) ids_out[k] = id;
        ++k;
    }
    *n_out = k;
    return k > cap && !(cap == 0 && !ids_out) ? ESC_E_LIMIT : ESC_OK;
}

#if ESC_MEASURE
// Measurement library only (not in the header; tests/node_verify_child.py): device i's context of
// a multi-device context, so that a test can send a node event to one device's copy of the table
// alone and show that esc_nodes_verify finds a difference no other device has.
int32_t esc_debug_multi_sub(esc_ctx* c, int32_t i, esc_ctx** out) {
    if (!c || !c->multi || !out || !esc::multi_sub(c, i)) return ESC_E_INVAL;
    *out = esc::multi_sub(c, i);
    return ESC_OK;
}
#endif

}  // extern "C"
