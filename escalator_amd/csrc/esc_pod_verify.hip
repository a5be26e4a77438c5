// esc_pod_verify.hip — the host runtime's seventh file (esc_ctx.h): esc_pods_verify, the read-only
// compare of a batch of pods with the bytes their slots hold, its kernel, and
// esc_pods_live_ids.
//
// The batch is checked once (batch_shape, as esc_pods_upsert checks it), every pod's place is
// taken from the host mirrors and compared with the device allocations' recorded sizes, and the
// batch goes up in chunks through the context's pinned staging buffer (esc_audit_pods' two
// halves): per pod one PvPod — its fields and its place — and its records and pairs, then one
// launch per chunk with one lane per pod.  The status bytes come back through the same half; a
// half is refilled only after its chunk's bytes are back (an event per half).  Device scratch:
// one chunk buffer per half, the host's class table and the report's words; freed on every way
// out.
#include "esc_ctx.h"

using namespace esc;

namespace {

// One pod of a chunk as the kernel reads it: its own fields and its place by the host mirrors.
struct PvPod {
    uint32_t f, cpu0, pair0;
    int32_t where;             // K: the class index in the host's table; -1: a C slot
    int64_t mem0;
    uint32_t pos;              // K: the position in the class; C: the C-array index
    uint32_t cf;               // C: the slot's flags by the host (its room)
    uint32_t rof, pof;         // its first record / extra pair in the chunk's arrays
    uint32_t ro, po;           // C: the slot's first record / pair in the device's arrays
};
static_assert(sizeof(PvPod) == 48, "staged as 16-B words");

enum PvWord : int { PW_ABSENT = 0, PW_CLASS, PW_VALUE, PW_BIND, PW_FIRST, PW_N };

struct PodVerifyDev {
    const uint32_t* kb;        // replica 0
    const uint32_t *flags, *cpu0, *pair0, *xp;
    const int64_t *mem0, *xc_cpu, *xc_mem;
    const PodClass* hcls;      // the HOST's class table (every place was checked against it)
    int64_t* rep;              // [PW_N]: four sums and a minimum (preset to INT64_MAX)
};

__device__ __forceinline__ int64_t pv_wave_min(int64_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int64_t w = (int64_t)__shfl_xor((unsigned long long)v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}

// One lane per pod of the chunk.  A status the host preset with ABSENT or CLASS is final: such a
// pod has no place to read.  Every other pod's words are gathered from its slot and compared by
// the writers' own walks (kb_pod_same, c_pod_same: esc_kblock.h); the loads of one pod do not
// depend on each other, so a lane has all of them in flight.  Every status byte has one writer.
// The counts and the lowest bad index are reduced per wave (ballots and a shuffle minimum), then
// per block in LDS; one thread adds the block's sums and takes its minimum with one relaxed
// agent-scope 64-bit atomic per report word that has something to add.
__global__ __launch_bounds__(256) void k_pods_verify(PodVerifyDev D, const PvPod* __restrict__ pods,
                                                     const int64_t* __restrict__ xc_cpu, const int64_t* __restrict__ xc_mem,
                                                     const uint32_t* __restrict__ xp, uint8_t* __restrict__ stat, int64_t i0,
                                                     int32_t m) {
    __shared__ uint32_t s_cnt[4][4];
    __shared__ int64_t s_first[4];
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    uint32_t st = 0;
    if (i < m) {
        st = stat[i];
        if (!(st & (ESC_PV_ABSENT | ESC_PV_CLASS))) {
            const PvPod v = pods[i];
            bool same;
            if (v.where >= 0) {
                const PodClass C = D.hcls[v.where];
                const int64_t blk = kb_block(C, C.t0 + (int64_t)(v.pos / TILE));
                same = kb_pod_same(C, D.kb, blk, (int64_t)(v.pos % TILE), v.f, v.cpu0, v.mem0, v.pair0, xc_cpu + v.rof,
                                   xc_mem + v.rof, xp + v.pof);
            } else {
                same = c_pod_same(v.cf, (int64_t)v.pos, (int64_t)v.ro, (int64_t)v.po, v.f, v.cpu0, v.mem0, v.pair0,
                                  xc_cpu + v.rof, xc_mem + v.rof, xp + v.pof, [&](int arr, int64_t at) -> uint64_t {
                                      switch (arr) {
                                      case CA_FLAGS: return (uint64_t)D.flags[at];
                                      case CA_CPU0: return (uint64_t)D.cpu0[at];
                                      case CA_MEM0: return (uint64_t)D.mem0[at];
                                      case CA_PAIR0: return (uint64_t)D.pair0[at];
                                      case CA_XC_CPU: return (uint64_t)D.xc_cpu[at];
                                      case CA_XC_MEM: return (uint64_t)D.xc_mem[at];
                                      default: return (uint64_t)D.xp[at];
                                      }
                                  });
            }
            if (!same) st |= ESC_PV_VALUE;
        }
        stat[i] = (uint8_t)st;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t c0 = (uint32_t)__popcll(__ballot((st & ESC_PV_ABSENT) != 0)), c1 = (uint32_t)__popcll(__ballot((st & ESC_PV_CLASS) != 0));
    const uint32_t c2 = (uint32_t)__popcll(__ballot((st & ESC_PV_VALUE) != 0)), c3 = (uint32_t)__popcll(__ballot((st & ESC_PV_BIND) != 0));
    const int64_t first = pv_wave_min(st ? i0 + i : INT64_MAX);
    if (lane == 0) {
        s_cnt[wave][0] = c0; s_cnt[wave][1] = c1; s_cnt[wave][2] = c2; s_cnt[wave][3] = c3;
        s_first[wave] = first;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t f = INT64_MAX;
        for (int w = 0; w < 4; ++w) f = s_first[w] < f ? s_first[w] : f;
        for (int k = 0; k < 4; ++k) {
            const uint32_t c = s_cnt[0][k] + s_cnt[1][k] + s_cnt[2][k] + s_cnt[3][k];
            if (c) __hip_atomic_fetch_add(D.rep + k, (int64_t)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (f != INT64_MAX) __hip_atomic_fetch_min(D.rep + PW_FIRST, f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// A node index as esc_pods_verify compares it: NONE, an index outside the table and an absent
// slot all mean unbound.
uint32_t pv_node(const esc_ctx* c, uint32_t j) {
    return j == NONE || (int64_t)j >= c->n_nodes || (size_t)j >= c->h_nflags.size() || (c->h_nflags[j] & ESC_NF_ABSENT) ? NONE : j;
}

size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

int32_t verify_one(esc_ctx* c, const int64_t* ids, const esc_pod_soa* p, const uint32_t* pod_node, uint8_t* status_out,
                   esc_pods_verify_report* out) {
    if (!c || !out || !p || p->n_pods < 0 || (p->n_pods > 0 && (!ids || !p->flags || !p->cpu0 || !p->mem0 || !p->pair0)))
        return ESC_E_INVAL;
    if (!c->has_device) return ESC_E_NODEV;
    if (!c->pods_loaded || c->stale || c->pods.empty()) return ESC_E_STATE;
    if (pod_node && !c->placed) return ESC_E_STATE;
    const int64_t n = p->n_pods;
    const esc_pods_verify_report zero = {0, 0, 0, 0, 0, -1};
    if (n == 0) {
        *out = zero;
        return ESC_OK;
    }
    BatchShape sh;
    if (int32_t rc = batch_shape(c, ids, p, sh)) return rc;

    hipSetDevice(c->device);
    hipStream_t st = c->stream;
    if (int32_t rc = pstage_ensure(c)) return rc;
    // The sizes every place is compared with: the host's, cut to the device allocations' own.
    const PodBuf& b0 = c->pods[0];
    const int64_t n_cls = (int64_t)c->h_cls.size(), ct = c->c_tiles, npad = ct * CTILE;
    const int64_t kb_words = dev_bytes_from(b0.kb) / 4;
    const bool c_ok = (int64_t)c->h_cflags.size() == npad && (int64_t)c->h_xc_base.size() == ct + 1 &&
                      (int64_t)c->h_xp_base.size() == ct + 1;
    const int64_t c_slots = c_ok ? std::min({npad, dev_bytes_from(b0.flags) / 4, dev_bytes_from(b0.cpu0) / 4,
                                             dev_bytes_from(b0.pair0) / 4, dev_bytes_from(b0.mem0) / 8}) : 0;
    const int64_t n_xc = c_ok ? std::min<int64_t>({(int64_t)c->h_xc_base[ct], dev_bytes_from(b0.xc_cpu) / 8, dev_bytes_from(b0.xc_mem) / 8}) : 0;
    const int64_t n_xp = c_ok ? std::min<int64_t>((int64_t)c->h_xp_base[ct], dev_bytes_from(b0.xp) / 4) : 0;
    // the classes a K place may name: a holdable class whose tiles lie inside the K blocks
    std::vector<int> cls_id((size_t)n_cls, -1);
    for (int64_t i = 0; i < n_cls; ++i) {
        const PodClass& k = c->h_cls[i];
        if (kb_class_id(k) < 0 || k.wt != k_tile_weight(kb_nrec(k), k.nxp, k.packed) || k.t0 < 0 || k.t1 < k.t0 || k.kb0 < 0 || (k.kb0 & 3)) continue;
        if (k.kb0 + (k.t1 - k.t0) * (int64_t)k.wt * KB_UNIT > kb_words) continue;
        cls_id[i] = kb_class_id(k);
    }
    // The C slots' record and pair offsets, once per tile the batch names (a serial pass: the
    // fill below is threaded and only reads them).
    const int64_t n_ids = (int64_t)c->pod_cls.size();
    std::vector<int32_t> tile_at;
    std::vector<std::array<uint32_t, 2 * CTILE>> tile_off;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t id = ids[i];
        if (id >= n_ids || c->pod_cls[id] != -1) continue;
        const int64_t d = c->pod_pos[id];
        if (d < 0 || d >= c_slots) continue;
        if (tile_at.empty()) tile_at.assign((size_t)ct, -1);
        const int64_t t = d / CTILE;
        if (tile_at[t] >= 0) continue;
        tile_at[t] = (int32_t)tile_off.size();
        tile_off.emplace_back();
        uint32_t ro = c->h_xc_base[t], po = c->h_xp_base[t];
        for (int l = 0; l < CTILE; ++l) {
            tile_off.back()[2 * l] = ro;
            tile_off.back()[2 * l + 1] = po;
            ro += pf_xctr(c->h_cflags[t * CTILE + l]);
            po += pf_xpair(c->h_cflags[t * CTILE + l]);
        }
    }

    PodAuditScratch S;
    Stager G{c, st};
    PodVerifyDev D{};
    D.kb = b0.kb;
    D.flags = b0.flags; D.cpu0 = b0.cpu0; D.pair0 = b0.pair0; D.xp = b0.xp;
    D.mem0 = b0.mem0; D.xc_cpu = b0.xc_cpu; D.xc_mem = b0.xc_mem;
    int64_t* h_rep = reinterpret_cast<int64_t*>(c->h_pstage + 2 * PSTAGE_HALF);
    for (int k = 0; k < PW_N; ++k) h_rep[k] = k == PW_FIRST ? INT64_MAX : 0;
    HIP_TRY(S.get(&D.rep, (size_t)PW_N));
    HIP_TRY(hipMemcpyAsync(D.rep, h_rep, (size_t)PW_N * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(S.get(&G.dev[0], PSTAGE_HALF));
    HIP_TRY(S.get(&G.dev[1], PSTAGE_HALF));
    PodClass* d_hcls = nullptr;
    HIP_TRY(S.get(&d_hcls, (size_t)std::max<int64_t>(n_cls, 1)));
    if ((size_t)n_cls * sizeof(PodClass) > PSTAGE_HALF) return ESC_E_LIMIT;   // (never: at most POD_CLASS_IDS classes)
    if (int32_t rc = G.next()) return rc;
    if (n_cls) std::memcpy(G.host(), c->h_cls.data(), (size_t)n_cls * sizeof(PodClass));
    if (int32_t rc = G.send(d_hcls, 0, (size_t)n_cls * sizeof(PodClass))) return rc;
    if (int32_t rc = G.done()) return rc;
    D.hcls = d_hcls;

    // every pod's records and pairs in the batch end where the next pod's begin
    auto rec_end = [&](int64_t i) { return i + 1 < n ? sh.rof[i + 1] : sh.rof[i] + (int64_t)pf_xctr(p->flags[i]); };
    auto pair_end = [&](int64_t i) { return i + 1 < n ? sh.pof[i + 1] : sh.pof[i] + (int64_t)pf_xpair(p->flags[i]); };
    struct Pending { int64_t i0 = 0, m = 0; size_t at = 0; } pend[2];
    auto harvest = [&](int h) {
        if (status_out && pend[h].m)
            std::memcpy(status_out + pend[h].i0, c->h_pstage + (size_t)h * PSTAGE_HALF + pend[h].at, (size_t)pend[h].m);
        pend[h].m = 0;
    };
    const int T = host_threads();
    for (int64_t i0 = 0; i0 < n;) {
        // the chunk: as many pods as one half holds (pods, records, pairs, status bytes)
        int64_t i1 = i0;
        size_t bytes = 64;
        while (i1 < n) {
            const size_t add = sizeof(PvPod) + 1 + 16 * (size_t)(rec_end(i1) - sh.rof[i1]) + 4 * (size_t)(pair_end(i1) - sh.pof[i1]);
            if (bytes + add > PSTAGE_HALF) break;
            bytes += add;
            ++i1;
        }
        if (i1 == i0) return ESC_E_LIMIT;                    // (never: one pod is at most 8.5 KB)
        const int64_t m = i1 - i0, r0 = sh.rof[i0], nr = rec_end(i1 - 1) - r0, q0 = sh.pof[i0], nq = pair_end(i1 - 1) - q0;
        const size_t xc_at = up16((size_t)m * sizeof(PvPod)), xm_at = xc_at + up16((size_t)nr * 8);
        const size_t xp_at = xm_at + up16((size_t)nr * 8), st_at = xp_at + up16((size_t)nq * 4);
        if (int32_t rc = G.next()) return rc;
        harvest(G.h);
        uint8_t* hb = G.host();
        PvPod* hp = reinterpret_cast<PvPod*>(hb);
        if (nr) {
            std::memcpy(hb + xc_at, p->xc_cpu + r0, (size_t)nr * 8);
            std::memcpy(hb + xm_at, p->xc_mem + r0, (size_t)nr * 8);
        }
        if (nq) std::memcpy(hb + xp_at, p->xp_pair + q0, (size_t)nq * 4);
        par_chunks(m, T, [&](int, int64_t lo, int64_t hi) {
            for (int64_t k = lo; k < hi; ++k) {
                const int64_t i = i0 + k, id = ids[i];
                const uint32_t f = p->flags[i];
                PvPod v{};
                v.f = f; v.cpu0 = p->cpu0[i]; v.pair0 = p->pair0[i]; v.mem0 = p->mem0[i];
                v.rof = (uint32_t)(sh.rof[i] - r0);
                v.pof = (uint32_t)(sh.pof[i] - q0);
                uint8_t s = 0;
                const int32_t ci = id < n_ids ? c->pod_cls[id] : -2;
                if (ci == -2) {
                    s = ESC_PV_ABSENT;
                } else if (ci >= 0) {
                    const int64_t q = c->pod_pos[id];
                    if (ci >= n_cls || cls_id[ci] < 0 || cls_id[ci] != (int)sh.sid[i] || q < 0 ||
                        q >= (c->h_cls[ci].t1 - c->h_cls[ci].t0) * TILE) {
                        s = ESC_PV_CLASS;
                    } else {
                        v.where = ci;
                        v.pos = (uint32_t)q;
                    }
                } else {
                    const int64_t d = c->pod_pos[id];
                    v.where = -1;
                    if (ci != -1 || d < 0 || d >= c_slots || !c_room(c->h_cflags[d], f)) {
                        s = ESC_PV_CLASS;
                    } else {
                        const uint32_t cf = c->h_cflags[d];
                        const std::array<uint32_t, 2 * CTILE>& to = tile_off[(size_t)tile_at[d / CTILE]];
                        v.pos = (uint32_t)d;
                        v.cf = cf;
                        v.ro = to[2 * (d % CTILE)];
                        v.po = to[2 * (d % CTILE) + 1];
                        if ((int64_t)v.ro + pf_xctr(cf) > n_xc || (int64_t)v.po + pf_xpair(cf) > n_xp) s = ESC_PV_CLASS;
                    }
                }
                if (pod_node) {
                    const uint32_t have = ci != -2 && id < (int64_t)c->h_pod_node.size() ? pv_node(c, c->h_pod_node[id]) : NONE;
                    if (have != pv_node(c, pod_node[i])) s |= ESC_PV_BIND;
                }
                hp[k] = v;
                hb[st_at + k] = s;
            }
        });
        if (int32_t rc = G.send(nullptr, 0, (size_t)m * sizeof(PvPod))) return rc;
        if (int32_t rc = G.send(nullptr, xc_at, (size_t)nr * 8)) return rc;
        if (int32_t rc = G.send(nullptr, xm_at, (size_t)nr * 8)) return rc;
        if (int32_t rc = G.send(nullptr, xp_at, (size_t)nq * 4)) return rc;
        if (int32_t rc = G.send(nullptr, st_at, (size_t)m)) return rc;
        uint8_t* d = G.chunk();
        hipLaunchKernelGGL(k_pods_verify, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, D, reinterpret_cast<const PvPod*>(d),
                           reinterpret_cast<const int64_t*>(d + xc_at), reinterpret_cast<const int64_t*>(d + xm_at),
                           reinterpret_cast<const uint32_t*>(d + xp_at), d + st_at, i0, (int32_t)m);
        HIP_TRY(hipGetLastError());
        if (status_out) HIP_TRY(hipMemcpyAsync(hb + st_at, d + st_at, (size_t)m, hipMemcpyDeviceToHost, st));
        pend[G.h].i0 = i0; pend[G.h].m = m; pend[G.h].at = st_at;
        if (int32_t rc = G.done()) return rc;
        i0 = i1;
    }
    HIP_TRY(hipMemcpyAsync(h_rep, D.rep, (size_t)PW_N * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    harvest(0);
    harvest(1);
    *out = zero;
    out->n_checked = n;
    out->n_absent = h_rep[PW_ABSENT];
    out->n_class = h_rep[PW_CLASS];
    out->n_value = h_rep[PW_VALUE];
    out->n_bind = h_rep[PW_BIND];
    out->first_bad = h_rep[PW_FIRST] == INT64_MAX ? -1 : h_rep[PW_FIRST];
    return ESC_OK;
}

}  // namespace

extern "C" {

int32_t esc_pods_verify(esc_ctx* c, const int64_t* ids, const esc_pod_soa* pods, const uint32_t* pod_node, uint8_t* status_out,
                        esc_pods_verify_report* out) {
    if (c && c->multi) return esc::multi_pods_verify(c, ids, pods, pod_node, status_out, out);
    return verify_one(c, ids, pods, pod_node, status_out, out);
}

int32_t esc_pods_live_ids(const esc_ctx* c, int64_t* ids_out, int64_t cap, int64_t* n_out) {
    if (c && c->multi) return esc::multi_pods_live_ids(c, ids_out, cap, n_out);
    if (!c || !n_out || cap < 0 || (cap > 0 && !ids_out)) return ESC_E_INVAL;
    if (!c->has_device) return ESC_E_NODEV;
    if (!c->pods_loaded || (c->stale & STALE_PODS)) return ESC_E_STATE;
    int64_t k = 0;
    for (int64_t id = 0; id < (int64_t)c->pod_cls.size(); ++id) {
        if (c->pod_cls[id] == -2) continue;
        if (k < cap) ids_out[k] = id;
        ++k;
    }
    *n_out = k;
    return k > cap && !(cap == 0 && !ids_out) ? ESC_E_LIMIT : ESC_OK;
}

}  // extern "C"
