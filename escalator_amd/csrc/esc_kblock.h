// esc_kblock.h — the K section's classes and tile blocks: the one description of
// where a K pod's words lie, shared by the kernels (esc_kernels.h), the host runtime and the
// host-only layout plans (esc_pod_layout.h).  No HIP header: tests/pod_grow_check.cpp builds it
// with the host compiler.
#pragma once

#include <stdint.h>

#include "esc_common.h"

#if defined(__HIPCC__)
#define ESC_KB_HD __host__ __device__ inline
#else
#define ESC_KB_HD inline
#endif

namespace esc {

// A class of homogeneous pod tiles: every pod of the class has the same record
// signature (extra regular containers, init containers, overhead, extra pairs), so every
// field and record k of a tile's 256 pods is one contiguous 256-entry row.
struct PodClass {
    int64_t t0, t1;            // tiles [t0, t1) of the K section
    int64_t kb0, rsv;          // u32-word offset of tile t0's block in the K-block array
    int64_t w0;                // K1 work weight of the tiles before t0
    uint32_t xreg, xinit, ovh, nxp;
    uint32_t kind;             // selects K1's pipeline: plain (xreg + xinit + ovh) * 4 + nxp, packed 16 + nxp,
                               // packed small 20 + nxp (a packed class has no records: kp_fold); inert
                               // K_KIND_INERT + nxp, which no pipeline takes (kb_inert below)
    uint32_t wt;               // size of one tile's block in KB_UNIT words: its 16-B loads per lane, and its
                               // K1 work weight unless the class is inert (kb_k1_wt)
    uint32_t packed;           // the tile format: 0 plain, 1 packed (12 B / pod), 2 packed small (8 B / pod):
                               // kp_*, kp8_* below (an inert class: 2)
    uint32_t pad;
};
// weight of a K tile with R records and NXP extra pairs per pod: its block size in half-KB
// units (128 u32 words; the packed small block's u16 pair rows are half a KB each).  Packed
// tiles hold no records (R is the plain layout's alone).
constexpr uint32_t k_tile_weight(uint32_t R, uint32_t NXP, uint32_t packed = 0) {
    return packed == 2 ? 4 + NXP : (packed ? 2 * (3 + NXP) : 2 * (5 + 4 * R + NXP));
}
constexpr uint32_t k_kind(uint32_t R, uint32_t NXP, uint32_t packed) {
    return packed ? 16 + (packed - 1) * 4 + NXP : R * 4 + NXP;
}
constexpr uint32_t K_TILE_WEIGHT_MIN = 4;   // the lightest tile (packed small, no records or pairs)
constexpr int64_t KB_UNIT = 128;            // u32 words per weight unit
constexpr int POD_SIG_IDS = 128;     // signatures with <= 3 extra records and <= 3 extra pairs
constexpr int POD_CLASS_IDS = 512;   // class id = signature | packed << 7, an inert class's signature | 3 << 7
// Inert classes: packed small tiles of pods no group can ever count (pod_inert,
// esc_pod_layout.h).  Every per-class mechanism treats them as the packed small class of the
// same extra-pair count; they weigh nothing in K1's plan, so no workgroup's share holds one of
// their tiles, and their kind is one no K1 pipeline is instantiated for.
constexpr int POD_INERT_ID0 = 3 * POD_SIG_IDS;
constexpr uint32_t K_KIND_INERT = 24;
ESC_KB_HD bool kb_inert(const PodClass& C) { return C.kind >= K_KIND_INERT; }
// K1 work weight of one tile of the class: its block size, or 0 when K1 never streams it
ESC_KB_HD uint32_t kb_k1_wt(const PodClass& C) { return kb_inert(C) ? 0u : C.wt; }
constexpr int K1_SEGS = 4;           // class runs per K1 workgroup in the work plan (at most)

// K blocks (tile-major K section).  Tile t of a class is ONE contiguous block of wt KB
// (wt = 5 + 4R + NXP): a wave streams a tile as wt consecutive 1-KB wave-loads from one
// address range instead of wt loads from 4 + 2R + 1 separate arrays (the SoA streams cost
// 6.5 % at 100 M pods and 4 % at 12.5 M in scripts/k1_shape_probe.hip, profiles/r02_v8).
// Word offsets inside a block (u32 words; 8-byte rows are 512 words = 256 entries):
//   flags [0, 256)  cpu0 [256, 512)  mem0 [512, 1024)  pair0 [1024, 1280)
//   record k: cpu [1280 + 1024k, +512), mem [+512, +1024)   extra pair k: [1280 + 1024R + 256k, +256)
// 4-byte rows hold pod s at entry s; 8-byte rows at pos64(s) = (s%4/2)*128 + 2(s/4) + s%2,
// so that lane l's 16-B load of either width covers its pods 4l..4l+3 and every wave-load
// reads one contiguous 1 KB.
constexpr int KB_CPU0 = 256, KB_MEM0 = 512, KB_PAIR0 = 1024, KB_REC = 1280;
ESC_KB_HD int64_t kb_pos64(int64_t s) { return ((s & 3) >> 1) * 128 + 2 * (s >> 2) + (s & 1); }
// first word of tile t's block (t a tile of class C)
ESC_KB_HD int64_t kb_block(const PodClass& C, int64_t t) { return C.kb0 + (t - C.t0) * (int64_t)C.wt * KB_UNIT; }
ESC_KB_HD uint32_t kb_nrec(const PodClass& C) { return C.xreg + C.xinit + C.ovh; }
// 8-byte element index (into the array viewed as int64) of record k's cpu (mem: +256) of pod s
ESC_KB_HD int64_t kb_rec64(int64_t blk, uint32_t k, int64_t s) {
    return (blk + KB_REC + 1024 * (int64_t)k) / 2 + kb_pos64(s);
}
// Packed K blocks (PodClass::packed): the same tile-major block with the pod's effective
// request — its container records folded into one (cpu, mem) on the host, kp_fold below —
// packed into 12 B per pod instead of 20 + 16 per record:
//   word  [0, 256)            pair0 (bits 0..27, KP_PAIR_NONE = no pair) | the pod's own flag
//                             bits DAEMONSET, STATIC, HAS_SEL, AFF_BLOCK at bits 28..31 (every
//                             other flag bit is the class signature's)
//   u64   [256, 768)          cpu | mem << 20 at kb_pos64(s): the effective request
//   u32   extra pair k        [768 + 256k, +256), as in the plain layout
// A pod is packed when cpu0 and every record cpu are in [0, 2^20 - 1), mem0 and every record
// mem in [0, 2^44 - 1) (an init record's key may instead be absent), pair0 < 2^28 - 1
// (kp_fits) and its effective request is in the same ranges — the range of K1's LDS fast
// path.  A packed class has no records (signature (0, 0, 0, nxp)); every other K pod keeps
// its records in the plain layout of its own signature.
constexpr int KP_CM0 = 256, KP_XP = 768;
constexpr uint32_t KP_FLAG_SHIFT = 28;
constexpr uint32_t KP_PAIR_NONE = (1u << KP_FLAG_SHIFT) - 1;
constexpr uint32_t KP_POD_FLAGS = ESC_PF_DAEMONSET | ESC_PF_STATIC | ESC_PF_HAS_SEL | ESC_PF_AFF_BLOCK;
constexpr int KP_CPU_BITS = 20;
// the fields' masks and the exclusive bounds of the packed ranges (the names are from the
// all-ones sentinel a packed init record's absent key had; no record is stored now)
constexpr uint64_t KP_CPU_ABSENT = (uint64_t(1) << KP_CPU_BITS) - 1;
constexpr uint64_t KP_MEM_ABSENT = (uint64_t(1) << 44) - 1;
// Packed small K blocks (PodClass::packed == 2): a packed pod whose effective request also
// has cpu < 2^14 m and mem < 2^34 B (16 cores, 16 GiB: most pods), in a context with fewer
// than 2^14 - 1 group pairs, is ONE u64 (8 B):
//   u64   [0, 512)            cpu | mem << 14 | pair0 << 48 (14 bits; KP8_PAIR_NONE: no
//                             pair, or one no group selects) | daemonset << 62 |
//                             blocks-default << 63 (static, has-selector or affinity: the
//                             default filter's other conditions, node_group.go:263-273)
//                             A daemonset pod (and a free slot) is stored with no pairs and
//                             blocks-default set, so K1 adds it nowhere without a test.
//   u16   extra pair k        [512 + 128k, +128) words: pod s at u16 index s (0xFFFF: none,
//                             or one no group selects)
constexpr int KP8_XP = 512;
constexpr int KP8_CPU_BITS = 14, KP8_MEM_BITS = 34, KP8_PAIR_SHIFT = 48;
constexpr uint64_t KP8_CPU_MASK = (uint64_t(1) << KP8_CPU_BITS) - 1;
constexpr uint64_t KP8_MEM_MASK = (uint64_t(1) << KP8_MEM_BITS) - 1;
constexpr uint32_t KP8_PAIR_NONE = (1u << 14) - 1;
constexpr uint64_t KP8_DS = uint64_t(1) << 62, KP8_NODEF = uint64_t(1) << 63;
ESC_KB_HD bool kp8_fits(int64_t cpu, int64_t mem) {
    return cpu >= 0 && (uint64_t)cpu <= KP8_CPU_MASK && mem >= 0 && (uint64_t)mem <= KP8_MEM_MASK;
}
ESC_KB_HD uint64_t kp8_word(uint32_t f, uint32_t cpu0, int64_t mem0, uint32_t pair0) {
    const bool ds = (f & ESC_PF_DAEMONSET) != 0;
    const uint64_t q = pair0 < KP8_PAIR_NONE && !ds ? pair0 : KP8_PAIR_NONE;
    return (uint64_t)cpu0 | (uint64_t)mem0 << KP8_CPU_BITS | q << KP8_PAIR_SHIFT | (ds ? KP8_DS | KP8_NODEF : 0) |
           ((f & (ESC_PF_STATIC | ESC_PF_HAS_SEL | ESC_PF_AFF_BLOCK)) ? KP8_NODEF : 0);
}
// extra pair k of pod s: its u32-word index (plain and packed blocks) or, in a packed small
// block, its u16 index (kb_pair reads either)
constexpr uint32_t KP8_XP_NONE = 0xFFFFu;
ESC_KB_HD int64_t kb_xp(const PodClass& C, int64_t blk, uint32_t k, int64_t s) {
    if (C.packed == 2) return (blk + KP8_XP + 128 * (int64_t)k) * 2 + s;
    if (C.packed) return blk + KP_XP + 256 * (int64_t)k + s;
    return blk + KB_REC + 1024 * (int64_t)kb_nrec(C) + 256 * (int64_t)k + s;
}
// the first u32 word of the extra-pair rows of the block at blk, and their size in words
ESC_KB_HD int64_t kb_xp_row0(const PodClass& C, int64_t blk) {
    if (C.packed == 2) return blk + KP8_XP;
    return kb_xp(C, blk, 0, 0);
}
ESC_KB_HD int64_t kb_xp_words(const PodClass& C) { return (int64_t)C.nxp * (C.packed == 2 ? 128 : 256); }
ESC_KB_HD uint32_t kb_pair(const PodClass& C, const uint32_t* kb, int64_t blk, uint32_t k, int64_t s) {
    if (C.packed == 2) {
        const uint32_t q = reinterpret_cast<const uint16_t*>(kb)[kb_xp(C, blk, k, s)];
        return q == KP8_XP_NONE ? NONE : q;
    }
    return kb[kb_xp(C, blk, k, s)];
}
// A freed / padding slot: daemonset-flagged, no pair (put as in kb_write_pod below).
// put(width, index, value): width 8 = int64 element index, 4 = u32 word, 2 = u16 element.
template <class Put>
ESC_KB_HD void kb_write_free(const PodClass& C, int64_t blk, int64_t sl, Put&& put) {
    if (C.packed == 2) {
        put(8, blk / 2 + kb_pos64(sl), KP8_DS | KP8_NODEF | (uint64_t)KP8_PAIR_NONE << KP8_PAIR_SHIFT);
        for (uint32_t k = 0; k < C.nxp; ++k) put(2, kb_xp(C, blk, k, sl), KP8_XP_NONE);   // no pairs (see kp8_word)
    } else {
        put(4, blk + sl, C.packed ? (ESC_PF_DAEMONSET << KP_FLAG_SHIFT) | KP_PAIR_NONE : ESC_PF_DAEMONSET);
    }
}
// Is a (cpu, mem) pair inside the packed ranges?  (init: an init container's record, whose
// absent key, INT64_MIN, is allowed.)
ESC_KB_HD bool kp_val_fits(int64_t cpu, int64_t mem, bool init) {
    const bool c = (cpu >= 0 && (uint64_t)cpu < KP_CPU_ABSENT) || (init && cpu == INT64_MIN);
    const bool m = (mem >= 0 && (uint64_t)mem < KP_MEM_ABSENT) || (init && mem == INT64_MIN);
    return c && m;
}
// packed 8-byte value of an effective request inside the packed ranges
ESC_KB_HD uint64_t kp_val(int64_t cpu, int64_t mem) { return (uint64_t)cpu | ((uint64_t)mem << KP_CPU_BITS); }
ESC_KB_HD int64_t kp_cpu(uint64_t v) { return (int64_t)(v & KP_CPU_ABSENT); }
ESC_KB_HD int64_t kp_mem(uint64_t v) { return (int64_t)(v >> KP_CPU_BITS); }
ESC_KB_HD uint32_t kp_word(uint32_t flags, uint32_t pair0) {
    return ((flags & KP_POD_FLAGS) << KP_FLAG_SHIFT) | (pair0 == NONE ? KP_PAIR_NONE : pair0);
}
ESC_KB_HD uint32_t kp_pair0(uint32_t w) {
    const uint32_t q = w & KP_PAIR_NONE;
    return q == KP_PAIR_NONE ? NONE : q;
}
// full ESC_PF_* flags of a packed pod as stored: its own bits + the class signature (which
// has no records: the pod reads back as one container with its effective request)
ESC_KB_HD uint32_t kp_flags(const PodClass& C, uint32_t w) {
    return (w >> KP_FLAG_SHIFT) | (C.nxp << ESC_PF_XPAIR_SHIFT);
}
// Are the pod's own values all inside the packed ranges?  (xc_cpu / xc_mem: its extra
// records, regular, then init, then overhead, as esc_pod_soa lists them.)
ESC_KB_HD bool kp_fits(uint32_t f, uint32_t cpu0, int64_t mem0, uint32_t pair0, const int64_t* xc_cpu,
                                        const int64_t* xc_mem) {
    if (!(pair0 == NONE || pair0 < KP_PAIR_NONE) || !kp_val_fits((int64_t)cpu0, mem0, false)) return false;
    const uint32_t nreg = pf_xreg(f), ninit = pf_xinit(f), n = pf_xctr(f);
    for (uint32_t k = 0; k < n; ++k)
        if (!kp_val_fits(xc_cpu[k], xc_mem[k], k >= nreg && k < nreg + ninit)) return false;
    return true;
}
// The fold: a K-section pod whose values pass kp_fits has its effective request
// (pod_request, esc_common.h) computed once on the host — its container requests are fixed for
// the pod's life; a change arrives as an upsert, which rewrites the slot.  Every value is
// then in [0, 2^44) and there are at most 4 of them, so the request is in [0, 2^47): nothing
// wraps.  Returns the layout the pod takes, with the request in cpu / mem: 2 the packed small
// block (in a context of n_gp < KP8_PAIR_NONE group pairs), 1 the packed block, 0 the plain
// block of its own signature, records kept (kp_fits failed, or the request is outside the
// packed ranges; cpu / mem are then not meaningful).
ESC_KB_HD uint32_t kp_fold(uint32_t f, uint32_t cpu0, int64_t mem0, uint32_t pair0, const int64_t* xc_cpu,
                                            const int64_t* xc_mem, uint32_t n_gp, int64_t& cpu, int64_t& mem) {
    cpu = (int64_t)cpu0;
    mem = mem0;
    if (!kp_fits(f, cpu0, mem0, pair0, xc_cpu, xc_mem)) return 0;
    uint32_t o = 0;
    pod_request(f, cpu0, mem0, xc_cpu, xc_mem, o, cpu, mem);
    if (n_gp < KP8_PAIR_NONE && kp8_fits(cpu, mem)) return 2;
    return kp_val_fits(cpu, mem, false) ? 1 : 0;
}
// Can no group ever count the pod, whatever the groups' state?  A daemonset pod is excluded
// by both filters (node_group.go:221, :259); a pod that blocks the default filter (static, a
// selector, a blocking affinity) joins only the slots of its pairs, so it is inert when none
// of them is a group pair (< n_gp).  A pod that does not block the default filter joins the
// default slot and is never inert.  (escalator_amd/layout.py inert_mask restates it.)  Host and
// device: esc_pods_compact classifies the pods it re-homes on the device.
ESC_KB_HD bool pod_inert(uint32_t f, uint32_t pair0, const uint32_t* xp, uint32_t n_gp) {
    if (f & ESC_PF_DAEMONSET) return true;
    if (!(f & (ESC_PF_STATIC | ESC_PF_HAS_SEL | ESC_PF_AFF_BLOCK))) return false;
    if (pair0 < n_gp) return false;
    for (uint32_t k = 0, np = pf_xpair(f); k < np; ++k)
        if (xp[k] < n_gp) return false;
    return true;
}

// K class of a pod, the one place that decides it: -1 for the C section (more
// than 3 extra container records or more than 3 extra pairs); else the fold (kp_fold) either
// packs the pod's effective request — class id = its pair count np | packed << 7, packed 2
// for the packed small block and 1 for the packed block, a signature without records — or
// leaves the pod its records in the plain class of its own signature.  xc_cpu / xc_mem: the
// pod's own records (null when it has none).  xp: its extra pairs (null when it has none).  A
// pod of the packed small block that is inert (pod_inert) takes the inert class of its pair
// count instead, id np | 3 << 7: the same tile, kept out of K1's stream.
ESC_KB_HD int pod_class_id(uint32_t f, uint32_t cpu0, int64_t mem0, uint32_t pair0, const int64_t* xc_cpu,
                        const int64_t* xc_mem, const uint32_t* xp, uint32_t n_gp) {
    const uint32_t xr = pf_xreg(f), xi = pf_xinit(f), ov = (f & ESC_PF_HAS_OVH) ? 1u : 0u, np = pf_xpair(f);
    if (xr + xi + ov > 3 || np > 3) return -1;
    int64_t cpu, mem;
    const uint32_t packed = kp_fold(f, cpu0, mem0, pair0, xc_cpu, xc_mem, n_gp, cpu, mem);
    if (packed == 2 && pod_inert(f, pair0, xp, n_gp)) return (int)(np | POD_INERT_ID0);
    if (packed) return (int)(np | packed * POD_SIG_IDS);
    return (int)(((xr * 4 + xi) * 2 + ov) * 4 + np);
}

// The head of K pod s of the block at word blk, any layout: ESC_PF_* flags (the class
// signature's counts included; a packed small pod's static / has-selector / affinity bits
// read back as ESC_PF_HAS_SEL), pair0 (NONE: none, or no group's in a small block) and the
// first container's cpu / mem (a packed pod's: its effective request); kb_rec: record k's
// cpu / mem of a plain pod (an absent init key INT64_MIN; packed classes have no records).
struct KHead {
    uint32_t flags, pair0;
    int64_t cpu0, mem0;
};
ESC_KB_HD KHead kb_head(const PodClass& C, const uint32_t* kb, int64_t blk, int64_t s) {
    KHead h;
    const int64_t* kb64 = reinterpret_cast<const int64_t*>(kb);
    if (C.packed == 2) {
        const uint64_t w = (uint64_t)kb64[blk / 2 + kb_pos64(s)];
        h.flags = kp_flags(C, 0) | ((w & KP8_DS) ? ESC_PF_DAEMONSET : 0u) | ((w & KP8_NODEF) ? ESC_PF_HAS_SEL : 0u);
        const uint32_t q = (uint32_t)(w >> KP8_PAIR_SHIFT) & KP8_PAIR_NONE;
        h.pair0 = q == KP8_PAIR_NONE ? NONE : q;
        h.cpu0 = (int64_t)(w & KP8_CPU_MASK);
        h.mem0 = (int64_t)((w >> KP8_CPU_BITS) & KP8_MEM_MASK);
    } else if (C.packed) {
        const uint32_t w0 = kb[blk + s];
        const uint64_t v = (uint64_t)kb64[(blk + KP_CM0) / 2 + kb_pos64(s)];
        h.flags = kp_flags(C, w0);
        h.pair0 = kp_pair0(w0);
        h.cpu0 = kp_cpu(v);
        h.mem0 = kp_mem(v);
    } else {
        h.flags = kb[blk + s];
        h.pair0 = kb[blk + KB_PAIR0 + s];
        h.cpu0 = kb[blk + KB_CPU0 + s];
        h.mem0 = kb64[(blk + KB_MEM0) / 2 + kb_pos64(s)];
    }
    return h;
}
ESC_KB_HD void kb_rec(const PodClass& C, const uint32_t* kb, int64_t blk, uint32_t k, int64_t s,
                                       int64_t& cpu, int64_t& mem) {
    const int64_t* kb64 = reinterpret_cast<const int64_t*>(kb);
    const int64_t o = kb_rec64(blk, k, s);
    cpu = kb64[o];
    mem = kb64[o + 256];
}

// Every word a K-class pod occupies in its tile (load and in-place upserts): put(width,
// index, value) as for kb_write_free.  xc_cpu / xc_mem are the pod's own records (by its
// flags f); a packed class stores their fold (the class kp_fold chose for the pod).
template <class Put>
ESC_KB_HD void kb_write_pod(const PodClass& C, int64_t blk, int64_t sl, uint32_t f, uint32_t cpu0,
                                             int64_t mem0, uint32_t pair0, const int64_t* xc_cpu,
                                             const int64_t* xc_mem, const uint32_t* xp, Put&& put) {
    const uint32_t R = kb_nrec(C);
    if (C.packed) {
        int64_t cpu, mem;
        uint32_t o = 0;
        pod_request(f, cpu0, mem0, xc_cpu, xc_mem, o, cpu, mem);
        if (C.packed == 2) {
            put(8, blk / 2 + kb_pos64(sl), kp8_word(f, (uint32_t)cpu, mem, pair0));
        } else {
            put(4, blk + sl, kp_word(f, pair0));
            put(8, (blk + KP_CM0) / 2 + kb_pos64(sl), kp_val(cpu, mem));
        }
    } else {
        put(4, blk + sl, f);
        put(4, blk + KB_CPU0 + sl, cpu0);
        put(8, (blk + KB_MEM0) / 2 + kb_pos64(sl), (uint64_t)mem0);
        put(4, blk + KB_PAIR0 + sl, pair0);
        for (uint32_t k = 0; k < R; ++k) {
            const int64_t o = kb_rec64(blk, k, sl);
            put(8, o, (uint64_t)xc_cpu[k]);
            put(8, o + 256, (uint64_t)xc_mem[k]);
        }
    }
    if (C.packed == 2) {                       // u16 pairs; a daemonset pod has none (kp8_word)
        for (uint32_t k = 0; k < C.nxp; ++k)
            put(2, kb_xp(C, blk, k, sl), (f & ESC_PF_DAEMONSET) || xp[k] >= KP8_XP_NONE ? KP8_XP_NONE : xp[k]);
    } else {
        for (uint32_t k = 0; k < C.nxp; ++k) put(4, kb_xp(C, blk, k, sl), xp[k]);
    }
}

// esc_pods_grow: one class of the re-cut K section as k_kb_regrow reads it.
// New tile t of [t0, t1) is block j = t - t0 of the class, at word new_kb0 + j * wt * KB_UNIT of
// the new array; its source is block j of the old array (from word old_kb0) when j < old_tiles,
// else the class's free tile at word tmpl of the staged templates.
struct KbRegrowCls {
    int64_t t0, t1;
    int64_t old_kb0, old_tiles;
    int64_t new_kb0, tmpl;
    uint32_t wt, pad;
};
static_assert(sizeof(KbRegrowCls) == 56, "k_kb_regrow reads the staged table as 8-B words");

// esc_pods_compact: one class of the re-cut K section as k_pc_move reads it.  The
// class's live pods are elements [start, start + live) of the sorted (class, bucket, source)
// elements and take positions [0, live) of its tiles; a position past them copies the same slot
// of the class's free tile at word tmpl of the staged templates (-1: the class has no tile).
struct PcCls {
    int64_t start, live;
    int64_t tmpl, pad;
};
// The pod of a K-holdable C slot as its own shape (its records and pairs first of each kind in
// the slot's room, the rest neutral): what pod_class_id and kb_write_pod take.
struct CPod {
    uint32_t f, cpu0, pair0, ok;       // ok: at most 3 own records and 3 own pairs
    int64_t mem0;
};
struct CPodRec {                       // its records (regular, init, overhead side by side) and pairs; one per
    int64_t xc[3], xm[3];              // lane in LDS, so that the shared rule's loops index memory, not registers
    uint32_t xp[3], pad;
};
static_assert(sizeof(CPodRec) == 64, "one LDS row per lane");
constexpr uint32_t K_TILE_WEIGHT_MAX = k_tile_weight(3, 3);   // the heaviest tile (plain, 3 records, 3 pairs)

// esc_audit_pods.  The class id (pod_class_id's numbering) of the pods a class
// holds, from the class's own fields; -1 for fields no class can have.
ESC_KB_HD int kb_class_id(const PodClass& C) {
    if (C.packed > 2 || C.nxp > 3 || C.xreg > 3 || C.xinit > 3 || C.ovh > 1 || kb_nrec(C) > 3) return -1;
    if (C.packed && kb_nrec(C)) return -1;
    if (kb_inert(C)) return C.packed == 2 ? (int)(C.nxp | POD_INERT_ID0) : -1;
    if (C.packed) return (int)(C.nxp | C.packed * POD_SIG_IDS);
    return (int)(((C.xreg * 4 + C.xinit) * 2 + C.ovh) * 4 + C.nxp);
}
// The class id the stored words of K pod s of the block at word blk re-derive to: the words
// read back as every reader reads them (kb_head, kb_rec, kb_pair) and classified by the one rule
// (pod_class_id) in a context of n_gp group pairs.  For a pod that kb_write_pod wrote into a
// class the rule chose this is that class's id (kb_class_id): a packed pod reads back as one
// container with its folded request, which folds to itself; a plain pod reads back whole.  A
// slot of a free tile (kb_write_free over zeroes) re-derives to the inert class of the tile's
// pair count where the context has packed small classes (n_gp < KP8_PAIR_NONE), else to the
// packed class of that count: never to a plain class, and to a packed or packed small class
// only as said.  Where it re-derives to its own class (an inert class; a packed class without
// packed small ones) a free slot and a live daemonset pod of zero request are the same words,
// and a freed plain slot keeps its pod's other words, so the free lists, not this function,
// say which slot is free.
// r: one CPodRec of scratch (a lane's LDS row on the
// device, so that the rule's loops index memory).  The class must be a holdable one
// (kb_class_id(C) >= 0) and the block inside the array: the caller checks both.
ESC_KB_HD int kb_pod_class(const PodClass& C, const uint32_t* kb, int64_t blk, int64_t s, uint32_t n_gp, CPodRec& r) {
    const KHead h = kb_head(C, kb, blk, s);
    const uint32_t R = C.packed ? 0u : kb_nrec(C);
    for (uint32_t k = 0; k < 3; ++k) {
        r.xc[k] = r.xm[k] = 0;
        if (k < R) kb_rec(C, kb, blk, k, s, r.xc[k], r.xm[k]);
        r.xp[k] = k < C.nxp ? kb_pair(C, kb, blk, k, s) : NONE;
    }
    // a plain pod's stored flags carry its own counts; more than the class's rows hold is read
    // as a class no tile has, never as a longer record list
    if (!C.packed && (pf_xctr(h.flags) != R || pf_xpair(h.flags) != C.nxp)) return -1;
    return pod_class_id(h.flags, (uint32_t)h.cpu0, h.mem0, h.pair0, r.xc, r.xm, r.xp, n_gp);
}

// Every word a pod occupies in a C slot (esc_pods_upsert into a C slot): put(array, index,
// value) with array one of CArr.  cf: the slot's flags, whose counts are its room; d: its
// C-array index; ro / po: its first record / pair in the record and pair arrays.  The slot keeps
// its counts and takes the pod's own bits; the pod's records and pairs come first of each kind in
// the room and the rest is neutral (0 for regular and overhead records, INT64_MIN for init keys,
// NONE for pairs).  The room must hold the pod (c_room, esc_pod_layout.h).
enum CArr : int { CA_FLAGS = 0, CA_CPU0, CA_MEM0, CA_PAIR0, CA_XC_CPU, CA_XC_MEM, CA_XP };
template <class Put>
ESC_KB_HD void c_write_pod(uint32_t cf, int64_t d, int64_t ro, int64_t po, uint32_t f, uint32_t cpu0, int64_t mem0,
                           uint32_t pair0, const int64_t* xc_cpu, const int64_t* xc_mem, const uint32_t* xp, Put&& put) {
    put(CA_FLAGS, d, (uint64_t)((cf & ~KP_POD_FLAGS) | (f & KP_POD_FLAGS)));
    put(CA_CPU0, d, (uint64_t)cpu0);
    put(CA_MEM0, d, (uint64_t)mem0);
    put(CA_PAIR0, d, (uint64_t)pair0);
    const uint32_t xr = pf_xreg(f), xi = pf_xinit(f), ov = (f & ESC_PF_HAS_OVH) ? 1u : 0u;
    int64_t o = ro;
    for (uint32_t k = 0; k < pf_xreg(cf); ++k, ++o) {
        put(CA_XC_CPU, o, (uint64_t)(k < xr ? xc_cpu[k] : 0));
        put(CA_XC_MEM, o, (uint64_t)(k < xr ? xc_mem[k] : 0));
    }
    for (uint32_t k = 0; k < pf_xinit(cf); ++k, ++o) {
        put(CA_XC_CPU, o, (uint64_t)(k < xi ? xc_cpu[xr + k] : INT64_MIN));
        put(CA_XC_MEM, o, (uint64_t)(k < xi ? xc_mem[xr + k] : INT64_MIN));
    }
    if (cf & ESC_PF_HAS_OVH) {
        put(CA_XC_CPU, o, (uint64_t)(ov ? xc_cpu[xr + xi] : 0));
        put(CA_XC_MEM, o, (uint64_t)(ov ? xc_mem[xr + xi] : 0));
    }
    const uint32_t nx = pf_xpair(f);
    for (uint32_t k = 0; k < pf_xpair(cf); ++k) put(CA_XP, po + k, (uint64_t)(k < nx ? xp[k] : NONE));
}

// esc_pods_verify.  Does K slot sl of the block at word blk of class C hold exactly
// what kb_write_pod would write for this pod?  The writer's own walk with a put that reads and
// compares: get(width, index) returns the stored word, widths and indices as put's.  The
// differences are or-ed, not tested one by one, so that a lane's loads are all in flight before
// the first is needed.  The class must be the pod's (pod_class_id == kb_class_id(C)): its rows
// are then as many as the pod's records and pairs.
template <class Get>
ESC_KB_HD bool kb_pod_same(const PodClass& C, int64_t blk, int64_t sl, uint32_t f, uint32_t cpu0, int64_t mem0,
                           uint32_t pair0, const int64_t* xc_cpu, const int64_t* xc_mem, const uint32_t* xp, Get&& get) {
    uint64_t diff = 0;
    kb_write_pod(C, blk, sl, f, cpu0, mem0, pair0, xc_cpu, xc_mem, xp, [&](int width, int64_t at, uint64_t v) {
        const uint64_t m = width == 8 ? ~uint64_t(0) : (width == 4 ? uint64_t(0xFFFFFFFFu) : uint64_t(0xFFFFu));
        diff |= ((uint64_t)get(width, at) ^ v) & m;
    });
    return diff == 0;
}
// The same over K blocks in memory.
ESC_KB_HD bool kb_pod_same(const PodClass& C, const uint32_t* kb, int64_t blk, int64_t sl, uint32_t f, uint32_t cpu0,
                           int64_t mem0, uint32_t pair0, const int64_t* xc_cpu, const int64_t* xc_mem,
                           const uint32_t* xp) {
    return kb_pod_same(C, blk, sl, f, cpu0, mem0, pair0, xc_cpu, xc_mem, xp, [&](int width, int64_t at) -> uint64_t {
        if (width == 8) return (uint64_t)reinterpret_cast<const int64_t*>(kb)[at];
        if (width == 4) return (uint64_t)kb[at];
        return (uint64_t)reinterpret_cast<const uint16_t*>(kb)[at];
    });
}
// Does C slot d (flags cf, records from ro, pairs from po) hold exactly what c_write_pod would
// write for this pod?  get(array, index) returns the stored word of a CArr array.
template <class Get>
ESC_KB_HD bool c_pod_same(uint32_t cf, int64_t d, int64_t ro, int64_t po, uint32_t f, uint32_t cpu0, int64_t mem0,
                          uint32_t pair0, const int64_t* xc_cpu, const int64_t* xc_mem, const uint32_t* xp, Get&& get) {
    uint64_t diff = 0;
    c_write_pod(cf, d, ro, po, f, cpu0, mem0, pair0, xc_cpu, xc_mem, xp,
                [&](int arr, int64_t at, uint64_t v) { diff |= (uint64_t)get(arr, at) ^ v; });
    return diff == 0;
}

}  // namespace esc
