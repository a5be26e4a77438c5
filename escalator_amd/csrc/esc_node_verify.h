// esc_node_verify.h — the compare rule of esc_nodes_verify in one place: one
// node of the caller's batch, as the host stages it, against the words the resident node table
// holds for its id.  k_nodes_verify (esc_node_verify.hip) runs nv_compare on the device and
// tests/node_verify_check.cpp runs the same function with the host compiler.  No HIP header.
#pragma once

#include <stdint.h>

#include "esc_common.h"

#if defined(__HIPCC__)
#define ESC_NV_HD __host__ __device__ inline
#else
#define ESC_NV_HD inline
#endif

namespace esc {

// One node of a chunk as the kernel reads it: its own fields and, from the host mirrors, where
// its extra labels lie.  Nothing here was read from the device.
struct NvNode {
    uint32_t id;               // the table slot (< the columns' slots unless NV_M_ABSENT)
    uint32_t flags;            // ESC_NF_UNSCHED | ESC_NF_TAINTED | the extra-label count: nothing else
    uint32_t label0;
    uint32_t xl_at;            // its first extra label among the chunk's label words
    int64_t cpu, mem;
    int64_t created, taint_s;
    int64_t inst;
    uint32_t xl_dev;           // its first extra label in the device's words, by the host's h_xl_off
    uint8_t no_delete;
    uint8_t mask;              // NV_M_*
    uint16_t pad;
};
static_assert(sizeof(NvNode) == 64, "staged as 16-B words");

// NvNode::mask: which facts are compared, and what the host decided before the launch
constexpr uint8_t NV_M_TAINT = 1, NV_M_NODEL = 2, NV_M_INST = 4;
constexpr uint8_t NV_M_ABSENT = 8;     // the id lies outside the table's columns: nothing is read
constexpr uint8_t NV_M_NO_XL = 16;     // xl_dev + the count leaves the device's label words: SHAPE, no label word read
constexpr uint8_t NV_M_FACTS = 32;     // the id lies outside the facts' arrays: FACTS, neither fact read

// The table's columns as the reader names them.
enum NvCol : int { NV_FLAGS = 0, NV_LABEL0, NV_CPU, NV_MEM, NV_CREATED, NV_TAINT_S, NV_NO_DELETE, NV_INST, NV_XL };

constexpr uint32_t NV_FLAG_BITS = ESC_NF_UNSCHED | ESC_NF_TAINTED | (ESC_PF_CNT_MASK << ESC_NF_XLBL_SHIFT);

// The status byte (ESC_NV_*) of node v, whose extra labels are xl[0 .. count).  rd(column, index)
// returns the table's word as uint64.  Every index is the record's: the id for the eight
// columns, xl_dev + k for label word k — no word read here is used as an index or a bound.  The
// eight column reads do not depend on each other or on a compare, so a lane has them all in
// flight; the label words are read only when the device's count equals the batch's, and the loop
// runs to the batch's count.
template <class R>
ESC_NV_HD uint32_t nv_compare(const NvNode& v, const uint32_t* xl, R&& rd) {
    if (v.mask & NV_M_ABSENT) return ESC_NV_ABSENT;
    const int64_t id = (int64_t)v.id;
    const uint32_t f = (uint32_t)rd(NV_FLAGS, id), l0 = (uint32_t)rd(NV_LABEL0, id);
    const int64_t cpu = (int64_t)rd(NV_CPU, id), mem = (int64_t)rd(NV_MEM, id), created = (int64_t)rd(NV_CREATED, id);
    const int64_t taint_s = (v.mask & NV_M_TAINT) ? (int64_t)rd(NV_TAINT_S, id) : v.taint_s;
    const uint32_t no_del = (v.mask & NV_M_NODEL) ? (uint32_t)rd(NV_NO_DELETE, id) : (uint32_t)v.no_delete;
    const int64_t inst = (v.mask & NV_M_INST) ? (int64_t)rd(NV_INST, id) : v.inst;
    if (f & ESC_NF_ABSENT) return ESC_NV_ABSENT;
    const uint32_t nx = nf_xlbl(v.flags);
    uint64_t shape = (uint64_t)(l0 ^ v.label0) | (uint64_t)(nf_xlbl(f) ^ nx) | (uint64_t)(created ^ v.created) |
                     (uint64_t)(v.mask & NV_M_NO_XL);
    const uint64_t status = (uint64_t)((f ^ v.flags) & (ESC_NF_UNSCHED | ESC_NF_TAINTED)) | (uint64_t)(cpu ^ v.cpu) |
                            (uint64_t)(mem ^ v.mem);
    const uint64_t facts = (uint64_t)(taint_s ^ v.taint_s) | (uint64_t)((no_del != 0) != (v.no_delete != 0)) |
                           (uint64_t)(v.mask & NV_M_FACTS);
    const uint64_t insts = (uint64_t)(inst ^ v.inst);
    if (!shape)
        for (uint32_t k = 0; k < nx; ++k) shape |= (uint64_t)((uint32_t)rd(NV_XL, (int64_t)v.xl_dev + k) ^ xl[k]);
    return (shape ? ESC_NV_SHAPE : 0u) | (status ? ESC_NV_STATUS : 0u) | (facts ? ESC_NV_FACTS : 0u) |
           (insts ? ESC_NV_INST : 0u);
}

}  // namespace esc
