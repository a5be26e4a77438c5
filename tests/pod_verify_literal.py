"""A pod's STORED FORM, restated from the layout text of include/escalator_hip.h / DESIGN.md §3 and
escalator_amd/layout.py (class_ids, folded_request): the class id of the pod plus the canonical
words a slot of that class keeps of it.  tests/test_gpu_pods_verify.py derives every expected
esc_pods_verify status from it; it never calls the library.

A pod here is a dict ``{"f": flags, "cpu0", "mem0", "pair0", "xc": [(cpu, mem), ...], "xp": [pair, ...]}``
with the records in the packed order (regular, init, overhead) and the counts in the flags.

  packed small / inert class   the folded request, pair0 (none when the pod is a daemonset pod or
                               the id does not fit 14 bits below the sentinel), the daemonset bit,
                               ONE blocks-default bit (daemonset, static, has-selector, affinity),
                               the extra pairs (none for a daemonset pod or an id of 0xFFFF and up)
  packed class                 the pod's four own bits, pair0, the folded request, the extra pairs
  plain class                  the flags, cpu0, mem0, pair0, every record, the extra pairs
  C slot of room R             the room's counts with the pod's four own bits, cpu0, mem0, pair0,
                               the records first of each kind in the room and the rest neutral (0;
                               INT64_MIN for init keys), the pairs, then ESC_NONE
"""
import numpy as np

from escalator_amd import layout

NONE = 0xFFFFFFFF
INT64_MIN = -(1 << 63)
ABSENT, CLASS, VALUE, BIND = 1, 2, 4, 8
OWN = 0xF                                            # daemonset, static, has-selector, affinity
SPARE_ROOM = (4, 2, 1, 6)                            # a spare C slot: regular, init, overhead, pairs


def flags(own=0, reg=0, init=0, ovh=0, pairs=0):
    return own | (ovh << 4) | (reg << 8) | (init << 16) | (pairs << 24)


def counts(f):
    return (f >> 8) & 0xFF, (f >> 16) & 0xFF, (f >> 4) & 1, (f >> 24) & 0x3F


def pod(cpu0=100, mem0=1 << 20, pair0=NONE, own=0, reg=(), init=(), ovh=None, xp=()):
    xc = list(reg) + list(init) + ([ovh] if ovh else [])
    return {"f": flags(own, len(reg), len(init), 1 if ovh else 0, len(xp)), "cpu0": cpu0, "mem0": mem0, "pair0": pair0,
            "xc": xc, "xp": list(xp)}


def soa(pods):
    """The packed SoA (what Context.pods_upsert / pods_verify take) of a list of pods."""
    return {"flags": np.array([p["f"] for p in pods], np.uint32), "cpu0": np.array([p["cpu0"] for p in pods], np.uint32),
            "mem0": np.array([p["mem0"] for p in pods], np.int64), "pair0": np.array([p["pair0"] for p in pods], np.uint32),
            "xc_cpu": np.array([c for p in pods for c, _ in p["xc"]], np.int64),
            "xc_mem": np.array([m for p in pods for _, m in p["xc"]], np.int64),
            "xp_pair": np.array([q for p in pods for q in p["xp"]], np.uint32)}


def class_ids(pods, n_gp):
    return [int(x) for x in layout.class_ids(soa(pods), n_gp)] if pods else []


def room_of(p):
    """The room a C pod's slot has when the load gave it one: its own counts."""
    return counts(p["f"])


def fits_room(room, p):
    r, i, v, q = counts(p["f"])
    return r <= room[0] and i <= room[1] and v <= room[2] and q <= room[3]


def stored_k(p, cid):
    """The words a slot of class `cid` keeps of pod p (cid its own class id)."""
    own = p["f"] & OWN
    if cid >= 128:
        cpu, mem = (int(x[0]) for x in layout.folded_request(soa([p])))
        if cid >= 256:
            ds = own & 1
            pair0 = NONE if ds or p["pair0"] >= (1 << 14) - 1 else p["pair0"]
            xp = [NONE if ds or q >= 0xFFFF else q for q in p["xp"]]
            return ("small", cpu, mem, pair0, ds, 1 if own else 0, tuple(xp))
        return ("packed", own, p["pair0"], cpu, mem, tuple(p["xp"]))
    return ("plain", p["f"], p["cpu0"], p["mem0"], p["pair0"], tuple(p["xc"]), tuple(p["xp"]))


def stored_c(p, room):
    reg, init, ovh, np_ = counts(p["f"])
    xc = p["xc"]
    recs = list(xc[:reg]) + [(0, 0)] * (room[0] - reg)
    recs += list(xc[reg:reg + init]) + [(INT64_MIN, INT64_MIN)] * (room[1] - init)
    recs += (list(xc[reg + init:]) if ovh else [(0, 0)]) if room[2] else []
    return ("c", p["f"] & OWN, p["cpu0"], p["mem0"], p["pair0"], tuple(recs), tuple(p["xp"]) + (NONE,) * (room[3] - np_))


def expect(resident, offered, n_gp, where):
    """esc_pods_verify's status (without BIND) of every offered pod.  resident[i]: the pod the
    device holds under that id (None: absent); where[i]: None for a K-resident pod, else the room
    (regular, init, overhead, pairs) of the C slot it lies in."""
    rc = class_ids([r for r in resident if r is not None], n_gp)
    oc = class_ids(offered, n_gp)
    out, k = [], 0
    for r, o, c, w in zip(resident, offered, oc, where):
        if r is None:
            out.append(ABSENT)
            continue
        cid = rc[k]
        k += 1
        if w is None:
            assert cid >= 0, "a C pod needs its slot's room"
            out.append(CLASS if c != cid else (VALUE if stored_k(o, cid) != stored_k(r, cid) else 0))
        else:
            out.append(CLASS if not fits_room(w, o) else (VALUE if stored_c(o, w) != stored_c(r, w) else 0))
    return np.array(out, np.uint8)
