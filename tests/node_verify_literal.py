"""What esc_nodes_verify must answer, restated in numpy without calling the library.

``Mirror`` holds, per node-table slot, the packed words last sent to the device: a test calls the
method of the same name beside every load and node event it makes (``load``, ``add``, ``delete``,
``relabel``, ``update``, ``facts``, ``instantiated``, ``compact``), each restating what the header
says that call writes.  ``expect`` then compares a batch, packed as the caller's store holds it,
with those words by the header's rule and returns the status bytes; ``report`` derives the report
from status bytes."""
import numpy as np

ABSENT, SHAPE, STATUS, FACTS, INST = 1, 2, 4, 8, 16
UNSCHED, TAINTED, TRACKED = 1, 2, 4
I64_MIN = -(1 << 63)


def split(N):
    """The packed nodes of a batch one by one: (flags, label0, cpu, mem, created, [extra labels])."""
    out, at = [], 0
    for i in range(len(N["flags"])):
        f = int(N["flags"][i])
        nx = (f >> 8) & 0xFF
        out.append((f, int(N["label0"][i]), int(N["cpu"][i]), int(N["mem"][i]), int(N["created_ns"][i]),
                    [int(x) for x in N["xl_pair"][at:at + nx]]))
        at += nx
    assert at == len(N["xl_pair"])
    return out


class Mirror:
    def __init__(self):
        self.slot = {}                       # index -> dict(f, label0, cpu, mem, created, xl, taint, nodel, inst)
        self.n = 0                           # slots used so far (a deleted slot is not reused)

    def load(self, N):
        self.slot, self.n = {}, 0
        self.add(N)

    def add(self, N):
        ids = []
        for f, l0, cpu, mem, created, xl in split(N):
            self.slot[self.n] = {"f": f, "label0": l0, "cpu": cpu, "mem": mem, "created": created, "xl": xl,
                                 "taint": I64_MIN, "nodel": 0, "inst": I64_MIN}
            ids.append(self.n)
            self.n += 1
        return ids

    def placement(self, taint_s, no_delete):
        for j in range(self.n):
            if j in self.slot:
                self.slot[j]["taint"], self.slot[j]["nodel"] = int(taint_s[j]), int(no_delete[j])

    def delete(self, ids):
        for j in ids:
            del self.slot[int(j)]

    def relabel(self, ids, N):
        for j, (f, l0, cpu, mem, created, xl) in zip(ids, split(N)):
            self.slot[int(j)].update(f=f, label0=l0, cpu=cpu, mem=mem, created=created, xl=xl)

    def update(self, ids, flags, cpu, mem):
        for j, f, c, m in zip(ids, flags, cpu, mem):
            s = self.slot[int(j)]
            s.update(f=(s["f"] & ~(UNSCHED | TAINTED)) | (int(f) & (UNSCHED | TAINTED)), cpu=int(c), mem=int(m))

    def facts(self, ids, taint_s, no_delete):
        for j, t, d in zip(ids, taint_s, no_delete):
            self.slot[int(j)].update(taint=int(t), nodel=int(d))

    def instantiated(self, ids, inst_ns):
        for j, t in zip(ids, inst_ns):
            self.slot[int(j)]["inst"] = int(t)

    def compact(self, new_index):
        live = sorted(self.slot)
        assert [int(new_index[j]) for j in live] == list(range(len(live)))
        assert all(int(new_index[j]) == -1 for j in range(self.n) if j not in self.slot)
        self.slot = {k: self.slot[j] for k, j in enumerate(live)}
        self.n = len(live)

    def live_ids(self):
        return sorted(self.slot)

    def expect(self, ids, N, taint_s=None, no_delete=None, inst_ns=None):
        out = np.zeros(len(ids), np.uint8)
        for i, (j, (f, l0, cpu, mem, created, xl)) in enumerate(zip(ids, split(N))):
            s = self.slot.get(int(j))
            if s is None:
                out[i] = ABSENT
                continue
            st = 0
            if l0 != s["label0"] or xl != s["xl"] or created != s["created"]:
                st |= SHAPE
            if (f ^ s["f"]) & (UNSCHED | TAINTED) or cpu != s["cpu"] or mem != s["mem"]:
                st |= STATUS
            if (taint_s is not None and int(taint_s[i]) != s["taint"]) or \
                    (no_delete is not None and (int(no_delete[i]) != 0) != (s["nodel"] != 0)):
                st |= FACTS
            if inst_ns is not None and int(inst_ns[i]) != s["inst"]:
                st |= INST
            out[i] = st
        return out


def report(status):
    bad = np.flatnonzero(status)
    return {"n_checked": len(status), "n_absent": int(np.count_nonzero(status & ABSENT)),
            "n_shape": int(np.count_nonzero(status & SHAPE)), "n_status": int(np.count_nonzero(status & STATUS)),
            "n_facts": int(np.count_nonzero(status & FACTS)), "n_inst": int(np.count_nonzero(status & INST)),
            "first_bad": int(bad[0]) if len(bad) else -1}
